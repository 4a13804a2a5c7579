// antsrl_popfitness.hip — k_pop_fitness: every member's episode reward off the monitor's block (include/antsrl.h,
// "Population-based training"; the entry antsrl_pop_fitness is in antsrl_popapi.hip).
//
// One workgroup of MON_THREADS = 256 per member, grid P.  Member p owns environments [p Em, (p + 1) Em).  The workgroup
// takes them one after the other: an environment's total is the monitor's total[e] (monitor_row_total: slot t adds ants
// t, t + 256, ... ascending, the slots folded with s = 128 ... 1), which lane e % 256 takes into its member slot (slot t
// holds environments t, t + 256, ... ascending); the member's slots are folded the same way at the end, with the min and
// the max of the environments' totals.  episode_reward is read only; row[p] has one writer.  No atomics, float64 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_monitor_dev.h"
#include "antsrl_population.h"

__global__ void __launch_bounds__(MON_THREADS) k_pop_fitness(const double *__restrict__ er, int Em, int N, double *__restrict__ row)
{
    __shared__ double xs[MON_THREADS], xmn[MON_THREADS], xmx[MON_THREADS];
    const int p = (int)blockIdx.x, t = (int)threadIdx.x;
    const double *mine = er + (size_t)p * (size_t)Em * (size_t)N;
    double sum = 0.0, mn = 0.0, mx = 0.0;
    for (int e = 0; e < Em; ++e) { // (uniform per workgroup)
        const double total = monitor_row_total(mine + (size_t)e * (size_t)N, N, xs, t);
        if ((e & (MON_THREADS - 1)) == t) monitor_slot_take(total, e == t, sum, mn, mx);
        __syncthreads(); // xs[0] is read before the next environment's slots are written
    }
    xs[t] = sum; xmn[t] = mn; xmx[t] = mx;
    monitor_fold3(xs, xmn, xmx, t, Em);
    if (t == 0) {
        double *r = row + (size_t)p * 3;
        r[0] = xs[0]; r[1] = xmn[0]; r[2] = xmx[0];
    }
}

hipError_t antsrl_launch_pop_fitness(const double *episode_reward, int Em, int N, int P, double *row, hipStream_t st)
{
    hipLaunchKernelGGL(k_pop_fitness, dim3((unsigned)P), dim3(MON_THREADS), 0, st, episode_reward, Em, N, row);
    return hipGetLastError();
}
