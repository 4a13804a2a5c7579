// antsrl_stats.hip — the colony statistics' kernels (include/antsrl.h, "The colony statistics"; antsrl_stats.h holds the
// block's layout and the order of the sums).  What a training run reports of the task itself — food at the anthill, on the
// map and in the mandibles, explored cells, pheromone on the map — as one row of 7 + 2 C words per environment, reduced
// on the device in two launches, nothing read back.  The C-ABI entries are in antsrl_logapi.hip.
//
//   k_stats_cells   one workgroup of 256 per (segment of 4096 canonical cells, environment): every cell's values once
//                   (antsrl_cellread.h: one 16-byte load per cell on the interleaved records), the segment's partials
//                   into the scratch
//   k_stats_fold    one workgroup of 256 per environment: the partials' planes and the ants' holding folded into the row,
//                   timestep and anthill_food copied
// No atomics; every word has one writer per launch; k_stats_fold reads what k_stats_cells wrote (stream order).
#include "antsrl_util.h"
#include "antsrl_cellread.h"
#include "antsrl_stats.h"

struct StatsArgs {
    StatsLayout L;
    double *row, *scratch;
    int cur;
};

// x[i] += x[i + s] for i < s, s = 128, ..., 1, over the workgroup's 256 slots; the result in x[0]
template <typename T>
__device__ __forceinline__ void stats_fold(T *x, const int t)
{
    __syncthreads();
    for (int s = STATS_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) x[t] = x[t] + x[t + s];
        __syncthreads();
    }
}

template <bool INTER>
__global__ void __launch_bounds__(STATS_THREADS) k_stats_cells(const KP p, const StatsArgs a)
{
    __shared__ double xs[1 + ANTSRL_MAX_PHERO][STATS_THREADS];
    __shared__ int32_t xn[2 + ANTSRL_MAX_PHERO][STATS_THREADS]; // a slot counts at most 16 cells, a segment 4096
    const StatsLayout &L = a.L;
    const int t = (int)threadIdx.x;
    const size_t seg = blockIdx.x, e = blockIdx.y;
    const bool expl = L.has_expl != 0;
    double food = 0.0, ph[ANTSRL_MAX_PHERO] = {0.0, 0.0, 0.0, 0.0};
    int32_t n_food = 0, n_expl = 0, n_ph[ANTSRL_MAX_PHERO] = {0, 0, 0, 0};
    const size_t g0 = seg * STATS_SEG + (size_t)t;
    auto take = [&](const CellAll &v) {
        food = food + (double)v.food;
        n_food += v.food > 0.0f;
        n_expl += v.explored;
#pragma unroll
        for (int c = 0; c < ANTSRL_MAX_PHERO; ++c) {
            ph[c] = ph[c] + (double)v.ph[c];
            n_ph[c] += v.ph[c] > 0.0f;
        }
    };
    if (INTER && (seg + 1) * STATS_SEG <= L.G) {
        // a whole segment of 16-byte records: eight loads in flight per lane, then their values in ascending order
        constexpr int B = 8;
        for (int k0 = 0; k0 < STATS_SEG / STATS_THREADS; k0 += B) {
            float4 r[B];
#pragma unroll
            for (int k = 0; k < B; ++k) r[k] = cell_record(p, a.cur, e, L.G, (uint32_t)(g0 + (size_t)(k0 + k) * STATS_THREADS));
#pragma unroll
            for (int k = 0; k < B; ++k) take(cell_all_of(p, r[k], e, (uint32_t)(g0 + (size_t)(k0 + k) * STATS_THREADS), expl));
        }
    } else {
        for (size_t g = g0; g < L.G; g += STATS_THREADS) take(cell_all<INTER>(p, a.cur, e, L.G, (uint32_t)g, expl));
    }
    xs[0][t] = food; xn[0][t] = n_food; xn[1][t] = n_expl;
#pragma unroll
    for (int c = 0; c < ANTSRL_MAX_PHERO; ++c) { xs[1 + c][t] = ph[c]; xn[2 + c][t] = n_ph[c]; }
    __syncthreads();
    for (int s = STATS_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            xs[0][t] = xs[0][t] + xs[0][t + s];
            xn[0][t] += xn[0][t + s]; xn[1][t] += xn[1][t + s];
            for (int c = 0; c < L.C; ++c) {
                xs[1 + c][t] = xs[1 + c][t] + xs[1 + c][t + s];
                xn[2 + c][t] += xn[2 + c][t + s];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        double *d = a.scratch + e * (size_t)L.P * L.nseg + seg; // plane q of this environment at d + q * nseg
        int64_t *n = reinterpret_cast<int64_t *>(d);
        d[STATS_P_FOOD_LEFT * L.nseg] = xs[0][0];
        n[STATS_P_FOOD_CELLS * L.nseg] = xn[0][0];
        n[STATS_P_EXPLORED_CELLS * L.nseg] = xn[1][0];
        for (int c = 0; c < L.C; ++c) {
            d[(size_t)(STATS_P_PHERO + 2 * c) * L.nseg] = xs[1 + c][0];
            n[(size_t)(STATS_P_PHERO + 2 * c + 1) * L.nseg] = xn[2 + c][0];
        }
    }
}

__global__ void __launch_bounds__(STATS_THREADS) k_stats_fold(const KP p, const StatsArgs a)
{
    __shared__ double xs[STATS_THREADS];
    __shared__ int64_t xn[STATS_THREADS];
    const StatsLayout &L = a.L;
    const int t = (int)threadIdx.x;
    const size_t e = blockIdx.x;
    double *row = a.row + e * (size_t)L.Q;
    int64_t *rown = reinterpret_cast<int64_t *>(row);
    // ---- the planes of partials: plane q -> word w (a double plane when `real`)
    for (int q = 0; q < L.P; ++q) {
        const bool real = q == STATS_P_FOOD_LEFT || (q >= STATS_P_PHERO && ((q - STATS_P_PHERO) & 1) == 0);
        const int w = q == STATS_P_FOOD_LEFT ? STATS_W_FOOD_LEFT : q == STATS_P_FOOD_CELLS ? STATS_W_FOOD_CELLS
                    : q == STATS_P_EXPLORED_CELLS ? STATS_W_EXPLORED_CELLS : STATS_W_PHERO + (q - STATS_P_PHERO);
        const double *d = a.scratch + (e * (size_t)L.P + (size_t)q) * L.nseg;
        if (real) {
            double sum = 0.0;
            for (size_t s = (size_t)t; s < L.nseg; s += STATS_THREADS) sum = sum + d[s];
            __syncthreads(); // (the previous plane's x[0] has been read)
            xs[t] = sum;
            stats_fold(xs, t);
            if (t == 0) row[w] = xs[0];
        } else {
            const int64_t *n = reinterpret_cast<const int64_t *>(d);
            int64_t sum = 0;
            for (size_t s = (size_t)t; s < L.nseg; s += STATS_THREADS) sum += n[s];
            __syncthreads();
            xn[t] = sum;
            stats_fold(xn, t);
            if (t == 0) rown[w] = (q == STATS_P_EXPLORED_CELLS && !L.has_expl) ? (int64_t)-1 : xn[0];
        }
    }
    // ---- the ants: food_carried, n_carrying (k_monitor_report's order: slot t takes the ants t, t + 256, ...)
    const float *hold = p.s.holding + e * (size_t)p.N;
    double sum = 0.0;
    int64_t cnt = 0;
    for (int n = t; n < p.N; n += STATS_THREADS) {
        const float h = hold[n];
        sum = sum + (double)h;
        cnt += h > 0.0f;
    }
    __syncthreads();
    xs[t] = sum; xn[t] = cnt;
    stats_fold(xs, t);
    stats_fold(xn, t);
    if (t == 0) {
        row[STATS_W_FOOD_CARRIED] = xs[0];
        rown[STATS_W_N_CARRYING] = xn[0];
        rown[STATS_W_TIMESTEP] = (int64_t)p.s.timestep[e];
        row[STATS_W_ANTHILL_FOOD] = p.s.anthill_food[e];
    }
}

hipError_t antsrl_launch_stats_row(const KP &p, int cur, const StatsLayout &L, double *row, double *scratch, hipStream_t st)
{
    StatsArgs a = {L, row, scratch, cur};
    const dim3 grid((unsigned)L.nseg, (unsigned)L.E);
    if (p.ps == 4 && p.fs == 4)
        hipLaunchKernelGGL(k_stats_cells<true>, grid, dim3(STATS_THREADS), 0, st, p, a);
    else
        hipLaunchKernelGGL(k_stats_cells<false>, grid, dim3(STATS_THREADS), 0, st, p, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_stats_fold, dim3((unsigned)L.E), dim3(STATS_THREADS), 0, st, p, a);
    return hipGetLastError();
}
