// antsrl_monitor.hip — the training monitor (include/antsrl.h, "The training monitor"; antsrl_monitor.h holds the block's
// layout and the order of the sums): the kernels and, in front of them, the C-ABI entries antsrl_monitor_sizes / _init /
// _step / _end_episode.
//
//   k_monitor_accum        a step that does not report: episode_reward += (double)reward, one element per lane, no reduction
//   k_monitor_report       a step that reports: one workgroup of 256 per environment accumulates its row and reduces it
//                          in the same pass ({total, min, max} in the order of sums)
//   k_monitor_end_episode  the episode's row (workgroup 0 folds the totals of the episode's last report), episode_reward = 0
// Thread 0 of workgroup 0 of a step's kernel keeps the running loss.  No atomics; every word has one writer per launch.
//
// The entries validate every argument before any HIP call and enqueue on the caller's stream: no handle, no allocation,
// no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_device.h"
#include "antsrl_fail.h"
#include "antsrl_monitor.h"
#include "antsrl_monitor_dev.h" // the slots and their folds, shared with antsrl_popfitness.hip

struct MonitorStep {
    double *er;          // episode_reward [E][N]
    const float *reward; // [E][N]
    double *head;        // avg_loss, n_losses, last_loss
    double *report;      // reports[report_slot] ([E][3]) on a reporting step
    MonitorLoss loss;
    int N, M;            // ants per environment, E * N
};

// main.py:106-109 in float64: the first loss is the average, later ones 0.99 * avg + 0.01 * loss, each product rounded before
// the add (the build's -ffp-contract=off)
__device__ __forceinline__ void monitor_loss(double *head, const MonitorLoss &loss)
{
    if (!loss.has) return;
    const double l = loss.dev ? (double)*loss.dev : loss.host;
    int64_t *n_losses = reinterpret_cast<int64_t *>(head + 1);
    const int64_t n = *n_losses;
    head[0] = n == 0 ? l : 0.99 * head[0] + 0.01 * l;
    *n_losses = n + 1;
    head[2] = l;
}

__global__ void __launch_bounds__(MON_THREADS) k_monitor_accum(MonitorStep a)
{
    const int i = (int)(blockIdx.x * MON_THREADS + threadIdx.x); // M < 2^31 and the grid covers M rounded up to 256
    if (i < a.M) a.er[i] = a.er[i] + (double)a.reward[i];
    if (i == 0) monitor_loss(a.head, a.loss);
}

__global__ void __launch_bounds__(MON_THREADS) k_monitor_report(MonitorStep a)
{
    __shared__ double xs[MON_THREADS], xmn[MON_THREADS], xmx[MON_THREADS];
    const int e = (int)blockIdx.x, t = (int)threadIdx.x, N = a.N;
    double *er = a.er + (size_t)e * N;
    const float *rw = a.reward + (size_t)e * N;
    double sum = 0.0, mn = 0.0, mx = 0.0;
    for (int n = t; n < N; n += MON_THREADS) {
        const double v = er[n] + (double)rw[n];
        er[n] = v;
        monitor_slot_take(v, n == t, sum, mn, mx);
    }
    xs[t] = sum; xmn[t] = mn; xmx[t] = mx;
    monitor_fold3(xs, xmn, xmx, t, N); // slots t >= N hold no ant
    if (t == 0) {
        double *r = a.report + (size_t)e * 3;
        r[0] = xs[0]; r[1] = xmn[0]; r[2] = xmx[0];
        if (e == 0) monitor_loss(a.head, a.loss);
    }
}

// last_report: reports[last_report_slot] ([E][3]) or NULL (the episode had no report: grand_total = 0)
__global__ void __launch_bounds__(MON_THREADS) k_monitor_end_episode(double *er, int M, const double *head,
                                                                      const double *last_report, int E, double *row)
{
    __shared__ double xs[MON_THREADS];
    const int t = (int)threadIdx.x;
    if (blockIdx.x == 0) { // (reads nothing this launch writes)
        double sum = 0.0;
        if (last_report)
            for (int e = t; e < E; e += MON_THREADS) sum = sum + last_report[(size_t)e * 3];
        xs[t] = sum;
        monitor_fold(xs, t);
        if (t == 0) {
            row[0] = xs[0];
            row[1] = head[0];
            row[2] = (double)*reinterpret_cast<const int64_t *>(head + 1);
        }
    }
    const int i = (int)(blockIdx.x * MON_THREADS) + t;
    if (i < M) er[i] = 0.0;
}

hipError_t antsrl_launch_monitor_step(double *state, const MonitorLayout &L, const float *reward, const MonitorLoss &loss,
                                      int report_slot, hipStream_t st)
{
    MonitorStep a;
    a.er = state; a.reward = reward; a.head = state + L.avg_loss; a.loss = loss;
    a.N = L.N; a.M = L.E * L.N;
    a.report = report_slot >= 0 ? state + L.reports + (size_t)report_slot * (size_t)L.E * 3 : nullptr;
    if (report_slot >= 0)
        hipLaunchKernelGGL(k_monitor_report, dim3((unsigned)L.E), dim3(MON_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(k_monitor_accum, dim3((unsigned)((a.M + MON_THREADS - 1) / MON_THREADS)), dim3(MON_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t antsrl_launch_monitor_end_episode(double *state, const MonitorLayout &L, int episode_slot, int last_report_slot,
                                             hipStream_t st)
{
    const int M = L.E * L.N;
    const double *last = last_report_slot >= 0 ? state + L.reports + (size_t)last_report_slot * (size_t)L.E * 3 : nullptr;
    hipLaunchKernelGGL(k_monitor_end_episode, dim3((unsigned)((M + MON_THREADS - 1) / MON_THREADS)), dim3(MON_THREADS), 0, st,
                       state, M, state + L.avg_loss, last, L.E, state + L.episodes + (size_t)episode_slot * 3);
    return hipGetLastError();
}

// ---- the C-ABI ---------------------------------------------------------------------------------------------------------

static int monitor_check(const char *who, int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes,
                         MonitorLayout *L)
{
    if (n_envs < 1 || n_ants < 1) return fail(ANTSRL_E_INVALID, "%s: n_envs and n_ants must be >= 1 (%d, %d)", who, n_envs, n_ants);
    if ((long long)n_envs * n_ants > 0x7fffffffLL - MON_THREADS)
        return fail(ANTSRL_E_INVALID, "%s: n_envs * n_ants must be below 2^31 - 256", who);
    if (max_reports < 1 || max_episodes < 1)
        return fail(ANTSRL_E_INVALID, "%s: max_reports and max_episodes must be >= 1 (%d, %d)", who, max_reports, max_episodes);
    *L = antsrl_monitor_layout(n_envs, n_ants, max_reports, max_episodes);
    return ANTSRL_OK;
}

static int monitor_state(const char *who, const void *state)
{
    if (!state) return fail(ANTSRL_E_INVALID, "%s: NULL state", who);
    if ((uintptr_t)state & 7) return fail(ANTSRL_E_INVALID, "%s: state must be 8-byte aligned", who);
    return ANTSRL_OK;
}

extern "C" int antsrl_monitor_sizes(int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes, size_t *bytes)
{
    const char *who = "monitor_sizes";
    MonitorLayout L;
    const int rc = monitor_check(who, n_envs, n_ants, max_reports, max_episodes, &L);
    if (rc != ANTSRL_OK) return rc;
    if (!bytes) return fail(ANTSRL_E_INVALID, "%s: NULL bytes", who);
    *bytes = L.words * 8;
    return ANTSRL_OK;
}

extern "C" int antsrl_monitor_init(void *state, int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes,
                                   void *stream)
{
    const char *who = "monitor_init";
    MonitorLayout L;
    int rc = monitor_check(who, n_envs, n_ants, max_reports, max_episodes, &L);
    if (rc == ANTSRL_OK) rc = monitor_state(who, state);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(hipMemsetAsync(state, 0, L.words * 8, (hipStream_t)stream), who); // +0.0 and 0 everywhere
}

extern "C" int antsrl_monitor_step(void *state, int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes,
                                   const float *reward, const float *loss_dev, double loss_host, int has_loss,
                                   int report_slot, void *stream)
{
    const char *who = "monitor_step";
    MonitorLayout L;
    int rc = monitor_check(who, n_envs, n_ants, max_reports, max_episodes, &L);
    if (rc == ANTSRL_OK) rc = monitor_state(who, state);
    if (rc != ANTSRL_OK) return rc;
    if (!reward) return fail(ANTSRL_E_INVALID, "%s: NULL reward", who);
    if (((uintptr_t)reward | (uintptr_t)loss_dev) & 3) return fail(ANTSRL_E_INVALID, "%s: reward and loss_dev must be 4-byte aligned", who);
    if (report_slot < -1 || report_slot >= max_reports)
        return fail(ANTSRL_E_INVALID, "%s: report_slot %d is not -1 (no report) or in [0, max_reports = %d)", who, report_slot, max_reports);
    MonitorLoss loss = {loss_dev, loss_host, has_loss != 0};
    return enqueued(antsrl_launch_monitor_step((double *)state, L, reward, loss, report_slot, (hipStream_t)stream), who);
}

extern "C" int antsrl_monitor_end_episode(void *state, int32_t n_envs, int32_t n_ants, int32_t max_reports,
                                          int32_t max_episodes, int episode_slot, int last_report_slot, void *stream)
{
    const char *who = "monitor_end_episode";
    MonitorLayout L;
    int rc = monitor_check(who, n_envs, n_ants, max_reports, max_episodes, &L);
    if (rc == ANTSRL_OK) rc = monitor_state(who, state);
    if (rc != ANTSRL_OK) return rc;
    if (episode_slot < 0 || episode_slot >= max_episodes)
        return fail(ANTSRL_E_INVALID, "%s: episode_slot %d is not in [0, max_episodes = %d)", who, episode_slot, max_episodes);
    if (last_report_slot < -1 || last_report_slot >= max_reports)
        return fail(ANTSRL_E_INVALID, "%s: last_report_slot %d is not -1 (no report) or in [0, max_reports = %d)", who,
                    last_report_slot, max_reports);
    return enqueued(antsrl_launch_monitor_end_episode((double *)state, L, episode_slot, last_report_slot, (hipStream_t)stream), who);
}
