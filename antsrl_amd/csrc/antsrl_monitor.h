// antsrl_monitor.h — the training monitor on the device (antsrl_monitor.hip): what main.py keeps around its step
// (episode_reward :89/:100, avg_loss :59/:106-109, mean_reward / total_reward :115-120, all_loss / all_reward :151-152) as
// one caller-allocated device block and one launch per step.  include/antsrl.h, "The training monitor", is the
// specification; this header holds the block's layout and THE ORDER OF THE SUMS the kernels keep.
//
// The block, in float64 / int64 words of 8 bytes, dense, in this order (MonitorLayout):
//     episode_reward  double [E][N]
//     avg_loss        double            the running loss (main.py:106-109)
//     n_losses        int64             losses seen; 0 = main.py's None
//     last_loss       double            the last loss seen
//     reports         double [max_reports][E][3]     {total, min, max} of episode_reward[e][:]
//     episodes        double [max_episodes][3]       {grand_total, avg_loss, n_losses}
//
// The order of the sums (MON_THREADS = 256 slots; every add a float64 add, round to nearest even):
//     total[e]:     slot t starts at +0.0 and adds episode_reward[e][n] for n = t, t + 256, t + 512, ... ascending; the 256
//                   slots are folded with x[i] += x[i + s] for i < s, s = 128, 64, ..., 1; total = x[0].
//     grand_total:  the same rule over the environments' totals of one report: slot t takes e = t, t + 256, ...
//     min / max:    order-free; slot t (< N) starts from its first ant, a slot without an ant takes no part.
// A step that does not report reduces nothing: it is the element-wise accumulate alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_fail.h"

#define MON_THREADS 256 // one workgroup of the report pass: the slots of the order of sums (four waves)

struct MonitorLayout {
    int E, N, max_reports, max_episodes;
    size_t avg_loss, n_losses, last_loss, reports, episodes, words; // offsets and the total, in 8-byte words
};

static inline MonitorLayout antsrl_monitor_layout(int E, int N, int max_reports, int max_episodes)
{
    MonitorLayout L;
    L.E = E; L.N = N; L.max_reports = max_reports; L.max_episodes = max_episodes;
    L.avg_loss = (size_t)E * (size_t)N;
    L.n_losses = L.avg_loss + 1;
    L.last_loss = L.avg_loss + 2;
    L.reports = L.avg_loss + 3;
    L.episodes = L.reports + (size_t)max_reports * (size_t)E * 3;
    L.words = L.episodes + (size_t)max_episodes * 3;
    return L;
}

struct MonitorLoss {
    const float *dev; // the loss on the device, or NULL: then `host`
    double host;
    int has;          // 0: this step has no loss
};

// one launch each
ANTSRL_INTERNAL hipError_t antsrl_launch_monitor_step(double *state, const MonitorLayout &L, const float *reward,
                                                      const MonitorLoss &loss, int report_slot, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_monitor_end_episode(double *state, const MonitorLayout &L, int episode_slot,
                                                             int last_report_slot, hipStream_t st);
