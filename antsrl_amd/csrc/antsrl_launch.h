// antsrl_launch.h — the environment's launchers and predicates: defined beside their kernels, called by antsrl_capi.hip.
// Both sides include this header; the default arguments are here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_device.h"
#include "antsrl_fail.h"

// the steps of one Environment.update (update_env's `phases`, antsrl_update_env.h)
#define UPD_WALLS 1
#define UPD_ROCKS 2
#define UPD_ANTS 4
#define UPD_ANTHILL 8
#define UPD_ALL (UPD_WALLS | UPD_ROCKS | UPD_ANTS | UPD_ANTHILL)

// antsrl_act.hip
ANTSRL_INTERNAL hipError_t antsrl_launch_act(const KP &p, const int8_t *rot, const int8_t *ph, int cur, float *obs,
                                             float *agent_state, float *reward, uint8_t *done, int flags, hipStream_t st);
ANTSRL_INTERNAL bool antsrl_act_fits(const KP &p);
ANTSRL_INTERNAL bool antsrl_act_needs_hbm_maps(const KP &p);
// antsrl_sweep.hip
ANTSRL_INTERNAL hipError_t antsrl_launch_sweep(const KP &p, int cur, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_phero_wall_clear(const KP &p, hipStream_t st, int buf = 0);
ANTSRL_INTERNAL hipError_t antsrl_launch_phero_renorm(const KP &p, hipStream_t st);
// antsrl_update.hip
ANTSRL_INTERNAL hipError_t antsrl_launch_update(const KP &p, const double *jitter, int out_buf, hipStream_t st,
                                                int phases = UPD_ALL);
ANTSRL_INTERNAL hipError_t antsrl_launch_collect_full(const KP &p, hipStream_t st);
// antsrl_state.hip
ANTSRL_INTERNAL hipError_t antsrl_launch_reset(const KP &p, const AntsInit *in, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_generate(const KP &p, const AntsGen &g, uint64_t seed, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_set_activation(const KP &p, const float *act, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_read_state(const KP &p, int which, int cur, void *dst, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_perceptive_field(const KP &p, uint8_t *dst, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_obs_coords(const KP &p, int32_t *dst, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_give_reward(const KP &p, const double *reward, double threshold, float *reward_out,
                                                     hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_copy16(void *dst, const void *src, size_t bytes, hipStream_t st);
// antsrl_perceive.hip: the cell-meta path
ANTSRL_INTERNAL bool antsrl_meta_supported(const KP &p);
ANTSRL_INTERNAL int antsrl_perceive_run(const KP &p);
ANTSRL_INTERNAL hipError_t antsrl_launch_move(const KP &p, const int8_t *rot, const int8_t *ph, uint8_t *done, int do_step,
                                              uint32_t seq, hipStream_t st);
ANTSRL_INTERNAL bool antsrl_update_move_supported(const KP &p);
ANTSRL_INTERNAL hipError_t antsrl_launch_update_move(const KP &p, int out_buf, double g_dep, double inv_g_dep, const int8_t *rot,
                                                     const int8_t *ph, uint8_t *done, uint32_t seq, hipStream_t st,
                                                     bool with_frames);
ANTSRL_INTERNAL bool antsrl_inloop_policy_supported(const KP &p);
ANTSRL_INTERNAL bool antsrl_perceive_fast(const KP &p);
ANTSRL_INTERNAL hipError_t antsrl_launch_perceive(const KP &p, int cur, float *obs, float *agent_state, float *reward, int flags,
                                                  uint32_t seq, hipStream_t st, const PolArgs *pol, uint32_t obs_pitch,
                                                  bool generic);
ANTSRL_INTERNAL bool antsrl_explored_summary_supported(const KP &p, bool with_policy);
ANTSRL_INTERNAL hipError_t antsrl_launch_explored_summary(const KP &p, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_meta_rebase(const KP &p, hipStream_t st);
// antsrl_checkpoint.hip: k_env_copy over the table of antsrl_checkpoint.h (save, load, fork)
struct EnvCopyTable;
ANTSRL_INTERNAL hipError_t antsrl_launch_env_copy(const EnvCopyTable &t, hipStream_t st);
// antsrl_policy.hip
ANTSRL_INTERNAL hipError_t antsrl_launch_policy_pack(unsigned char *pack, const float *w1, const float *b1, const float *w2,
                                                     const float *b2, const float *w3, const float *b3, int F, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_policy(const float *obs, const float *agent_state, const float *w1, const float *b1,
                                                const float *w2, const float *b2, const float *w3, const float *b3, int8_t *rot,
                                                int8_t *ph, float *logits, int M, int F, hipStream_t st, bool obs_bf16);
