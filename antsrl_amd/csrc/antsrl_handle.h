// antsrl_handle.h — the environment's handle (AntsHandle of include/antsrl.h) and what an API file other than
// antsrl_capi.hip, where both helpers are defined, needs of it.  A fresh handle is all zero but for the initialisers below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_device.h"
#include "antsrl_fail.h"

struct AntsHandle {
    AntsCfg cfg;
    KP p;
    int cur;               // pheromone buffer holding the current grid
    int steps_since_update;// RLApi.step calls since the last Environment.update
    bool need_full_collect = true; // next update must run Anthill.update over the whole grid
    bool is_reset;
    bool episode_over;     // a refused auto-reset left a finished episode behind (see antsrl_step_update)
    size_t ws_bytes[2];    // the state block and the record block (one block: [0] is all of it, [1] = 0)
    AntsGen gen;           // device generator parameters (antsrl_generate)
    bool has_gen;
    uint64_t episode_seed; // seed of the current episode
    int host_timestep = 1; // mirrors Environment.timestep (all envs step in lockstep)
    long long sweeps;      // scaled mode: updates since the units were last re-based
    bool obs_bf16;         // observation buffers are bfloat16 (antsrl_set_obs_format)
    uint32_t obs_pitch;    // elements between two ants' observation rows (antsrl_set_obs_row_stride), 0 = dense
    bool prc_generic;      // k_perceive's generic kernel is pinned (antsrl_set_perceive_path)
    bool prc_noskip;       // the fast kernel ignores the explored summary, none is kept (ANTSRL_PERCEIVE_FAST_NOSKIP)
    uint32_t sum_obs;      // observations since the last reset: the explored summary's refresh cadence (summary_cadence)
    bool sum_due;          // a refresh of the summary is due behind the observation just enqueued (summary_refresh_due)
    bool sum_live;         // a refresh has been enqueued since the last reset: k_perceive consumes the summary (ACT_SUMMARY)
    bool need_wall_clear;  // scaled mode: initial grid may hold pheromone on wall cells
    hipEvent_t ev[ANTSRL_TIMING_EVENTS]; // measurement hook (antsrl_set_timing_events)
    bool ev_armed;
    uint32_t obs_seq;      // cell-meta path: observations since the explored stamps were last re-based
    PolArgs pol;           // in-loop policy (antsrl_set_inloop_policy); pol.pack == NULL: none
    // Deferred update (include/antsrl.h): Environment.update was requested, its host-side bookkeeping is done, its
    // kernel has NOT been enqueued yet — the next antsrl_step runs it fused with the move (k_update_move); every other
    // entry point that touches the state enqueues it first (flush_pending).
    bool pend_update;
    KP pend_p;             // kernel parameters as they stood at the update's call (g_dep / inv_g_dep differ afterwards)
    int pend_out_buf;
    int phase_next;        // antsrl_update_phase: the next phase of an Environment.update in progress (0: none in progress)
};

// Enqueues a deferred update on its own (k_update_one), e.g. ahead of a state read.
ANTSRL_INTERNAL int flush_pending(AntsHandle *h, hipStream_t st);

// What an entry asks of its (non-NULL) handle before it touches the state: a handle without an episode is refused, and
// one between two phases of antsrl_update_phase as well — unless the entry only reads, which is what the phases are for.
enum MidUpdate { MID_UPDATE_REFUSED, MID_UPDATE_ALLOWED };
ANTSRL_INTERNAL int handle_ready(const AntsHandle *h, MidUpdate mid);
