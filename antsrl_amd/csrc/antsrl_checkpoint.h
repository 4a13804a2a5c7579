// antsrl_checkpoint.h — what antsrl_checkpoint_save / _load / antsrl_fork_envs (antsrl_capi.hip) and their one kernel
// k_env_copy (antsrl_checkpoint.hip) share: the copy table the kernel is driven by, and the host blob's layout.
#pragma once
#include <stdint.h>
#include "../../include/antsrl.h"

// ---- the copy table (a kernel argument, passed by value) ---------------------------------------------------------------
// One entry per array of the carve.  A ROW of an array is `bytes` bytes: the whole array (save / load: one row per array,
// rows == 0) or one environment's slice of it (fork: `bytes` is the array's bytes per environment, row i goes from
// src + pair_src[i] * bytes to dst + pair_dst[i] * bytes).  A row is cut into chunks of ENV_COPY_CHUNK bytes, one
// workgroup pass each; `first_chunk` is the entry's first chunk in a row's numbering (a prefix sum, so a workgroup finds
// its array with a short scan of the table).
#define ENV_COPY_MAX_ARRAYS 40   // the carve has at most 33 arrays (antsrl_workspace_map)
#define ENV_COPY_MAX_PAIRS 640   // (src, dst) pairs of one launch: what fits the 4 KiB of kernel arguments beside the table
#define ENV_COPY_CHUNK 16384u    // 256 lanes x 4 x 16 bytes

struct EnvCopyArray {
    const unsigned char *src;
    unsigned char *dst;
    uint64_t bytes;       // of one row
    uint32_t first_chunk; // chunks of the arrays in front of this one, per row
    uint32_t _pad;
};

struct EnvCopyTable {
    EnvCopyArray a[ENV_COPY_MAX_ARRAYS];
    int32_t n_arrays;
    int32_t rows;            // 0: whole arrays (one row each, no pair is read); n >= 1: pairs [0, n)
    uint32_t chunks_per_row; // the sum of every array's chunks
    uint32_t _pad;
    uint16_t pair_src[ENV_COPY_MAX_PAIRS]; // (an environment index fits 16 bits: n_envs <= 65535)
    uint16_t pair_dst[ENV_COPY_MAX_PAIRS];
};

static inline uint32_t env_copy_chunks(uint64_t bytes) { return (uint32_t)((bytes + ENV_COPY_CHUNK - 1) / ENV_COPY_CHUNK); }

// ---- the host blob -----------------------------------------------------------------------------------------------------
// Every AntsHandle field an entry point changes after antsrl_create and that belongs to the episode (include/antsrl.h,
// "CHECKPOINT"); what belongs to the loading handle (the observation format and pitch, the perceive path, the in-loop
// policy, the timing events) is not in it.  Written over a zeroed struct: equal states give equal bytes.
#define ANTSRL_CKPT_MAGIC 0x4b435441u // "ATCK"
#define ANTSRL_CKPT_VERSION 1u

struct AntsCkptBlob {
    uint32_t magic, version;
    uint64_t size; // sizeof(AntsCkptBlob)
    AntsCfg cfg;   // the saving handle's, whole
    int32_t cur, steps_since_update, host_timestep;
    uint32_t obs_seq, sum_obs;
    uint8_t need_full_collect, is_reset, episode_over, has_gen, sum_due, sum_live, need_wall_clear, _pad[5];
    int64_t sweeps;
    uint64_t episode_seed;
    double deposit_strength; // KP::deposit_strength (antsrl_set_activation changes it)
    AntsGen gen;             // walls_input stored as NULL
};
