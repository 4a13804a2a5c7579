// antsrl_recorder.h — the episode recorder's block (antsrl_recorder.hip; include/antsrl.h, "The episode recorder", is the
// specification): where every section of the static part and of a frame lies, for S selected environments of N ants, R
// rocks, C pheromone channels and G = W * H cells.  Every section starts 16-byte aligned: a section of n bytes takes
// a16(n) = n rounded up to 16.
//
//   static part, per selected environment (st_env bytes; S of them, in the order the indices were given):
//       anthill_xyr   int32 [3]                (16 bytes)
//       rock_rw       double [R][2]            {radius, weight}
//       walls         uint8 [W][H]             a16(G)
//   then max_frames frames of frame_bytes = S * fr_env bytes; per selected environment:
//       timestep      int32                    (16 bytes)
//       anthill_food  double                   (16 bytes)
//       rock_centers  double [R][2]
//       ants_xyt      double [N][3]            a16(24 N)
//       holding       float  [N]               a16(4 N)
//       mandibles     uint8  [N]               a16(N)
//       reward_state  uint8  [N]               a16(N)
//       phero         uint8  [C] planes of [W][H], each plane a16(G) bytes
//       food          uint8  [W][H]            a16(G)
//       explored      uint8  [W][H]            a16(G); the section is ABSENT without a heatmap
// The kernels write every byte of every section, its padding (zeros) included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_device.h"
#include "antsrl_fail.h"

#define ANTSRL_RECORDER_THREADS 256

struct RecorderLayout {
    int S, N, R, C, has_expl;
    size_t G, Gp;                                       // cells, a16(cells)
    size_t st_xyr, st_rock_rw, st_walls, st_env;        // static part, offsets inside one environment's piece
    size_t fr_timestep, fr_anthill_food, fr_rock_centers, fr_xyt, fr_holding, fr_mandibles, fr_reward_state, fr_phero, fr_food, fr_explored,
        fr_env;                                         // a frame, offsets inside one environment's piece
    size_t static_bytes, frame_bytes;
};

__host__ __device__ static inline size_t rec_a16(size_t n) { return (n + 15) / 16 * 16; }

static inline RecorderLayout antsrl_recorder_layout(int S, int N, int R, int C, size_t G, int has_expl)
{
    RecorderLayout L;
    L.S = S; L.N = N; L.R = R; L.C = C; L.has_expl = has_expl;
    L.G = G; L.Gp = rec_a16(G);
    L.st_xyr = 0;
    L.st_rock_rw = 16;
    L.st_walls = L.st_rock_rw + 16 * (size_t)R;
    L.st_env = L.st_walls + L.Gp;
    L.fr_timestep = 0;
    L.fr_anthill_food = 16;
    L.fr_rock_centers = 32;
    L.fr_xyt = L.fr_rock_centers + 16 * (size_t)R;
    L.fr_holding = L.fr_xyt + rec_a16(24 * (size_t)N);
    L.fr_mandibles = L.fr_holding + rec_a16(4 * (size_t)N);
    L.fr_reward_state = L.fr_mandibles + rec_a16((size_t)N);
    L.fr_phero = L.fr_reward_state + rec_a16((size_t)N);
    L.fr_food = L.fr_phero + (size_t)C * L.Gp;
    L.fr_explored = L.fr_food + L.Gp;
    L.fr_env = L.fr_explored + (has_expl ? L.Gp : 0);
    L.static_bytes = (size_t)S * L.st_env;
    L.frame_bytes = (size_t)S * L.fr_env;
    return L;
}

// the selected environments travel by value, in the kernel arguments
struct RecorderSel {
    int32_t env[ANTSRL_RECORDER_MAX_ENVS];
};

// one launch each; `dst`: the static part's / the frame's first byte
ANTSRL_INTERNAL hipError_t antsrl_launch_record_static(const KP &p, const RecorderLayout &L, const RecorderSel &sel,
                                                       unsigned char *dst, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_record_frame(const KP &p, int cur, const RecorderLayout &L, const RecorderSel &sel,
                                                      unsigned char *dst, hipStream_t st);
