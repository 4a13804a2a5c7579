// antsrl_stats.h — the colony statistics' block (antsrl_stats.hip; include/antsrl.h, "The colony statistics", is the
// specification): where a row's words and the scratch's partials lie, and THE ORDER OF THE SUMS the kernels keep, for E
// environments of N ants, C pheromone channels and G = W * H cells.
//
// The block, in float64 / int64 words of 8 bytes, dense: max_rows rows of E records of Q = 7 + 2 C words, then the scratch.
//     word 0       int64   timestep              4       double  food_carried
//          1       double  anthill_food          5       int64   n_carrying
//          2       double  food_left             6       int64   explored_cells, -1 without an explored map
//          3       int64   food_cells            7 + 2c  double  phero_mass[c]        8 + 2c  int64  phero_cells[c]
// The scratch holds, per environment, P = 3 + 2 C planes of nseg = ceil(G / STATS_SEG) partials, [E][P][nseg] (a plane is
// contiguous, so the second stage reads it coalesced); plane 0 food_left, 1 food_cells, 2 explored_cells, 3 + 2c
// phero_mass[c], 4 + 2c phero_cells[c].
//
// The order of the sums (STATS_THREADS = 256 slots; every add a float64 add, round to nearest even; no atomics):
//     cells:   the canonical cell ids g = x * H + y are cut into segments of STATS_SEG = 4096; one workgroup per (segment,
//              environment).  Slot t starts at +0.0 / 0 and takes the cells seg * 4096 + t + 256 k, k = 0, 1, ..., ascending,
//              skipping g >= G; the 256 slots are folded with x[i] += x[i + s] for i < s, s = 128, ..., 1; x[0] is the
//              segment's partial.
//     fold:    one workgroup per environment: slot t takes the partials of the segments t, t + 256, ... ascending, the same
//              fold; food_carried likewise over the ants t, t + 256, ... (k_monitor_report's rule).
// The counts are int64 and exact; they take the same path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_device.h"
#include "antsrl_fail.h"

#define STATS_THREADS 256
#define STATS_SEG 4096

enum { STATS_W_TIMESTEP = 0, STATS_W_ANTHILL_FOOD, STATS_W_FOOD_LEFT, STATS_W_FOOD_CELLS, STATS_W_FOOD_CARRIED,
       STATS_W_N_CARRYING, STATS_W_EXPLORED_CELLS, STATS_W_PHERO };
enum { STATS_P_FOOD_LEFT = 0, STATS_P_FOOD_CELLS, STATS_P_EXPLORED_CELLS, STATS_P_PHERO };

struct StatsLayout {
    int E, C, Q, P, has_expl;      // Q: words of a record, P: planes of partials
    size_t G, nseg;
    size_t row_words, scratch_words; // E * Q; E * P * nseg
};

static inline StatsLayout antsrl_stats_layout(int E, int C, size_t G, int has_expl)
{
    StatsLayout L;
    L.E = E; L.C = C; L.Q = 7 + 2 * C; L.P = 3 + 2 * C; L.has_expl = has_expl;
    L.G = G; L.nseg = (G + STATS_SEG - 1) / STATS_SEG;
    L.row_words = (size_t)E * (size_t)L.Q;
    L.scratch_words = (size_t)E * (size_t)L.P * L.nseg;
    return L;
}

// two launches: the segments' partials into `scratch`, then the row
ANTSRL_INTERNAL hipError_t antsrl_launch_stats_row(const KP &p, int cur, const StatsLayout &L, double *row, double *scratch,
                                                   hipStream_t st);
