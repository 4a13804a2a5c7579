// antsrl_recorder.hip — the episode recorder's kernels (include/antsrl.h, "The episode recorder"; antsrl_recorder.h holds
// the block's layout).  What the replay viewer needs of the chosen environments — Environment.save_state's visualisation
// copies (environment.py:36-40): uint8 grids and the ants — goes into a device-resident frame log, one launch per step,
// nothing read back.  The C-ABI entries are in antsrl_logapi.hip.
//
//   k_record_static   once per recorded episode: anthill_xyr, the rocks' radius and weight, the walls
//   k_record_frame    once per recorded step: timestep, anthill_food, rock centres, the ants, and the pheromone / food /
//                     explored grids as uint8
// blockIdx.y is the slot of a selected environment (their indices travel in the kernel arguments); the workgroups of a
// slot share that environment's work items in a grid-stride loop.  An item of a grid section is FOUR consecutive
// canonical cells packed into one 4-byte store, so a wave writes 256 contiguous bytes and no two lanes share a word; the
// tail of a section (cells past W * H, up to the section's 16-byte padding) belongs to the item that holds the last cell
// and to the all-padding items behind it, which store zeros.  The per-cell loads are k_read_state's (antsrl_cellread.h).
// No atomics, no LDS, one writer per word.
#include "antsrl_util.h"
#include "antsrl_cellread.h"
#include "antsrl_recorder.h"

// float -> uint8 as the viewer's copies cast it (pheromone.py:17, food.py:10: numpy's astype(np.uint8)): truncation
// toward zero for 0 <= v < 256; 256 and above saturates to 255 (include/antsrl.h states the rule)
__device__ __forceinline__ uint32_t rec_u8(const float v)
{
    return v >= 256.0f ? 255u : (uint32_t)(uint8_t)(int32_t)v;
}

struct RecorderArgs {
    RecorderLayout L;
    RecorderSel sel;
    unsigned char *dst;
    int cur;
};

__global__ void __launch_bounds__(ANTSRL_RECORDER_THREADS) k_record_static(const KP p, const RecorderArgs a)
{
    const RecorderLayout &L = a.L;
    const size_t e = (size_t)a.sel.env[blockIdx.y];
    unsigned char *dst = a.dst + (size_t)blockIdx.y * L.st_env;
    const size_t nq = L.Gp / 4, items = nq + 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
        if (i < nq) {
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t g = 4 * i + k;
                if (g < L.G) w |= (uint32_t)cell_bit(p, p.s.walls_bits, e, (uint32_t)g) << (8 * k);
            }
            reinterpret_cast<uint32_t *>(dst + L.st_walls)[i] = w;
        } else {
            int32_t *xyr = reinterpret_cast<int32_t *>(dst + L.st_xyr);
            for (int j = 0; j < 3; ++j) xyr[j] = p.s.anthill_xyr[3 * e + j];
            xyr[3] = 0;
            double *rw = reinterpret_cast<double *>(dst + L.st_rock_rw);
            for (int q = 0; q < L.R; ++q) {
                rw[2 * q] = p.s.rock_r[e * L.R + q];
                rw[2 * q + 1] = p.s.rock_w[e * L.R + q];
            }
        }
    }
}

__global__ void __launch_bounds__(ANTSRL_RECORDER_THREADS) k_record_frame(const KP p, const RecorderArgs a)
{
    const RecorderLayout &L = a.L;
    const size_t e = (size_t)a.sel.env[blockIdx.y];
    unsigned char *dst = a.dst + (size_t)blockIdx.y * L.fr_env;
    const size_t N = (size_t)L.N, Np = (N + 3) / 4 * 4, nqa = rec_a16(N) / 4;
    const size_t nq = L.Gp / 4, n_grid = (size_t)(L.C + 1 + L.has_expl) * nq;
    const size_t items = n_grid + Np + 2 * nqa + 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
        if (i < n_grid) { // ---- four cells of one grid plane
            const size_t plane = i / nq, q = i - plane * nq;
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t g = 4 * q + k;
                if (g >= L.G) continue;
                uint32_t b;
                if (plane < (size_t)L.C) b = rec_u8(cell_phero(p, a.cur, e, L.G, (uint32_t)g, (int)plane));
                else if (plane == (size_t)L.C) b = rec_u8(cell_food(p, e, L.G, (uint32_t)g));
                else b = cell_explored(p, e, L.G, (uint32_t)g);
                w |= b << (8 * k);
            }
            // (the planes follow each other: phero [C], food, explored — fr_phero + plane * Gp)
            reinterpret_cast<uint32_t *>(dst + L.fr_phero + plane * L.Gp)[q] = w;
            continue;
        }
        size_t j = i - n_grid;
        if (j < Np) { // ---- one ant: x, y, theta and holding (slots past N: the sections' padding)
            float *hold = reinterpret_cast<float *>(dst + L.fr_holding);
            double *xyt = reinterpret_cast<double *>(dst + L.fr_xyt);
            if (j < N) {
                const size_t ia = e * N + j;
                xyt[3 * j] = p.s.x[ia]; xyt[3 * j + 1] = p.s.y[ia]; xyt[3 * j + 2] = p.s.theta[ia];
                hold[j] = p.s.holding[ia];
            } else {
                hold[j] = 0.0f;
                if (j == N && (N & 1)) xyt[3 * N] = 0.0; // 24 N is 8 short of a multiple of 16
            }
            continue;
        }
        j -= Np;
        if (j < 2 * nqa) { // ---- four ants' mandibles / reward_state
            const bool rs = j >= nqa;
            const size_t q = rs ? j - nqa : j;
            const uint8_t *src = (rs ? p.s.reward_state : p.s.mandibles) + e * N;
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < N) w |= (uint32_t)src[4 * q + k] << (8 * k);
            reinterpret_cast<uint32_t *>(dst + (rs ? L.fr_reward_state : L.fr_mandibles))[q] = w;
            continue;
        }
        // ---- the environment's own values
        int32_t *ts = reinterpret_cast<int32_t *>(dst + L.fr_timestep);
        ts[0] = p.s.timestep[e];
        ts[1] = ts[2] = ts[3] = 0;
        double *af = reinterpret_cast<double *>(dst + L.fr_anthill_food);
        af[0] = p.s.anthill_food[e];
        af[1] = 0.0;
        double *rc = reinterpret_cast<double *>(dst + L.fr_rock_centers);
        for (int q = 0; q < L.R; ++q) {
            rc[2 * q] = p.s.rock_cx[e * L.R + q];
            rc[2 * q + 1] = p.s.rock_cy[e * L.R + q];
        }
    }
}

static unsigned rec_blocks(size_t items)
{
    size_t b = (items + ANTSRL_RECORDER_THREADS - 1) / ANTSRL_RECORDER_THREADS;
    return (unsigned)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}

hipError_t antsrl_launch_record_static(const KP &p, const RecorderLayout &L, const RecorderSel &sel, unsigned char *dst,
                                       hipStream_t st)
{
    RecorderArgs a = {L, sel, dst, 0};
    hipLaunchKernelGGL(k_record_static, dim3(rec_blocks(L.Gp / 4 + 1), (unsigned)L.S), dim3(ANTSRL_RECORDER_THREADS), 0, st, p, a);
    return hipGetLastError();
}

hipError_t antsrl_launch_record_frame(const KP &p, int cur, const RecorderLayout &L, const RecorderSel &sel,
                                      unsigned char *dst, hipStream_t st)
{
    RecorderArgs a = {L, sel, dst, cur};
    const size_t N = (size_t)L.N;
    const size_t items = (size_t)(L.C + 1 + L.has_expl) * (L.Gp / 4) + (N + 3) / 4 * 4 + 2 * (rec_a16(N) / 4) + 1;
    hipLaunchKernelGGL(k_record_frame, dim3(rec_blocks(items), (unsigned)L.S), dim3(ANTSRL_RECORDER_THREADS), 0, st, p, a);
    return hipGetLastError();
}
