// antsrl_rework.hip — inference of the rework agent's net (CollectModelRework, agents/collect_agent_rework.py:24-63;
// antsrl_rework.h has the shapes and the collapsed buffer): the ten layers have no activation between them, so they are
// multiplied out once per weight change (k_rework_collapse, float64) and every step is NQ dot products of length D per
// row (k_rework_act, fp32): a stream over the observation tensor.
//
// k_rework_collapse — one workgroup per output row o of Wc (NQ workgroups of 256 threads).  Row o of the head's last layer
// (rotation_layer4 row o for o < n_rot, else pheromone_layer2 row o - n_rot) is widened to float64 as v, bc = that
// layer's bias[o]; then v is pushed down through the layers below it, the head's own first and layer4, 3, 2, 1 last
// (W_l [out][in], b_l [out], float32 widened exactly):
//     bc  <- (((bc + v[0] b_l[0]) + v[1] b_l[1]) + ...) + v[out-1] b_l[out-1]
//     v'[c] = (((0 + v[0] W_l[0][c]) + v[1] W_l[1][c]) + ...) + v[out-1] W_l[out-1][c]        for every c < in
// every product rounded to float64 before it is added (-ffp-contract=off), the contracted index ascending: thread t
// owns the columns c = t, t + 256, ... (coalesced over W_l's rows), the last thread also the bias sum.  v lives in
// LDS (two buffers of RW_MAX_D doubles).  After layer1, Wc[o][c] = (float)v[c] and bc[o] = (float)bc: one rounding
// each.  No atomics: every launch gives the same bits.  It runs once per weight change and is not tuned.
//
// k_rework_act<OBS16, NQP> — q[m][o] = bc[o] + sum_k x[m][k] Wc[o][k], x = cat[obs row, agent_state row], both argmaxes
// (first maximum).  NQP is NQ padded to 8 or 16 (zero rows), so that the accumulators stay in registers.  Wc is copied
// once per workgroup into LDS (NQP x Dp floats, Dp = D rounded up to 64, zero beyond D, in the order the lanes read it).
// Sixteen lanes share a row: lane l of the group takes k = 64 c + 4 l .. + 3 of every 64-input chunk c, so a group reads
// 256 contiguous bytes (fp32) of its row per load instruction and a wave four rows; a wave works on two such sets of
// four rows at a time (RW_U) and issues the loads of four chunks together (RW_G).  Outputs 2 p and 2 p + 1 share one
// packed fma (v_pk_fma_f32: each half is the fmaf below).
// Order of a row's sums, the same for every row whatever M, its place in the batch, the grid and the format:
//     lane l:   a = 0;  for c ascending, for i = 0..3:  a = fmaf(x[64 c + 4 l + i], Wc[o][64 c + 4 l + i], a)
//     group:    a += a of lane l ^ 1;  then l ^ 2;  then 7 - l within its eight;  then 15 - l     (every lane holds the sum)
//     q = a + bc[o]
// Loads: a chunk that lies inside the observation row (64 (c + 1) <= F) is read with one 16-byte load per lane (fp32,
// 4-byte aligned: a row starts at 4 m F bytes) or three aligned dwords and a funnel shift (bf16: a row starts at 2 m F
// bytes, on an odd element for odd m F; the third dword is clamped to the buffer's last whole dword and is only used
// where it lies inside).  The chunks that hold the row's end, the two agent_state inputs and the zero pad are read
// element by element on addresses clamped into the row, then selected.  Rows past M are clamped to row M - 1 and not
// written.  Nothing outside obs, agent_state and the collapsed buffer is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_rework.h"

#define RW_TPB 256
#define RW_U 2              // sets of four rows a wave has in flight
#define RW_G 4              // chunks of a row whose loads are issued together
#define RW_MAX_BLOCKS 1024  // 4 workgroups per CU, what 120 VGPRs admit; rows beyond are looped

typedef float rw_f32x2 __attribute__((ext_vector_type(2)));

// inputs of layer l in the state_dict's order (its outputs are the inputs of the layer above it)
__device__ __forceinline__ int rw_in(const ReworkDims &d, int l)
{
    switch (l) {
    case 0: return d.D;
    case 1: return d.g1;
    case 2: return d.g2;
    case 3: return d.g3;
    case 4: return d.D;
    case 5: return d.r1;
    case 6: return d.r2;
    case 7: return d.r3;
    case 8: return d.D;
    default: return d.p1;
    }
}

__global__ void __launch_bounds__(RW_TPB)
k_rework_collapse(const ReworkParams P, const ReworkDims d, float *__restrict__ collapsed)
{
    __shared__ double vbuf[2][RW_MAX_D];
    const int o = blockIdx.x, tid = threadIdx.x;
    const bool rot = o < d.n_rot;
    const int start = rot ? 7 : 9, row = rot ? o : o - d.n_rot;
    const int npush = rot ? 7 : 5; // rotation_layer3, 2, 1, layer4, 3, 2, 1  /  pheromone_layer1, layer4, 3, 2, 1
    int width = rw_in(d, start);
    double *cur = vbuf[0], *nxt = vbuf[1];
    for (int c = tid; c < width; c += RW_TPB) cur[c] = (double)P.p[2 * start][(size_t)row * width + c];
    double bc = (double)P.p[2 * start + 1][row]; // (the last thread's is the one that counts)
    __syncthreads();
    for (int s = 0; s < npush; ++s) {
        const int l = rot ? 6 - s : (s == 0 ? 8 : 4 - s);
        const float *__restrict__ W = P.p[2 * l], *__restrict__ b = P.p[2 * l + 1];
        const int in = rw_in(d, l); // rw_out(d, l) == width
        for (int c = tid; c < in; c += RW_TPB) {
            double a = 0.0;
            for (int i = 0; i < width; ++i) a = a + cur[i] * (double)W[(size_t)i * in + c];
            nxt[c] = a;
        }
        if (tid == RW_TPB - 1)
            for (int i = 0; i < width; ++i) bc = bc + cur[i] * (double)b[i];
        __syncthreads();
        double *t = cur;
        cur = nxt;
        nxt = t;
        width = in;
    }
    // width == D
    const int NQ = d.n_rot + d.n_ph;
    for (int c = tid; c < d.D; c += RW_TPB) collapsed[(size_t)o * d.D + c] = (float)cur[c];
    if (tid == RW_TPB - 1) collapsed[(size_t)NQ * d.D + o] = (float)bc;
}

hipError_t antsrl_launch_rework_collapse(const ReworkParams &P, const ReworkDims &d, float *collapsed, hipStream_t st)
{
    hipLaunchKernelGGL(k_rework_collapse, dim3(d.n_rot + d.n_ph), dim3(RW_TPB), 0, st, P, d, collapsed);
    return hipGetLastError();
}

template <bool OBS16, int NQP>
__global__ void __launch_bounds__(RW_TPB)
k_rework_act(const float *__restrict__ collapsed, const void *__restrict__ obs_, const float *__restrict__ agent_state,
             int8_t *__restrict__ rot_out, int8_t *__restrict__ ph_out, float *__restrict__ q_out, const int M, const int F,
             const int n_rot, const int n_ph, const int nchunks)
{
    // Wc in LDS, zero rows past NQ, zero columns past D, in the order a lane reads it: [output pair p][chunk c][half h]
    // [lane l][4] with the four floats Wc[2p][k], Wc[2p+1][k], Wc[2p][k+1], Wc[2p+1][k+1] at k = 64 c + 4 l + 2 h
    extern __shared__ __align__(16) float ws[];
    const int D = F + 2, NQ = n_rot + n_ph, Dp = 64 * nchunks;
    for (int idx = threadIdx.x; idx < NQP * Dp; idx += RW_TPB) {
        const int p = idx / (2 * Dp), r = idx - p * (2 * Dp), c = r >> 7, h = (r >> 6) & 1, l = (r >> 2) & 15, e = r & 3;
        const int o = 2 * p + (e & 1), k = 64 * c + 4 * l + 2 * h + (e >> 1);
        const bool in = o < NQ && k < D;
        const float w = collapsed[in ? (size_t)o * D + k : 0]; // unconditional load on a clamped address, then select
        ws[idx] = in ? w : 0.0f;
    }
    __syncthreads();

    const float *obs = static_cast<const float *>(obs_);
    const uint16_t *obs16 = static_cast<const uint16_t *>(obs_);
    const uint32_t *obs32 = static_cast<const uint32_t *>(obs_);
    const size_t last_dword = (size_t)M * F / 2 - 1; // bf16: the buffer's last whole dword (used by full chunks: F >= 64)
    const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15;
    const int wave = (blockIdx.x * RW_TPB + threadIdx.x) >> 6, nwaves = (gridDim.x * RW_TPB) >> 6;
    const int nfull = F / 64;                  // chunks that lie inside the observation row
    const int npass = (int)(((long long)M + 4 * RW_U - 1) / (4 * RW_U));
    float bias[NQP];
#pragma unroll
    for (int o = 0; o < NQP; ++o) bias[o] = collapsed[(size_t)NQ * D + (o < NQ ? o : 0)];
    for (int pass = wave; pass < npass; pass += nwaves) {
        long long m[RW_U];
        size_t base[RW_U]; // element index of the row's start, the row clamped into the batch
        float as0[RW_U], as1[RW_U];
#pragma unroll
        for (int u = 0; u < RW_U; ++u) {
            m[u] = (long long)pass * (4 * RW_U) + 4 * u + g;
            const size_t mc = (size_t)(m[u] < M ? m[u] : M - 1);
            base[u] = mc * F;
            as0[u] = agent_state[mc * 2];
            as1[u] = agent_state[mc * 2 + 1];
        }
        rw_f32x2 acc[RW_U][NQP / 2]; // outputs 2 p and 2 p + 1: one packed fma for both
#pragma unroll
        for (int u = 0; u < RW_U; ++u)
#pragma unroll
            for (int p = 0; p < NQP / 2; ++p) acc[u][p] = rw_f32x2{0.0f, 0.0f};
        // a chunk inside the observation row: one wide load per row (bf16: three aligned dwords and a funnel shift)
        auto load_full = [&](int c, float(&x)[RW_U][4]) {
            const int k = 64 * c + 4 * l;
#pragma unroll
            for (int u = 0; u < RW_U; ++u) {
                if (OBS16) {
                    const size_t e = base[u] + k, d0 = e >> 1;
                    const size_t d2 = d0 + 2 < last_dword ? d0 + 2 : last_dword;
                    const uint32_t w0 = obs32[d0], w1 = obs32[d0 + 1], w2 = obs32[d2];
                    const uint32_t sh = (uint32_t)(e & 1) * 16u;
                    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh), hi = __builtin_amdgcn_alignbit(w2, w1, sh);
                    x[u][0] = __uint_as_float(lo << 16);
                    x[u][1] = __uint_as_float(lo & 0xffff0000u);
                    x[u][2] = __uint_as_float(hi << 16);
                    x[u][3] = __uint_as_float(hi & 0xffff0000u);
                } else {
                    const RwF4 v = *reinterpret_cast<const RwF4 *>(obs + base[u] + k);
#pragma unroll
                    for (int i = 0; i < 4; ++i) x[u][i] = v.v[i];
                }
            }
        };
        // the row's end, agent_state, the zero pad: loads on addresses clamped into the row, then selects
        // (every load unconditional: inside a per-lane branch each one gets its own s_waitcnt vmcnt(0))
        auto load_tail = [&](int c, float(&x)[RW_U][4]) {
            const int k = 64 * c + 4 * l;
#pragma unroll
            for (int u = 0; u < RW_U; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const size_t e = base[u] + min(k + i, F - 1);
                    x[u][i] = OBS16 ? __uint_as_float((uint32_t)obs16[e] << 16) : obs[e];
                }
#pragma unroll
            for (int u = 0; u < RW_U; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int kk = k + i;
                    x[u][i] = kk < F ? x[u][i] : (kk == F ? as0[u] : (kk == F + 1 ? as1[u] : 0.0f));
                }
        };
        auto mac = [&](int c, const float(&x)[RW_U][4]) {
#pragma unroll
            for (int p = 0; p < NQP / 2; ++p) {
                const float *wp = ws + ((p * nchunks + c) * 2) * 64 + 4 * l;
                const float4 wa = *reinterpret_cast<const float4 *>(wp), wb = *reinterpret_cast<const float4 *>(wp + 64);
#pragma unroll
                for (int u = 0; u < RW_U; ++u) {
                    acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][0], x[u][0]}, rw_f32x2{wa.x, wa.y}, acc[u][p]);
                    acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][1], x[u][1]}, rw_f32x2{wa.z, wa.w}, acc[u][p]);
                    acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][2], x[u][2]}, rw_f32x2{wb.x, wb.y}, acc[u][p]);
                    acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][3], x[u][3]}, rw_f32x2{wb.z, wb.w}, acc[u][p]);
                }
            }
        };
        // the loads of RW_G chunks are issued before the first of them is used: a wave keeps RW_G * RW_U wide loads in
        // flight (one chunk at a time: float32 rows 0.069 ms instead of 0.057 at 512 x 512 rows of 294)
        int c = 0;
        for (; c + RW_G <= nfull; c += RW_G) {
            float x[RW_G][RW_U][4];
#pragma unroll
            for (int j = 0; j < RW_G; ++j) load_full(c + j, x[j]);
#pragma unroll
            for (int j = 0; j < RW_G; ++j) mac(c + j, x[j]);
        }
        for (; c < nchunks; ++c) {
            float x[RW_U][4];
            if (c < nfull)
                load_full(c, x);
            else
                load_tail(c, x);
            mac(c, x);
        }
#pragma unroll
        for (int u = 0; u < RW_U; ++u) {
            float q[NQP];
#pragma unroll
            for (int o = 0; o < NQP; ++o) q[o] = rw_group_sum(acc[u][o >> 1][o & 1]) + bias[o];
            // first maximum of each head (a NaN never wins)
            int ir = 0, ip = 0;
            float br = q[0], bp = 0.0f;
#pragma unroll
            for (int o = 1; o < NQP; ++o) {
                if (o < n_rot && q[o] > br) {
                    br = q[o];
                    ir = o;
                }
                if (o == n_rot) bp = q[o];
                if (o > n_rot && o < NQ && q[o] > bp) {
                    bp = q[o];
                    ip = o - n_rot;
                }
            }
            if (l == 0 && m[u] < M) {
                rot_out[m[u]] = (int8_t)(ir - n_rot / 2);
                ph_out[m[u]] = (int8_t)ip;
                if (q_out) {
#pragma unroll
                    for (int o = 0; o < NQP; ++o)
                        if (o < NQ) q_out[(size_t)m[u] * NQ + o] = q[o];
                }
            }
        }
    }
}

template <bool OBS16, int NQP>
static hipError_t rw_launch_act(const float *collapsed, const ReworkDims &d, const void *obs, const float *agent_state, int M,
                                int8_t *rot, int8_t *ph, float *q_out, hipStream_t st)
{
    const int nchunks = (d.D + 63) / 64;
    const size_t lds = (size_t)NQP * 64 * nchunks * sizeof(float); // <= 64 KiB (NQP 16, D 1024)
    const long long want = ((long long)M + 16 * RW_U - 1) / (16 * RW_U); // a workgroup's four waves take 16 RW_U rows a pass
    const int blocks = (int)(want < RW_MAX_BLOCKS ? want : RW_MAX_BLOCKS);
    hipLaunchKernelGGL((k_rework_act<OBS16, NQP>), dim3(blocks), dim3(RW_TPB), lds, st, collapsed, obs, agent_state, rot, ph,
                       q_out, M, d.F, d.n_rot, d.n_ph, nchunks);
    return hipGetLastError();
}

hipError_t antsrl_launch_rework_act(const float *collapsed, const ReworkDims &d, const void *obs, bool obs_bf16,
                                    const float *agent_state, int M, int8_t *rot, int8_t *ph, float *q_out, hipStream_t st)
{
    const bool small = d.n_rot + d.n_ph <= 8;
    if (obs_bf16)
        return small ? rw_launch_act<true, 8>(collapsed, d, obs, agent_state, M, rot, ph, q_out, st)
                     : rw_launch_act<true, 16>(collapsed, d, obs, agent_state, M, rot, ph, q_out, st);
    return small ? rw_launch_act<false, 8>(collapsed, d, obs, agent_state, M, rot, ph, q_out, st)
                 : rw_launch_act<false, 16>(collapsed, d, obs, agent_state, M, rot, ph, q_out, st);
}
