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
// k_rework_act<OBS16, NQP, SEL = false> — q[m][o] = bc[o] + sum_k x[m][k] Wc[o][k], x = cat[obs row, agent_state row], both argmaxes
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
//
// k_rework_act<OBS16, NQP, SEL = true>, "k_rework_act_select" — k_rework_act and antsrl_agent_select_actions'
// epsilon-greedy in one launch (antsrl_policy_rework_select).  It is the same kernel text, so an evaluated row gets
// k_rework_act's bits, and SEL = false compiles to the instructions and registers it had without the switch.  A wave pass is
// 4 RW_U consecutive rows, hence a contiguous range of colonies.  In front of its loads the pass finds out which of its
// rows belong to a colony that explores this step (antsrl_draw.h): lane j of the wave looks after row j of the pass.
// When the pass lies inside one colony (always, once n_ants is a multiple of 4 RW_U) the colony and its explore draw are
// wave-uniform and computed once, in scalar registers; a pass that straddles colonies makes one draw per row and
// collects the flags with a ballot.  Either way the flags end up in a scalar mask and every branch on it is wave-uniform:
//     every row of the pass explores:  no load, no fma; lanes 0 .. 4 RW_U - 1 draw their row's two actions and store them
//     no row explores:                 k_rework_act's pass
//     mixed:                           the exploring rows' lanes draw and store, then k_rework_act's pass on all rows,
//                                      of which the evaluating lanes of the exploring rows store nothing (actions or q)
// The three draws of a row share their first two rounds (draw_env_step: colony and step); a drawn action costs the other
// two.  explored[e] is written by the lane whose row is colony e's first ant: one writer.  No atomics, no LDS beyond Wc.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_draw.h"
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

// SEL false: antsrl_policy_rework (`sel` is not read); SEL true: antsrl_policy_rework_select ("k_rework_act_select")
template <bool OBS16, int NQP, bool SEL>
__global__ void __launch_bounds__(RW_TPB)
k_rework_act(const float *__restrict__ collapsed, const void *__restrict__ obs_, const float *__restrict__ agent_state,
             int8_t *__restrict__ rot_out, int8_t *__restrict__ ph_out, float *__restrict__ q_out, const int M, const int F,
             const int n_rot, const int n_ph, const int nchunks, const ReworkSelect sel)
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
    // (SEL: the pass index in a scalar register, so that a pass inside one colony keeps its explore draw on the scalar unit)
    for (int pass = SEL ? __builtin_amdgcn_readfirstlane(wave) : wave; pass < npass; pass += nwaves) {
        // SEL: lane j < 4 RW_U looks after row `first + j` of the pass: its colony `env`, its ant index `ant` there, and
        // `key`, the two rounds every draw of that colony at this step starts with.  `ex` and `rows` are wave-uniform.
        uint32_t ex = 0;   // bit j: row first + j belongs to a colony that explores this step
        uint32_t rows = 0; // bit j: row first + j lies inside the batch
        if (SEL) {
            uint32_t env, ant;
            uint64_t key;
            const uint32_t first = (uint32_t)pass * (4 * RW_U), valid = min((uint32_t)(4 * RW_U), (uint32_t)M - first);
            const uint32_t e0 = first / sel.n_ants, a0 = first - e0 * sel.n_ants;
            rows = (1u << valid) - 1u;
            if (a0 + valid <= sel.n_ants) { // the pass lies inside one colony: one draw, on wave-uniform values
                env = e0;
                ant = a0 + (uint32_t)(lane & (4 * RW_U - 1));
                key = draw_env_step(sel.seed, (uint64_t)sel.env_base + e0, sel.step);
                ex = draw_u01(draw_item(key, 0, ANTSRL_DRAW_EXPLORE)) < sel.epsilon ? rows : 0u;
            } else { // it straddles colonies: one draw per row, lanes past the batch on its last row (masked by `rows`)
                const uint32_t r = min(first + (uint32_t)(lane & (4 * RW_U - 1)), (uint32_t)M - 1u);
                env = r / sel.n_ants;
                ant = r - env * sel.n_ants;
                key = draw_env_step(sel.seed, (uint64_t)sel.env_base + env, sel.step);
                ex = (uint32_t)__ballot(draw_u01(draw_item(key, 0, ANTSRL_DRAW_EXPLORE)) < sel.epsilon) & rows;
            }
            // the drawn actions, by the row's lane alone, and in front of the evaluation, across which only `ex` then lives
            if (ex != 0 && lane < 4 * RW_U && ((ex >> lane) & 1u)) {
                const size_t row = (size_t)first + lane;
                rot_out[row] = (int8_t)((int)draw_below(draw_item(key, ant, ANTSRL_DRAW_ROTATION), (uint32_t)n_rot) - n_rot / 2);
                ph_out[row] = (int8_t)draw_below(draw_item(key, ant, ANTSRL_DRAW_PHEROMONE), (uint32_t)n_ph);
            }
            // a colony's flag is written by the lane of its first ant's row: one writer
            if (sel.explored && lane < 4 * RW_U && ((rows >> lane) & 1u) && ant == 0) sel.explored[env] = (uint8_t)((ex >> lane) & 1u);
        }
        if (!SEL || ex != rows) { // (wave-uniform) a pass whose rows all explore loads nothing and multiplies nothing
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
                // (SEL: an exploring row of a mixed pass was evaluated like the others and is not stored from here)
                if (l == 0 && m[u] < M && !(SEL && ((ex >> (4 * u + g)) & 1u))) {
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
}

// sel: NULL launches k_rework_act
template <bool OBS16, int NQP>
static hipError_t rw_launch_act(const float *collapsed, const ReworkDims &d, const void *obs, const float *agent_state, int M,
                                const ReworkSelect *sel, int8_t *rot, int8_t *ph, float *q_out, hipStream_t st)
{
    const int nchunks = (d.D + 63) / 64;
    const size_t lds = (size_t)NQP * 64 * nchunks * sizeof(float); // <= 64 KiB (NQP 16, D 1024)
    const long long want = ((long long)M + 16 * RW_U - 1) / (16 * RW_U); // a workgroup's four waves take 16 RW_U rows a pass
    const int blocks = (int)(want < RW_MAX_BLOCKS ? want : RW_MAX_BLOCKS);
    if (sel)
        hipLaunchKernelGGL((k_rework_act<OBS16, NQP, true>), dim3(blocks), dim3(RW_TPB), lds, st, collapsed, obs, agent_state,
                           rot, ph, q_out, M, d.F, d.n_rot, d.n_ph, nchunks, *sel);
    else
        hipLaunchKernelGGL((k_rework_act<OBS16, NQP, false>), dim3(blocks), dim3(RW_TPB), lds, st, collapsed, obs, agent_state,
                           rot, ph, q_out, M, d.F, d.n_rot, d.n_ph, nchunks, ReworkSelect{});
    return hipGetLastError();
}

static hipError_t rw_dispatch_act(const float *collapsed, const ReworkDims &d, const void *obs, bool obs_bf16,
                                  const float *agent_state, int M, const ReworkSelect *sel, int8_t *rot, int8_t *ph,
                                  float *q_out, hipStream_t st)
{
    const bool small = d.n_rot + d.n_ph <= 8;
    if (obs_bf16)
        return small ? rw_launch_act<true, 8>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st)
                     : rw_launch_act<true, 16>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st);
    return small ? rw_launch_act<false, 8>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st)
                 : rw_launch_act<false, 16>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st);
}

hipError_t antsrl_launch_rework_act(const float *collapsed, const ReworkDims &d, const void *obs, bool obs_bf16,
                                    const float *agent_state, int M, int8_t *rot, int8_t *ph, float *q_out, hipStream_t st)
{
    return rw_dispatch_act(collapsed, d, obs, obs_bf16, agent_state, M, nullptr, rot, ph, q_out, st);
}

hipError_t antsrl_launch_rework_act_select(const float *collapsed, const ReworkDims &d, const void *obs, bool obs_bf16,
                                           const float *agent_state, int M, const ReworkSelect &sel, int8_t *rot, int8_t *ph,
                                           float *q_out, hipStream_t st)
{
    return rw_dispatch_act(collapsed, d, obs, obs_bf16, agent_state, M, &sel, rot, ph, q_out, st);
}
