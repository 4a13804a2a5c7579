// antsrl_reworktrain.hip — the DQN training step of the rework agent's net (CollectAgentRework.train,
// agents/collect_agent_rework.py:110-152; antsrl_reworktrain.h has the arguments and the workspace's layout,
// include/antsrl.h the contract).  CollectModelRework has no activation, so with x[b] a minibatch row, dq[b] the loss's
// derivative by the row's NQ outputs (non-zero at the two actions taken only),
//     G = sum_b dq[b] (x) x[b]  [NQ][D],   s = sum_b dq[b]  [NQ]
// M_l [NQ][out_l] the head rows pushed DOWN to layer l's output (the v of k_rework_collapse on its way; the unit rows at a
// head's last layer) and A_l [NQ][out_l] the pseudo-rows pushed UP (A_l = A_in(l) W_l^T + s (x) b_l, A of x being G), every
// layer's gradient is
//     dW_l = sum_k M_l[k] (x) A_in(l)[k],   db_l = sum_k M_l[k] s[k]        k over the pseudo-rows of l's head
// and no B x width activation exists.  Four launches, no atomics, every sum in a fixed order:
//
// k_reworktrain_down  — k_rework_collapse on the flat block (one workgroup per row o, the same float64 sequence, so the
//     model's collapsed buffer has that kernel's bits), storing v in front of every push as M_l[o]; rows of the other
//     head's layers are written as zeros.
// k_reworktrain_batch<NQP> — the stream over the rows: the hot path.  Both collapsed buffers (the model's from the
//     workspace, the target's from the caller) lie in LDS, zero-padded to [NQP][Dp], Dp = D rounded up to 64.  A workgroup
//     takes RT_ROWS = 16 minibatch rows at a time, one per 16 lanes, in k_rework_act's lane layout and order of sums
//     (lane l: k = 64 c + 4 l .. + 3, c ascending, fmaf; the group sum by DPP; + bc): q of the row under the model, q' of
//     its successor under the target, then per head
//         y = reward + discount * max q' * !done,   d = q[a] - y,   g = d * 2 / (n B)
//     (a clamped to [0, n)), handed over in LDS.  Then thread t owns the columns c = t, t + 256, ... of G: for the 16 rows
//     in ascending order it reads x[c] again (the line is in cache) and adds g_rot x[c] to its accumulator of row a_rot and
//     g_ph x[c] to that of row n_rot + a_ph: product rounded, then added; NQP accumulators per column, selected, not
//     indexed.  s and the two sums of d^2 ride along in threads 0 .. NQ - 1 and 64.  Rows beyond the grid's reach are
//     looped (workgroup w: rows 16 (w + i parts) ..), so a workgroup's partial is a sum over its rows in ascending order
//     from zero; it is written to slot w of the workspace.  Rows past B are row B - 1 with g = 0.
//     Loads: a chunk inside the observation row with one 4-byte-aligned 16-byte load per lane, the chunk with the row's
//     end, agent_state and the pad element by element on addresses clamped into the row, then selected.  idx is clamped
//     to [0, n_rows).  Nothing outside the arrays is read.
// k_reworktrain_up    — one workgroup per pseudo-row k: the partials added in workgroup order from zero (fp32) give
//     G[k], s[k] and, in workgroup 0, loss = L_rot / (n_rot B) + L_ph / (n_ph B); then A_l[k] in float64, thread j the
//     output j:  a = ((0 + A_in[0] W[j][0]) + A_in[1] W[j][1]) + ..., then a + s[k] b[j]; every product rounded before it is
//     added.  layer1..4, then rotation_layer1..3 (k < n_rot) or pheromone_layer1 (the others' rows: zeros).
// k_reworktrain_grad  — one thread per trained float i: its tensor from the block's offsets, then
//     (float)(((0 + M_l[k0][o] A[k0][c]) + M_l[k0 + 1][o] A[k0 + 1][c]) + ...) in float64 (s[k] for a bias, G widened for
//     layer1), stored if the caller wants it, and Adam on that float (adam_at) in a fused step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_lds_optin.h"
#include "antsrl_reworktrain.h"

#define RT_TPB 256
static_assert(RT_MAX_PARTS <= RT_TPB, "k_reworktrain_up loads one partial per thread");
#define RT_INFO 8 // floats of a row's hand-over in LDS: g_rot, g_ph, d_rot^2, d_ph^2, a_rot, n_rot + a_ph (int), the replay row (int64)

void antsrl_reworktrain_layout(const ReworkDims &d, int B, ReworkTrainLayout *L)
{
    const int NQ = d.n_rot + d.n_ph;
    const int out[RW_LAYERS] = {d.g1, d.g2, d.g3, d.D, d.r1, d.r2, d.r3, d.n_rot, d.p1, d.n_ph};
    const int in[RW_LAYERS] = {d.D, d.g1, d.g2, d.g3, d.D, d.r1, d.r2, d.r3, d.D, d.p1};
    const int src[RW_LAYERS] = {-1, 0, 1, 2, 3, 4, 5, 6, 3, 8};
    size_t off = 0;
    for (int l = 0; l < RW_LAYERS; ++l) {
        L->out[l] = out[l];
        L->in[l] = in[l];
        L->src[l] = src[l];
        L->k0[l] = l < 4 ? 0 : (l < 8 ? 0 : d.n_rot);
        L->k1[l] = l < 4 ? NQ : (l < 8 ? d.n_rot : NQ);
        L->off[2 * l] = off;
        off += (size_t)out[l] * in[l];
        L->off[2 * l + 1] = off;
        off += (size_t)out[l];
    }
    L->off[2 * RW_LAYERS] = off;
    const int passes = (B + RT_ROWS - 1) / RT_ROWS;
    L->parts = passes < RT_MAX_PARTS ? passes : RT_MAX_PARTS;
    L->part_stride = (NQ * d.D + NQ + 2 + 63) / 64 * 64;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    L->collapsed = take(sizeof(float) * ((size_t)NQ * d.D + NQ));
    for (int l = 0; l < RW_LAYERS; ++l) L->M[l] = take(sizeof(double) * NQ * out[l]);
    L->partials = take(sizeof(float) * (size_t)L->parts * L->part_stride);
    L->G = take(sizeof(float) * ((size_t)NQ * d.D + NQ));
    for (int l = 0; l < RW_LAYERS; ++l) L->A[l] = (l == 7 || l == 9) ? 0 : take(sizeof(double) * NQ * out[l]);
    L->bytes = at;
}

__global__ void __launch_bounds__(RT_TPB) k_reworktrain_down(const ReworkTrainArgs a)
{
    __shared__ double vbuf[2][RW_MAX_D];
    const ReworkDims &d = a.d;
    const ReworkTrainLayout &L = a.L;
    const int o = blockIdx.x, tid = threadIdx.x, NQ = d.n_rot + d.n_ph;
    const bool rot = o < d.n_rot;
    const int last = rot ? 7 : 9, row = rot ? o : o - d.n_rot;
    const int npush = rot ? 7 : 5; // rotation_layer3, 2, 1, layer4, 3, 2, 1  /  pheromone_layer1, layer4, 3, 2, 1
    const float *__restrict__ P = a.model;
    // this row of M in the layers above layer4: zeros in the other head's, the unit row in its own last
    for (int l = 4; l < RW_LAYERS; ++l) {
        if ((l < 8) == rot && l != last) continue;
        double *M = reinterpret_cast<double *>(a.work + L.M[l]) + (size_t)o * L.out[l];
        for (int c = tid; c < L.out[l]; c += RT_TPB) M[c] = (l == last && c == row) ? 1.0 : 0.0;
    }
    int width = L.in[last];
    double *cur = vbuf[0], *nxt = vbuf[1];
    for (int c = tid; c < width; c += RT_TPB) cur[c] = (double)P[L.off[2 * last] + (size_t)row * width + c];
    double bc = (double)P[L.off[2 * last + 1] + row]; // (the last thread's is the one that counts)
    __syncthreads();
    for (int s = 0; s < npush; ++s) {
        const int l = rot ? 6 - s : (s == 0 ? 8 : 4 - s);
        const float *__restrict__ W = P + L.off[2 * l], *__restrict__ b = P + L.off[2 * l + 1];
        const int in = L.in[l]; // L.out[l] == width
        double *M = reinterpret_cast<double *>(a.work + L.M[l]) + (size_t)o * width;
        for (int c = tid; c < width; c += RT_TPB) M[c] = cur[c];
        for (int c = tid; c < in; c += RT_TPB) {
            double v = 0.0;
            for (int i = 0; i < width; ++i) v = v + cur[i] * (double)W[(size_t)i * in + c];
            nxt[c] = v;
        }
        if (tid == RT_TPB - 1)
            for (int i = 0; i < width; ++i) bc = bc + cur[i] * (double)b[i];
        __syncthreads();
        double *t = cur;
        cur = nxt;
        nxt = t;
        width = in;
    }
    // width == D
    float *collapsed = reinterpret_cast<float *>(a.work + L.collapsed);
    for (int c = tid; c < d.D; c += RT_TPB) collapsed[(size_t)o * d.D + c] = (float)cur[c];
    if (tid == RT_TPB - 1) collapsed[(size_t)NQ * d.D + o] = (float)bc;
}

template <int NQP>
__global__ void __launch_bounds__(RT_TPB) k_reworktrain_batch(const ReworkTrainArgs a)
{
    // [NQP][Dp] of the model, [NQP][Dp] of the target (zero rows past NQ, zero columns past D), their biases [2][NQP], then
    // the rows' hand-over [RT_ROWS][RT_INFO]
    extern __shared__ __align__(16) float ws[];
    const int F = a.d.F, D = a.d.D, n_rot = a.d.n_rot, NQ = a.d.n_rot + a.d.n_ph, B = a.B;
    const int nchunks = (D + 63) / 64, Dp = 64 * nchunks, nfull = F / 64;
    float *wm = ws, *wt = ws + NQP * Dp, *bias = ws + 2 * NQP * Dp, *info = bias + 2 * NQP;
    const float *__restrict__ cm = reinterpret_cast<const float *>(a.work + a.L.collapsed), *__restrict__ ct = a.target;
    const int tid = threadIdx.x;
    for (int i = tid; i < NQP * Dp; i += RT_TPB) {
        const int o = i / Dp, k = i - o * Dp;
        const bool in = o < NQ && k < D;
        const size_t src = in ? (size_t)o * D + k : 0; // unconditional loads on a clamped address, then selects
        const float m = cm[src], t = ct[src];
        wm[i] = in ? m : 0.0f;
        wt[i] = in ? t : 0.0f;
    }
    if (tid < 2 * NQP) {
        const int o = tid & (NQP - 1);
        const float v = (tid < NQP ? cm : ct)[(size_t)NQ * D + (o < NQ ? o : 0)];
        bias[tid] = o < NQ ? v : 0.0f;
    }
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, l = lane & 15, r = 4 * (tid >> 6) + g;
    const int npass = (B + RT_ROWS - 1) / RT_ROWS;
    float acc[4][NQP];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < NQP; ++k) acc[j][k] = 0.0f;
    float sacc = 0.0f, lrot = 0.0f, lph = 0.0f;
    for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) {
        {
            const int b = pass * RT_ROWS + r;
            const bool valid = b < B;
            const int bb = valid ? b : B - 1;
            const long long ri = dqn_row(a, bb);
            const float *__restrict__ xs = a.states + (size_t)ri * F, *__restrict__ xn = a.new_states + (size_t)ri * F;
            const float as0 = a.agent_states[(size_t)ri * 2], as1 = a.agent_states[(size_t)ri * 2 + 1];
            const float an0 = a.new_agent_states[(size_t)ri * 2], an1 = a.new_agent_states[(size_t)ri * 2 + 1];
            float q[NQP], qn[NQP];
#pragma unroll
            for (int o = 0; o < NQP; ++o) q[o] = qn[o] = 0.0f;
            for (int c = 0; c < nchunks; ++c) {
                const int k = 64 * c + 4 * l;
                float x[4], y[4];
                if (c < nfull) { // (uniform) the chunk lies inside the observation row
                    const RwF4 vx = *reinterpret_cast<const RwF4 *>(xs + k), vy = *reinterpret_cast<const RwF4 *>(xn + k);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        x[i] = vx.v[i];
                        y[i] = vy.v[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = min(k + i, F - 1);
                        x[i] = xs[e];
                        y[i] = xn[e];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int kk = k + i;
                        x[i] = kk < F ? x[i] : (kk == F ? as0 : (kk == F + 1 ? as1 : 0.0f));
                        y[i] = kk < F ? y[i] : (kk == F ? an0 : (kk == F + 1 ? an1 : 0.0f));
                    }
                }
#pragma unroll
                for (int o = 0; o < NQP; ++o) {
                    const float4 w = *reinterpret_cast<const float4 *>(wm + o * Dp + k);
                    const float4 v = *reinterpret_cast<const float4 *>(wt + o * Dp + k);
                    q[o] = fmaf(x[0], w.x, q[o]);
                    q[o] = fmaf(x[1], w.y, q[o]);
                    q[o] = fmaf(x[2], w.z, q[o]);
                    q[o] = fmaf(x[3], w.w, q[o]);
                    qn[o] = fmaf(y[0], v.x, qn[o]);
                    qn[o] = fmaf(y[1], v.y, qn[o]);
                    qn[o] = fmaf(y[2], v.z, qn[o]);
                    qn[o] = fmaf(y[3], v.w, qn[o]);
                }
            }
#pragma unroll
            for (int o = 0; o < NQP; ++o) {
                q[o] = rw_group_sum(q[o]) + bias[o];
                qn[o] = rw_group_sum(qn[o]) + bias[NQP + o];
            }
            const long long ar64 = a.actions[(size_t)ri * 2], ap64 = a.actions[(size_t)ri * 2 + 1];
            const int ar = ar64 < 0 ? 0 : (ar64 >= n_rot ? n_rot - 1 : (int)ar64);
            const int apk = n_rot + (ap64 < 0 ? 0 : (ap64 >= a.d.n_ph ? a.d.n_ph - 1 : (int)ap64));
            const float rew = a.rewards[ri], live = a.dones[ri] ? 0.0f : 1.0f;
            float mr = qn[0], mp = 0.0f, qr = q[0], qp = 0.0f;
#pragma unroll
            for (int o = 1; o < NQP; ++o) {
                if (o < n_rot) mr = fmaxf(mr, qn[o]);
                if (o == n_rot) mp = qn[o];
                if (o > n_rot && o < NQ) mp = fmaxf(mp, qn[o]);
            }
#pragma unroll
            for (int o = 0; o < NQP; ++o) {
                qr = o == ar ? q[o] : qr;
                qp = o == apk ? q[o] : qp;
            }
            const float dr = qr - (rew + a.discount * mr * live), dp = qp - (rew + a.discount * mp * live);
            if (l == 0) {
                float *ri_out = info + r * RT_INFO;
                ri_out[0] = valid ? dr * a.dq_rot : 0.0f;
                ri_out[1] = valid ? dp * a.dq_ph : 0.0f;
                ri_out[2] = valid ? dr * dr : 0.0f;
                ri_out[3] = valid ? dp * dp : 0.0f;
                reinterpret_cast<int *>(ri_out)[4] = ar;
                reinterpret_cast<int *>(ri_out)[5] = apk;
                *reinterpret_cast<long long *>(ri_out + 6) = ri;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < RT_ROWS; ++rr) {
            const float *in = info + rr * RT_INFO;
            const float gr = in[0], gp = in[1];
            const int ar = reinterpret_cast<const int *>(in)[4], apk = reinterpret_cast<const int *>(in)[5];
            const size_t ri = (size_t) * reinterpret_cast<const long long *>(in + 6);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (RT_TPB * j < D) { // (uniform)
                    const int c = min(tid + RT_TPB * j, D - 1);
                    const float xo = a.states[ri * F + min(c, F - 1)], xa = a.agent_states[ri * 2 + max(c - F, 0)];
                    const float x = c < F ? xo : xa;
                    const float tr = gr * x, tp = gp * x;
#pragma unroll
                    for (int k = 0; k < NQP; ++k) acc[j][k] = acc[j][k] + (k == ar ? tr : (k == apk ? tp : 0.0f));
                }
            }
            sacc = sacc + (tid == ar ? gr : (tid == apk ? gp : 0.0f));
            lrot = lrot + in[2];
            lph = lph + in[3];
        }
        __syncthreads(); // the hand-over is free for the next rows
    }
    float *part = reinterpret_cast<float *>(a.work + a.L.partials) + (size_t)blockIdx.x * a.L.part_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = tid + RT_TPB * j;
        if (c < D) {
#pragma unroll
            for (int k = 0; k < NQP; ++k)
                if (k < NQ) part[(size_t)k * D + c] = acc[j][k];
        }
    }
    if (tid < NQ) part[(size_t)NQ * D + tid] = sacc;
    if (tid == 64) {
        part[(size_t)NQ * D + NQ] = lrot;
        part[(size_t)NQ * D + NQ + 1] = lph;
    }
}

__global__ void __launch_bounds__(RT_TPB) k_reworktrain_up(const ReworkTrainArgs a)
{
    __shared__ double vbuf[2][RW_MAX_D];
    __shared__ double s_sh;
    __shared__ float tail[3][RT_MAX_PARTS];
    const ReworkDims &d = a.d;
    const ReworkTrainLayout &L = a.L;
    const int k = blockIdx.x, tid = threadIdx.x, NQ = d.n_rot + d.n_ph, D = d.D;
    const bool rot = k < d.n_rot;
    const float *__restrict__ part = reinterpret_cast<const float *>(a.work + L.partials);
    const size_t PS = L.part_stride;
    float *G = reinterpret_cast<float *>(a.work + L.G), *S = G + (size_t)NQ * D;
    double *cur = vbuf[0], *nxt = vbuf[1];
    // s[k] and the two loss sums: the partials' values through LDS (loaded side by side), then added in workgroup order
    if (tid < L.parts) {
        tail[0][tid] = part[tid * PS + (size_t)NQ * D + k];
        tail[1][tid] = part[tid * PS + (size_t)NQ * D + NQ];
        tail[2][tid] = part[tid * PS + (size_t)NQ * D + NQ + 1];
    }
    for (int c = tid; c < D; c += RT_TPB) {
        float gsum = 0.0f;
#pragma unroll 8
        for (int w = 0; w < L.parts; ++w) gsum = gsum + part[w * PS + (size_t)k * D + c];
        G[(size_t)k * D + c] = gsum;
        cur[c] = (double)gsum;
    }
    __syncthreads();
    if (tid == RT_TPB - 1) {
        float ssum = 0.0f;
        for (int w = 0; w < L.parts; ++w) ssum = ssum + tail[0][w];
        S[k] = ssum;
        s_sh = (double)ssum;
    }
    if (k == 0 && tid == RT_TPB - 65) { // (another wave)
        float lr = 0.0f, lp = 0.0f;
        for (int w = 0; w < L.parts; ++w) {
            lr = lr + tail[1][w];
            lp = lp + tail[2][w];
        }
        *a.loss = lr * a.loss_rot + lp * a.loss_ph;
    }
    // this row of A in the other head's layers: zeros
    for (int l = 4; l < 9; ++l) {
        if (l == 7 || (l < 8) == rot) continue;
        double *A = reinterpret_cast<double *>(a.work + L.A[l]) + (size_t)k * L.out[l];
        for (int j = tid; j < L.out[l]; j += RT_TPB) A[j] = 0.0;
    }
    __syncthreads();
    const double sk = s_sh;
    const float *__restrict__ P = a.model;
    const int nlayers = rot ? 7 : 5; // layer1..4, then rotation_layer1..3 / pheromone_layer1
    for (int s = 0; s < nlayers; ++s) {
        const int l = (!rot && s == 4) ? 8 : s;
        const float *__restrict__ W = P + L.off[2 * l], *__restrict__ b = P + L.off[2 * l + 1];
        const int in = L.in[l], out = L.out[l];
        double *A = reinterpret_cast<double *>(a.work + L.A[l]) + (size_t)k * out;
        for (int j = tid; j < out; j += RT_TPB) {
            const float *__restrict__ w = W + (size_t)j * in;
            double v = 0.0;
            for (int c = 0; c < in; ++c) v = v + cur[c] * (double)w[c];
            v = v + sk * (double)b[j];
            nxt[j] = v;
            A[j] = v;
        }
        __syncthreads();
        double *t = cur;
        cur = nxt;
        nxt = t;
    }
}

__global__ void __launch_bounds__(RT_TPB) k_reworktrain_grad(const ReworkTrainArgs a)
{
    const ReworkTrainLayout &L = a.L;
    const size_t i = (size_t)blockIdx.x * RT_TPB + threadIdx.x;
    if (i >= L.off[2 * RW_LAYERS]) return;
    int t = 0;
    for (int u = 1; u < 2 * RW_LAYERS; ++u) t += i >= L.off[u] ? 1 : 0;
    const int l = t >> 1, in = L.in[l], out = L.out[l], D = a.d.D, NQ = a.d.n_rot + a.d.n_ph;
    const size_t local = i - L.off[t];
    const bool bias = t & 1;
    const int o = bias ? (int)local : (int)(local / in), c = bias ? 0 : (int)(local - (size_t)o * in);
    const double *__restrict__ M = reinterpret_cast<const double *>(a.work + L.M[l]);
    const float *__restrict__ G = reinterpret_cast<const float *>(a.work + L.G), *__restrict__ S = G + (size_t)NQ * D;
    const int src = L.src[l];
    const double *__restrict__ A = reinterpret_cast<const double *>(a.work + L.A[src < 0 ? 0 : src]);
    double v = 0.0;
    for (int k = L.k0[l]; k < L.k1[l]; ++k) {
        const double x = bias ? (double)S[k] : (src < 0 ? (double)G[(size_t)k * in + c] : A[(size_t)k * in + c]);
        v = v + M[(size_t)k * out + o] * x;
    }
    const float g = (float)v;
    if (a.grads) a.grads[i] = g;
    if (a.adam.on) adam_at(a.model, a.adam, i, g);
}

template <int NQP>
static hipError_t rt_launch_batch(const ReworkTrainArgs &a, hipStream_t st)
{
    const int Dp = (a.d.D + 63) / 64 * 64;
    const size_t lds = sizeof(float) * ((size_t)2 * NQP * Dp + 2 * NQP + RT_ROWS * RT_INFO); // <= 128.6 KiB (NQP 16, D 1024)
    if (lds > 65536) {
        const hipError_t e = antsrl_lds_optin<k_reworktrain_batch<NQP>>(lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_reworktrain_batch<NQP>), dim3(a.L.parts), dim3(RT_TPB), lds, st, a);
    return hipGetLastError();
}

hipError_t antsrl_launch_reworktrain(const ReworkTrainArgs &a, hipStream_t st)
{
    const int NQ = a.d.n_rot + a.d.n_ph;
    hipLaunchKernelGGL(k_reworktrain_down, dim3(NQ), dim3(RT_TPB), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = NQ <= 8 ? rt_launch_batch<8>(a, st) : rt_launch_batch<16>(a, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_reworktrain_up, dim3(NQ), dim3(RT_TPB), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t P = a.L.off[2 * RW_LAYERS];
    hipLaunchKernelGGL(k_reworktrain_grad, dim3((unsigned)((P + RT_TPB - 1) / RT_TPB)), dim3(RT_TPB), 0, st, a);
    return hipGetLastError();
}
