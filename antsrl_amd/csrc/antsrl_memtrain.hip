// antsrl_memtrain.hip — one DQN training step of the memory agent net `CollectModelMemory` on the device: what the
// reference's CollectAgentMemory.train (agents/collect_agent_memory.py:133-176) computes for a minibatch of B
// transitions, as two stages.
//
//   grad   target forward on (new_states, new_agent_states) through the trunk and both Q heads (no memory head);
//          model forward on (states, agent_states), keeping every layer output; per head
//          y = r + discount * max(q') * (1 - done) and dL/dq = 2 (q - y) / (B n_head) at the taken action, 0 elsewhere
//          (the reference's target tensor is the no-grad q with that one entry replaced, so every other entry of
//          q - target is exactly 0); loss = sum over both heads of (q_a - y)^2 / (B n_head); backward through the heads
//          into g, then L4, L3, L2, L1 with the ReLU masks; dW = sum_rows dOut^T In, db = sum_rows dOut into one flat
//          fp32 buffer of the 18 trained tensors (state_dict order).  dx is not needed.
//   apply  Adam (torch.optim.Adam's single-tensor arithmetic: m.lerp_(g, 1 - beta1), v = v beta2 + (1 - beta2) g g,
//          p += -step_size m / (sqrt(v) / sqrt(bc2) + eps)) over the flat buffer, writing the fp32 masters, m, v and the
//          bf16 operand packs the next grad stage reads.  The step size and bias corrections come from the host.
// The memory head (memory_layer1-3, forget_layer) is not in the loss: the reference leaves its .grad None and Adam skips
// it, so neither stage touches its masters (they are only ever copied, target := model).
//
// Precision contract (what tests/memory_train_ref.py::bf16_train_grads restates):
//  - MFMA operands are bf16, accumulation fp32 (v_mfma_f32_32x32x16_bf16): the forward layer inputs (x, hidden values,
//    g, head intermediates) and weights, the backward dOut operands and the saved activations of dW = dOut^T In;
//  - biases, ReLU and its mask (from the fp32 output: relu(z) > 0 exactly when z > 0), the residual with the fp32 x, the
//    TD target, dL/dq, the bias gradients (sums of the fp32 dOut), the loss and all of Adam are fp32;
//  - the masters and Adam's m / v are fp32.  Every buffer between launches is fp32; operands are rounded to bf16 as
//    they are loaded.
//
// Layout.  Every GEMM is one wave per 32 x 32 output tile (no LDS), C = A . B with A read as rows of an fp32 matrix (or
// the gathered x) and B = W^T read from a bf16 pack with k contiguous: forward C[b][o] = sum_i In[b][i] W[o][i] (pack W),
// backward data dIn[b][i] = sum_o dOut[b][o] W[o][i] (pack W^T).  The weight gradient dW[o][i] = sum_b dOut[b][o] In[b][i]
// reduces over rows: each wave owns one tile of dW over a fixed chunk of rows and writes an fp32 partial; k_mt_finalize
// sums the chunks in ascending order.  No floating-point atomics: the result is bit-identical from run to run.
//
// Launches per step: grad = 7 forward (target and model grouped) + 1 TD + 6 backward data + 1 weight gradient + 1
// finalize = 16, apply = 1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_adam.h"
#include "antsrl_memtrain.h"
#include "antsrl_memtrain_dev.h"

static inline size_t mt_al(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int mt_r32(int v) { return (v + 31) / 32 * 32; }

void antsrl_memtrain_state_layout(const MemNetDims &d, MemTrainLayout *L)
{
    const int out[MT_NP] = {d.h2, d.h3, d.h1, d.D, d.h2, d.h3, d.n_rot, d.h1, d.n_ph, d.h2, d.h2, d.mem, d.mem};
    const int in[MT_NP] = {d.D, d.h2, d.h3, d.h1, d.D, d.h2, d.h3, d.D, d.h1, d.D, d.h2, d.h2, d.h2};
    size_t off = 0, pe = 0;
    for (int l = 0; l < MT_NP; ++l) {
        L->out[l] = out[l];
        L->in[l] = in[l];
        L->poff[l] = off;
        off += (size_t)out[l] * in[l] + out[l];
        if (l == MT_NT - 1) L->trained_floats = off;
    }
    L->params_floats = off;
    for (int l = 0; l < MT_NT; ++l) {
        L->Np[l] = mt_r32(out[l]);
        L->Kp[l] = mt_r32(in[l]);
        L->woff[l] = pe;
        pe += (size_t)L->Np[l] * L->Kp[l];
        L->wtoff[l] = pe;
        pe += (size_t)L->Np[l] * L->Kp[l];
    }
    L->pack_elems = pe;
    L->m_off = mt_al(L->params_floats * 4, 256);
    L->v_off = mt_al(L->m_off + L->trained_floats * 4, 256);
    L->pack_off = mt_al(L->v_off + L->trained_floats * 4, 256);
    L->bytes = mt_al(L->pack_off + pe * 2, 256);
}

void antsrl_memtrain_work_layout(const MemNetDims &d, int B, MemTrainWork *W)
{
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    const int Bp = mt_r32(B);
    W->Bp = Bp;
    // fixed row chunks for the weight gradient: at most MT_MAXCHUNK, each a multiple of 32 rows, at least 256 rows
    int nch = (Bp + 255) / 256;
    if (nch > MT_MAXCHUNK) nch = MT_MAXCHUNK;
    W->chunk = mt_r32((Bp + nch - 1) / nch);
    W->nchunk = (Bp + W->chunk - 1) / W->chunk;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off = mt_al(off + floats, 64); return o; };
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l < MT_NT; ++l) W->act[n][l] = take((size_t)Bp * L.Np[l]);
    size_t *dout[MT_NT] = {&W->dh1, &W->dh2, &W->dh3, &W->dg, &W->dr1, &W->dr2, &W->dqr, &W->dp1, &W->dqp};
    for (int l = 0; l < MT_NT; ++l) *dout[l] = take((size_t)Bp * L.Np[l]);
    size_t pc = 0;
    for (int l = 0; l < MT_NT; ++l) {
        W->part_layer[l] = pc;
        pc += (size_t)L.Np[l] * L.Kp[l] + L.Np[l];
    }
    W->part_chunk = pc;
    W->part = take(pc * W->nchunk);
    W->nloss = (Bp + MT_TD_BLOCK - 1) / MT_TD_BLOCK;
    W->lossp = take(W->nloss);
    W->bytes = off * 4;
}

// ------------------------------------------------------------------------------------------------------------------
// kernels: the structs and the device code under them are antsrl_memtrain_dev.h's, the bodies textual includes that
// the population's kernels run too (antsrl_popmemtrain.hip)
// ------------------------------------------------------------------------------------------------------------------
// grouped GEMM, forward and backward data
__global__ void __launch_bounds__(64 * MT_WAVES) k_mt_gemm(MtGemm G)
{
    const MtAsFilled at{};
#include "antsrl_memtrain_gemm_body.inc"
}

// TD targets, dL/dq and the loss partials: one thread per row
__global__ void __launch_bounds__(MT_TD_BLOCK) k_mt_td(MtTd T)
{
#include "antsrl_memtrain_td_body.inc"
}

// weight gradients: one wave per (row chunk, 32 x 32 tile of dW); the in-tile-0 waves also sum db over their chunk
__global__ void __launch_bounds__(64 * MT_WAVES) k_mt_wgrad(MtWgrad G)
{
    const MtAsFilled at{};
#include "antsrl_memtrain_wgrad_body.inc"
}

// finalize: sum the chunk partials in ascending order into the flat gradient; the last thread sums the loss partials
__global__ void __launch_bounds__(256) k_mt_finalize(MtLayers T, const float *part, size_t part_chunk, int nchunk,
                                                     float *grads, const float *lossp, int nloss, float *loss)
{
#include "antsrl_memtrain_finalize_body.inc"
}

// apply: Adam + repack (update = 0: repack only)
__global__ void __launch_bounds__(256) k_mt_adam(MtLayers T, float *params, float *m, float *v, __bf16 *pack,
                                                 const float *grads, int update, float step_size, float bc2_sqrt,
                                                 float w1, float beta2, float w2, float eps)
{
#include "antsrl_memtrain_adam_body.inc"
}

// ------------------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------------------
MtLayers antsrl_memtrain_layers(const MemTrainLayout &L, const MemTrainWork *W)
{
    MtLayers T;
    for (int l = 0; l < MT_NT; ++l) {
        T.poff[l] = L.poff[l];
        T.woff[l] = L.woff[l];
        T.wtoff[l] = L.wtoff[l];
        T.part[l] = W ? W->part_layer[l] : 0;
        T.out[l] = L.out[l];
        T.in[l] = L.in[l];
        T.Np[l] = L.Np[l];
        T.Kp[l] = L.Kp[l];
    }
    T.trained = L.trained_floats;
    return T;
}

hipError_t antsrl_launch_memtrain_apply(const MemNetDims &d, unsigned char *state, const float *grads, float step_size,
                                        float bc2_sqrt, float w1, float beta2, float w2, float eps, hipStream_t st)
{
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    const MtLayers T = antsrl_memtrain_layers(L, nullptr);
    const unsigned blocks = (unsigned)((L.trained_floats + 255) / 256);
    hipLaunchKernelGGL(k_mt_adam, dim3(blocks), dim3(256), 0, st, T, reinterpret_cast<float *>(state),
                       reinterpret_cast<float *>(state + L.m_off), reinterpret_cast<float *>(state + L.v_off),
                       reinterpret_cast<__bf16 *>(state + L.pack_off), grads, grads ? 1 : 0, step_size, bc2_sqrt, w1, beta2,
                       w2, eps);
    return hipGetLastError();
}

hipError_t antsrl_launch_memtrain_repack(const MemNetDims &d, unsigned char *state, hipStream_t st)
{
    return antsrl_launch_memtrain_apply(d, state, nullptr, 0.0f, 1.0f, 0.1f, 0.999f, 0.001f, 1e-8f, st);
}

struct MtLaunch {
    MtGemm G;
    int tiles;
};

static void mt_add(MtLaunch &Lc, MtProb p, int Bp)
{
    p.tiles = (Bp / 32) * (p.N / 32);
    p.tile0 = Lc.tiles;
    Lc.tiles += p.tiles;
    Lc.G.p[Lc.G.np++] = p;
}

static hipError_t mt_run(MtLaunch &Lc, const MemTrainRun &run)
{
    return run.gemm(Lc.G, (unsigned)((Lc.tiles + MT_WAVES - 1) / MT_WAVES));
}

// The step's launch list, written once: which problems go into which launch, and in what order.  `run` puts each
// kernel on its stream: the single step's k_mt_* (below), or the population's k_pop_mt_* on a grid (x, P) with every
// argument as it is filled here, for member 0.
hipError_t antsrl_memtrain_grad_list(const MemNetDims &d, const unsigned char *state, const unsigned char *target,
                                     const MemTrainBatch &bt, int B, float discount, float *grads, float *loss,
                                     unsigned char *work, const MemTrainRun &run)
{
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    MemTrainWork W;
    antsrl_memtrain_work_layout(d, B, &W);
    const int Bp = W.Bp, A = d.A + d.mem;
    float *wk = reinterpret_cast<float *>(work);
    const unsigned char *net[2] = {target, state};
    const float *par[2] = {reinterpret_cast<const float *>(target), reinterpret_cast<const float *>(state)};
    auto Wp = [&](int n, int l) { return reinterpret_cast<const __bf16 *>(net[n] + L.pack_off) + L.woff[l]; };
    auto WTp = [&](int n, int l) { return reinterpret_cast<const __bf16 *>(net[n] + L.pack_off) + L.wtoff[l]; };
    auto bias = [&](int n, int l) { return par[n] + L.poff[l] + (size_t)L.out[l] * L.in[l]; };
    auto act = [&](int n, int l) { return wk + W.act[n][l]; };
    MtX X[2] = {{bt.new_states, bt.new_agent_states, bt.idx, B, d.F, A}, {bt.states, bt.agent_states, bt.idx, B, d.F, A}};
    hipError_t e;

    // forward, both nets grouped per layer: (layer, input layer or -1 for x, relu, residual)
    const int fl[7][2] = {{0, -1}, {1, -1}, {2, -1}, {3, -1}, {4, 7}, {5, 8}, {6, -1}};
    const int in_of[MT_NT] = {-1, 0, 1, 2, 3, 4, 5, 3, 7};
    for (int s = 0; s < 7; ++s) {
        MtLaunch Lc{};
        Lc.G.x[0] = X[0];
        Lc.G.x[1] = X[1];
        for (int q = 0; q < 2; ++q) {
            const int l = fl[s][q];
            if (l < 0) continue;
            for (int n = 0; n < 2; ++n) {
                MtProb p{};
                p.a = in_of[l] < 0 ? nullptr : act(n, in_of[l]);
                p.lda = in_of[l] < 0 ? 0 : L.Np[in_of[l]];
                p.xnet = n;
                p.w = Wp(n, l);
                p.ldw = L.Kp[l];
                p.K = L.Kp[l];
                p.bias = bias(n, l);
                p.nb = L.out[l];
                p.c = act(n, l);
                p.ldc = L.Np[l];
                p.N = L.Np[l];
                p.relu = l < 3;
                p.resid = l == 3;
                mt_add(Lc, p, Bp);
            }
        }
        if ((e = mt_run(Lc, run)) != hipSuccess) return e;
    }

    // TD targets and dL/dq
    {
        MtTd T;
        T.tqr = act(0, 6); T.tqp = act(0, 8); T.qr = act(1, 6); T.qp = act(1, 8);
        T.dqr = wk + W.dqr; T.dqp = wk + W.dqp;
        T.rewards = bt.rewards; T.actions = bt.actions; T.idx = bt.idx; T.dones = bt.dones;
        T.lossp = wk + W.lossp;
        T.B = B; T.n_rot = d.n_rot; T.n_ph = d.n_ph;
        T.discount = discount;
        T.norm_r = (float)(2.0 / ((double)B * d.n_rot));
        T.norm_p = (float)(2.0 / ((double)B * d.n_ph));
        T.inv_r = (float)(1.0 / ((double)B * d.n_rot));
        T.inv_p = (float)(1.0 / ((double)B * d.n_ph));
        if ((e = run.td(T, (unsigned)W.nloss)) != hipSuccess) return e;
    }

    // backward data (model): dIn = dOut . W (pack W^T), masked by the ReLU of the layer that produced In
    float *dout[MT_NT] = {wk + W.dh1, wk + W.dh2, wk + W.dh3, wk + W.dg, wk + W.dr1, wk + W.dr2, wk + W.dqr, wk + W.dp1, wk + W.dqp};
    auto bwd = [&](int l) { // dOut of layer l -> dOut of its input layer
        MtProb p{};
        const int il = in_of[l];
        p.a = dout[l]; p.lda = L.Np[l];
        p.w = WTp(1, l); p.ldw = L.Np[l]; p.K = L.Np[l];
        p.c = dout[il]; p.ldc = L.Np[il]; p.N = L.Np[il];
        p.mask = il < 3 ? act(1, il) : nullptr; p.ldm = L.Np[il];
        p.xnet = 1;
        return p;
    };
    {
        MtLaunch Lc{};
        mt_add(Lc, bwd(6), Bp); // R3 -> dr2
        mt_add(Lc, bwd(8), Bp); // P2 -> dp1
        if ((e = mt_run(Lc, run)) != hipSuccess) return e;
    }
    {
        MtLaunch Lc{};
        mt_add(Lc, bwd(5), Bp); // R2 -> dr1
        if ((e = mt_run(Lc, run)) != hipSuccess) return e;
    }
    {
        MtLaunch Lc{};
        MtProb p = bwd(4); // R1 + P1 -> dg
        p.a2 = dout[7]; p.lda2 = L.Np[7];
        p.w2 = WTp(1, 7); p.ldw2 = L.Np[7]; p.K2 = L.Np[7];
        mt_add(Lc, p, Bp);
        if ((e = mt_run(Lc, run)) != hipSuccess) return e;
    }
    for (int l = 3; l >= 1; --l) { // L4 -> dh3, L3 -> dh2, L2 -> dh1
        MtLaunch Lc{};
        mt_add(Lc, bwd(l), Bp);
        if ((e = mt_run(Lc, run)) != hipSuccess) return e;
    }

    // weight gradients: row-chunk partials
    {
        MtWgrad G{};
        G.x = X[1];
        G.part = wk + W.part;
        G.part_chunk = W.part_chunk;
        G.chunk = W.chunk;
        G.Bp = Bp;
        int tiles = 0;
        for (int l = 0; l < MT_NT; ++l) {
            MtWg &p = G.p[G.np++];
            p.dy = dout[l]; p.lddy = L.Np[l];
            p.x = in_of[l] < 0 ? nullptr : act(1, in_of[l]);
            p.ldx = in_of[l] < 0 ? 0 : L.Np[in_of[l]];
            p.Np = L.Np[l]; p.Kp = L.Kp[l];
            p.off = W.part_layer[l];
            p.tiles = (L.Np[l] / 32) * (L.Kp[l] / 32) * W.nchunk;
            p.tile0 = tiles;
            tiles += p.tiles;
        }
        if ((e = run.wgrad(G, (unsigned)((tiles + MT_WAVES - 1) / MT_WAVES))) != hipSuccess) return e;
    }
    {
        const MtLayers T = antsrl_memtrain_layers(L, &W);
        const unsigned blocks = (unsigned)((L.trained_floats + 1 + 255) / 256);
        const MtFinalize Z = {wk + W.part, W.part_chunk, W.nchunk, grads, wk + W.lossp, W.nloss, loss};
        if ((e = run.finalize(T, Z, blocks)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// the single step: the list's kernels as they are, on one stream
struct MtRunSingle final : MemTrainRun {
    hipStream_t st;
    explicit MtRunSingle(hipStream_t s) : st(s) {}
    hipError_t gemm(const MtGemm &G, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_mt_gemm, dim3(blocks), dim3(64 * MT_WAVES), 0, st, G);
        return hipGetLastError();
    }
    hipError_t td(const MtTd &T, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_mt_td, dim3(blocks), dim3(MT_TD_BLOCK), 0, st, T);
        return hipGetLastError();
    }
    hipError_t wgrad(const MtWgrad &G, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_mt_wgrad, dim3(blocks), dim3(64 * MT_WAVES), 0, st, G);
        return hipGetLastError();
    }
    hipError_t finalize(const MtLayers &T, const MtFinalize &Z, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_mt_finalize, dim3(blocks), dim3(256), 0, st, T, Z.part, Z.part_chunk, Z.nchunk, Z.grads, Z.lossp,
                           Z.nloss, Z.loss);
        return hipGetLastError();
    }
};

hipError_t antsrl_launch_memtrain_grad(const MemNetDims &d, const unsigned char *state, const unsigned char *target,
                                       const MemTrainBatch &bt, int B, float discount, float *grads, float *loss,
                                       unsigned char *work, hipStream_t st)
{
    return antsrl_memtrain_grad_list(d, state, target, bt, B, discount, grads, loss, work, MtRunSingle(st));
}
