// antsrl_popmemtrain.hip — the DQN training step of P memory nets (CollectModelMemory, antsrl_memtrain.hip) in the
// launches of one: 16 + 1 = 17 whatever P is (include/antsrl.h, "The population of memory nets"; antsrl_population.h
// holds the layout; DESIGN.md §7.29 the reasons and the measurements).
//
// As in antsrl_population.hip, each kernel is the single step's kernel with the member taken from the grid's y
// dimension: it moves the single step's arguments (filled by the host for member 0, by the ONE launch list both forms
// run, antsrl_memtrain_grad_list) to its member and then runs the SAME body text the single kernel runs, included
// inside both (antsrl_population.hip's header says why the bodies are includes and not __device__ callees):
//   k_pop_mt_gemm      antsrl_memtrain_gemm_body.inc      (k_mt_gemm)      grid (ceil(tiles / 4), P)    7 + 6 launches
//   k_pop_mt_td        antsrl_memtrain_td_body.inc        (k_mt_td)        grid (nloss, P)
//   k_pop_mt_wgrad     antsrl_memtrain_wgrad_body.inc     (k_mt_wgrad)     grid (ceil(tiles / 4), P)
//   k_pop_mt_finalize  antsrl_memtrain_finalize_body.inc  (k_mt_finalize)  grid (ceil((trained + 1) / 256), P)
//   k_pop_mt_adam      antsrl_memtrain_adam_body.inc      (k_mt_adam)      grid (ceil(trained / 256), P)
// What moves: a net's state block (masters, Adam's moments, packs) by the state stride, everything in the workspace by
// the workspace stride (both multiples of 256 bytes, the launcher refuses others: a member's blocks start as aligned as
// a single trainer's, for mt_row8's 32-byte and the packs' 16-byte loads), the ring's arrays by the member's slab, idx
// by B, grads by trained_floats, loss by 1; discount and Adam's step size come from the by-value table.
// So member p computes, bit for bit, what antsrl_memtrain_grad + antsrl_memtrain_apply compute on its own blocks, slab
// and idx row.  No atomics, no LDS beyond k_mt_td's, no scratch; no kernel reads what another member's workgroups write.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_adam.h"
#include "antsrl_memtrain.h"
#include "antsrl_memtrain_dev.h"
#include "antsrl_population.h"

// how far member p's blocks lie behind member 0's
struct PopMtStride {
    size_t state, work; // bytes: MemTrainLayout::bytes, MemTrainWork::bytes
    size_t rows;        // rows of a member's ring slab
    size_t trained;     // floats of a member's gradient
};

static_assert(sizeof(MtGemm) + sizeof(PopMtStride) <= 4096, "k_pop_mt_gemm's arguments");
static_assert(sizeof(PopTable) + sizeof(MtTd) + sizeof(PopMtStride) <= 4096, "k_pop_mt_td's arguments");
static_assert(sizeof(MtWgrad) + sizeof(PopMtStride) <= 4096, "k_pop_mt_wgrad's arguments");
static_assert(sizeof(MtLayers) + sizeof(MtFinalize) + sizeof(PopMtStride) + sizeof(PopRunningLoss) <= 4096, "k_pop_mt_finalize's arguments");
static_assert(sizeof(PopTable) + sizeof(MtLayers) + sizeof(PopMtStride) + 5 * sizeof(void *) + 6 * sizeof(float) <= 4096,
              "k_pop_mt_adam's arguments");

// p moved by `bytes`; NULL (an operand a problem does not have) stays NULL
template <class T> __device__ __forceinline__ T *pop_mt_moved(T *p, const size_t bytes)
{
    return p ? reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + bytes) : nullptr;
}

// The body's `at` for a member: an operand of member 0 as the member reads it
struct PopMtAt {
    size_t member;
    PopMtStride S;
    template <class T> __device__ __forceinline__ T *state(T *p) const { return pop_mt_moved(p, member * S.state); }
    template <class T> __device__ __forceinline__ T *work(T *p) const { return pop_mt_moved(p, member * S.work); }

    __device__ __forceinline__ MtProb operator()(const MtProb &p0) const
    {
        MtProb p = p0;
        p.w = state(p0.w); p.w2 = state(p0.w2); p.bias = state(p0.bias);
        p.a = work(p0.a); p.a2 = work(p0.a2); p.mask = work(p0.mask); p.c = work(p0.c);
        return p;
    }
    __device__ __forceinline__ MtX operator()(const MtX &x0) const
    {
        MtX x = x0;
        x.obs = x0.obs + member * S.rows * (size_t)x0.F;
        x.ag = x0.ag + member * S.rows * (size_t)x0.A;
        x.idx = x0.idx + member * (size_t)x0.B;
        return x;
    }
    __device__ __forceinline__ MtWg operator()(const MtWg &p0) const
    {
        MtWg p = p0;
        p.dy = work(p0.dy); p.x = work(p0.x);
        return p;
    }
    __device__ __forceinline__ MtTd operator()(const MtTd &t0, const PopTable &tab) const
    {
        MtTd t = t0;
        t.tqr = work(t0.tqr); t.tqp = work(t0.tqp); t.qr = work(t0.qr); t.qp = work(t0.qp);
        t.dqr = work(t0.dqr); t.dqp = work(t0.dqp); t.lossp = work(t0.lossp);
        t.rewards = t0.rewards + member * S.rows;
        t.actions = t0.actions + member * S.rows * 2;
        t.dones = t0.dones + member * S.rows;
        t.idx = t0.idx + member * (size_t)t0.B;
        t.discount = tab.m[member].discount;
        return t;
    }
};

__global__ void __launch_bounds__(64 * MT_WAVES) k_pop_mt_gemm(const MtGemm G, const PopMtStride S)
{
    const PopMtAt at = {blockIdx.y, S};
#include "antsrl_memtrain_gemm_body.inc"
}

__global__ void __launch_bounds__(MT_TD_BLOCK) k_pop_mt_td(const MtTd T0, const PopTable tab, const PopMtStride S)
{
    const PopMtAt at = {blockIdx.y, S};
    const MtTd T = at(T0, tab);
#include "antsrl_memtrain_td_body.inc"
}

__global__ void __launch_bounds__(64 * MT_WAVES) k_pop_mt_wgrad(const MtWgrad G, const PopMtStride S)
{
    const PopMtAt at = {blockIdx.y, S};
#include "antsrl_memtrain_wgrad_body.inc"
}

__global__ void __launch_bounds__(256) k_pop_mt_finalize(const MtLayers T, const MtFinalize Z, const PopMtStride S,
                                                         const PopRunningLoss rl)
{
    // the body's names, for this member
    const PopMtAt at = {blockIdx.y, S};
    const float *part = at.work(Z.part), *lossp = at.work(Z.lossp);
    const size_t part_chunk = Z.part_chunk;
    const int nchunk = Z.nchunk, nloss = Z.nloss;
    float *grads = Z.grads + at.member * S.trained, *loss = Z.loss + at.member;
#include "antsrl_memtrain_finalize_body.inc"
    // main.py:106-109 in float64, antsrl_monitor.hip's arithmetic (each product rounded before the add: the build's
    // -ffp-contract=off) and k_pop_lintrain's `first` rule, by the thread that has just written the member's loss
    if (rl.running_loss && e == T.trained) {
        const double l = (double)*loss;
        rl.running_loss[blockIdx.y] = rl.first ? l : 0.99 * rl.running_loss[blockIdx.y] + 0.01 * l;
    }
}

__global__ void __launch_bounds__(256) k_pop_mt_adam(const MtLayers T, float *params0, float *m0, float *v0, __bf16 *pack0,
                                                     const float *grads0, const PopTable tab, const PopMtStride S,
                                                     const float bc2_sqrt, const float w1, const float beta2, const float w2,
                                                     const float eps)
{
    // the body's names, for this member
    const PopMtAt at = {blockIdx.y, S};
    float *params = at.state(params0), *m = at.state(m0), *v = at.state(v0);
    __bf16 *pack = at.state(pack0);
    const float *grads = grads0 + at.member * S.trained;
    const int update = 1;
    const float step_size = tab.m[blockIdx.y].step_size;
#include "antsrl_memtrain_adam_body.inc"
}

// ------------------------------------------------------------------ launcher (antsrl_population.h)
// the list's kernels for every member: the single step's grid in x, the members in y
struct PopMtRun final : MemTrainRun {
    const PopTable &t;
    PopMtStride S;
    PopRunningLoss rl;
    unsigned P;
    hipStream_t st;
    PopMtRun(const PopTable &t_, const PopMtStride &S_, const PopRunningLoss &rl_, int P_, hipStream_t st_)
        : t(t_), S(S_), rl(rl_), P((unsigned)P_), st(st_) {}
    hipError_t gemm(const MtGemm &G, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_pop_mt_gemm, dim3(blocks, P), dim3(64 * MT_WAVES), 0, st, G, S);
        return hipGetLastError();
    }
    hipError_t td(const MtTd &T, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_pop_mt_td, dim3(blocks, P), dim3(MT_TD_BLOCK), 0, st, T, t, S);
        return hipGetLastError();
    }
    hipError_t wgrad(const MtWgrad &G, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_pop_mt_wgrad, dim3(blocks, P), dim3(64 * MT_WAVES), 0, st, G, S);
        return hipGetLastError();
    }
    hipError_t finalize(const MtLayers &T, const MtFinalize &Z, unsigned blocks) const override
    {
        hipLaunchKernelGGL(k_pop_mt_finalize, dim3(blocks, P), dim3(256), 0, st, T, Z, S, rl);
        return hipGetLastError();
    }
};

hipError_t antsrl_launch_pop_memtrain(const MemNetDims &d, unsigned char *states, const unsigned char *targets,
                                      const MemTrainBatch &bt, long long rows, int B, const PopTable &t, int P,
                                      const AdamArgs &adam, float *grads, float *loss, const PopRunningLoss &rl,
                                      unsigned char *work, hipStream_t st)
{
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    MemTrainWork W;
    antsrl_memtrain_work_layout(d, B, &W);
    // every member's blocks start as aligned as a single trainer's; idx is a population's only way to name rows
    if (P < 1 || P > ANTSRL_POP_MAX || rows < 1 || !bt.idx || L.bytes % 256 || W.bytes % 256 || ((uintptr_t)states & 255) ||
        ((uintptr_t)targets & 255) || ((uintptr_t)work & 255))
        return hipErrorInvalidValue;
    const PopMtStride S = {L.bytes, W.bytes, (size_t)rows, L.trained_floats};
    // 16 launches: the one list, filled for member 0 (the discount is the table's)
    hipError_t e = antsrl_memtrain_grad_list(d, states, targets, bt, B, 0.0f, grads, loss, work, PopMtRun(t, S, rl, P, st));
    if (e != hipSuccess) return e;
    // + 1: Adam and the repack, antsrl_launch_memtrain_apply's launch per member
    const MtLayers T = antsrl_memtrain_layers(L, nullptr);
    const unsigned blocks = (unsigned)((L.trained_floats + 255) / 256);
    hipLaunchKernelGGL(k_pop_mt_adam, dim3(blocks, (unsigned)P), dim3(256), 0, st, T, reinterpret_cast<float *>(states),
                       reinterpret_cast<float *>(states + L.m_off), reinterpret_cast<float *>(states + L.v_off),
                       reinterpret_cast<__bf16 *>(states + L.pack_off), (const float *)grads, t, S, adam.bc2_sqrt, adam.w1m,
                       adam.beta2, adam.w2m, adam.eps);
    return hipGetLastError();
}
