// antsrl_memtrain_dev.h — what the kernels of the memory net's training step take and the device code under their
// bodies, for the single step (antsrl_memtrain.hip: k_mt_*) and the population's (antsrl_popmemtrain.hip: k_pop_mt_*).
// The bodies themselves are the textual includes antsrl_memtrain_*_body.inc, run by both forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_memtrain.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define MT_WAVES 4    // waves (independent output tiles) per workgroup
#define MT_MAXP 4     // problems per grouped GEMM launch
#define MT_MAXCHUNK 64
#define MT_TD_BLOCK 256

// ------------------------------------------------------------------------------------------------------------------
// operands
// ------------------------------------------------------------------------------------------------------------------
struct MtX { // x = cat[obs.view(F), agent_state(A)] of B minibatch rows, read through idx straight from the replay arrays
    const float *obs, *ag;
    const int64_t *idx;
    int B, F, A;
};

__device__ __forceinline__ float mt_x(const MtX &X, int b, int k)
{
    if (b >= X.B || k >= X.F + X.A) return 0.0f;
    const size_t row = X.idx ? (size_t)X.idx[b] : (size_t)b;
    return k < X.F ? X.obs[row * X.F + k] : X.ag[row * X.A + (k - X.F)];
}

__device__ __forceinline__ bf16x8 mt_row8(const float *p) // 8 consecutive fp32 (32-byte aligned) as bf16
{
    const float4 u = reinterpret_cast<const float4 *>(p)[0], v = reinterpret_cast<const float4 *>(p)[1];
    bf16x8 r;
    r[0] = (__bf16)u.x; r[1] = (__bf16)u.y; r[2] = (__bf16)u.z; r[3] = (__bf16)u.w;
    r[4] = (__bf16)v.x; r[5] = (__bf16)v.y; r[6] = (__bf16)v.z; r[7] = (__bf16)v.w;
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// grouped GEMM: forward and backward data
// ------------------------------------------------------------------------------------------------------------------
struct MtProb {
    const float *a; int lda;              // A rows [Bp][lda] fp32, or NULL: the gathered x of net `xnet`
    const __bf16 *w; int ldw; int K;      // B(k, j) = w[j * ldw + k]; K a multiple of 32
    const float *a2; int lda2;            // optional second segment, summed into the same accumulator (a2 NULL: none)
    const __bf16 *w2; int ldw2; int K2;
    const float *bias; int nb;            // fp32 bias of the nb real columns, or NULL
    const float *mask; int ldm;           // output *= (mask > 0), or NULL
    float *c; int ldc; int N;             // output [Bp][ldc], N columns (a multiple of 32)
    int relu, resid, xnet;                // relu; add the fp32 x of net xnet (the residual); which x feeds A
    int tiles, tile0;
};
struct MtGemm {
    MtProb p[MT_MAXP];
    MtX x[2]; // 0: target rows (new_states, new_agent_states), 1: model rows (states, agent_states)
    int np;
};

__device__ __forceinline__ f32x16 mt_segment(f32x16 acc, const float *a, int lda, const MtX *X, const __bf16 *w, int ldw,
                                             int K, int arow, int bcol, int h)
{
    const __bf16 *wp = w + (size_t)bcol * ldw + 8 * h;
    if (a) {
        const float *ap = a + (size_t)arow * lda + 8 * h;
        for (int k0 = 0; k0 < K; k0 += 16)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mt_row8(ap + k0), *reinterpret_cast<const bf16x8 *>(wp + k0), acc, 0, 0, 0);
    } else {
        for (int k0 = 0; k0 < K; k0 += 16) {
            bf16x8 av;
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = (__bf16)mt_x(*X, arow, k0 + 8 * h + j);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, *reinterpret_cast<const bf16x8 *>(wp + k0), acc, 0, 0, 0);
        }
    }
    return acc;
}

// ------------------------------------------------------------------------------------------------------------------
// TD targets, dL/dq and the loss partials: one thread per row
// ------------------------------------------------------------------------------------------------------------------
struct MtTd {
    const float *tqr, *tqp, *qr, *qp; // target / model head outputs [Bp][32]
    float *dqr, *dqp;                 // [Bp][32]
    const float *rewards;
    const int64_t *actions, *idx;
    const uint8_t *dones;
    float *lossp;
    int B, n_rot, n_ph;
    float discount, norm_r, norm_p, inv_r, inv_p; // norm = 2 / (B n_head), inv = 1 / (B n_head)
};

__device__ __forceinline__ float mt_max(const float *q, int n)
{
    float m = q[0];
    for (int k = 1; k < n; ++k) m = q[k] > m ? q[k] : m;
    return m;
}

// ------------------------------------------------------------------------------------------------------------------
// weight gradients: one wave per (row chunk, 32 x 32 tile of dW); the in-tile-0 waves also sum db over their chunk
// ------------------------------------------------------------------------------------------------------------------
struct MtWg {
    const float *dy; int lddy;  // dOut [Bp][lddy]
    const float *x; int ldx;    // In [Bp][ldx], or NULL: the gathered model x
    int Np, Kp;
    size_t off;                 // this layer's block in a chunk's partials
    int tiles, tile0;           // (Np / 32) (Kp / 32) nchunk
};
struct MtWgrad {
    MtWg p[MT_NT];
    MtX x;
    float *part;
    size_t part_chunk;
    int chunk, Bp, np;
};

// ------------------------------------------------------------------------------------------------------------------
// finalize and apply
// ------------------------------------------------------------------------------------------------------------------
struct MtLayers { // the trained layers' place in the flat buffer and in the partials / packs
    size_t poff[MT_NT], woff[MT_NT], wtoff[MT_NT], part[MT_NT];
    int out[MT_NT], in[MT_NT], Np[MT_NT], Kp[MT_NT];
    size_t trained;
};

__device__ __forceinline__ int mt_layer_of(const MtLayers &T, size_t e)
{
    int l = 0;
#pragma unroll
    for (int i = 1; i < MT_NT; ++i) l = e >= T.poff[i] ? i : l;
    return l;
}

// The single step's kernels read their operands as the host filled them.  A body names an operand through `at`
// (at(G.p[i]), at(G.x[n])): this one for k_mt_gemm and k_mt_wgrad, a population's member for k_pop_mt_*.
struct MtAsFilled {
    template <class T> __device__ __forceinline__ const T &operator()(const T &v) const { return v; }
    __device__ __forceinline__ float *work(float *p) const { return p; }
};

// the trained layers of a layout (W: with the partials' places, or NULL for the apply stage)
MtLayers antsrl_memtrain_layers(const MemTrainLayout &L, const MemTrainWork *W);
