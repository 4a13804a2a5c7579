// antsrl_memtrain.h — the on-device DQN training step of the memory agent net (antsrl_memtrain.hip), shared with the
// C-ABI.  The net's dimensions are antsrl_memnet.h's MemNetDims (D = F + A + mem, A = agent_dim).
//
// A net's STATE is one device buffer (256-byte aligned), antsrl_memtrain_state_layout:
//   params  fp32, the 26 tensors of CollectModelMemory.state_dict() in its order, each dense ([out][in], then [out])
//   m, v    fp32, Adam's moments of the 18 TRAINED tensors (the first 18 of the state_dict: layer1-4,
//           rotation_layer1-3, pheromone_layer1-2, each weight then bias), in that order
//   packs   bf16 MFMA operand form of the 9 trained layers: per layer W [Np][Kp] then W^T [Kp][Np]
//           (Np = out rounded up to 32, Kp = in rounded up to 32, zero padding)
// The memory head (memory_layer1-3, forget_layer) is never trained: its masters are kept bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "antsrl_fail.h"
#include "antsrl_memnet.h"

#define MT_NT 9   // trained layers: L1 L2 L3 L4 R1 R2 R3 P1 P2 (state_dict order)
#define MT_NP 13  // all layers of the state_dict

struct MemTrainLayout {
    int out[MT_NP], in[MT_NP];          // real widths, state_dict order
    size_t poff[MT_NP];                 // float offset of layer l's weight in params (its bias follows it)
    size_t params_floats, trained_floats;
    int Np[MT_NT], Kp[MT_NT];           // padded widths of the trained layers
    size_t woff[MT_NT], wtoff[MT_NT];   // bf16 element offsets of W and W^T in the packs
    size_t pack_elems;
    size_t m_off, v_off, pack_off, bytes; // byte offsets in the state buffer, total bytes
};

// Workspace of a grad stage for B rows (float offsets): fp32 activations and output gradients ([Bp][width],
// Bp = B rounded up to 32), the row-chunk weight-gradient partials and the per-block loss partials.
struct MemTrainWork {
    int Bp, nchunk, chunk;    // padded rows, row chunks of the weight-gradient reduction, rows per chunk
    size_t act[2][9];         // per net (0 target, 1 model): h1 h2 h3 g r1 r2 qr p1 qp
    size_t dqr, dqp, dr2, dr1, dp1, dg, dh3, dh2, dh1; // output gradients (model only)
    size_t part;              // weight-gradient partials: [nchunk][part_chunk]
    size_t part_layer[MT_NT]; // layer l's block in one chunk: [Np][Kp] weight, then [Np] bias
    size_t part_chunk;
    size_t lossp;             // per-block loss partials
    int nloss;
    size_t bytes;
};

void antsrl_memtrain_state_layout(const MemNetDims &d, MemTrainLayout *L);
void antsrl_memtrain_work_layout(const MemNetDims &d, int B, MemTrainWork *W);

struct MemTrainBatch {
    const float *states, *agent_states, *rewards, *new_states, *new_agent_states;
    const int64_t *actions, *idx; // actions [N][2] (rotation index, pheromone index); idx [B] or NULL (rows 0..B-1)
    const uint8_t *dones;         // bool [N]
};

#define MT_MAX_B (1 << 24) // rows of a minibatch

// The grad stage's launch list (7 forward, TD, 6 backward data, weight gradient, finalize: 16 launches) is written once,
// antsrl_memtrain_grad_list, and run by both forms of the step through a MemTrainRun: the single step's puts k_mt_* on
// its stream, the population's (antsrl_popmemtrain.hip) k_pop_mt_* on a grid (blocks, P).  The kernels' argument structs
// are antsrl_memtrain_dev.h's.
struct MtGemm;
struct MtTd;
struct MtWgrad;
struct MtLayers;
struct MtFinalize { // k_mt_finalize's arguments behind the layers
    const float *part;
    size_t part_chunk;
    int nchunk;
    float *grads;
    const float *lossp;
    int nloss;
    float *loss;
};
struct MemTrainRun { // blocks: the grid's x dimension
    virtual hipError_t gemm(const MtGemm &G, unsigned blocks) const = 0;
    virtual hipError_t td(const MtTd &T, unsigned blocks) const = 0;
    virtual hipError_t wgrad(const MtWgrad &G, unsigned blocks) const = 0;
    virtual hipError_t finalize(const MtLayers &T, const MtFinalize &Z, unsigned blocks) const = 0;

protected:
    ~MemTrainRun() = default;
};
hipError_t antsrl_memtrain_grad_list(const MemNetDims &d, const unsigned char *state, const unsigned char *target,
                                     const MemTrainBatch &b, int B, float discount, float *grads, float *loss,
                                     unsigned char *work, const MemTrainRun &run);

// the shape's rules of every entry of the net (antsrl_memapi.hip), for an entry elsewhere: *d, or the refusal under `who`
ANTSRL_INTERNAL int antsrl_memnet_dims(const char *who, const AntsMemNetShape *s, MemNetDims *d);
// ... and the precision's: ANTSRL_MEMNET_BF16 or ANTSRL_MEMNET_FP32, anything else refused as the _ex entries refuse it
ANTSRL_INTERNAL int antsrl_memnet_precision(const char *who, int precision);

hipError_t antsrl_launch_memtrain_repack(const MemNetDims &d, unsigned char *state, hipStream_t st);
hipError_t antsrl_launch_memtrain_grad(const MemNetDims &d, const unsigned char *state, const unsigned char *target,
                                       const MemTrainBatch &b, int B, float discount, float *grads, float *loss,
                                       unsigned char *work, hipStream_t st);
// grads NULL: repack only (the bf16 packs from the masters).  w1 = 1 - beta1 and w2 = 1 - beta2 as the host rounds them.
hipError_t antsrl_launch_memtrain_apply(const MemNetDims &d, unsigned char *state, const float *grads, float step_size,
                                        float bc2_sqrt, float w1, float beta2, float w2, float eps, hipStream_t st);
