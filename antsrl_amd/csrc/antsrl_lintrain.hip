// antsrl_lintrain.hip — CollectAgent.train (agents/collect_agent.py:105-148) for the linear net config 5 runs, as ONE
// launch when the minibatch fits one workgroup (up to 512 rows, its 4 waves taking up to 4 tiles each: the reference's
// 264 are nine 32-row tiles) and two otherwise.  include/antsrl.h ("The linear agent's training step") holds the contract; DESIGN.md §7.11 the reasons.
//
// Stage A (k_lintrain), one wave per 32 minibatch rows.  Lane (r, h) = (lane & 31, lane >> 5) gathers row idx[r] of
// states / new_states straight from the replay arrays, 8 floats per k-step, rounds them to bf16 and multiplies them
// with layer1 exactly as the acting kernel does (k_policy_flat, antsrl_policy.hip): W1's observation columns as bf16 A
// fragments in LDS (zero for k >= F), v_mfma_f32_32x32x16_bf16 over the k-steps in ascending order from a zero
// accumulator, then  h = acc + (as0 * w1[.][F] + as1 * w1[.][F + 1]) + b1  in fp32 on bf16-rounded operands.  Equal
// operands in an equal order of MFMAs and additions: the heads are trained on the hidden values the acting kernel sees,
// bit for bit.  Everything behind that is fp32: the six head outputs of h (the model's heads), the six of h' (the live
// layer2, the target layer3), the two TD targets, dL/dq and the loss terms.  The acting kernel rounds h and the head
// weights to bf16 for its second MFMA; the training forward does NOT: the masters, the gradient and Adam are fp32, and a
// q rounded to 2^-9 relative would put more noise into q - y than a step at lr 1e-4 moves.
// The wave leaves h (with a column of ones for the biases) and dq (with the row's loss term) in its LDS tile, and lane l
// then sums outputs l, l + 64, l + 128, l + 192 of the 199 (198 gradients, the loss) over the 32 rows in row order, on
// top of what it has from its earlier tiles.  The workgroup adds its waves' sums in wave order.
// Stage B: one workgroup adds the workgroups' partials in index order (k_lintrain_finish; with one workgroup there is
// nothing to add and stage A goes on itself), writes the gradients and the loss and applies Adam (antsrl_adam.h) to the
// 198 floats.  No atomics anywhere: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_lds_optin.h"
#include "antsrl_lintrain_dev.h" // lt_epilogue, lt_lds, the LDS layout: shared with antsrl_population.hip

// One wave per SIMD (amdgpu_waves_per_eu(1, 1)): with two workgroups resident on a CU, about 1 launch in 17 at F = 294 and
// 512 workgroups left ONE workgroup's 199 partials different from every other launch's, always one of the first 256
// workgroups (the first on its CU), finite; with one wave per SIMD, 0 of 400 (profiles/dqn_launch_repeat.py; DESIGN §7.13: the mechanism is not known, the
// condition is).  Up to 256 workgroups there was one wave per SIMD anyway.
template <int NW> // waves per workgroup
__global__ void __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(1, 1))) k_lintrain(const LinTrainArgs a)
{
#include "antsrl_lintrain_body.inc"
}

__global__ void __launch_bounds__(256) k_lintrain_finish(const LinTrainArgs a, const int nblocks)
{
    if (threadIdx.x >= LT_OUT) return;
    float s = 0.0f;
    for (int b = 0; b < nblocks; ++b) s += a.batch.partials[(size_t)b * LT_PART + threadIdx.x];
    lt_epilogue(a, threadIdx.x, s);
}

// Adam alone on P floats from a flat gradient (antsrl_launch_adam, antsrl_adam.h)
__global__ void __launch_bounds__(256) k_adam_flat(float *params, const AdamArgs o, const float *grads, const int P)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < P) adam_at(params, o, p, grads[p]);
}

int antsrl_lintrain_blocks(int B, int F)
{
    (void)F;
    const int ntiles = (B + 31) / 32;
    if (ntiles <= LT_FUSED_TILES) return 1; // one workgroup: its 4 waves take up to 4 tiles each, then finish themselves
    const int blocks = (ntiles + 3) / 4;
    return blocks > LT_MAX_BLOCKS ? LT_MAX_BLOCKS : blocks;
}

hipError_t antsrl_launch_lintrain(const LinTrainArgs &a, hipStream_t st)
{
    const int blocks = antsrl_lintrain_blocks(a.batch.B, a.batch.F);
    const size_t lds = lt_lds(a.batch.ksteps, 4); // up to 91 KB at the widest rows: above 64 KiB it is an opt-in per device
    hipError_t e = antsrl_lds_optin<k_lintrain<4>>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lintrain<4>, dim3(blocks), dim3(256), lds, st, a);
    if ((e = hipGetLastError()) != hipSuccess || blocks == 1) return e;
    hipLaunchKernelGGL(k_lintrain_finish, dim3(1), dim3(256), 0, st, a, blocks);
    return hipGetLastError();
}

hipError_t antsrl_launch_adam(float *params, const AdamArgs &o, const float *grads, int P, hipStream_t st)
{
    hipLaunchKernelGGL(k_adam_flat, dim3((P + 255) / 256), dim3(256), 0, st, params, o, grads, P);
    return hipGetLastError();
}
