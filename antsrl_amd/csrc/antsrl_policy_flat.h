// antsrl_policy_flat.h — what the two kernels that run the linear net's flat-stream acting form share around its body:
// k_policy_flat (antsrl_policy.hip: one net over the whole batch) and k_pop_policy (antsrl_population.hip: one net per
// member of a population, the member taken from the grid).  The body itself — the W1 staging, the tile image, the order
// of the MFMAs and of the additions — is ONE text, antsrl_policy_flat_body.inc, included inside both kernels, so the two
// give equal bits for equal rows and weights; here are its types, its LDS sizes and the wave hand-off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) uint32_t stream4u;

#define POL_HIDDEN 32
#define POL_MAX_KSTEPS 64 // (F + 2) <= 1024 inputs: W1 as bf16 fits 64 KiB of LDS
#define POL_FLAT_THREADS 128 // two waves per workgroup, each with a tile image of its own

__device__ __forceinline__ void pol_wave_sync()
{
    // LDS hand-off inside one wave: its LDS instructions execute in order, only the compiler must not reorder
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the flat form's LDS image per wave (bf16 elements) and its dynamic LDS: W1's observation columns + two images
static inline int pol_flat_tile_elems(int F) { return (32 * F + 32 + 7) / 8 * 8; }
static inline size_t pol_flat_lds(int F)
{
    const int ks = (F + 15) / 16;
    return (size_t)POL_HIDDEN * (16 * ks + 8) * 2 + 2 * (size_t)pol_flat_tile_elems(F) * 2;
}
// whether the flat form takes rows of F elements at all (else antsrl_launch_policy falls back to k_policy_mlp)
static inline bool pol_flat_fits(int F) { return (F + 15) / 16 <= POL_MAX_KSTEPS && pol_flat_lds(F) <= 160 * 1024; }
