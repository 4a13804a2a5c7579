// antsrl_memnet.h — shapes and packed layout of the memory agent net (antsrl_memnet.hip), shared with the C-ABI.
// The packed layout is private to the library: antsrl_memnet_packed_bytes reports its size, nothing else of it
// crosses the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// Packed layers, in the order the kernel consumes them:
//   0 L1 (x -> h2)  1 L2 (h2 -> h3)  2 L3 (h3 -> h1)  3 L4 (h1 -> D)
//   4 R1 (g -> h2)  5 R2 (h2 -> h3)  6 R3 (h3 -> n_rot, one tile)
//   7 P1 (g -> h1)  8 P2 (h1 -> n_ph, one tile)
//   9 M1 (g -> h2) 10 M2 (h2 -> h2) 11 M3 | Fg (h2 -> two tiles: memory_layer3 rows in tile 0, forget_layer rows in tile 1)
// Each: bf16 A fragments [out tile][k-step][64 lanes][8] (1 KiB per fragment; layers fed from registers in the permuted
// k order of the accumulator, see antsrl_memnet.hip), then the fp32 bias [32 * out tiles] (zero rows past the width);
// every block starts on a 256-byte boundary.
// The fp32 pack (antsrl_memnet_f32.hip) has the same blocks, with fp32 A fragments [out tile][k-group of 8 inputs]
// [64 lanes][4] (also 1 KiB per fragment; ks counts k-groups there).
#define MN_NLAYERS 12

struct MemNetDims {
    int F, A, mem, D, h1, h2, h3, n_rot, n_ph;
};

struct MemNetLayout {
    int Dp;                       // D rounded up to 32
    int ks[MN_NLAYERS];           // k-steps of 16 inputs (bf16), k-groups of 8 inputs (fp32)
    int tout[MN_NLAYERS];         // 32-row output tiles
    size_t frag_off[MN_NLAYERS];  // byte offsets into the packed buffer
    size_t bias_off[MN_NLAYERS];
    size_t bytes;                 // total packed size
};

struct MemNetParams {
    const float *p[26]; // the 26 tensors of CollectModelMemory.state_dict(), in its order (weight, bias per layer)
};

bool antsrl_memnet_layout(const MemNetDims &d, MemNetLayout *L);
hipError_t antsrl_launch_memnet_pack(unsigned char *pack, const MemNetParams &P, const MemNetDims &d, hipStream_t st);
hipError_t antsrl_launch_memnet(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                int8_t *ph, float *q_out, hipStream_t st);
// fp32 operands (ANTSRL_MEMNET_FP32): same shapes, arguments and outputs
bool antsrl_memnet_layout_f32(const MemNetDims &d, MemNetLayout *L);
hipError_t antsrl_launch_memnet_pack_f32(unsigned char *pack, const MemNetParams &P, const MemNetDims &d, hipStream_t st);
hipError_t antsrl_launch_memnet_f32(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                    const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                    int8_t *ph, float *q_out, hipStream_t st);
// the same forwards over a device-resident list of 32-ant tiles (tiles[0 .. *n_live), see antsrl_policy_memory_tiles):
// listed tiles get what the launchers above write for their ants, bit for bit; the other ants are not written
hipError_t antsrl_launch_memnet_tiles(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                      const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                      int8_t *ph, float *q_out, const int32_t *tiles, const int32_t *n_live, hipStream_t st);
hipError_t antsrl_launch_memnet_f32_tiles(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                          const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                          int8_t *ph, float *q_out, const int32_t *tiles, const int32_t *n_live,
                                          hipStream_t st);
