// antsrl_checkpoint.hip — k_env_copy: the one kernel behind antsrl_checkpoint_save / _load / antsrl_fork_envs
// (antsrl_capi.hip).  A table-driven device-to-device copy (antsrl_checkpoint.h): per array a source base, a destination
// base and a row length; whole arrays (save, load) or the rows of a list of (src env, dst env) pairs (fork).
//
// A row moves with the widest access its two addresses share: 16 bytes per lane where src and dst are congruent modulo
// 16 (every whole array: both sides are 256-byte aligned; a forked row whose length or whose environment distance is a
// multiple of 16), 4 bytes where they are congruent modulo 4 only (12-byte anthill rows, 8 N bytes with N odd), single
// bytes otherwise (`mandibles` rows of N = 33 bytes between environments an odd distance apart).  The bytes in front of
// the destination's first aligned unit and behind its last are copied one by one, so no access of any width touches a byte
// outside [row, row + bytes) on either side.  Plain loads and stores, no atomics; rows never overlap (the entries check).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_checkpoint.h"
#include "antsrl_launch.h"

static_assert(sizeof(EnvCopyTable) <= 4096, "the table is a kernel argument");

// Chunk k of the row [s, s + L) -> [d, d + L) in units of T, (s ^ d) being a multiple of sizeof(T): the units
// [k * U, (k + 1) * U) of the aligned body, U = ENV_COPY_CHUNK / sizeof(T); chunk 0 also takes the head and the tail.
// (Four loads in front of four stores, the clamped index keeping every load inside the body: k_copy16's idiom.)
template <typename T>
static __device__ __forceinline__ void copy_chunk(unsigned char *__restrict__ d, const unsigned char *__restrict__ s,
                                                  const uint64_t L, const uint32_t k)
{
    constexpr uint64_t W = sizeof(T), U = ENV_COPY_CHUNK / W;
    const uint64_t lead = (W - ((uintptr_t)d & (W - 1))) & (W - 1);
    const uint64_t head = lead < L ? lead : L;
    const uint64_t nb = (L - head) / W, tail = L - head - nb * W;
    const T *__restrict__ sp = (const T *)(s + head);
    T *__restrict__ dp = (T *)(d + head);
    const uint64_t lo = (uint64_t)k * U, hi = lo + U < nb ? lo + U : nb;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 1024) {
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = sp[min(i + (uint64_t)u * 256, hi - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + (uint64_t)u * 256 < hi) dp[i + (uint64_t)u * 256] = v[u];
    }
    if (k == 0) { // head and tail: fewer than sizeof(T) bytes each
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        if (threadIdx.x < tail) d[L - tail + threadIdx.x] = s[L - tail + threadIdx.x];
    }
}

__global__ void __launch_bounds__(256) k_env_copy(const EnvCopyTable t)
{
    const uint32_t rows = t.rows > 0 ? (uint32_t)t.rows : 1u;
    const uint64_t total = (uint64_t)rows * t.chunks_per_row;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) { // (uniform per workgroup)
        const uint32_t row = (uint32_t)(w / t.chunks_per_row), c = (uint32_t)(w % t.chunks_per_row);
        int a = 0;
        while (a + 1 < t.n_arrays && t.a[a + 1].first_chunk <= c) ++a;
        const uint64_t L = t.a[a].bytes;
        const unsigned char *s = t.a[a].src;
        unsigned char *d = t.a[a].dst;
        if (t.rows > 0) {
            s += (uint64_t)t.pair_src[row] * L;
            d += (uint64_t)t.pair_dst[row] * L;
        }
        const uint32_t k = c - t.a[a].first_chunk;
        const uintptr_t x = (uintptr_t)s ^ (uintptr_t)d;
        if ((x & 15) == 0) copy_chunk<uint4>(d, s, L, k);
        else if ((x & 3) == 0) copy_chunk<uint32_t>(d, s, L, k);
        else copy_chunk<uint8_t>(d, s, L, k);
    }
}

hipError_t antsrl_launch_env_copy(const EnvCopyTable &t, hipStream_t st)
{
    const uint64_t total = (uint64_t)(t.rows > 0 ? t.rows : 1) * t.chunks_per_row;
    if (total == 0) return hipSuccess;
    // a memory-bound copy: at most 8 workgroups per CU's worth of them, the rest of the chunks by stride
    const unsigned grid = (unsigned)(total < 2048 ? total : 2048);
    hipLaunchKernelGGL(k_env_copy, dim3(grid), dim3(256), 0, st, t);
    return hipGetLastError();
}
