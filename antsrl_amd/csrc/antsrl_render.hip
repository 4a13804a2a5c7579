// antsrl_render.hip — the episode renderer's kernels (include/antsrl.h, "The episode renderer"; antsrl_render.h holds the
// launch arguments, the tile and the colours).  RGB frames of a recorded episode straight from the recorder's block
// (antsrl_recorder.h), which is all these kernels read: the live state is not touched.
//
//   k_render_food_max   one workgroup per (frame, environment): the maximum of the uint8 food plane (the viewer divides
//                       by np.max(obj.qte) + 0.0001 per frame, visualize.py:231)
//   k_render_layer      layer_only: one thread per cell, the colour layer (the chain of mix_alpha calls,
//                       visualize.py:23-26, :220-244) as RGBA, stored along y as one dword per cell
//   k_render_frames     one workgroup per tile of TX x TY cells (TY by the zoom) of one environment of one frame:
//                         1. the cell's colour, ONCE per cell: the float64 chain, then the integer composition
//                            (background, anthill, colour layer, wall) into LDS; the grid bytes are read along y
//                         2. the ants into an LDS owner tile: a strided loop over the ants, the disc's bounding box against
//                            the tile, atomicMax of i + 1 — the highest index wins whatever the launch order, and no pixel
//                            loops over the ants
//                         3. every pixel's colour (cell, then rocks, then the owning ant) over its owner slot
//                         4. the tile's rows of pixels written along px: whole dwords, single bytes only where a row's
//                            ends are not dword aligned (3-byte pixels: a row shares a dword with the tile beside it)
//
// The float64 chain is written with one operation per statement in the association of the reference's numpy expression;
// the library is built with -ffp-contract=off and float64 division is correctly rounded, so the bytes are numpy's.
#include "antsrl_util.h"
#include "antsrl_render.h"

#define RENDER_VIEW_BACKGROUND 1
#define RENDER_VIEW_ANTS 2
#define RENDER_VIEW_EXPLORED 4
#define RENDER_VIEW_PHERO 8
#define RENDER_VIEW_FOOD 16
#define RENDER_VIEW_ROCKS 32

struct LayerState {
    double A;
    int c[3];
};

// one mix_alpha call for one cell: colour `col` at alpha `a` over the state
__device__ __forceinline__ void mix_alpha(LayerState &s, const int col0, const int col1, const int col2, const double a)
{
    const double inv = 1.0 - s.A;
    const double t = a * inv;
    const double m = s.A + t;
    const double den = m + 0.001;
    const int col[3] = {col0, col1, col2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double own = (double)s.c[k] * s.A;
        const double add = ((double)col[k] * a) * inv;
        const double v = (own + add) / den;
        s.c[k] = (int)(uint8_t)(int)v; // 0 <= v < 255: astype(np.uint8) truncates
    }
    s.A = m;
}

// the colour layer of canonical cell g of one environment's piece `fe` of a frame: R | G << 8 | B << 16 | alpha8 << 24
__device__ __forceinline__ uint32_t layer_cell(const RenderArgs &a, const unsigned char *fe, const size_t g, const int food_max)
{
    const RecorderLayout &L = a.L;
    LayerState s = {0.0, {255, 255, 255}};
    if (a.view & RENDER_VIEW_FOOD) {
        const double den = (double)food_max + 0.0001;
        const double q = (double)fe[L.fr_food + g] / den;
        mix_alpha(s, 64, 255, 64, q * 0.3);
    }
    if (a.view & RENDER_VIEW_PHERO) {
        for (int k = 0; k < L.C; ++k) {
            const double q = (double)fe[L.fr_phero + (size_t)k * L.Gp + g] / a.phero_den;
            mix_alpha(s, a.col[k][0], a.col[k][1], a.col[k][2], q * 0.6);
        }
    }
    if ((a.view & RENDER_VIEW_EXPLORED) && L.has_expl) {
        const double q = (double)(fe[L.fr_explored + g] != 0) / 1.0;
        mix_alpha(s, 255, 255, 0, q * 0.3);
    }
    const uint32_t alpha8 = (uint32_t)(uint8_t)(int)(s.A * 255.0);
    return (uint32_t)s.c[0] | (uint32_t)s.c[1] << 8 | (uint32_t)s.c[2] << 16 | alpha8 << 24;
}

__device__ __forceinline__ const unsigned char *frame_env(const RenderArgs &a, const int f, const int s)
{
    return a.block + a.L.static_bytes + (size_t)(a.first + f) * a.L.frame_bytes + (size_t)s * a.L.fr_env;
}

__global__ void __launch_bounds__(ANTSRL_RENDER_THREADS) k_render_food_max(const RenderArgs a)
{
    __shared__ int best;
    const int s = blockIdx.x % a.L.S, f = blockIdx.x / a.L.S;
    const unsigned char *food = frame_env(a, f, s) + a.L.fr_food;
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    // (a section starts 16-byte aligned and a16(G) bytes of it belong to the block: whole dwords, the tail masked)
    const size_t G = a.L.G, nq = (G + 3) / 4;
    uint32_t m = 0;
    for (size_t q = threadIdx.x; q < nq; q += ANTSRL_RENDER_THREADS) {
        uint32_t w = reinterpret_cast<const uint32_t *>(food)[q];
        const size_t left = G - 4 * q;
        if (left < 4) w &= (1u << (8 * left)) - 1u;
        const uint32_t b = max(max(w & 255u, (w >> 8) & 255u), max((w >> 16) & 255u, w >> 24));
        m = max(m, b);
    }
    if (m) atomicMax(&best, (int)m);
    __syncthreads();
    if (threadIdx.x == 0) a.fmax[blockIdx.x] = best;
}

__global__ void __launch_bounds__(ANTSRL_RENDER_THREADS) k_render_layer(const RenderArgs a)
{
    const size_t g = (size_t)blockIdx.x * ANTSRL_RENDER_THREADS + threadIdx.x;
    if (g >= a.L.G) return;
    const int s = blockIdx.y, f = blockIdx.z;
    const size_t fs = (size_t)f * a.L.S + s;
    const uint32_t v = layer_cell(a, frame_env(a, f, s), g, a.fmax[fs]);
    reinterpret_cast<uint32_t *>(a.out)[fs * a.L.G + g] = v;
}

// out = (src * alpha + dst * (255 - alpha) + 127) / 255 per channel, on colours packed R | G << 8 | B << 16
__device__ __forceinline__ uint32_t blend(const uint32_t src, const uint32_t alpha, const uint32_t dst)
{
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t sv = (src >> (8 * k)) & 255u, dv = (dst >> (8 * k)) & 255u;
        out |= ((sv * alpha + dv * (255u - alpha) + 127u) / 255u) << (8 * k);
    }
    return out;
}

__device__ __forceinline__ uint32_t rgb(const uint32_t r, const uint32_t g, const uint32_t b) { return r | g << 8 | b << 16; }

// an ant's centre in pixels: (int)(x * Z), (int)(y * Z) (the conversion saturates; the box arithmetic is 64-bit)
__device__ __forceinline__ void ant_centre(const double *xyt, const int i, const int Z, long long &cx, long long &cy)
{
    cx = (long long)(int)(xyt[3 * (size_t)i] * (double)Z);
    cy = (long long)(int)(xyt[3 * (size_t)i + 1] * (double)Z);
}

__global__ void __launch_bounds__(ANTSRL_RENDER_THREADS) k_render_frames(const RenderArgs a)
{
    extern __shared__ uint32_t lds[];
    const RecorderLayout &L = a.L;
    constexpr int TX = ANTSRL_RENDER_TX, NT = ANTSRL_RENDER_THREADS;
    const int Z = a.Z, TY = a.TY, PW = TX * Z, PH = TY * Z, npix = PW * PH;
    uint32_t *own = lds;          // [PH][PW]: the owning ant's index + 1, then the pixel's colour
    uint32_t *cellc = lds + npix; // [TY][TX]: the cell's colour
    const int tiles_x = (a.W + TX - 1) / TX;
    const int x0 = (int)(blockIdx.x % tiles_x) * TX, y0 = (int)(blockIdx.x / tiles_x) * TY;
    const int s = blockIdx.y, f = blockIdx.z;
    const size_t fs = (size_t)f * L.S + s;
    const unsigned char *fe = frame_env(a, f, s);
    const unsigned char *se = a.block + (size_t)s * L.st_env;
    const int tid = threadIdx.x;

    for (int i = tid; i < npix; i += NT) own[i] = 0;
    // ---- 1. the cells (y is the fast axis of [W][H]: neighbouring lanes read neighbouring bytes)
    for (int ci = tid; ci < TX * TY; ci += NT) {
        const int lx = ci / TY, ly = ci % TY;
        const int x = x0 + lx, y = y0 + ly;
        if (x < a.W && y < a.H) {
            const size_t g = (size_t)x * a.H + y;
            const uint32_t lay = layer_cell(a, fe, g, a.fmax[fs]);
            const bool bg = a.view & RENDER_VIEW_BACKGROUND;
            uint32_t c = bg ? rgb(ANTSRL_RENDER_DIRT_R, ANTSRL_RENDER_DIRT_G, ANTSRL_RENDER_DIRT_B) : 0u;
            if (bg) {
                const int32_t *xyr = reinterpret_cast<const int32_t *>(se + L.st_xyr);
                const long long dx = (long long)xyr[0] - x, dy = (long long)xyr[1] - y, r = xyr[2];
                if (dx * dx + dy * dy <= r * r) c = blend(rgb(0, 0, 255), ANTSRL_RENDER_ANTHILL_ALPHA, c);
            }
            c = blend(lay & 0xffffffu, lay >> 24, c);
            if (bg && se[L.st_walls + g]) c = rgb(ANTSRL_RENDER_WALL_R, ANTSRL_RENDER_WALL_G, ANTSRL_RENDER_WALL_B);
            cellc[ly * TX + lx] = c;
        }
    }
    __syncthreads();
    // ---- 2. the ants' discs into the owner tile
    const long long px0 = (long long)x0 * Z, py0 = (long long)y0 * Z;
    const long long px1 = min(px0 + PW, (long long)a.W * Z), py1 = min(py0 + PH, (long long)a.H * Z); // the tile inside the image
    const double *xyt = reinterpret_cast<const double *>(fe + L.fr_xyt);
    const long long ra = a.ra;
    if (a.view & RENDER_VIEW_ANTS) {
        for (int i = tid; i < L.N; i += NT) {
            long long cx, cy;
            ant_centre(xyt, i, Z, cx, cy);
            const long long bx0 = max(cx - ra, px0), bx1 = min(cx + ra + 1, px1);
            const long long by0 = max(cy - ra, py0), by1 = min(cy + ra + 1, py1);
            for (long long py = by0; py < by1; ++py)
                for (long long px = bx0; px < bx1; ++px) {
                    const long long dx = px - cx, dy = py - cy;
                    if (dx * dx + dy * dy <= ra * ra) atomicMax(&own[(int)(py - py0) * PW + (int)(px - px0)], (uint32_t)i + 1u);
                }
        }
    }
    __syncthreads();
    // ---- 3. every pixel's colour, over its owner slot (the thread that reads a slot is the one that writes it)
    const int wpx = (int)(px1 - px0), wpy = (int)(py1 - py0); // pixels of the tile inside the image
    const double *rc = reinterpret_cast<const double *>(fe + L.fr_rock_centers);
    const double *rw = reinterpret_cast<const double *>(se + L.st_rock_rw);
    const float *hold = reinterpret_cast<const float *>(fe + L.fr_holding);
    const unsigned char *rstate = fe + L.fr_reward_state;
    const int nrock = (a.view & RENDER_VIEW_ROCKS) ? L.R : 0;
    for (int i = tid; i < npix; i += NT) {
        const int lpx = i % PW, lpy = i / PW;
        if (lpx >= wpx || lpy >= wpy) continue;
        uint32_t c = cellc[(lpy / Z) * TX + lpx / Z];
        if (nrock) {
            const double fx = ((double)(px0 + lpx) + 0.5) / (double)Z, fy = ((double)(py0 + lpy) + 0.5) / (double)Z;
            for (int q = 0; q < nrock; ++q) {
                const double dx = fx - rc[2 * q], dy = fy - rc[2 * q + 1], rad = rw[2 * q];
                const double dx2 = dx * dx, dy2 = dy * dy;
                if (dx2 + dy2 <= rad * rad) c = rgb(ANTSRL_RENDER_ROCK_R, ANTSRL_RENDER_ROCK_G, ANTSRL_RENDER_ROCK_B);
            }
        }
        const uint32_t o = own[i];
        if (o) {
            const int ia = (int)o - 1;
            long long cx, cy;
            ant_centre(xyt, ia, Z, cx, cy);
            const long long dx = px0 + lpx - cx, dy = py0 + lpy - cy, rh = ra / 2;
            if (hold[ia] > 0.0f && dx * dx + dy * dy <= rh * rh) c = rgb(64, 255, 64);
            else {
                const double rs = (double)rstate[ia];
                const uint32_t hi = (uint32_t)(uint8_t)(int)(255.0 * rs / 255.0), lo = (uint32_t)(uint8_t)(int)(128.0 * rs / 255.0);
                c = rgb(hi, hi, lo);
            }
        }
        own[i] = c;
    }
    __syncthreads();
    // ---- 4. the rows of pixels, along px
    const size_t row_bytes = (size_t)a.W * Z * 3;
    unsigned char *img = a.out + fs * ((size_t)a.H * Z * row_bytes);
    const int len = wpx * 3;               // bytes of one of the tile's rows
    const int ndw = (len + 3) / 4 + 1;     // dwords that can hold them, whatever the row's alignment
    for (int it = tid; it < wpy * ndw; it += NT) {
        const int lpy = it / ndw, j = it % ndw;
        unsigned char *row = img + (size_t)(py0 + lpy) * row_bytes + (size_t)px0 * 3;
        const int lead = (int)((uintptr_t)row & 3); // the row starts `lead` bytes into a dword
        const int k0 = 4 * j - lead;                // this item's dword: bytes k0 .. k0 + 3 of the row
        if (k0 >= len) continue;
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = k0 + b;
            if (k < 0 || k >= len) continue;
            const int p = k / 3, ch = k - 3 * p;
            w |= ((own[lpy * PW + p] >> (8 * ch)) & 255u) << (8 * b);
        }
        if (k0 >= 0 && k0 + 4 <= len) *reinterpret_cast<uint32_t *>(row + k0) = w;
        else {
            for (int b = 0; b < 4; ++b)
                if (k0 + b >= 0 && k0 + b < len) row[k0 + b] = (unsigned char)(w >> (8 * b));
        }
    }
}

hipError_t antsrl_launch_render(const RenderArgs &a, int layer_only, hipStream_t st)
{
    const unsigned S = (unsigned)a.L.S, count = (unsigned)a.count;
    hipLaunchKernelGGL(k_render_food_max, dim3(S * count), dim3(ANTSRL_RENDER_THREADS), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (layer_only) {
        hipLaunchKernelGGL(k_render_layer, dim3((unsigned)render_layer_groups(a.L.G), S, count), dim3(ANTSRL_RENDER_THREADS), 0, st, a);
    } else {
        const size_t lds = 4 * ((size_t)ANTSRL_RENDER_TX * a.TY * (size_t)(a.Z * a.Z + 1));
        hipLaunchKernelGGL(k_render_frames, dim3((unsigned)render_tiles(a.W, a.H, a.Z), S, count), dim3(ANTSRL_RENDER_THREADS), lds, st, a);
    }
    return hipGetLastError();
}
