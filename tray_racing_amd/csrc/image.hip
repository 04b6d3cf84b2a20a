// image.hip - gfx950 (MI355X, wave64) image passes after the walk (include/trx.h, "the frame's image"): the edge-aware
// filter over the AO visibility pass's counts, the edge-aware upsample of the sparse pass's counts and the shading of a
// frame's records to RGBA8.  A translation unit of its
// own: nothing here is seen by kernels.hip, whose instructions stay what they were.
//
// Arithmetic contract (DESIGN.md "Numerics"): binary32, no contraction, IEEE divide, dot = (ax*bx + ay*by) + az*bz.  The
// filter compares in float and sums in integers, the shade divides once and then only compares, so a host twin
// (tests/image_twin.py) gives the same bits; the heat map is a fixed sequence of such operations (tests/heat_twin.py), and so
// is a level of the value filter over float planes (k_atrous, tests/value_filter_twin.py) and the upsample of a low-grid float plane (k_plane_upsample, tests/indirect_sparse_twin.py).
#include "image.h"

#pragma clang fp contract(off)

namespace trx {
namespace {

#define TRX_F32_MAX 3.402823466e+38f
#define TRX_INVALID 0xFFFFFFFFu

constexpr uint32_t kNotSurface = 0xFFFFFFFFu; // a cell's count word in LDS: outside the image, or no surface there

// The edge-aware AO filter (trx_ao_filter_dev).  One workgroup per 32 x 8 pixel tile; lane l of the workgroup is pixel
// (l & 31, l >> 5) of the tile, so a wave is two rows of 32 pixels: its global loads and its store are two runs of
// consecutive records, and its LDS reads are - per 32-lane half, the unit ds_read_b32 banks over - 32 consecutive
// dwords of one row, conflict-free whatever the row pitch (32 + 2 * radius dwords).
//   phase 1: the (32 + 2r) x (8 + 2r) cells of the tile and its halo into LDS as separate arrays (depth, count word and,
// with normals, three components): every input pixel is read from memory once per workgroup.  A cell outside the image
// or without a surface gets kNotSurface and no further loads - its count and normal are never looked at.
//   phase 2: every lane walks its (2r + 1)^2 window out of LDS.  At r = 4 with normals that is 81 x 5 LDS reads per
// pixel against 33 B from memory; the pass is bound by the LDS there and by memory at small radii.
// 12.8 KB of LDS per workgroup with normals, 5.1 KB without.
template <bool NORMALS>
__global__ void __launch_bounds__(256) k_ao_filter(const AoFilterParams P) {
    __shared__ float s_t[kFilterMaxCells];
    __shared__ uint32_t s_cnt[kFilterMaxCells];
    __shared__ float s_n[NORMALS ? 3 * kFilterMaxCells : 1];
    const uint32_t r = P.radius;
    const uint32_t hw = kFilterTileW + 2u * r, hh = kFilterTileH + 2u * r, cells = hw * hh;
    const uint32_t tiles_x = (P.width + kFilterTileW - 1u) / kFilterTileW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = (int)(tx * kFilterTileW) - (int)r, y0 = (int)(ty * kFilterTileH) - (int)r;
    for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
        const uint32_t cy = c / hw, cx = c - cy * hw;
        const int gx = x0 + (int)cx, gy = y0 + (int)cy;
        float t = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        uint32_t cnt = kNotSurface;
        if (gx >= 0 && gy >= 0 && (uint32_t)gx < P.width && (uint32_t)gy < P.height) {
            const size_t i = (size_t)gy * P.width + (uint32_t)gx;
            const trx_hit h = P.primary[i];
            if (h.t < TRX_F32_MAX && h.prim != TRX_INVALID) {
                t = h.t;
                cnt = P.counts[i];
                if constexpr (NORMALS) {
                    const float *n = P.attr[i].normal;
                    nx = n[0]; ny = n[1]; nz = n[2];
                }
            }
        }
        s_t[c] = t;
        s_cnt[c] = cnt;
        if constexpr (NORMALS) {
            s_n[c] = nx;
            s_n[kFilterMaxCells + c] = ny;
            s_n[2u * kFilterMaxCells + c] = nz;
        }
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
    const uint32_t px = tx * kFilterTileW + lx, py = ty * kFilterTileH + ly;
    if (px >= P.width || py >= P.height) return;
    const uint32_t c0 = (ly + r) * hw + lx + r;
    trx_ao_term out;
    out.unoccluded = 0;
    out.samples = 0;
    if (s_cnt[c0] != kNotSurface) {
        const float tp = s_t[c0], tol = P.depth_tol * tp;
        float npx = 0.0f, npy = 0.0f, npz = 0.0f;
        if constexpr (NORMALS) {
            npx = s_n[c0]; npy = s_n[kFilterMaxCells + c0]; npz = s_n[2u * kFilterMaxCells + c0];
        }
        uint32_t sum = 0u, accepted = 0u;
        for (uint32_t dy = 0; dy <= 2u * r; dy++) {
            const uint32_t row = (ly + dy) * hw + lx;
            for (uint32_t dx = 0; dx <= 2u * r; dx++) {
                const uint32_t c = row + dx;
                const uint32_t cq = s_cnt[c];
                bool ok = cq != kNotSurface && __builtin_fabsf(s_t[c] - tp) <= tol;
                if constexpr (NORMALS)
                    ok = ok && (npx * s_n[c] + npy * s_n[kFilterMaxCells + c]) + npz * s_n[2u * kFilterMaxCells + c] >= P.normal_cos;
                ok = ok || c == c0;
                sum += ok ? cq : 0u;
                accepted += ok ? 1u : 0u;
            }
        }
        out.unoccluded = (uint16_t)sum;
        out.samples = (uint16_t)(P.n_samples * accepted);
    }
    P.out[(size_t)py * P.width + px] = out;
}

// The edge-aware upsample of the sparse visibility pass's counts (trx_ao_upsample_dev; the rules are stated in include/trx.h).
// The filter's shape: one workgroup per 32 x 8 tile of full-resolution pixels, lane l is pixel (l & 31, l >> 5).
//   phase 1: the low cells under the tile - columns (32 tx) / s .. (32 tx + 31) / s, rows likewise - and a halo of r cells
// into LDS as separate arrays (depth, count word, three normal components).  A cell's depth and normal are the
// full-resolution records of its pixel (X s + px0, Y s + py0), a gather at a pitch of s records; its count is the low
// grid's byte.  A cell outside the low grid, whose pixel is outside the image, or without a surface gets kNotSurface.
// At most kUpsampleMaxCells cells (image.h): 8.6 KB with normals, 3.5 KB without.
//   phase 2: every lane reads its own pixel's depth and normal from memory (consecutive records) and walks the (2r + 1)^2
// cells around cell (x / s, y / s) out of LDS.  A 32-lane half is one row of pixels and reads, per window step, the dwords
// row * pitch + x / s + const: s neighbouring lanes name the same dword (one broadcast), the distinct dwords are at most 32
// CONSECUTIVE ones, and ds_read_b32 banks a half over (address / 4) mod 32 - so no two distinct dwords of a half share a
// bank, whatever the row pitch (it is 8 .. 36 dwords here) and whatever s.
template <bool NORMALS>
__global__ void __launch_bounds__(256) k_ao_upsample(const AoUpsampleParams P) {
    __shared__ float s_t[kUpsampleMaxCells];
    __shared__ uint32_t s_cnt[kUpsampleMaxCells];
    __shared__ float s_n[NORMALS ? 3 * kUpsampleMaxCells : 1];
    const uint32_t r = P.radius, st = P.stride;
    const uint32_t tiles_x = (P.width + kFilterTileW - 1u) / kFilterTileW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t cx_first = (tx * kFilterTileW) / st, cy_first = (ty * kFilterTileH) / st;
    const uint32_t hw = (tx * kFilterTileW + kFilterTileW - 1u) / st - cx_first + 1u + 2u * r;
    const uint32_t hh = (ty * kFilterTileH + kFilterTileH - 1u) / st - cy_first + 1u + 2u * r;
    const uint32_t cells = hw * hh; // <= kUpsampleMaxCells for st >= 1, r <= kUpsampleMaxRadius (image.h)
    const int x0 = (int)cx_first - (int)r, y0 = (int)cy_first - (int)r;
    for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
        const uint32_t cy = c / hw, cx = c - cy * hw;
        const int X = x0 + (int)cx, Y = y0 + (int)cy;
        float t = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        uint32_t cnt = kNotSurface;
        if (X >= 0 && Y >= 0 && (uint32_t)X < P.lo_width && (uint32_t)Y < P.lo_height) {
            const uint32_t gx = (uint32_t)X * st + P.px0, gy = (uint32_t)Y * st + P.py0;
            if (gx < P.width && gy < P.height) {
                const size_t i = (size_t)gy * P.width + gx;
                const trx_hit h = P.primary[i];
                if (h.t < TRX_F32_MAX && h.prim != TRX_INVALID) {
                    t = h.t;
                    cnt = P.counts_lo[(size_t)Y * P.lo_width + (uint32_t)X];
                    if constexpr (NORMALS) {
                        const float *n = P.attr[i].normal;
                        nx = n[0]; ny = n[1]; nz = n[2];
                    }
                }
            }
        }
        s_t[c] = t;
        s_cnt[c] = cnt;
        if constexpr (NORMALS) {
            s_n[c] = nx;
            s_n[kUpsampleMaxCells + c] = ny;
            s_n[2u * kUpsampleMaxCells + c] = nz;
        }
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
    const uint32_t px = tx * kFilterTileW + lx, py = ty * kFilterTileH + ly;
    if (px >= P.width || py >= P.height) return;
    const size_t ip = (size_t)py * P.width + px;
    const trx_hit hp = P.primary[ip];
    trx_ao_term out;
    out.unoccluded = 0;
    out.samples = 0;
    if (hp.t < TRX_F32_MAX && hp.prim != TRX_INVALID) {
        const float tp = hp.t, tol = P.depth_tol * tp;
        float npx = 0.0f, npy = 0.0f, npz = 0.0f;
        if constexpr (NORMALS) {
            const float *n = P.attr[ip].normal;
            npx = n[0]; npy = n[1]; npz = n[2];
        }
        // the window's first cell, and the cell whose pixel is p itself (none when p is not a pixel of this phase)
        const uint32_t qx = px / st, qy = py / st;
        const uint32_t wx = qx - cx_first, wy = qy - cy_first;
        const uint32_t own = (px - qx * st == P.px0 && py - qy * st == P.py0) ? (wy + r) * hw + wx + r : kNotSurface;
        uint32_t sum = 0u, accepted = 0u, sum_all = 0u, surfaces = 0u;
        for (uint32_t dy = 0; dy <= 2u * r; dy++) {
            const uint32_t row = (wy + dy) * hw + wx;
            for (uint32_t dx = 0; dx <= 2u * r; dx++) {
                const uint32_t c = row + dx;
                const uint32_t cq = s_cnt[c];
                const bool surf = cq != kNotSurface;
                bool ok = surf && __builtin_fabsf(s_t[c] - tp) <= tol;
                if constexpr (NORMALS)
                    ok = ok && (npx * s_n[c] + npy * s_n[kUpsampleMaxCells + c]) + npz * s_n[2u * kUpsampleMaxCells + c] >= P.normal_cos;
                ok = ok || c == own;
                sum += ok ? cq : 0u;
                accepted += ok ? 1u : 0u;
                sum_all += surf ? cq : 0u;
                surfaces += surf ? 1u : 0u;
            }
        }
        // no cell accepted: every surface cell of the window (FALLBACK); none of those either: {0, 0} (EMPTY)
        if (accepted == 0u) {
            sum = sum_all;
            accepted = surfaces;
        }
        out.unoccluded = (uint16_t)sum;
        out.samples = (uint16_t)(P.n_samples * accepted);
    }
    P.out[ip] = out;
}

// Shading to RGBA8 (trx_shade_*_dev): one lane per record.  The colour is one IEEE division at most; its 8-bit code is the
// number of thresholds thr[1..255] it reaches (trx_image_code_table: the host's powf(col, 2.2f) * 255 truncated, turned
// into the smallest binary32 of every code), found in 8 steps in the workgroup's copy of the table in LDS - the device
// evaluates no pow.  NaN and negative colours reach no threshold (code 0), everything from 1 upward reaches all (255).
template <int MODE>
__global__ void __launch_bounds__(256) k_shade(const ShadeParams P) {
    __shared__ float s_thr[256];
    s_thr[threadIdx.x] = P.thr[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_items) return;
    float col = 0.0f;
    if constexpr (MODE == kShadeReference) {
        // rt_gpu_software.hlsl:130-142 / src/rt_cpu/rt_cpu.rs:57-85: 1 / t where the primary ray missed, else the AO term
        const float t = P.primary[i].t;
        if (t < TRX_F32_MAX) {
            const float at = P.ao[i].t;
            col = at < TRX_F32_MAX ? __fdiv_rn(at, 1.0f + at) : 1.0f;
        } else {
            col = __fdiv_rn(1.0f, t);
        }
    } else if constexpr (MODE == kShadeCounts) {
        const uint32_t n = P.counts[i];
        col = n == TRX_AO_NO_SURFACE ? 0.0f : __fdiv_rn((float)n, (float)P.n_samples);
    } else {
        const trx_ao_term a = P.term[i];
        col = a.samples == 0 ? 0.0f : __fdiv_rn((float)a.unoccluded, (float)a.samples);
    }
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1) c += col >= s_thr[c + step] ? step : 0u;
    reinterpret_cast<uint32_t *>(P.rgba)[i] = c * 0x00010101u | 0xFF000000u; // {c, c, c, 255}
}

// The value shade (trx_shade_value_dev, kShadeValue): k_shade's table, search and store over float values taken as they are.
// A kernel of its own name beside k_shade's three instantiations, which stay the parent commit's.
__global__ void __launch_bounds__(256) k_value(const ShadeParams P) {
    __shared__ float s_thr[256];
    s_thr[threadIdx.x] = P.thr[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_items) return;
    const float col = P.value[i];
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1) c += col >= s_thr[c + step] ? step : 0u;
    reinterpret_cast<uint32_t *>(P.rgba)[i] = c * 0x00010101u | 0xFF000000u; // {c, c, c, 255}
}

// The heat map's ten colours (include/trx.h, trx_shade_heat_dev): binary32 k / 255.0f, the division done by the compiler.
__device__ const float kHeatPalette[10][3] = {
    {0 / 255.0f, 2 / 255.0f, 91 / 255.0f},    {0 / 255.0f, 108 / 255.0f, 251 / 255.0f}, {0 / 255.0f, 221 / 255.0f, 221 / 255.0f},
    {51 / 255.0f, 221 / 255.0f, 0 / 255.0f},  {255 / 255.0f, 252 / 255.0f, 0 / 255.0f}, {255 / 255.0f, 180 / 255.0f, 0 / 255.0f},
    {255 / 255.0f, 104 / 255.0f, 0 / 255.0f}, {226 / 255.0f, 22 / 255.0f, 0 / 255.0f},  {191 / 255.0f, 0 / 255.0f, 83 / 255.0f},
    {145 / 255.0f, 0 / 255.0f, 65 / 255.0f}};

// S(a, b, v) of the rule: q = clamp((v - a) / (b - a), 0, 1), (q * q) * (3 - 2 * q)
__device__ __forceinline__ float heat_step(float a, float b, float v) {
    const float q = fminf(fmaxf(__fdiv_rn(v - a, b - a), 0.0f), 1.0f);
    return (q * q) * (3.0f - 2.0f * q);
}

// The PROFILE_RT heat map (trx_shade_heat_dev; the rule is stated in include/trx.h): a record's count, scaled, picks one of
// ten colours and blends it with its two neighbours.  Each operation is one binary32 operation of the rule, in its order -
// tests/heat_twin.py evaluates the same ones in numpy and the bytes are compared for every count there is.
__global__ void __launch_bounds__(256) k_heat(const HeatParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_items) return;
    const trx_ray_cost rc = P.cost[i];
    const float x = (P.which == TRX_HEAT_NODES ? (float)(8u * (uint32_t)rc.n_node) : (float)rc.n_tri) * P.scale;
    const float s = x * 10.0f;
    const int cur = s >= 9.0f ? 9 : (int)s; // min((int)s, 9), also where s is beyond the integers (s is never NaN or negative)
    const int prv = cur > 0 ? cur - 1 : 0, nxt = cur < 9 ? cur + 1 : 9;
    const float c = (float)cur;
    const float lo = heat_step(c - 0.8f, c + 0.8f, s);
    const float hi = heat_step((c + 1.0f) - 0.8f, (c + 1.0f) + 0.8f, s);
    const float wc = lo * (1.0f - hi), wp = 1.0f - lo, wn = hi;
    uint32_t px = 0xFF000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float r = (wc * kHeatPalette[cur][ch] + wp * kHeatPalette[prv][ch]) + wn * kHeatPalette[nxt][ch];
        r = fminf(fmaxf(r, 0.0f), 1.0f);
        px |= (uint32_t)(uint8_t)floorf(r * 255.0f + 0.5f) << (8 * ch);
    }
    reinterpret_cast<uint32_t *>(P.rgba)[i] = px;
}

// One level of the value filter (trx_value_filter_dev; the rules are stated in include/trx.h): the 5 x 5 B3-spline kernel
// with its taps s = P.spacing pixels apart, every tap under the AO filter's acceptance rule.  A level couples only pixels of
// one residue class in y mod s (and x mod s), so the workgroup is not a pixel-space tile - its halo of 2s would be 32
// pixels deep at s = 16 - but 32 consecutive x of 8 LATTICE rows y0 + k * s of one row class; lane l is pixel
// (32 tx + (l & 31), y0 + (l >> 5) * s), a wave two lattice rows of 32 pixels.
//   phase 1: those rows, two lattice rows above and below and 2s columns either side - (32 + 4s) x 12 cells - into LDS as
// separate arrays (depth, value, three normal components), k_ao_filter's layout.  A cell is a run element of one image row, so
// the global loads are whole runs of consecutive records at every level.  A cell outside the image or without a surface gets
// the depth +inf - "no tap" - and loads nothing further.
//   phase 2: every lane visits its 25 taps in the stated order out of LDS, cell (row + dy) * pitch + x + dx * s: per 32-lane
// half, the unit ds_read_b32 banks over, 32 consecutive dwords of one row - conflict-free whatever the pitch and the spacing.
// The sums are the rule's operations one by one (contraction is off in this file); a skipped tap leaves num and den as they
// are.  The last level adds the pixel's base, read by the lane that then writes the value: d_base may be d_out.
template <bool NORMALS>
__global__ void __launch_bounds__(256) k_atrous(const AtrousParams P) {
    __shared__ float s_t[kAtrousMaxCells];
    __shared__ float s_v[kAtrousMaxCells];
    __shared__ float s_n[NORMALS ? 3 * kAtrousMaxCells : 1];
    const uint32_t s = P.spacing; // 1 .. kAtrousMaxSpacing (launch_atrous)
    const uint32_t hw = kAtrousTileW + 4u * s, cells = hw * kAtrousRows; // <= kAtrousMaxCells
    const uint32_t tiles_x = (P.width + kAtrousTileW - 1u) / kAtrousTileW;
    const uint32_t classes = s < P.height ? s : P.height; // row classes that hold a row
    const uint32_t rest = blockIdx.x / tiles_x, tx = blockIdx.x - rest * tiles_x;
    const uint32_t grp = rest / classes, cls = rest - grp * classes;
    const uint64_t y0 = (uint64_t)cls + (uint64_t)grp * (kAtrousTileRows * s);
    if (y0 >= P.height) return; // (a class with fewer groups of rows than the fullest one: the whole workgroup leaves)
    const int64_t x_first = (int64_t)(tx * kAtrousTileW) - (int64_t)(2u * s);
    for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
        const uint32_t cy = c / hw, cx = c - cy * hw;
        const int64_t gx = x_first + (int64_t)cx, gy = (int64_t)y0 + ((int64_t)cy - 2) * (int64_t)s;
        float t = __builtin_inff(), v = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (gx >= 0 && gy >= 0 && gx < (int64_t)P.width && gy < (int64_t)P.height) {
            const size_t i = (size_t)gy * P.width + (size_t)gx;
            const trx_hit h = P.primary[i];
            if (h.t < TRX_F32_MAX && h.prim != TRX_INVALID) {
                t = h.t;
                v = P.in[i];
                if constexpr (NORMALS) {
                    const float *n = P.attr[i].normal;
                    nx = n[0]; ny = n[1]; nz = n[2];
                }
            }
        }
        s_t[c] = t;
        s_v[c] = v;
        if constexpr (NORMALS) {
            s_n[c] = nx;
            s_n[kAtrousMaxCells + c] = ny;
            s_n[2u * kAtrousMaxCells + c] = nz;
        }
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
    const uint32_t px = tx * kAtrousTileW + lx;
    const uint64_t py = y0 + (uint64_t)ly * s;
    if (px >= P.width || py >= P.height) return;
    const size_t ip = (size_t)py * P.width + px;
    const uint32_t c0 = (ly + 2u) * hw + lx + 2u * s;
    const float tp = s_t[c0];
    const bool with_base = P.last != 0u && P.base != nullptr;
    if (!(tp < TRX_F32_MAX)) { // no surface: the plane's own bits - at the last level the base's - copied
        const uint32_t *src = reinterpret_cast<const uint32_t *>(with_base ? P.base : P.in);
        const uint32_t bits = src[ip];
        reinterpret_cast<uint32_t *>(P.out)[ip] = bits;
        return;
    }
    const float tol = P.depth_tol * tp;
    float npx = 0.0f, npy = 0.0f, npz = 0.0f;
    if constexpr (NORMALS) {
        npx = s_n[c0]; npy = s_n[kAtrousMaxCells + c0]; npz = s_n[2u * kAtrousMaxCells + c0];
    }
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (uint32_t dy = 0; dy < 5u; dy++) {
        const uint32_t row = (ly + dy) * hw + lx;
#pragma unroll
        for (uint32_t dx = 0; dx < 5u; dx++) {
            constexpr uint32_t k[5] = {1u, 4u, 6u, 4u, 1u};
            const float w = (float)(k[dy] * k[dx]);
            const uint32_t c = row + dx * s;
            const float tq = s_t[c];
            bool ok = tq < TRX_F32_MAX && __builtin_fabsf(tq - tp) <= tol;
            if constexpr (NORMALS)
                ok = ok && (npx * s_n[c] + npy * s_n[kAtrousMaxCells + c]) + npz * s_n[2u * kAtrousMaxCells + c] >= P.normal_cos;
            ok = ok || (dy == 2u && dx == 2u);
            const float term = w * s_v[c];
            num = ok ? num + term : num;
            den = ok ? den + w : den;
        }
    }
    float f = __fdiv_rn(num, den);
    if (with_base) f = P.base[ip] + f;
    P.out[ip] = f;
}

// The edge-aware upsample of a low grid of floats (trx_value_upsample_dev; the rules are stated in include/trx.h): what
// k_ao_upsample is to the sparse visibility pass's counts, for the sparse indirect pass's values.  Its shape, tile, cells
// and window: one workgroup per 32 x 8 tile of full-resolution pixels, lane l is pixel (l & 31, l >> 5).
//   phase 1: the low cells under the tile and a halo of r cells into LDS as separate arrays (depth, value, three normal
// components).  A cell's depth and normal are the full-resolution records of its pixel (X s + px0, Y s + py0); its value is
// the low grid's float.  A cell outside the low grid, whose pixel is outside the image, or without a surface gets the depth
// +inf - "no cell" - and the value 0, and loads nothing further.  At most kUpsampleMaxCells cells: 8 640 B with normals,
// 3 456 B without.
//   phase 2: every lane reads its own pixel's depth and normal from memory (consecutive records) and walks the (2r + 1)^2
// cells around cell (x / s, y / s) out of LDS in the stated order.  k_ao_upsample's reads, so its argument holds: a 32-lane
// half is one row of pixels and reads, per window step, the dwords row * pitch + x / s + const - s neighbouring lanes name
// the same dword (one broadcast), the distinct ones are at most 32 CONSECUTIVE dwords, and ds_read_b32 banks a half over
// (address / 4) mod 32: conflict-free whatever the pitch (8 .. 36 dwords) and whatever s.
// Two pairs of sums run side by side - over the accepted cells and over all surface cells (FALLBACK) - each the rule's
// operations one by one (contraction is off in this file); a cell that does not count is a select that leaves the pair as it
// is, so a NaN or an infinity there stays out.  The weights are positive, so den > 0 says that a cell was accepted.  The
// lane reads its base, then writes its value: d_base may be d_out.
template <bool NORMALS>
__global__ void __launch_bounds__(256) k_plane_upsample(const PlaneUpsampleParams P) {
    __shared__ float s_t[kUpsampleMaxCells];
    __shared__ float s_v[kUpsampleMaxCells];
    __shared__ float s_n[NORMALS ? 3 * kUpsampleMaxCells : 1];
    const uint32_t r = P.radius, st = P.stride;
    const uint32_t tiles_x = (P.width + kFilterTileW - 1u) / kFilterTileW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t cx_first = (tx * kFilterTileW) / st, cy_first = (ty * kFilterTileH) / st;
    const uint32_t hw = (tx * kFilterTileW + kFilterTileW - 1u) / st - cx_first + 1u + 2u * r;
    const uint32_t hh = (ty * kFilterTileH + kFilterTileH - 1u) / st - cy_first + 1u + 2u * r;
    const uint32_t cells = hw * hh; // <= kUpsampleMaxCells for st >= 1, r <= kUpsampleMaxRadius (image.h)
    const int x0 = (int)cx_first - (int)r, y0 = (int)cy_first - (int)r;
    for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
        const uint32_t cy = c / hw, cx = c - cy * hw;
        const int X = x0 + (int)cx, Y = y0 + (int)cy;
        float t = __builtin_inff(), v = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (X >= 0 && Y >= 0 && (uint32_t)X < P.lo_width && (uint32_t)Y < P.lo_height) {
            const uint32_t gx = (uint32_t)X * st + P.px0, gy = (uint32_t)Y * st + P.py0;
            if (gx < P.width && gy < P.height) {
                const size_t i = (size_t)gy * P.width + gx;
                const trx_hit h = P.primary[i];
                if (h.t < TRX_F32_MAX && h.prim != TRX_INVALID) {
                    t = h.t;
                    v = P.in_lo[(size_t)Y * P.lo_width + (uint32_t)X];
                    if constexpr (NORMALS) {
                        const float *n = P.attr[i].normal;
                        nx = n[0]; ny = n[1]; nz = n[2];
                    }
                }
            }
        }
        s_t[c] = t;
        s_v[c] = v;
        if constexpr (NORMALS) {
            s_n[c] = nx;
            s_n[kUpsampleMaxCells + c] = ny;
            s_n[2u * kUpsampleMaxCells + c] = nz;
        }
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
    const uint32_t px = tx * kFilterTileW + lx, py = ty * kFilterTileH + ly;
    if (px >= P.width || py >= P.height) return;
    const size_t ip = (size_t)py * P.width + px;
    const trx_hit hp = P.primary[ip];
    if (!(hp.t < TRX_F32_MAX && hp.prim != TRX_INVALID)) { // no surface: the base's bits copied, +0 without a base
        uint32_t bits = 0u;
        if (P.base) bits = reinterpret_cast<const uint32_t *>(P.base)[ip];
        reinterpret_cast<uint32_t *>(P.out)[ip] = bits;
        return;
    }
    const float tp = hp.t, tol = P.depth_tol * tp;
    float npx = 0.0f, npy = 0.0f, npz = 0.0f;
    if constexpr (NORMALS) {
        const float *n = P.attr[ip].normal;
        npx = n[0]; npy = n[1]; npz = n[2];
    }
    // the window's first cell, and the cell whose pixel is p itself (none when p is not a pixel of this phase)
    const uint32_t qx = px / st, qy = py / st;
    const uint32_t wx = qx - cx_first, wy = qy - cy_first;
    const uint32_t own = (px - qx * st == P.px0 && py - qy * st == P.py0) ? (wy + r) * hw + wx + r : 0xFFFFFFFFu;
    float num = 0.0f, den = 0.0f, num_all = 0.0f, den_all = 0.0f;
    for (uint32_t dy = 0; dy <= 2u * r; dy++) {
        const uint32_t row = (wy + dy) * hw + wx;
        const uint32_t ky = dy <= r ? dy + 1u : 2u * r + 1u - dy; // k[|dy - r|] = r + 1 - |dy - r|
        for (uint32_t dx = 0; dx <= 2u * r; dx++) {
            const uint32_t kx = dx <= r ? dx + 1u : 2u * r + 1u - dx;
            const float w = (float)(ky * kx);
            const uint32_t c = row + dx;
            const float tq = s_t[c];
            const bool surf = tq < TRX_F32_MAX;
            bool ok = surf && __builtin_fabsf(tq - tp) <= tol;
            if constexpr (NORMALS)
                ok = ok && (npx * s_n[c] + npy * s_n[kUpsampleMaxCells + c]) + npz * s_n[2u * kUpsampleMaxCells + c] >= P.normal_cos;
            ok = ok || c == own;
            const float term = w * s_v[c];
            num = ok ? num + term : num;
            den = ok ? den + w : den;
            num_all = surf ? num_all + term : num_all;
            den_all = surf ? den_all + w : den_all;
        }
    }
    // no cell accepted: every surface cell of the window (FALLBACK); none of those either: +0 (EMPTY)
    if (!(den > 0.0f)) {
        num = num_all;
        den = den_all;
    }
    float f = den > 0.0f ? __fdiv_rn(num, den) : 0.0f;
    if (P.base) f = P.base[ip] + f;
    P.out[ip] = f;
}

// The colour compose (trx_material_compose_dev; include/trx.h, "materials"): one lane per record, planes at c * n_items.  A
// record with t < FLT_MAX and prim < n_tris (which rules 0xFFFFFFFF out) is a surface record of the scene, its index into the
// material table was validated on upload; any other record - a caller's too - reads neither table and is background.  All of a
// lane's reads come before its writes, so out may be the indirect planes.  A streaming kernel: no scratch, no LDS.
__global__ void __launch_bounds__(256) k_compose(const ComposeParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_items) return;
    const size_t n = P.n_items;
    const trx_hit ph = P.primary[i];
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (ph.t < TRX_F32_MAX && ph.prim < P.n_tris) {
        const float2 *mp = reinterpret_cast<const float2 *>(P.materials + P.tri_material[ph.prim]);
        const float2 m0 = mp[0], m1 = mp[1], m2 = mp[2]; // {albedo r, g}, {albedo b, emission r}, {emission g, b}
        const float E = P.direct[i];
        float Ir = E, Ig = E, Ib = E;
        if (P.indirect) {
            Ir = E + P.indirect[i];
            Ig = E + P.indirect[n + i];
            Ib = E + P.indirect[2u * n + i];
        }
        r = m1.y + m0.x * Ir;
        g = m2.x + m0.y * Ig;
        b = m2.y + m1.x * Ib;
    }
    P.out[i] = r;
    P.out[n + i] = g;
    P.out[2u * n + i] = b;
}

// The colour shade (trx_shade_rgb_dev): k_value's code, three times per record.  The 1 KiB table is searched where it lies:
// every wave reads the same few lines of it, which stay in cache, and the kernel takes no LDS.
__device__ __forceinline__ uint32_t colour_code(const float *thr, float col) {
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1) c += col >= thr[c + step] ? step : 0u;
    return c;
}
__global__ void __launch_bounds__(256) k_rgb_shade(const ShadeRgbParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_items) return;
    const size_t n = P.n_items;
    const uint32_t r = colour_code(P.thr, P.colour[i]), g = colour_code(P.thr, P.colour[n + i]), b = colour_code(P.thr, P.colour[2u * n + i]);
    reinterpret_cast<uint32_t *>(P.rgba)[i] = r | g << 8 | b << 16 | 0xFF000000u; // {r, g, b, 255}
}

// The textured albedo of every record (trx_surface_albedo_dev; include/trx.h, "THE TEXTURED ALBEDO"): one lane per record,
// planes at c * n_items.  k_compose's surface rule: a record with t < FLT_MAX and prim < n_tris is a surface record of the
// scene, and every table index formed from it was validated when its table was set; any other record - a caller's too - reads
// no table and gets +0.  u and v are used as they come (the sampling rule survives any float).  Gathers only: no scratch, no LDS.
__global__ void __launch_bounds__(256) k_surface_albedo(const SurfaceAlbedoParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_items) return;
    const size_t n = P.n_items;
    const trx_hit ph = P.hits[i];
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (ph.t < TRX_F32_MAX && ph.prim < P.n_tris) {
        const uint32_t m = P.tri_material[ph.prim];
        const float2 *mp = reinterpret_cast<const float2 *>(P.materials + m);
        const float2 m0 = mp[0]; // {albedo r, g}
        r = m0.x;
        g = m0.y;
        b = P.materials[m].albedo[2];
        const float2 uv = *reinterpret_cast<const float2 *>(P.attr + i); // {u, v}: the record's first 8 bytes
        textured_albedo(P.tex, ph.prim, m, uv.x, uv.y, r, g, b);
    }
    P.out[i] = r;
    P.out[n + i] = g;
    P.out[2u * n + i] = b;
}

// The colour compose over an albedo plane (trx_albedo_compose_dev): k_compose with albedo_c(m) replaced by the plane's value,
// the same association and the same background rule.  All of a lane's reads come before its writes, so out may be the indirect
// planes.
__global__ void __launch_bounds__(256) k_albedo_compose(const AlbedoComposeParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_items) return;
    const size_t n = P.n_items;
    const trx_hit ph = P.primary[i];
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (ph.t < TRX_F32_MAX && ph.prim < P.n_tris) {
        const float2 *mp = reinterpret_cast<const float2 *>(P.materials + P.tri_material[ph.prim]);
        const float2 m1 = mp[1], m2 = mp[2]; // {albedo b, emission r}, {emission g, b}
        const float Ar = P.albedo[i], Ag = P.albedo[n + i], Ab = P.albedo[2u * n + i];
        const float E = P.direct[i];
        float Ir = E, Ig = E, Ib = E;
        if (P.indirect) {
            Ir = E + P.indirect[i];
            Ig = E + P.indirect[n + i];
            Ib = E + P.indirect[2u * n + i];
        }
        r = m1.y + Ar * Ir;
        g = m2.x + Ag * Ig;
        b = m2.y + Ab * Ib;
    }
    P.out[i] = r;
    P.out[n + i] = g;
    P.out[2u * n + i] = b;
}

} // namespace

hipError_t launch_surface_albedo(const SurfaceAlbedoParams &p, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    if (!p.hits || !p.attr || !p.out || !p.materials || !p.tri_material) return hipErrorInvalidValue;
    // (a texture set is whole or absent: the kernel reads all four tables once it has seen descs)
    if (p.tex.descs && (!p.tex.texels || !p.tex.material_texture || !p.tex.srgb)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_surface_albedo, dim3((p.n_items + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_albedo_compose(const AlbedoComposeParams &p, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    if (!p.primary || !p.albedo || !p.direct || !p.out || !p.materials || !p.tri_material) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_albedo_compose, dim3((p.n_items + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_compose(const ComposeParams &p, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    if (!p.primary || !p.direct || !p.out || !p.materials || !p.tri_material) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_compose, dim3((p.n_items + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_shade_rgb(const ShadeRgbParams &p, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    if (!p.thr || !p.colour || !p.rgba) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rgb_shade, dim3((p.n_items + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_heat(const HeatParams &p, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(k_heat, dim3((p.n_items + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_ao_filter(const AoFilterParams &p, hipStream_t stream) {
    const uint64_t tiles = (uint64_t)((p.width + kFilterTileW - 1u) / kFilterTileW) * ((p.height + kFilterTileH - 1u) / kFilterTileH);
    if (tiles == 0) return hipSuccess;
    if (tiles > 0x7fffffffull || p.radius > kFilterMaxRadius) return hipErrorInvalidValue;
    if (p.attr) hipLaunchKernelGGL(k_ao_filter<true>, dim3((uint32_t)tiles), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(k_ao_filter<false>, dim3((uint32_t)tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_ao_upsample(const AoUpsampleParams &p, hipStream_t stream) {
    const uint64_t tiles = (uint64_t)((p.width + kFilterTileW - 1u) / kFilterTileW) * ((p.height + kFilterTileH - 1u) / kFilterTileH);
    if (tiles == 0) return hipSuccess;
    // (what bounds the kernel's LDS indices and its reads of the low grid)
    if (tiles > 0x7fffffffull || p.radius > kUpsampleMaxRadius || p.stride == 0 || p.stride > kUpsampleMaxStride || p.px0 >= p.stride ||
        p.py0 >= p.stride || p.lo_width != (p.width + p.stride - 1u) / p.stride || p.lo_height != (p.height + p.stride - 1u) / p.stride)
        return hipErrorInvalidValue;
    if (p.attr) hipLaunchKernelGGL(k_ao_upsample<true>, dim3((uint32_t)tiles), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(k_ao_upsample<false>, dim3((uint32_t)tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_plane_upsample(const PlaneUpsampleParams &p, hipStream_t stream) {
    const uint64_t tiles = (uint64_t)((p.width + kFilterTileW - 1u) / kFilterTileW) * ((p.height + kFilterTileH - 1u) / kFilterTileH);
    if (tiles == 0) return hipSuccess;
    // (what bounds the kernel's LDS indices and its reads of the low grid)
    if (tiles > 0x7fffffffull || p.radius > kUpsampleMaxRadius || p.stride == 0 || p.stride > kUpsampleMaxStride || p.px0 >= p.stride ||
        p.py0 >= p.stride || p.lo_width != (p.width + p.stride - 1u) / p.stride || p.lo_height != (p.height + p.stride - 1u) / p.stride ||
        p.in_lo == p.out)
        return hipErrorInvalidValue;
    if (p.attr) hipLaunchKernelGGL(k_plane_upsample<true>, dim3((uint32_t)tiles), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(k_plane_upsample<false>, dim3((uint32_t)tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_atrous(const AtrousParams &p, hipStream_t stream) {
    // (what bounds the kernel's LDS indices: a power of two up to kAtrousMaxSpacing)
    if (p.spacing == 0 || p.spacing > kAtrousMaxSpacing || (p.spacing & (p.spacing - 1u)) != 0 || p.in == p.out) return hipErrorInvalidValue;
    if (p.width == 0 || p.height == 0) return hipSuccess;
    // per tile column: every row class that holds a row, and in each as many groups of 8 lattice rows as the fullest class has
    const uint64_t tiles_x = (p.width + kAtrousTileW - 1u) / kAtrousTileW, classes = p.spacing < p.height ? p.spacing : p.height;
    const uint64_t lattice_rows = ((uint64_t)p.height + p.spacing - 1u) / p.spacing;
    const uint64_t blocks = tiles_x * classes * ((lattice_rows + kAtrousTileRows - 1u) / kAtrousTileRows);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (p.attr) hipLaunchKernelGGL(k_atrous<true>, dim3((uint32_t)blocks), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(k_atrous<false>, dim3((uint32_t)blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_shade(const ShadeParams &p, int mode, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    const dim3 grid((p.n_items + 255u) / 256u), block(256);
    switch (mode) {
    case kShadeReference: hipLaunchKernelGGL(k_shade<kShadeReference>, grid, block, 0, stream, p); break;
    case kShadeCounts: hipLaunchKernelGGL(k_shade<kShadeCounts>, grid, block, 0, stream, p); break;
    case kShadeTerm: hipLaunchKernelGGL(k_shade<kShadeTerm>, grid, block, 0, stream, p); break;
    case kShadeValue: hipLaunchKernelGGL(k_value, grid, block, 0, stream, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace trx
