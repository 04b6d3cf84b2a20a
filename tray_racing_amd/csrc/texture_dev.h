// texture_dev.h - THE TEXTURED ALBEDO (include/trx.h): the one device statement of how a surface record's albedo is sampled
// from the scene's texture set.  Every kernel that needs a textured albedo calls textured_albedo(); tests/texture_twin.py
// restates it in numpy.  Every operation is rounded once in binary32 (the translation units that include this are built
// without contraction, with correctly rounded division).
#ifndef TRX_TEXTURE_DEV_H
#define TRX_TEXTURE_DEV_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace trx {

// The scene's texcoord table and texture set as a kernel sees them; texcoords or descs null = none.  Every index a kernel
// forms was validated when the tables were set: material_texture[m] < the number of descriptors (or 0xFFFFFFFF), every
// descriptor's offset + width * height within the texel array.
struct TextureTables {
    const float2 *texcoords;          // three per triangle: (s0, t0), (s1, t1), (s2, t2)
    const uint4 *descs;               // {offset, width, height, format | filter << 8}
    const uint32_t *texels;           // RGBA8 words
    const uint32_t *material_texture; // per material: a descriptor index or 0xFFFFFFFF
    const float *srgb;                // 256 floats (trx_texture_srgb_table)
};

#ifdef __HIPCC__
// one channel of a tap: (float)c8 / 255.0f, or the sRGB table's entry
__device__ __forceinline__ float texel_channel(const float *srgb, bool is_srgb, uint32_t word, uint32_t shift) {
    const uint32_t c8 = (word >> shift) & 0xffu;
    return is_srgb ? srgb[c8] : __fdiv_rn((float)c8, 255.0f);
}

// repeat wrap: s - floorf(s), with the 1.0f a tiny negative s rounds to taken to 0
__device__ __forceinline__ float wrap_repeat(float s) {
    const float f = s - floorf(s);
    return f >= 1.0f ? 0.0f : f;
}

// (ar, ag, ab) holds albedo(m) on entry and A on return: unchanged where the rule falls back to the material's albedo.
__device__ __forceinline__ void textured_albedo(const TextureTables &T, uint32_t prim, uint32_t m, float u, float v, float &ar, float &ag,
                                                float &ab) {
    if (!T.texcoords || !T.descs) return;
    const uint32_t tex = T.material_texture[m];
    if (tex == 0xffffffffu) return;
    const float2 *uv = T.texcoords + (size_t)prim * 3u;
    const float2 a = uv[0], b = uv[1], c = uv[2];
    const float w = (1.0f - u) - v;
    const float s = (w * a.x + u * b.x) + v * c.x;
    const float t = (w * a.y + u * b.y) + v * c.y;
    if (!(fabsf(s) < __builtin_inff()) || !(fabsf(t) < __builtin_inff())) return; // (NaN compares false)
    const uint4 d = T.descs[tex];
    const uint32_t W = d.y, H = d.z;
    const bool is_srgb = (d.w & 0xffu) != 0u, bilinear = (d.w >> 8) != 0u;
    const uint32_t *tx = T.texels + d.x;
    const float fs = wrap_repeat(s), ft = wrap_repeat(t); // in [0, 1)
    float vr, vg, vb;
    if (!bilinear) {
        const uint32_t ix = min((uint32_t)(fs * (float)W), W - 1u), iy = min((uint32_t)(ft * (float)H), H - 1u);
        const uint32_t p = tx[iy * W + ix];
        vr = texel_channel(T.srgb, is_srgb, p, 0u);
        vg = texel_channel(T.srgb, is_srgb, p, 8u);
        vb = texel_channel(T.srgb, is_srgb, p, 16u);
    } else {
        // x in [-0.5, W - 0.5] (fs * W may round up to W), so x0 in [-1, W - 1]: ix0 == -1 wraps to W - 1, ix1 == W to 0.  The
        // min() never binds; it is what keeps the four reads inside the texture whatever the arithmetic above is changed to.
        const float x = fs * (float)W - 0.5f, y = ft * (float)H - 0.5f;
        const float x0 = floorf(x), y0 = floorf(y);
        const float fx = x - x0, fy = y - y0;
        const int jx = (int)x0, jy = (int)y0;
        const uint32_t ix0 = min(jx < 0 ? W - 1u : (uint32_t)jx, W - 1u), iy0 = min(jy < 0 ? H - 1u : (uint32_t)jy, H - 1u);
        const uint32_t ix1 = (uint32_t)(jx + 1) >= W ? 0u : (uint32_t)(jx + 1), iy1 = (uint32_t)(jy + 1) >= H ? 0u : (uint32_t)(jy + 1);
        const uint32_t p00 = tx[iy0 * W + ix0], p10 = tx[iy0 * W + ix1], p01 = tx[iy1 * W + ix0], p11 = tx[iy1 * W + ix1];
        float val[3];
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) {
            const float c00 = texel_channel(T.srgb, is_srgb, p00, 8u * k), c10 = texel_channel(T.srgb, is_srgb, p10, 8u * k);
            const float c01 = texel_channel(T.srgb, is_srgb, p01, 8u * k), c11 = texel_channel(T.srgb, is_srgb, p11, 8u * k);
            const float top = c00 + fx * (c10 - c00), bot = c01 + fx * (c11 - c01);
            val[k] = top + fy * (bot - top);
        }
        vr = val[0], vg = val[1], vb = val[2];
    }
    ar = ar * vr;
    ag = ag * vg;
    ab = ab * vb;
}
#endif // __HIPCC__

} // namespace trx

#endif // TRX_TEXTURE_DEV_H
