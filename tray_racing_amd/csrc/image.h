// image.h - launch interface between api_image.cpp and the image passes after the walk (image.hip): the edge-aware AO
// filter and the shading to RGBA8 (include/trx.h, "the frame's image").  No traversal kernel knows about them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/trx.h"
#include "texture_dev.h"

namespace trx {

// k_ao_filter: one workgroup of 256 lanes per kFilterTileW x kFilterTileH pixel tile (a wave = two rows of 32 pixels).
// The tile and its halo of `radius` pixels on every side are loaded once into LDS, then every lane sums its window.
constexpr uint32_t kFilterTileW = 32, kFilterTileH = 8;
constexpr uint32_t kFilterMaxRadius = TRX_MAX_AO_FILTER_RADIUS;
constexpr uint32_t kFilterMaxCells = (kFilterTileW + 2 * kFilterMaxRadius) * (kFilterTileH + 2 * kFilterMaxRadius); // 640
struct AoFilterParams {
    const trx_hit *primary;   // whole image, y * width + x
    const trx_hit_attr *attr; // or null: no normal test
    const uint8_t *counts;
    trx_ao_term *out;
    uint32_t width, height, n_samples, radius;
    float depth_tol, normal_cos;
};
hipError_t launch_ao_filter(const AoFilterParams &p, hipStream_t stream);

// k_ao_upsample (trx_ao_upsample_dev): the filter's shape - one workgroup of 256 lanes per kFilterTileW x kFilterTileH tile of
// FULL-resolution pixels - over the cells of the sparse visibility pass's low grid (cell (X, Y) = pixel (X * stride + px0,
// Y * stride + py0)).  LDS holds the low cells under the tile and a halo of `radius` cells: 32 consecutive pixels cover
// floor((a + 31) / s) - floor(a / s) + 1 cells, 32 at s = 1 and at most 17 beyond, so stride 1 at the largest radius is the
// largest case: (32 + 2r) x (8 + 2r) cells.
constexpr uint32_t kUpsampleMaxStride = TRX_MAX_AO_STRIDE;
constexpr uint32_t kUpsampleMaxRadius = TRX_MAX_AO_UPSAMPLE_RADIUS;
constexpr uint32_t kUpsampleMaxCells = (kFilterTileW + 2 * kUpsampleMaxRadius) * (kFilterTileH + 2 * kUpsampleMaxRadius); // 432
struct AoUpsampleParams {
    const trx_hit *primary;   // whole FULL-resolution image, y * width + x
    const trx_hit_attr *attr; // or null: no normal test
    const uint8_t *counts_lo; // the low grid, Y * lo_width + X
    trx_ao_term *out;         // full resolution
    uint32_t width, height, lo_width, lo_height;
    uint32_t stride, px0, py0;
    uint32_t n_samples, radius;
    float depth_tol, normal_cos;
};
hipError_t launch_ao_upsample(const AoUpsampleParams &p, hipStream_t stream);

// k_plane_upsample (trx_value_upsample_dev): k_ao_upsample's shape and window over a low grid of FLOATS - the sparse indirect
// pass's values - with the weighted float sums of the header's rule in place of the integer counts.  The same tile, the same
// cells in LDS (kUpsampleMaxCells: depth, value and, with normals, three components - 20 B or 8 B a cell).
static_assert(TRX_MAX_VALUE_UPSAMPLE_RADIUS == TRX_MAX_AO_UPSAMPLE_RADIUS, "k_plane_upsample stages kUpsampleMaxCells cells");
struct PlaneUpsampleParams {
    const trx_hit *primary;   // whole FULL-resolution image, y * width + x
    const trx_hit_attr *attr; // or null: no normal test
    const float *in_lo;       // the low grid, Y * lo_width + X
    const float *base;        // full resolution, or null; may be `out`
    float *out;               // full resolution
    uint32_t width, height, lo_width, lo_height;
    uint32_t stride, px0, py0;
    uint32_t radius;
    float depth_tol, normal_cos;
};
hipError_t launch_plane_upsample(const PlaneUpsampleParams &p, hipStream_t stream);

// k_atrous (trx_value_filter_dev): one level of the a-trous filter at spacing s = 1 << level.  A level couples only pixels
// of one residue class in y mod s (and in x mod s), so a workgroup of 256 lanes takes kAtrousTileW consecutive x of
// kAtrousTileRows LATTICE rows y0 + k * s of one row class, and stages those rows, two lattice rows above and below and 2s
// columns either side into LDS: (32 + 4s) x 12 cells, 432 at s = 1 and kAtrousMaxCells = 1152 at s = 16 - the footprint
// grows linearly with s where a pixel-space tile with a halo of 2s would grow with its square.
constexpr uint32_t kAtrousTileW = 32, kAtrousTileRows = 8;
constexpr uint32_t kAtrousMaxLevels = TRX_MAX_VALUE_FILTER_LEVELS;
constexpr uint32_t kAtrousMaxSpacing = 1u << (kAtrousMaxLevels - 1);                               // 16
constexpr uint32_t kAtrousRows = kAtrousTileRows + 4;                                              // 12 staged lattice rows
constexpr uint32_t kAtrousMaxCells = (kAtrousTileW + 4 * kAtrousMaxSpacing) * kAtrousRows;         // 1152
struct AtrousParams {
    const trx_hit *primary;   // whole image, y * width + x
    const trx_hit_attr *attr; // or null: no normal test
    const float *in;          // the level's input plane u
    const float *base;        // last level only, or null; may be `out`
    float *out;               // the level's output plane u' (never `in`)
    uint32_t width, height, spacing;
    uint32_t last;            // 1: the pass's last level - the base is added, a pixel without a surface gets its base
    float depth_tol, normal_cos;
};
hipError_t launch_atrous(const AtrousParams &p, hipStream_t stream);

// k_shade: one lane per record, 4 bytes {c, c, c, 255} written per record; c by an 8-step search of the 256 thresholds
// (trx_image_code_table) each workgroup first copies into LDS.  kShadeValue (trx_shade_value_dev) launches k_value: the same
// table, search and store over float values.
enum ShadeMode : int { kShadeReference = 0, kShadeCounts = 1, kShadeTerm = 2, kShadeValue = 3 };
struct ShadeParams {
    const float *thr;        // 256 floats, device memory
    const trx_hit *primary;  // kShadeReference
    const trx_hit *ao;       // kShadeReference
    const uint8_t *counts;   // kShadeCounts
    const trx_ao_term *term; // kShadeTerm
    uint8_t *rgba;
    uint32_t n_items;
    uint32_t n_samples;      // kShadeCounts
    const float *value;      // kShadeValue (last: the fields the other modes read keep their offsets)
};
hipError_t launch_shade(const ShadeParams &p, int mode, hipStream_t stream);

// The colour image (include/trx.h, "materials"): both kernels are elementwise over n_items records, planes at c * n_items.
//   k_compose    (trx_material_compose_dev) one lane per record: 8 B of primary record, the u16 index and 24 B of material for
//                a surface record of the scene (prim < n_tris; every index was validated on upload), 4 B of the direct plane
//                and 12 B of the indirect planes (none with a null pointer) read, 12 B written: emission + albedo * (E + I_c),
//                +0 for any other record.  Every lane reads before it writes: out may be indirect.
//   k_rgb_shade  (trx_shade_rgb_dev) one lane per record: 12 B read, {code(R), code(G), code(B), 255} written, each code by
//                k_value's 8-step search - in the table where it lies in device memory (1 KiB, cache-resident), not in LDS.
struct ComposeParams {
    const trx_hit *primary;
    const float *direct;
    const float *indirect;         // three planes, or null
    float *out;                    // three planes
    const trx_material *materials;
    const uint16_t *tri_material;
    uint32_t n_items, n_tris;
};
hipError_t launch_compose(const ComposeParams &p, hipStream_t stream);
struct ShadeRgbParams {
    const float *thr;   // 256 floats, device memory
    const float *colour; // three planes
    uint8_t *rgba;
    uint32_t n_items;
};
hipError_t launch_shade_rgb(const ShadeRgbParams &p, hipStream_t stream);

// The textured albedo (include/trx.h, "texture coordinates and albedo textures"): both kernels are elementwise over n_items
// records in any layout, planes at c * n_items.
//   k_surface_albedo  (trx_surface_albedo_dev) one lane per record: 8 B of hit record and 8 B of u, v read; for a surface record
//                     of the scene (prim < n_tris) the u16 material index and 12 B of albedo, then - with tables, a textured
//                     material and finite coordinates - the texture index, the 16 B descriptor, 24 B of texcoords and one or
//                     four 4 B texels (texture_dev.h); 12 B written: the albedo, +0 for any other record.
//   k_albedo_compose  (trx_albedo_compose_dev) k_compose with the albedo read from three planes instead of the material:
//                     emission + A_c * (E + I_c).  Every lane reads before it writes: out may be indirect.
struct SurfaceAlbedoParams {
    const trx_hit *hits;
    const trx_hit_attr *attr;
    float *out; // three planes
    const trx_material *materials;
    const uint16_t *tri_material;
    TextureTables tex;
    uint32_t n_items, n_tris;
};
hipError_t launch_surface_albedo(const SurfaceAlbedoParams &p, hipStream_t stream);
struct AlbedoComposeParams {
    const trx_hit *primary;
    const float *albedo;           // three planes
    const float *direct;
    const float *indirect;         // three planes, or null
    float *out;                    // three planes
    const trx_material *materials; // (the emission)
    const uint16_t *tri_material;
    uint32_t n_items, n_tris;
};
hipError_t launch_albedo_compose(const AlbedoComposeParams &p, hipStream_t stream);

// k_heat: the PROFILE_RT heat map (trx_shade_heat_dev) - one lane per record, 4 bytes of per-ray counts read, 4 bytes
// {r, g, b, 255} written.  No table in LDS, no pow: the colour is arithmetic on the count.
struct HeatParams {
    const trx_ray_cost *cost;
    uint8_t *rgba;
    uint32_t n_items;
    uint32_t which; // TRX_HEAT_NODES / TRX_HEAT_TRIS
    float scale;
};
hipError_t launch_heat(const HeatParams &p, hipStream_t stream);

} // namespace trx
