// refit_gpu.h - BVH refit (include/trx.h, trx_scene_refit / trx_refit_nodes): new vertices for every triangle record, the
// topology of the node buffer kept, every quantisation frame and child box recomputed bottom-up.
//
// The per-node work is ONE __host__ __device__ function (refit_node) that the host twin (api_refit.cpp) and the device
// kernels (refit_gpu.cpp) both call, so that the two produce the same bytes.  It restates the builder's rules:
//   triangle record  convert_tris for TRX_TRI_VERTS_36 (api.cpp): e1 = v0 - v1, e2 = v2 - v0, ng = e1 x e2
//   leaf box         min / max over the three vertices of every triangle of the slot (builder, api_build.cpp refs.box)
//   inner box        the union of the boxes of the child node's own children (the f32 box array below, never the bytes)
//   encoding         Collapser::emit (builder.cpp) and k8_encode (collapse_gpu.cpp): quant_scale, the doubling while
//                    255 steps do not reach the far plane, floor / ceil with the reciprocal, the clamp, the two
//                    conservative correction loops
//   TLAS leaf box    the refit box of BLAS node instance_offsets[k] + entry[k]; with instance transforms its 8 corners
//                    go through object_to_world[k] and the result is padded (instance_world_box, shared with
//                    trx_flat_build_instanced)
// The builder's own encoders are left as they are (the golden buffers pin their bytes); tests/test_refit.py shows the
// three agree: a refit with the build's own inputs returns the build's bytes.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "cwbvh_format.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TRX_HD __host__ __device__
#else
#define TRX_HD
#endif

namespace trx {

// min / max with std::min / std::max's answer for equal operands (the first one), so that signed zeros come out as the
// builder's do
TRX_HD inline float rf_min(float a, float b) { return b < a ? b : a; }
TRX_HD inline float rf_max(float a, float b) { return a < b ? b : a; }

TRX_HD inline uint32_t rf_bits(float f) {
    union { float f; uint32_t u; } c;
    c.f = f;
    return c.u;
}
TRX_HD inline float rf_float(uint32_t u) {
    union { float f; uint32_t u; } c;
    c.u = u;
    return c.f;
}

// The box of one instance in world space: the 8 corners of its BLAS box through the column-major affine object_to_world
// (NULL = identity), ((m0 x + m4 y) + m8 z) + m12 per row, then padded by a few ulps of its magnitude (the ray is taken
// to object space by the rounded INVERSE, which does not commute exactly with transforming the box forward).
TRX_HD inline void instance_world_box(const Aabb &bb, const float *m, Aabb &wb) {
    for (int a = 0; a < 3; a++) {
        wb.mn[a] = 3.402823466e+38f;
        wb.mx[a] = -3.402823466e+38f;
    }
    for (int c = 0; c < 8; c++) {
        const float p[3] = {c & 1 ? bb.mx[0] : bb.mn[0], c & 2 ? bb.mx[1] : bb.mn[1], c & 4 ? bb.mx[2] : bb.mn[2]};
        float q[3] = {p[0], p[1], p[2]};
        if (m)
            for (int r = 0; r < 3; r++) q[r] = m[r] * p[0] + m[4 + r] * p[1] + m[8 + r] * p[2] + m[12 + r];
        for (int a = 0; a < 3; a++) {
            wb.mn[a] = rf_min(wb.mn[a], q[a]);
            wb.mx[a] = rf_max(wb.mx[a], q[a]);
        }
    }
    for (int a = 0; a < 3; a++) {
        const float pad = 1e-5f * (rf_max(fabsf(wb.mn[a]), fabsf(wb.mx[a])) + (wb.mx[a] - wb.mn[a])) + 1e-30f;
        wb.mn[a] -= pad;
        wb.mx[a] += pad;
    }
}

// One 48-byte device triangle record from 9 vertex floats, exactly as convert_tris writes it for TRX_TRI_VERTS_36.
TRX_HD inline void refit_tri_record(const float *v, TriDev &t) {
    for (int k = 0; k < 3; k++) {
        t.v0[k] = v[k];
        t.e1[k] = v[k] - v[3 + k];
        t.e2[k] = v[6 + k] - v[k];
    }
    t.ngx = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
    t.ngy = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
    t.ngz = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
}

// What refit_node reads and writes.  nodes: the buffer refitted in place (a node reads only its own bytes and the boxes
// of its children, which lower height levels finished).  seg_base[i]: first node of node i's BVH segment (the BLAS it
// belongs to, or the TLAS), which its child_base_idx is relative to.
struct RefitCtx {
    uint4 *nodes;
    float *boxes;             // n_nodes * 6: min xyz, max xyz of every node after the refit
    const float *verts;       // n_tris * 9
    const uint32_t *seg_base; // n_nodes
    const uint32_t *inst;     // n_inst BLAS offsets, or null
    const uint32_t *entry;    // n_inst entry nodes, or null (node 0 of the BLAS)
    const float *o2w;         // n_inst column-major 4x4, or null (no transforms: instance boxes unpadded)
    uint32_t n_inst, tlas_start;
};

TRX_HD inline uint32_t leaf_count(uint8_t m) {
    const uint32_t bits = m >> 5;
    return bits == 1 ? 1u : bits == 3 ? 2u : bits == 7 ? 3u : 0u;
}

// The encoder rule of Collapser::emit for one axis: quantisation step of a node whose box spans [mn, mx].
TRX_HD inline float refit_quant_step(float mn, float mx) {
    // quant_scale: the smallest power of two >= max(extent, 1e-20) / 255
    const float extent = mx - mn;
    const float x = (extent < 1e-20f ? 1e-20f : extent) * (1.0f / 255.0f);
    const uint32_t xb = rf_bits(x);
    float e = rf_float((xb & 0x7fffffu) ? ((xb >> 23) + 1u) << 23 : xb);
    // make sure 255 steps reach the far plane after rounding
    while (ceil(((double)mx - (double)mn) / (double)e) > 255.0) e *= 2.0f;
    return e;
}

// ... and the two planes of a child box [cmn, cmx] in that frame.
TRX_HD inline void refit_quant_planes(float p, float e, float cmn, float cmx, uint32_t &qlo, uint32_t &qhi) {
    const float rcp = 1.0f / e;
    float lo = floorf((cmn - p) * rcp);
    float hi = ceilf((cmx - p) * rcp);
    lo = lo < 0.0f ? 0.0f : lo; // std::min(std::max(v, 0), 255)
    lo = 255.0f < lo ? 255.0f : lo;
    hi = hi < 0.0f ? 0.0f : hi;
    hi = 255.0f < hi ? 255.0f : hi;
    // keep the decoded planes conservative under f32 rounding of (c - p)
    while (lo > 0.0f && (double)p + (double)lo * (double)e > (double)cmn) lo -= 1.0f;
    while (hi < 255.0f && (double)p + (double)hi * (double)e < (double)cmx) hi += 1.0f;
    qlo = (uint32_t)lo & 0xffu;
    qhi = (uint32_t)hi & 0xffu;
}

// Refits node i: child boxes from the triangles / instances / children's boxes, a new frame, new child bytes; imask,
// bases, child_meta and the bytes of empty slots kept.  A node without children (the empty scene's root) is left as it
// is and reports the point box at its origin.
TRX_HD inline void refit_node(const RefitCtx &c, uint32_t i) {
    uint4 w[5];
    for (int k = 0; k < 5; k++) w[k] = c.nodes[(size_t)i * 5 + k];
    const uint32_t child_base = w[1].x, prim_base = w[1].y;
    uint8_t meta[8];
    for (int s = 0; s < 8; s++) meta[s] = (uint8_t)(((s < 4 ? w[1].z : w[1].w) >> (8 * (s & 3))) & 0xffu);
    const bool in_tlas = c.n_inst > 0 && i >= c.tlas_start;
    const uint32_t base = c.seg_base[i];
    Aabb cb[8];
    Aabb nb;
    for (int a = 0; a < 3; a++) {
        nb.mn[a] = INFINITY;
        nb.mx[a] = -INFINITY;
    }
    bool any = false;
    uint32_t rank = 0;
    for (int s = 0; s < 8; s++) {
        const uint8_t m = meta[s];
        if (m == 0) continue;
        Aabb b;
        for (int a = 0; a < 3; a++) {
            b.mn[a] = INFINITY;
            b.mx[a] = -INFINITY;
        }
        if ((m & 0x18) == 0x18) {
            const float *x = c.boxes + (size_t)(base + child_base + rank) * 6;
            for (int a = 0; a < 3; a++) {
                b.mn[a] = x[a];
                b.mx[a] = x[3 + a];
            }
            rank++;
        } else {
            const uint32_t first = prim_base + (m & 0x1fu), cnt = leaf_count(m);
            for (uint32_t j = first; j < first + cnt; j++) {
                Aabb pb;
                if (in_tlas) {
                    const uint32_t node = c.inst[j] + (c.entry ? c.entry[j] : 0u);
                    const float *x = c.boxes + (size_t)node * 6;
                    for (int a = 0; a < 3; a++) {
                        pb.mn[a] = x[a];
                        pb.mx[a] = x[3 + a];
                    }
                    if (c.o2w) {
                        const Aabb ob = pb;
                        instance_world_box(ob, c.o2w + (size_t)j * 16, pb);
                    }
                } else {
                    const float *v = c.verts + (size_t)j * 9;
                    for (int a = 0; a < 3; a++) {
                        pb.mn[a] = rf_min(v[a], rf_min(v[3 + a], v[6 + a]));
                        pb.mx[a] = rf_max(v[a], rf_max(v[3 + a], v[6 + a]));
                    }
                }
                for (int a = 0; a < 3; a++) {
                    b.mn[a] = rf_min(b.mn[a], pb.mn[a]);
                    b.mx[a] = rf_max(b.mx[a], pb.mx[a]);
                }
            }
        }
        cb[s] = b;
        for (int a = 0; a < 3; a++) {
            nb.mn[a] = rf_min(nb.mn[a], b.mn[a]);
            nb.mx[a] = rf_max(nb.mx[a], b.mx[a]);
        }
        any = true;
    }
    float *out_box = c.boxes + (size_t)i * 6;
    if (!any) {
        const uint32_t pw[3] = {w[0].x, w[0].y, w[0].z};
        for (int a = 0; a < 3; a++) out_box[a] = out_box[3 + a] = rf_float(pw[a]);
        return;
    }
    float p[3], e[3];
    uint32_t ebyte[3];
    for (int a = 0; a < 3; a++) {
        p[a] = nb.mn[a];
        e[a] = refit_quant_step(nb.mn[a], nb.mx[a]);
        ebyte[a] = (rf_bits(e[a]) >> 23) & 0xffu;
    }
    // planes min_x,max_x,min_y,max_y,min_z,max_z as words {lo slots 0-3, slots 4-7}; empty slots keep their bytes
    uint32_t q[6][2] = {{w[2].x, w[2].y}, {w[2].z, w[2].w}, {w[3].x, w[3].y}, {w[3].z, w[3].w}, {w[4].x, w[4].y}, {w[4].z, w[4].w}};
    for (int s = 0; s < 8; s++) {
        if (meta[s] == 0) continue;
        const uint32_t sh = 8u * (uint32_t)(s & 3), keep = ~(0xffu << sh);
        for (int a = 0; a < 3; a++) {
            uint32_t lo, hi;
            refit_quant_planes(p[a], e[a], cb[s].mn[a], cb[s].mx[a], lo, hi);
            q[2 * a][s >> 2] = (q[2 * a][s >> 2] & keep) | (lo << sh);
            q[2 * a + 1][s >> 2] = (q[2 * a + 1][s >> 2] & keep) | (hi << sh);
        }
    }
    uint4 *o = c.nodes + (size_t)i * 5;
    o[0] = make_uint4(rf_bits(p[0]), rf_bits(p[1]), rf_bits(p[2]), ebyte[0] | (ebyte[1] << 8) | (ebyte[2] << 16) | (w[0].w & 0xff000000u));
    o[2] = make_uint4(q[0][0], q[0][1], q[1][0], q[1][1]);
    o[3] = make_uint4(q[2][0], q[2][1], q[3][0], q[3][1]);
    o[4] = make_uint4(q[4][0], q[4][1], q[5][0], q[5][1]);
    for (int a = 0; a < 3; a++) {
        out_box[a] = nb.mn[a];
        out_box[3 + a] = nb.mx[a];
    }
}

// The refit's schedule over a node buffer: nodes by HEIGHT (a node lies above every child it references; a TLAS leaf's
// children are the BLAS entry nodes of its primitives), so that processing the levels in ascending order finishes every
// BLAS before any TLAS node reads its box - shared BLASes and re-braided subtrees included.  No index order is assumed.
struct RefitTopology {
    std::vector<uint32_t> order;       // node ids, level after level (ascending node id inside a level)
    std::vector<uint32_t> level_start; // n_levels + 1 offsets into order
    std::vector<uint32_t> seg_base;    // per node: first node of its segment
};
// Returns 0, or TRX_ERR_FORMAT with *why set when the references form a cycle.  The buffer must have passed
// validate_nodes (every index in range); entry may be null.
int refit_topology(const CwbvhNode *nodes, uint64_t n_nodes, const uint32_t *inst, uint32_t n_inst, uint32_t tlas_start,
                   const uint32_t *entry, RefitTopology &topo, const char **why);

// Device side (refit_gpu.cpp).  Everything is enqueued on `stream`; nothing synchronises.
struct RefitResult {
    uint32_t bad_input; // some vertex coordinate is not finite
    uint32_t e_ok;      // every node exponent byte is 0 or >= 21
    uint32_t p_ok;      // ... and every node origin is +0 or 2^-36 <= |p| <= 2^59
    uint32_t root_e;    // exponent bytes of the root node (scene diagonal)
};
bool refit_launch_check(const float *d_verts, uint64_t n_tris, RefitResult *d_result, hipStream_t stream);
bool refit_launch_tris(const float *d_verts, uint64_t n_tris, float4 *d_tris, hipStream_t stream);
bool refit_launch_level(const RefitCtx &ctx, const uint32_t *d_order, uint32_t begin, uint32_t count, hipStream_t stream);
bool refit_launch_stats(const uint4 *d_nodes, uint64_t n_nodes, uint32_t root, RefitResult *d_result, hipStream_t stream);

} // namespace trx
