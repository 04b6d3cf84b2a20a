// refit_gpu.h - BVH refit (include/trx.h, trx_scene_refit / trx_refit_nodes): new vertices for every triangle record, the
// topology of the node buffer kept, every quantisation frame and child box recomputed bottom-up.
//
// The per-node work is ONE __host__ __device__ function (refit_node) that the host twin (api_refit.cpp) and the device
// kernels (refit_gpu.cpp) both call, so that the two produce the same bytes.  Where it does what the builder does it calls
// the builder's own rules (build_rules.h), which is why a refit with the build's own inputs returns the build's bytes
// (tests/test_refit.py, tests/test_refit_twin.py) - for signed zeros too, although the refit folds a node's box over its
// children in slot order and the builder in merge order, so that a minimum over +0 and -0 may keep the other zero:
// frame_origin writes a zero origin as +0 on both sides.
//   triangle record  convert_tris for TRX_TRI_VERTS_36 (api.cpp): e1 = v0 - v1, e2 = v2 - v0, ng = e1 x e2
//   leaf box         min / max over the three vertices of every triangle of the slot, the first of equal ones as grow_pt
//                    keeps it (builder, api_build.cpp refs.box)
//   inner box        the union of the boxes of the child node's own children (the f32 box array below, never the bytes)
//   encoding         frame_origin, quant_step and quant_planes, as Collapser::emit (builder.cpp) and k8_encode (collapse_gpu.cpp)
//   TLAS leaf box    the refit box of BLAS node instance_offsets[k] + entry[k]; with instance transforms it goes through
//                    instance_world_box, as in trx_flat_build_instanced
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "build_rules.h"

namespace trx {

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
                grow(b, pb);
            }
        }
        cb[s] = b;
        grow(nb, b);
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
        p[a] = frame_origin(nb.mn[a]);
        e[a] = quant_step(nb.mn[a], nb.mx[a]);
        ebyte[a] = (rf_bits(e[a]) >> 23) & 0xffu;
    }
    // planes min_x,max_x,min_y,max_y,min_z,max_z as words {lo slots 0-3, slots 4-7}; empty slots keep their bytes
    uint32_t q[6][2] = {{w[2].x, w[2].y}, {w[2].z, w[2].w}, {w[3].x, w[3].y}, {w[3].z, w[3].w}, {w[4].x, w[4].y}, {w[4].z, w[4].w}};
    for (int s = 0; s < 8; s++) {
        if (meta[s] == 0) continue;
        const uint32_t sh = 8u * (uint32_t)(s & 3), keep = ~(0xffu << sh);
        for (int a = 0; a < 3; a++) {
            uint32_t lo, hi;
            quant_planes(p[a], e[a], cb[s].mn[a], cb[s].mx[a], lo, hi);
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
