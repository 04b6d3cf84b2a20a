// build_rules.h - the rules of the BVH build that more than one place must apply identically, each stated once as a
// __host__ __device__ function: the host builder (builder.cpp, compiled by the host compiler alone: no HIP header is
// needed here without __HIPCC__), its device stages (ploc_gpu.cpp, reinsert_gpu.cpp, collapse_gpu.cpp) and the refit
// (refit_gpu.h).  A tree built on the device is the host's tree byte for byte, and a refit with the build's own inputs
// returns the build's bytes, because all of them call these bodies: the same binary32 / binary64 operations in the
// same order, no contraction.  What differs between host and device - how a node, a box or a decision is fetched - is a
// parameter (a callable).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "cwbvh_format.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TRX_HD __host__ __device__
#else
#define TRX_HD
#endif

namespace trx {

// ---- records ---------------------------------------------------------------------------------------------------------
struct Node2 { // one BVH2 node, on the host and in device memory
    Aabb box;
    uint32_t left;  // inner: index of the left child
    uint32_t right; // inner: index of the right child
    uint32_t prim;  // leaf: primitive id
    uint32_t count; // primitives below this node (1 = leaf)
};
static_assert(sizeof(Node2) == 40, "Node2 layout");

// One entry of the collapse's cost table (Ylitie et al. 2017, section 4.2; seven per BVH2 node): 8 bytes, 8-byte aligned,
// so that a kernel fetches one with a single load.
enum : uint8_t { kLeaf = 0, kInternal = 1, kDistribute = 2 };
struct alignas(8) Decision {
    float cost;
    uint8_t type, dl, dr, pad;
};
static_assert(sizeof(Decision) == 8 && alignof(Decision) == 8, "Decision layout");

// ---- boxes -----------------------------------------------------------------------------------------------------------
// min / max with std::min / std::max's answer for equal operands: the FIRST one.  Signed zeros depend on it (fminf(+0, -0)
// is -0 on the device, std::min(+0, -0) is +0), and a node's origin is its box minimum.
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

TRX_HD inline void grow(Aabb &a, const Aabb &b) {
    for (int k = 0; k < 3; k++) {
        a.mn[k] = rf_min(a.mn[k], b.mn[k]);
        a.mx[k] = rf_max(a.mx[k], b.mx[k]);
    }
}
TRX_HD inline void grow_pt(Aabb &a, const float *p) {
    for (int k = 0; k < 3; k++) {
        a.mn[k] = rf_min(a.mn[k], p[k]);
        a.mx[k] = rf_max(a.mx[k], p[k]);
    }
}
TRX_HD inline float half_area(const Aabb &b) {
    const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    if (!(dx >= 0.f) || !(dy >= 0.f) || !(dz >= 0.f)) return 0.f;
    return dx * dy + dy * dz + dz * dx;
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
        grow_pt(wb, q);
    }
    for (int a = 0; a < 3; a++) {
        const float pad = 1e-5f * (rf_max(fabsf(wb.mn[a]), fabsf(wb.mx[a])) + (wb.mx[a] - wb.mn[a])) + 1e-30f;
        wb.mn[a] -= pad;
        wb.mx[a] += pad;
    }
}

// ---- Morton codes of the PLOC stage ------------------------------------------------------------------------------------
TRX_HD inline uint64_t spread21(uint64_t x) { // 21 bits -> every third bit
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
TRX_HD inline uint64_t morton_key21(const uint64_t q[3]) { return spread21(q[0]) | (spread21(q[1]) << 1) | (spread21(q[2]) << 2); }
// 42 bits per axis: the 126-bit key is l | h << 63, where l interleaves the low 21 bits of every axis (63 bits) and h
// the high 21 bits
TRX_HD inline void morton_key42(const uint64_t q[3], uint64_t &l, uint64_t &h) {
    const uint64_t lo[3] = {q[0] & 0x1fffffull, q[1] & 0x1fffffull, q[2] & 0x1fffffull}, hi[3] = {q[0] >> 21, q[1] >> 21, q[2] >> 21};
    l = morton_key21(lo);
    h = morton_key21(hi);
}

// the grid of the codes: centroid c of an axis falls into cell (c - lo) * scale, in binary64
struct MortonFrame {
    double lo[3], scale[3];
};
TRX_HD inline uint64_t morton_quant(float c, double lo, double scale) {
    const double v = ((double)c - lo) * scale;
    return v <= 0.0 ? 0ull : (uint64_t)v;
}
// (host) bits per axis: 21 or 42
inline MortonFrame morton_frame(const float *centroids, uint32_t n, int bits) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            lo[k] = rf_min(lo[k], centroids[3 * (size_t)i + k]);
            hi[k] = rf_max(hi[k], centroids[3 * (size_t)i + k]);
        }
    MortonFrame f;
    for (int k = 0; k < 3; k++) {
        const double ext = (double)hi[k] - (double)lo[k];
        f.lo[k] = (double)lo[k];
        f.scale[k] = ext > 0.0 ? ((double)((1ull << bits) - 1ull)) / ext : 0.0;
    }
    return f;
}

// ---- PLOC: the neighbour cluster i of m chooses, looking r >= 1 places either side; box_at(j) is cluster j's box --------
template <class BoxAt>
TRX_HD inline uint32_t ploc_nearest(uint32_t i, uint32_t m, uint32_t r, BoxAt box_at) {
    const Aabb bi = box_at(i);
    const uint32_t j0 = i > r ? i - r : 0u, j1 = i + r < m - 1u ? i + r : m - 1u;
    float best = INFINITY, pair_area = -1.f;
    uint32_t best_j = i == 0 ? 1u : i - 1u;
    const uint32_t pair = i ^ 1u; // (always within the window: r >= 1; past the end for the last of an odd m)
    for (uint32_t j = j0; j <= j1; j++) {
        if (j == i) continue;
        Aabb u = bi;
        grow(u, box_at(j));
        const float a = half_area(u);
        if (j == pair) pair_area = a;
        if (a < best) { // first of equals: the lowest index ...
            best = a;
            best_j = j;
        }
    }
    // ... unless the pair partner i ^ 1 is one of the equals: then i and i ^ 1 choose each other whenever neither has a
    // strictly better neighbour, so a run of tied clusters (duplicates, boxes without area, areas that are all 0 or all
    // +inf) halves every round.  With the lowest index alone every cluster of such a run points at i - r, only the first
    // two are mutual, and the tree becomes a chain built in O(n) rounds.  A cluster whose candidate areas are all different
    // chooses as before.
    if (pair_area == best) best_j = pair;
    return best_j;
}

// ---- BVH2 -> 8-wide collapse (Ylitie et al. 2017, section 4.2) ---------------------------------------------------------
// The seven decisions of a node of half-area `area` over `count` primitives; cl[k] / cr[k]: cost of decision k of its left
// / right child (not read for a leaf).
TRX_HD inline void collapse_costs(float area, uint32_t count, const float *cl, const float *cr, uint32_t max_prims, float traversal_cost,
                                  float prim_cost, Decision *out) {
    if (count == 1) {
        for (int i = 0; i < 7; i++) out[i] = Decision{area * prim_cost, kLeaf, 0xff, 0xff, 0};
        return;
    }
    const float cost_leaf = count <= max_prims ? area * (float)count * prim_cost : INFINITY;
    float cost_dist = INFINITY;
    // (1 + 7 slots unless a split costs less: where the children's costs have overflowed to +inf none does, and a 0xff here
    // would send collapsed_children to decision 255 of the children - another node's entries)
    uint8_t bl = 0, br = 6;
    for (int k = 0; k < 7; k++) {
        const float c = cl[k] + cr[6 - k];
        if (c < cost_dist) {
            cost_dist = c;
            bl = (uint8_t)k;
            br = (uint8_t)(6 - k);
        }
    }
    const float cost_internal = cost_dist + area * traversal_cost;
    Decision prev = cost_leaf < cost_internal ? Decision{cost_leaf, kLeaf, bl, br, 0} : Decision{cost_internal, kInternal, bl, br, 0};
    out[0] = prev;
    for (int i = 1; i < 7; i++) {
        float best = prev.cost;
        uint8_t l = 0xff, r = 0xff;
        for (int k = 0; k < i; k++) {
            const float c = cl[k] + cr[i - k - 1];
            if (c < best) {
                best = c;
                l = (uint8_t)k;
                r = (uint8_t)(i - k - 1);
            }
        }
        if (l != 0xff) prev = Decision{best, kDistribute, l, r, 0};
        out[i] = prev;
    }
}

// The BVH2 nodes that become the children of the 8-wide node made from ni, left to right (distribute decisions followed);
// returns how many, of which the first eight are in `children` (more than eight: the table is not one collapse_costs
// wrote).  node_links(n, left, right, count) fetches a node's links, decision_at(k) entry k of the table (7 * node + i).
template <class Links, class DecisionAt>
TRX_HD inline int collapsed_children(uint32_t ni, Links node_links, DecisionAt decision_at, uint32_t *children) {
    // pending visits, the next one on top: {node, decision index | expand flag << 8}
    uint32_t st_n[16], st_i[16];
    int sp = 0, count = 0;
    st_n[0] = ni;
    st_i[0] = 0x100u;
    sp = 1;
    while (sp > 0) {
        sp--;
        const uint32_t n = st_n[sp], ii = st_i[sp];
        if (!(ii & 0x100u)) {
            if (count < 8) children[count] = n;
            count++;
            continue;
        }
        uint32_t left, right, cnt;
        node_links(n, left, right, cnt);
        if (cnt == 1) {
            if (count < 8) children[count] = n;
            count++;
            continue;
        }
        const Decision d = decision_at((size_t)n * 7 + (ii & 0xffu));
        const bool xr = decision_at((size_t)right * 7 + d.dr).type == kDistribute;
        const bool xl = decision_at((size_t)left * 7 + d.dl).type == kDistribute;
        if (sp + 2 > 16) return 9; // cannot happen: at most eight children, a pending visit per child
        st_n[sp] = right;
        st_i[sp] = xr ? (0x100u | d.dr) : 0u;
        sp++;
        st_n[sp] = left;
        st_i[sp] = xl ? (0x100u | d.dl) : 0u;
        sp++;
    }
    return count;
}

// Greedy octant-slot assignment (embree/src/bvh_embree.rs:284-349): slot_child[s] = which of the `count` children goes to
// slot s, or -1.  child_box_at(c) is child c's box.
template <class BoxAt>
TRX_HD inline void assign_slots(const Aabb &box, BoxAt child_box_at, int count, int *slot_child) {
    const float pc[3] = {0.5f * (box.mn[0] + box.mx[0]), 0.5f * (box.mn[1] + box.mx[1]), 0.5f * (box.mn[2] + box.mx[2])};
    float cost[8][8];
    for (int c = 0; c < count; c++) {
        const Aabb cb = child_box_at(c);
        const float d[3] = {0.5f * (cb.mn[0] + cb.mx[0]) - pc[0], 0.5f * (cb.mn[1] + cb.mx[1]) - pc[1], 0.5f * (cb.mn[2] + cb.mx[2]) - pc[2]};
        for (int s = 0; s < 8; s++) {
            const float sx = (s & 4) ? -1.f : 1.f, sy = (s & 2) ? -1.f : 1.f, sz = (s & 1) ? -1.f : 1.f;
            cost[c][s] = d[0] * sx + d[1] * sy + d[2] * sz;
        }
    }
    int assignment[8];
    bool filled[8];
    for (int c = 0; c < 8; c++) {
        assignment[c] = -1;
        filled[c] = false;
        slot_child[c] = -1;
    }
    for (;;) {
        float min_cost = 3.402823466e+38f;
        int min_slot = -1, min_index = -1;
        for (int c = 0; c < count; c++) {
            if (assignment[c] != -1) continue;
            for (int s = 0; s < 8; s++) {
                if (!filled[s] && cost[c][s] < min_cost) {
                    min_cost = cost[c][s];
                    min_slot = s;
                    min_index = c;
                }
            }
        }
        if (min_slot < 0) break;
        filled[min_slot] = true;
        assignment[min_index] = min_slot;
    }
    for (int c = 0; c < count; c++) {
        int s = assignment[c];
        if (s < 0) { // non-finite centre: first free slot
            for (s = 0; s < 8 && filled[s]; s++) {}
            if (s > 7) s = 7;
            filled[s] = true;
        }
        slot_child[s] = c;
    }
}

// ---- node encoding (embree/src/bvh_embree_to_cwbvh.rs:85-186) -----------------------------------------------------------
// Origin of one axis of a node's frame: the box minimum, a zero minimum always as +0.  Which zero a box minimum keeps
// depends on the order its contents were folded in (rf_min keeps the first of equals), and the builders fold in merge
// order where the refit folds in slot order; the bytes must not.  -0 would also cost the scene the exact shortcut of
// origins that are +0 or 2^-36 <= |p| <= 2^59 (trx_scene_create, exp_exact == 2) for nothing.
TRX_HD inline float frame_origin(float mn) { return mn == 0.0f ? 0.0f : mn; }

// Quantisation step of one axis of a node whose box spans [mn, mx].
TRX_HD inline float quant_step(float mn, float mx) {
    // the smallest power of two >= x = max(extent, 1e-20) / 255, read off x's bits (what frexp / ldexp give: ldexp(1, k) for
    // x = m * 2^k, one less where m is exactly 0.5).  A box wider than FLT_MAX has extent +inf although its planes are
    // finite: frexp leaves the exponent 0 there, so the step starts at 1 and the loop below finds the finite one.
    const float extent = mx - mn;
    const float x = (extent < 1e-20f ? 1e-20f : extent) * (1.0f / 255.0f);
    const uint32_t xb = rf_bits(x);
    float e = (xb & 0x7f800000u) == 0x7f800000u ? 1.0f : rf_float((xb & 0x7fffffu) ? ((xb >> 23) + 1u) << 23 : xb);
    // make sure 255 steps reach the far plane after rounding
    while (ceil(((double)mx - (double)mn) / (double)e) > 255.0) e *= 2.0f;
    return e;
}

// ... and the two planes of a child box [cmn, cmx] in the frame of origin p and step e.
TRX_HD inline void quant_planes(float p, float e, float cmn, float cmx, uint32_t &qlo, uint32_t &qhi) {
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

// child_meta of slot s: an inner child, or a leaf of `count` (1..3) triangles starting `first` triangles into the node's own
TRX_HD inline uint8_t inner_meta(int s) { return (uint8_t)((24 + s) | 0x20); }
TRX_HD inline uint8_t leaf_meta(uint32_t first, uint32_t count) {
    const uint32_t unary = count == 1 ? 0x20u : count == 2 ? 0x60u : count == 3 ? 0xE0u : 0u;
    return (uint8_t)(first | unary);
}
TRX_HD inline uint32_t leaf_count(uint8_t m) {
    const uint32_t bits = m >> 5;
    return bits == 1 ? 1u : bits == 3 ? 2u : bits == 7 ? 3u : 0u;
}

} // namespace trx
