// kernels.hip — gfx950 (MI355X, wave64) CWBVH closest-hit kernels.
//
// One persistent wave = 64 ray slots.  Waves pull 64-item chunks (an 8x8 pixel
// tile, or 64 explicit rays) from one work queue per XCD, heaviest tiles first
// (order filed by the first frame of a view from each tile's measured work), traverse with a
// per-lane stack striped through LDS (entry i of lane l at [i*64 + l]:
// conflict-free ds_write_b64/ds_read_b64) that spills to HBM past kLdsStack
// entries, and run the triangle tests of a node step cooperatively: the wave's
// (ray, triangle) pairs are spread over all 64 lanes and committed by their
// owners in order.  DESIGN.md section 4 has the measurements behind each choice.
//
// What each function restates (paths relative to the tray_racing checkout):
//   node_intersect   src/rt_gpu/rt_gpu_software_query.hlsl:213-303
//   tri test         src/rt_gpu/rt_gpu_software_query.hlsl:89-129
//   traversal        src/rt_gpu/rt_gpu_software_query.hlsl:328-438,
//                    src/rt_gpu/rt_gpu_software_query_tlas.hlsl:333-500
//   primary ray      src/rt_gpu/rt_gpu_software.hlsl:69-80, src/rt_cpu/rt_cpu.rs:38-55
//   AO ray           src/rt_gpu/rt_gpu_software.hlsl:105-121, src/rt_cpu/rt_cpu.rs:61-76,
//                    src/rt_gpu/sampling.hlsl:5-51
//
// What k_trace shares with the small kernels at the end of this file (k_hit_attr, k_ao_rays, k_ao_reduce) is stated once:
// TRX_AO_RAY (the AO ray of a primary hit), normal_to_world and TRX_RAY_TO_OBJECT (an instance's rows), and inside k_trace
// TRX_PUBLISH_RAY (a lane's ray into LDS).  Where such a statement is a macro, the function form was built and changed the
// register assignment of some k_trace instantiation; the comment at the macro says which.
//
// Arithmetic contract (DESIGN.md "Numerics"): binary32, no contraction
// (-ffp-contract=off; the only fused op is the explicit fmaf of
// TRX_SEM_NODE_FMA), IEEE divide and sqrt, dot = (ax*bx + ay*by) + az*bz.
#include "kernels.h"

#ifndef TRX_NODE_UNROLL
#define TRX_NODE_UNROLL 2
#endif

#pragma clang fp contract(off)

// Diagnostic builds (never the product): TRX_DEV_TUNE = run-time experiment switches (TraceParams::tune), TRX_TAIL_DIAG =
// what every wave did last and when, TRX_STAMPS = per-wave cycle accounting of the loop's phases (every stamp drains the
// memory counters first, so a phase owns the latency of what it issued).  They are compile-time flags tested with
// `if constexpr` / plain `if` on a constant - the product build folds every such branch away (same instructions as
// without them: build/kernels.s is compared) - instead of preprocessor blocks woven through the walk.
#ifdef TRX_DEV_TUNE
#define TRX_K_TUNE true
#else
#define TRX_K_TUNE false
#endif
#ifdef TRX_TAIL_DIAG
#define TRX_K_TAIL true
#else
#define TRX_K_TAIL false
#endif
#ifdef TRX_STAMPS
#define TRX_K_STAMPS true
#else
#define TRX_K_STAMPS false
#endif
#define TRX_STAMP(acc)                                                  \
    do {                                                                \
        if constexpr (kStamps) {                                        \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
            acc += now_ - stamp_prev;                                   \
            stamp_prev = now_;                                          \
        }                                                               \
    } while (0)

// k_trace: a lane's ray where the cooperative triangle rounds read it - {o, tmin}, {d, 0} in the wave's table in LDS.  Text:
// as a lambda beside finish_lane the walks that call it from inside other lambdas (thin walk, drain) come out in other
// registers; one expression, not a do { } while (0): a loop statement renumbers the kernel's jump destinations.
#define TRX_PUBLISH_RAY()                                                      \
    ((void)(lds_ray[2u * lane] = make_float4(r.ox, r.oy, r.oz, r.tmin)),       \
     (void)(lds_ray[2u * lane + 1u] = make_float4(r.dx, r.dy, r.dz, 0.0f)))

namespace trx {
namespace {

// __ballot() takes an int: a bool that lives as a lane mask is first turned into 0 / 1 per lane and compared again (two
// vector instructions where the mask was already there); the builtin takes the bool
__device__ __forceinline__ unsigned long long ballot64(bool b) { return __builtin_amdgcn_ballot_w64(b); }

constexpr bool kTune = TRX_K_TUNE, kTailDiag = TRX_K_TAIL, kStamps = TRX_K_STAMPS;

#define TRX_F32_MAX 3.402823466e+38f
#define TRX_F32_EPSILON 1.1920929e-7f
#define TRX_INVALID 0xFFFFFFFFu

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

struct Ray {
    float ox, oy, oz;
    float dx, dy, dz;    // after the zero-direction fix (query.hlsl:334)
    float ix, iy, iz;    // 1/d, IEEE divide (TRX_SEM_NODE_RCP)
    float tmin;
    uint32_t oct_inv4;
};

// NODE bit0: multiply by precomputed reciprocal, bit1: fused plane evaluation
template <int NODE>
__device__ __forceinline__ float plane(float q, float a, float b) {
    if (NODE & 2) return __builtin_fmaf(q, a, b);
    return q * a + b;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Four registers with no defined contents (a frozen undef: costs no instruction), for values that only the lanes
// which go on to load them will read.
__device__ __forceinline__ float4 unspecified4() {
    f32x4 v;
    v = __builtin_nondeterministic_value(v);
    return make_float4(v.x, v.y, v.z, v.w);
}
// ... and one (the plain walk's per-trip words: a `= 0` at the head of the trip is a v_mov in every trip).  An empty
// asm statement's output, not a frozen undef: where the value meets a computed one at a join the compiler gives a
// frozen undef the value 0, and that is the v_mov again.  (volatile: not hoisted out of the loop, where it would hold
// a register for the whole walk)
__device__ __forceinline__ uint32_t unspecified1() {
    uint32_t v;
    asm volatile("" : "=v"(v));
    return v;
}

// two planes at once: q * a + b on both halves (separate roundings unless NODE & 2)
template <int NODE>
__device__ __forceinline__ f32x2 plane2(f32x2 q, float a, float b) {
    const f32x2 a2 = {a, a}, b2 = {b, b};
    if (NODE & 2) return __builtin_elementwise_fma(q, a2, b2);
    return q * a2 + b2;
}

__device__ __forceinline__ float ubyte(uint32_t x, int j) { return (float)((x >> (8 * j)) & 0xffu); }

// The quantisation frame of a node as the ray sees it (query.hlsl:237-243): a = e / d, b = (p - o) / d per axis, in the
// arithmetic the NODE variant asks for - shared by the three node tests below (per lane, decode-once, children-per-lane).
// A macro, not a function: it declares ax .. bz in the test that uses it (as a function with reference parameters the
// compiler schedules the tests differently; as text the product's instructions are those of the three written-out copies).
//   pow2: the shader divides per node (query.hlsl:237-243).  e is a power of two, and a correctly rounded quotient
// scales exactly with powers of two: RN(2^k / d) = 2^k * RN(1 / d) bit for bit, as long as neither side leaves
// the normal range - which pow2_exact() below guarantees from the ray (every |d| normal and <= 2^20) and the
// scene (every exponent byte 0 or >= 21); overflow to infinity happens to both sides at the same threshold.
// Three of the six IEEE divisions of a node step become multiplications by the ray's 1/d.
//   The other three, b = (p - o) / d, have a numerator that is no power of two.  With y = RN(1 / d) - the ray's r.ix, an IEEE
// division at ray set-up - the correctly rounded quotient takes ONE correction step (Markstein): q0 = RN(a y),
// rem = a - d q0 (exact in one fma), q = RN(q0 + rem y) = RN(a / d), as long as no intermediate leaves the normal range
// (div_by_rcp: three instructions where the compiler's `/` is eleven).  Whether the identity holds depends on the two
// significands only - scaling by powers of two commutes with every step - and tools/ubench/div_exhaustive.hip checks
// all 2^46 pairs of them on the GPU against `/` (profiles/r05_div_exhaustive.log: 0 mismatches in 7.04e13), plus 2^36
// random pairs over the admitted exponents and zero numerators.  Admitted: 2^-30 <= |d| <= 2^20 and a = +0 or
// 2^-60 <= |a| <= 2^60 - every product, remainder and quotient then stays between 2^-127+24 and 2^127; a = +0 comes out
// as the zero of the right sign (worked through in DESIGN.md section 3), a = -0 would not.  Nothing of that is looked
// at per node step: the RAY carries a flag (finish_ray_dir: every origin component 0 or 2^-36 <= |o| <= 2^59) and the
// SCENE one (trx_scene_create in api.cpp, exp_exact = 2: every component of every node's p is +0 or 2^-36 <= |p| <= 2^59), and the
// difference of two such floats is +0 or a multiple of 2^-59 no larger than 2^60.  shortcut = 2: both shortcuts for
// this step (every lane that takes it), 1: the power-of-two one only, 0: the shader's six divisions.
// RN(a / d) from y = RN(1 / d): see above for when
__device__ __forceinline__ float div_by_rcp(float a, float d, float y) {
    const float q0 = a * y;
    const float rem = __builtin_fmaf(-d, q0, a);
    return __builtin_fmaf(rem, y, q0);
}
#define TRX_NODE_FRAME(r, n0, pow2)                                                                         \
    const float px = __uint_as_float(n0.x), py = __uint_as_float(n0.y), pz = __uint_as_float(n0.z);         \
    const uint32_t e_imask = n0.w;                                                                          \
    const float ex = __uint_as_float((e_imask & 0xffu) << 23);                                              \
    const float ey = __uint_as_float(((e_imask >> 8) & 0xffu) << 23);                                       \
    const float ez = __uint_as_float(((e_imask >> 16) & 0xffu) << 23);                                      \
    float ax, ay, az, bx, by, bz;                                                                           \
    if (NODE & 1) {                                                                                         \
        ax = ex * r.ix;                                                                                     \
        ay = ey * r.iy;                                                                                     \
        az = ez * r.iz;                                                                                     \
        bx = (px - r.ox) * r.ix;                                                                            \
        by = (py - r.oy) * r.iy;                                                                            \
        bz = (pz - r.oz) * r.iz;                                                                            \
    } else if (pow2) {                                                                                      \
        ax = ex * r.ix;                                                                                     \
        ay = ey * r.iy;                                                                                     \
        az = ez * r.iz;                                                                                     \
        if (pow2 > 1) {                                                                                     \
            bx = div_by_rcp(px - r.ox, r.dx, r.ix);                                                         \
            by = div_by_rcp(py - r.oy, r.dy, r.iy);                                                         \
            bz = div_by_rcp(pz - r.oz, r.dz, r.iz);                                                         \
        } else {                                                                                            \
            bx = (px - r.ox) / r.dx;                                                                        \
            by = (py - r.oy) / r.dy;                                                                        \
            bz = (pz - r.oz) / r.dz;                                                                        \
        }                                                                                                   \
    } else {                                                                                                \
        ax = ex / r.dx;                                                                                     \
        ay = ey / r.dy;                                                                                     \
        az = ez / r.dz;                                                                                     \
        bx = (px - r.ox) / r.dx;                                                                            \
        by = (py - r.oy) / r.dy;                                                                            \
        bz = (pz - r.oz) / r.dz;                                                                            \
    }

template <int NODE>
__device__ __forceinline__ uint32_t node_intersect(const Ray &r, float max_distance, const uint4 n0,
                                                   const uint4 n1, const uint4 n2, const uint4 n3,
                                                   const uint4 n4, const int pow2) {
    TRX_NODE_FRAME(r, n0, pow2)
    const bool nx = r.dx < 0.0f, ny = r.dy < 0.0f, nz = r.dz < 0.0f;
    uint32_t hit_mask = 0;
#pragma unroll TRX_NODE_UNROLL
    for (int i = 0; i < 2; i++) {
        const uint32_t meta4 = i == 0 ? n1.z : n1.w;
        const uint32_t is_inner4 = (meta4 & (meta4 << 1)) & 0x10101010u;
        const uint32_t inner_mask4 = (is_inner4 >> 4) * 0xffu;
        const uint32_t bit_index4 = (meta4 ^ (r.oct_inv4 & inner_mask4)) & 0x1f1f1f1fu;
        const uint32_t child_bits4 = (meta4 >> 5) & 0x07070707u;
        const uint32_t q_lo_x = i == 0 ? n2.x : n2.y, q_hi_x = i == 0 ? n2.z : n2.w;
        const uint32_t q_lo_y = i == 0 ? n3.x : n3.y, q_hi_y = i == 0 ? n3.z : n3.w;
        const uint32_t q_lo_z = i == 0 ? n4.x : n4.y, q_hi_z = i == 0 ? n4.z : n4.w;
        const uint32_t x_min = nx ? q_hi_x : q_lo_x, x_max = nx ? q_lo_x : q_hi_x;
        const uint32_t y_min = ny ? q_hi_y : q_lo_y, y_max = ny ? q_lo_y : q_hi_y;
        const uint32_t z_min = nz ? q_hi_z : q_lo_z, z_max = nz ? q_lo_z : q_hi_z;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // the near and far plane of one axis go through the same multiply and add: as a float2
            // they are one v_pk_mul_f32 + one v_pk_add_f32 (two IEEE operations per lane in the issue
            // slot of one), or one v_pk_fma_f32; the VALU issue rate is what bounds this kernel
            const f32x2 tx = plane2<NODE>(f32x2{ubyte(x_min, j), ubyte(x_max, j)}, ax, bx);
            const f32x2 ty = plane2<NODE>(f32x2{ubyte(y_min, j), ubyte(y_max, j)}, ay, by);
            const f32x2 tz = plane2<NODE>(f32x2{ubyte(z_min, j), ubyte(z_max, j)}, az, bz);
            const float tmin = fmaxf(fmaxf(fmaxf(tx.x, ty.x), tz.x), 0.0001f);
            const float tmax = fminf(fminf(fminf(tx.y, ty.y), tz.y), max_distance);
            if (tmin <= tmax) {
                const uint32_t child_bits = (child_bits4 >> (8 * j)) & 0xffu;
                const uint32_t bit_index = (bit_index4 >> (8 * j)) & 0xffu;
                hit_mask |= child_bits << bit_index;
            }
        }
    }
    return hit_mask;
}

// A wave-uniform node step (every lane visits the same node) converts the child planes to floats ONCE for the wave: the
// 48 byte-to-float conversions and the 12 near / far selects of the per-lane test are the same work 64 times over.  Two
// tables in LDS, [3 axes][8 children][2]: dec_pos holds {min, max} of a child's axis, dec_neg {max, min}; a lane picks
// the table of an axis by ADDRESS (the sign of its direction: the near plane is the max plane when the direction is
// negative) - every lane of a sign class reads the same bytes, which LDS broadcasts - so that each {near, far} pair
// arrives in the two consecutive registers the packed arithmetic of plane2 wants.  (Until round 4 the table was
// plane-major and the pairs were put together with two register moves each: 37 moves in a 178-instruction test.)
//
// The decode-once test over the children a PACKET test left (round 5).  In a wave-uniform node step of coherent primary
// rays most of the eight children are missed by every ray of the wave (bistro-class frame: 1.65 children left on average,
// none in a fifth of the steps; profiles/r05_cullhist.log).  The packet test (trace_walk_plain.inc): with the rays' common
// origin and bounds [lo, hi] of their 1/d per axis, each {child, plane} lane of the decode stage also evaluates the
// plane's parameter at the end of the interval that bounds it from below (near planes) or above (far planes) - the
// SAME multiplications and additions as the per-ray test, at operands that bound every ray's: round-to-nearest
// multiplication and addition are monotone in each operand, so the values bound what any ray of the wave computes - and
// a child whose largest lower bound exceeds its smallest upper bound is entered by no ray: it is left out for the whole
// wave.  This function is the per-ray test of the children that remain (`keep`, wave-uniform, bit c = child c): the
// operations of node_intersect on the same operands, child by child in a scalar loop; a child left out would have
// contributed nothing to the mask.  keep = 0xff: all eight (a wave whose rays do not qualify for the packet test).
//   The literal-division variants (NODE bit 0 clear) take part where a step's rays all take both division shortcuts
// (shortcut level 2: a = e RN(1/d) as here, b = RN(c / d) by div_by_rcp).  RN(c / d) is within 3 x 2^-24 (relative) of
// RN(c RN(1/d)), the value the bounds are computed from, so the packet test widens the b interval by 2^-21 of its ends'
// magnitudes (nothing is near the subnormals there: the level-2 flags keep |c| in 2^-60 .. 2^60 or zero, and a zero c gives
// a zero b on both sides); a is the same product in both variants.
struct NodeFrame {
    float ax, ay, az, bx, by, bz;
};
template <int NODE>
__device__ __forceinline__ NodeFrame node_frame(const Ray &r, uint4 n0, const int pow2) {
    // (every lane holds the same record: the exponent word is a scalar, its three scale words are formed by the scalar
    // unit - six shifts and ands a lane otherwise - and the multiplications take them as scalar operands; the same floats)
    n0.w = (uint32_t)__builtin_amdgcn_readfirstlane((int)n0.w);
    TRX_NODE_FRAME(r, n0, pow2)
    return NodeFrame{ax, ay, az, bx, by, bz};
}
template <int NODE>
__device__ __forceinline__ uint32_t node_intersect_kept(const Ray &r, float max_distance, const NodeFrame f, const uint4 n1,
                                                        const float *dec_pos, const float *dec_neg, uint32_t keep) {
    float ax = f.ax, ay = f.ay, az = f.az, bx = f.bx, by = f.by, bz = f.bz;
    const float2 *const qx = reinterpret_cast<const float2 *>(r.dx < 0.0f ? dec_neg : dec_pos);
    const float2 *const qy = reinterpret_cast<const float2 *>((r.dy < 0.0f ? dec_neg : dec_pos) + 16);
    const float2 *const qz = reinterpret_cast<const float2 *>((r.dz < 0.0f ? dec_neg : dec_pos) + 32);
    // (the node is the same for every lane: its child_meta bytes are scalars, and so is everything derived from them but
    // the slot of an inner child, which depends on the ray's octant)
    const uint32_t meta_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)n1.z), meta_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)n1.w);
    const uint32_t oct = r.oct_inv4 & 0xffu;
    uint32_t hit_mask = 0;
    // (the eight meta bytes as ONE scalar pair: a child's byte is one 64-bit shift, not a compare, a select and a shift;
    // and a step whose packet test leaves no child - one in five - is the branch that is taken, so that the loop's exit
    // falls through into what follows.  profiles/walk_scalar_cost.log)
    const unsigned long long meta = ((unsigned long long)meta_hi << 32) | meta_lo;
    if (__builtin_expect(keep == 0u, 0)) return 0u;
    // (requesting the planes of the next child before this one's are used - the loop software-pipelined - measured slower,
    // profiles/r05_ab_19_cull_pipelined.log)
    for (uint32_t m = keep; m != 0u; m &= m - 1u) {
        const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__builtin_ctz(m))); // (wave-uniform: a scalar)
        const float2 x = qx[j], y = qy[j], z = qz[j]; // {near, far}
        // (no instruction: the six operands are redefined inside the loop's block, where instruction selection sees the
        // pairs {a, a}, {b, b} of plane2 and takes both halves from one register, op_sel_hi, as in node_intersect; formed
        // ahead of the loop they were six register moves a step)
        asm("" : "+v"(ax), "+v"(ay), "+v"(az), "+v"(bx), "+v"(by), "+v"(bz));
        const f32x2 tx = plane2<NODE>(f32x2{x.x, x.y}, ax, bx);
        const f32x2 ty = plane2<NODE>(f32x2{y.x, y.y}, ay, by);
        const f32x2 tz = plane2<NODE>(f32x2{z.x, z.y}, az, bz);
        const float tmin = fmaxf(fmaxf(fmaxf(tx.x, ty.x), tz.x), 0.0001f);
        const float tmax = fminf(fminf(fminf(tx.y, ty.y), tz.y), max_distance);
        const uint32_t mj = (uint32_t)(meta >> (8u * j)) & 0xffu;
        const uint32_t child_bits = mj >> 5;
        // child_bits << bit_index with bit_index = (meta ^ (oct & inner_mask)) & 0x1f, as in node_intersect
        uint32_t word;
        if ((mj & 0x18u) == 0x18u) word = child_bits << ((mj ^ oct) & 0x1fu);
        else word = child_bits << (mj & 0x1fu);
        if (tmin <= tmax) hit_mask |= word;
    }
    return hit_mask;
}

// C consecutive CHILDREN of a node.  The thin walk calls it with C = 1: the eight lanes that share a ray take a child each
// (two and four children to a lane were built and declined with the four- and two-lane walks, trace_thin.inc).  The loop over
// one child stays as written: without it the same operations reach the scheduler in another order and every kernel with a
// thin walk comes out in other registers.  The same IEEE operations on the same operands as the per-child body of
// node_intersect: this lane's contribution to the hit mask, child_bits << bit_index for every child of its share whose box
// the ray enters.  q = the six plane words of the share, C bytes each, in the order {x near, x far, y near, y far, z near,
// z far} (near = the max plane where the direction is negative); meta = its C child_meta bytes.
template <int NODE, int C>
__device__ __forceinline__ uint32_t node_children_intersect(const Ray &r, float max_distance, const uint4 n0, uint32_t meta,
                                                            const uint32_t q[6], const int pow2) {
    TRX_NODE_FRAME(r, n0, pow2)
    const uint32_t is_inner4 = (meta & (meta << 1)) & 0x10101010u;
    const uint32_t inner_mask4 = (is_inner4 >> 4) * 0xffu;
    const uint32_t bit_index4 = (meta ^ (r.oct_inv4 & inner_mask4)) & 0x1f1f1f1fu;
    const uint32_t child_bits4 = (meta >> 5) & 0x07070707u;
    uint32_t hit_mask = 0u;
#pragma unroll
    for (int j = 0; j < C; j++) {
        const f32x2 tx = plane2<NODE>(f32x2{ubyte(q[0], j), ubyte(q[1], j)}, ax, bx);
        const f32x2 ty = plane2<NODE>(f32x2{ubyte(q[2], j), ubyte(q[3], j)}, ay, by);
        const f32x2 tz = plane2<NODE>(f32x2{ubyte(q[4], j), ubyte(q[5], j)}, az, bz);
        const float tmin = fmaxf(fmaxf(fmaxf(tx.x, ty.x), tz.x), 0.0001f);
        const float tmax = fminf(fminf(fminf(tx.y, ty.y), tz.y), max_distance);
        if (tmin <= tmax) hit_mask |= ((child_bits4 >> (8 * j)) & 0xffu) << ((bit_index4 >> (8 * j)) & 0xffu);
    }
    return hit_mask;
}

// Groups of eight lanes (thin waves): the value of a group's first lane in all of them, and the OR of all of them in the
// first - both on the DPP network (VALU only).  Every lane of the wave must be active.
__device__ __forceinline__ uint32_t group_first(uint32_t v) {
    const uint32_t q = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x00, 0xf, 0xf, false);  // quad_perm [0,0,0,0]
    const uint32_t h = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q, 0x114, 0xf, 0xf, false); // row_shr:4
    return (__lane_id() & 4u) ? h : q;
}
__device__ __forceinline__ uint32_t group_or_to_first(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true); // row_shl:1 (0 past the row's end)
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x102, 0xf, 0xf, true); // row_shl:2
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0xf, true); // row_shl:4
    return v; // (complete in the first lane of every group; the others hold partial ORs)
}

// TriDev = {v0, e1 = v0 - v1, e2 = v2 - v0} as three float4; ng = cross(e1, e2) (query.hlsl:93) rides in the
// w lanes, evaluated at upload exactly as written there.
template <bool EARLY = false>
__device__ __forceinline__ bool intersect_tri(const Ray &r, const float4 a, const float4 b, const float4 c4,
                                              float &t, bool tie_first) {
    const float e1x = b.x, e1y = b.y, e1z = b.z;
    const float e2x = c4.x, e2y = c4.y, e2z = c4.z;
    const float ngx = a.w, ngy = b.w, ngz = c4.w;
    const float cx = a.x - r.ox, cy = a.y - r.oy, cz = a.z - r.oz;
    const float rx = r.dy * cz - r.dz * cy;
    const float ry = r.dz * cx - r.dx * cz;
    const float rz = r.dx * cy - r.dy * cx;
    const float det = dot3(ngx, ngy, ngz, r.dx, r.dy, r.dz);
    const float un = dot3(rx, ry, rz, e2x, e2y, e2z), vn = dot3(rx, ry, rz, e1x, e1y, e1z);
    if (EARLY) {
        // u = un * (1 / det) and v = vn * (1 / det) carry the sign bits sign(un) ^ sign(det), sign(vn) ^ sign(det)
        // whatever the magnitudes (a product's sign is the XOR of its operands', 1 / x keeps the sign of x, also
        // for zeros and infinities); where a NaN appears the test below rejects anyway.  A set sign bit rejects the
        // triangle (query.hlsl:111-116), so when NO lane of the wave can still accept, the IEEE divide, w, tt and the
        // range test are skipped for the whole wave.  Lanes that go on compute exactly what they always did.
        const uint32_t neg = ((__float_as_uint(un) ^ __float_as_uint(det)) | (__float_as_uint(vn) ^ __float_as_uint(det))) & 0x80000000u;
        if (__ballot(neg == 0u) == 0ull) return false;
    }
    const float inv_det = 1.0f / det;
    const float u = un * inv_det;
    const float v = vn * inv_det;
    const float w = 1.0f - u - v;
    const uint32_t hit = __float_as_uint(u) | __float_as_uint(v) | __float_as_uint(w);
    if (inv_det != 0.0f && (hit & 0x80000000u) == 0) {
        const float tt = dot3(ngx, ngy, ngz, cx, cy, cz) * inv_det;
        // (tie_first ? tt < t : tt <= t, written so that the wave-uniform flag is a scalar mask operation: as a select
        // between the two comparisons it compiles to five vector instructions per test)
        const bool lt = tt < t, eq = tt == t;
        const bool closer = lt | (eq & !tie_first); // (bitwise: no short-circuit branches)
        if ((tt >= r.tmin) & closer) {
            t = tt;
            return true;
        }
    }
    return false;
}


// (LITERAL: a node test that divides - the flags are only looked at there)
template <bool LITERAL>
__device__ __forceinline__ void finish_ray_dir(Ray &r, float dx, float dy, float dz) {
    r.dx = dx == 0.0f ? TRX_F32_EPSILON : dx;
    r.dy = dy == 0.0f ? TRX_F32_EPSILON : dy;
    r.dz = dz == 0.0f ? TRX_F32_EPSILON : dz;
    r.ix = 1.0f / r.dx;
    r.iy = 1.0f / r.dy;
    r.iz = 1.0f / r.dz;
    r.oct_inv4 = (r.dx < 0.0f ? 0u : 0x04040404u) | (r.dy < 0.0f ? 0u : 0x02020202u) |
                 (r.dz < 0.0f ? 0u : 0x01010101u);
    if (!LITERAL) return;
    // bits 31 and 30 (masked out wherever oct_inv4 is used) switch the literal-division shortcuts of TRX_NODE_FRAME off:
    // bit 31 - a direction component outside 2^-30 .. 2^20 (or NaN): this ray divides six times per node like the shader's
    // text (e / d = e * (1/d) needs |d| normal and <= 2^20; the lower bound is the tighter one of div_by_rcp);
    // bit 30 - an origin component that is neither 0 nor within 2^-36 .. 2^59: (p - o) / d is divided
    const float lo = 0x1p-30f, hi = 1048576.0f; // a NaN fails both
    const bool exact = fabsf(r.dx) >= lo && fabsf(r.dx) <= hi && fabsf(r.dy) >= lo && fabsf(r.dy) <= hi &&
                       fabsf(r.dz) >= lo && fabsf(r.dz) <= hi;
    if (!exact) r.oct_inv4 |= 0x80000000u;
    const float olo = 0x1p-36f, ohi = 0x1p59f;
    const bool org = (r.ox == 0.0f || (fabsf(r.ox) >= olo && fabsf(r.ox) <= ohi)) && (r.oy == 0.0f || (fabsf(r.oy) >= olo && fabsf(r.oy) <= ohi)) &&
                     (r.oz == 0.0f || (fabsf(r.oz) >= olo && fabsf(r.oz) <= ohi));
    if (!org) r.oct_inv4 |= 0x40000000u;
}

// Wave-uniform: which shortcuts may this node step of the literal-division variants take (TRX_NODE_FRAME: 0, 1 or 2)?
__device__ __forceinline__ int pow2_exact(const TraceParams &P, const Ray &r, bool act) {
    if (P.exp_exact == 0u) return 0;
    if (__ballot(act && (r.oct_inv4 >> 30) != 0u) == 0ull) return (int)P.exp_exact;
    return __ballot(act && (r.oct_inv4 >> 31) != 0u) == 0ull ? 1 : 0;
}

__device__ __forceinline__ void mat4_mul(const float *m, float v0, float v1, float v2, float v3, float &r0,
                                         float &r1, float &r2, float &r3) {
    r0 = ((m[0] * v0 + m[4] * v1) + m[8] * v2) + m[12] * v3;
    r1 = ((m[1] * v0 + m[5] * v1) + m[9] * v2) + m[13] * v3;
    r2 = ((m[2] * v0 + m[6] * v1) + m[10] * v2) + m[14] * v3;
    r3 = ((m[3] * v0 + m[7] * v1) + m[11] * v2) + m[15] * v3;
}

__device__ __forceinline__ void primary_dir(const ViewDev &view, uint32_t w, uint32_t h, uint32_t px,
                                            uint32_t py, float &dx, float &dy, float &dz) {
    const float u = (float)px / (float)w;
    float v = (float)py / (float)h;
    v = 1.0f - v;
    const float cx = u * 2.0f - 1.0f, cy = v * 2.0f - 1.0f;
    float vx, vy, vz, vw;
    mat4_mul(view.proj_inv, cx, cy, 1.0f, 1.0f, vx, vy, vz, vw);
    const float s = vw;
    vx = vx / s;
    vy = vy / s;
    vz = vz / s;
    vw = vw / s;
    float wx, wy, wz, ww;
    mat4_mul(view.view_inv, vx, vy, vz, vw, wx, wy, wz, ww);
    dx = wx - view.eye[0];
    dy = wy - view.eye[1];
    dz = wz - view.eye[2];
    const float inv = 1.0f / sqrtf(dot3(dx, dy, dz, dx, dy, dz));
    dx *= inv;
    dy *= inv;
    dz *= inv;
}

__device__ __forceinline__ uint32_t uhash(uint32_t a, uint32_t b) {
    uint32_t x = (a * 1597334673u) ^ (b * 3812015801u);
    x = x ^ (x >> 16);
    x *= 0x7feb352du;
    x = x ^ (x >> 15);
    x *= 0x846ca68bu;
    x = x ^ (x >> 16);
    return x;
}
__device__ __forceinline__ float hash_noise(uint32_t x, uint32_t y, uint32_t frame) {
    return (float)uhash(x, (y << 11) + frame) * (1.0f / 4294967296.0f);
}

// Explicit sin / cos of theta in [0, 2 pi], operation for operation what the test suite's CPU restatement evaluates:
// the binary64 algorithm the GNU C library publishes for sinf / cosf - quadrant through a scaled integer
// conversion, r = x - n * pi/2, a degree-7 odd and a degree-8 even polynomial - rounded once to binary32.  On a Linux
// host that IS the reference CPU path's sin / cos (Rust's f32::sin / cos are libm's; checked bit for bit against glibc
// for every binary32 in [0, 2 pi]).  Once per AO ray; binary64 vector arithmetic runs at full rate on this part.
__device__ __forceinline__ void sincos_det(float theta, float &s, float &c) {
    const uint32_t top = (__float_as_uint(theta) >> 20) & 0x7ffu;
    double x = (double)theta;
    int n = 0;
    if (top >= 0x3f4u) { // |theta| >= 0.75
        const double q = x * 0x1.45F306DC9C883p+23; // 2/pi * 2^24
        n = ((int)q + 0x800000) >> 24;
        x = x - (double)n * 0x1.921FB54442D18p0;
    }
    const double x2 = x * x;
    const double x3 = x * x2;
    const double s1 = 0x1.1107605230bc4p-7 + x2 * -0x1.994eb3774cf24p-13;
    const double x7 = x3 * x2;
    const double sa = x + x3 * -0x1.555545995a603p-3;
    float sp = (float)(sa + x7 * s1);
    const double x4 = x2 * x2;
    const double c2 = -0x1.6c087e89a359dp-10 + x2 * 0x1.99343027bf8c3p-16;
    const double c1 = 0x1p0 + x2 * -0x1.ffffffd0c621cp-2;
    const double x6 = x4 * x2;
    const double ca = c1 + x4 * 0x1.55553e1068f19p-5;
    float cp = (float)(ca + x6 * c2);
    if (top < 0x398u) { // |theta| < 2^-12
        sp = theta;
        cp = 1.0f;
    }
    switch (n & 3) {
    case 0: s = sp; c = cp; break;
    case 1: s = cp; c = -sp; break;
    case 2: s = -sp; c = -cp; break;
    default: s = -cp; c = sp; break;
    }
}

// An instance's world-to-object rows r0, r1, r2 ({m0 m1 m2 t} each), stated once for the two walks, the refill and the small
// kernels below.  The world ray (wo, wd) in the instance's object space: three rows on the origin, assigned to ox, oy, oz, and
// their 3x3 part on the direction, DECLARED here as dx, dy, dz - not renormalised, so t keeps its world-space meaning (the TODO
// at query_tlas.hlsl:433).  Text: as a function the two-level service walk comes out in other registers.
#define TRX_RAY_TO_OBJECT(r0, r1, r2, wox, woy, woz, wdx, wdy, wdz, ox, oy, oz, dx, dy, dz) \
    ox = ((r0.x * wox + r0.y * woy) + r0.z * woz) + r0.w;                                   \
    oy = ((r1.x * wox + r1.y * woy) + r1.z * woz) + r1.w;                                   \
    oz = ((r2.x * wox + r2.y * woy) + r2.z * woz) + r2.w;                                   \
    const float dx = (r0.x * wdx + r0.y * wdy) + r0.z * wdz;                                \
    const float dy = (r1.x * wdx + r1.y * wdy) + r1.z * wdz;                                \
    const float dz = (r2.x * wdx + r2.y * wdy) + r2.z * wdz;
// An object-space normal in world space: the transpose of the rows' 3x3 part (not normalised).
__device__ __forceinline__ float3 normal_to_world(const float4 r0, const float4 r1, const float4 r2, float nx, float ny, float nz) {
    return make_float3((r0.x * nx + r1.x * ny) + r2.x * nz, (r0.y * nx + r1.y * ny) + r2.y * nz, (r0.z * nx + r1.z * ny) + r2.z * nz);
}

// The AO ray of a primary hit (rt_gpu_software.hlsl:105-121), stated once for the refill of k_trace<kModeAo / kModeFused>
// (trace_refill.inc) and for k_ao_rays.  In: the hit triangle's normal n (world space, any length), the primary ray's unit
// direction d, the hit's t, the eye, ao_eps, the pixel and the noise seed.  Out: the origin o - the hit point pulled back by
// ao_eps - and, in d, the unit direction - cosine-weighted around n flipped toward the viewer.  n comes out normalised and
// flipped.  Text, not a function, for the reason TRX_NODE_FRAME is: as a function the refill's registers and loads come out
// in another order in every AO kernel; the arguments are evaluated where the text names them.
#define TRX_AO_RAY(nx, ny, nz, dx, dy, dz, t, eye, ao_eps, px, py, seed, ox, oy, oz)                        \
    const float ninv_ = 1.0f / sqrtf(dot3(nx, ny, nz, nx, ny, nz));                                         \
    nx *= ninv_; ny *= ninv_; nz *= ninv_;                                                                  \
    const float nd_ = (nx * -dx + ny * -dy) + nz * -dz;                                                     \
    const float sg_ = copysignf(1.0f, nd_);                                                                 \
    nx *= sg_; ny *= sg_; nz *= sg_;                                                                        \
    ox = (eye[0] + dx * t) - dx * ao_eps;                                                                   \
    oy = (eye[1] + dy * t) - dy * ao_eps;                                                                   \
    oz = (eye[2] + dz * t) - dz * ao_eps;                                                                   \
    const float u1_ = hash_noise(px, py, seed);                                                             \
    const float u2_ = hash_noise(px, py, seed + 1024u);                                                     \
    const float rr_ = sqrtf(u1_);                                                                           \
    const float theta_ = u2_ * 6.28318530717958647692f;                                                     \
    float sn_, cs_;                                                                                         \
    sincos_det(theta_, sn_, cs_);                                                                           \
    const float lx_ = rr_ * cs_, ly_ = rr_ * sn_, lz_ = sqrtf(fmaxf(0.0f, 1.0f - u1_));                     \
    const float sign_ = nz >= 0.0f ? 1.0f : -1.0f;                                                          \
    const float aa_ = -1.0f / (sign_ + nz);                                                                 \
    const float bb_ = nx * ny * aa_;                                                                        \
    const float b1x_ = 1.0f + sign_ * nx * nx * aa_, b1y_ = sign_ * bb_, b1z_ = -sign_ * nx;                \
    const float b2x_ = bb_, b2y_ = sign_ + ny * ny * aa_, b2z_ = -ny;                                       \
    dx = (b1x_ * lx_ + b2x_ * ly_) + nx * lz_;                                                              \
    dy = (b1y_ * lx_ + b2y_ * ly_) + ny * lz_;                                                              \
    dz = (b1z_ * lx_ + b2z_ * ly_) + nz * lz_;                                                              \
    const float dinv_ = 1.0f / sqrtf(dot3(dx, dy, dz, dx, dy, dz));                                         \
    dx *= dinv_; dy *= dinv_; dz *= dinv_;

__device__ __forceinline__ uint32_t read_xcc_id() {
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x;
}

// Wave64 inclusive scans on the DPP network (row shifts, then row broadcasts): VALU only, no LDS.
// Every lane of the wave must be active.
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return v;
}

// Order-preserving image of a float's bits (a < b as floats <=> image(a) < image(b) as unsigned, for non-NaN values
// with -0.0 below +0.0: callers canonicalise zeros first) and its inverse.
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ uint32_t unordered_bits(uint32_t k) {
    return k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu);
}

// Position of the (j+1)-th highest set bit of m (bits 0..23; m has more than j bits set): rank from the bottom, then
// a branch-free descent over 12 / 6 / 3 / 1 / 1 bits.
__device__ __forceinline__ uint32_t select_from_top(uint32_t m, uint32_t j) {
    uint32_t r = (uint32_t)__popc(m) - j, pos = 0u, c;
    c = (uint32_t)__popc(m & 0xfffu);
    if (r > c) { r -= c; pos = 12u; }
    c = (uint32_t)__popc((m >> pos) & 0x3fu);
    if (r > c) { r -= c; pos += 6u; }
    c = (uint32_t)__popc((m >> pos) & 0x7u);
    if (r > c) { r -= c; pos += 3u; }
    c = (m >> pos) & 1u;
    if (r > c) { r -= c; pos += 1u; }
    c = (m >> pos) & 1u;
    if (r > c) pos += 1u;
    return pos;
}

__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// x / d for a launch-uniform d whose m = floor(2^32 / d) comes with the launch parameters (m = 2^32 - 1 for d <= 1): the
// estimate mulhi(x, m) is x / d or one less for every 32-bit x, one correction step makes it exact.  (A division left to
// the compiler computes the same kind of reciprocal on the vector unit and keeps it in a vector register across the
// whole walk - four of them in the refill of kernels that sit at the register budget.)
__device__ __forceinline__ uint32_t div_uniform(uint32_t x, uint32_t d, uint32_t m) {
    const uint32_t q = __umulhi(x, m);
    return x - q * d >= d ? q + 1u : q;
}

// The kernel arguments, through a pointer whose origin the compiler cannot see (k_trace's refill): loads through it
// are scalar loads from the kernel-argument segment that stay where they are written.
__device__ __forceinline__ const TraceParams *refill_params() {
    int zero;
    asm volatile("s_mov_b32 %0, 0" : "=s"(zero));
    zero = __builtin_amdgcn_readfirstlane(zero); // (tells the compiler what the constraint cannot: wave-uniform)
    return (const TraceParams *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + zero);
}

// The LDS part of the per-lane stacks is addressed through an explicit LDS (address space 3) pointer.  A pop reads either
// LDS or, past kLdsStack entries, HBM: as two loads through generic pointers of the same shape the optimizer merges them
// into ONE load of a selected address - a flat load on the walk's hot path, which also waits for every node record
// requested ahead (vmcnt).  Round 4 shipped that for a while: AO passes +8-10 %, profiles/r04_flat_stack_pop.log.
// tests/test_kernel_resources.py holds the line (no flat_load_dwordx2 in any trace kernel).
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
__device__ __forceinline__ uint2 lds_ld(const lds_u32x2 *p) {
    const u32x2 v = *p;
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void lds_st(lds_u32x2 *p, uint2 e) { *p = u32x2{e.x, e.y}; }

// Appends the parked {tile, list} entries to the next frame's tile lists.  A wave files all its tiles of a class under one
// shard, so its entries fall into a few groups (one per class it met); the first lane of a group claims the group's
// slots with ONE returning atomic, the groups' atomics go out together, and every lane stores its tile at its rank
// within the group.  (One atomic per ENTRY - round 1 and 2 - was 32 400 a frame on 128 counters, most of them as the
// waves leave; in a natural-order frame neighbouring tiles share a class and a few counters took them all: 0.08 ms of a
// bistro-class first frame, 0.11 ms of a kitchen-class one, profiles/r03_filing_cost.log.)
__device__ __forceinline__ void flush_pending(const TraceParams &P, uint32_t *wr_set, const uint2 *lds_pend, uint32_t n, uint32_t lane) {
    __builtin_amdgcn_wave_barrier();
    uint2 e = make_uint2(0u, 0xffffffffu);
    // (the address is formed HERE: left alone the compiler forms it at kernel start and carries - or spills - it to the epilogue)
    asm volatile("" : "+v"(lane));
    if (lane < n) e = lds_pend[lane];
    const bool valid = e.y < 16u * kLptShards; // (a list index can only be out of range if LDS was corrupted: never turn that into a stray global atomic)
    // the lanes that share this lane's list: one ballot per class (the shard is the wave's, so the class names the list)
    unsigned long long mine = 0ull;
    const uint32_t cls = valid ? e.y / kLptShards : 0xffffffffu;
#pragma nounroll
    for (uint32_t c = 0; c < 16u; c++) { // (a loop, not sixteen copies: this runs once or twice per wave and must not cost the walk a register)
        const unsigned long long m = __ballot(cls == c);
        if (cls == c) mine = m;
    }
    const uint32_t leader = (uint32_t)__ffsll((long long)mine) - 1u; // (mine != 0 for a valid lane: it contains the lane itself)
    const uint32_t rank = (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
    uint32_t base = 0u;
    if (valid && lane == leader) base = atomicAdd(&wr_set[e.y], (uint32_t)__popcll(mine));
    base = (uint32_t)__shfl((int)base, (int)(valid ? leader : lane));
    if (valid) {
        const uint32_t pos = base + rank;
        if (pos < P.lpt_cap) wr_set[16u * kLptShards + (size_t)e.y * P.lpt_cap + pos] = e.x;
    }
    __builtin_amdgcn_wave_barrier();
}

// The same without the grouping, one atomic per entry: for the flush in the middle of a frame (a wave that has parked
// kLptPend tiles - 4K frames), where the walk's registers are live and the grouped version would cost it a spill.
__device__ __forceinline__ void flush_pending_plain(const TraceParams &P, uint32_t *wr_set, const uint2 *lds_pend, uint32_t n, uint32_t lane) {
    __builtin_amdgcn_wave_barrier();
    if (lane < n) {
        const uint2 e = lds_pend[lane];
        if (e.y < 16u * kLptShards) {
            const uint32_t pos = atomicAdd(&wr_set[e.y], 1u);
            if (pos < P.lpt_cap) wr_set[16u * kLptShards + (size_t)e.y * P.lpt_cap + pos] = e.x;
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// 16-byte and 8-byte accesses that go all the way to memory (`sc0 sc1`: system scope): the ray service's porter reads request
// granules out of pinned host memory and writes answers there while the host looks on (trace_service.inc)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 sys_load128(const void *p) {
    u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// PIPE (BLAS-only walks): the fetch of a ray's NEXT node is issued right after the node test that names it, before
// the triangle phase of the node just tested, so the two memory round trips of a step overlap (the next node does
// not depend on the triangles' results, only its test does: it reads the shrunken t).  A ray then occupies its lane
// for one trip more (its last trip has triangle work only), which is why coherent, issue-bound frames do not want it.
template <bool TLAS>
using KernelParams = std::conditional_t<TLAS, TraceParamsTlas, TraceParams>; // (kernels.h, TraceParamsTlas)

template <int MODE, bool TLAS, int NODE, bool PIPE, bool COUNT>
__global__ void __launch_bounds__(kMaxBlock, TRX_MIN_WAVES) k_trace(const KernelParams<TLAS> P) {
    // (P is the kernel's ONLY parameter: refill_params() reads it back from offset 0 of the kernel-argument segment)
    static_assert(!(PIPE && TLAS), "the pipelined walk is BLAS-only");
    // triangles of a lane requested together in a per-lane triangle round (the two-level walk has fewer registers to spare)
    constexpr int kBatch = TLAS ? kTriBatchTlas : (PIPE ? kTriBatchPipe : kTriBatch);
#include "trace_state.inc"
#include "trace_queues.inc"
#include "trace_stack.inc"
#include "trace_thin.inc"
    if constexpr (MODE == kModeService) {
#include "trace_service.inc"
    } else {
    for (;;) {
        TRX_STAMP(k_pop);
#include "trace_refill.inc"
        TRX_STAMP(k_refill);
        if (__ballot(has_ray) == 0ull) {
            if (exhausted) {
                if (kMerge && merge_open && wave_in_block == 0u) {
                    // leaving: close the door, or find that the second wave has just offered its rays
                    uint32_t old = 0u;
                    if (lane == 0u) old = atomicCAS(&merge_ctl[0], 0u, kMergeClosed);
                    old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
                    merge_open = false;
                    if (old != 0u) {
                        merge_open = true;
                        need_take = old;
                    }
                }
                if (!(kMerge && need_take != 0u)) break;
            } else {
                continue;
            }
        }

#include "trace_triangles.inc"
#include "trace_drain.inc"
        if (kMerge && need_take != 0u) {
            merge_take(need_take);
            need_take = 0u;
        }
        if constexpr (!PIPE) {
#include "trace_walk_plain.inc"
        } else {
#include "trace_walk_pipe.inc"
        }
        if (kThin && go_thin) {
            // (nothing comes back from the thin walk of a dry wave - except a fused frame's lane that waits to become an AO
            // ray - so it runs AFTER the loop, where the registers the loop carries are dead)
            if (!kFused) break;
            go_thin = false;
            thin_all(); // returns with no ray left, or with a lane waiting to become an AO ray
        }
    }
    if (kThin && !kFused && go_thin) thin_all(); // returns with no ray left

    }

#include "trace_epilogue.inc"
}


#undef wave_global
#undef wray

template <int MODE, bool TLAS, int NODE, bool PIPE, bool COUNT>
hipError_t launch_one(const TraceParamsTlas &p, int grid, hipStream_t stream) {
    // grid = total waves; p.waves_per_block waves share a workgroup (and nothing else)
    const int wpb = (int)p.waves_per_block;
    const size_t lds = (size_t)wpb * kLdsBytesPerWave;
    const KernelParams<TLAS> &kp = p; // (single-level kernels: the TraceParams part)
    hipLaunchKernelGGL((k_trace<MODE, TLAS, NODE, PIPE, COUNT>), dim3(grid / wpb), dim3(kWave * wpb), lds, stream, kp);
    return hipGetLastError();
}

template <int MODE, bool TLAS, bool PIPE, bool COUNT>
hipError_t launch_node(const TraceParamsTlas &p, int node, int grid, hipStream_t stream) {
    switch (node) {
    case 0: return launch_one<MODE, TLAS, 0, PIPE, COUNT>(p, grid, stream);
    case 1: return launch_one<MODE, TLAS, 1, PIPE, COUNT>(p, grid, stream);
    case 2: return launch_one<MODE, TLAS, 2, PIPE, COUNT>(p, grid, stream);
    default: return launch_one<MODE, TLAS, 3, PIPE, COUNT>(p, grid, stream);
    }
}

template <int MODE>
hipError_t launch_mode(const TraceParamsTlas &p, bool tlas, int node, bool count, bool pipe, int grid, hipStream_t stream) {
    if constexpr (MODE == kModeService) {
        // (the resident kernel is the plain thin walk, single- or two-level: no pipelining, no counting)
        if (count) return hipErrorInvalidValue;
        return tlas ? launch_node<MODE, true, false, false>(p, node, grid, stream) : launch_node<MODE, false, false, false>(p, node, grid, stream);
    } else {
        // (the one-launch frame exists for single-level scenes: the two-level walk has no registers to spare for the in-place
        // hand-over - it spills - so trx_trace_frame_dev runs a two-level frame as two launches, api_trace.cpp)
        if constexpr (MODE == kModeFused) {
            if (tlas) return hipErrorInvalidValue;
        } else
        if (tlas) { // the two-level walk is not pipelined
            if (count) return launch_node<MODE, true, false, true>(p, node, grid, stream);
            return launch_node<MODE, true, false, false>(p, node, grid, stream);
        }
        // (coherent primary rays do not gain from the pipelined walk)
        if constexpr (MODE != kModePrimary) {
            if (pipe) {
                if (count) return launch_node<MODE, false, true, true>(p, node, grid, stream);
                return launch_node<MODE, false, true, false>(p, node, grid, stream);
            }
        }
        if (count) return launch_node<MODE, false, false, true>(p, node, grid, stream);
        return launch_node<MODE, false, false, false>(p, node, grid, stream);
    }
}

template <int MODE, bool TLAS, int NODE, bool PIPE, bool COUNT>
int occupancy_one() {
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_trace<MODE, TLAS, NODE, PIPE, COUNT>, kWave,
                                                     kLdsBytesPerWave) != hipSuccess)
        return 0;
    return blocks;
}

int node_variant(uint32_t sem) {
    return ((sem & TRX_SEM_NODE_RCP) ? 1 : 0) | ((sem & TRX_SEM_NODE_FMA) ? 2 : 0);
}

// The pixel of lane k of a shard's local tile, for the small kernels below (the refill of k_trace states it with div_uniform,
// trace_refill.inc): false where the tile's 8x8 block leaves the image.  rec = the pixel's record, laid out by the shard like
// the hit buffers.
__device__ __forceinline__ bool tile_pixel(const TileGeom &G, uint32_t local_tile, uint32_t k, uint32_t &px, uint32_t &py, uint32_t &rec) {
    const uint32_t tile = local_tile * G.shard_count + G.shard_index;
    const uint32_t ty = tile / G.tiles_x;
    px = (tile - ty * G.tiles_x) * 8u + (k & 7u);
    py = ty * 8u + (k >> 3);
    rec = G.compact ? local_tile * 64u + k : py * G.width + px;
    return px < G.width && py < G.height;
}

// Hit attributes (include/trx.h, trx_hit_attr): one lane per hit record.  The ray the committing triangle test saw is
// rebuilt - the explicit ray, or the primary ray of the record's pixel; with instance transforms the world ray as given
// through the instance's world-to-object rows (TRX_RAY_TO_OBJECT, as the walks do) - and the test's u, v are recomputed with
// intersect_tri's operations, restated here; the normal is the AO pass's before its flip (normal_to_world, as the refill does).  A gather: 8 B of hit,
// 4 B of instance id, 48 B of triangle (and 48 B of rows) per record, 24 B written.  Primary frames are walked in the
// tile order of the trace (64 lanes = one 8x8 tile), so a wave's hits are the same tile's.
template <int MODE>
__global__ void __launch_bounds__(256) k_hit_attr(const HitAttrParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_items) return;
    uint32_t rec = item;
    float ox, oy, oz, dx, dy, dz;
    if constexpr (MODE == kAttrPrimary) {
        uint32_t px, py;
        if (!tile_pixel(P.geom, item >> 6, item & 63u, px, py, rec)) return; // (the trace writes no record for it either)
        primary_dir(P.view, P.geom.width, P.geom.height, px, py, dx, dy, dz);
        ox = P.view.eye[0]; oy = P.view.eye[1]; oz = P.view.eye[2];
    } else {
        const float4 *rp = reinterpret_cast<const float4 *>(P.rays + item);
        const float4 a = rp[0], b = rp[1];
        ox = a.x; oy = a.y; oz = a.z;
        dx = b.x; dy = b.y; dz = b.z;
    }
    const uint32_t prim = P.hits[rec].prim;
    float4 r0 = make_float4(1.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
    bool ok = prim < P.n_tris;
    if (P.inst_xform) {
        const uint32_t inst = P.inst[rec];
        ok = ok && inst < P.n_inst;
        if (ok) {
            const float4 *m = P.inst_xform + (size_t)inst * 3;
            r0 = m[0]; r1 = m[1]; r2 = m[2];
        }
    }
    float u = 0.0f, v = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (ok) {
        const float4 *tp = P.tris + (size_t)prim * 3;
        const float4 a = tp[0], b = tp[1], c4 = tp[2];
        const float e1x = b.x, e1y = b.y, e1z = b.z;
        const float e2x = c4.x, e2y = c4.y, e2z = c4.z;
        nx = a.w; ny = b.w; nz = c4.w;
        if (P.inst_xform) {
            // the object-space ray the BLAS walk tested with
            float tox, toy, toz;
            TRX_RAY_TO_OBJECT(r0, r1, r2, ox, oy, oz, dx, dy, dz, tox, toy, toz, tdx, tdy, tdz)
            ox = tox; oy = toy; oz = toz;
            dx = tdx; dy = tdy; dz = tdz;
        }
        // finish_ray_dir's zero-direction fix (query.hlsl:334)
        dx = dx == 0.0f ? TRX_F32_EPSILON : dx;
        dy = dy == 0.0f ? TRX_F32_EPSILON : dy;
        dz = dz == 0.0f ? TRX_F32_EPSILON : dz;
        // intersect_tri's u, v
        const float cx = a.x - ox, cy = a.y - oy, cz = a.z - oz;
        const float rx = dy * cz - dz * cy;
        const float ry = dz * cx - dx * cz;
        const float rz = dx * cy - dy * cx;
        const float det = dot3(nx, ny, nz, dx, dy, dz);
        const float un = dot3(rx, ry, rz, e2x, e2y, e2z), vn = dot3(rx, ry, rz, e1x, e1y, e1z);
        const float inv_det = 1.0f / det;
        u = un * inv_det;
        v = vn * inv_det;
        if (P.inst_xform) {
            const float3 w = normal_to_world(r0, r1, r2, nx, ny, nz);
            nx = w.x; ny = w.y; nz = w.z;
        }
        const float ninv = 1.0f / sqrtf(dot3(nx, ny, nz, nx, ny, nz));
        nx *= ninv; ny *= ninv; nz *= ninv;
    }
    trx_hit_attr out;
    out.u = u;
    out.v = v;
    out.normal[0] = nx;
    out.normal[1] = ny;
    out.normal[2] = nz;
    out._pad = 0u;
    P.out[rec] = out;
}

// The shading normal (include/trx.h, "THE SHADING NORMAL"; kernels.h, ShadingNormalParams): one lane per record, no
// traversal.  The record's attribute record comes back with its geometric normal replaced by the interpolated vertex normal
// where the header's rule adopts it, and bit for bit as it was everywhere else - an out-of-range prim or instance id
// included, which reads no table (CALLER RECORDS; t is not looked at, as in k_hit_attr).  The ray direction is the light
// term's: primary_dir of the pixel, or the ray's direction words, no zero-direction fix.  A gather: 8 B of hit, 4 B of
// instance id, 24 B of attributes, 48 B of normals (and 48 B of rows) per record, 24 B written; primary frames in the tile
// order of the trace, like k_hit_attr.  Each lane reads its record before it writes it: out may be attr.
template <int MODE>
__global__ void __launch_bounds__(256) k_shading_normal(const ShadingNormalParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_items) return;
    uint32_t rec = item;
    float dx, dy, dz;
    if constexpr (MODE == kAttrPrimary) {
        uint32_t px, py;
        if (!tile_pixel(P.geom, item >> 6, item & 63u, px, py, rec)) return;
        primary_dir(P.view, P.geom.width, P.geom.height, px, py, dx, dy, dz);
    } else {
        const float4 b = reinterpret_cast<const float4 *>(P.rays + item)[1];
        dx = b.x; dy = b.y; dz = b.z;
    }
    const uint32_t prim = P.hits[rec].prim;
    trx_hit_attr A = P.attr[rec];
    float4 r0 = make_float4(1.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
    bool ok = prim < P.n_tris;
    if (P.inst_xform) {
        const uint32_t inst = P.inst[rec];
        ok = ok && inst < P.n_inst;
        if (ok) {
            const float4 *m = P.inst_xform + (size_t)inst * 3;
            r0 = m[0]; r1 = m[1]; r2 = m[2];
        }
    }
    if (ok) {
        const float4 *np = P.normals + (size_t)prim * 3;
        const float4 n0 = np[0], n1 = np[1], n2 = np[2];
        const float u = A.u, v = A.v;
        const float gx = A.normal[0], gy = A.normal[1], gz = A.normal[2];
        const float w = (1.0f - u) - v;
        float mx = (w * n0.x + u * n1.x) + v * n2.x;
        float my = (w * n0.y + u * n1.y) + v * n2.y;
        float mz = (w * n0.z + u * n1.z) + v * n2.z;
        if (P.inst_xform) {
            const float3 t = normal_to_world(r0, r1, r2, mx, my, mz);
            mx = t.x; my = t.y; mz = t.z;
        }
        const float q = dot3(mx, my, mz, mx, my, mz);
        const float inv = 1.0f / sqrtf(q);
        float sx = mx * inv, sy = my * inv, sz = mz * inv;
        const float c = dot3(sx, sy, sz, gx, gy, gz);
        const float sg = copysignf(1.0f, c);
        sx *= sg; sy *= sg; sz *= sg;
        const float a = (gx * -dx + gy * -dy) + gz * -dz;
        const float b = (sx * -dx + sy * -dy) + sz * -dz;
        // adopted only where the light term's flip is the same for s as for g (false for a NaN on either side)
        if (q > 0.0f && q < __builtin_inff() && c == c && ((a > 0.0f && b > 0.0f) || (a < 0.0f && b < 0.0f))) {
            A.normal[0] = sx;
            A.normal[1] = sy;
            A.normal[2] = sz;
            A._pad = 0u;
        }
    }
    P.out[rec] = A;
}

// AO visibility (include/trx.h, trx_ao_rays_dev / trx_trace_ao_visibility_dev; kernels.h, AoRaysParams).
// The AO ray of every (tile, sample, pixel) as an explicit ray: what the refill of k_trace<kModeAo> builds for that pixel
// and seed (trace_refill.inc) through the same statements - primary_dir, normal_to_world, TRX_AO_RAY - with tmin = 0 and
// tmax = the AO radius.  Its own: the addressing and the inert ray - a pixel whose primary record is a miss gets it (all
// words 0 but tmax = -1: no walk commits a hit on it, every walk starts from min(tmax, FLT_MAX)).  A streaming kernel: 8 B of
// primary record, 48 B of triangle (and 48 B of rows) read per ray, 32 B written.
//   SPARSE (trx_trace_ao_visibility_sparse_dev): the addressing alone differs - the tile is one of the low grid, its cell
// names the pixel of the full image whose ray this is; everything from the primary record on is the dense pass's statement.
template <bool SPARSE>
__global__ void __launch_bounds__(256) k_ao_rays(const AoRaysParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * P.n_samples * 64u) return;
    const uint32_t unit = item >> 6, k = item & 63u;
    const uint32_t lt = unit / P.n_samples, sample = unit - lt * P.n_samples;
    uint32_t px, py, rec;
    bool inside;
    if constexpr (SPARSE) {
        uint32_t cx, cy, cell;
        inside = tile_pixel(P.lo, P.tile0 + lt, k, cx, cy, cell);
        px = cx * P.stride + P.px0;
        py = cy * P.stride + P.py0;
        inside = inside && px < P.geom.width && py < P.geom.height;
        rec = py * P.geom.width + px;
    } else {
        inside = tile_pixel(P.geom, P.tile0 + lt, k, px, py, rec);
    }
    if (!inside && !P.scratch) return; // (the trace writes no record for it either)
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    trx_hit ph;
    ph.t = __builtin_inff();
    ph.prim = TRX_INVALID;
    if (inside) ph = P.primary[rec];
    if (surface_record(ph, P.n_tris)) { // (kernels.h: a caller's record that fails it is a miss - the inert ray)
        float dx, dy, dz;
        primary_dir(P.view, P.geom.width, P.geom.height, px, py, dx, dy, dz);
        const float4 *tp = P.tris + (size_t)ph.prim * 3;
        float nx = tp[0].w, ny = tp[1].w, nz = tp[2].w; // cross(e1, e2)
        if (P.inst_xform) {
            const uint32_t pi = P.primary_inst[rec];
            if (instance_row(pi, P.n_inst)) {
                const float4 *m = P.inst_xform + (size_t)pi * 3;
                const float3 w = normal_to_world(m[0], m[1], m[2], nx, ny, nz);
                nx = w.x; ny = w.y; nz = w.z;
            }
        }
        const uint32_t seed = P.frame + sample;
        TRX_AO_RAY(nx, ny, nz, dx, dy, dz, ph.t, P.view.eye, P.ao_eps, px, py, seed, a.x, a.y, a.z)
        b.x = dx; b.y = dy; b.z = dz;
        b.w = P.tmax;
    }
    float4 *out = reinterpret_cast<float4 *>(P.rays + (P.scratch ? item : rec));
    out[0] = a;
    out[1] = b;
}

// One lane per pixel of the chunk's tiles: the samples of the chunk whose ray was NOT occluded, set (first samples of the
// tile: TRX_AO_NO_SURFACE where the primary record is a miss - the inert ray names it) or added to the pixel's count.
//   SPARSE: one lane per cell of the low grid's tiles, the count at the cell's place in the low grid; a cell whose pixel
// leaves the image carries the inert ray too, so it gets TRX_AO_NO_SURFACE.
template <bool SPARSE>
__global__ void __launch_bounds__(256) k_ao_reduce(const AoRaysParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * 64u) return;
    const uint32_t lt = item >> 6, k = item & 63u;
    uint32_t px, py, rec;
    if (!tile_pixel(SPARSE ? P.lo : P.geom, P.tile0 + lt, k, px, py, rec)) return;
    const uint32_t base = lt * P.n_samples * 64u + k;
    const bool surface = !(P.rays[base].tmax < 0.0f);
    uint32_t n = 0u;
    for (uint32_t s = 0; s < P.n_samples; s++) n += P.flags[base + s * 64u] == 0u ? 1u : 0u;
    if (P.first) P.counts[rec] = (uint8_t)(surface ? n : kAoNoSurface);
    else if (surface) P.counts[rec] = (uint8_t)(P.counts[rec] + n);
}

// Direct light (include/trx.h, "THE SHADOW RAY"; kernels.h, LightRaysParams).  The unit direction toward a directional light.
__device__ __forceinline__ void light_toward(const trx_light &L, float &lx, float &ly, float &lz) {
    const float inv = 1.0f / sqrtf(dot3(L.position[0], L.position[1], L.position[2], L.position[0], L.position[1], L.position[2]));
    lx = L.position[0] * inv;
    ly = L.position[1] * inv;
    lz = L.position[2] * inv;
}

// The shadow ray of every (tile, sample, pixel) toward ONE light as an explicit ray: k_ao_rays' addressing, primary
// direction, normal (the first five statements of TRX_AO_RAY, restated: the rest of that text is the AO direction) and
// origin with shadow_eps for ao_eps; then the header's light point, direction, reach and facing test.  The inert ray goes to
// pixels without a surface and to samples that do not face the light.  A streaming kernel like k_ao_rays: 8 B of primary
// record, 48 B of triangle (and 48 B of rows) read per ray, 32 B written; the light is launch-uniform (scalar loads).
__global__ void __launch_bounds__(256) k_light_rays(const LightRaysParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * P.n_samples * 64u) return;
    const uint32_t unit = item >> 6, k = item & 63u;
    const uint32_t lt = unit / P.n_samples, sample = unit - lt * P.n_samples;
    uint32_t px, py, rec;
    const bool inside = tile_pixel(P.geom, P.tile0 + lt, k, px, py, rec);
    if (!inside && !P.scratch) return; // (the trace writes no record for it either)
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    trx_hit ph;
    ph.t = __builtin_inff();
    ph.prim = TRX_INVALID;
    if (inside) ph = P.primary[rec];
    if (surface_record(ph, P.n_tris)) { // (kernels.h: a caller's record that fails it is a miss - the inert ray)
        float dx, dy, dz;
        primary_dir(P.view, P.geom.width, P.geom.height, px, py, dx, dy, dz);
        const float4 *tp = P.tris + (size_t)ph.prim * 3;
        float nx = tp[0].w, ny = tp[1].w, nz = tp[2].w; // cross(e1, e2)
        if (P.inst_xform) {
            const uint32_t pi = P.primary_inst[rec];
            if (instance_row(pi, P.n_inst)) {
                const float4 *m = P.inst_xform + (size_t)pi * 3;
                const float3 w = normal_to_world(m[0], m[1], m[2], nx, ny, nz);
                nx = w.x; ny = w.y; nz = w.z;
            }
        }
        const float ninv = 1.0f / sqrtf(dot3(nx, ny, nz, nx, ny, nz));
        nx *= ninv; ny *= ninv; nz *= ninv;
        const float nd = (nx * -dx + ny * -dy) + nz * -dz;
        const float sg = copysignf(1.0f, nd);
        nx *= sg; ny *= sg; nz *= sg;
        const float ox = (P.view.eye[0] + dx * ph.t) - dx * P.shadow_eps;
        const float oy = (P.view.eye[1] + dy * ph.t) - dy * P.shadow_eps;
        const float oz = (P.view.eye[2] + dz * ph.t) - dz * P.shadow_eps;
        float lx, ly, lz, tmax;
        if (P.light.kind == TRX_LIGHT_DIRECTIONAL) {
            light_toward(P.light, lx, ly, lz);
            tmax = TRX_F32_MAX;
        } else {
            float Lx = P.light.position[0], Ly = P.light.position[1], Lz = P.light.position[2];
            if (P.light.kind == TRX_LIGHT_RECT) {
                const uint32_t seed = P.seed0 + sample;
                const float u1 = hash_noise(px, py, seed);
                const float u2 = hash_noise(px, py, seed + 1024u);
                Lx = (Lx + u1 * P.light.edge1[0]) + u2 * P.light.edge2[0];
                Ly = (Ly + u1 * P.light.edge1[1]) + u2 * P.light.edge2[1];
                Lz = (Lz + u1 * P.light.edge1[2]) + u2 * P.light.edge2[2];
            }
            const float vx = Lx - ox, vy = Ly - oy, vz = Lz - oz;
            const float dist = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
            const float inv = 1.0f / dist;
            lx = vx * inv; ly = vy * inv; lz = vz * inv;
            tmax = fminf(dist, TRX_F32_MAX);
        }
        if (dot3(nx, ny, nz, lx, ly, lz) > 0.0f) { // (false for NaN: a light at the hit point)
            a.x = ox; a.y = oy; a.z = oz;
            b = make_float4(lx, ly, lz, tmax);
        }
    }
    float4 *out = reinterpret_cast<float4 *>(P.rays + (P.scratch ? item : rec));
    out[0] = a;
    out[1] = b;
}

// One lane per pixel of the chunk's tiles: the samples of the chunk whose shadow ray was cast (not inert) and NOT occluded,
// set (first samples of the tile: TRX_AO_NO_SURFACE where the primary record is a miss) or added to the pixel's count in the
// light's plane.  The surface comes from the primary record: an inert ray here may be a sample facing away.
__global__ void __launch_bounds__(256) k_light_reduce(const LightRaysParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * 64u) return;
    const uint32_t lt = item >> 6, k = item & 63u;
    uint32_t px, py, rec;
    if (!tile_pixel(P.geom, P.tile0 + lt, k, px, py, rec)) return;
    const trx_hit ph = P.primary[rec];
    const bool surface = surface_record(ph, P.n_tris); // (as k_light_rays decided it)
    const uint32_t base = lt * P.n_samples * 64u + k;
    uint32_t n = 0u;
    for (uint32_t s = 0; s < P.n_samples; s++)
        n += P.flags[base + s * 64u] == 0u && !(P.rays[base + s * 64u].tmax < 0.0f) ? 1u : 0u;
    if (P.first) P.counts[rec] = (uint8_t)(surface ? n : kAoNoSurface);
    else if (surface) P.counts[rec] = (uint8_t)(P.counts[rec] + n);
}

// The light term (include/trx.h, trx_light_term_dev): one lane per pixel of the shard's tiles.  The ambient times the
// filtered AO term, then light after light the unshadowed analytic term times the traced visibility, in the header's order
// of operations.  Streaming: 8 B of primary record, 24 B of attributes, one byte per light (and 4 B of AO term) read, 4 B
// written; the lights are launch-uniform.
__global__ void __launch_bounds__(256) k_light_term(const LightTermParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * 64u) return;
    uint32_t px, py, rec;
    if (!tile_pixel(P.geom, item >> 6, item & 63u, px, py, rec)) return;
    const trx_hit ph = P.primary[rec];
    float E = 0.0f;
    if (ph.t < TRX_F32_MAX && ph.prim != TRX_INVALID) {
        float dx, dy, dz;
        primary_dir(P.view, P.geom.width, P.geom.height, px, py, dx, dy, dz);
        const trx_hit_attr at = P.attr[rec];
        float nx = at.normal[0], ny = at.normal[1], nz = at.normal[2];
        const float nd = (nx * -dx + ny * -dy) + nz * -dz;
        const float sg = copysignf(1.0f, nd);
        nx *= sg; ny *= sg; nz *= sg;
        const float Px = P.view.eye[0] + dx * ph.t, Py = P.view.eye[1] + dy * ph.t, Pz = P.view.eye[2] + dz * ph.t;
        float amb = 1.0f;
        if (P.term) {
            const trx_ao_term tm = P.term[rec];
            amb = tm.samples == 0 ? 0.0f : (float)tm.unoccluded / (float)tm.samples;
        }
        E = P.ambient * amb;
        for (uint32_t li = 0; li < P.n_lights; li++) {
            const trx_light &L = P.lights[li];
            float g;
            if (L.kind == TRX_LIGHT_DIRECTIONAL) {
                float lx, ly, lz;
                light_toward(L, lx, ly, lz);
                g = dot3(nx, ny, nz, lx, ly, lz);
            } else {
                float Cx = L.position[0], Cy = L.position[1], Cz = L.position[2];
                if (L.kind == TRX_LIGHT_RECT) {
                    Cx = (Cx + 0.5f * L.edge1[0]) + 0.5f * L.edge2[0];
                    Cy = (Cy + 0.5f * L.edge1[1]) + 0.5f * L.edge2[1];
                    Cz = (Cz + 0.5f * L.edge1[2]) + 0.5f * L.edge2[2];
                }
                const float vx = Cx - Px, vy = Cy - Py, vz = Cz - Pz;
                const float q = dot3(vx, vy, vz, vx, vy, vz);
                const float inv = 1.0f / sqrtf(q);
                g = dot3(nx, ny, nz, vx * inv, vy * inv, vz * inv) / q;
            }
            uint32_t cnt = P.lit[(size_t)li * P.plane_stride + rec];
            cnt = cnt == kAoNoSurface ? 0u : cnt;
            const float nk = (float)(L.kind == TRX_LIGHT_RECT ? P.n_samples : 1u);
            if (g > 0.0f) E = E + (L.intensity * g) * ((float)cnt / nk);
        }
    }
    P.value[rec] = E;
}

// One-bounce indirect light (include/trx.h, "indirect light"; kernels.h, BounceParams).  What the shadow-ray kernel and the
// weight kernel share of a bounce: the ray, its hit and its attribute record at `index`; false where the bounce found no
// surface (an inert bounce ray, a miss).  d = the bounce direction, n = the attribute normal flipped against d, Q = the hit
// point - the header's statements, one binary32 operation each.
struct BounceHit {
    float dx, dy, dz, nx, ny, nz, qx, qy, qz;
};
__device__ __forceinline__ bool bounce_hit(const BounceParams &P, uint32_t index, BounceHit &B) {
    const float4 *rp = reinterpret_cast<const float4 *>(P.bounce_rays + index);
    const float4 a = rp[0], b = rp[1];
    const trx_hit bh = P.bounce_hits[index];
    if (b.w < 0.0f || !(bh.t < TRX_F32_MAX) || bh.prim == TRX_INVALID) return false;
    const trx_hit_attr at = P.bounce_attr[index];
    B.dx = b.x; B.dy = b.y; B.dz = b.z;
    const float nd = (at.normal[0] * -B.dx + at.normal[1] * -B.dy) + at.normal[2] * -B.dz;
    const float sg = copysignf(1.0f, nd);
    B.nx = at.normal[0] * sg; B.ny = at.normal[1] * sg; B.nz = at.normal[2] * sg;
    B.qx = a.x + B.dx * bh.t;
    B.qy = a.y + B.dy * bh.t;
    B.qz = a.z + B.dz * bh.t;
    return true;
}

// The shadow ray of every (tile, sample, pixel) from its bounce hit toward ONE light: k_light_rays with the primary hit
// replaced by the bounce hit - the normal comes from the attribute record, so no triangle and no instance row is read.  A
// streaming kernel: 32 B of bounce ray, 8 B of hit, 24 B of attributes read per ray, 32 B written; the light is launch-uniform.
//   SPARSE (trx_trace_indirect_sparse_dev; scratch layout): the tile is one of the low grid, and the rect light's noise is
// taken at the cell's pixel of the full image - k_ao_rays' mapping; everything else is the dense statement.  A cell whose
// pixel leaves the image carries the inert bounce ray, so its coordinates are never looked at.
template <bool SPARSE>
__global__ void __launch_bounds__(256) k_bounce_light_rays(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * P.n_samples * 64u) return;
    const uint32_t unit = item >> 6, k = item & 63u;
    const uint32_t lt = unit / P.n_samples, sample = unit - lt * P.n_samples;
    uint32_t px, py, rec;
    uint32_t index;
    if constexpr (SPARSE) {
        uint32_t cx, cy;
        tile_pixel(P.lo, P.tile0 + lt, k, cx, cy, rec);
        px = cx * P.stride + P.px0;
        py = cy * P.stride + P.py0;
        index = item;
    } else {
        const bool inside = tile_pixel(P.geom, P.tile0 + lt, k, px, py, rec);
        if (!inside && !P.scratch) return; // (no record is there)
        index = P.scratch ? item : rec;
    }
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    BounceHit B;
    if (bounce_hit(P, index, B)) { // (scratch layout: a lane outside the image reads the inert bounce ray k_ao_rays wrote there)
        const float ox = B.qx - B.dx * P.shadow_eps;
        const float oy = B.qy - B.dy * P.shadow_eps;
        const float oz = B.qz - B.dz * P.shadow_eps;
        float lx, ly, lz, tmax;
        if (P.light.kind == TRX_LIGHT_DIRECTIONAL) {
            light_toward(P.light, lx, ly, lz);
            tmax = TRX_F32_MAX;
        } else {
            float Lx = P.light.position[0], Ly = P.light.position[1], Lz = P.light.position[2];
            if (P.light.kind == TRX_LIGHT_RECT) {
                const uint32_t seed = P.seed0 + sample;
                const float u1 = hash_noise(px, py, seed);
                const float u2 = hash_noise(px, py, seed + 1024u);
                Lx = (Lx + u1 * P.light.edge1[0]) + u2 * P.light.edge2[0];
                Ly = (Ly + u1 * P.light.edge1[1]) + u2 * P.light.edge2[1];
                Lz = (Lz + u1 * P.light.edge1[2]) + u2 * P.light.edge2[2];
            }
            const float vx = Lx - ox, vy = Ly - oy, vz = Lz - oz;
            const float dist = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
            const float inv = 1.0f / dist;
            lx = vx * inv; ly = vy * inv; lz = vz * inv;
            tmax = fminf(dist, TRX_F32_MAX);
        }
        if (dot3(B.nx, B.ny, B.nz, lx, ly, lz) > 0.0f) { // (false for NaN: a light at the bounce hit)
            a.x = ox; a.y = oy; a.z = oz;
            b = make_float4(lx, ly, lz, tmax);
        }
    }
    float4 *out = reinterpret_cast<float4 *>(P.rays + index);
    out[0] = a;
    out[1] = b;
}

// One lane per (tile, sample, pixel) of the scratch: s (0 before the first light) + intensity * g where the shadow ray toward
// this light was cast and is not occluded and g > 0; g is the light term's, at the bounce hit, toward the light's centre.
__global__ void __launch_bounds__(256) k_bounce_weight(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * P.n_samples * 64u) return;
    float s = P.first ? 0.0f : P.sum[item];
    BounceHit B;
    if (!(P.rays[item].tmax < 0.0f) && P.flags[item] == 0u && bounce_hit(P, item, B)) {
        const trx_light &L = P.light;
        float g;
        if (L.kind == TRX_LIGHT_DIRECTIONAL) {
            float lx, ly, lz;
            light_toward(L, lx, ly, lz);
            g = dot3(B.nx, B.ny, B.nz, lx, ly, lz);
        } else {
            float Cx = L.position[0], Cy = L.position[1], Cz = L.position[2];
            if (L.kind == TRX_LIGHT_RECT) {
                Cx = (Cx + 0.5f * L.edge1[0]) + 0.5f * L.edge2[0];
                Cy = (Cy + 0.5f * L.edge1[1]) + 0.5f * L.edge2[1];
                Cz = (Cz + 0.5f * L.edge1[2]) + 0.5f * L.edge2[2];
            }
            const float vx = Cx - B.qx, vy = Cy - B.qy, vz = Cz - B.qz;
            const float q = dot3(vx, vy, vz, vx, vy, vz);
            const float inv = 1.0f / sqrtf(q);
            g = dot3(B.nx, B.ny, B.nz, vx * inv, vy * inv, vz * inv) / q;
        }
        if (g > 0.0f) s = s + L.intensity * g;
    }
    P.sum[item] = s;
}

// One lane per pixel of the chunk's tiles (the lanes outside the image too: their sums are 0): A (0 before the first samples
// of the tile) + the chunk's s, samples ascending.
__global__ void __launch_bounds__(256) k_bounce_gather(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * 64u) return;
    const uint32_t lt = item >> 6, k = item & 63u;
    const uint32_t from = lt * P.n_samples * 64u + k;
    float A = P.first ? 0.0f : P.acc[item];
    for (uint32_t s = 0; s < P.n_samples; s++) A = A + P.sum[from + s * 64u];
    P.acc[item] = A;
}

// One lane per pixel of the chunk's tiles: the pass's value.  base is read before value is written, by the same lane: they
// may be one buffer.  The surface is k_ao_rays' (kernels.h, surface_record): a caller's record that got the inert bounce
// ray keeps its base bit for bit.
//   SPARSE: one lane per cell of the low grid's tiles, the value at the cell's place in the low grid (there is no base: the
// dense statement with base = 0.0f); the primary record is that of the cell's pixel in the full image, and a cell whose
// pixel leaves the image gets +0.
template <bool SPARSE>
__global__ void __launch_bounds__(256) k_bounce_finish(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * 64u) return;
    uint32_t px, py, rec;
    if constexpr (SPARSE) {
        uint32_t cell;
        if (!tile_pixel(P.lo, P.tile0 + (item >> 6), item & 63u, px, py, cell)) return;
        px = px * P.stride + P.px0;
        py = py * P.stride + P.py0;
        float out = 0.0f;
        if (px < P.geom.width && py < P.geom.height) {
            const trx_hit ph = P.primary[(size_t)py * P.geom.width + px];
            if (surface_record(ph, P.n_tris)) out = out + (P.albedo * P.acc[item]) / (float)P.n_total;
        }
        P.value[cell] = out;
        return;
    }
    if (!tile_pixel(P.geom, P.tile0 + (item >> 6), item & 63u, px, py, rec)) return;
    const trx_hit ph = P.primary[rec];
    float out = P.base ? P.base[rec] : 0.0f;
    if (surface_record(ph, P.n_tris)) out = out + (P.albedo * P.acc[item]) / (float)P.n_total;
    P.value[rec] = out;
}

// k_bounce_gather in colour (include/trx.h, rule 5c): one lane per pixel of the chunk's tiles, three running sums per lane
// (plane c of acc at c * n_tiles * 64).  Per sample the wave's 64 lanes read 64 consecutive floats of sum, 64 consecutive hits
// and the tmax word of 64 consecutive bounce rays; the u16 index and the 24 B material are gathers into tables of at most
// 1.5 MiB that stay in cache.  A bounce without a surface (bounce_hit's test) adds nothing.  hit.prim is the walk's own answer
// and every index of tri_material was checked against the table on upload: the prim < n_tris test is surface_record's, for a
// scratch that holds anything else.  A streaming kernel: no scratch, no LDS.
__global__ void __launch_bounds__(256) k_bounce_gather_rgb(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lanes = P.n_tiles * 64u;
    if (item >= lanes) return;
    const uint32_t lt = item >> 6, k = item & 63u;
    const uint32_t from = lt * P.n_samples * 64u + k;
    float Ar = 0.0f, Ag = 0.0f, Ab = 0.0f;
    if (!P.first) {
        Ar = P.acc[item];
        Ag = P.acc[lanes + item];
        Ab = P.acc[2u * lanes + item];
    }
    for (uint32_t s = 0; s < P.n_samples; s++) {
        const uint32_t index = from + s * 64u;
        const float sf = P.sum[index];
        const float tmax = P.bounce_rays[index].tmax;
        const trx_hit bh = P.bounce_hits[index];
        if (tmax < 0.0f || !surface_record(bh, P.n_tris)) continue;
        const float2 *mp = reinterpret_cast<const float2 *>(P.materials + P.tri_material[bh.prim]);
        const float2 m0 = mp[0], m1 = mp[1], m2 = mp[2]; // {albedo r, g}, {albedo b, emission r}, {emission g, b}
        Ar = Ar + (m0.x * sf + m1.y);
        Ag = Ag + (m0.y * sf + m2.x);
        Ab = Ab + (m1.x * sf + m2.y);
    }
    P.acc[item] = Ar;
    P.acc[lanes + item] = Ag;
    P.acc[2u * lanes + item] = Ab;
}

// k_bounce_finish in colour: three planes of `plane` floats, out_c = A_c / n_total at a surface record (k_bounce_finish's
// surface and cell -> pixel mapping), +0 elsewhere; there is no base.
template <int SPARSE> // (an int: tests select the grey kernels' sparse instantiations by the bool's mangling)
__global__ void __launch_bounds__(256) k_bounce_finish_rgb(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lanes = P.n_tiles * 64u;
    if (item >= lanes) return;
    uint32_t px, py, rec;
    bool surf;
    if constexpr (SPARSE) {
        if (!tile_pixel(P.lo, P.tile0 + (item >> 6), item & 63u, px, py, rec)) return;
        px = px * P.stride + P.px0;
        py = py * P.stride + P.py0;
        surf = px < P.geom.width && py < P.geom.height && surface_record(P.primary[(size_t)py * P.geom.width + px], P.n_tris);
    } else {
        if (!tile_pixel(P.geom, P.tile0 + (item >> 6), item & 63u, px, py, rec)) return;
        surf = surface_record(P.primary[rec], P.n_tris);
    }
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (surf) {
        const float n = (float)P.n_total;
        r = P.acc[item] / n;
        g = P.acc[lanes + item] / n;
        b = P.acc[2u * lanes + item] / n;
    }
    if (rec >= P.plane) return; // (never: the launch checked the planes against the geometry)
    P.value[rec] = r;
    P.value[(size_t)P.plane + rec] = g;
    P.value[2u * (size_t)P.plane + rec] = b;
}

// Emissive triangles as sampled lights (include/trx.h, "emitters"; kernels.h, EmitterBuildParams / EmitterParams).
// One lane per emitter: the world-space record of the (instance, prim) pair from the scene's own triangle record - V0,
// E1 = -e1 (the record stores v0 - v1), E2 = e2 - points and edges through the instance's object-to-world matrix in the
// header's association, NG = cross(E1, E2) of the world-space edges.  kinv is the host's to fill in.  64 B written per lane.
__global__ void __launch_bounds__(256) k_emitter_build(const EmitterBuildParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n) return;
    const uint2 pr = P.pairs[i];
    float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e1 = v0, e2 = v0, ng = v0;
    if (pr.y < P.n_tris && (!P.o2w || pr.x < P.n_inst)) { // (the host formed every pair from the scene's own tables)
        const float4 *tp = P.tris + (size_t)pr.y * 3;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        float px = a.x, py = a.y, pz = a.z;
        float ax = -b.x, ay = -b.y, az = -b.z;
        float bx = c.x, by = c.y, bz = c.z;
        if (P.o2w) {
            const float *m = P.o2w + (size_t)pr.x * 16; // m[c * 4 + r]
            const float wx = ((m[0] * px + m[4] * py) + m[8] * pz) + m[12];
            const float wy = ((m[1] * px + m[5] * py) + m[9] * pz) + m[13];
            const float wz = ((m[2] * px + m[6] * py) + m[10] * pz) + m[14];
            px = wx; py = wy; pz = wz;
            const float ux = (m[0] * ax + m[4] * ay) + m[8] * az;
            const float uy = (m[1] * ax + m[5] * ay) + m[9] * az;
            const float uz = (m[2] * ax + m[6] * ay) + m[10] * az;
            ax = ux; ay = uy; az = uz;
            const float tx = (m[0] * bx + m[4] * by) + m[8] * bz;
            const float ty = (m[1] * bx + m[5] * by) + m[9] * bz;
            const float tz = (m[2] * bx + m[6] * by) + m[10] * bz;
            bx = tx; by = ty; bz = tz;
        }
        v0 = make_float4(px, py, pz, 0.0f);
        e1 = make_float4(ax, ay, az, __uint_as_float((uint32_t)P.tri_material[pr.y]));
        e2 = make_float4(bx, by, bz, __uint_as_float(pr.y));
        ng = make_float4(ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, __uint_as_float(pr.x));
    }
    float4 *out = P.out + (size_t)i * 4;
    out[0] = v0;
    out[1] = e1;
    out[2] = e2;
    out[3] = ng;
}

// Selection (include/trx.h): j = the number of i in 0 .. n - 2 with c[i] <= u0, found by bisection over the non-decreasing c
// - at most 20 steps for TRX_MAX_EMITTERS, no step at all for one emitter; no clamp, no special value of u0 (a NaN reaches
// no c[i]: emitter 0).  The result is below n whatever u0 is.
__device__ __forceinline__ uint32_t emitter_select(const float *cdf, uint32_t n_emitters, float u0) {
    uint32_t lo = 0u, hi = n_emitters - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] <= u0) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_emitter_select(const EmitterSelectParams P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n) return;
    P.j[i] = emitter_select(P.cdf, P.n_emitters, P.u0[i]);
}

// Rules E2 to E4 for one sample at the point o with the flipped normal n: the emitter, the point on it, the shadow ray (a, b:
// left as they are - the inert ray - where no ray is cast) and the geometric weight; false (wgeo untouched) where the sample
// contributes nothing.  One 64-byte gather into the table per lane, and the search.
__device__ __forceinline__ bool emitter_sample(const float4 *emitters, const float *cdf, uint32_t n_emitters, uint32_t px, uint32_t py,
                                               uint32_t se, float emitter_eps, float ox, float oy, float oz, float nx, float ny, float nz,
                                               float4 &a, float4 &b, float &wgeo, uint32_t &j) {
    const float u0 = hash_noise(px, py, se);
    const float u1 = hash_noise(px, py, se + 1024u);
    const float u2 = hash_noise(px, py, se + 4096u);
    j = emitter_select(cdf, n_emitters, u0);
    const float4 *ep = emitters + (size_t)j * 4;
    const float4 V0 = ep[0], E1 = ep[1], E2 = ep[2], NG = ep[3];
    const float su = sqrtf(u1);
    const float b1 = su * (1.0f - u2);
    const float b2 = su * u2;
    const float yx = (V0.x + b1 * E1.x) + b2 * E2.x;
    const float yy = (V0.y + b1 * E1.y) + b2 * E2.y;
    const float yz = (V0.z + b1 * E1.z) + b2 * E2.z;
    const float vx = yx - ox, vy = yy - oy, vz = yz - oz;
    const float q = dot3(vx, vy, vz, vx, vy, vz);
    const float dist = sqrtf(q);
    const float inv = 1.0f / dist;
    const float lx = vx * inv, ly = vy * inv, lz = vz * inv;
    const float tmax = dist - dist * emitter_eps;
    const float c = dot3(nx, ny, nz, lx, ly, lz);
    const float ar = 0.5f * fabsf(dot3(NG.x, NG.y, NG.z, lx, ly, lz));
    const float wg = ((c * ar) / q) * V0.w;
    if (!(c > 0.0f && wg > 0.0f && wg < __builtin_inff())) return false; // (NaN fails: a light at the hit point, a zero-area or edge-on emitter)
    a.x = ox; a.y = oy; a.z = oz;
    b = make_float4(lx, ly, lz, tmax);
    wgeo = wg;
    return true;
}

// The shadow ray of every (tile, sample, pixel) toward the emitter its noise selects: k_light_rays up to the origin - the
// addressing, the primary direction, the flipped normal, o with shadow_eps (rule E1 is THE SHADOW RAY's statement) - then
// emitter_sample.  In scratch layout wgeo (+0 where the inert ray went) and j go beside the ray.  A streaming kernel like
// k_light_rays, plus the 64-byte table gather and the search; 32 (+ 8) B written.
__global__ void __launch_bounds__(256) k_emitter_rays(const EmitterParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * P.n_samples * 64u) return;
    const uint32_t unit = item >> 6, k = item & 63u;
    const uint32_t lt = unit / P.n_samples, sample = unit - lt * P.n_samples;
    uint32_t px, py, rec;
    const bool inside = tile_pixel(P.geom, P.tile0 + lt, k, px, py, rec);
    if (!inside && !P.scratch) return; // (the trace writes no record for it either)
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    float wgeo = 0.0f;
    uint32_t j = 0u;
    trx_hit ph;
    ph.t = __builtin_inff();
    ph.prim = TRX_INVALID;
    if (inside) ph = P.primary[rec];
    if (surface_record(ph, P.n_tris)) { // (kernels.h: a caller's record that fails it is a miss - the inert ray)
        float dx, dy, dz;
        primary_dir(P.view, P.geom.width, P.geom.height, px, py, dx, dy, dz);
        const float4 *tp = P.tris + (size_t)ph.prim * 3;
        float nx = tp[0].w, ny = tp[1].w, nz = tp[2].w; // cross(e1, e2)
        if (P.inst_xform) {
            const uint32_t pi = P.primary_inst[rec];
            if (instance_row(pi, P.n_inst)) {
                const float4 *m = P.inst_xform + (size_t)pi * 3;
                const float3 w = normal_to_world(m[0], m[1], m[2], nx, ny, nz);
                nx = w.x; ny = w.y; nz = w.z;
            }
        }
        const float ninv = 1.0f / sqrtf(dot3(nx, ny, nz, nx, ny, nz));
        nx *= ninv; ny *= ninv; nz *= ninv;
        const float nd = (nx * -dx + ny * -dy) + nz * -dz;
        const float sg = copysignf(1.0f, nd);
        nx *= sg; ny *= sg; nz *= sg;
        const float ox = (P.view.eye[0] + dx * ph.t) - dx * P.shadow_eps;
        const float oy = (P.view.eye[1] + dy * ph.t) - dy * P.shadow_eps;
        const float oz = (P.view.eye[2] + dz * ph.t) - dz * P.shadow_eps;
        emitter_sample(P.emitters, P.cdf, P.n_emitters, px, py, P.seed0 + sample, P.emitter_eps, ox, oy, oz, nx, ny, nz, a, b, wgeo, j);
    }
    const uint32_t index = P.scratch ? item : rec;
    float4 *out = reinterpret_cast<float4 *>(P.rays + index);
    out[0] = a;
    out[1] = b;
    if (P.wgeo) {
        P.wgeo[index] = wgeo;
        P.pick[index] = j;
    }
}

// One lane per pixel of the chunk's tiles (rule E5): three running sums (k_bounce_gather_rgb's layout of acc), samples
// ascending - wgeo * emission_c of the emitter's material where the ray was cast (wgeo > 0) and is not occluded.  Per sample
// the wave reads 64 consecutive floats, indices and flags; the emitter's material index and the 12 B of emission are gathers
// into tables that stay in cache.  With `last` the sums are not stored: the lane writes the pass's value, base read first.
__global__ void __launch_bounds__(256) k_emitter_gather_rgb(const EmitterParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lanes = P.n_tiles * 64u;
    if (item >= lanes) return;
    const uint32_t lt = item >> 6, k = item & 63u;
    const uint32_t from = lt * P.n_samples * 64u + k;
    float Ar = 0.0f, Ag = 0.0f, Ab = 0.0f;
    if (!P.first) {
        Ar = P.acc[item];
        Ag = P.acc[lanes + item];
        Ab = P.acc[2u * lanes + item];
    }
    for (uint32_t s = 0; s < P.n_samples; s++) {
        const uint32_t index = from + s * 64u;
        const float wg = P.wgeo[index];
        const uint32_t j = P.pick[index];
        if (!(wg > 0.0f) || P.flags[index] != 0u || j >= P.n_emitters) continue;
        const uint32_t m = __float_as_uint(P.emitters[(size_t)j * 4 + 1].w);
        const trx_material *mp = P.materials + m;
        Ar = Ar + wg * mp->emission[0];
        Ag = Ag + wg * mp->emission[1];
        Ab = Ab + wg * mp->emission[2];
    }
    if (!P.last) {
        P.acc[item] = Ar;
        P.acc[lanes + item] = Ag;
        P.acc[2u * lanes + item] = Ab;
        return;
    }
    uint32_t px, py, rec;
    if (!tile_pixel(P.geom, P.tile0 + lt, k, px, py, rec)) return;
    if (rec >= P.plane) return; // (never: the launch checked the planes against the geometry)
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (P.base) {
        r = P.base[rec];
        g = P.base[(size_t)P.plane + rec];
        b = P.base[2u * (size_t)P.plane + rec];
    }
    if (surface_record(P.primary[rec], P.n_tris)) {
        const float n = (float)P.n_total;
        r = r + Ar / n;
        g = g + Ag / n;
        b = b + Ab / n;
    }
    P.value[rec] = r;
    P.value[(size_t)P.plane + rec] = g;
    P.value[2u * (size_t)P.plane + rec] = b;
}

// Emitters at bounce hits (rule 5e): k_bounce_light_rays with the light replaced by emitter_sample at the bounce hit - its
// addressing, its sparse instantiation (the noise at the cell's pixel of the full image), o = Q - d * shadow_eps, the
// attribute normal flipped against d.  Scratch layout only: wgeo and j go beside the ray.
template <int SPARSE>
__global__ void __launch_bounds__(256) k_bounce_emitter_rays(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= P.n_tiles * P.n_samples * 64u) return;
    const uint32_t unit = item >> 6, k = item & 63u;
    const uint32_t lt = unit / P.n_samples, sample = unit - lt * P.n_samples;
    uint32_t px, py, rec;
    if constexpr (SPARSE) {
        uint32_t cx, cy;
        tile_pixel(P.lo, P.tile0 + lt, k, cx, cy, rec);
        px = cx * P.stride + P.px0;
        py = cy * P.stride + P.py0;
    } else {
        tile_pixel(P.geom, P.tile0 + lt, k, px, py, rec);
    }
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    float wgeo = 0.0f;
    uint32_t j = 0u;
    BounceHit B;
    if (bounce_hit(P, item, B)) { // (a lane outside the image reads the inert bounce ray k_ao_rays wrote there)
        const float ox = B.qx - B.dx * P.shadow_eps;
        const float oy = B.qy - B.dy * P.shadow_eps;
        const float oz = B.qz - B.dz * P.shadow_eps;
        emitter_sample(P.emitters, P.cdf, P.n_emitters, px, py, P.seed0 + sample, P.emitter_eps, ox, oy, oz, B.nx, B.ny, B.nz, a, b, wgeo, j);
    }
    float4 *out = reinterpret_cast<float4 *>(P.rays + item);
    out[0] = a;
    out[1] = b;
    P.wgeo[item] = wgeo;
    P.pick[item] = j;
}

// k_bounce_gather_rgb under rule 5e: A_c = A_c + albedo_c(m) * (s + X_c), X_c = wgeo * emission_c(emitter) where that ray was
// cast and is not occluded (flags holds the emitter rays' answers: the lights' were consumed by k_bounce_weight), else +0;
// the bounce triangle's own emission is not added.
__global__ void __launch_bounds__(256) k_bounce_emitter_gather(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lanes = P.n_tiles * 64u;
    if (item >= lanes) return;
    const uint32_t lt = item >> 6, k = item & 63u;
    const uint32_t from = lt * P.n_samples * 64u + k;
    float Ar = 0.0f, Ag = 0.0f, Ab = 0.0f;
    if (!P.first) {
        Ar = P.acc[item];
        Ag = P.acc[lanes + item];
        Ab = P.acc[2u * lanes + item];
    }
    for (uint32_t s = 0; s < P.n_samples; s++) {
        const uint32_t index = from + s * 64u;
        const float sf = P.has_lights ? P.sum[index] : 0.0f;
        const float tmax = P.bounce_rays[index].tmax;
        const trx_hit bh = P.bounce_hits[index];
        if (tmax < 0.0f || !surface_record(bh, P.n_tris)) continue;
        const float2 *mp = reinterpret_cast<const float2 *>(P.materials + P.tri_material[bh.prim]);
        const float2 m0 = mp[0], m1 = mp[1]; // {albedo r, g}, {albedo b, emission r}
        float Xr = 0.0f, Xg = 0.0f, Xb = 0.0f;
        const float wg = P.wgeo[index];
        const uint32_t j = P.pick[index];
        if (wg > 0.0f && P.flags[index] == 0u && j < P.n_emitters) {
            const trx_material *ep = P.materials + __float_as_uint(P.emitters[(size_t)j * 4 + 1].w);
            Xr = wg * ep->emission[0];
            Xg = wg * ep->emission[1];
            Xb = wg * ep->emission[2];
        }
        Ar = Ar + m0.x * (sf + Xr);
        Ag = Ag + m0.y * (sf + Xg);
        Ab = Ab + m1.x * (sf + Xb);
    }
    P.acc[item] = Ar;
    P.acc[lanes + item] = Ag;
    P.acc[2u * lanes + item] = Ab;
}

// k_bounce_gather_rgb (EMITTERS false, rule 5c) and k_bounce_emitter_gather (EMITTERS true, rule 5e) with albedo_c(m) replaced
// by THE TEXTURED ALBEDO (include/trx.h) sampled at the bounce hit: u, v of bounce_attr[index], the texcoords of bounce_hit.prim,
// the texture of its material (textured_albedo, texture_dev.h: the statement k_surface_albedo shares).  Everything else is those
// kernels' word for word - the same reads, the same order of the float sums.  Launched only with a texcoord table and a
// texture set on the scene (BounceParams::tex); per sample the 8 B of u, v, and for a textured material the descriptor, 24 B of
// texcoords and one or four texels, are gathers on top of theirs.  No scratch, no LDS.
template <bool EMITTERS>
__global__ void __launch_bounds__(256) k_bounce_gather_tex(const BounceParams P) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lanes = P.n_tiles * 64u;
    if (item >= lanes) return;
    const uint32_t lt = item >> 6, k = item & 63u;
    const uint32_t from = lt * P.n_samples * 64u + k;
    float Ar = 0.0f, Ag = 0.0f, Ab = 0.0f;
    if (!P.first) {
        Ar = P.acc[item];
        Ag = P.acc[lanes + item];
        Ab = P.acc[2u * lanes + item];
    }
    for (uint32_t s = 0; s < P.n_samples; s++) {
        const uint32_t index = from + s * 64u;
        const float sf = !EMITTERS || P.has_lights ? P.sum[index] : 0.0f;
        const float tmax = P.bounce_rays[index].tmax;
        const trx_hit bh = P.bounce_hits[index];
        if (tmax < 0.0f || !surface_record(bh, P.n_tris)) continue;
        const uint32_t m = P.tri_material[bh.prim];
        const float2 *mp = reinterpret_cast<const float2 *>(P.materials + m);
        const float2 m0 = mp[0], m1 = mp[1], m2 = mp[2]; // {albedo r, g}, {albedo b, emission r}, {emission g, b}
        const float2 uv = *reinterpret_cast<const float2 *>(P.bounce_attr + index); // {u, v}: the record's first 8 bytes
        float ar = m0.x, ag = m0.y, ab = m1.x;
        textured_albedo(P.tex, bh.prim, m, uv.x, uv.y, ar, ag, ab);
        if (EMITTERS) {
            float Xr = 0.0f, Xg = 0.0f, Xb = 0.0f;
            const float wg = P.wgeo[index];
            const uint32_t j = P.pick[index];
            if (wg > 0.0f && P.flags[index] == 0u && j < P.n_emitters) {
                const trx_material *ep = P.materials + __float_as_uint(P.emitters[(size_t)j * 4 + 1].w);
                Xr = wg * ep->emission[0];
                Xg = wg * ep->emission[1];
                Xb = wg * ep->emission[2];
            }
            Ar = Ar + ar * (sf + Xr);
            Ag = Ag + ag * (sf + Xg);
            Ab = Ab + ab * (sf + Xb);
        } else {
            Ar = Ar + (ar * sf + m1.y);
            Ag = Ag + (ag * sf + m2.x);
            Ab = Ab + (ab * sf + m2.y);
        }
    }
    P.acc[item] = Ar;
    P.acc[lanes + item] = Ag;
    P.acc[2u * lanes + item] = Ab;
}

} // namespace

// (the sparse form of the bounce kernels exists for the scratch layout of a whole image only: what bounds their cell -> pixel
// mapping and k_bounce_finish's writes to the low grid)
static bool bounce_sparse_ok(const BounceParams &p) {
    return p.scratch && p.stride <= TRX_MAX_AO_STRIDE && p.px0 < p.stride && p.py0 < p.stride && p.lo.shard_count == 1u && !p.lo.compact &&
           p.geom.shard_count == 1u && !p.geom.compact && p.lo.width == (p.geom.width + p.stride - 1u) / p.stride &&
           p.lo.height == (p.geom.height + p.stride - 1u) / p.stride;
}

// (the emitter mode of the bounce kernels: the table, its search array, a count the search cannot leave, and the scratch beside the rays)
static bool bounce_emitters_ok(const BounceParams &p) {
    return p.scratch && p.emitters && p.cdf && p.wgeo && p.pick && p.materials && p.n_emitters >= 1u && p.n_emitters <= TRX_MAX_EMITTERS;
}

hipError_t launch_bounce_emitter_rays(const BounceParams &p, hipStream_t stream) {
    const uint64_t n = (uint64_t)p.n_tiles * p.n_samples * 64u;
    if (n == 0) return hipSuccess;
    if (n > 0xffffff00ull || !bounce_emitters_ok(p)) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n + 255u) / 256u));
    if (p.stride) {
        if (!bounce_sparse_ok(p)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_bounce_emitter_rays<1>, grid, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(k_bounce_emitter_rays<0>, grid, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_emitter_build(const EmitterBuildParams &p, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.n > TRX_MAX_EMITTERS || !p.tris || !p.pairs || !p.tri_material || !p.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_emitter_build, dim3((p.n + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_emitter_select(const EmitterSelectParams &p, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.n > 0xffffff00u || !p.cdf || !p.u0 || !p.j || p.n_emitters < 1u || p.n_emitters > TRX_MAX_EMITTERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_emitter_select, dim3((p.n + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

static bool emitter_params_ok(const EmitterParams &p) {
    return p.emitters && p.cdf && p.n_emitters >= 1u && p.n_emitters <= TRX_MAX_EMITTERS;
}

hipError_t launch_emitter_rays(const EmitterParams &p, hipStream_t stream) {
    const uint64_t n = (uint64_t)p.n_tiles * p.n_samples * 64u;
    if (n == 0) return hipSuccess;
    if (n > 0xffffff00ull || !emitter_params_ok(p) || (!p.scratch && p.n_samples != 1u) || (p.wgeo && (!p.pick || !p.scratch))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_emitter_rays, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_emitter_gather(const EmitterParams &p, hipStream_t stream) {
    if (p.n_tiles == 0) return hipSuccess;
    if (p.n_tiles > 0x3ffffffu || !emitter_params_ok(p) || !p.materials || !p.wgeo || !p.pick || !p.acc || !p.scratch || p.n_total == 0u)
        return hipErrorInvalidValue;
    if (p.last) {
        // (the three planes hold every record the kernel can form: k_emitter_gather_rgb writes nothing at or past `plane`)
        const uint64_t need = p.geom.compact ? ((uint64_t)p.tile0 + p.n_tiles) * 64u : (uint64_t)p.geom.width * p.geom.height;
        if (!p.value || p.plane < need) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_emitter_gather_rgb, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_bounce_light_rays(const BounceParams &p, hipStream_t stream) {
    const uint64_t n = (uint64_t)p.n_tiles * p.n_samples * 64u;
    if (n == 0) return hipSuccess;
    if (n > 0xffffff00ull || p.light.kind > TRX_LIGHT_RECT || (!p.scratch && p.n_samples != 1u)) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n + 255u) / 256u));
    if (p.stride) {
        if (!bounce_sparse_ok(p)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_bounce_light_rays<true>, grid, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(k_bounce_light_rays<false>, grid, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_bounce_weight(const BounceParams &p, hipStream_t stream) {
    const uint64_t n = (uint64_t)p.n_tiles * p.n_samples * 64u;
    if (n == 0) return hipSuccess;
    if (n > 0xffffff00ull || p.light.kind > TRX_LIGHT_RECT || !p.scratch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bounce_weight, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_bounce_gather(const BounceParams &p, hipStream_t stream) {
    if (p.n_tiles == 0) return hipSuccess;
    if (p.n_tiles > 0x3ffffffu) return hipErrorInvalidValue;
    if (p.materials) {
        if (!p.tri_material || !p.scratch) return hipErrorInvalidValue;
        if (p.tex.texcoords && p.tex.descs) { // the textured gathers (a texture set is whole or absent; the attributes are read)
            if (!p.tex.texels || !p.tex.material_texture || !p.tex.srgb || !p.bounce_attr) return hipErrorInvalidValue;
            if (p.emitters) {
                if (!bounce_emitters_ok(p)) return hipErrorInvalidValue;
                hipLaunchKernelGGL(k_bounce_gather_tex<true>, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
            } else {
                hipLaunchKernelGGL(k_bounce_gather_tex<false>, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
            }
            return hipGetLastError();
        }
        if (p.emitters) {
            if (!bounce_emitters_ok(p)) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_bounce_emitter_gather, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(k_bounce_gather_rgb, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_bounce_gather, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_bounce_finish(const BounceParams &p, hipStream_t stream) {
    if (p.n_tiles == 0) return hipSuccess;
    if (p.n_tiles > 0x3ffffffu || p.n_total == 0u) return hipErrorInvalidValue;
    const dim3 grid((p.n_tiles * 64u + 255u) / 256u);
    if (p.materials) {
        // (the three planes hold every record the kernel can form: k_bounce_finish_rgb writes nothing at or past `plane`)
        if (p.base) return hipErrorInvalidValue;
        if (p.stride) {
            if (!bounce_sparse_ok(p) || (uint64_t)p.plane != (uint64_t)p.lo.width * p.lo.height) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_bounce_finish_rgb<1>, grid, dim3(256), 0, stream, p);
        } else {
            const uint64_t need = p.geom.compact ? ((uint64_t)p.tile0 + p.n_tiles) * 64u : (uint64_t)p.geom.width * p.geom.height;
            if (p.plane < need) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_bounce_finish_rgb<0>, grid, dim3(256), 0, stream, p);
        }
        return hipGetLastError();
    }
    if (p.stride) {
        if (!bounce_sparse_ok(p) || p.base) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_bounce_finish<true>, grid, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(k_bounce_finish<false>, grid, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_ao_rays(const AoRaysParams &p, hipStream_t stream) {
    const uint64_t n = (uint64_t)p.n_tiles * p.n_samples * 64u;
    if (n == 0) return hipSuccess;
    if (n > 0xffffff00ull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n + 255u) / 256u));
    if (p.stride) {
        // (the sparse form exists for the scratch layout of a whole image only)
        if (!p.scratch || p.stride > TRX_MAX_AO_STRIDE || p.px0 >= p.stride || p.py0 >= p.stride || p.lo.shard_count != 1u || p.lo.compact ||
            p.geom.shard_count != 1u || p.geom.compact)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_ao_rays<true>, grid, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(k_ao_rays<false>, grid, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_ao_reduce(const AoRaysParams &p, hipStream_t stream) {
    if (p.n_tiles == 0) return hipSuccess;
    const dim3 grid((p.n_tiles * 64u + 255u) / 256u);
    if (p.stride) hipLaunchKernelGGL(k_ao_reduce<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(k_ao_reduce<false>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_light_rays(const LightRaysParams &p, hipStream_t stream) {
    const uint64_t n = (uint64_t)p.n_tiles * p.n_samples * 64u;
    if (n == 0) return hipSuccess;
    if (n > 0xffffff00ull || p.light.kind > TRX_LIGHT_RECT) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_light_rays, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_light_reduce(const LightRaysParams &p, hipStream_t stream) {
    if (p.n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_light_reduce, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_light_term(const LightTermParams &p, hipStream_t stream) {
    if (p.n_tiles == 0) return hipSuccess;
    if (p.n_lights > TRX_MAX_LIGHTS || p.n_tiles > 0x3ffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_light_term, dim3((p.n_tiles * 64u + 255u) / 256u), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_hit_attr(const HitAttrParams &p, int mode, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    const dim3 grid((p.n_items + 255u) / 256u), block(256);
    if (mode == kAttrPrimary) hipLaunchKernelGGL(k_hit_attr<kAttrPrimary>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(k_hit_attr<kAttrRays>, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_shading_normal(const ShadingNormalParams &p, int mode, hipStream_t stream) {
    if (p.n_items == 0) return hipSuccess;
    const dim3 grid((p.n_items + 255u) / 256u), block(256);
    if (mode == kAttrPrimary) hipLaunchKernelGGL(k_shading_normal<kAttrPrimary>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(k_shading_normal<kAttrRays>, grid, block, 0, stream, p);
    return hipGetLastError();
}

int trace_grid_size(int device, int mode, bool tlas, uint32_t sem, bool count) {
    (void)mode;
    (void)sem;
    (void)count;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
    // Every product variant is held to <= 128 VGPRs without scratch (tests/test_kernel_resources.py) and owns the same
    // kLdsBytesPerWave of LDS, so all of them fit four waves to a SIMD (16 to a CU: 16 x 10 240 B = the 160 KB exactly): the
    // grid sized from one variant per TLAS flavour is resident for every variant, whatever the workgroup shape
    int per_cu = tlas ? occupancy_one<kModePrimary, true, 1, false, false>() : occupancy_one<kModePrimary, false, 1, false, false>();
    if (per_cu <= 0) per_cu = 8;
    if (per_cu > 32) per_cu = 32;
    return per_cu * prop.multiProcessorCount;
}

hipError_t launch_trace(const TraceParamsTlas &p, int mode, bool tlas, uint32_t sem, bool count, bool pipe, int grid,
                        hipStream_t stream) {
    const int node = node_variant(sem);
    switch (mode) {
    case kModePrimary: return launch_mode<kModePrimary>(p, tlas, node, count, pipe, grid, stream);
    case kModeAo: return launch_mode<kModeAo>(p, tlas, node, count, pipe, grid, stream);
    case kModeRays: return launch_mode<kModeRays>(p, tlas, node, count, pipe, grid, stream);
    case kModeFused: return launch_mode<kModeFused>(p, tlas, node, count, pipe, grid, stream);
    case kModeService: return launch_mode<kModeService>(p, tlas, node, count, pipe, grid, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace trx
