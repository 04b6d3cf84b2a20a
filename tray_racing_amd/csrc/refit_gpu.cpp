// refit_gpu.cpp - the device half of the BVH refit (refit_gpu.h; driven by api_refit.cpp): the finiteness check that runs
// before anything is written, the triangle records, one launch per height level over that level's node list, and the
// reduction behind the scene's exp_exact word and diagonal.
//
// One launch per level rather than one bottom-up kernel with arrival counters: the eight XCDs' L2s are not coherent with
// each other and a CU's L1 is not refreshed by another CU's stores, so a one-launch form needs agent-scope release /
// acquire on every hand-off between a child and its parent; a kernel boundary gives that visibility for free.  The levels
// are few (tree height: about a dozen single-level, the sum of both levels' heights two-level).
#include "refit_gpu.h"

namespace trx {
namespace {

constexpr uint32_t kBlock = 256;

inline uint32_t blocks_for(uint64_t n, uint32_t cap) {
    const uint64_t b = (n + kBlock - 1) / kBlock;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

__device__ inline bool finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(kBlock) void k_refit_check(const uint32_t *v, uint64_t n, RefitResult *res) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) bad |= !finite_bits(v[i]);
    if (bad) atomicOr(&res->bad_input, 1u);
}

__global__ __launch_bounds__(kBlock) void k_refit_tris(const float *v, uint64_t n, float4 *tris) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        float x[9];
        for (int k = 0; k < 9; k++) x[k] = v[i * 9 + k];
        TriDev t;
        refit_tri_record(x, t);
        tris[i * 3 + 0] = make_float4(t.v0[0], t.v0[1], t.v0[2], t.ngx);
        tris[i * 3 + 1] = make_float4(t.e1[0], t.e1[1], t.e1[2], t.ngy);
        tris[i * 3 + 2] = make_float4(t.e2[0], t.e2[1], t.e2[2], t.ngz);
    }
}

__global__ __launch_bounds__(kBlock) void k_refit_level(RefitCtx ctx, const uint32_t *order, uint32_t begin, uint32_t count) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= count) return;
    refit_node(ctx, order[begin + t]);
}

// api.cpp (trx_scene_create) derives the same two flags from the host copy of the nodes
__global__ __launch_bounds__(kBlock) void k_refit_stats(const uint4 *nodes, uint64_t n, uint32_t root, RefitResult *res) {
    bool e_ok = true, p_ok = true;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint4 w = nodes[i * 5];
        const uint32_t pw[3] = {w.x, w.y, w.z};
        for (int k = 0; k < 3; k++) {
            const uint32_t eb = (w.w >> (8 * k)) & 0xffu;
            e_ok = e_ok && (eb == 0u || eb >= 21u);
            const float a = fabsf(__uint_as_float(pw[k]));
            p_ok = p_ok && (pw[k] == 0u || (a >= 0x1p-36f && a <= 0x1p59f));
        }
        if (i == root) res->root_e = w.w & 0xffffffu;
    }
    if (!e_ok) atomicAnd(&res->e_ok, 0u);
    if (!p_ok) atomicAnd(&res->p_ok, 0u);
}

} // namespace

bool refit_launch_check(const float *d_verts, uint64_t n_tris, RefitResult *d_result, hipStream_t stream) {
    const uint64_t n = n_tris * 9;
    hipLaunchKernelGGL(k_refit_check, dim3(blocks_for(n, 4096)), dim3(kBlock), 0, stream, (const uint32_t *)d_verts, n, d_result);
    return hipGetLastError() == hipSuccess;
}

bool refit_launch_tris(const float *d_verts, uint64_t n_tris, float4 *d_tris, hipStream_t stream) {
    if (n_tris == 0) return true;
    hipLaunchKernelGGL(k_refit_tris, dim3(blocks_for(n_tris, 8192)), dim3(kBlock), 0, stream, d_verts, n_tris, d_tris);
    return hipGetLastError() == hipSuccess;
}

bool refit_launch_level(const RefitCtx &ctx, const uint32_t *d_order, uint32_t begin, uint32_t count, hipStream_t stream) {
    if (count == 0) return true;
    hipLaunchKernelGGL(k_refit_level, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, ctx, d_order, begin, count);
    return hipGetLastError() == hipSuccess;
}

bool refit_launch_stats(const uint4 *d_nodes, uint64_t n_nodes, uint32_t root, RefitResult *d_result, hipStream_t stream) {
    hipLaunchKernelGGL(k_refit_stats, dim3(blocks_for(n_nodes, 1024)), dim3(kBlock), 0, stream, d_nodes, n_nodes, root, d_result);
    return hipGetLastError() == hipSuccess;
}

} // namespace trx
