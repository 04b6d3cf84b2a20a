// build_device.h - what the device stages of the build (ploc_gpu.cpp, reinsert_gpu.cpp, collapse_gpu.cpp) share beyond the
// rules of build_rules.h: error handling, the device switch, the explicit loads of a BVH2 node and the per-wave append; the
// level lists of a BVH2 (frontier expansion: a kernel and its host loop) are in build_levels.h for the two stages that walk
// a tree by levels.  HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "build_rules.h"
#include "hip_owned.h"

namespace trx {

using trxapi::DevBuf;
using trxapi::Event;

// in a function returning bool with a std::string `err` in scope
#define TRX_BUILD_TRY(expr)                                          \
    do {                                                             \
        hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess) {                                      \
            err = std::string(#expr) + ": " + hipGetErrorString(e_); \
            return false;                                            \
        }                                                            \
    } while (0)

constexpr int kBlock = 256;
inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// Makes `device` current; the caller's current device is put back when the scope ends, whatever happens in between.
class DeviceScope {
    int prev_ = -1;

  public:
    DeviceScope() = default;
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    ~DeviceScope() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    bool enter(int device, std::string &err) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
            err = "no HIP device " + std::to_string(device) + " for the GPU build stage";
            return false;
        }
        return reenter(device, err);
    }
    // ... a device that an earlier enter() has checked (the calls on an open reinsertion context)
    bool reenter(int device, std::string &err) {
        (void)hipGetDevice(&prev_);
        TRX_BUILD_TRY(hipSetDevice(device));
        return true;
    }
};

// 40 bytes, 8-byte aligned: five 8-byte loads
__device__ __forceinline__ Node2 load_node(const Node2 *nodes, uint32_t i) {
    const uint2 *p = reinterpret_cast<const uint2 *>(nodes + i);
    const uint2 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
    Node2 n;
    n.box.mn[0] = __uint_as_float(a.x); n.box.mn[1] = __uint_as_float(a.y); n.box.mn[2] = __uint_as_float(b.x);
    n.box.mx[0] = __uint_as_float(b.y); n.box.mx[1] = __uint_as_float(c.x); n.box.mx[2] = __uint_as_float(c.y);
    n.left = d.x; n.right = d.y; n.prim = e.x; n.count = e.y;
    return n;
}
__device__ __forceinline__ void load_links(const Node2 *nodes, uint32_t i, uint32_t &left, uint32_t &right, uint32_t &prim, uint32_t &count) {
    const uint2 *p = reinterpret_cast<const uint2 *>(nodes + i);
    const uint2 d = p[3], e = p[4];
    left = d.x; right = d.y; prim = e.x; count = e.y;
}

// `want` consecutive places at the end of a list whose length is *counter: one atomic per wave.
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, uint32_t want) {
    const uint32_t lane = __lane_id();
    uint32_t scan = want; // inclusive prefix sum over the wave
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(scan, d, 64);
        if ((int)lane >= d) scan += up;
    }
    const uint32_t total = __shfl(scan, 63, 64);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(counter, total);
    base = __shfl(base, 63, 64);
    return base + scan - want;
}

} // namespace trx
