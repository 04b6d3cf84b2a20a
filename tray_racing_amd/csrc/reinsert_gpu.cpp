// reinsert_gpu.cpp — the BVH2 reinsertion pass with one batch per iteration (Meister & Bittner 2018, "Parallel Reinsertion for
// Bounding Volume Hierarchy Optimization"; the pass obvhs runs after PLOC, knob reinsertion_batch_ratio behind the
// reference's -r, src/main.rs:113-118) on the GPU: one thread per candidate, every candidate of a batch against the same
// tree.  A search is a branch-and-bound walk of a few hundred dependent node reads - latency on a CPU core (2-3 s of a
// reference-default build of a 3.9 M triangle scene on 16 cores), throughput here.  Same search order, same tie rule, same
// box unions and half-areas (build_rules.h) as Reinserter::find in builder.cpp, so found[] is the host's found[], candidate
// for candidate (tests/test_gpu_builder.py).  The moves are applied here too (further down): the tree stays on the device
// from the first iteration to the last.
#include "reinsert_gpu.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>

#include "build_levels.h"

namespace trx {
namespace {

constexpr uint32_t kStackCap = 128; // entries per search (a DFS that pushes two and pops one per level: depth + 1)

// Reinserter::search: best place below `top` for a box of area `area`; `gain` is what the tree has saved so far by
// taking the node out.  The stack holds {gain, node}; an entry that cannot win is not even pushed (the host prunes it
// when it pops it: best_gain only grows in between, so the same entries are dropped, a little earlier).
__device__ __forceinline__ bool search_dev(const Node2 *nodes, uint2 *stk, uint32_t stride, uint32_t top, float gain,
                                           const Aabb &box, float area, uint32_t &best_to, float &best_gain) {
    uint32_t sp = 0;
    float g = gain;
    uint32_t id = top;
    bool have = true;
    for (;;) {
        if (!have) {
            if (sp == 0) return true;
            sp--;
            const uint2 e = stk[(size_t)sp * stride];
            g = __uint_as_float(e.x);
            id = e.y;
        }
        have = false;
        if (!(g - area > best_gain)) continue; // even a zero-growth insertion cannot win (nor a NaN: Reinserter::search)
        const Node2 dst = load_node(nodes, id);
        Aabb merged = dst.box;
        grow(merged, box);
        const float here = g - half_area(merged); // new inner node holding {dst, node}
        if (here > best_gain) {
            best_gain = here;
            best_to = id;
        }
        if (dst.count > 1) {
            // going below dst instead grows dst to `merged`
            const float below = here + half_area(dst.box);
            if (!(below - area > best_gain)) continue;
            // the host pushes left, then right, and pops right first: right is walked now, left waits
            if (sp + 1 > kStackCap) return false;
            stk[(size_t)sp * stride] = make_uint2(__float_as_uint(below), dst.left);
            sp++;
            g = below;
            id = dst.right;
            have = true;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_find(const Node2 *nodes, const uint32_t *parent, const uint32_t *cand, uint32_t n_cand,
                                                 uint32_t *found, uint2 *stacks) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    uint2 *const stk = stacks + tid;
    for (uint32_t k = tid; k < n_cand; k += stride) {
        const uint32_t from = cand[k];
        const uint32_t p = parent[from];
        if (p == 0u || p == kReinsertNone) { // the root's children stay (as on the host)
            found[k] = kReinsertNone;
            continue;
        }
        const Node2 self = load_node(nodes, from);
        const Aabb box = self.box;
        const float area = half_area(box);
        Node2 pn = load_node(nodes, p);
        float gain = half_area(pn.box); // p disappears
        float best_gain = 0.f;
        uint32_t best_to = kReinsertNone;
        if (!(gain < INFINITY)) { // overflowed half-areas: the node stays (Reinserter::find)
            found[k] = kReinsertNone;
            continue;
        }
        uint32_t sib = pn.left == from ? pn.right : pn.left;
        bool ok = search_dev(nodes, stk, stride, sib, gain, box, area, best_to, best_gain);
        Aabb shrunk = load_node(nodes, sib).box; // what the path node looks like without `from`
        uint32_t cur = p;
        while (ok) {
            const uint32_t up = parent[cur];
            if (up == kReinsertNone) break;
            const Node2 un = load_node(nodes, up);
            sib = un.left == cur ? un.right : un.left;
            ok = search_dev(nodes, stk, stride, sib, gain, box, area, best_to, best_gain);
            grow(shrunk, load_node(nodes, sib).box);
            gain += half_area(un.box) - half_area(shrunk);
            if (!(gain < INFINITY)) break;
            cur = up;
        }
        found[k] = ok ? best_to : kReinsertOverflow;
    }
}

// Candidate keys: {area bits, ~index} - descending key order is area descending, index ascending (areas are >= 0, so their
// bit patterns order like the floats); the root, its children and anything without a parent get key 0 and sort last.
__global__ void __launch_bounds__(kBlock) k_keys(const Node2 *nodes, const uint32_t *parent, uint32_t n, unsigned long long *keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long key = 0ull;
    if (i != 0u && parent[i] != 0u && parent[i] != kReinsertNone) {
        const Node2 nd = load_node(nodes, i);
        key = ((unsigned long long)__float_as_uint(half_area(nd.box)) << 32) | (unsigned long long)(~i);
    }
    keys[i] = key;
}
__global__ void __launch_bounds__(kBlock) k_ids(const unsigned long long *keys, uint32_t take, uint32_t *ids) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < take) ids[k] = ~(uint32_t)keys[k];
}

// ---- the moves of a whole iteration, applied on the device -------------------------------------------------------------
// Reinserter::apply_batch takes the candidates in order: a move is skipped when an earlier APPLIED move re-linked one of
// its six nodes, or when its target has meanwhile come to lie below the node it moves.  Without the second rule that is a
// greedy independent set in candidate order, which has one fixed point whatever order it is computed in: rounds of "claim
// my nodes with my index (atomic min); mine on all six -> accepted; lost one to an accepted move -> rejected".  The second
// rule is then CHECKED for the accepted moves, each against the tree as the accepted moves before it leave it (parent
// links followed through those moves' re-linkings); if no move trips it, the sequential pass would not have tripped it
// either and the accepted set is exactly what it applies - so it is applied here, all moves at once (their six-node sets
// are disjoint), and the boxes are recomputed level by level.  If one does trip it the iteration goes to the host.
struct Six {
    uint32_t from, p, s, g, to, tp; // p == kReinsertNone: this candidate has no move to make
};
enum : uint8_t { kNoMove = 0, kUndecided = 1, kAccepted = 2, kRejected = 3 };

__global__ void __launch_bounds__(kBlock) k_six(const Node2 *nodes, const uint32_t *parent, const uint32_t *cand, const uint32_t *found,
                                                uint32_t n_cand, Six *six, uint8_t *status) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_cand) return;
    Six m;
    m.from = cand[k];
    m.to = found[k];
    m.p = m.s = m.g = m.tp = kReinsertNone;
    bool ok = m.to != kReinsertNone && m.to != kReinsertOverflow;
    if (ok) {
        const uint32_t p = parent[m.from];
        ok = p != 0u && p != kReinsertNone && m.to != p && m.to != m.from && parent[m.to] != kReinsertNone;
        if (ok) {
            uint32_t left, right;
            {
                const uint2 d = reinterpret_cast<const uint2 *>(nodes + p)[3];
                left = d.x;
                right = d.y;
            }
            const uint32_t s = left == m.from ? right : left;
            ok = m.to != s; // already its sibling: nothing to gain
            if (ok) {
                m.p = p;
                m.s = s;
                m.g = parent[p];
                m.tp = parent[m.to];
            }
        }
    }
    six[k] = m;
    status[k] = ok ? kUndecided : kNoMove;
}
__global__ void __launch_bounds__(kBlock) k_overflowed(const uint32_t *found, uint32_t n_cand, uint32_t *flags) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_cand && found[k] == kReinsertOverflow) atomicOr(flags, 4u);
}
__global__ void __launch_bounds__(kBlock) k_claim(const Six *six, const uint8_t *status, uint32_t n_cand, uint32_t *claim, int reset) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_cand) return;
    const uint8_t st = status[k];
    if (st == kNoMove) return;
    const Six m = six[k];
    const uint32_t v[6] = {m.from, m.p, m.s, m.g, m.to, m.tp};
    if (reset) { // every node some candidate may claim: free again
        for (int i = 0; i < 6; i++) claim[v[i]] = kReinsertNone;
    } else if (st == kUndecided || st == kAccepted) {
        for (int i = 0; i < 6; i++) atomicMin(&claim[v[i]], k);
    }
}
__global__ void __launch_bounds__(kBlock) k_decide(const Six *six, uint8_t *status, uint32_t n_cand, const uint32_t *claim, uint32_t *undecided) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_cand || status[k] != kUndecided) return;
    const Six m = six[k];
    const uint32_t v[6] = {m.from, m.p, m.s, m.g, m.to, m.tp};
    bool mine = true, lost = false;
    for (int i = 0; i < 6; i++) {
        const uint32_t c = claim[v[i]];
        if (c != k) {
            mine = false;
            // (an accepted move's status is final; one accepted in this very launch may still read as undecided here:
            // the rejection then comes a round later)
            if (c < k && reinterpret_cast<const volatile uint8_t *>(status)[c] == kAccepted) lost = true;
        }
    }
    if (mine)
        status[k] = kAccepted;
    else if (lost)
        status[k] = kRejected;
    else
        atomicAdd(undecided, 1u);
}
// claim[] holds the accepted moves only.  Does `to` lie below `from` once the accepted moves before k are in?
__global__ void __launch_bounds__(kBlock) k_verify(const Six *six, const uint8_t *status, uint32_t n_cand, const uint32_t *parent,
                                                   const uint32_t *claim, uint32_t *flags) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_cand || status[k] != kAccepted) return;
    const Six m = six[k];
    uint32_t x = m.to;
    for (uint32_t steps = 0;; steps++) {
        if (steps > 65536u) { // (cannot happen on a tree: some earlier move must have tripped the rule itself)
            atomicOr(flags, 2u);
            return;
        }
        uint32_t up = parent[x];
        const uint32_t j = claim[x];
        if (j < k) { // x is re-linked by an accepted move that comes first
            const Six o = six[j];
            if (x == o.from || x == o.to) up = o.p;
            else if (x == o.p) up = o.tp;
            else if (x == o.s) up = o.g;
        }
        if (up == kReinsertNone) return;
        if (up == m.from) {
            atomicOr(flags, 1u);
            return;
        }
        x = up;
    }
}
// Reinserter::move's re-linking for every accepted move (the boxes follow in k_refit)
__global__ void __launch_bounds__(kBlock) k_apply(const Six *six, const uint8_t *status, uint32_t n_cand, Node2 *nodes, uint32_t *parent,
                                                  uint32_t *moved) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_cand || status[k] != kAccepted) return;
    const Six m = six[k];
    // replace_child(g, p, s)
    if (nodes[m.g].left == m.p) nodes[m.g].left = m.s; else nodes[m.g].right = m.s;
    parent[m.s] = m.g;
    // replace_child(tp, to, p): the target's parent as it is now (g and tp may be one node, s and tp too)
    const uint32_t tp = parent[m.to];
    if (nodes[tp].left == m.to) nodes[tp].left = m.p; else nodes[tp].right = m.p;
    parent[m.p] = tp;
    nodes[m.p].left = m.to;
    nodes[m.p].right = m.from;
    parent[m.to] = m.p;
    parent[m.from] = m.p;
    atomicAdd(moved, 1u);
}

// Boxes of the inner nodes, level by level from the deepest: box = left's grown by right's.  The value does not depend on
// the order but the sign of a zero does (the first operand's), so Reinserter::run_whole_iterations puts every box into this
// form before the first iteration; refit_up then leaves these very bits on the host.
__global__ void __launch_bounds__(kBlock) k_refit(Node2 *nodes, const uint32_t *list, uint32_t n) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = list[t];
    const Node2 nd = load_node(nodes, i);
    if (nd.count == 1) return;
    Aabb b = load_node(nodes, nd.left).box;
    grow(b, load_node(nodes, nd.right).box);
    nodes[i].box = b;
}

} // namespace

struct ReinsertDevice {
    int device = -1;
    size_t n_nodes = 0;
    int grid = 0;
    DevBuf<Node2> nodes;
    DevBuf<uint32_t> parent, cand, found;
    DevBuf<uint2> stacks;
    // allocated by the first iteration
    DevBuf<unsigned long long> keys_a, keys_b;
    DevBuf<unsigned char> sort_tmp;
    DevBuf<Six> six; // at most every node is a candidate
    DevBuf<uint8_t> status;
    DevBuf<uint32_t> claim, list, words; // words: undecided, flags, moved, level counter
    Event ev0, ev1;
};

void reinsert_dev_close(ReinsertDevice *c) {
    if (!c) return;
    DeviceScope scope; // the buffers go with their own device current
    std::string err;
    (void)scope.reenter(c->device, err);
    delete c;
}

bool reinsert_dev_open(int device, size_t n_nodes, ReinsertDevice **out, std::string &err) {
    DeviceScope scope;
    if (!scope.enter(device, err)) return false;
    std::unique_ptr<ReinsertDevice, void (*)(ReinsertDevice *)> c(new ReinsertDevice, reinsert_dev_close); // (nothing leaks on a failure)
    c->device = device;
    c->n_nodes = n_nodes;
    hipDeviceProp_t prop;
    TRX_BUILD_TRY(hipGetDeviceProperties(&prop, device));
    c->grid = std::max(1, prop.multiProcessorCount) * 4; // four 256-thread blocks per CU: ~260 k searches in flight
    const size_t n = std::max<size_t>(n_nodes, 1);
    TRX_BUILD_TRY(c->nodes.alloc(n));
    TRX_BUILD_TRY(c->parent.alloc(n));
    TRX_BUILD_TRY(c->cand.alloc(n));
    TRX_BUILD_TRY(c->found.alloc(n));
    TRX_BUILD_TRY(c->stacks.alloc((size_t)c->grid * kBlock * kStackCap));
    TRX_BUILD_TRY(c->ev0.create());
    TRX_BUILD_TRY(c->ev1.create());
    *out = c.release();
    return true;
}

bool reinsert_dev_upload(ReinsertDevice *c, const void *nodes, const uint32_t *parent, std::string &err) {
    if (!c) {
        err = "reinsert_dev_upload: no context";
        return false;
    }
    DeviceScope scope;
    if (!scope.reenter(c->device, err)) return false;
    TRX_BUILD_TRY(hipMemcpy(c->nodes.get(), nodes, c->n_nodes * sizeof(Node2), hipMemcpyHostToDevice));
    TRX_BUILD_TRY(hipMemcpy(c->parent.get(), parent, c->n_nodes * 4, hipMemcpyHostToDevice));
    return true;
}

bool reinsert_dev_download(ReinsertDevice *c, void *nodes, uint32_t *parent, std::string &err) {
    if (!c) {
        err = "reinsert_dev_download: no context";
        return false;
    }
    DeviceScope scope;
    if (!scope.reenter(c->device, err)) return false;
    TRX_BUILD_TRY(hipMemcpy(nodes, c->nodes.get(), c->n_nodes * sizeof(Node2), hipMemcpyDeviceToHost));
    TRX_BUILD_TRY(hipMemcpy(parent, c->parent.get(), c->n_nodes * 4, hipMemcpyDeviceToHost));
    return true;
}

bool reinsert_dev_iteration_resident(ReinsertDevice *c, uint32_t take, uint32_t *ids, uint32_t *found, uint32_t *moved, bool *to_host,
                                     double *seconds, std::string &err, bool force_host, uint32_t *rounds_out) {
    if (!c || take > c->n_nodes || c->n_nodes > 0x7fffffffull || !moved || !to_host) {
        err = "reinsert_dev_iteration_resident: bad arguments";
        return false;
    }
    *moved = 0;
    *to_host = false;
    if (take == 0) return true;
    DeviceScope scope;
    if (!scope.reenter(c->device, err)) return false;
    const uint32_t n = (uint32_t)c->n_nodes;
    if (!c->keys_a) {
        TRX_BUILD_TRY(c->keys_a.alloc(n));
        TRX_BUILD_TRY(c->keys_b.alloc(n));
        size_t bytes = 0;
        TRX_BUILD_TRY(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, bytes, c->keys_a.get(), c->keys_b.get(), (int)n, 0, 64, (hipStream_t) nullptr));
        TRX_BUILD_TRY(c->sort_tmp.alloc(std::max<size_t>(bytes, 16))); // (never 0: a null buffer asks hipcub for the size)
    }
    if (!c->six) {
        TRX_BUILD_TRY(c->six.alloc(n));
        TRX_BUILD_TRY(c->status.alloc(n));
        TRX_BUILD_TRY(c->claim.alloc(n));
        TRX_BUILD_TRY(c->list.alloc(n));
        TRX_BUILD_TRY(c->words.alloc(16));
        TRX_BUILD_TRY(hipMemset(c->claim.get(), 0xff, (size_t)n * 4)); // nobody claims anything; kept that way between iterations
    }
    Six *const six = c->six.get();
    TRX_BUILD_TRY(hipEventRecord(c->ev0.get(), nullptr));
    // candidates and their places, as reinsert_dev_iteration finds them - on the tree that is already here
    hipLaunchKernelGGL(k_keys, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, c->nodes.get(), c->parent.get(), n, c->keys_a.get());
    TRX_BUILD_TRY(hipGetLastError());
    size_t bytes = c->sort_tmp.count();
    TRX_BUILD_TRY(hipcub::DeviceRadixSort::SortKeysDescending(c->sort_tmp.get(), bytes, c->keys_a.get(), c->keys_b.get(), (int)n, 0, 64, (hipStream_t) nullptr));
    const dim3 over_take((take + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_ids, over_take, dim3(kBlock), 0, nullptr, c->keys_b.get(), take, c->cand.get());
    const int blocks = (int)std::min<size_t>((size_t)c->grid, ((size_t)take + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_find, dim3(blocks), dim3(kBlock), 0, nullptr, c->nodes.get(), c->parent.get(), c->cand.get(), take, c->found.get(), c->stacks.get());
    TRX_BUILD_TRY(hipGetLastError());
    // a search that outgrew its stack is repeated on the host: the whole iteration goes there
    hipLaunchKernelGGL(k_six, over_take, dim3(kBlock), 0, nullptr, c->nodes.get(), c->parent.get(), c->cand.get(), c->found.get(), take, six, c->status.get());
    TRX_BUILD_TRY(hipGetLastError());
    uint32_t words[4] = {0, 0, 0, 0}; // undecided, flags, moved, level counter
    bool host = force_host;
    {
        // (an overflowed search: found == kReinsertOverflow somewhere; counted with a tiny reduction over found on the host
        // side would need the array - the flag kernel below does it in place)
        TRX_BUILD_TRY(hipMemset(c->words.get(), 0, 16));
    }
    // independent set in candidate order
    int rounds = 0;
    for (; !host; rounds++) {
        if (rounds > 512) { // (a dependency chain this long is not a tree anyone built; the host decides)
            host = true;
            break;
        }
        TRX_BUILD_TRY(hipMemsetAsync(c->words.get(), 0, 4, nullptr));
        hipLaunchKernelGGL(k_claim, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->claim.get(), 1);
        hipLaunchKernelGGL(k_claim, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->claim.get(), 0);
        hipLaunchKernelGGL(k_decide, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->claim.get(), c->words.get());
        TRX_BUILD_TRY(hipGetLastError());
        TRX_BUILD_TRY(hipMemcpy(words, c->words.get(), 4, hipMemcpyDeviceToHost));
        if (words[0] == 0) break;
    }
    if (!host) {
        // claims of the accepted moves only, then the rule the independent set does not know
        hipLaunchKernelGGL(k_claim, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->claim.get(), 1);
        hipLaunchKernelGGL(k_claim, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->claim.get(), 0);
        hipLaunchKernelGGL(k_verify, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->parent.get(), c->claim.get(), c->words.get() + 1);
        hipLaunchKernelGGL(k_overflowed, over_take, dim3(kBlock), 0, nullptr, c->found.get(), take, c->words.get() + 1);
        TRX_BUILD_TRY(hipGetLastError());
        TRX_BUILD_TRY(hipMemcpy(words, c->words.get(), 16, hipMemcpyDeviceToHost));
        host = words[1] != 0;
    }
    if (rounds_out) *rounds_out = (uint32_t)rounds;
    // (free the claims again whatever happens next)
    hipLaunchKernelGGL(k_claim, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->claim.get(), 1);
    TRX_BUILD_TRY(hipGetLastError());
    if (host) {
        *to_host = true;
        TRX_BUILD_TRY(hipEventRecord(c->ev1.get(), nullptr));
        TRX_BUILD_TRY(hipMemcpy(ids, c->cand.get(), (size_t)take * 4, hipMemcpyDeviceToHost));
        TRX_BUILD_TRY(hipMemcpy(found, c->found.get(), (size_t)take * 4, hipMemcpyDeviceToHost));
    } else {
        hipLaunchKernelGGL(k_apply, over_take, dim3(kBlock), 0, nullptr, six, c->status.get(), take, c->nodes.get(), c->parent.get(), c->words.get() + 2);
        TRX_BUILD_TRY(hipGetLastError());
        // boxes: levels top-down (kept as lists), then refit bottom-up
        std::vector<uint32_t> level;
        if (!expand_levels("reinsert_dev_iteration_resident", c->nodes.get(), n, c->list.get(), c->words.get() + 3, level, err)) return false;
        for (size_t L = level.size() - 1; L-- > 0;)
            hipLaunchKernelGGL(k_refit, dim3((level[L + 1] - level[L] + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, c->nodes.get(),
                               c->list.get() + level[L], level[L + 1] - level[L]);
        TRX_BUILD_TRY(hipGetLastError());
        TRX_BUILD_TRY(hipEventRecord(c->ev1.get(), nullptr));
        TRX_BUILD_TRY(hipMemcpy(words, c->words.get(), 16, hipMemcpyDeviceToHost));
        *moved = words[2];
    }
    if (seconds) {
        float ms = 0.f;
        TRX_BUILD_TRY(hipEventSynchronize(c->ev1.get()));
        TRX_BUILD_TRY(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()));
        *seconds += ms * 1e-3;
    }
    return true;
}

} // namespace trx
