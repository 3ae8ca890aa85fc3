// The frontier walker: the chunked expansion over the suffixes that occur (frontier.hpp has its leaves), with what happens to the
// children of the last level -- the SINK -- left to the caller.  The k-mer spectrum and dumps (spectrum.hip), the canonical staging
// walk (canonical.hip through spectrum_stage) and both passes of the sparse-table builder (sparse_table.hip) are this walk.
//
// A node is a suffix that occurs: {key, l, h}.  The seeds are the root [0, total), the non-empty entries of a flat direct table, or
// (in a descent) the nodes of a stack level; a pair step takes every node two symbols further from one or two pair-block lines (16
// children), a plane step one symbol further from its plane-block lines (4 children; the odd last level, and every level without a
// pair index); on run blocks an 8-lane group ranks the four symbols with constrain_any, as extend.hip does: correct, not tuned.
// Children narrower than the prune width are dropped at every level; the others go to the next frontier, in whatever order the blocks
// finish, with one atomic per workgroup.  The LAST level is not materialised: its children go to the sink (unless the walk stages
// them: then the last level is a frontier like the others and a hook gets every chunk's).
// The seeds are worked through in chunks that keep the frontiers inside a fixed scratch allocation: a chunk that overflows a frontier
// is taken again at half the size -- the sink has seen nothing of it, the last level runs only behind levels that all fitted -- and
// the next chunk is sized by the widest frontier of the last.  A SINGLE seed whose subtree does not fit is expanded one step into a
// small stack buffer and its children become the seeds of a walk one level down (at most 16 nodes per stack level, at most k levels).
//
// A sink is a small struct passed to the kernels by value (PlainSink has the defaults; a sink hides what it changes).  It says
//     keeps(width)         which children of the last level it takes
//     begin / end          what a workgroup does before its first and after its last node (S::kLdsWords words of LDS are its own;
//                          S::Thread is what a thread carries from node to node)
//     place(mine, cur)     called by every thread of the block with the number of children it keeps: a slot for them, if the sink has slots
//     take(...)            one kept child of the last level
//     see / tally          what it observes about the children of EVERY level, kept or not: see() per child into an S::Seen, tally()
//                          by every thread of the block into the kWalkTallies per-depth counters of the chunk in hand
// The sink is a template parameter, so a user's kernels hold its own sink's code and nothing of the others'.
// Include from HIP translation units only.  Integer work bound by random 128-byte lines: no MFMA.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "frontier.hpp"
#include "kernels.hpp"
#include "rank_ops.hpp"

namespace msbwt {
namespace {

constexpr uint32_t kWalkMaxDepth = 32;      // a key is one 2-bit word
constexpr uint64_t kWalkMinFrontier = 64;   // fewest nodes a frontier buffer may hold (a node's 16 children must fit four times over)
constexpr int kWalkTallies = 2;
// cursor block (u64 words) at the start of the scratch; depths 0..32
constexpr int kWalkCur = 0;        // [0 .. 33): nodes appended to the frontier of depth d by the chunk in hand ([k]: taken by the sink)
constexpr int kWalkTally = 40;     // [40 + 40 j + d], j < kWalkTallies: what the sink tallied about the children at depth d, chunk in hand
constexpr int kWalkTallyStride = 40;
constexpr int kWalkOverflow = 120; // a frontier of the chunk in hand was too small
constexpr int kWalkChunkWords = 121;  // (what reset_chunk zeroes)
constexpr int kWalkSink = 128;     // [128 .. 136): the sink's own words, kept from chunk to chunk
constexpr int kWalkSinkWords = 8;
constexpr int kWalkCursorWords = kWalkSink + kWalkSinkWords;
constexpr size_t kWalkHeadBytes = 32768;  // cursors, then the re-seeding stack
constexpr size_t kWalkStackOffset = 4096;
constexpr uint32_t kWalkStackNodes = 16;  // per stack level: the children of one node
static_assert(kWalkCursorWords * sizeof(unsigned long long) <= kWalkStackOffset, "the cursors end before the stack");
static_assert(kWalkStackOffset + (kWalkMaxDepth + 1) * kWalkStackNodes * sizeof(Node) <= kWalkHeadBytes, "the stack fits the head");
static_assert(kWalkMinFrontier >= kWalkStackNodes, "a single node's children always fit a frontier");

constexpr int kStepPair = 0, kStepPlane = 1, kStepRuns = 2;

struct WalkIndex {  // the index, and what the levels before the last keep
    const uint4 *blocks, *overflow, *pair_blocks;
    const uint64_t *pair_super;
    uint32_t s96;
    uint64_t prune;  // >= 1: children narrower than this are dropped
};

// the sink that takes every non-empty child, does nothing with it and observes nothing
struct PlainSink {
    static constexpr uint32_t kLdsWords = 0;
    struct Thread {};
    struct Seen {};
    __device__ __forceinline__ bool keeps(uint64_t width) const { return width != 0u; }
    __device__ __forceinline__ void begin(uint32_t *) const {}
    __device__ __forceinline__ void end(Thread &, uint32_t *, unsigned long long *) const {}
    __device__ __forceinline__ uint64_t place(uint32_t, unsigned long long *) const { return 0; }
    __device__ __forceinline__ void take(Thread &, uint32_t *, unsigned long long *, uint64_t, uint64_t, uint64_t, uint64_t &) const {}
    __device__ __forceinline__ void see(Seen &, uint64_t, uint32_t) const {}
    __device__ __forceinline__ void tally(const Seen &, unsigned long long *) const {}
};

// ---- seeds [i0, i0 + np): of `nodes` (a stack level), of the flat table, or the root ------------------------------------------
__global__ __launch_bounds__(kFrontierThreads) void k_frontier_seed(const uint4 *__restrict__ flat, const Node *__restrict__ nodes, uint64_t i0, uint64_t np,
                                                                    uint64_t total, uint64_t prune, Node *__restrict__ out, uint64_t cap,
                                                                    unsigned long long *__restrict__ cur, uint32_t depth) {
    for (uint64_t base = uint64_t(blockIdx.x) * kFrontierThreads; base < np; base += uint64_t(gridDim.x) * kFrontierThreads) {
        const uint64_t i = base + threadIdx.x;
        Node nd{0, 0, 0};
        bool keep = false;
        if (i < np) {
            nd = nodes ? nodes[i0 + i] : seed_node(flat, i0 + i, total);
            keep = nd.h - nd.l >= prune && nd.h > nd.l;
        }
        const uint64_t at = reserve(keep ? 1u : 0u, cur + kWalkCur + depth);
        if (keep) {
            if (at < cap) out[at] = nd;
            else atomicOr(cur + kWalkOverflow, 1ull);
        }
    }
}

// ---- one step: every node of `in` -> its children; kFinal = false: appended to `out`, true: handed to the sink -----------------
template <int kStep, bool kFinal, class S>
__global__ __launch_bounds__(kFrontierThreads) void k_frontier_expand(const Node *__restrict__ in, uint64_t in_cap, uint32_t depth, WalkIndex env, Node *__restrict__ out,
                                                                      uint64_t cap, unsigned long long *__restrict__ cur, S sink) {
    constexpr bool kPair = kStep == kStepPair;
    constexpr uint32_t kKids = kPair ? 16u : 4u, kAdv = kPair ? 2u : 1u;
    constexpr uint32_t kLanes = kStep == kStepRuns ? uint32_t(kGroup) : 1u;  // lanes that work on one node
    constexpr uint32_t kPer = uint32_t(kFrontierThreads) / kLanes;
    __shared__ uint32_t lds[kFinal && S::kLdsWords != 0u ? S::kLdsWords : 1u];
    // An earlier level of this chunk overflowed its frontier: the slots of the thread whose reservation straddled the end were never
    // written, so this level must not read them (raw allocation contents would become wild line addresses), and the host takes the
    // whole chunk again -- nothing of it may reach a frontier or the sink.
    if (cur[kWalkOverflow] != 0ull) return;
    typename S::Thread carried{};
    if (kFinal) sink.begin(lds);
    const uint64_t n = min(uint64_t(cur[kWalkCur + depth]), in_cap);
    for (uint64_t base = uint64_t(blockIdx.x) * kPer; base < n; base += uint64_t(gridDim.x) * kPer) {
        const uint64_t i = base + threadIdx.x / kLanes;
        const bool owner = i < n && threadIdx.x % kLanes == 0u;  // the lane that emits the node's children
        Node nd{0, 0, 0};
        PairStep st;
        uint64_t nl[4] = {0, 0, 0, 0}, nh[4] = {0, 0, 0, 0};
        if (i < n) {
            nd = in[i];
            if constexpr (kPair) {
                pair_step_lines(nd, env.pair_blocks, env.s96 != 0u, st);
            } else if constexpr (kStep == kStepPlane) {
                plane_step(nd, env.blocks, nl, nh);
            } else {  // (the same branch in all 8 lanes of a group)
#pragma unroll 1
                for (uint32_t q = 0; q < 4u; ++q) {
                    const Range r = constrain_any(1u, env.blocks, env.overflow, q == 3u ? 5u : q + 1u, nd.l, nd.h, threadIdx.x & uint32_t(kGroup - 1));
                    nl[q] = r.l;
                    nh[q] = r.h;
                }
            }
        }
        auto range_of = [&](uint32_t p, uint64_t &a, uint64_t &b) {
            if constexpr (kPair) {
                pair_child(env.pair_super, st, p, a, b);
            } else {
                a = nl[p];
                b = nh[p];
            }
        };
        uint32_t mask = 0;
        typename S::Seen seen{};
        if (owner) {
            const bool cheap = kPair && st.same_super();  // widths without a 64-bit operation
#pragma unroll
            for (uint32_t p = 0; p < kKids; ++p) {
                uint64_t width;
                if (cheap) {
                    width = uint64_t(st.H.rel[p] - st.L.rel[p]);
                } else {
                    uint64_t a, b;
                    range_of(p, a, b);
                    width = b - a;
                }
                const bool keep = kFinal ? sink.keeps(width) : width >= env.prune;
                mask |= (keep ? 1u : 0u) << p;
                sink.see(seen, width, p);
            }
        }
        sink.tally(seen, cur + kWalkTally + depth + kAdv);
        const uint32_t mine = uint32_t(__popc(mask));
        uint64_t at = 0;
        if (!kFinal) {
            at = reserve(mine, cur + kWalkCur + depth + kAdv);
            if (mine != 0u && at + mine > cap) {
                atomicOr(cur + kWalkOverflow, 1ull);
                mask = 0;
            }
        } else {
            block_add(mine, cur + kWalkCur + depth + kAdv);
            at = sink.place(mine, cur);
        }
#pragma unroll
        for (uint32_t p = 0; p < kKids; ++p) {
            if (((mask >> p) & 1u) == 0u) continue;
            uint64_t a, b;
            range_of(p, a, b);
            const uint64_t key = kPair ? pair_child_key(nd.key, depth, p) : plane_child_key(nd.key, depth, p);
            if (!kFinal) out[at++] = Node{key, a, b};
            else sink.take(carried, lds, cur, key, a, b, at);
        }
    }
    if (kFinal) sink.end(carried, lds, cur);
}

// ---- sizes (pure) ----
// nodes per frontier buffer: `wanted`, or automatic -- 2^27 when HBM is plentiful, what an eighth of the free bytes holds otherwise,
// 2^16 at least, and never more than the index can fill (a level's nodes are disjoint non-empty ranges, at most `total` of them: a
// toy index must not pay for a 6 GB allocation per walk)
inline uint64_t walk_frontier_nodes(uint64_t total, uint64_t free_bytes, uint64_t wanted) {
    if (wanted) return std::max(wanted, kWalkMinFrontier);
    const uint64_t by_memory = std::max<uint64_t>(uint64_t(1) << 16, std::min<uint64_t>(uint64_t(1) << 27, free_bytes / 8 / (2 * sizeof(Node))));
    return std::min(by_memory, std::max<uint64_t>(total + 1024, 4096));
}
inline uint64_t walk_work_bytes(uint64_t frontier_nodes) { return kWalkHeadBytes + 2 * frontier_nodes * sizeof(Node); }  // cursors, the stack, two frontiers
inline uint64_t walk_nodes_in(uint64_t work_bytes) { return work_bytes > kWalkHeadBytes ? (work_bytes - kWalkHeadBytes) / (2 * sizeof(Node)) : 0; }

// what a walk did
struct WalkRecord {
    uint64_t chunks = 0;    // chunks of seeds that went through every level
    uint64_t retries = 0;   // chunks taken again at half the size after a frontier overflowed
    uint64_t descents = 0;  // single seeds whose subtree did not fit: expanded one step and re-seeded from their children
    uint64_t nodes[kWalkMaxDepth + 1] = {};                // nodes at depth d that survived the pruning; [k]: the children the sink kept
    uint64_t tally[kWalkTallies][kWalkMaxDepth + 1] = {};  // what the sink tallied at depth d
};

// Staging: per_chunk(d_nodes, m) gets the m >= 1 nodes of a chunk's last level in a frontier buffer that the next chunk overwrites
// (after the synchronisation that reads the chunk's cursors); what it returns other than hipSuccess ends the walk.
using WalkChunkHook = std::function<hipError_t(const void *d_nodes, uint64_t m)>;

// kRunBlocks = false: a walk over plane blocks only (no run-block kernels are made for it)
template <class S, bool kRunBlocks = true>
class Walker {
  public:
    // flat: the flat direct table the walk starts from (flat_depth < k symbols), nullptr: from the root
    Walker(const IndexView &ix, const void *flat, int flat_depth, uint32_t k, uint64_t prune, const S &sink, void *d_work, uint64_t frontier_nodes, hipStream_t stream,
           const WalkChunkHook *stage = nullptr)
        : ix_(ix), flat_(static_cast<const uint4 *>(flat)), seed_depth_(uint32_t(flat_depth)), k_(k), sink_(sink), cap_(frontier_nodes), stream_(stream), hook_(stage),
          cur_(kWalkCursorWords, 0ull) {
        env_ = WalkIndex{static_cast<const uint4 *>(ix.blocks), static_cast<const uint4 *>(ix.overflow), static_cast<const uint4 *>(ix.pair_blocks), ix.pair_super,
                         ix.pair_stride96 ? 1u : 0u, std::max<uint64_t>(prune, 1)};
        if (flat_ == nullptr || flat_depth <= 0 || uint32_t(flat_depth) >= k) {
            flat_ = nullptr;
            seed_depth_ = 0;
        }
        char *base = static_cast<char *>(d_work);
        dcur_ = reinterpret_cast<unsigned long long *>(base);
        stack_ = reinterpret_cast<Node *>(base + kWalkStackOffset);
        a_ = reinterpret_cast<Node *>(base + kWalkHeadBytes);
        b_ = a_ + cap_;
    }

    // Synchronises the stream chunk by chunk: the host steers.
    hipError_t run() {
        rec_ = WalkRecord{};
        if (k_ < 1 || k_ > kWalkMaxDepth || cap_ < kWalkMinFrontier) return hipErrorInvalidValue;
        if (ix_.total == 0) return hipSuccess;
        if (ix_.blocks == nullptr || (!kRunBlocks && ix_.block_format == kBlocksRuns)) return hipErrorInvalidValue;
        hipError_t e = hipMemsetAsync(dcur_, 0, kWalkCursorWords * sizeof(unsigned long long), stream_);
        if (e != hipSuccess) return e;
        const uint64_t parents = flat_ ? (uint64_t(1) << (2 * seed_depth_)) : 1;
        return walk(flat_, nullptr, parents, seed_depth_, 0);
    }
    const WalkRecord &record() const { return rec_; }
    uint32_t seed_depth() const { return seed_depth_; }
    uint64_t cursor(int word) const { return cur_[word]; }  // as the last chunk left it: for the sink's words

  private:
    int step_at(uint32_t depth) const {
        if (ix_.block_format == kBlocksRuns) return kStepRuns;
        return (ix_.pair_blocks && ix_.pair_super && k_ - depth >= 2u) ? kStepPair : kStepPlane;
    }
    static uint32_t advance(int step) { return step == kStepPair ? 2u : 1u; }
    static uint32_t grid_for_nodes(uint64_t n, uint32_t lanes) {
        const uint64_t blocks = (n * lanes + kFrontierThreads - 1) / kFrontierThreads;
        return uint32_t(std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 256ull * 8));
    }

    // (every level is launched for the most nodes its input can hold: the kernels read the true count from the cursor)
    template <bool kFinal>
    void expand(int step, const Node *in, uint64_t in_cap, uint32_t depth, Node *out, uint64_t cap) {
        const uint32_t grid = grid_for_nodes(in_cap, step == kStepRuns ? uint32_t(kGroup) : 1u);
        if (step == kStepPair)
            hipLaunchKernelGGL((k_frontier_expand<kStepPair, kFinal, S>), dim3(grid), dim3(kFrontierThreads), 0, stream_, in, in_cap, depth, env_, out, cap, dcur_, sink_);
        else if (step == kStepPlane)
            hipLaunchKernelGGL((k_frontier_expand<kStepPlane, kFinal, S>), dim3(grid), dim3(kFrontierThreads), 0, stream_, in, in_cap, depth, env_, out, cap, dcur_, sink_);
        else if constexpr (kRunBlocks)
            hipLaunchKernelGGL((k_frontier_expand<kStepRuns, kFinal, S>), dim3(grid), dim3(kFrontierThreads), 0, stream_, in, in_cap, depth, env_, out, cap, dcur_, sink_);
    }

    void seed(const uint4 *flat, const Node *nodes, uint64_t i0, uint64_t np, uint32_t depth) {
        hipLaunchKernelGGL(k_frontier_seed, dim3(grid_for_nodes(np, 1)), dim3(kFrontierThreads), 0, stream_, flat, nodes, i0, np, ix_.total, env_.prune, a_, cap_, dcur_,
                           depth);
    }

    hipError_t read_cursors() {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(cur_.data(), dcur_, kWalkCursorWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        return e;
    }
    // the chunk's frontier counts, its tallies and its overflow mark start again from 0 (the sink's words stay)
    hipError_t reset_chunk() { return hipMemsetAsync(dcur_, 0, kWalkChunkWords * sizeof(unsigned long long), stream_); }

    // what the chunk in hand counted at depth d joins the record
    void record_depth(uint32_t d) {
        rec_.nodes[d] += cur_[kWalkCur + d];
        for (int j = 0; j < kWalkTallies; ++j) rec_.tally[j][d] += cur_[kWalkTally + kWalkTallyStride * j + d];
    }

    // seeds [i0, i0 + np) at `depth` through every level; the last one feeds the sink
    hipError_t run_chunk(const uint4 *flat, const Node *nodes, uint64_t i0, uint64_t np, uint32_t depth) {
        seed(flat, nodes, i0, np, depth);
        Node *in = a_, *out = b_;
        while (depth < k_) {
            const int step = step_at(depth);
            if (depth + advance(step) >= k_ && !staging()) expand<true>(step, in, cap_, depth, out, cap_);
            else expand<false>(step, in, cap_, depth, out, cap_);
            depth += advance(step);
            std::swap(in, out);
        }
        staged_ = in;  // (the frontier written last)
        return read_cursors();
    }

    hipError_t walk(const uint4 *flat, const Node *nodes, uint64_t n, uint32_t depth, uint32_t level) {
        // Chunks of seeds: the first is small, the following ones are sized by what the last one's widest frontier was, aiming at a
        // quarter of the buffer; a chunk that overflows is taken again at half the size (the sink has seen nothing of it).
        uint64_t np = std::min<uint64_t>(n, uint64_t(1) << 16);
        for (uint64_t i0 = 0; i0 < n;) {
            const uint64_t c = std::min(np, n - i0);
            hipError_t e = run_chunk(flat, nodes, i0, c, depth);
            if (e != hipSuccess) return e;
            if (cur_[kWalkOverflow] != 0) {
                if ((e = reset_chunk()) != hipSuccess) return e;
                if (c > 1) {
                    ++rec_.retries;
                    np = std::max<uint64_t>(1, c / 2);
                    continue;
                }
                // one seed's subtree does not fit: one step into the stack (never the last step: that one materialises nothing, or when
                // staging at most 16 nodes, and cannot overflow), and its children are the seeds of a walk one level down
                const int step = step_at(depth);
                const uint32_t below = depth + advance(step);
                if (below >= k_ || level + 1 > kWalkMaxDepth) return hipErrorOutOfMemory;
                Node *kids = stack_ + uint64_t(level + 1) * kWalkStackNodes;
                seed(flat, nodes, i0, 1, depth);
                expand<false>(step, a_, cap_, depth, kids, kWalkStackNodes);
                if ((e = read_cursors()) != hipSuccess) return e;
                if (cur_[kWalkOverflow] != 0) return hipErrorOutOfMemory;  // (16 children always fit)
                const uint64_t m = cur_[kWalkCur + below];
                record_depth(depth);
                for (int j = 0; j < kWalkTallies; ++j) rec_.tally[j][below] += cur_[kWalkTally + kWalkTallyStride * j + below];  // (the re-seeding counts the children, no more)
                ++rec_.descents;
                if ((e = reset_chunk()) != hipSuccess) return e;
                if (m != 0 && (e = walk(nullptr, kids, m, below, level + 1)) != hipSuccess) return e;
                i0 += 1;
                np = 1;
                continue;
            }
            ++rec_.chunks;
            unsigned long long widest = 1;
            for (uint32_t d = depth; d <= k_; ++d) {
                record_depth(d);
                if (d < k_ || staging()) widest = std::max(widest, cur_[kWalkCur + d]);  // (the last level is not materialised unless staged)
            }
            if (staging() && cur_[kWalkCur + k_] != 0 && (e = (*hook_)(staged_, cur_[kWalkCur + k_])) != hipSuccess) return e;
            if ((e = reset_chunk()) != hipSuccess) return e;
            i0 += c;
            const double per_seed = double(widest) / double(c);
            np = uint64_t(std::max(1.0, std::min(double(uint64_t(1) << 26), double(cap_) / 4.0 / std::max(per_seed, 1e-6))));
        }
        return hipSuccess;
    }

    bool staging() const { return hook_ != nullptr; }

    const IndexView &ix_;
    const uint4 *flat_;
    uint32_t seed_depth_, k_;
    WalkIndex env_;
    S sink_;
    unsigned long long *dcur_;  // the cursor block
    Node *stack_, *a_, *b_;
    uint64_t cap_;              // nodes a frontier holds
    hipStream_t stream_;
    const WalkChunkHook *hook_;  // staging: what takes a chunk's last level
    const Node *staged_ = nullptr;
    WalkRecord rec_;
    std::vector<unsigned long long> cur_;
};

}  // namespace
}  // namespace msbwt
