// gfx950: the k-mers an index holds -- abundance spectrum and k-mer dump (spectrum.hpp) -- by the frontier expansion the sparse-table
// builder uses (frontier.hpp, sparse_table.hip), run to depth k.
//
// A node is a suffix that occurs: {key, l, h}, key = its packed 2-bit word.  The seeds are the root [0, total) or the non-empty entries of
// the flat direct table; a pair step takes every node two symbols further from one or two pair-block lines (16 children), a plane step
// one symbol further from its plane-block lines (4 children; the odd last level, and every level without a pair index); on run blocks
// an 8-lane group ranks the four symbols with constrain_any, as extend.hip does: correct, not tuned.  Children go to the next frontier
// with one atomic per workgroup.  The LAST level is not materialised: its children go to the sink --
//     histogram   width h - l -> a bin; bins below kLdsBins in an LDS histogram flushed once per workgroup, wider ones by global atomics
//     count/mark  how many k-mers lie in the count window; for a sorted dump the bit of each one's l in a bitmap over the rows
//     append      the records, wherever the workgroup's reservation puts them
//     scatter     the records, each at rank(l) of the bitmap: ranges of distinct k-mers are disjoint and in lexicographic order, so
//                 the number of marked rows below l IS the record's place in ascending k-mer order -- no sort
//     stage       (the canonical calls, canonical.hip) the last level IS materialised, by the step that fills every other frontier, and
//                 the chunk's k-mers {word, l, h} are handed to the caller's hook before the next chunk overwrites them; a last
//                 frontier that overflows is a frontier that overflows
// A count window [m, ..] prunes: a k-mer never occurs more often than any of its suffixes, so a node narrower than m is dropped at
// every level (the spectrum itself does not prune).
// The seeds are worked through in chunks that keep the frontiers inside a fixed scratch allocation, as in the builder: a chunk that
// overflows a frontier is taken again at half the size -- the sink has seen nothing of it, the last level runs only behind levels
// that all fitted -- and the next chunk is sized by the widest frontier of the last.  A SINGLE seed whose subtree does not fit is
// expanded one step into a small stack buffer and its children become the seeds of a walk one level down (at most 16 nodes per stack
// level, at most k levels).  Integer work bound by random 128-byte lines: no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "frontier.hpp"
#include "rank_ops.hpp"
#include "run_encode.hpp"
#include "spectrum.hpp"

namespace msbwt {
namespace {

constexpr int kThreads = kFrontierThreads;
// cursor block (u64 words) at the start of the scratch; depths 0..32
constexpr int kCur = 0;        // [0 .. 33): nodes appended to the frontier of depth d by the chunk in hand ([k]: taken by the sink)
constexpr int kOverflow = 40;  // a frontier of the chunk in hand was too small
constexpr int kOut = 41;       // append sink: records written so far
constexpr int kOccur = 42;     // histogram sink: sum of the widths
constexpr int kCursorWords = 64;
constexpr size_t kHeadBytes = 32768;                   // cursors, then the re-seeding stack
constexpr size_t kStackOffset = 4096;
constexpr uint32_t kStackNodes = 16;                   // per stack level: the children of one node
static_assert(kStackOffset + (kSpectrumMaxK + 1) * kStackNodes * sizeof(Node) <= kHeadBytes, "the stack fits the head");
static_assert(kSpectrumMinFrontier >= kStackNodes, "a single node's children always fit a frontier");

constexpr uint32_t kLdsBins = 2048;  // counts below this are tallied in LDS (8 KB): almost all of a read set's mass
constexpr int kStepPair = 0, kStepPlane = 1, kStepRuns = 2;
constexpr int kSinkHist = 0, kSinkCount = 1, kSinkAppend = 2, kSinkScatter = 3, kSinkStage = 4;  // (kSinkStage: the host's alone, no kernel sees it)
constexpr uint32_t kRankWords = uint32_t(kSpectrumRankRows / 32);

struct Env {  // the index, and what the levels before the last keep
    const uint4 *blocks, *overflow, *pair_blocks;
    const uint64_t *pair_super;
    uint32_t s96;
    uint64_t prune;  // >= 1: children narrower than this are dropped
};

struct Sink {
    int mode;
    uint64_t min, max;             // the count window (max: all-ones = none)
    unsigned long long *hist;      // kSinkHist
    uint64_t n_bins;
    uint32_t *bitmap;              // kSinkCount (optional), kSinkScatter
    const uint64_t *prefix;        // kSinkScatter: marked rows before every kSpectrumRankRows rows
    uint64_t *kmers, *counts, *l;  // the dumps (counts, l optional)
    uint64_t capacity;
    uint32_t *flags;
};

__device__ __forceinline__ void block_add64(uint64_t mine, unsigned long long *acc) {  // one atomic per wave
    const unsigned long long s = wave_sum<unsigned long long>(mine);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(acc, s);
}

// ---- seeds [i0, i0 + np): of `nodes` (a stack level), of the flat table, or the root ------------------------------------------
__global__ __launch_bounds__(kThreads) void k_spectrum_seed(const uint4 *__restrict__ flat, const Node *__restrict__ nodes, uint64_t i0, uint64_t np, uint64_t total,
                                                            uint64_t prune, Node *__restrict__ out, uint64_t cap, unsigned long long *__restrict__ cur, uint32_t depth) {
    for (uint64_t base = uint64_t(blockIdx.x) * kThreads; base < np; base += uint64_t(gridDim.x) * kThreads) {
        const uint64_t i = base + threadIdx.x;
        Node nd{0, 0, 0};
        bool keep = false;
        if (i < np) {
            nd = nodes ? nodes[i0 + i] : seed_node(flat, i0 + i, total);
            keep = nd.h - nd.l >= prune && nd.h > nd.l;
        }
        const uint64_t at = reserve(keep ? 1u : 0u, cur + kCur + depth);
        if (keep) {
            if (at < cap) out[at] = nd;
            else atomicOr(cur + kOverflow, 1ull);
        }
    }
}

// ---- one step: every node of `in` -> its children; kFinal = false: appended to `out`, true: handed to the sink -----------------
template <int kStep, bool kFinal>
__global__ __launch_bounds__(kThreads) void k_spectrum_expand(const Node *__restrict__ in, uint64_t in_cap, uint32_t depth, Env env, Node *__restrict__ out, uint64_t cap,
                                                              unsigned long long *__restrict__ cur, Sink sink) {
    constexpr bool kPair = kStep == kStepPair;
    constexpr uint32_t kKids = kPair ? 16u : 4u, kAdv = kPair ? 2u : 1u;
    constexpr uint32_t kLanes = kStep == kStepRuns ? uint32_t(kGroup) : 1u;  // lanes that work on one node
    constexpr uint32_t kPer = uint32_t(kThreads) / kLanes;
    __shared__ uint32_t lds_hist[kFinal ? kLdsBins : 1u];
    // An earlier level of this chunk overflowed its frontier: its last slots were never written, and the host takes the whole chunk
    // again -- nothing of it may reach a frontier or the sink (as in k_sparse_expand_pair).
    if (cur[kOverflow] != 0ull) return;
    const bool hist = kFinal && sink.mode == kSinkHist;
    if (hist) {
        for (uint32_t b = threadIdx.x; b < kLdsBins; b += kThreads) lds_hist[b] = 0u;
        __syncthreads();
    }
    const uint64_t n = min(uint64_t(cur[kCur + depth]), in_cap);
    uint64_t occurrences = 0;
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
                const bool keep = kFinal ? (width >= sink.min && width <= sink.max) : width >= env.prune;
                mask |= (keep ? 1u : 0u) << p;
            }
        }
        const uint32_t mine = uint32_t(__popc(mask));
        uint64_t at = 0;
        if (!kFinal) {
            at = reserve(mine, cur + kCur + depth + kAdv);
            if (mine != 0u && at + mine > cap) {
                atomicOr(cur + kOverflow, 1ull);
                mask = 0;
            }
        } else {
            block_add(mine, cur + kCur + depth + kAdv);
            if (sink.mode == kSinkAppend) at = reserve(mine, cur + kOut);
        }
#pragma unroll
        for (uint32_t p = 0; p < kKids; ++p) {
            if (((mask >> p) & 1u) == 0u) continue;
            uint64_t a, b;
            range_of(p, a, b);
            const uint64_t key = kPair ? pair_child_key(nd.key, depth, p) : plane_child_key(nd.key, depth, p);
            if (!kFinal) {
                out[at++] = Node{key, a, b};
                continue;
            }
            const uint64_t width = b - a;
            if (sink.mode == kSinkHist) {
                const uint64_t bin = min(width, sink.n_bins - 1u);
                if (bin < kLdsBins) atomicAdd(&lds_hist[bin], 1u);
                else atomicAdd(sink.hist + bin, 1ull);
                occurrences += width;
            } else if (sink.mode == kSinkCount) {
                if (sink.bitmap) atomicOr(sink.bitmap + (a >> 5), 1u << (uint32_t(a) & 31u));
            } else {
                uint64_t place = at++;
                if (sink.mode == kSinkScatter) {  // marked rows below a: the checkpoint, whole words of the block, the word's low bits
                    const uint64_t word = a >> 5, first = (a / kSpectrumRankRows) * kRankWords;
                    place = sink.prefix[a / kSpectrumRankRows];
                    for (uint64_t j = first; j < word; ++j) place += uint32_t(__popc(sink.bitmap[j]));
                    place += uint32_t(__popc(sink.bitmap[word] & low_bits(int(uint32_t(a) & 31u))));
                }
                if (place < sink.capacity) {
                    sink.kmers[place] = key;
                    if (sink.counts) sink.counts[place] = width;
                    if (sink.l) sink.l[place] = a;
                } else {
                    atomicOr(sink.flags, kFlagInternal);
                }
            }
        }
    }
    if (hist) {
        __syncthreads();
        const uint32_t bins = uint32_t(min(uint64_t(kLdsBins), sink.n_bins));
        for (uint32_t b = threadIdx.x; b < bins; b += kThreads) {
            const uint32_t c = lds_hist[b];
            if (c) atomicAdd(sink.hist + b, (unsigned long long)c);
        }
        block_add64(occurrences, cur + kOccur);
    }
}

// checkpoint b = marked rows in block b of the bitmap (scanned afterwards)
__global__ __launch_bounds__(256) void k_spectrum_block_marks(const uint32_t *__restrict__ bitmap, uint64_t nblocks, uint64_t *__restrict__ prefix) {
    for (uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; b < nblocks; b += uint64_t(gridDim.x) * blockDim.x) {
        const uint4 *w = reinterpret_cast<const uint4 *>(bitmap + b * kRankWords);
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRankWords / 4u; ++j) {
            const uint4 v = w[j];
            c += uint32_t(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
        }
        prefix[b] = c;
    }
}

uint32_t grid_for_nodes(uint64_t n, uint32_t lanes) {
    const uint64_t blocks = (n * lanes + kThreads - 1) / kThreads;
    return uint32_t(std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 256ull * 8));
}

uint64_t rank_blocks(uint64_t total) { return total / kSpectrumRankRows + 1; }

struct Work {
    unsigned long long *cur;
    Node *stack, *a, *b;
    uint64_t cap;
};

Work carve(void *d_work, uint64_t frontier_nodes) {
    Work w;
    char *base = static_cast<char *>(d_work);
    w.cur = reinterpret_cast<unsigned long long *>(base);
    w.stack = reinterpret_cast<Node *>(base + kStackOffset);
    w.cap = frontier_nodes;
    w.a = reinterpret_cast<Node *>(base + kHeadBytes);
    w.b = w.a + w.cap;
    return w;
}

struct RankView {  // the sorted dump's scratch: bitmap | checkpoints | scan scratch
    uint32_t *bitmap;
    uint64_t *prefix, *scan;
    uint64_t nblocks;
};

RankView rank_view(const void *d_rank, uint64_t total) {
    RankView r;
    r.nblocks = rank_blocks(total);
    char *base = static_cast<char *>(const_cast<void *>(d_rank));
    r.bitmap = reinterpret_cast<uint32_t *>(base);
    r.prefix = reinterpret_cast<uint64_t *>(base + r.nblocks * (kSpectrumRankRows / 8));
    r.scan = r.prefix + r.nblocks;
    return r;
}

class Walker {
  public:
    Walker(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t prune, const Sink &sink, void *d_work, uint64_t frontier_nodes, SpectrumInfo *info,
           hipStream_t stream, const SpectrumChunkHook *hook = nullptr)
        : ix_(ix), seeds_(seeds), k_(k), sink_(sink), w_(carve(d_work, frontier_nodes)), info_(info), stream_(stream), hook_(hook), cur_(kCursorWords, 0ull) {
        env_ = Env{static_cast<const uint4 *>(ix.blocks), static_cast<const uint4 *>(ix.overflow), static_cast<const uint4 *>(ix.pair_blocks), ix.pair_super,
                   ix.pair_stride96 ? 1u : 0u, std::max<uint64_t>(prune, 1)};
        if (seeds_.flat == nullptr || seeds_.flat_depth <= 0 || uint32_t(seeds_.flat_depth) >= k) seeds_ = SpectrumSeeds{};
    }

    hipError_t run() {
        *info_ = SpectrumInfo{};
        info_->k = k_;
        info_->seed_depth = uint64_t(seeds_.flat_depth);
        if (k_ < 1 || k_ > kSpectrumMaxK || w_.cap < kSpectrumMinFrontier) return hipErrorInvalidValue;
        if (ix_.total == 0) return hipSuccess;
        if (ix_.blocks == nullptr) return hipErrorInvalidValue;
        hipError_t e = hipMemsetAsync(w_.cur, 0, kCursorWords * sizeof(unsigned long long), stream_);
        if (e != hipSuccess) return e;
        const uint64_t parents = seeds_.flat ? (uint64_t(1) << (2 * seeds_.flat_depth)) : 1;
        return walk(static_cast<const uint4 *>(seeds_.flat), nullptr, parents, uint32_t(seeds_.flat_depth), 0);
    }
    uint64_t occurrences() const { return cur_[kOccur]; }

  private:
    int step_at(uint32_t depth) const {
        if (ix_.block_format == kBlocksRuns) return kStepRuns;
        return (ix_.pair_blocks && ix_.pair_super && k_ - depth >= 2u) ? kStepPair : kStepPlane;
    }
    static uint32_t advance(int step) { return step == kStepPair ? 2u : 1u; }

    template <bool kFinal>
    void expand(int step, const Node *in, uint64_t in_cap, uint32_t depth, Node *out, uint64_t cap) {
        const uint32_t grid = grid_for_nodes(in_cap, step == kStepRuns ? uint32_t(kGroup) : 1u);
        if (step == kStepPair)
            hipLaunchKernelGGL((k_spectrum_expand<kStepPair, kFinal>), dim3(grid), dim3(kThreads), 0, stream_, in, in_cap, depth, env_, out, cap, w_.cur, sink_);
        else if (step == kStepPlane)
            hipLaunchKernelGGL((k_spectrum_expand<kStepPlane, kFinal>), dim3(grid), dim3(kThreads), 0, stream_, in, in_cap, depth, env_, out, cap, w_.cur, sink_);
        else
            hipLaunchKernelGGL((k_spectrum_expand<kStepRuns, kFinal>), dim3(grid), dim3(kThreads), 0, stream_, in, in_cap, depth, env_, out, cap, w_.cur, sink_);
    }

    void seed(const uint4 *flat, const Node *nodes, uint64_t i0, uint64_t np, uint32_t depth) {
        hipLaunchKernelGGL(k_spectrum_seed, dim3(grid_for_nodes(np, 1)), dim3(kThreads), 0, stream_, flat, nodes, i0, np, ix_.total, env_.prune, w_.a, w_.cap, w_.cur,
                           depth);
    }

    hipError_t read_cursors() {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(cur_.data(), w_.cur, kCursorWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        return e;
    }
    // the chunk's frontier counts and its overflow mark start again from 0 (the sink's words stay)
    hipError_t reset_chunk() { return hipMemsetAsync(w_.cur, 0, (kOverflow + 1) * sizeof(unsigned long long), stream_); }

    // seeds [i0, i0 + np) at `depth` through every level; the last one feeds the sink
    hipError_t run_chunk(const uint4 *flat, const Node *nodes, uint64_t i0, uint64_t np, uint32_t depth) {
        seed(flat, nodes, i0, np, depth);
        Node *in = w_.a, *out = w_.b;
        while (depth < k_) {
            const int step = step_at(depth);
            if (depth + advance(step) >= k_ && !staging()) expand<true>(step, in, w_.cap, depth, out, w_.cap);
            else expand<false>(step, in, w_.cap, depth, out, w_.cap);
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
            if (cur_[kOverflow] != 0) {
                if ((e = reset_chunk()) != hipSuccess) return e;
                if (c > 1) {
                    ++info_->retries;
                    np = std::max<uint64_t>(1, c / 2);
                    continue;
                }
                // one seed's subtree does not fit: one step into the stack (never the last step: that one materialises nothing, or when
                // staging at most 16 nodes, and cannot overflow), and its children are the seeds of a walk one level down
                const int step = step_at(depth);
                if (depth + advance(step) >= k_ || level + 1 > kSpectrumMaxK) return hipErrorOutOfMemory;
                Node *kids = w_.stack + uint64_t(level + 1) * kStackNodes;
                seed(flat, nodes, i0, 1, depth);
                expand<false>(step, w_.a, w_.cap, depth, kids, kStackNodes);
                if ((e = read_cursors()) != hipSuccess) return e;
                if (cur_[kOverflow] != 0) return hipErrorOutOfMemory;  // (16 children always fit)
                const uint64_t m = cur_[kCur + depth + advance(step)];
                info_->nodes[depth] += cur_[kCur + depth];
                ++info_->descents;
                if ((e = reset_chunk()) != hipSuccess) return e;
                if (m != 0 && (e = walk(nullptr, kids, m, depth + advance(step), level + 1)) != hipSuccess) return e;
                i0 += 1;
                np = 1;
                continue;
            }
            ++info_->chunks;
            unsigned long long widest = 1;
            for (uint32_t d = depth; d <= k_; ++d) {
                info_->nodes[d] += cur_[kCur + d];
                if (d < k_ || staging()) widest = std::max(widest, cur_[kCur + d]);  // (the last level is not materialised unless staged)
            }
            if (staging() && cur_[kCur + k_] != 0 && (e = (*hook_)(staged_, cur_[kCur + k_])) != hipSuccess) return e;
            if ((e = reset_chunk()) != hipSuccess) return e;
            i0 += c;
            const double per_seed = double(widest) / double(c);
            np = uint64_t(std::max(1.0, std::min(double(uint64_t(1) << 26), double(w_.cap) / 4.0 / std::max(per_seed, 1e-6))));
        }
        return hipSuccess;
    }

    bool staging() const { return sink_.mode == kSinkStage; }

    const IndexView &ix_;
    SpectrumSeeds seeds_;
    uint32_t k_;
    Env env_;
    Sink sink_;
    Work w_;
    SpectrumInfo *info_;
    hipStream_t stream_;
    const SpectrumChunkHook *hook_;  // kSinkStage: what takes a chunk's k-mers
    const Node *staged_ = nullptr;
    std::vector<unsigned long long> cur_;
};

}  // namespace

uint64_t spectrum_frontier_nodes(uint64_t total, uint64_t free_bytes, uint64_t wanted) {
    if (wanted) return std::max(wanted, kSpectrumMinFrontier);
    const uint64_t by_memory = std::max<uint64_t>(uint64_t(1) << 16, std::min<uint64_t>(uint64_t(1) << 27, free_bytes / 8 / (2 * sizeof(Node))));
    return std::min(by_memory, std::max<uint64_t>(total + 1024, 4096));
}

uint64_t spectrum_work_bytes(uint64_t frontier_nodes) { return kHeadBytes + 2 * frontier_nodes * sizeof(Node); }

uint64_t spectrum_rank_bytes(uint64_t total) {
    const uint64_t nblocks = rank_blocks(total);
    return nblocks * (kSpectrumRankRows / 8) + (nblocks + scan_scratch_words(nblocks)) * sizeof(uint64_t);
}

hipError_t spectrum_histogram(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, void *d_work, uint64_t frontier_nodes, uint64_t *d_hist, uint64_t n_bins,
                              uint64_t *distinct, uint64_t *occurrences, SpectrumInfo *info, hipStream_t stream) {
    if (n_bins < 2 || !d_hist || !d_work) return hipErrorInvalidValue;
    Sink sink{};
    sink.mode = kSinkHist;
    sink.min = 1;
    sink.max = ~0ull;
    sink.hist = reinterpret_cast<unsigned long long *>(d_hist);
    sink.n_bins = n_bins;
    Walker walker(ix, seeds, k, 1, sink, d_work, frontier_nodes, info, stream);
    const hipError_t e = walker.run();
    if (e != hipSuccess) return e;
    *distinct = info->nodes[k];
    *occurrences = walker.occurrences();
    return hipSuccess;
}

hipError_t spectrum_count(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t min_count, uint64_t max_count, void *d_work, uint64_t frontier_nodes,
                          void *d_rank, uint64_t *n, SpectrumInfo *info, hipStream_t stream) {
    if (!d_work) return hipErrorInvalidValue;
    Sink sink{};
    sink.mode = kSinkCount;
    sink.min = std::max<uint64_t>(min_count, 1);
    sink.max = max_count ? max_count : ~0ull;
    RankView r{};
    if (d_rank) {
        r = rank_view(d_rank, ix.total);
        const hipError_t e = hipMemsetAsync(r.bitmap, 0, r.nblocks * (kSpectrumRankRows / 8), stream);
        if (e != hipSuccess) return e;
        sink.bitmap = r.bitmap;
    }
    Walker walker(ix, seeds, k, sink.min, sink, d_work, frontier_nodes, info, stream);
    hipError_t e = walker.run();
    if (e != hipSuccess) return e;
    *n = info->nodes[k];
    if (d_rank) {
        hipLaunchKernelGGL(k_spectrum_block_marks, dim3(uint32_t(std::min<uint64_t>((r.nblocks + 255) / 256, 2048))), dim3(256), 0, stream, r.bitmap, r.nblocks, r.prefix);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = exclusive_scan(r.prefix, r.nblocks, r.scan, stream)) != hipSuccess) return e;
        e = hipStreamSynchronize(stream);
    }
    return e;
}

hipError_t spectrum_dump(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t min_count, uint64_t max_count, void *d_work, uint64_t frontier_nodes,
                         const void *d_rank, uint64_t *d_kmers, uint64_t *d_counts, uint64_t *d_l, uint64_t capacity, uint32_t *flags, SpectrumInfo *info,
                         hipStream_t stream) {
    if (!d_work || !d_kmers || !flags) return hipErrorInvalidValue;
    Sink sink{};
    sink.mode = d_rank ? kSinkScatter : kSinkAppend;
    sink.min = std::max<uint64_t>(min_count, 1);
    sink.max = max_count ? max_count : ~0ull;
    if (d_rank) {
        const RankView r = rank_view(d_rank, ix.total);
        sink.bitmap = r.bitmap;
        sink.prefix = r.prefix;
    }
    sink.kmers = d_kmers;
    sink.counts = d_counts;
    sink.l = d_l;
    sink.capacity = capacity;
    sink.flags = flags;
    Walker walker(ix, seeds, k, sink.min, sink, d_work, frontier_nodes, info, stream);
    return walker.run();
}

hipError_t spectrum_stage(const IndexView &ix, SpectrumSeeds seeds, uint32_t k, uint64_t prune, void *d_work, uint64_t frontier_nodes, const SpectrumChunkHook &per_chunk,
                          SpectrumInfo *info, hipStream_t stream) {
    if (!d_work || !per_chunk) return hipErrorInvalidValue;
    Sink sink{};
    sink.mode = kSinkStage;
    Walker walker(ix, seeds, k, prune, sink, d_work, frontier_nodes, info, stream, &per_chunk);
    return walker.run();
}

}  // namespace msbwt
