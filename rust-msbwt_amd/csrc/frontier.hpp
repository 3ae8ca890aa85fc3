// Frontier expansion over the suffixes that OCCUR -- the leaves: the node, the workgroup's slot reservation and sums, the seeds, and
// what one pair-block line (16 children, two symbols deeper) or one plane-block line (4 children, one symbol deeper) says about a
// node's bounds.  frontier_walk.hpp is the walk made of them (its kernels, chunks, retries and descents), which the builder of the
// sparse suffix table (sparse_table.hip) and the k-mer spectrum / enumeration (spectrum.hip) run with their own sinks.
// Include from HIP translation units only (the names are per translation unit, as in rank_ops.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rank_ops.hpp"
#include "workgroup.hpp"

namespace msbwt {
namespace {

// a suffix that occurs: key = the table index of the direct table (A C G T -> 0..3, step t at bits [2t, 2t+2), step 0 = the LAST
// symbol) -- which is also the packed 2-bit word of msbwt_kmers_pack_2bit -- and its range [l, h)
struct Node {
    uint64_t key, l, h;
};

constexpr int kFrontierThreads = 512;
constexpr int kFrontierWaves = kFrontierThreads / 64;

// this thread's first of `mine` consecutive slots behind *cursor: one atomic per workgroup.  Every thread of the block calls it.
__device__ __forceinline__ uint64_t reserve(uint32_t mine, unsigned long long *cursor) {
    __shared__ uint32_t wave_total[kFrontierWaves];
    __shared__ unsigned long long block_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_sum(mine);
    if (lane == 63u) wave_total[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kFrontierWaves; ++w) {
            const uint32_t x = wave_total[w];
            wave_total[w] = t;
            t += x;
        }
        block_base = t ? atomicAdd(cursor, (unsigned long long)t) : 0ull;
    }
    __syncthreads();
    const uint64_t first = block_base + wave_total[wave] + (inc - mine);
    __syncthreads();  // (the shared words are rewritten by the next call)
    return first;
}

// adds the block's sum of `mine` to *acc
__device__ __forceinline__ void block_add(uint32_t mine, unsigned long long *acc) {
    __shared__ uint32_t part[kFrontierWaves];
    const uint32_t s = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kFrontierWaves; ++w) t += part[w];
        if (t) atomicAdd(acc, (unsigned long long)t);
    }
    __syncthreads();
}

// seed `idx`: entry idx of the flat direct table (16-byte {l, h} entries), or the root [0, total) without one; empty = l == h
__device__ __forceinline__ Node seed_node(const uint4 *__restrict__ flat, uint64_t idx, uint64_t total) {
    if (flat == nullptr) return Node{0, 0, total};
    const uint4 e = flat[idx];
    return Node{idx, (uint64_t(e.y) << 32) | e.x, (uint64_t(e.w) << 32) | e.z};
}

// ---- what one pair-block line says about a position: the 16 pair counts before it, relative to the superblock ---------------
struct PairSixteen {
    uint32_t rel[16];  // header field + matches among the block's first r positions
};

__device__ __forceinline__ void pair_line_sixteen(const uint4 *__restrict__ blk, uint32_t r, PairSixteen &out) {
    const uint4 a0 = blk[0], a1 = blk[1], b0 = blk[2], b1 = blk[3], v = blk[kPairValidChunk];
    const uint4 h5 = blk[kPairLoChunk], h6 = blk[kPairLoChunk + 1], h7 = blk[kPairHiChunk];
    const uint32_t A0[4] = {a0.x, a0.y, a0.z, a0.w}, A1[4] = {a1.x, a1.y, a1.z, a1.w}, B0[4] = {b0.x, b0.y, b0.z, b0.w},
                   B1[4] = {b1.x, b1.y, b1.z, b1.w}, V[4] = {v.x, v.y, v.z, v.w};
    const uint32_t lo16[8] = {h5.x, h5.y, h5.z, h5.w, h6.x, h6.y, h6.z, h6.w}, hi8[4] = {h7.x, h7.y, h7.z, h7.w};
    uint32_t am[4][4], bm[4][4];  // [code][word]: positions (among the first r) whose S / S2 is that code
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t low = low_bits(min(max(int(r) - 32 * w, 0), 32));
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t n0 = (c & 1u) - 1u, n1 = ((c >> 1) & 1u) - 1u;
            am[c][w] = (A0[w] ^ n0) & (A1[w] ^ n1) & V[w] & low;
            bm[c][w] = (B0[w] ^ n0) & (B1[w] ^ n1);
        }
    }
#pragma unroll
    for (uint32_t p = 0; p < 16; ++p) {
        const uint32_t a = p >> 2, b = p & 3u;
        uint32_t cnt = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) cnt += uint32_t(__popc(am[a][w] & bm[b][w]));
        const uint32_t field = ((lo16[p >> 1] >> ((p & 1u) * 16u)) & 0xFFFFu) | (((hi8[p >> 2] >> ((p & 3u) * 8u)) & 0xFFu) << 16);
        out.rel[p] = field + cnt;
    }
}

// One pair step of a node: the lines of its two bounds (one line when both lie in the same block) and their superblocks.  While
// same_super() holds, child p's width is H.rel[p] - L.rel[p] without a 64-bit operation; its range comes from pair_child.
struct PairStep {
    PairSixteen L, H;
    uint64_t sb_l, sb_h;
    __device__ __forceinline__ bool same_super() const { return sb_l == sb_h; }
};

__device__ __forceinline__ void pair_step_lines(const Node &nd, const uint4 *__restrict__ pair_blocks, bool s96, PairStep &st) {
    const uint64_t bl = pair_block_of(nd.l, s96), start_l = pair_block_start(bl, s96);
    const bool same = (nd.h - start_l) < 128u;
    const uint64_t bh = same ? bl : pair_block_of(nd.h, s96);
    pair_line_sixteen(pair_blocks + bl * 8u, uint32_t(nd.l - start_l), st.L);
    pair_line_sixteen(pair_blocks + bh * 8u, uint32_t(nd.h - pair_block_start(bh, s96)), st.H);
    st.sb_l = bl >> kPairSuperBlocks;
    st.sb_h = bh >> kPairSuperBlocks;
}

// child p = 4 a + b of the step (first a, then b): its range, and its key at `depth` symbols so far
__device__ __forceinline__ void pair_child(const uint64_t *__restrict__ pair_super, const PairStep &st, uint32_t p, uint64_t &nl, uint64_t &nh) {
    nl = pair_super[st.sb_l * 16u + p] + st.L.rel[p];
    nh = pair_super[st.sb_h * 16u + p] + st.H.rel[p];
}
__device__ __forceinline__ uint64_t pair_child_key(uint64_t key, uint32_t depth, uint32_t p) {
    return key | (uint64_t(p >> 2) << (2u * depth)) | (uint64_t(p & 3u) << (2u * depth + 2u));
}

// ---- one symbol further from the plane blocks ----------------------------------------------------------------------------------
// start_index[s] + rank(s, pos) for the four ACGT symbols by ONE thread straight from the plane block (plane_index.hpp)
__device__ __forceinline__ void plane_line_four(const uint4 *__restrict__ blk, uint32_t r, uint64_t (&out)[4]) {
    uint32_t cnt[4] = {0, 0, 0, 0}, meta[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint4 c = blk[j];
        meta[j] = c.w;
        const uint32_t low = low_bits(min(max(int(r) - 32 * j, 0), 32));
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t s = q == 3u ? 5u : q + 1u;
            const uint32_t x0 = (s & 1u) ? 0u : ~0u, x1 = (s & 2u) ? 0u : ~0u, x2 = (s & 4u) ? 0u : ~0u;
            cnt[q] += uint32_t(__popc((c.x ^ x0) & (c.y ^ x1) & (c.z ^ x2) & low));
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t s = q == 3u ? 5u : q + 1u;
        const uint32_t hi = (((s >> 2) ? meta[7] : meta[6]) >> ((s & 3u) * 8u)) & 0xFFu;
        out[q] = ((uint64_t(hi) << 32) | meta[s]) + cnt[q];
    }
}

// One plane step of a node: the ranges [nl[q], nh[q]) of its four children q (A C G T), key | q << 2 depth
__device__ __forceinline__ void plane_step(const Node &nd, const uint4 *__restrict__ blocks, uint64_t (&nl)[4], uint64_t (&nh)[4]) {
    plane_line_four(blocks + (nd.l >> 8) * 8u, uint32_t(nd.l) & 255u, nl);
    plane_line_four(blocks + (nd.h >> 8) * 8u, uint32_t(nd.h) & 255u, nh);
}
__device__ __forceinline__ uint64_t plane_child_key(uint64_t key, uint32_t depth, uint32_t q) { return key | (uint64_t(q) << (2u * depth)); }

}  // namespace
}  // namespace msbwt
