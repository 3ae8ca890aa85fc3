// gfx950 (MI355X, CDNA4): count_kmers when k IS the depth of a complete sparse suffix table (sparse_table.hpp) -- the table's range is
// the count, a query is ONE hashed 128-byte bucket line.  The lanes kernel (lanes_kernel.hpp) serves that case as a search that happens
// to have no steps: ring, tickets per query, second-line slots, a full wait after every step.  This kernel is the lookup alone: lines are
// fetched in the shape that set the line-rate ceiling (tools/ubench_granule.hip) -- 8 lanes per line, 16 bytes per lane, plain loads
// into registers, eight lines per lane in flight --, and every lane then scans its OWN query's line.
//
// A wave owns a tile of 64 consecutive queries (matrix mode: n x k symbol codes):
//   1. lane q validates and packs row q (the tile's bytes staged through LDS and packed four symbols an instruction, search_common.hpp)
//      and hashes it once: bucket, tag;
//   2. the NEXT tile's bytes are asked for -- they travel while this tile's lines do;
//   3. eight batches of eight lines are asked for back to back: in batch b the 8-lane group g fetches the bucket of query 8 b + g;
//   4. half a tile at a time the landed pieces are handed to their queries' lanes through LDS (the lanes kernel's conflict-free line
//      layout), and lane q scans the line of query q: the scan of lookup_kernel.hpp over an accessor that reads LDS;
//   5. the few queries whose bucket had displaced entries go on to the next bucket, up to eight of them per further batch (wave-uniform
//      loop, at most `probe` rounds);
//   6. rows with '$' / 'N' -- no table entry stands for them -- are searched from [0, total) right here, eight at a time, one 8-lane group
//      each (rank_ops.hpp, constrain: plane blocks), rows with a code >= 6 get u64::MAX and the status flag: what the lanes kernel gives
//      them; counts leave as one coalesced store per tile.
// Tiles are dealt out like the lanes kernel's (sharded atomic tickets, a segment ahead).  6.3 KiB of LDS per wave, no scratch.
#include "lookup_kernel.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "rank_ops.hpp"

namespace msbwt {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLookupWaves = 4;    // per workgroup; every wave works alone (wave-level synchronisation only)
constexpr int kHalfBatches = 4;    // batches of eight lines whose pieces pass through LDS at a time: half a tile

// A batch's 64 pieces take one region of LDS, lane j's at piece j; as in the lanes kernel (lanes_kernel.hpp, region_base) every odd
// region is pushed 128 bytes further, and lane (g, c) holds chunk c ^ g of its group's line, so that the 64 lanes' read-back of "chunk j
// of my line" touches every bank once per 16 lanes.
__device__ constexpr uint32_t lookup_region_base(uint32_t i) { return 136u * (i >> 1) + 72u * (i & 1u); }
__device__ __forceinline__ uint32_t lookup_line_base(uint32_t s) { return lookup_region_base(s >> 3) + 8u * (s & 7u); }  // line of slot s = 8 region + group

struct LookupScratch {
    uint4 rows[(kStageLead + uint32_t(kTile) * uint32_t(kMaxShortK)) / 16u];  // the tile's query bytes (pack_row_swar reads in front of a row: kStageLead)
    uint4 lines[(kHalfBatches / 2) * 136];                                    // half a tile's bucket lines
};

// a table line is used once and the table dwarfs the caches (the launch's condition: IndexView::stream_lines): the non-temporal hint
__device__ __forceinline__ uint4 load_line_piece(const uint4 *p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// lane of the g-th lowest set bit of `mask` for the lanes of group g (64: the mask has fewer); *rest = the mask without its eight lowest
__device__ __forceinline__ uint32_t nth_set_for_group(uint64_t mask, uint32_t group, uint64_t *rest) {
    uint32_t src = 64u;
#pragma unroll
    for (uint32_t g = 0; g < 8u; ++g) {
        if (mask != 0ull) {  // wave-uniform
            const uint32_t at = uint32_t(__builtin_ctzll(mask));
            mask &= mask - 1ull;
            src = group == g ? at : src;
        }
    }
    *rest = mask;
    return src;
}

// kTagBits: the table's layout (lookup_layout).  Six waves per SIMD is what the LDS allows (24 per CU): at most 80 VGPRs.
template <int kTagBits>
__global__ __launch_bounds__(64 * kLookupWaves) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_count_kmers_lookup(const uint4 *__restrict__ table, uint32_t nbuckets, uint32_t probe, uint32_t depth,
                                                                          const uint4 *__restrict__ side, const uint4 *__restrict__ blocks, uint64_t total,
                                                                          const uint8_t *__restrict__ kmers, uint32_t k, uint64_t n,
                                                                          uint64_t *__restrict__ out, uint32_t *__restrict__ flags,
                                                                          unsigned long long *__restrict__ tile_counter, uint32_t grain) {
    constexpr SparseLayout L = lookup_layout(kTagBits);
    __shared__ LookupScratch scratch[kLookupWaves];
    const uint32_t lane = threadIdx.x & 63u, sub = lane & 7u, group = lane >> 3;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint4 *stage = scratch[wave].rows;
    uint4 *lines = scratch[wave].lines;
    const uint8_t *stage_bytes = reinterpret_cast<const uint8_t *>(stage) + kStageLead;
    const uint32_t *line_words = reinterpret_cast<const uint32_t *>(lines);
    const uint64_t ntiles = (n + kTile - 1) / kTile;
    const uint32_t nbits = 2u * depth;
    const uint32_t my_chunk = sub ^ group;  // the piece of its group's line this lane fetches

    // tiles in segments of `grain`, dealt out by tickets as in the lanes kernel: a wave's first segment is its own index, further ones
    // come from one of up to kTicketCounters counters, drawn a segment ahead; without counters (small launches) the waves stride
    const uint32_t nwaves = gridDim.x * uint32_t(kLookupWaves), gw = blockIdx.x * uint32_t(kLookupWaves) + wave;
    const uint32_t ncounters = min(uint32_t(kTicketCounters), max(1u, nwaves >> 3));
    const uint32_t my_counter = (gw >> 3) % ncounters;
    uint64_t static_next = (uint64_t(gw) + nwaves) * grain;
    auto take_ticket = [&]() -> uint64_t {
        if (tile_counter == nullptr) {
            const uint64_t t = static_next;
            static_next += uint64_t(nwaves) * grain;
            return t;
        }
        unsigned long long t = 0;
        if (lane == 0u) t = atomicAdd(tile_counter + my_counter * 16u, 1ull);
        const uint64_t drawn = (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(t >> 32))))) << 32) |
                               uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(t))));
        return (uint64_t(nwaves) + my_counter + drawn * uint64_t(ncounters)) * grain;
    };
    uint64_t next_tile = uint64_t(gw) * grain;
    uint32_t seg_left = grain;
    uint64_t seg_after = take_ticket();

    constexpr int kPieces = kTile * kMaxShortK / 16 / 64;  // 16-byte pieces of a tile per lane: 2
    uint4 rows[kPieces];
    auto fetch_rows = [&](uint64_t tile) {
#pragma unroll
        for (int i = 0; i < kPieces; ++i) rows[i] = make_uint4(0, 0, 0, 0);
        if (tile >= ntiles) return;
        const uint64_t q0 = tile * kTile;
        const uint32_t nbytes = uint32_t(min(uint64_t(kTile), n - q0)) * k;
#pragma unroll
        for (int i = 0; i < kPieces; ++i) rows[i] = load_piece(kmers + q0 * k, nbytes, lane + 64u * uint32_t(i));
    };
    fetch_rows(next_tile);

    while (next_tile < ntiles) {
        const uint64_t q0 = next_tile * kTile;
        const uint32_t in_tile = uint32_t(min(uint64_t(kTile), n - q0));
        ++next_tile;
        if (--seg_left == 0u) {
            next_tile = seg_after;
            seg_left = grain;
            seg_after = take_ticket();
        }
        // ---- 1: this lane's row -> bucket and tag ----
#pragma unroll
        for (int i = 0; i < kPieces; ++i) stage[kStageLead / 16u + lane + 64u * uint32_t(i)] = rows[i];
        wave_lds_sync();
        const bool valid = lane < in_tile;
        PackedQuery<3> pq;
        pq.tidx = 0;
        pq.bad = false;
        pq.acgt = true;
        if (valid) pack_row_swar<3, 32>(k, depth, stage_bytes + lane * k, pq);
        const bool bad = valid && pq.bad;
        bool odd = valid && !pq.bad && !pq.acgt;       // '$' / 'N' in the row: searched, below
        bool pending = valid && !pq.bad && pq.acgt;    // to be looked up
        const uint64_t x = sparse_mix(pq.tidx, nbits);
        uint32_t bucket = pending ? sparse_bucket(x, nbits, nbuckets) : 0u;  // (a lane without a lookup names line 0: its group's load is a cache hit)
        const uint32_t want_lo = sparse_tag(x, L), want_hi = sparse_tag_hi(x, L);
        uint32_t dist = 0;
        uint64_t count = bad ? ~0ull : 0ull;
        // ---- 2: the next tile's rows start their trip ----
        fetch_rows(next_tile);
        // ---- 3: eight batches of eight lines ----
        uint4 v[8];
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) {
            const uint32_t gb = uint32_t(__shfl(int(bucket), int(8u * b + group)));
            v[b] = load_line_piece(table + uint64_t(gb) * 8u + my_chunk);
        }
        // this lane's query in the line of slot s of the staged lines
        auto look_up = [&](uint32_t s) {
            const uint32_t base = lookup_line_base(s), g7 = s & 7u;
            auto word_at = [&](uint32_t i) -> uint32_t { return line_words[(base + ((i >> 2) ^ g7)) * 4u + (i & 3u)]; };
            const LookupFound f = lookup_scan_line(L, want_lo, want_hi, word_at);
            if (f.width == kSparseEscapeWidth) {  // a high-copy suffix: its range is a flat {l, h} entry of the side array
                const uint4 e = side[lookup_entry_l(L, f.slot, word_at)];
                count = ((uint64_t(e.w) << 32) | e.z) - ((uint64_t(e.y) << 32) | e.x);
                pending = false;
            } else if (f.width != 0u) {
                count = f.width;
                pending = false;
            } else if (f.header > L.slots && dist < probe) {  // entries of this bucket were displaced: the next one
                ++bucket;
                ++dist;
            } else {  // a miss in a complete table: the suffix does not occur
                pending = false;
            }
        };
        // ---- 4: half a tile at a time through LDS, every lane scans its own query's line ----
#pragma unroll
        for (uint32_t half = 0; half < 2u; ++half) {
#pragma unroll
            for (uint32_t r = 0; r < uint32_t(kHalfBatches); ++r) lines[lookup_region_base(r) + lane] = v[kHalfBatches * half + r];
            wave_lds_sync();
            if ((lane >> 5) == half && pending) look_up(lane & 31u);
            wave_lds_sync();
        }
        // ---- 5: lookups that go on to the next bucket ----
        for (uint64_t todo = __ballot(pending); todo != 0ull; todo = __ballot(pending)) {  // wave-uniform
            uint64_t rest;
            const uint32_t src = nth_set_for_group(todo, group, &rest);
            const uint32_t theirs = uint32_t(__shfl(int(bucket), int(src & 63u)));  // (every lane shuffles: a pending lane's bucket is read)
            const uint32_t gb = src < 64u ? theirs : 0u;
            lines[lookup_region_base(0) + lane] = load_line_piece(table + uint64_t(gb) * 8u + my_chunk);
            wave_lds_sync();
            // the owner's rank among the pending lanes names the group that fetched its line
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(todo >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(todo), 0u));
            if (pending && rank < 8u) look_up(rank);
            wave_lds_sync();
        }
        // ---- 6: rows the table has no entry for ----
        if (__ballot(bad) != 0ull && bad) atomicOr(flags, kFlagInvalidSymbol);
        for (uint64_t todo = __ballot(odd); todo != 0ull;) {  // wave-uniform, rare
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(todo >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(todo), 0u));
            const uint32_t src = nth_set_for_group(todo, group, &todo);
            const bool gactive = src < 64u;
            const uint8_t *row = stage_bytes + (src & 63u) * k;  // (the tile's bytes stay staged until the next tile's replace them)
            Range r{0, total};
            bool broken = false;
            for (uint32_t j = k; j-- > 0u;) {  // wave-uniform trip count; a group leaves the steps once its range is empty
                if (gactive && r.l != r.h && !broken) {
                    r = constrain(blocks, uint32_t(row[j]), r.l, r.h, sub);
                    broken = r.h > total || r.l > r.h;
                }
            }
            const uint64_t got = broken ? ~0ull : r.h - r.l;
            const uint32_t from = (rank & 7u) * 8u;
            const uint64_t mine = (uint64_t(uint32_t(__shfl(int(uint32_t(got >> 32)), int(from)))) << 32) | uint32_t(__shfl(int(uint32_t(got)), int(from)));
            const bool was_broken = __shfl(int(broken), int(from)) != 0;
            if (odd && rank < 8u) {
                count = mine;
                odd = false;
                if (was_broken) atomicOr(flags, kFlagInternal);
            }
        }
        if (valid) out[q0 + lane] = count;
        wave_lds_sync();  // every lane has read its staged bytes: the next tile's may replace them
    }
}

template <int kTagBits>
uint32_t lookup_resident_blocks() {
    static const uint32_t cached = [] {
        int device = 0, cus = 0, per_cu = 0;
        if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_count_kmers_lookup<kTagBits>, 64 * kLookupWaves, 0) != hipSuccess || cus <= 0 || per_cu <= 0)
            return 6u * 256u;
        return uint32_t(cus) * uint32_t(per_cu);
    }();
    return cached;
}

template <int kTagBits>
hipError_t launch_lookup_layout(const IndexView &ix, const SparseView &sp, const QuerySource &src, uint32_t *flags, hipStream_t stream) {
    const uint64_t tiles = (src.n + kTile - 1) / kTile;
    if (tiles > (1ull << 32)) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((tiles + kLookupWaves - 1) / kLookupWaves, lookup_resident_blocks<kTagBits>());
    const uint64_t waves = blocks * kLookupWaves;
    const bool tickets = ix.tile_counter != nullptr && tiles > waves;
    if (tickets) {
        const hipError_t zeroed = hipMemsetAsync(ix.tile_counter, 0, kTicketBytes, stream);
        if (zeroed != hipSuccess) return zeroed;
    }
    const uint32_t grain = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(16, tiles / (waves * 8))));
    if (std::getenv("MSBWT_VERBOSE"))
        std::fprintf(stderr, "[msbwt] lookup kernel <%d>: depth %u, %llu queries, %llu workgroups\n", kTagBits, sp.depth, (unsigned long long)src.n,
                     (unsigned long long)blocks);
    hipLaunchKernelGGL((k_count_kmers_lookup<kTagBits>), dim3(uint32_t(blocks)), dim3(64 * kLookupWaves), 0, stream, static_cast<const uint4 *>(sp.lines),
                       sp.nbuckets, sp.probe, sp.depth, static_cast<const uint4 *>(sp.side), static_cast<const uint4 *>(ix.blocks), ix.total, src.data, src.k, src.n,
                       src.out_fwd, flags, tickets ? static_cast<unsigned long long *>(ix.tile_counter) : nullptr, grain);
    return hipGetLastError();
}

}  // namespace

// Which launches: decided shape by shape (query matrix / read windows x tag width) by alternating this kernel and the lanes kernel on one
// card, and a shape is served here only where this kernel's slowest run beat the lanes kernel's fastest (docs/MEASUREMENT_HISTORY.md):
//   query matrix, 40-bit tags, a table far larger than the caches (stream_lines; human scale: 9.21-9.34 -> 8.52-9.03 ms)   here
//   query matrix, 40-bit tags, a table of a few GB (C4: 3.051-3.053 against 3.036-3.075 ms)                               lanes kernel
//   query matrix, 24-bit tags (C2, cache-resident: 0.234-0.238 against 0.246 ms)                                         lanes kernel
//   query matrix, 32-bit tags; read windows (no such kernel body yet)                                                    not measured: lanes kernel
bool lookup_serves(const IndexView &ix, const QuerySource &src, bool reads) {
    if (reads || ix.search_kernel != kSearchAuto || ix.block_format != kBlocksPlanes || ix.counters != nullptr || ix.done != nullptr || !ix.stream_lines) return false;
    if (src.packed != 0u || src.inline_n != 0u || src.range_stride != 0u || src.out_index != nullptr || src.place_inline != 0u || src.n < uint64_t(kTile)) return false;
    const SparseView *sp = sparse_for(ix, src.k);
    return sp != nullptr && sp->tier == 0u && sp->depth == src.k && sparse_layout(sp->depth).tag_bits == 40u;
}

hipError_t launch_lookup(const IndexView &ix, const QuerySource &src, uint32_t *flags, hipStream_t stream) {
    if (!lookup_serves(ix, src, false) || (reinterpret_cast<uintptr_t>(src.data) & 15u) != 0) return hipErrorInvalidValue;
    return launch_lookup_layout<40>(ix, *sparse_for(ix, src.k), src, flags, stream);
}

}  // namespace msbwt
