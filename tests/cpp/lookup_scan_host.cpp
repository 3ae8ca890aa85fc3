// The bucket scan of the lookup kernel (csrc/lookup_kernel.hpp) run on the host, under AddressSanitizer and UBSan: buckets of the three
// complete layouts are filled THROUGH the SparseLayout descriptors by linear probing as the builder does it (sparse_table.hip), with keys
// crafted through the inverted hash, and every present and absent key is counted by lookup_count -- the very scan the kernel runs over
// the lines it has staged.  Lines are kept in a map and every access is checked against the table's nbuckets + probe lines.
// Build: g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rust-msbwt_amd/csrc tests/cpp/lookup_scan_host.cpp
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "lookup_kernel.hpp"

using namespace msbwt;

namespace {

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

uint64_t inverse_odd(uint64_t a) {  // modulo 2^64 (and so modulo every 2^n): Newton's iteration doubles the correct bits
    uint64_t x = a;
    for (int i = 0; i < 6; ++i) x *= 2 - a * x;
    return x;
}

uint64_t unmix(uint64_t mixed, uint32_t n) {  // sparse_mix backwards
    const uint64_t mask = (uint64_t(1) << n) - 1u;
    uint64_t x = mixed & mask;
    x ^= x >> (n >> 1);
    x = (x * inverse_odd(0xD6E8FEB86659FD93ull)) & mask;
    x ^= x >> (n >> 1);
    x = (x * inverse_odd(0x9E3779B97F4A7C15ull)) & mask;
    return x;
}

struct Table {
    SparseLayout L;
    uint32_t depth, n, nbuckets, probe;
    std::map<uint64_t, std::array<uint32_t, 32>> lines;  // the lines that hold anything; every other line is zero
    std::vector<std::array<uint64_t, 2>> side;
    std::map<uint64_t, uint64_t> present;  // key -> count
    uint64_t last_line_read = 0;

    explicit Table(uint32_t d) : L(sparse_layout(d)), depth(d), n(2 * d) {
        nbuckets = uint32_t(sparse_min_buckets(int(d)));
        probe = uint32_t(sparse_probe_limit(int(d), nbuckets));
        CHECK(probe >= 7 && probe <= kSparseMaxProbe);
    }
    uint32_t word(uint64_t b, uint32_t i) {
        CHECK(b < uint64_t(nbuckets) + probe && i < 32);
        last_line_read = b > last_line_read ? b : last_line_read;
        const auto it = lines.find(b);
        return it == lines.end() ? 0u : it->second.at(i);
    }
    static void put_byte(std::array<uint32_t, 32> &line, uint32_t byte, uint32_t v) {
        uint32_t &w = line.at(byte >> 2);
        w = (w & ~(0xFFu << ((byte & 3u) * 8u))) | ((v & 0xFFu) << ((byte & 3u) * 8u));
    }
    static uint32_t get_half(const std::array<uint32_t, 32> &line, uint32_t byte) { return (line.at(byte >> 2) >> ((byte & 3u) * 8u)) & 0xFFFFu; }
    uint32_t used(const std::array<uint32_t, 32> &line) const {
        uint32_t u = 0;
        for (uint32_t i = 0; i < L.slots; ++i) u += (L.width_byte ? (line.at((L.width_byte + i) >> 2) >> (((L.width_byte + i) & 3u) * 8u)) & 0xFFu : line.at(i) >> kSparseWidthShift) != 0u;
        return u;
    }
    // the key with this mixed value occurs `count` times: an entry where linear probing finds room; -> how far from home
    uint32_t insert(uint64_t mixed, uint64_t count) {
        const uint64_t key = unmix(mixed, n);
        CHECK(sparse_mix(key, n) == mixed && count > 0 && present.count(key) == 0);
        present[key] = count;
        uint64_t b = sparse_bucket(mixed, n, nbuckets);
        for (uint32_t dist = 0; dist <= probe; ++dist, ++b) {
            auto &line = lines[b];
            const uint32_t header = get_half(line, L.header_byte);
            if (header < 0xFFFFu) line.at(L.header_byte >> 2) = (line.at(L.header_byte >> 2) & 0x0000FFFFu) | ((header + 1u) << 16);
            const uint32_t i = used(line);
            if (i == L.slots) continue;
            const bool wide = count >= kSparseEscapeWidth;
            const uint32_t width = wide ? kSparseEscapeWidth : uint32_t(count);
            uint64_t l = 1000u * present.size() + (uint64_t(b & 0xFFu) << 32);  // any 40-bit start of a range
            if (wide) {
                l = side.size();
                side.push_back({77u, 77u + count});
            }
            line.at(i) = sparse_tag(mixed, L) | (L.width_byte ? 0u : width << kSparseWidthShift);
            if (L.width_byte) put_byte(line, L.width_byte + i, width);
            if (L.tag_hi_byte) put_byte(line, L.tag_hi_byte + i, sparse_tag_hi(mixed, L));
            line.at(L.l_lo_word + i) = uint32_t(l);
            put_byte(line, L.l_hi_byte + i, uint32_t(l >> 32));
            return dist;
        }
        CHECK(!"no slot within the probe limit");
        return 0;
    }
    uint64_t count(uint64_t key) {
        return lookup_count(L, key, n, nbuckets, probe, [&](uint64_t b, uint32_t i) { return word(b, i); },
                            [&](uint64_t j) { return side.at(j)[1] - side.at(j)[0]; });
    }
    // [lo, hi) of the mixed values homed in bucket b
    void window(uint64_t b, uint64_t &lo, uint64_t &hi) const {
        const auto first_top = [&](uint64_t bucket) { return ((bucket << 32) + nbuckets - 1) / nbuckets; };
        lo = first_top(b) << (n - 32);
        hi = first_top(b + 1) << (n - 32);
    }
};

void run(uint32_t depth) {
    Table t(depth);
    const SparseLayout &L = t.L;
    const uint64_t tag_span = uint64_t(1) << L.tag_bits;
    std::vector<uint64_t> absent;
    uint64_t lo, hi;
    // a bucket exactly full: every entry found at home, an absent key homed there ends there (header == slots: nothing was displaced)
    const uint64_t nb = t.nbuckets;
    t.window(nb / 8, lo, hi);
    for (uint32_t i = 0; i < L.slots; ++i) CHECK(t.insert(lo + 3 + 5 * i, 1 + i) == 0);
    absent.push_back(lo + 4);
    // tag 0: present beside empty slots, and absent in a bucket with empty slots (an empty slot's tag word matches it)
    // (at the least bucket count a tag recurs every probe + 1 buckets: the values with tag 0 are the multiples of 2^tag_bits)
    const uint64_t tag0 = (uint64_t(1) << (t.n - 2)), tag0_absent = tag0 + 5 * tag_span;
    CHECK(sparse_tag(tag0, L) == 0 && sparse_tag_hi(tag0, L) == 0 && sparse_tag(tag0_absent, L) == 0 && sparse_tag_hi(tag0_absent, L) == 0);
    t.window(sparse_bucket(tag0, t.n, t.nbuckets), lo, hi);
    CHECK(tag0 >= lo && tag0 < hi && lo + 9 != tag0);
    CHECK(t.insert(lo + 9, 3) == 0);
    CHECK(t.insert(tag0, 5) == 0);
    t.window(sparse_bucket(tag0_absent, t.n, t.nbuckets), lo, hi);
    CHECK(tag0_absent >= lo && tag0_absent < hi && lo + 9 != tag0_absent);
    CHECK(t.insert(lo + 9, 2) == 0);
    absent.push_back(tag0_absent);
    // 40-bit tags: entries of one bucket that share their low word, and an absent key that shares it too
    if (L.tag_hi_byte != 0) {
        t.window(nb / 2 + 100, lo, hi);
        const uint64_t base = ((lo >> 32) + 1) << 32 | 0x5EEDBEE5u;
        for (uint64_t j = 0; j < 3; ++j) CHECK(base + (j << 32) < hi && t.insert(base + (j << 32), 7 + j) == 0);
        absent.push_back(base + (uint64_t(3) << 32));
    }
    // the escape width: a range 255 and more wide lives in the side array; 254 is the widest that does not
    t.window(nb / 2 + 200, lo, hi);
    CHECK(t.insert(lo + 1, 254) == 0);
    CHECK(t.insert(lo + 2, 255) == 0);
    CHECK(t.insert(lo + 3, 1000000007ull) == 0);
    CHECK(t.side.size() == 2);
    // chains of `probe`: slots * probe + 1 keys homed in ONE bucket, the last one exactly `probe` buckets from home -- mid-table, and at
    // the last bucket, where the chain ends in line nbuckets - 1 + probe: the last line there is
    for (const uint64_t home : {3 * nb / 4, nb - 1}) {
        t.window(home, lo, hi);
        uint32_t far = 0;
        for (uint32_t i = 0; i < L.slots * t.probe + 1; ++i) far = t.insert(lo + 1 + 2 * i, 1 + i % 200);
        CHECK(far == t.probe);
        absent.push_back(lo + 2);  // walks the whole chain and ends at the probe limit
        if (home + 3 < t.nbuckets) {
            t.window(home + 3, lo, hi);
            absent.push_back(lo + 6);  // homed inside a foreign chain
        }
    }
    t.last_line_read = 0;
    for (const auto &kv : t.present) CHECK(t.count(kv.first) == kv.second);
    CHECK(t.last_line_read == uint64_t(t.nbuckets) - 1 + t.probe);
    for (const uint64_t mixed : absent) {
        const uint64_t key = unmix(mixed, t.n);
        CHECK(sparse_mix(key, t.n) == mixed && t.present.count(key) == 0 && t.count(key) == 0);
    }
    // keys homed where nothing is: the first and the last bucket's neighbours
    CHECK(t.count(unmix(12345, t.n)) == 0);
    std::printf("depth %u: %u-bit tags, %u slots, probe %u: %zu present and %zu absent keys\n", depth, L.tag_bits, L.slots, t.probe, t.present.size(), absent.size());
}

}  // namespace

int main() {
    for (const uint32_t depth : {16u, 24u, 25u, 28u, 30u, 31u}) run(depth);
    std::printf("lookup scan: all host checks passed\n");
    return 0;
}
