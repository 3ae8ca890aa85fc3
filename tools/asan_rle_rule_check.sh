#!/bin/bash
# CPU-only sanitizer pass over the host side of the RLE digit rule (GPU AddressSanitizer is not available on this pool):
# csrc/rle_subruns.hpp's recurrence and merge.hip's scan_merge_input, which is built on it, in a stand-alone program with
# -fsanitize=address,undefined on the host side of the hipcc line (scan_merge_input lives in merge.hip, so that unit and the
# encoder it links against are compiled whole).  The program calls no HIP function and needs no GPU.
# It compares totals, long-piece counts and statuses with a byte-serial restatement of the format over seeded random streams
# and over the edge streams of the GPU tests (a run's digits across byte 16 and byte 4096, eight and nine digits, 2^40 - 1 and 2^40).
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
cat > "$WORK/main.cpp" <<'CPP'
#include <cstdio>
#include <random>
#include <vector>
#include "merge.hpp"
#include "rle_subruns.hpp"
using namespace msbwt;

// the format, byte by byte, with nothing shared with the code under test: a byte's weight is 32^(bytes of its symbol right
// before it), kept exactly while it fits and as "too heavy" from 2^40 on
static MergeInputStatus restated(const std::vector<uint8_t> &s, uint64_t *total, uint64_t *pieces) {
    const unsigned __int128 limit = (unsigned __int128)1 << 40;
    unsigned __int128 sum = 0, weight = 1;
    uint64_t np = 0;
    for (size_t i = 0; i < s.size(); ++i) {
        const unsigned sym = s[i] % 8, digit = s[i] / 8;
        if (sym > 5) return MergeInputStatus::kInvalidSymbol;
        weight = i > 0 && s[i - 1] % 8 == sym ? (weight < limit ? weight * 32 : limit) : 1;
        if (digit == 0) continue;
        if (weight >= limit) return MergeInputStatus::kTooLarge;
        const unsigned __int128 value = weight * digit;
        sum += value;
        if (sum >= limit) return MergeInputStatus::kTooLarge;
        if (value >= 1024) np += uint64_t((value + (1u << 20) - 1) >> 20);
    }
    *total = uint64_t(sum);
    *pieces = np;
    return MergeInputStatus::kOk;
}

static int failures = 0;
static void check(const std::vector<uint8_t> &s, const char *what) {
    uint64_t want_total = 0, want_pieces = 0;
    const MergeInputStatus want = restated(s, &want_total, &want_pieces);
    MergeInput got_in;
    std::vector<uint8_t> exact(s);  // the sanitizer sees a read past the last byte
    const MergeInputStatus got = scan_merge_input(exact.data(), exact.size(), &got_in);
    if (got != want || (want == MergeInputStatus::kOk && (got_in.total != want_total || got_in.long_pieces != want_pieces))) {
        std::printf("MISMATCH %s: status %d / %d, total %llu / %llu, pieces %llu / %llu\n", what, int(got), int(want), (unsigned long long)got_in.total,
                    (unsigned long long)want_total, (unsigned long long)got_in.long_pieces, (unsigned long long)want_pieces);
        ++failures;
    }
}

static std::vector<uint8_t> run_across_byte(size_t first_byte, const std::vector<unsigned> &digits) {
    std::vector<uint8_t> s;
    for (size_t i = 0; i < first_byte; ++i) s.push_back(uint8_t((1 + i % 2) | 1 << 3));
    for (unsigned d : digits) s.push_back(uint8_t(5 | d << 3));
    s.push_back(3 | 8 << 3);
    s.push_back(3 | 1 << 3);
    return s;
}

int main() {
    // the exponent stops at kMaxDigits however long a run of bytes is, and from there a byte stands for nothing
    int e = 0;
    for (int i = 1; i < 100; ++i) {
        e = next_exponent(e, true);
        const int want = i < kMaxDigits ? i : kMaxDigits;
        if (e != want || subrun_too_large(1, e) != (i >= kMaxDigits) || subrun_too_large(0, e) ||
            subrun_value(31, e) != (i < kMaxDigits ? uint64_t(31) << (5 * i) : 0)) {
            std::printf("MISMATCH exponent after %d bytes\n", i);
            ++failures;
        }
    }
    if (next_exponent(e, false) != 0) ++failures;
    check({}, "empty");
    check(run_across_byte(4095, {5, 7, 0, 3}), "tile border");
    check(run_across_byte(15, {5, 7, 0, 3}), "thread border");
    check(run_across_byte(13, {0, 0, 0, 0, 0, 0, 0, 1}), "eight digits");
    check(run_across_byte(13, {0, 0, 0, 0, 0, 0, 0, 31}), "eight digits, the largest");
    check(run_across_byte(13, {31, 31, 31, 31, 31, 31, 31, 31}), "2^40 - 1 in one run, and more behind it");
    check(run_across_byte(13, {0, 0, 0, 0, 0, 0, 0, 1, 0}), "a ninth digit of zero");
    check(run_across_byte(13, {0, 0, 0, 0, 0, 0, 0, 0, 1}), "a ninth digit");
    check(run_across_byte(0, std::vector<unsigned>(40, 0)), "forty zero digits");
    {
        std::vector<unsigned> d(40, 0);
        d[13] = 16;  // 16 * 32^13 = 2^69: zero in 64 bits
        check(run_across_byte(3, d), "a fourteenth digit");
        d[13] = 0, d[39] = 1;
        check(run_across_byte(3, d), "a fortieth digit");
    }
    {
        std::vector<uint8_t> s;  // 2^40 - 1 symbols, then one more
        for (int i = 0; i < 8; ++i) s.push_back(uint8_t(1 | 31 << 3));
        check(s, "2^40 - 1");
        s.push_back(2 | 1 << 3);
        check(s, "2^40");
        s.back() = 6 | 1 << 3;
        check(s, "a bad symbol behind 2^40 - 1");
    }
    std::mt19937_64 rng(11);
    for (int round = 0; round < 4000; ++round) {
        std::vector<uint8_t> s(size_t(rng() % 300));
        const int stick = int(rng() % 100), zero = int(rng() % 100), bad = round % 7 == 0 ? 2 : 0, low = int(rng() % 3);
        for (size_t i = 0; i < s.size(); ++i) {
            unsigned sym = unsigned(rng() % 6);
            if (i && int(rng() % 100) < stick) sym = s[i - 1] & 7u;
            if (int(rng() % 1000) < bad) sym = 6 + unsigned(rng() % 2);
            unsigned digit = int(rng() % 100) < zero ? 0u : unsigned(rng() % 32);
            if (low == 0 && i && (s[i - 1] & 7u) == sym) digit = rng() % 4 ? 0u : 1u;  // long runs that stay small
            s[i] = uint8_t(sym | digit << 3);
        }
        check(s, "random");
    }
    if (failures) return 1;
    std::puts("rle rule asan ok");
    return 0;
}
CPP
"$HIPCC" -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Irust-msbwt_amd/csrc "$WORK/main.cpp" rust-msbwt_amd/csrc/merge.hip rust-msbwt_amd/csrc/run_encode.hip \
    -o "$WORK/rle_rule_asan"
ASAN_OPTIONS=detect_leaks=1 "$WORK/rle_rule_asan"
