// msbwt_hip.hpp -- header-only C++17 mirror of the reference's `msbwt_core::BWT` trait and of
// `rle_bwt::RleBWT`, over the C ABI of msbwt_hip.h.
//
// The reference is Rust (src/msbwt_core.rs:28-162, src/rle_bwt.rs); where no Rust toolchain is
// available this is the compiled-language host side: same names, same argument meaning, same
// error behaviour (io errors -> std::system_error / msbwt::UnexpectedEof, the reference's
// panics -> msbwt::Panic).  The Rust `impl BWT for GpuRleBWT` over the same symbols is in
// INTEGRATION.md.  Every query runs on the GPU; there is no CPU fallback.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <iterator>
#include <stdexcept>
#include <string>
#include <system_error>
#include <vector>

#include "msbwt_hip.h"

namespace msbwt {

constexpr std::size_t VC_LEN = MSBWT_VC_LEN;            // src/msbwt_core.rs:4
constexpr std::size_t LETTER_BITS = MSBWT_LETTER_BITS;  // :6
constexpr std::size_t NUMBER_BITS = MSBWT_NUMBER_BITS;  // :8
constexpr std::size_t NUM_POWER = MSBWT_NUM_POWER;      // :10
constexpr std::uint8_t MASK = MSBWT_MASK;               // :12
constexpr std::uint8_t COUNT_MASK = MSBWT_COUNT_MASK;   // :14

/// Half-open range [l, h) of the BWT (src/msbwt_core.rs:18-24).
struct BWTRange {
    std::uint64_t l = 0;
    std::uint64_t h = 0;
    bool operator==(const BWTRange &o) const { return l == o.l && h == o.h; }
    bool operator!=(const BWTRange &o) const { return !(*this == o); }
};

/// What the reference does with `panic!` / `assert!` / an out-of-bounds index.
struct Panic : std::runtime_error {
    int code;
    Panic(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
/// io::ErrorKind::UnexpectedEof (src/rle_bwt.rs:129-148).
struct UnexpectedEof : std::runtime_error {
    explicit UnexpectedEof(const std::string &m) : std::runtime_error(m) {}
};

/// The trait surface (src/msbwt_core.rs:28-162).
class BWT {
  public:
    virtual ~BWT() = default;
    virtual void load_vector(const std::vector<std::uint8_t> &bwt) = 0;
    virtual void load_numpy_file(const std::string &filename) = 0;
    virtual std::uint64_t get_symbol_count(std::uint8_t symbol) const = 0;
    virtual std::uint64_t get_total_size() const = 0;
    virtual BWTRange constrain_range(std::uint8_t sym, const BWTRange &input_range) const = 0;
    virtual std::uint64_t count_kmer(const std::vector<std::uint8_t> &kmer) const = 0;
};

/// Drop-in for `RleBWT` (src/rle_bwt.rs:14-24) whose index lives in the HBM of an MI355X.
class RleBWT final : public BWT {
  public:
    RleBWT() : RleBWT(8) {}                                    // RleBWT::new(), :297
    static RleBWT with_bin_power(std::uint8_t bin_power, int device = -1) { return RleBWT(bin_power, device); }  // :309
    explicit RleBWT(std::uint8_t bin_power, int device = -1) : raw_(msbwt_rle_new_on_device(bin_power, device)) {
        if (!raw_) throw std::bad_alloc();
    }
    ~RleBWT() override { msbwt_rle_free(raw_); }
    RleBWT(RleBWT &&o) noexcept : raw_(o.raw_) { o.raw_ = nullptr; }
    RleBWT &operator=(RleBWT &&o) noexcept {
        if (this != &o) {
            msbwt_rle_free(raw_);
            raw_ = o.raw_;
            o.raw_ = nullptr;
        }
        return *this;
    }
    RleBWT(const RleBWT &) = delete;
    RleBWT &operator=(const RleBWT &) = delete;

    void load_vector(const std::vector<std::uint8_t> &bwt) override {
        check(msbwt_rle_load_vector(raw_, bwt.data(), bwt.size()));
    }
    void load_numpy_file(const std::string &filename) override { check(msbwt_rle_load_numpy_file(raw_, filename.c_str())); }
    std::uint64_t get_symbol_count(std::uint8_t symbol) const override {
        if (symbol >= VC_LEN) throw Panic(MSBWT_ERR_INVALID_SYMBOL, "index out of bounds: symbol >= 6");  // :174
        return msbwt_rle_get_symbol_count(raw_, symbol);
    }
    std::uint64_t get_total_size() const override { return msbwt_rle_get_total_size(raw_); }
    BWTRange constrain_range(std::uint8_t sym, const BWTRange &r) const override {
        BWTRange out;
        check(msbwt_rle_constrain_range(raw_, sym, r.l, r.h, &out.l, &out.h));
        return out;
    }
    std::uint64_t count_kmer(const std::vector<std::uint8_t> &kmer) const override {
        std::uint64_t out = 0;
        check(msbwt_rle_count_kmer(raw_, kmer.data(), kmer.size(), &out));
        return out;
    }

    // ---- construction from reads (DynamicBWT::create_from_fastx, src/dynamic_bwt.rs:453-473; naive_bwt's semantics) ----
    /// RLE bytes of the multi-string BWT of the reads: read r is reads[offsets[r] .. offsets[r + 1]), symbol codes 1..5 or, with
    /// `ascii`, text as string_util::convert_stoi maps it.  Built on the GPU; the handle's own index stays as it is.
    std::vector<std::uint8_t> build_from_reads(const std::vector<std::uint8_t> &reads, const std::vector<std::uint64_t> &offsets, bool ascii = false) {
        if (offsets.empty()) return {};
        const std::size_t n = offsets.size() - 1;
        std::vector<std::uint8_t> out(static_cast<std::size_t>(offsets[n] - offsets[0]) + n + 1);
        std::uint64_t len = 0;
        static const std::uint8_t none = 0;
        check(msbwt_rle_build_from_reads(raw_, reads.empty() ? &none : reads.data(), offsets.data(), n, ascii ? 1 : 0, out.data(), out.size(), &len));
        out.resize(static_cast<std::size_t>(len));
        return out;
    }
    /// build_from_reads, then the result loaded as load_vector would load it.
    void load_reads(const std::vector<std::uint8_t> &reads, const std::vector<std::uint64_t> &offsets, bool ascii = false) {
        static const std::uint8_t none = 0;
        static const std::uint64_t zero = 0;
        check(msbwt_rle_load_reads(raw_, reads.empty() ? &none : reads.data(), offsets.empty() ? &zero : offsets.data(), offsets.empty() ? 0 : offsets.size() - 1,
                                   ascii ? 1 : 0));
    }
    /// Most suffixes the builder sorts at once (0 = automatic, from the free HBM); results never depend on it.
    void set_build_piece(std::uint64_t suffixes) { check(msbwt_rle_set_build_piece(raw_, suffixes)); }

    // ---- merge (bwt_util::pairwise_bwt_merge, src/bwt_util.rs:21-141, iterated on the GPU) ----
    /// RLE bytes of the BWT of the union of the read sets behind the BWTs rle0 and rle1; rows of equal rotations: those of rle0
    /// first.  from_second (optional): one bit per merged row, bit i & 7 of byte i >> 3 set = the row came from rle1.
    std::vector<std::uint8_t> merge(const std::vector<std::uint8_t> &rle0, const std::vector<std::uint8_t> &rle1, std::vector<std::uint8_t> *from_second = nullptr) {
        std::vector<std::uint8_t> out(rle0.size() + rle1.size() + 1);
        std::uint64_t len = 0;
        if (from_second) from_second->assign(static_cast<std::size_t>((symbols_of(rle0) + symbols_of(rle1) + 7) / 8) + 1, 0);
        int rc = msbwt_rle_merge(raw_, rle0.data(), rle0.size(), rle1.data(), rle1.size(), out.data(), out.size(), &len, from_second ? from_second->data() : nullptr);
        if (rc == MSBWT_ERR_INVALID_ARG && len > out.size()) {  // inputs that were not canonical
            out.resize(static_cast<std::size_t>(len));
            rc = msbwt_rle_merge(raw_, rle0.data(), rle0.size(), rle1.data(), rle1.size(), out.data(), out.size(), &len, from_second ? from_second->data() : nullptr);
        }
        check(rc);
        out.resize(static_cast<std::size_t>(len));
        return out;
    }
    /// merge, then the result loaded as load_vector would load it.
    void load_merged(const std::vector<std::uint8_t> &rle0, const std::vector<std::uint8_t> &rle1) {
        check(msbwt_rle_load_merged(raw_, rle0.data(), rle0.size(), rle1.data(), rle1.size()));
    }
    /// RLE bytes of the BWT of the union of the read sets behind the BWTs rles (at most MSBWT_MERGE_MAX_INPUTS), merged in one
    /// pass.  sources (optional): one byte per merged row, the index of the BWT the row came from; rows of equal rotations: lower
    /// index first.
    std::vector<std::uint8_t> merge_many(const std::vector<std::vector<std::uint8_t>> &rles, std::vector<std::uint8_t> *sources = nullptr) {
        std::vector<std::uint8_t> flat;
        std::vector<std::uint64_t> offsets(1, 0);
        std::uint64_t symbols = 0;
        for (const auto &r : rles) {
            flat.insert(flat.end(), r.begin(), r.end());
            offsets.push_back(flat.size());
            symbols += symbols_of(r);
        }
        std::vector<std::uint8_t> out(flat.size() + 1);
        std::uint64_t len = 0;
        if (sources) sources->assign(symbols < (1ull << 40) ? static_cast<std::size_t>(symbols) : 0, 0);  // (2^40 and more: the library refuses)
        std::uint8_t *where = sources && !sources->empty() ? sources->data() : nullptr;
        int rc = msbwt_rle_merge_many(raw_, flat.data(), offsets.data(), rles.size(), out.data(), out.size(), &len, where);
        if (rc == MSBWT_ERR_INVALID_ARG && len > out.size()) {  // inputs that were not canonical
            out.resize(static_cast<std::size_t>(len));
            rc = msbwt_rle_merge_many(raw_, flat.data(), offsets.data(), rles.size(), out.data(), out.size(), &len, where);
        }
        check(rc);
        out.resize(static_cast<std::size_t>(len));
        return out;
    }
    /// merge_many, then the result loaded as load_vector would load it.
    void load_merged_many(const std::vector<std::vector<std::uint8_t>> &rles) {
        std::vector<std::uint8_t> flat;
        std::vector<std::uint64_t> offsets(1, 0);
        for (const auto &r : rles) {
            flat.insert(flat.end(), r.begin(), r.end());
            offsets.push_back(flat.size());
        }
        check(msbwt_rle_load_merged_many(raw_, flat.data(), offsets.data(), rles.size()));
    }

    // ---- counts by source: how often a k-mer occurs in each input of a merged BWT ----
    /// Attaches the source vector of a merge (one byte per row of the loaded index: merge_many's `sources`) so that
    /// count_kmers_by_source can answer; n_sources 0 = the largest entry + 1.  clear_sources detaches; every load drops it.
    void set_sources(const std::vector<std::uint8_t> &sources, std::size_t n_sources = 0) {
        static const std::uint8_t none = 0;
        if (!n_sources) {
            for (std::uint8_t s : sources) n_sources = std::max<std::size_t>(n_sources, s);
            n_sources += 1;
        }
        check(msbwt_rle_set_sources(raw_, sources.empty() ? &none : sources.data(), sources.size(), n_sources));
    }
    void clear_sources() { check(msbwt_rle_set_sources(raw_, nullptr, 0, 0)); }
    /// load_merged_many with the merge's own source vector attached (rles.size() sources).
    void load_merged_many_sources(const std::vector<std::vector<std::uint8_t>> &rles) {
        std::vector<std::uint8_t> flat;
        std::vector<std::uint64_t> offsets(1, 0);
        for (const auto &r : rles) {
            flat.insert(flat.end(), r.begin(), r.end());
            offsets.push_back(flat.size());
        }
        check(msbwt_rle_load_merged_many_sources(raw_, flat.data(), offsets.data(), rles.size()));
    }
    std::size_t source_count() const { return static_cast<std::size_t>(msbwt_rle_source_count(raw_)); }
    std::vector<std::uint64_t> source_totals() const {
        std::vector<std::uint64_t> out(source_count());
        if (!out.empty()) check(msbwt_rle_source_totals(raw_, out.data()));
        return out;
    }
    /// n x source_count() row-major: [source_count() i + s] = occurrences of row i (of n x k symbol codes) in input s.
    std::vector<std::uint64_t> count_kmers_by_source(const std::vector<std::uint8_t> &kmers, std::size_t k) const {
        const std::size_t n = k ? kmers.size() / k : 0;
        if (k && kmers.size() % k) throw std::invalid_argument("kmers.size() is not a multiple of k");
        std::vector<std::uint64_t> out(n * source_count() + 1);
        check(msbwt_rle_count_kmers_by_source(raw_, kmers.data(), k, n, out.data()));
        out.resize(n * source_count());
        return out;
    }
    /// The rows of every source inside each range, n x source_count() row-major.
    std::vector<std::uint64_t> range_sources(const std::vector<BWTRange> &ranges) const {
        std::vector<std::uint64_t> l(ranges.size() + 1), h(ranges.size() + 1), out(ranges.size() * source_count() + 1);
        for (std::size_t i = 0; i < ranges.size(); ++i) {
            l[i] = ranges[i].l;
            h[i] = ranges[i].h;
        }
        check(msbwt_rle_range_sources(raw_, l.data(), h.data(), ranges.size(), out.data()));
        out.resize(ranges.size() * source_count());
        return out;
    }
    void count_kmers_by_source_device(const void *d_kmers, std::size_t k, std::size_t n, void *d_out, void *hip_stream) const {
        check(msbwt_rle_count_kmers_by_source_device(raw_, d_kmers, k, n, d_out, hip_stream));
    }
    void range_sources_device(const void *d_l, const void *d_h, std::size_t n, void *d_out, void *hip_stream) const {
        check(msbwt_rle_range_sources_device(raw_, d_l, d_h, n, d_out, hip_stream));
    }
    /// HBM bytes the attachment holds; rows per checkpoint.
    static std::uint64_t source_index_plan(std::uint64_t total_rows, std::size_t n_sources) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_source_index_plan(total_rows, n_sources, &bytes);
        if (rc) throw Panic(rc, "msbwt_source_index_plan");
        return bytes;
    }
    static std::size_t source_block_rows() { return msbwt_source_block_rows(); }
    /// The widest range counted from the source bytes alone, without a checkpoint (tests probe its borders).
    static std::size_t source_narrow_rows() { return msbwt_source_narrow_rows(); }

    // ---- spectrum and enumeration: the k-mers the index holds, 1 <= k <= 32 ----
    /// What kmer_spectrum returns: hist[c] = distinct k-mers that occur exactly c times (the last bin: that often or more).
    struct Spectrum {
        std::vector<std::uint64_t> hist;
        std::uint64_t distinct = 0, occurrences = 0;
    };
    /// What enumerate_kmers returns: record i is the k-mer words[i] (the 2-bit word of msbwt_kmers_pack_2bit), which occurs counts[i]
    /// times in rows [l[i], l[i] + counts[i]).
    struct Kmers {
        std::vector<std::uint64_t> words, counts, l;
    };
    Spectrum kmer_spectrum(std::size_t k, std::size_t bins = 256) const {
        Spectrum s;
        s.hist.assign(bins, 0);
        check(msbwt_rle_kmer_spectrum(raw_, k, s.hist.data(), bins, &s.distinct, &s.occurrences));
        return s;
    }
    /// The k-mers with min_count <= count <= max_count (0: no upper limit), ascending when `sorted`: both calls of the two-call pattern.
    Kmers enumerate_kmers(std::size_t k, std::uint64_t min_count = 1, std::uint64_t max_count = 0, bool sorted = true) const {
        Kmers out;
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_kmers(raw_, k, min_count, max_count, sorted ? 1 : 0, nullptr, nullptr, nullptr, 0, &n));
        out.words.resize(static_cast<std::size_t>(n));
        out.counts.resize(out.words.size());
        out.l.resize(out.words.size());
        if (n) check(msbwt_rle_enumerate_kmers(raw_, k, min_count, max_count, sorted ? 1 : 0, out.words.data(), out.counts.data(), out.l.data(), n, &n));
        return out;
    }
    /// Device buffers of `capacity` u64 each (d_counts, d_l may be null) -> the number of k-mers that qualify; capacity 0 only counts.
    std::uint64_t enumerate_kmers_device(std::size_t k, std::uint64_t min_count, std::uint64_t max_count, bool sorted, void *d_words, void *d_counts, void *d_l,
                                         std::uint64_t capacity, void *hip_stream) const {
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_kmers_device(raw_, k, min_count, max_count, sorted ? 1 : 0, d_words, d_counts, d_l, capacity, &n, hip_stream));
        return n;
    }
    /// Most nodes per frontier buffer of the walks (0 = automatic, else at least MSBWT_SPECTRUM_MIN_FRONTIER); results never depend on it.
    void set_spectrum_frontier(std::uint64_t nodes) { check(msbwt_rle_set_spectrum_frontier(raw_, nodes)); }
    /// The MSBWT_SPECTRUM_INFO_WORDS words of msbwt_rle_spectrum_info (include/msbwt_hip.h names them).
    std::vector<std::uint64_t> spectrum_info() const {
        std::vector<std::uint64_t> out(MSBWT_SPECTRUM_INFO_WORDS);
        check(msbwt_rle_spectrum_info(raw_, out.data()));
        return out;
    }
    /// HBM bytes a walk allocates (and frees again) with the automatic frontier.
    static std::uint64_t spectrum_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::uint64_t records = 0, bool sorted = false) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_spectrum_plan(total_rows, free_hbm_bytes, records, sorted ? 1 : 0, &bytes);
        if (rc) throw Panic(rc, "msbwt_spectrum_plan");
        return bytes;
    }
    // ---- canonical k-mers: a k-mer and its reverse complement as one class (include/msbwt_hip.h has the definitions) ----
    /// What enumerate_canonical_kmers returns: class i has the canonical word words[i], which occurs own[i] times, and its reverse
    /// complement other[i] times (0 for a palindrome); the class count is own[i] + other[i].  In the order the walk produces them.
    struct CanonicalKmers {
        std::vector<std::uint64_t> words, own, other;
    };
    /// The spectrum over the classes: hist[min(own + other, bins - 1)], the number of classes, the sum of their counts.
    Spectrum canonical_kmer_spectrum(std::size_t k, std::size_t bins = 256) const {
        Spectrum s;
        s.hist.assign(bins, 0);
        check(msbwt_rle_canonical_kmer_spectrum(raw_, k, s.hist.data(), bins, &s.distinct, &s.occurrences));
        return s;
    }
    /// The classes with min_count <= own + other <= max_count (0: no upper limit): both calls of the two-call pattern.
    CanonicalKmers enumerate_canonical_kmers(std::size_t k, std::uint64_t min_count = 1, std::uint64_t max_count = 0) const {
        CanonicalKmers out;
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_canonical_kmers(raw_, k, min_count, max_count, nullptr, nullptr, nullptr, 0, &n));
        out.words.resize(static_cast<std::size_t>(n));
        out.own.resize(out.words.size());
        out.other.resize(out.words.size());
        if (n) check(msbwt_rle_enumerate_canonical_kmers(raw_, k, min_count, max_count, out.words.data(), out.own.data(), out.other.data(), n, &n));
        return out;
    }
    /// Packed reverse complements of packed k-mers, 1 <= k <= 32 (pure host function).
    static std::vector<std::uint64_t> reverse_complement_2bit(const std::vector<std::uint64_t> &words, std::size_t k) {
        std::vector<std::uint64_t> out(words.size());
        const int rc = msbwt_kmers_reverse_complement_2bit(words.data(), k, words.size(), out.data());
        if (rc) throw Panic(rc, "msbwt_kmers_reverse_complement_2bit");
        return out;
    }
    /// HBM bytes a canonical call allocates (and frees again) with the automatic frontier.
    static std::uint64_t canonical_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::uint64_t records = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_canonical_plan(total_rows, free_hbm_bytes, records, &bytes);
        if (rc) throw Panic(rc, "msbwt_canonical_plan");
        return bytes;
    }
    // ---- k-mers by source: one spectrum per input of a merged index, the dump filtered by per-source counts (sources attached) ----
    /// What kmer_spectrum_by_source returns: hist[s * bins + c] = k-mers of the index that input s holds exactly c times (the last bin:
    /// that often or more; bin 0: not at all), sharing[j] = k-mers held by exactly j inputs, per input the k-mers it holds and their occurrences.
    struct SourceSpectrum {
        std::size_t sources = 0, bins = 0;
        std::vector<std::uint64_t> hist, sharing, distinct, occurrences;
    };
    /// What enumerate_kmers_by_source returns: k-mer words[i] occurs counts[i * sources + s] times in input s, in rows from l[i] on.
    struct SourceKmers {
        std::size_t sources = 0;
        std::vector<std::uint64_t> words, counts, l;
    };
    /// "No upper limit" in max_counts; 0 there means ABSENT from that input.
    static constexpr std::uint64_t kNoLimit = ~std::uint64_t(0);
    SourceSpectrum kmer_spectrum_by_source(std::size_t k, std::size_t bins = 256) const {
        SourceSpectrum s;
        s.sources = static_cast<std::size_t>(msbwt_rle_source_count(raw_));
        s.bins = bins;
        s.hist.assign(std::max<std::size_t>(s.sources, 1) * bins, 0);
        s.sharing.assign(s.sources + 1, 0);
        s.distinct.assign(std::max<std::size_t>(s.sources, 1), 0);
        s.occurrences.assign(std::max<std::size_t>(s.sources, 1), 0);
        check(msbwt_rle_kmer_spectrum_by_source(raw_, k, s.hist.data(), bins, s.sharing.data(), s.distinct.data(), s.occurrences.data()));
        return s;
    }
    /// The k-mers with min_counts[s] <= c_s <= max_counts[s] for every input s (empty vectors: zeros / no limits) and min_total <= sum <=
    /// max_total (0: no upper limit), ascending when `sorted`: both calls of the two-call pattern.
    SourceKmers enumerate_kmers_by_source(std::size_t k, const std::vector<std::uint64_t> &min_counts, const std::vector<std::uint64_t> &max_counts,
                                          std::uint64_t min_total = 1, std::uint64_t max_total = 0, bool sorted = true) const {
        SourceKmers out;
        out.sources = static_cast<std::size_t>(msbwt_rle_source_count(raw_));
        if ((!min_counts.empty() && min_counts.size() != out.sources) || (!max_counts.empty() && max_counts.size() != out.sources))
            throw Panic(MSBWT_ERR_INVALID_ARG, "enumerate_kmers_by_source: one limit per source");
        const std::uint64_t *lo = min_counts.empty() ? nullptr : min_counts.data(), *hi = max_counts.empty() ? nullptr : max_counts.data();
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_kmers_by_source(raw_, k, lo, hi, min_total, max_total, sorted ? 1 : 0, nullptr, nullptr, nullptr, 0, &n));
        out.words.resize(static_cast<std::size_t>(n));
        out.counts.resize(out.words.size() * out.sources);
        out.l.resize(out.words.size());
        if (n) check(msbwt_rle_enumerate_kmers_by_source(raw_, k, lo, hi, min_total, max_total, sorted ? 1 : 0, out.words.data(), out.counts.data(), out.l.data(), n, &n));
        return out;
    }
    /// Device buffers (d_counts: capacity x sources u64; d_counts, d_l may be null) -> the number of k-mers that qualify; capacity 0 only
    /// counts.  The limits are host arrays (null: zeros / no limits).
    std::uint64_t enumerate_kmers_by_source_device(std::size_t k, const std::uint64_t *min_counts, const std::uint64_t *max_counts, std::uint64_t min_total,
                                                   std::uint64_t max_total, bool sorted, void *d_words, void *d_counts, void *d_l, std::uint64_t capacity,
                                                   void *hip_stream) const {
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_kmers_by_source_device(raw_, k, min_counts, max_counts, min_total, max_total, sorted ? 1 : 0, d_words, d_counts, d_l, capacity, &n,
                                                         hip_stream));
        return n;
    }
    /// What enumerate_kmer_graph returns: the k-mers that occur often enough, ascending, with one edge byte each -- bit j (A C G T ->
    /// 0..3): the (k+1)-mer j.q is an edge (a predecessor), bit 4 + j: q.j is one (a successor).
    struct KmerGraph {
        std::vector<std::uint64_t> words, counts, l;
        std::vector<std::uint8_t> edges;
    };
    /// What kmer_graph_degrees returns: table[5 * i + o] = the k-mers with i predecessors and o successors.
    struct GraphDegrees {
        std::uint64_t table[25] = {};
        std::uint64_t nodes = 0, edges = 0;
    };
    /// Nodes: the k-mers with count >= max(min_count, 1); edges: the (k+1)-mers with count >= min_edge (0: the node threshold).
    KmerGraph enumerate_kmer_graph(std::size_t k, std::uint64_t min_count = 1, std::uint64_t min_edge = 0) const {
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_kmer_graph(raw_, k, min_count, min_edge, nullptr, nullptr, nullptr, nullptr, 0, &n));
        KmerGraph g;
        g.words.resize(n);
        g.counts.resize(n);
        g.l.resize(n);
        g.edges.resize(n);
        if (n) check(msbwt_rle_enumerate_kmer_graph(raw_, k, min_count, min_edge, g.words.data(), g.counts.data(), g.l.data(), g.edges.data(), n, &n));
        return g;
    }
    /// Device buffers (each may be null; d_edges: bytes, any alignment) -> the number of k-mers that qualify; capacity 0 only counts.
    std::uint64_t enumerate_kmer_graph_device(std::size_t k, std::uint64_t min_count, std::uint64_t min_edge, void *d_words, void *d_counts, void *d_l, void *d_edges,
                                              std::uint64_t capacity, void *hip_stream) const {
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_kmer_graph_device(raw_, k, min_count, min_edge, d_words, d_counts, d_l, d_edges, capacity, &n, hip_stream));
        return n;
    }
    GraphDegrees kmer_graph_degrees(std::size_t k, std::uint64_t min_count = 1, std::uint64_t min_edge = 0) const {
        GraphDegrees d;
        check(msbwt_rle_kmer_graph_degrees(raw_, k, min_count, min_edge, d.table, &d.nodes, &d.edges));
        return d;
    }
    /// HBM bytes a host graph dump of `records` nodes allocates (and frees again) with the automatic frontier.
    static std::uint64_t kmer_graph_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::uint64_t records = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_kmer_graph_plan(total_rows, free_hbm_bytes, records, &bytes);
        if (rc) throw Panic(rc, "msbwt_kmer_graph_plan");
        return bytes;
    }
    /// What enumerate_unitigs returns: unitig u is symbols[offsets[u] .. offsets[u + 1]) in symbol codes (A C G T = 1 2 3 5), ascending
    /// by first k-mer; count_sums[u] = the sum of its nodes' counts; ends[u]: low nibble = predecessor bits of its first node, high
    /// nibble = successor bits of its last; flags[u] bit 0 = circular.
    struct Unitigs {
        std::vector<std::uint8_t> symbols;
        std::vector<std::uint64_t> offsets, count_sums;
        std::vector<std::uint8_t> ends, flags;
        std::size_t size() const { return count_sums.size(); }
    };
    /// The non-branching paths of the k-mer graph (nodes: count >= max(min_count, 1); edges: count >= min_edge, 0: the node threshold).
    Unitigs enumerate_unitigs(std::size_t k, std::uint64_t min_count = 1, std::uint64_t min_edge = 0) const {
        std::uint64_t n = 0, s = 0;
        check(msbwt_rle_enumerate_unitigs(raw_, k, min_count, min_edge, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, &n, &s));
        Unitigs u;
        u.symbols.resize(s);
        u.offsets.resize(n + 1);
        u.count_sums.resize(n);
        u.ends.resize(n);
        u.flags.resize(n);
        if (n)
            check(msbwt_rle_enumerate_unitigs(raw_, k, min_count, min_edge, u.symbols.data(), u.offsets.data(), u.count_sums.data(), u.ends.data(), u.flags.data(), n, s,
                                              &n, &s));
        return u;
    }
    /// Device buffers (each may be null; the byte arrays at any alignment) -> the unitigs; *symbol_total (may be null) = their symbols.
    /// Both capacities 0 only counts.
    std::uint64_t enumerate_unitigs_device(std::size_t k, std::uint64_t min_count, std::uint64_t min_edge, void *d_symbols, void *d_offsets, void *d_count_sums,
                                           void *d_ends, void *d_flags, std::uint64_t capacity_unitigs, std::uint64_t capacity_symbols, std::uint64_t *symbol_total,
                                           void *hip_stream) const {
        std::uint64_t n = 0;
        check(msbwt_rle_enumerate_unitigs_device(raw_, k, min_count, min_edge, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, capacity_unitigs, capacity_symbols,
                                                 &n, symbol_total, hip_stream));
        return n;
    }
    /// The last unitig call: nodes, edges, links, unitigs, symbols, circular unitigs, nodes of the longest unitig, jumping rounds.
    struct UnitigInfo {
        std::uint64_t nodes = 0, edges = 0, links = 0, unitigs = 0, symbols = 0, circular = 0, longest = 0, rounds = 0;
    };
    UnitigInfo unitig_info() const {
        std::uint64_t w[MSBWT_UNITIG_INFO_WORDS] = {};
        check(msbwt_rle_unitig_info(raw_, w));
        UnitigInfo i;
        i.nodes = w[0], i.edges = w[1], i.links = w[2], i.unitigs = w[3], i.symbols = w[4], i.circular = w[5], i.longest = w[6], i.rounds = w[7];
        return i;
    }
    /// HBM bytes a host unitig call over `nodes` nodes that fills every buffer allocates (and frees again) with the automatic frontier;
    /// unitigs = symbols = 0: the counting call.
    static std::uint64_t unitigs_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::uint64_t nodes = 0, std::uint64_t unitigs = 0,
                                      std::uint64_t symbols = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_unitigs_plan(total_rows, free_hbm_bytes, nodes, unitigs, symbols, &bytes);
        if (rc) throw Panic(rc, "msbwt_unitigs_plan");
        return bytes;
    }

    /// Canonical unitigs: the unitigs of the strand-merged graph (1 <= k <= 31), every class {q, rc(q)} in exactly one of them once; of a
    /// unitig and its mirror the one with the smaller first k-mer.  count_sums: sums of class counts.
    Unitigs enumerate_canonical_unitigs(std::size_t k, std::uint64_t min_count = 1, std::uint64_t min_edge = 0) const {
        std::uint64_t n = 0, s = 0;
        check(msbwt_rle_enumerate_canonical_unitigs(raw_, k, min_count, min_edge, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, &n, &s));
        Unitigs u;
        u.symbols.resize(s);
        u.offsets.resize(n + 1);
        u.count_sums.resize(n);
        u.ends.resize(n);
        u.flags.resize(n);
        if (n)
            check(msbwt_rle_enumerate_canonical_unitigs(raw_, k, min_count, min_edge, u.symbols.data(), u.offsets.data(), u.count_sums.data(), u.ends.data(),
                                                        u.flags.data(), n, s, &n, &s));
        return u;
    }
    /// Device buffers (each may be null; the byte arrays at any alignment) -> the unitigs; *symbol_total (may be null) = their symbols.
    std::uint64_t enumerate_canonical_unitigs_device(std::size_t k, std::uint64_t min_count, std::uint64_t min_edge, void *d_symbols, void *d_offsets,
                                                     void *d_count_sums, void *d_ends, void *d_flags, std::uint64_t capacity_unitigs,
                                                     std::uint64_t capacity_symbols, std::uint64_t *symbol_total, void *hip_stream = nullptr) const {
        std::uint64_t n = 0, s = 0;
        check(msbwt_rle_enumerate_canonical_unitigs_device(raw_, k, min_count, min_edge, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, capacity_unitigs,
                                                           capacity_symbols, &n, &s, hip_stream));
        if (symbol_total) *symbol_total = s;
        return n;
    }
    /// The last canonical unitig call, for the emitted set.
    struct CanonicalUnitigInfo {
        std::uint64_t classes = 0, edge_classes = 0, links = 0, unitigs = 0, symbols = 0, circular = 0, longest = 0, rounds = 0, palindromes = 0, cut_links = 0;
    };
    CanonicalUnitigInfo canonical_unitig_info() const {
        std::uint64_t w[MSBWT_CANONICAL_UNITIG_INFO_WORDS] = {};
        check(msbwt_rle_canonical_unitig_info(raw_, w));
        CanonicalUnitigInfo i;
        i.classes = w[0], i.edge_classes = w[1], i.links = w[2], i.unitigs = w[3], i.symbols = w[4], i.circular = w[5], i.longest = w[6], i.rounds = w[7];
        i.palindromes = w[8], i.cut_links = w[9];
        return i;
    }
    /// HBM bytes a host canonical unitig call over `classes` classes that fills every buffer allocates (and frees again).
    static std::uint64_t canonical_unitigs_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::uint64_t classes = 0, std::uint64_t unitigs = 0,
                                                std::uint64_t symbols = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_canonical_unitigs_plan(total_rows, free_hbm_bytes, classes, unitigs, symbols, &bytes);
        if (rc) throw Panic(rc, "msbwt_canonical_unitigs_plan");
        return bytes;
    }
    /// What enumerate_unitig_graph returns: the unitigs and the link table of the compacted graph.  Side 2u leaves unitig u forwards,
    /// side 2u + 1 leaves its reverse complement forwards; side a holds link_targets[link_offsets[a] .. link_offsets[a + 1]), an
    /// entry 2v + o per edge: it reaches the first node of v (o = 0) or the reverse complement of its last node (o = 1).  Canonical:
    /// flags[u] bit 1 = the unitig is its own reverse complement and has one side.
    struct UnitigGraph : Unitigs {
        std::vector<std::uint64_t> link_offsets, link_targets;
    };
    /// Either unitig call with the link table behind its columns (canonical: the strand-merged graph, 1 <= k <= 31).
    UnitigGraph enumerate_unitig_graph(std::size_t k, std::uint64_t min_count = 1, std::uint64_t min_edge = 0, bool canonical = false) const {
        const auto call = canonical ? msbwt_rle_enumerate_canonical_unitig_graph : msbwt_rle_enumerate_unitig_graph;
        std::uint64_t n = 0, s = 0, l = 0;
        check(call(raw_, k, min_count, min_edge, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, &n, &s, &l));
        UnitigGraph u;
        u.symbols.resize(s);
        u.offsets.resize(n + 1);
        u.count_sums.resize(n);
        u.ends.resize(n);
        u.flags.resize(n);
        u.link_offsets.resize(2 * n + 1);
        u.link_targets.resize(l);
        if (n)
            check(call(raw_, k, min_count, min_edge, u.symbols.data(), u.offsets.data(), u.count_sums.data(), u.ends.data(), u.flags.data(), u.link_offsets.data(),
                       u.link_targets.data(), n, s, l, &n, &s, &l));
        return u;
    }
    /// Device buffers (each may be null; the byte arrays at any alignment) -> the unitigs; *symbol_total and *links (each may be null)
    /// = their symbols and link entries.  All three capacities 0 only counts.
    std::uint64_t enumerate_unitig_graph_device(std::size_t k, std::uint64_t min_count, std::uint64_t min_edge, bool canonical, void *d_symbols, void *d_offsets,
                                                void *d_count_sums, void *d_ends, void *d_flags, void *d_link_offsets, void *d_link_targets,
                                                std::uint64_t capacity_unitigs, std::uint64_t capacity_symbols, std::uint64_t capacity_links,
                                                std::uint64_t *symbol_total, std::uint64_t *links, void *hip_stream = nullptr) const {
        const auto call = canonical ? msbwt_rle_enumerate_canonical_unitig_graph_device : msbwt_rle_enumerate_unitig_graph_device;
        std::uint64_t n = 0;
        check(call(raw_, k, min_count, min_edge, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, capacity_unitigs, capacity_symbols,
                   capacity_links, &n, symbol_total, links, hip_stream));
        return n;
    }
    /// HBM bytes a host unitig graph call that fills every buffer allocates (and frees again): the unitig call's plan and the link table;
    /// unitigs = symbols = links = 0: the counting call.
    static std::uint64_t unitig_graph_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::uint64_t nodes = 0, std::uint64_t unitigs = 0,
                                           std::uint64_t symbols = 0, std::uint64_t links = 0, bool canonical = false) {
        std::uint64_t bytes = 0;
        const int rc = (canonical ? msbwt_canonical_unitig_graph_plan : msbwt_unitig_graph_plan)(total_rows, free_hbm_bytes, nodes, unitigs, symbols, links, &bytes);
        if (rc) throw Panic(rc, canonical ? "msbwt_canonical_unitig_graph_plan" : "msbwt_unitig_graph_plan");
        return bytes;
    }
    /// What enumerate_unitig_graph_by_source returns: the unitig graph and, per unitig and per input of the merged index, the rows of
    /// that input in the ranges of the unitig's nodes (canonical: of both members of its classes, a palindrome once):
    /// source_sums[u * sources + s]; row u sums to count_sums[u].
    struct UnitigGraphBySource : UnitigGraph {
        std::vector<std::uint64_t> source_sums;
        std::size_t sources = 0;
    };
    /// Either unitig graph call with the matrix by source behind the link table, on an index with sources attached.
    UnitigGraphBySource enumerate_unitig_graph_by_source(std::size_t k, std::uint64_t min_count = 1, std::uint64_t min_edge = 0, bool canonical = false) const {
        const auto call = canonical ? msbwt_rle_enumerate_canonical_unitig_graph_by_source : msbwt_rle_enumerate_unitig_graph_by_source;
        std::uint64_t n = 0, s = 0, l = 0;
        check(call(raw_, k, min_count, min_edge, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, &n, &s, &l));
        UnitigGraphBySource u;
        u.sources = std::size_t(msbwt_rle_source_count(raw_));
        u.symbols.resize(s);
        u.offsets.resize(n + 1);
        u.count_sums.resize(n);
        u.ends.resize(n);
        u.flags.resize(n);
        u.link_offsets.resize(2 * n + 1);
        u.link_targets.resize(l);
        u.source_sums.resize(n * u.sources);
        if (n)
            check(call(raw_, k, min_count, min_edge, u.symbols.data(), u.offsets.data(), u.count_sums.data(), u.ends.data(), u.flags.data(), u.link_offsets.data(),
                       u.link_targets.data(), u.source_sums.data(), n, s, l, &n, &s, &l));
        return u;
    }
    /// Device buffers (each may be null; d_source_sums: capacity_unitigs x sources words) -> the unitigs, as enumerate_unitig_graph_device.
    std::uint64_t enumerate_unitig_graph_by_source_device(std::size_t k, std::uint64_t min_count, std::uint64_t min_edge, bool canonical, void *d_symbols, void *d_offsets,
                                                          void *d_count_sums, void *d_ends, void *d_flags, void *d_link_offsets, void *d_link_targets,
                                                          void *d_source_sums, std::uint64_t capacity_unitigs, std::uint64_t capacity_symbols,
                                                          std::uint64_t capacity_links, std::uint64_t *symbol_total, std::uint64_t *links,
                                                          void *hip_stream = nullptr) const {
        const auto call = canonical ? msbwt_rle_enumerate_canonical_unitig_graph_by_source_device : msbwt_rle_enumerate_unitig_graph_by_source_device;
        std::uint64_t n = 0;
        check(call(raw_, k, min_count, min_edge, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, d_source_sums, capacity_unitigs,
                   capacity_symbols, capacity_links, &n, symbol_total, links, hip_stream));
        return n;
    }
    /// HBM bytes a host unitig graph call by source that fills every buffer allocates (and frees again): the graph call's plan, the
    /// range words and the staged matrix; unitigs = symbols = links = 0: the counting call.
    static std::uint64_t unitig_graph_by_source_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::uint64_t nodes, std::uint64_t unitigs,
                                                     std::uint64_t symbols, std::uint64_t links, std::size_t n_sources, bool canonical = false) {
        std::uint64_t bytes = 0;
        const int rc = (canonical ? msbwt_canonical_unitig_graph_by_source_plan : msbwt_unitig_graph_by_source_plan)(total_rows, free_hbm_bytes, nodes, unitigs, symbols,
                                                                                                                     links, n_sources, &bytes);
        if (rc) throw Panic(rc, canonical ? "msbwt_canonical_unitig_graph_by_source_plan" : "msbwt_unitig_graph_by_source_plan");
        return bytes;
    }
    /// What trace_kmers returns: row i of symbols (n rows of max_steps bytes) holds steps[i] symbol codes (A C G T = 1 2 3 5) and zeros
    /// behind them; stops[i] is MSBWT_TRACE_DEAD_END .. MSBWT_TRACE_NOT_A_NODE; last[i] the node the walk ended on; bit j of fans[i] = the
    /// edge by symbol j leaves that node in the walk direction.
    struct Traces {
        std::vector<std::uint8_t> symbols;
        std::vector<std::uint64_t> steps;
        std::vector<std::uint8_t> stops;
        std::vector<std::uint64_t> edge_sums, last;
        std::vector<std::uint8_t> fans;
        std::uint64_t max_steps = 0;
        std::size_t size() const { return steps.size(); }
    };
    /// Traces (msbwt_hip.h, "traces"): from each packed seed k-mer (1 <= k <= 31) a walk through the k-mer graph, node by node, under
    /// `mode` (MSBWT_TRACE_UNIQUE, _UNITIG, _GREEDY) in `direction` (MSBWT_TRACE_RIGHT, _LEFT), max_steps steps at the most; targets:
    /// one a seed, or empty.
    Traces trace_kmers(const std::vector<std::uint64_t> &seeds, std::size_t k, std::uint64_t max_steps, int mode = MSBWT_TRACE_UNIQUE, int direction = MSBWT_TRACE_RIGHT,
                       std::uint64_t min_count = 1, std::uint64_t min_edge = 0, const std::vector<std::uint64_t> &targets = {}) const {
        if (!targets.empty() && targets.size() != seeds.size()) throw Panic(MSBWT_ERR_INVALID_ARG, "trace_kmers: one target a seed");
        const std::size_t n = seeds.size();
        Traces t;
        t.max_steps = max_steps;
        t.symbols.resize(n * max_steps);
        t.steps.resize(n);
        t.stops.resize(n);
        t.edge_sums.resize(n);
        t.last.resize(n);
        t.fans.resize(n);
        check(msbwt_rle_trace_kmers(raw_, seeds.data(), targets.empty() ? nullptr : targets.data(), k, n, min_count, min_edge, mode, direction, max_steps, t.symbols.data(),
                                    t.steps.data(), t.stops.data(), t.edge_sums.data(), t.last.data(), t.fans.data()));
        return t;
    }
    /// Device buffers (every output and d_targets may be null; the byte arrays at any alignment); synchronises hip_stream.
    void trace_kmers_device(const void *d_seeds, const void *d_targets, std::size_t k, std::size_t n, std::uint64_t min_count, std::uint64_t min_edge, int mode,
                            int direction, std::uint64_t max_steps, void *d_symbols, void *d_steps, void *d_stops, void *d_edge_sums, void *d_last, void *d_fans,
                            void *hip_stream = nullptr) const {
        check(msbwt_rle_trace_kmers_device(raw_, d_seeds, d_targets, k, n, min_count, min_edge, mode, direction, max_steps, d_symbols, d_steps, d_stops, d_edge_sums, d_last,
                                           d_fans, hip_stream));
    }
    /// The last trace call.
    struct TraceInfo {
        std::uint64_t walks = 0, rounds = 0, queries = 0, steps = 0, longest = 0, pieces = 0, scratch_bytes = 0, not_nodes = 0;
    };
    TraceInfo trace_info() const {
        std::uint64_t w[MSBWT_TRACE_INFO_WORDS] = {};
        check(msbwt_rle_trace_info(raw_, w));
        TraceInfo i;
        i.walks = w[0], i.rounds = w[1], i.queries = w[2], i.steps = w[3], i.longest = w[4], i.pieces = w[5], i.scratch_bytes = w[6], i.not_nodes = w[7];
        return i;
    }
    /// Most walks a trace call advances at once (0 = automatic, 2^20); results never depend on it.
    void set_trace_piece(std::uint64_t walks) { check(msbwt_rle_set_trace_piece(raw_, walks)); }
    /// HBM bytes of scratch a trace call of n walks allocates (and frees again) on an index that holds something.
    static std::uint64_t trace_plan(std::uint64_t n, std::uint64_t max_steps, int mode = MSBWT_TRACE_UNIQUE, bool targets = false, bool host = true,
                                    std::uint64_t piece = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_trace_plan(n, max_steps, mode, targets ? 1 : 0, host ? 1 : 0, piece, &bytes);
        if (rc) throw Panic(rc, "msbwt_trace_plan");
        return bytes;
    }
    /// Canonical traces (msbwt_hip.h, "canonical traces"): trace_kmers through the strand-merged graph of the canonical unitigs -- a k-mer
    /// counts with its reverse complement, edge_sums sums class counts, last is the word in the walk's orientation, and MSBWT_TRACE_UNITIG
    /// stops MSBWT_CANONICAL_TRACE_MIRROR where the link chosen is one of the canonical unitigs' cuts.
    Traces trace_canonical_kmers(const std::vector<std::uint64_t> &seeds, std::size_t k, std::uint64_t max_steps, int mode = MSBWT_TRACE_UNIQUE,
                                 int direction = MSBWT_TRACE_RIGHT, std::uint64_t min_count = 1, std::uint64_t min_edge = 0,
                                 const std::vector<std::uint64_t> &targets = {}) const {
        if (!targets.empty() && targets.size() != seeds.size()) throw Panic(MSBWT_ERR_INVALID_ARG, "trace_canonical_kmers: one target a seed");
        const std::size_t n = seeds.size();
        Traces t;
        t.max_steps = max_steps;
        t.symbols.resize(n * max_steps);
        t.steps.resize(n);
        t.stops.resize(n);
        t.edge_sums.resize(n);
        t.last.resize(n);
        t.fans.resize(n);
        check(msbwt_rle_trace_canonical_kmers(raw_, seeds.data(), targets.empty() ? nullptr : targets.data(), k, n, min_count, min_edge, mode, direction, max_steps,
                                              t.symbols.data(), t.steps.data(), t.stops.data(), t.edge_sums.data(), t.last.data(), t.fans.data()));
        return t;
    }
    /// Device buffers, as trace_kmers_device.
    void trace_canonical_kmers_device(const void *d_seeds, const void *d_targets, std::size_t k, std::size_t n, std::uint64_t min_count, std::uint64_t min_edge, int mode,
                                      int direction, std::uint64_t max_steps, void *d_symbols, void *d_steps, void *d_stops, void *d_edge_sums, void *d_last, void *d_fans,
                                      void *hip_stream = nullptr) const {
        check(msbwt_rle_trace_canonical_kmers_device(raw_, d_seeds, d_targets, k, n, min_count, min_edge, mode, direction, max_steps, d_symbols, d_steps, d_stops,
                                                     d_edge_sums, d_last, d_fans, hip_stream));
    }
    /// The last canonical trace call.
    TraceInfo canonical_trace_info() const {
        std::uint64_t w[MSBWT_CANONICAL_TRACE_INFO_WORDS] = {};
        check(msbwt_rle_canonical_trace_info(raw_, w));
        TraceInfo i;
        i.walks = w[0], i.rounds = w[1], i.queries = w[2], i.steps = w[3], i.longest = w[4], i.pieces = w[5], i.scratch_bytes = w[6], i.not_nodes = w[7];
        return i;
    }
    /// HBM bytes of scratch a canonical trace call of n walks allocates (and frees again) on an index that holds something.
    static std::uint64_t canonical_trace_plan(std::uint64_t n, std::uint64_t max_steps, int mode = MSBWT_TRACE_UNIQUE, bool targets = false, bool host = true,
                                              std::uint64_t piece = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_canonical_trace_plan(n, max_steps, mode, targets ? 1 : 0, host ? 1 : 0, piece, &bytes);
        if (rc) throw Panic(rc, "msbwt_canonical_trace_plan");
        return bytes;
    }
    /// What walk_rows returns: row i of symbols (n rows of max_steps bytes, empty for a locate) holds steps[i] symbol codes 1..5 in WALK
    /// order -- the last symbol of the prefix first -- and zeros behind them; stops[i] is MSBWT_WALK_DOLLAR, _MAX_STEPS or _BAD_ROW;
    /// last[i] the row the walk stands on; reads[i] the read for a DOLLAR stop (steps[i] is then the offset in it), else UINT64_MAX.
    struct Walks {
        std::vector<std::uint8_t> symbols;
        std::vector<std::uint64_t> steps;
        std::vector<std::uint8_t> stops;
        std::vector<std::uint64_t> last, reads;
        std::uint64_t max_steps = 0;
        std::size_t size() const { return steps.size(); }
        /// the prefix walk i went through, in reading order
        std::vector<std::uint8_t> sequence(std::size_t i) const {
            const std::uint8_t *row = symbols.data() + i * max_steps;
            return std::vector<std::uint8_t>(std::make_reverse_iterator(row + steps[i]), std::make_reverse_iterator(row));
        }
    };
    /// Left walks (msbwt_hip.h, "left walks"): from each BWT row the LF walk back through the text until it stands on a '$' or has
    /// taken max_steps steps.  with_symbols = false: locate.  A row at or beyond the total size panics with MSBWT_ERR_INVALID_RANGE.
    Walks walk_rows(const std::vector<std::uint64_t> &rows, std::uint64_t max_steps, bool with_symbols = true) const {
        const std::size_t n = rows.size();
        Walks w;
        w.max_steps = max_steps;
        if (with_symbols) w.symbols.resize(n * max_steps);
        w.steps.resize(n);
        w.stops.resize(n);
        w.last.resize(n);
        w.reads.resize(n);
        check(msbwt_rle_walk_rows(raw_, rows.data(), n, max_steps, with_symbols ? w.symbols.data() : nullptr, w.steps.data(), w.stops.data(), w.last.data(), w.reads.data()));
        return w;
    }
    /// walk_rows without symbols: reads[i] and steps[i] are the read and the offset of row i where stops[i] == MSBWT_WALK_DOLLAR.
    Walks locate_rows(const std::vector<std::uint64_t> &rows, std::uint64_t max_steps) const { return walk_rows(rows, max_steps, false); }
    /// Device buffers (every output may be null; the rows of symbols at any alignment); synchronises hip_stream.
    void walk_rows_device(const void *d_rows, std::size_t n, std::uint64_t max_steps, void *d_symbols, void *d_steps, void *d_stops, void *d_last, void *d_reads,
                          void *hip_stream = nullptr) const {
        check(msbwt_rle_walk_rows_device(raw_, d_rows, n, max_steps, d_symbols, d_steps, d_stops, d_last, d_reads, hip_stream));
    }
    /// What extract_reads returns: read j = symbols[offsets[j] .. offsets[j + 1]) in reading order; truncated = the reads longer than
    /// max_len, which come as their last max_len symbols.
    struct Reads {
        std::vector<std::uint8_t> symbols;
        std::vector<std::uint64_t> offsets;
        std::uint64_t truncated = 0;
        std::size_t size() const { return offsets.empty() ? 0 : offsets.size() - 1; }
    };
    /// The reads `ids` (each below get_symbol_count(0); read i is the i-th of the sorted read set), or, ids empty, the n reads from
    /// first_read on, as a ragged set in reading order.  One walk: the buffer holds n x max_len symbols before it shrinks.
    Reads extract_reads(const std::vector<std::uint64_t> &ids, std::uint64_t first_read, std::size_t n, std::uint64_t max_len) const {
        if (!ids.empty()) n = ids.size();
        Reads r;
        r.symbols.resize(std::max<std::size_t>(n * max_len, 1));
        r.offsets.resize(n + 1);
        std::uint64_t total = 0;
        check(msbwt_rle_extract_reads(raw_, ids.empty() ? nullptr : ids.data(), first_read, n, max_len, r.symbols.data(), r.offsets.data(), n * max_len, &total,
                                      &r.truncated));
        r.symbols.resize(total);
        return r;
    }
    /// Device buffers (d_ids, d_symbols and d_offsets may each be null) -> S, the symbols of the reads; synchronises hip_stream.
    std::uint64_t extract_reads_device(const void *d_ids, std::uint64_t first_read, std::size_t n, std::uint64_t max_len, void *d_symbols, void *d_offsets,
                                       std::uint64_t capacity_symbols, std::uint64_t *truncated = nullptr, void *hip_stream = nullptr) const {
        std::uint64_t total = 0;
        check(msbwt_rle_extract_reads_device(raw_, d_ids, first_read, n, max_len, d_symbols, d_offsets, capacity_symbols, &total, truncated, hip_stream));
        return total;
    }
    /// The last left-walk call.
    struct WalkInfo {
        std::uint64_t walks = 0, steps = 0, dollar = 0, max_steps = 0, bad_row = 0, pieces = 0, scratch_bytes = 0, us = 0;
    };
    WalkInfo walk_info() const {
        std::uint64_t w[MSBWT_WALK_INFO_WORDS] = {};
        check(msbwt_rle_walk_info(raw_, w));
        WalkInfo i;
        i.walks = w[0], i.steps = w[1], i.dollar = w[2], i.max_steps = w[3], i.bad_row = w[4], i.pieces = w[5], i.scratch_bytes = w[6], i.us = w[7];
        return i;
    }
    /// Most left walks a launch takes (0 = automatic, 2^20; at most 2^28); results never depend on it.
    void set_walk_piece(std::uint64_t walks) { check(msbwt_rle_set_walk_piece(raw_, walks)); }
    /// HBM bytes of scratch a walk_rows call of n walks allocates (and frees again) on an index that holds something.
    static std::uint64_t walk_plan(std::uint64_t n, std::uint64_t max_steps, bool symbols = true, bool host = true, std::uint64_t piece = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_walk_plan(n, max_steps, symbols ? 1 : 0, host ? 1 : 0, piece, &bytes);
        if (rc) throw Panic(rc, "msbwt_walk_plan");
        return bytes;
    }
    /// What read_overlaps returns: the records of query i are [offsets[i], offsets[i + 1]) of lengths / first / counts, in ascending
    /// length -- the reads first[r] .. first[r] + counts[r] begin with the last lengths[r] symbols of the query searched --; matched,
    /// edges and stops (MSBWT_OVERLAP_END, _EMPTY, _BAD_SYMBOL) hold one entry a query.  A counting call leaves the columns empty.
    struct Overlaps {
        std::vector<std::uint64_t> offsets, lengths, first, counts, matched, edges;
        std::vector<std::uint8_t> stops;
        std::size_t size() const { return matched.size(); }
        std::uint64_t records() const { return offsets.empty() ? 0 : offsets.back(); }
    };
    /// The suffix-prefix overlaps of n queries (symbol codes as a ragged set: query i = symbols[offsets[i] .. offsets[i + 1])) with
    /// the reads of the index, at least min_overlap and, max_overlap not 0, at most max_overlap symbols long; strand 1 searches the
    /// reverse complements.  records = false: a counting call, one search instead of two.
    Overlaps read_overlaps(const std::vector<std::uint8_t> &symbols, const std::vector<std::uint64_t> &offsets, std::uint64_t min_overlap,
                           std::uint64_t max_overlap = 0, int strand = 0, bool records = true) const {
        const std::size_t n = offsets.empty() ? 0 : offsets.size() - 1;
        const std::uint8_t none = 0;
        Overlaps o;
        o.offsets.resize(n + 1);
        o.matched.resize(n);
        o.edges.resize(n);
        o.stops.resize(n);
        std::uint64_t total = 0;
        const std::uint8_t *where = symbols.empty() ? &none : symbols.data();
        check(msbwt_rle_read_overlaps(raw_, where, offsets.data(), n, min_overlap, max_overlap, strand, o.offsets.data(), nullptr, nullptr, nullptr, 0, &total,
                                      o.matched.data(), o.edges.data(), o.stops.data()));
        if (!records || total == 0) return o;
        o.lengths.resize(total);
        o.first.resize(total);
        o.counts.resize(total);
        check(msbwt_rle_read_overlaps(raw_, where, offsets.data(), n, min_overlap, max_overlap, strand, o.offsets.data(), o.lengths.data(), o.first.data(), o.counts.data(),
                                      total, &total, o.matched.data(), o.edges.data(), o.stops.data()));
        return o;
    }
    /// Device buffers (every output may be null; the three columns come together or not at all) -> R, the records of all queries;
    /// synchronises hip_stream.
    std::uint64_t read_overlaps_device(const void *d_symbols, const void *d_offsets, std::size_t n, std::uint64_t min_overlap, std::uint64_t max_overlap, int strand,
                                       void *d_out_offsets, void *d_lengths, void *d_first, void *d_counts, std::uint64_t capacity_records, void *d_matched,
                                       void *d_edges, void *d_stops, void *hip_stream = nullptr) const {
        std::uint64_t total = 0;
        check(msbwt_rle_read_overlaps_device(raw_, d_symbols, d_offsets, n, min_overlap, max_overlap, strand, d_out_offsets, d_lengths, d_first, d_counts, capacity_records,
                                             &total, d_matched, d_edges, d_stops, hip_stream));
        return total;
    }
    /// The last read-overlap call.
    struct OverlapInfo {
        std::uint64_t queries = 0, symbols = 0, records = 0, edges = 0, end = 0, empty = 0, bad_symbol = 0, lines = 0, pieces = 0, scratch_bytes = 0, us = 0,
                      piece_symbols = 0, piece_records = 0;
    };
    OverlapInfo overlap_info() const {
        std::uint64_t w[MSBWT_OVERLAP_INFO_WORDS] = {};
        check(msbwt_rle_overlap_info(raw_, w));
        OverlapInfo i;
        i.queries = w[0], i.symbols = w[1], i.records = w[2], i.edges = w[3], i.end = w[4], i.empty = w[5], i.bad_symbol = w[6], i.lines = w[7], i.pieces = w[8];
        i.scratch_bytes = w[9], i.us = w[10], i.piece_symbols = w[11], i.piece_records = w[12];
        return i;
    }
    /// Most overlap queries a launch takes (0 = automatic, 2^20; at most 2^28); results never depend on it.
    void set_overlap_piece(std::uint64_t queries) { check(msbwt_rle_set_overlap_piece(raw_, queries)); }
    /// Peak HBM bytes of scratch a read_overlaps call of n queries allocates (and frees again) on an index that holds something.
    static std::uint64_t overlap_plan(std::uint64_t n, bool host = true, std::uint64_t piece = 0, std::uint64_t piece_symbols = 0, std::uint64_t piece_records = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_overlap_plan(n, host ? 1 : 0, piece, piece_symbols, piece_records, &bytes);
        if (rc) throw Panic(rc, "msbwt_overlap_plan");
        return bytes;
    }
    /// What bridge_kmers returns: row (i, j) of symbols (n x max_paths rows of max_steps bytes) holds lengths[i max_paths + j] symbol codes
    /// (A C G T = 1 2 3 5) in walk order and zeros behind them; an unused row has length 0.  stops[i] is MSBWT_BRIDGE_EXHAUSTED ..
    /// MSBWT_BRIDGE_NO_TARGET; the bridges of at most depths[i] edges are all counted in found[i]; live[i] walks were live at the stop.
    struct Bridges {
        std::vector<std::uint8_t> symbols;
        std::vector<std::uint64_t> lengths, edge_sums, found;
        std::vector<std::uint8_t> stops;
        std::vector<std::uint64_t> depths, live;
        std::uint64_t max_steps = 0, max_paths = 0;
        std::size_t size() const { return found.size(); }
        /// the symbols of bridge j of pair i, in walk order
        std::vector<std::uint8_t> row(std::size_t i, std::size_t j) const {
            const std::uint8_t *at = symbols.data() + (i * max_paths + j) * max_steps;
            return std::vector<std::uint8_t>(at, at + lengths[i * max_paths + j]);
        }
    };
    /// Bridges (msbwt_hip.h, "bridges"): for each pair of packed k-mers (seed, target), 1 <= k <= 31, every walk of the k-mer graph from
    /// the seed into the target of min_steps .. max_steps edges in `direction` (MSBWT_BRIDGE_RIGHT, _LEFT); at most max_paths are written
    /// a pair, and a pair whose level holds more than max_live walks stops TOO_WIDE.
    Bridges bridge_kmers(const std::vector<std::uint64_t> &seeds, const std::vector<std::uint64_t> &targets, std::size_t k, std::uint64_t max_steps,
                         std::uint64_t min_steps = 0, std::uint64_t max_paths = 4, std::uint64_t max_live = 64, int direction = MSBWT_BRIDGE_RIGHT,
                         std::uint64_t min_count = 1, std::uint64_t min_edge = 0) const {
        if (targets.size() != seeds.size()) throw Panic(MSBWT_ERR_INVALID_ARG, "bridge_kmers: one target a seed");
        const std::size_t n = seeds.size();
        Bridges b;
        b.max_steps = max_steps;
        b.max_paths = max_paths;
        b.symbols.resize(n * max_paths * max_steps);
        b.lengths.resize(n * max_paths);
        b.edge_sums.resize(n * max_paths);
        b.found.resize(n);
        b.stops.resize(n);
        b.depths.resize(n);
        b.live.resize(n);
        check(msbwt_rle_bridge_kmers(raw_, seeds.data(), targets.data(), k, n, min_count, min_edge, direction, min_steps, max_steps, max_paths, max_live, b.symbols.data(),
                                     b.lengths.data(), b.edge_sums.data(), b.found.data(), b.stops.data(), b.depths.data(), b.live.data()));
        return b;
    }
    /// Device buffers (every output may be null; the byte arrays at any alignment); synchronises hip_stream.
    void bridge_kmers_device(const void *d_seeds, const void *d_targets, std::size_t k, std::size_t n, std::uint64_t min_count, std::uint64_t min_edge, int direction,
                             std::uint64_t min_steps, std::uint64_t max_steps, std::uint64_t max_paths, std::uint64_t max_live, void *d_symbols, void *d_lengths,
                             void *d_edge_sums, void *d_found, void *d_stops, void *d_depths, void *d_live, void *hip_stream = nullptr) const {
        check(msbwt_rle_bridge_kmers_device(raw_, d_seeds, d_targets, k, n, min_count, min_edge, direction, min_steps, max_steps, max_paths, max_live, d_symbols, d_lengths,
                                            d_edge_sums, d_found, d_stops, d_depths, d_live, hip_stream));
    }
    /// The last bridge call.
    struct BridgeInfo {
        std::uint64_t pairs = 0, rounds = 0, queries = 0, expanded = 0, found = 0, pieces = 0, scratch_bytes = 0, widest = 0;
    };
    BridgeInfo bridge_info() const {
        std::uint64_t w[MSBWT_BRIDGE_INFO_WORDS] = {};
        check(msbwt_rle_bridge_info(raw_, w));
        BridgeInfo i;
        i.pairs = w[0], i.rounds = w[1], i.queries = w[2], i.expanded = w[3], i.found = w[4], i.pieces = w[5], i.scratch_bytes = w[6], i.widest = w[7];
        return i;
    }
    /// The frontier slots of a bridge call's piece (0 = automatic, 2^20; max_live where that is larger; at most 2^28); results never depend on it.
    void set_bridge_slots(std::uint64_t slots) { check(msbwt_rle_set_bridge_slots(raw_, slots)); }
    /// HBM bytes of scratch a bridge call of n pairs allocates (and frees again) on an index that holds something.
    static std::uint64_t bridge_plan(std::uint64_t n, std::uint64_t max_steps, std::uint64_t max_paths = 4, std::uint64_t max_live = 64, bool host = true,
                                     std::uint64_t slots = 0) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_bridge_plan(n, max_steps, max_paths, max_live, host ? 1 : 0, slots, &bytes);
        if (rc) throw Panic(rc, "msbwt_bridge_plan");
        return bytes;
    }
    /// HBM bytes of scratch the last k-mer walk call allocated (and freed again before it returned).
    std::uint64_t spectrum_scratch_bytes() const {
        std::uint64_t bytes = 0;
        check(msbwt_rle_spectrum_scratch_bytes(raw_, &bytes));
        return bytes;
    }
    /// HBM bytes a by-source call allocates (and frees again) with the automatic frontier.
    static std::uint64_t kmers_by_source_plan(std::uint64_t total_rows, std::uint64_t free_hbm_bytes, std::size_t n_sources, std::uint64_t records = 0,
                                              bool sorted = false) {
        std::uint64_t bytes = 0;
        const int rc = msbwt_kmers_by_source_plan(total_rows, free_hbm_bytes, n_sources, records, sorted ? 1 : 0, &bytes);
        if (rc) throw Panic(rc, "msbwt_kmers_by_source_plan");
        return bytes;
    }
    /// Symbols an RLE stream encodes, counted up to 2^40 (the library refuses more).
    static std::uint64_t symbols_of(const std::vector<std::uint8_t> &rle) {
        std::uint64_t total = 0;
        unsigned place = 0;
        for (std::size_t i = 0; i < rle.size() && total < (std::uint64_t(1) << 40); ++i) {
            place = i && (rle[i] & MSBWT_MASK) == (rle[i - 1] & MSBWT_MASK) ? place + 1 : 0;
            if (place < 8) total += std::uint64_t(rle[i] >> MSBWT_LETTER_BITS) << (MSBWT_NUMBER_BITS * place);
        }
        return total < (std::uint64_t(1) << 40) ? total : 0;
    }

    // ---- batch forms (the GPU entry points proper) ----
    /// kmers: n x k symbol codes, row-major.
    std::vector<std::uint64_t> count_kmers(const std::vector<std::uint8_t> &kmers, std::size_t k) const {
        const std::size_t n = k ? kmers.size() / k : 0;
        if (k && kmers.size() % k) throw std::invalid_argument("kmers.size() is not a multiple of k");
        std::vector<std::uint64_t> out(n);
        check(msbwt_rle_count_kmers(raw_, kmers.data(), k, n, out.data()));
        return out;
    }
    /// FM range [l, h) of every k-mer of n x k symbol codes ({0, 0} when it does not occur).
    std::vector<BWTRange> kmer_ranges(const std::vector<std::uint8_t> &kmers, std::size_t k) const {
        const std::size_t n = k ? kmers.size() / k : 0;
        if (k && kmers.size() % k) throw std::invalid_argument("kmers.size() is not a multiple of k");
        std::vector<std::uint64_t> l(n), h(n);
        check(msbwt_rle_kmer_ranges(raw_, kmers.data(), k, n, l.data(), h.data()));
        std::vector<BWTRange> out(n);
        for (std::size_t i = 0; i < n; ++i) out[i] = BWTRange{l[i], h[i]};
        return out;
    }
    /// Left-extension counts, n x 6 row-major: [6 i + c] = count_kmer([c] ++ row i), c = 0..5 ($ A C G N T).
    std::vector<std::uint64_t> count_kmer_extensions(const std::vector<std::uint8_t> &kmers, std::size_t k) const {
        const std::size_t n = k ? kmers.size() / k : 0;
        if (k && kmers.size() % k) throw std::invalid_argument("kmers.size() is not a multiple of k");
        std::vector<std::uint64_t> out(6 * n);
        check(msbwt_rle_count_kmer_extensions(raw_, kmers.data(), k, n, out.data()));
        return out;
    }
    std::vector<BWTRange> constrain_ranges(const std::vector<std::uint8_t> &syms, const std::vector<BWTRange> &ranges) const {
        if (syms.size() != ranges.size()) throw std::invalid_argument("syms and ranges differ in length");
        std::vector<std::uint64_t> l(ranges.size()), h(ranges.size()), ol(ranges.size()), oh(ranges.size());
        for (std::size_t i = 0; i < ranges.size(); ++i) {
            l[i] = ranges[i].l;
            h[i] = ranges[i].h;
        }
        check(msbwt_rle_constrain_ranges(raw_, syms.data(), l.data(), h.data(), ranges.size(), ol.data(), oh.data()));
        std::vector<BWTRange> out(ranges.size());
        for (std::size_t i = 0; i < ranges.size(); ++i) out[i] = BWTRange{ol[i], oh[i]};
        return out;
    }
    /// Every k-mer window of n equal-length ASCII reads; second = counts of the reverse complements.
    std::pair<std::vector<std::uint64_t>, std::vector<std::uint64_t>> count_read_kmers(const std::string &reads,
                                                                                     std::size_t read_len, std::size_t k) const {
        if (!read_len || reads.size() % read_len || k < 1 || k > read_len) throw std::invalid_argument("bad read_len / k");
        const std::size_t n = reads.size() / read_len, w = read_len - k + 1;
        std::vector<std::uint64_t> fwd(n * w), rc(n * w);
        check(msbwt_rle_count_read_kmers(raw_, reinterpret_cast<const std::uint8_t *>(reads.data()), read_len, n, k, 1,
                                         fwd.data(), rc.data()));
        return {std::move(fwd), std::move(rc)};
    }

    /// k-mers over ACGT as 2-bit words (pack_2bit): ceil(k / 32) words each, 8 bytes per 31-mer across PCIe instead of 31.
    std::vector<std::uint64_t> count_kmers_packed(const std::vector<std::uint64_t> &words, std::size_t k) const {
        const std::size_t per = k > 32 ? 2 : 1;
        if (k < 1 || k > 64 || words.size() % per) throw std::invalid_argument("bad k / words");
        std::vector<std::uint64_t> out(words.size() / per);
        check(msbwt_rle_count_kmers_packed(raw_, words.data(), k, out.size(), out.data(), 64));
        return out;
    }
    /// ... with 32-bit counts (half the bytes on the way back; Panic(MSBWT_ERR_OVERFLOW) if a count does not fit)
    std::vector<std::uint32_t> count_kmers_packed_u32(const std::vector<std::uint64_t> &words, std::size_t k) const {
        const std::size_t per = k > 32 ? 2 : 1;
        if (k < 1 || k > 64 || words.size() % per) throw std::invalid_argument("bad k / words");
        std::vector<std::uint32_t> out(words.size() / per);
        check(msbwt_rle_count_kmers_packed(raw_, words.data(), k, out.size(), out.data(), 32));
        return out;
    }
    /// n x k symbol codes (A C G T = 1 2 3 5) -> 2-bit words: the k-mer as a base-4 number, first symbol most significant
    static std::vector<std::uint64_t> pack_2bit(const std::vector<std::uint8_t> &kmers, std::size_t k) {
        if (k < 1 || k > 64 || kmers.size() % k) throw std::invalid_argument("bad k / kmers");
        std::vector<std::uint64_t> words(kmers.size() / k * (k > 32 ? 2 : 1));
        if (msbwt_kmers_pack_2bit(kmers.data(), k, kmers.size() / k, words.data()) != MSBWT_OK)
            throw std::invalid_argument("a symbol outside A C G T cannot be packed into two bits");
        return words;
    }

    /// Device batch (pointers on this handle's GPU), asynchronous on `hip_stream`; device_status() reports bad input.
    void count_kmers_device(const void *d_kmers, std::size_t k, std::size_t n, void *d_out, void *hip_stream = nullptr) const {
        check(msbwt_rle_count_kmers_device(raw_, d_kmers, k, n, d_out, hip_stream));
    }
    void device_status(void *hip_stream = nullptr) const { check(msbwt_rle_device_status(raw_, hip_stream)); }
    /// One process per GPU: every rank ends up with all ranks' counts (d_all[r * n_mine + i] = rank r's d_mine[i]).
    /// wire_bits 16 / 32 narrows the counts on the wire; device_status() throws Panic(MSBWT_ERR_OVERFLOW) if one did not fit.
    void allgather_counts(void *comm, const void *d_mine, std::size_t n_mine, void *d_all, int wire_bits = 64,
                          void *hip_stream = nullptr) const {
        check(msbwt_rle_allgather_counts(raw_, comm, d_mine, n_mine, d_all, wire_bits, hip_stream));
    }

    void set_table_depth(int depth) { check(msbwt_rle_set_table_depth(raw_, depth)); }
    void set_table_packed(int mode) { check(msbwt_rle_set_table_packed(raw_, mode)); }
    void set_pair_index(int mode) { check(msbwt_rle_set_pair_index(raw_, mode)); }
    void set_search_kernel(int mode) { check(msbwt_rle_set_search_kernel(raw_, mode)); }
    /// HBM the loaded index may hold (0 = no budget): the space / time knob, as bin_power is the reference's (rle_bwt.rs:309-322)
    void set_memory_budget(std::uint64_t bytes) { check(msbwt_rle_set_memory_budget(raw_, bytes)); }
    /// 1 = the library orders every batch it can before counting it; 0 and -1 (the default) = never: a switch, there is no automatic mode
    void set_batch_order(int mode) { check(msbwt_rle_set_batch_order(raw_, mode)); }
    /// sparse suffix table (the suffixes that occur, one hashed 128-byte bucket per lookup): -1 = automatic (default), 0 = off, 16..31 = that depth
    void set_sparse_table(int depth) { check(msbwt_rle_set_sparse_table(raw_, depth)); }
    /// the k this index will mostly be asked about (0 = unknown): the automatic sparse table goes as deep as min(k, 31) where its table fits, instead of 23
    void set_query_length(int k) { check(msbwt_rle_set_query_length(raw_, k)); }
    int get_query_length() const { return msbwt_rle_get_query_length(raw_); }
    /// two-tier form of the sparse table (entries for the suffixes that occur at least twice, filter bits for the rest: read sets with errors):
    /// -1 = where the complete table of a depth does not fit (default), 0 = never, 1 = always
    void set_sparse_tiers(int mode) { check(msbwt_rle_set_sparse_tiers(raw_, mode)); }
    bool get_sparse_tiers() const { return msbwt_rle_get_sparse_tiers(raw_) != 0; }
    /// the second, shallower sparse level (17-symbol suffixes, k undeclared): -1 = automatic (default), 0 = never
    void set_sparse_second(int mode) { check(msbwt_rle_set_sparse_second(raw_, mode)); }
    int get_sparse_table() const { return msbwt_rle_get_sparse_table(raw_); }
    void set_table_side(int mode) { check(msbwt_rle_set_table_side(raw_, mode)); }
    std::uint64_t device_bytes() const { return msbwt_rle_device_bytes(raw_); }
    int search_kernel_for(size_t k) const { return msbwt_rle_search_kernel_for(raw_, k); }
    msbwt_rle *raw() const { return raw_; }

    /// A copy of the loaded index on another GPU of the node (GPU -> GPU, no rebuild).
    RleBWT replicate(int device) const {
        msbwt_rle *other = msbwt_rle_replicate(raw_, device);
        if (!other) throw Panic(MSBWT_ERR_HIP, msbwt_rle_last_error(raw_));
        return RleBWT(other);
    }
    /// One batch sharded over several replicas (one per GPU); counts in query order.
    static std::vector<std::uint64_t> count_kmers_multi(const std::vector<const RleBWT *> &replicas,
                                                        const std::vector<std::uint8_t> &kmers, std::size_t k) {
        if (replicas.empty()) throw std::invalid_argument("no replicas");
        const std::size_t n = k ? kmers.size() / k : 0;
        std::vector<const msbwt_rle *> raws;
        for (const RleBWT *r : replicas) raws.push_back(r->raw_);
        std::vector<std::uint64_t> out(n);
        const int code = msbwt_rle_count_kmers_multi(raws.data(), raws.size(), kmers.data(), k, n, out.data());
        if (code != MSBWT_OK) throw Panic(code, "count_kmers_multi failed");
        return out;
    }

  private:
    explicit RleBWT(msbwt_rle *adopted) : raw_(adopted) {}
    void check(int code) const {
        if (code == MSBWT_OK) return;
        const std::string msg = msbwt_rle_last_error(raw_);
        switch (code) {
            case MSBWT_ERR_IO: throw std::system_error(std::make_error_code(std::errc::io_error), msg);
            case MSBWT_ERR_UNEXPECTED_EOF: throw UnexpectedEof(msg);
            default: throw Panic(code, msg);
        }
    }
    msbwt_rle *raw_;
};

/// An RCCL communicator over the GPUs of a one-process-per-GPU job, made through the library (librccl.so is bound at run
/// time).  Rank 0 calls RankComm::unique_id(), ships the bytes to the other ranks, every rank constructs a RankComm with its
/// GPU current; RleBWT::allgather_counts takes raw().
class RankComm {
  public:
    static std::array<unsigned char, MSBWT_COMM_ID_BYTES> unique_id() {
        std::array<unsigned char, MSBWT_COMM_ID_BYTES> id{};
        if (msbwt_comm_get_unique_id(id.data()) != MSBWT_OK) throw Panic(MSBWT_ERR_RCCL, "msbwt_comm_get_unique_id (is librccl.so there?)");
        return id;
    }
    RankComm(int nranks, const std::array<unsigned char, MSBWT_COMM_ID_BYTES> &id, int rank) {
        if (msbwt_comm_init_rank(&raw_, nranks, id.data(), rank) != MSBWT_OK) throw Panic(MSBWT_ERR_RCCL, "msbwt_comm_init_rank");
    }
    ~RankComm() {
        if (raw_) msbwt_comm_destroy(raw_);
    }
    RankComm(const RankComm &) = delete;
    RankComm &operator=(const RankComm &) = delete;
    void *raw() const { return raw_; }

  private:
    void *raw_ = nullptr;
};

// ---- string_util (src/string_util.rs) and bwt_converter (src/bwt_converter.rs) ----
inline std::vector<std::uint8_t> convert_stoi(const std::string &seq) {
    std::vector<std::uint8_t> out(seq.size());
    msbwt_convert_stoi(reinterpret_cast<const std::uint8_t *>(seq.data()), seq.size(), out.data());
    return out;
}
inline std::string convert_itos(const std::vector<std::uint8_t> &iseq) {
    std::string out(iseq.size(), '\0');
    msbwt_convert_itos(iseq.data(), iseq.size(), reinterpret_cast<std::uint8_t *>(&out[0]));
    return out;
}
inline std::vector<std::uint8_t> reverse_complement_i(const std::vector<std::uint8_t> &seq) {
    std::vector<std::uint8_t> out(seq.size());
    msbwt_reverse_complement_i(seq.data(), seq.size(), out.data());
    return out;
}
inline std::vector<std::uint8_t> convert_to_vec(const std::string &bwt) {
    const auto *p = reinterpret_cast<const std::uint8_t *>(bwt.data());
    const std::size_t need = msbwt_convert_to_vec(p, bwt.size(), nullptr, 0);
    if (need == SIZE_MAX) throw Panic(MSBWT_ERR_INVALID_SYMBOL, "Unexpected symbol in input");
    std::vector<std::uint8_t> out(need);
    msbwt_convert_to_vec(p, bwt.size(), out.data(), need);
    return out;
}
inline void save_bwt_numpy(const std::vector<std::uint8_t> &bwt, const std::string &filename) {
    if (msbwt_save_bwt_numpy(bwt.data(), bwt.size(), filename.c_str()) != MSBWT_OK)
        throw std::system_error(std::make_error_code(std::errc::io_error), "cannot write " + filename);
}

}  // namespace msbwt
