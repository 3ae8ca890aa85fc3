// The C++ mirror of the read overlaps (include/msbwt_hip.hpp): the methods exist with these signatures, the pure plan answers, and
// Overlaps counts its queries and records.  No device is touched.
#include "msbwt_hip.hpp"

int main() {
    using msbwt::RleBWT;
    // P = 64: 256 + pad(8 * 65) + pad(8 * 1), and in the host form 2 pad(8 * 65) + 2 pad(8 * 64) + pad(64) + pad(1000) + 3 pad(8 * 10)
    if (RleBWT::overlap_plan(200, false, 64) != 256 + 768 + 256) return 1;
    if (RleBWT::overlap_plan(200, false, 64, 1000, 10) != 1280) return 2;
    if (RleBWT::overlap_plan(200, true, 64, 1000, 10) != 1280 + 2 * 768 + 2 * 512 + 256 + 1024 + 3 * 256) return 3;
    if (RleBWT::overlap_plan(200, true, 64, 1000, 0) != 1280 + 2 * 768 + 2 * 512 + 256 + 1024 || RleBWT::overlap_plan(0) != 0) return 4;
    try {
        RleBWT::overlap_plan(std::uint64_t(1) << 40);
        return 5;
    } catch (const msbwt::Panic &p) {
        if (p.code != MSBWT_ERR_TOO_LARGE) return 6;
    }
    try {
        RleBWT::overlap_plan(2, true, (std::uint64_t(1) << 28) + 1);
        return 7;
    } catch (const msbwt::Panic &p) {
        if (p.code != MSBWT_ERR_INVALID_ARG) return 8;
    }
    RleBWT::Overlaps (RleBWT::*overlaps)(const std::vector<std::uint8_t> &, const std::vector<std::uint64_t> &, std::uint64_t, std::uint64_t, int, bool) const =
        &RleBWT::read_overlaps;
    std::uint64_t (RleBWT::*overlaps_device)(const void *, const void *, std::size_t, std::uint64_t, std::uint64_t, int, void *, void *, void *, void *, std::uint64_t,
                                             void *, void *, void *, void *) const = &RleBWT::read_overlaps_device;
    RleBWT::OverlapInfo (RleBWT::*info)() const = &RleBWT::overlap_info;
    void (RleBWT::*piece)(std::uint64_t) = &RleBWT::set_overlap_piece;
    if (!(overlaps && overlaps_device && info && piece)) return 9;
    RleBWT::Overlaps o;
    if (o.size() != 0 || o.records() != 0) return 10;
    o.offsets = {0, 1, 1, 3};
    o.matched = {2, 0, 4};
    RleBWT::OverlapInfo i;
    return o.size() == 3 && o.records() == 3 && i.piece_records == 0 && MSBWT_OVERLAP_END == 1 && MSBWT_OVERLAP_EMPTY == 2 && MSBWT_OVERLAP_BAD_SYMBOL == 3 &&
                   MSBWT_OVERLAP_INFO_WORDS == 13
               ? 0
               : 11;
}
