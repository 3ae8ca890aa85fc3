// The C++ mirror of the left walks (include/msbwt_hip.hpp): the methods exist with these signatures, the pure plan answers, and
// Walks::sequence turns a row of walk order into reading order.  No device is touched.
#include "msbwt_hip.hpp"

int main() {
    using msbwt::RleBWT;
    // 256 + 4 pad(8 * 200 -> 64 walks a piece: 512) + pad(64) + pad(64 * 7)
    if (RleBWT::walk_plan(200, 7, true, true, 64) != 256 + 4 * 512 + 256 + 512) return 1;
    if (RleBWT::walk_plan(200, 7, false, true, 64) != 256 + 4 * 512 + 256) return 2;
    if (RleBWT::walk_plan(200, 7, true, false, 64) != 256 || RleBWT::walk_plan(0, 7) != 0) return 3;
    try {
        RleBWT::walk_plan(2, std::uint64_t(1) << 40);
        return 4;
    } catch (const msbwt::Panic &p) {
        if (p.code != MSBWT_ERR_TOO_LARGE) return 5;
    }
    try {
        RleBWT::walk_plan(2, 2, true, true, (std::uint64_t(1) << 28) + 1);
        return 6;
    } catch (const msbwt::Panic &p) {
        if (p.code != MSBWT_ERR_INVALID_ARG) return 7;
    }
    RleBWT::Walks (RleBWT::*walk)(const std::vector<std::uint64_t> &, std::uint64_t, bool) const = &RleBWT::walk_rows;
    RleBWT::Walks (RleBWT::*locate)(const std::vector<std::uint64_t> &, std::uint64_t) const = &RleBWT::locate_rows;
    void (RleBWT::*walk_device)(const void *, std::size_t, std::uint64_t, void *, void *, void *, void *, void *, void *) const = &RleBWT::walk_rows_device;
    RleBWT::Reads (RleBWT::*extract)(const std::vector<std::uint64_t> &, std::uint64_t, std::size_t, std::uint64_t) const = &RleBWT::extract_reads;
    std::uint64_t (RleBWT::*extract_device)(const void *, std::uint64_t, std::size_t, std::uint64_t, void *, void *, std::uint64_t, std::uint64_t *, void *) const =
        &RleBWT::extract_reads_device;
    RleBWT::WalkInfo (RleBWT::*info)() const = &RleBWT::walk_info;
    void (RleBWT::*piece)(std::uint64_t) = &RleBWT::set_walk_piece;
    if (!(walk && locate && walk_device && extract && extract_device && info && piece)) return 8;
    RleBWT::Walks w;
    w.max_steps = 4;
    w.symbols = {3, 2, 1, 0, 5, 3, 2, 2};
    w.steps = {3, 4};
    if (w.size() != 2 || w.sequence(0) != std::vector<std::uint8_t>{1, 2, 3} || w.sequence(1) != std::vector<std::uint8_t>{2, 2, 3, 5}) return 9;
    RleBWT::Reads r;
    RleBWT::WalkInfo i;
    return r.size() == 0 && r.truncated == 0 && i.bad_row == 0 && MSBWT_WALK_DOLLAR == 1 && MSBWT_WALK_MAX_STEPS == 2 && MSBWT_WALK_BAD_ROW == 3 ? 0 : 10;
}
