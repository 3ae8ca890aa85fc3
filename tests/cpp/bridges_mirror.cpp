// The C++ mirror of the bridges (include/msbwt_hip.hpp): the methods exist with these signatures, the pure plan answers, and Bridges
// hands out its rows.  No device is touched.
#include "msbwt_hip.hpp"

int main() {
    using msbwt::RleBWT;
    // slots = 64, max_live = 8: P = 8 pairs, S = 64 states of W = 8 + 2 words:
    // 256 + pad(48 * 8) + 2 pad(8 * 10 * 64) + pad(8 * 64) + pad(8) + 2 pad(8 * max(256, 48))
    const std::uint64_t device = 256 + 512 + 2 * 5120 + 512 + 256 + 2 * 2048;
    if (RleBWT::bridge_plan(200, 40, 3, 8, false, 64) != device) return 1;
    // and in the host form 2 pad(8 * 8) + pad(8 * 3 * 40) + 2 pad(8 * 8 * 3) + 3 pad(8 * 8) + pad(8)
    if (RleBWT::bridge_plan(200, 40, 3, 8, true, 64) != device + 2 * 256 + 1024 + 2 * 256 + 3 * 256 + 256) return 2;
    if (RleBWT::bridge_plan(0, 40) != 0) return 3;
    try {
        RleBWT::bridge_plan(2, MSBWT_BRIDGE_MAX_STEPS_CAP + 1);
        return 4;
    } catch (const msbwt::Panic &p) {
        if (p.code != MSBWT_ERR_TOO_LARGE) return 5;
    }
    try {
        RleBWT::bridge_plan(2, 10, 0);
        return 6;
    } catch (const msbwt::Panic &p) {
        if (p.code != MSBWT_ERR_INVALID_ARG) return 7;
    }
    RleBWT::Bridges (RleBWT::*bridge)(const std::vector<std::uint64_t> &, const std::vector<std::uint64_t> &, std::size_t, std::uint64_t, std::uint64_t, std::uint64_t,
                                      std::uint64_t, int, std::uint64_t, std::uint64_t) const = &RleBWT::bridge_kmers;
    void (RleBWT::*device_form)(const void *, const void *, std::size_t, std::size_t, std::uint64_t, std::uint64_t, int, std::uint64_t, std::uint64_t, std::uint64_t,
                                std::uint64_t, void *, void *, void *, void *, void *, void *, void *, void *) const = &RleBWT::bridge_kmers_device;
    RleBWT::BridgeInfo (RleBWT::*info)() const = &RleBWT::bridge_info;
    void (RleBWT::*slots)(std::uint64_t) = &RleBWT::set_bridge_slots;
    if (!(bridge && device_form && info && slots)) return 8;
    RleBWT::Bridges b;
    if (b.size() != 0) return 9;
    b.max_steps = 3;
    b.max_paths = 2;
    b.symbols = {1, 2, 0, 0, 0, 0, 5, 5, 5, 3, 0, 0};
    b.lengths = {2, 0, 3, 1};
    b.found = {1, 2};
    RleBWT::BridgeInfo i;
    return b.size() == 2 && b.row(0, 0) == std::vector<std::uint8_t>{1, 2} && b.row(0, 1).empty() && b.row(1, 0) == std::vector<std::uint8_t>{5, 5, 5} &&
                   b.row(1, 1) == std::vector<std::uint8_t>{3} && i.widest == 0 && MSBWT_BRIDGE_EXHAUSTED == 1 && MSBWT_BRIDGE_NO_TARGET == 6 &&
                   MSBWT_BRIDGE_INFO_WORDS == 8 && MSBWT_BRIDGE_RIGHT == MSBWT_TRACE_RIGHT && MSBWT_BRIDGE_LEFT == MSBWT_TRACE_LEFT
               ? 0
               : 10;
}
