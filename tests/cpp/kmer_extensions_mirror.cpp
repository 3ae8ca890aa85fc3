// The k-mer range and extension calls through the C++ mirror (include/msbwt_hip.hpp), driven by tests/test_gpu_extensions.py:
//   kmer_extensions_mirror comp_msbwt.npy queries.bin k out.bin
// queries.bin: n x k symbol codes; out.bin receives n u64 l, n u64 h, then n x 6 u64 extension counts.  Needs an MI355X;
// without arguments it prints its usage.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "msbwt_hip.hpp"

int main(int argc, char **argv) {
    if (argc != 5) {
        std::printf("usage: %s comp_msbwt.npy queries.bin k out.bin\n", argv[0]);
        return 2;
    }
    try {
        msbwt::RleBWT bwt;
        bwt.load_numpy_file(argv[1]);
        std::ifstream in(argv[2], std::ios::binary);
        const std::vector<std::uint8_t> kmers((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const std::size_t k = std::stoul(argv[3]);
        const std::vector<msbwt::BWTRange> ranges = bwt.kmer_ranges(kmers, k);
        const std::vector<std::uint64_t> ext = bwt.count_kmer_extensions(kmers, k);
        std::vector<std::uint64_t> out;
        for (const auto &r : ranges) out.push_back(r.l);
        for (const auto &r : ranges) out.push_back(r.h);
        out.insert(out.end(), ext.begin(), ext.end());
        std::ofstream o(argv[4], std::ios::binary);
        o.write(reinterpret_cast<const char *>(out.data()), std::streamsize(out.size() * sizeof(std::uint64_t)));
        std::printf("%zu queries\n", ranges.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
