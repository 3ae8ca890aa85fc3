/* C host of the read extraction: the reads an index holds, written as FASTA.  The index is a .npy file of RLE bytes (the reference's
 * format); read i is the i-th of the sorted read set.  The reads go a piece at a time, so the buffers stay small whatever the index
 * holds; a read longer than --max-len comes as its last max-len symbols and is counted on stderr (exit status 3).
 *
 *   gcc -std=c11 -Iinclude examples/extract_reads.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o extract_reads
 *   ./extract_reads index.npy [--first N] [--count N] [--max-len L] [--piece N] > reads.fa
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

static int usage(const char *me) {
    fprintf(stderr, "usage: %s INDEX.npy [--first N] [--count N] [--max-len L] [--piece N]   (L >= 1, default 1024; piece >= 1, default 65536)\n", me);
    return 2;
}

int main(int argc, char **argv) {
    uint64_t first = 0, count = UINT64_MAX, max_len = 1024, piece = 65536;
    if (argc < 2 || argv[1][0] == '-') return usage(argv[0]);
    for (int a = 2; a < argc; a += 2) {
        uint64_t *into = !strcmp(argv[a], "--first") ? &first : !strcmp(argv[a], "--count") ? &count : !strcmp(argv[a], "--max-len") ? &max_len :
                         !strcmp(argv[a], "--piece") ? &piece : NULL;
        char *end = NULL;
        if (!into || a + 1 >= argc || argv[a + 1][0] == '-' || argv[a + 1][0] == '\0') return usage(argv[0]);
        *into = strtoull(argv[a + 1], &end, 10);
        if (*end) return usage(argv[0]);
    }
    if (max_len < 1 || piece < 1 || max_len >= (1ull << 40) / piece) return usage(argv[0]);

    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_numpy_file(bwt, argv[1]);
    if (rc != MSBWT_OK) return fail(bwt, "load_numpy_file", rc);
    const uint64_t reads = msbwt_rle_get_symbol_count(bwt, 0);
    if (first > reads) first = reads;
    if (count > reads - first) count = reads - first;

    /* a piece of n reads never has more than n x max_len symbols: one call a piece, one walk a call */
    uint8_t *symbols = (uint8_t *)malloc((size_t)(piece * max_len));
    uint64_t *offsets = (uint64_t *)malloc((size_t)(piece + 1) * sizeof(uint64_t));
    if (!symbols || !offsets) return 1;
    uint64_t truncated_in_all = 0, symbols_in_all = 0;
    for (uint64_t done = 0; done < count; done += piece) {
        const uint64_t n = count - done < piece ? count - done : piece;
        uint64_t total = 0, truncated = 0;
        rc = msbwt_rle_extract_reads(bwt, NULL, first + done, (size_t)n, max_len, symbols, offsets, n * max_len, &total, &truncated);
        if (rc != MSBWT_OK) return fail(bwt, "extract_reads", rc);
        for (uint64_t j = 0; j < n; ++j) {
            const uint64_t len = offsets[j + 1] - offsets[j];
            printf(">read_%llu length=%llu\n", (unsigned long long)(first + done + j), (unsigned long long)len);
            for (uint64_t p = offsets[j]; p < offsets[j + 1]; ++p) putchar("$ACGNT"[symbols[p] < 6 ? symbols[p] : 4]);
            putchar('\n');
        }
        truncated_in_all += truncated;
        symbols_in_all += total;
    }
    fprintf(stderr, "%llu reads of %llu, %llu symbols", (unsigned long long)count, (unsigned long long)reads, (unsigned long long)symbols_in_all);
    if (truncated_in_all) fprintf(stderr, "; %llu reads are longer than --max-len %llu and come as their last %llu symbols", (unsigned long long)truncated_in_all,
                                  (unsigned long long)max_len, (unsigned long long)max_len);
    fputc('\n', stderr);
    free(offsets);
    free(symbols);
    msbwt_rle_free(bwt);
    return truncated_in_all ? 3 : 0;
}
