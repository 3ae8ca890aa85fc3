/* C host of the read overlaps: all-against-all suffix-prefix overlaps of the reads an index holds.  The index is a .npy file of RLE
 * bytes (the reference's format); its reads are extracted a piece at a time and searched on both strands, and every overlap goes out
 * as one line `query read length strand`: the last `length` symbols of read `query` (strand 1: of its reverse complement) are the
 * first `length` symbols of read `read`.  A read found as itself at its whole length on strand 0 is left out.
 *
 *   gcc -std=c11 -Iinclude examples/read_overlaps.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o read_overlaps
 *   ./read_overlaps index.npy [--min-overlap M] [--max-len L] [--piece N] > edges.txt
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
    fprintf(stderr, "usage: %s INDEX.npy [--min-overlap M] [--max-len L] [--piece N]   (M >= 1, default 20; L >= 1, default 1024; piece >= 1, default 65536)\n", me);
    return 2;
}

int main(int argc, char **argv) {
    uint64_t min_overlap = 20, max_len = 1024, piece = 65536;
    if (argc < 2 || argv[1][0] == '-') return usage(argv[0]);
    for (int a = 2; a < argc; a += 2) {
        uint64_t *into = !strcmp(argv[a], "--min-overlap") ? &min_overlap : !strcmp(argv[a], "--max-len") ? &max_len : !strcmp(argv[a], "--piece") ? &piece : NULL;
        char *end = NULL;
        if (!into || a + 1 >= argc || argv[a + 1][0] == '-' || argv[a + 1][0] == '\0') return usage(argv[0]);
        *into = strtoull(argv[a + 1], &end, 10);
        if (*end) return usage(argv[0]);
    }
    if (min_overlap < 1 || max_len < 1 || piece < 1 || max_len >= (1ull << 40) / piece) return usage(argv[0]);

    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_numpy_file(bwt, argv[1]);
    if (rc != MSBWT_OK) return fail(bwt, "load_numpy_file", rc);
    const uint64_t reads = msbwt_rle_get_symbol_count(bwt, 0);

    uint8_t *symbols = (uint8_t *)malloc((size_t)(piece * max_len));
    uint64_t *offsets = (uint64_t *)malloc((size_t)(piece + 1) * sizeof(uint64_t));
    uint64_t *rec_offsets = (uint64_t *)malloc((size_t)(piece + 1) * sizeof(uint64_t));
    uint64_t *columns = NULL, capacity = 0, edges_in_all = 0, truncated_in_all = 0;
    if (!symbols || !offsets || !rec_offsets) return 1;
    for (uint64_t done = 0; done < reads; done += piece) {
        const uint64_t n = reads - done < piece ? reads - done : piece;
        uint64_t total = 0, truncated = 0;
        rc = msbwt_rle_extract_reads(bwt, NULL, done, (size_t)n, max_len, symbols, offsets, n * max_len, &total, &truncated);
        if (rc != MSBWT_OK) return fail(bwt, "extract_reads", rc);
        truncated_in_all += truncated;
        for (int strand = 0; strand < 2; ++strand) {
            /* the counting call says how many records there are: one search; the filling call costs two more */
            uint64_t records = 0;
            rc = msbwt_rle_read_overlaps(bwt, symbols, offsets, (size_t)n, min_overlap, 0, strand, NULL, NULL, NULL, NULL, 0, &records, NULL, NULL, NULL);
            if (rc != MSBWT_OK) return fail(bwt, "read_overlaps", rc);
            if (records > capacity) {
                free(columns);
                capacity = records;
                columns = (uint64_t *)malloc((size_t)capacity * 3 * sizeof(uint64_t));
                if (!columns) return 1;
            }
            if (records == 0) continue;
            uint64_t *lengths = columns, *first = columns + capacity, *counts = columns + 2 * capacity;
            rc = msbwt_rle_read_overlaps(bwt, symbols, offsets, (size_t)n, min_overlap, 0, strand, rec_offsets, lengths, first, counts, capacity, &records, NULL, NULL,
                                         NULL);
            if (rc != MSBWT_OK) return fail(bwt, "read_overlaps", rc);
            for (uint64_t q = 0; q < n; ++q) {
                const uint64_t id = done + q, whole = offsets[q + 1] - offsets[q];
                for (uint64_t r = rec_offsets[q]; r < rec_offsets[q + 1]; ++r)
                    for (uint64_t read = first[r]; read < first[r] + counts[r]; ++read) {
                        if (strand == 0 && read == id && lengths[r] == whole) continue; /* the read itself */
                        printf("%llu %llu %llu %d\n", (unsigned long long)id, (unsigned long long)read, (unsigned long long)lengths[r], strand);
                        ++edges_in_all;
                    }
            }
        }
    }
    fprintf(stderr, "%llu reads, %llu overlaps of at least %llu symbols", (unsigned long long)reads, (unsigned long long)edges_in_all, (unsigned long long)min_overlap);
    if (truncated_in_all) fprintf(stderr, "; %llu reads are longer than --max-len %llu and were searched as their last %llu symbols", (unsigned long long)truncated_in_all,
                                  (unsigned long long)max_len, (unsigned long long)max_len);
    fputc('\n', stderr);
    free(columns);
    free(rec_offsets);
    free(offsets);
    free(symbols);
    msbwt_rle_free(bwt);
    return truncated_in_all ? 3 : 0;
}
