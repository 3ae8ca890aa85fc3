/* C host of the counts by source: three small read sets are built and merged on the GPU, the merged BWT is loaded with the merge's
 * source vector attached, and one search gives a k-mer's count in each of the three sets.
 *
 *   gcc -std=c11 -Iinclude examples/count_by_source.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o count_by_source
 *   ./count_by_source ACG
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

#define SETS 3

static const char *const kReads[SETS][4] = {
    {"ACGTACGT", "ACGGT", "TTACG", NULL},
    {"ACGT", "CCCACG", NULL, NULL},
    {"GGGT", "TACGA", "ACGACG", "A"},
};

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2 || argv[1][0] == '-' || strlen(argv[1]) > 64) {
        fprintf(stderr, "usage: %s KMER   (over ACGTN$, at most 64 symbols; e.g. ACG)\n", argv[0]);
        return 2;
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    /* the BWT of every set, one after the other in one array, as msbwt_rle_merge_many takes them */
    uint8_t rle[SETS * 64];
    uint64_t rle_offsets[SETS + 1] = {0};
    for (int s = 0; s < SETS; ++s) {
        uint8_t text[64];
        uint64_t read_offsets[5] = {0}, len = 0;
        size_t n = 0;
        for (; n < 4 && kReads[s][n]; ++n) {
            memcpy(text + read_offsets[n], kReads[s][n], strlen(kReads[s][n]));
            read_offsets[n + 1] = read_offsets[n] + strlen(kReads[s][n]);
        }
        const int rc = msbwt_rle_build_from_reads(bwt, text, read_offsets, n, 1, rle + rle_offsets[s], 64, &len);
        if (rc != MSBWT_OK) return fail(bwt, "build_from_reads", rc);
        rle_offsets[s + 1] = rle_offsets[s] + len;
    }
    /* merge, load, and keep the source of every merged row in HBM */
    int rc = msbwt_rle_load_merged_many_sources(bwt, rle, rle_offsets, SETS);
    if (rc != MSBWT_OK) return fail(bwt, "load_merged_many_sources", rc);
    uint64_t totals[SETS], counts[SETS];
    if ((rc = msbwt_rle_source_totals(bwt, totals)) != MSBWT_OK) return fail(bwt, "source_totals", rc);
    uint8_t kmer[64];
    const size_t k = strlen(argv[1]);
    msbwt_convert_stoi((const uint8_t *)argv[1], k, kmer);
    if ((rc = msbwt_rle_count_kmers_by_source(bwt, kmer, k, 1, counts)) != MSBWT_OK) return fail(bwt, "count_kmers_by_source", rc);
    printf("%d sources, %llu merged rows\n", msbwt_rle_source_count(bwt), (unsigned long long)msbwt_rle_get_total_size(bwt));
    for (int s = 0; s < SETS; ++s)
        printf("set %d (%llu symbols): %s occurs %llu times\n", s, (unsigned long long)totals[s], argv[1], (unsigned long long)counts[s]);
    msbwt_rle_free(bwt);
    return 0;
}
