/* C host of the k-mers by source: three small read sets are built and merged on the GPU, the merged BWT is loaded with the merge's
 * source vector attached, and the index itself says which k-mers only set 0 holds, and how many k-mers one, two or all three sets share.
 * Nothing is dumped and filtered on the host: the predicate "any count in set 0, ABSENT from sets 1 and 2" runs on the device.
 *
 *   gcc -std=c11 -Iinclude examples/private_kmers.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o private_kmers
 *   ./private_kmers 3
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

#define SETS 3
#define BINS 16

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
    const long k = argc == 2 ? strtol(argv[1], NULL, 10) : 3;
    if (argc > 2 || (argc == 2 && argv[1][0] == '-') || k < 1 || k > 32) {
        fprintf(stderr, "usage: %s [K]   (1 <= K <= 32, default 3)\n", argv[0]);
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

    /* one spectrum per set, and the sharing tallies */
    uint64_t hist[SETS * BINS], sharing[SETS + 1], distinct[SETS], occurrences[SETS];
    if ((rc = msbwt_rle_kmer_spectrum_by_source(bwt, (size_t)k, hist, BINS, sharing, distinct, occurrences)) != MSBWT_OK)
        return fail(bwt, "kmer_spectrum_by_source", rc);
    for (int s = 0; s < SETS; ++s)
        printf("set %d holds %llu distinct %ld-mers (%llu occurrences); %llu of the index's it does not hold\n", s, (unsigned long long)distinct[s], k,
               (unsigned long long)occurrences[s], (unsigned long long)hist[s * BINS]);
    for (int j = 1; j <= SETS; ++j) printf("%llu %ld-mers are held by exactly %d set%s\n", (unsigned long long)sharing[j], k, j, j == 1 ? "" : "s");

    /* private to set 0: in max_counts UINT64_MAX is "no limit" and 0 is "absent from this set" */
    const uint64_t min_counts[SETS] = {1, 0, 0}, max_counts[SETS] = {UINT64_MAX, 0, 0};
    uint64_t n = 0;
    if ((rc = msbwt_rle_enumerate_kmers_by_source(bwt, (size_t)k, min_counts, max_counts, 0, 0, 1, NULL, NULL, NULL, 0, &n)) != MSBWT_OK)
        return fail(bwt, "enumerate_kmers_by_source", rc);
    uint64_t *words = malloc((n + 1) * sizeof *words), *counts = malloc((n + 1) * SETS * sizeof *counts);
    if (!words || !counts) return 1;
    if (n && (rc = msbwt_rle_enumerate_kmers_by_source(bwt, (size_t)k, min_counts, max_counts, 0, 0, 1, words, counts, NULL, n, &n)) != MSBWT_OK)
        return fail(bwt, "enumerate_kmers_by_source", rc);
    printf("%llu %ld-mers are private to set 0:\n", (unsigned long long)n, k);
    for (uint64_t i = 0; i < n; ++i) {
        char text[33] = {0};
        for (long j = 0; j < k; ++j) text[j] = "ACGT"[(words[i] >> (2 * (k - 1 - j))) & 3];
        printf("%s\t%llu\n", text, (unsigned long long)counts[i * SETS]);
    }
    free(words);
    free(counts);
    msbwt_rle_free(bwt);
    return 0;
}
