/* C host of the canonical traces: the reads given on the command line are loaded as an index, and from the first k-mer of every read
 * AND from its reverse complement a walk goes right through the strand-merged k-mer graph in unitig mode -- on while the path neither
 * branches nor merges nor folds back onto its own mirror.  The reads may come from either strand: a k-mer counts with its reverse
 * complement.  FASTA out: the seed with its extension, and in the header line the strand, the steps taken, why the walk stopped, and
 * the sum of the class counts of the (k+1)-mers it crossed.
 *
 *   gcc -std=c11 -Iinclude examples/trace_canonical_kmers.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o trace_canonical_kmers
 *   ./trace_canonical_kmers 5 AAGCTCATTGGA TCCAATGAGCTT
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

/* the packed reverse complement of a k-mer: its k fields in reverse order, each complemented */
static uint64_t reverse_complement(uint64_t word, size_t k) {
    uint64_t out = 0;
    for (size_t i = 0; i < k; ++i, word >>= 2) out = out << 2 | (3 - (word & 3));
    return out;
}

int main(int argc, char **argv) {
    static const char *const stops[] = {"", "DEAD_END", "BRANCH", "MERGE", "RETURNED", "TARGET", "MAX_STEPS", "NOT_A_NODE", "MIRROR"};
    char *end = NULL;
    const unsigned long k_arg = argc >= 3 ? strtoul(argv[1], &end, 10) : 0;
    if (argc < 3 || *end || k_arg < 1 || k_arg > 31) {
        fprintf(stderr, "usage: %s K READ [READ...]   (1 <= K <= 31, reads over ACGTN, from either strand)\n", argv[0]);
        return 2;
    }
    const size_t k = (size_t)k_arg, n_reads = (size_t)(argc - 2);
    uint64_t *offsets = (uint64_t *)calloc(n_reads + 1, sizeof(uint64_t));
    uint64_t max_steps = 1;
    for (size_t r = 0; r < n_reads; ++r) {
        offsets[r + 1] = offsets[r] + strlen(argv[2 + r]);
        max_steps += 2 * strlen(argv[2 + r]); /* a unitig has no more nodes than the reads have k-mers on both strands */
    }
    uint8_t *reads = (uint8_t *)malloc(offsets[n_reads] + 1);
    for (size_t r = 0; r < n_reads; ++r) memcpy(reads + offsets[r], argv[2 + r], (size_t)(offsets[r + 1] - offsets[r]));

    /* the seeds: the first k-mer of every read that has one over ACGT, packed two bits a symbol, and behind it its reverse complement */
    uint64_t *seeds = (uint64_t *)calloc(2 * n_reads, sizeof(uint64_t));
    size_t *read_of = (size_t *)calloc(n_reads, sizeof(size_t));
    uint8_t *codes = (uint8_t *)malloc(k);
    size_t n = 0;
    for (size_t r = 0; r < n_reads; ++r) {
        if (offsets[r + 1] - offsets[r] < k) continue;
        msbwt_convert_stoi(reads + offsets[r], k, codes);
        if (msbwt_kmers_pack_2bit(codes, k, 1, seeds + 2 * n) != MSBWT_OK) continue; /* an N among the first k symbols */
        seeds[2 * n + 1] = reverse_complement(seeds[2 * n], k);
        read_of[n++] = r;
    }

    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_reads(bwt, reads, offsets, n_reads, /*ascii=*/1);
    if (rc != MSBWT_OK) return fail(bwt, "load_reads", rc);
    uint8_t *symbols = (uint8_t *)calloc(2 * n * max_steps + 1, 1), *stop = (uint8_t *)calloc(2 * n + 1, 1);
    uint64_t *steps = (uint64_t *)calloc(2 * n + 1, sizeof(uint64_t)), *sums = (uint64_t *)calloc(2 * n + 1, sizeof(uint64_t));
    rc = msbwt_rle_trace_canonical_kmers(bwt, seeds, NULL, k, 2 * n, /*min_count=*/1, /*min_edge=*/0, MSBWT_TRACE_UNITIG, MSBWT_TRACE_RIGHT, max_steps, symbols, steps,
                                         stop, sums, NULL, NULL);
    if (rc != MSBWT_OK) return fail(bwt, "trace_canonical_kmers", rc);
    for (size_t i = 0; i < 2 * n; ++i) {
        printf(">read_%zu%s steps=%llu stop=%s edge_sum=%llu\n", read_of[i / 2], i % 2 ? "_rc" : "", (unsigned long long)steps[i],
               stops[stop[i] <= MSBWT_CANONICAL_TRACE_MIRROR ? stop[i] : 0], (unsigned long long)sums[i]);
        for (size_t j = 0; j < k; ++j) putchar("ACGT"[seeds[i] >> (2 * (k - 1 - j)) & 3]);
        for (uint64_t s = 0; s < steps[i]; ++s) putchar("$ACGNT"[symbols[i * max_steps + s]]);
        putchar('\n');
    }
    uint64_t info[MSBWT_CANONICAL_TRACE_INFO_WORDS];
    if ((rc = msbwt_rle_canonical_trace_info(bwt, info)) != MSBWT_OK) return fail(bwt, "canonical_trace_info", rc);
    fprintf(stderr, "%llu walks, %llu rounds, %llu queries searched, %llu steps in all\n", (unsigned long long)info[0], (unsigned long long)info[1],
            (unsigned long long)info[2], (unsigned long long)info[3]);
    free(sums);
    free(steps);
    free(stop);
    free(symbols);
    free(codes);
    free(read_of);
    free(seeds);
    free(reads);
    free(offsets);
    msbwt_rle_free(bwt);
    return 0;
}
