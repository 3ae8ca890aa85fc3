/* C host of the canonical unitigs: loads the BWT (.npy) of a read set from both strands and prints the non-branching paths of its
 * strand-merged k-mer graph as FASTA, every sequence once -- of a unitig and its reverse complement the one with the smaller first
 * k-mer --, ascending by first k-mer.  The header line of a unitig carries its number, its nodes, the mean class abundance of its
 * k-mers (both strands together), the predecessors of its first and the successors of its last node in the printed orientation, and
 * "circular" where it closes on itself.
 *
 *   gcc -std=c11 -Iinclude examples/canonical_unitigs.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o canonical_unitigs
 *   ./canonical_unitigs reads.bwt.npy 31 2 > unitigs.fa      (k = 31, k-mers and edges seen at least twice on both strands together)
 */
#include <stdio.h>
#include <stdlib.h>

#include "msbwt_hip.h"

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

int main(int argc, char **argv) {
    const long k = argc >= 3 ? strtol(argv[2], NULL, 10) : 0, min_count = argc >= 4 ? strtol(argv[3], NULL, 10) : 1;
    if (argc < 3 || argc > 4 || argv[1][0] == '-' || k < 1 || k > 31 || min_count < 1) {
        fprintf(stderr, "usage: %s FILE.npy K [MIN_COUNT]   (1 <= K <= 31; MIN_COUNT >= 1, default 1)\n", argv[0]);
        return 2;
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_numpy_file(bwt, argv[1]);
    if (rc != MSBWT_OK) return fail(bwt, "load_numpy_file", rc);
    /* the two-call pattern: count, allocate, fill */
    uint64_t n = 0, total = 0;
    if ((rc = msbwt_rle_enumerate_canonical_unitigs(bwt, (size_t)k, (uint64_t)min_count, 0, NULL, NULL, NULL, NULL, NULL, 0, 0, &n, &total)) != MSBWT_OK)
        return fail(bwt, "enumerate_canonical_unitigs", rc);
    uint8_t *symbols = malloc(total + 1), *ends = malloc(n + 1), *flags = malloc(n + 1);
    uint64_t *offsets = malloc((n + 1) * sizeof *offsets), *sums = malloc((n + 1) * sizeof *sums);
    if (!symbols || !ends || !flags || !offsets || !sums) return 1;
    offsets[0] = 0;
    if (n && (rc = msbwt_rle_enumerate_canonical_unitigs(bwt, (size_t)k, (uint64_t)min_count, 0, symbols, offsets, sums, ends, flags, n, total, &n, &total)) != MSBWT_OK)
        return fail(bwt, "enumerate_canonical_unitigs", rc);
    uint64_t info[MSBWT_CANONICAL_UNITIG_INFO_WORDS];
    if ((rc = msbwt_rle_canonical_unitig_info(bwt, info)) != MSBWT_OK) return fail(bwt, "canonical_unitig_info", rc);
    fprintf(stderr, "%llu classes (%llu palindromes), %llu edge classes, %llu links (%llu cut): %llu unitigs (%llu circular) of %llu symbols, the longest of %llu nodes; %llu rounds\n",
            (unsigned long long)info[0], (unsigned long long)info[8], (unsigned long long)info[1], (unsigned long long)info[2], (unsigned long long)info[9],
            (unsigned long long)info[3], (unsigned long long)info[5], (unsigned long long)info[4], (unsigned long long)info[6], (unsigned long long)info[7]);
    for (uint64_t u = 0; u < n; ++u) {
        const uint64_t length = offsets[u + 1] - offsets[u], nodes = length - (uint64_t)k + 1;
        char before[5] = {0}, after[5] = {0};
        for (int j = 0, a = 0, b = 0; j < 4; ++j) {
            if ((ends[u] >> j) & 1u) before[a++] = "ACGT"[j];
            if ((ends[u] >> (4 + j)) & 1u) after[b++] = "ACGT"[j];
        }
        printf(">unitig_%llu nodes=%llu mean=%.2f in=%s out=%s%s\n", (unsigned long long)u, (unsigned long long)nodes, (double)sums[u] / (double)nodes,
               before[0] ? before : "-", after[0] ? after : "-", (flags[u] & 1u) ? " circular" : "");
        for (uint64_t i = 0; i < length; ++i) putchar("$ACGNT"[symbols[offsets[u] + i] % 6u]);
        putchar('\n');
    }
    free(symbols);
    free(ends);
    free(flags);
    free(offsets);
    free(sums);
    msbwt_rle_free(bwt);
    return 0;
}
