/* C host of the spectrum and the k-mer dump: loads a BWT (.npy), prints the abundance histogram of its k-mers and the ten most
 * abundant ones.  The histogram says from which count on there are only ten k-mers left; the dump with that min_count fetches
 * exactly those -- the walk prunes everything rarer.
 *
 *   gcc -std=c11 -Iinclude examples/kmer_spectrum.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o kmer_spectrum
 *   ./kmer_spectrum reads.bwt.npy 21
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

#define BINS 65536
#define TOP 10

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

int main(int argc, char **argv) {
    const long k = argc == 3 ? strtol(argv[2], NULL, 10) : 21;
    if (argc < 2 || argc > 3 || argv[1][0] == '-' || k < 1 || k > 32) {
        fprintf(stderr, "usage: %s BWT.npy [K]   (1 <= K <= 32, default 21)\n", argv[0]);
        return 2;
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_numpy_file(bwt, argv[1]);
    if (rc != MSBWT_OK) return fail(bwt, "load_numpy_file", rc);
    uint64_t *hist = calloc(BINS, sizeof *hist), distinct = 0, occurrences = 0;
    if (!hist) return 1;
    if ((rc = msbwt_rle_kmer_spectrum(bwt, (size_t)k, hist, BINS, &distinct, &occurrences)) != MSBWT_OK) return fail(bwt, "kmer_spectrum", rc);
    printf("%llu distinct %ld-mers, %llu occurrences\ncount\tk-mers\n", (unsigned long long)distinct, k, (unsigned long long)occurrences);
    for (size_t c = 1; c < BINS; ++c)
        if (hist[c]) printf("%s%zu\t%llu\n", c == BINS - 1 ? ">=" : "", c, (unsigned long long)hist[c]);
    /* the smallest count with at most TOP k-mers at or above it (the most abundant bin is taken whatever it holds) */
    uint64_t above = 0, least = BINS - 1;
    for (size_t c = BINS - 1; c >= 1 && !(above && above + hist[c] > TOP); --c) {
        above += hist[c];
        least = c;
    }
    uint64_t n = 0;
    if ((rc = msbwt_rle_enumerate_kmers(bwt, (size_t)k, least, 0, 0, NULL, NULL, NULL, 0, &n)) != MSBWT_OK) return fail(bwt, "enumerate_kmers", rc);
    uint64_t *words = malloc((n + 1) * sizeof *words), *counts = malloc((n + 1) * sizeof *counts);
    if (!words || !counts) return 1;
    if (n && (rc = msbwt_rle_enumerate_kmers(bwt, (size_t)k, least, 0, 0, words, counts, NULL, n, &n)) != MSBWT_OK) return fail(bwt, "enumerate_kmers", rc);
    printf("most abundant (count >= %llu):\n", (unsigned long long)least);
    for (int shown = 0; shown < TOP && (uint64_t)shown < n; ++shown) {
        uint64_t best = shown;
        for (uint64_t i = shown + 1; i < n; ++i)
            if (counts[i] > counts[best]) best = i;
        const uint64_t w = words[best], c = counts[best];
        words[best] = words[shown];
        counts[best] = counts[shown];
        words[shown] = w;
        counts[shown] = c;
        char text[33] = {0};
        for (long i = 0; i < k; ++i) text[i] = "ACGT"[(w >> (2 * (k - 1 - i))) & 3];
        printf("%s\t%llu\n", text, (unsigned long long)c);
    }
    free(words);
    free(counts);
    free(hist);
    msbwt_rle_free(bwt);
    return 0;
}
