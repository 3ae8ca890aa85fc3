/* C host of the canonical spectrum and dump: loads a BWT (.npy) of reads from both strands and prints the abundance histogram of its
 * k-mers with a k-mer and its reverse complement counted as one, then the solid classes (count >= MIN) with their counts per strand.
 * A class seen once on each strand has count 2: msbwt_rle_enumerate_kmers with min_count 2 would drop both of its k-mers.
 *
 *   gcc -std=c11 -Iinclude examples/canonical_spectrum.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o canonical_spectrum
 *   ./canonical_spectrum reads.bwt.npy 21 2
 */
#include <stdio.h>
#include <stdlib.h>

#include "msbwt_hip.h"

#define BINS 65536
#define SHOWN 20

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

int main(int argc, char **argv) {
    const long k = argc >= 3 ? strtol(argv[2], NULL, 10) : 21, least = argc == 4 ? strtol(argv[3], NULL, 10) : 2;
    if (argc < 2 || argc > 4 || argv[1][0] == '-' || k < 1 || k > 32 || least < 1) {
        fprintf(stderr, "usage: %s BWT.npy [K [MIN]]   (1 <= K <= 32, default 21; MIN >= 1, default 2)\n", argv[0]);
        return 2;
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_numpy_file(bwt, argv[1]);
    if (rc != MSBWT_OK) return fail(bwt, "load_numpy_file", rc);
    uint64_t *hist = calloc(BINS, sizeof *hist), classes = 0, occurrences = 0;
    if (!hist) return 1;
    if ((rc = msbwt_rle_canonical_kmer_spectrum(bwt, (size_t)k, hist, BINS, &classes, &occurrences)) != MSBWT_OK) return fail(bwt, "canonical_kmer_spectrum", rc);
    printf("%llu canonical %ld-mers, %llu occurrences on both strands\ncount\tclasses\n", (unsigned long long)classes, k, (unsigned long long)occurrences);
    for (size_t c = 1; c < BINS; ++c)
        if (hist[c]) printf("%s%zu\t%llu\n", c == BINS - 1 ? ">=" : "", c, (unsigned long long)hist[c]);
    uint64_t n = 0;
    if ((rc = msbwt_rle_enumerate_canonical_kmers(bwt, (size_t)k, (uint64_t)least, 0, NULL, NULL, NULL, 0, &n)) != MSBWT_OK)
        return fail(bwt, "enumerate_canonical_kmers", rc);
    uint64_t *words = malloc((n + 1) * sizeof *words), *own = malloc((n + 1) * sizeof *own), *other = malloc((n + 1) * sizeof *other);
    if (!words || !own || !other) return 1;
    if (n && (rc = msbwt_rle_enumerate_canonical_kmers(bwt, (size_t)k, (uint64_t)least, 0, words, own, other, n, &n)) != MSBWT_OK)
        return fail(bwt, "enumerate_canonical_kmers", rc);
    printf("%llu classes with count >= %ld; the first %d in the order of the walk:\nk-mer\tas written\treverse complement\n", (unsigned long long)n, least, SHOWN);
    for (uint64_t i = 0; i < n && i < SHOWN; ++i) {
        char text[33] = {0};
        for (long j = 0; j < k; ++j) text[j] = "ACGT"[(words[i] >> (2 * (k - 1 - j))) & 3];
        printf("%s\t%llu\t%llu\n", text, (unsigned long long)own[i], (unsigned long long)other[i]);
    }
    free(words);
    free(own);
    free(other);
    free(hist);
    msbwt_rle_free(bwt);
    return 0;
}
