/* C host of the k-mer graph: loads a BWT (.npy), prints the table of (in, out) degrees of its k-mers and the branching nodes --
 * the k-mers with more than one predecessor or more than one successor -- with the neighbours their edge bytes name.
 *
 *   gcc -std=c11 -Iinclude examples/kmer_graph.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o kmer_graph
 *   ./kmer_graph reads.bwt.npy 21 2      (k = 21, nodes and edges that occur at least twice)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

#define SHOWN 50

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

static int bits_of(unsigned x) {
    int n = 0;
    for (; x; x >>= 1) n += (int)(x & 1u);
    return n;
}

int main(int argc, char **argv) {
    const long k = argc >= 3 ? strtol(argv[2], NULL, 10) : 21, min_count = argc >= 4 ? strtol(argv[3], NULL, 10) : 1;
    if (argc < 2 || argc > 4 || argv[1][0] == '-' || k < 1 || k > 32 || min_count < 1) {
        fprintf(stderr, "usage: %s BWT.npy [K [MIN_COUNT]]   (1 <= K <= 32, default 21; MIN_COUNT >= 1, default 1)\n", argv[0]);
        return 2;
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_numpy_file(bwt, argv[1]);
    if (rc != MSBWT_OK) return fail(bwt, "load_numpy_file", rc);
    uint64_t table[25], nodes = 0, edges = 0;
    if ((rc = msbwt_rle_kmer_graph_degrees(bwt, (size_t)k, (uint64_t)min_count, 0, table, &nodes, &edges)) != MSBWT_OK) return fail(bwt, "kmer_graph_degrees", rc);
    printf("%llu nodes (%ld-mers that occur %ld times or more), %llu edges\nin\\out\t0\t1\t2\t3\t4\n", (unsigned long long)nodes, k, min_count,
           (unsigned long long)edges);
    for (int i = 0; i < 5; ++i) {
        printf("%d", i);
        for (int o = 0; o < 5; ++o) printf("\t%llu", (unsigned long long)table[5 * i + o]);
        printf("\n");
    }
    uint64_t n = 0;
    if ((rc = msbwt_rle_enumerate_kmer_graph(bwt, (size_t)k, (uint64_t)min_count, 0, NULL, NULL, NULL, NULL, 0, &n)) != MSBWT_OK)
        return fail(bwt, "enumerate_kmer_graph", rc);
    uint64_t *words = malloc((n + 1) * sizeof *words), *counts = malloc((n + 1) * sizeof *counts);
    uint8_t *bytes = malloc(n + 1);
    if (!words || !counts || !bytes) return 1;
    if (n && (rc = msbwt_rle_enumerate_kmer_graph(bwt, (size_t)k, (uint64_t)min_count, 0, words, counts, NULL, bytes, n, &n)) != MSBWT_OK)
        return fail(bwt, "enumerate_kmer_graph", rc);
    printf("branching nodes (the first %d):\nk-mer\tcount\tpredecessors\tsuccessors\n", SHOWN);
    int shown = 0;
    for (uint64_t i = 0; i < n && shown < SHOWN; ++i) {
        const unsigned in = bytes[i] & 15u, out = bytes[i] >> 4;
        if (bits_of(in) < 2 && bits_of(out) < 2) continue;
        char text[33] = {0}, before[5] = {0}, after[5] = {0};
        for (long j = 0; j < k; ++j) text[j] = "ACGT"[(words[i] >> (2 * (k - 1 - j))) & 3];
        for (int j = 0, a = 0, b = 0; j < 4; ++j) {
            if ((in >> j) & 1u) before[a++] = "ACGT"[j];
            if ((out >> j) & 1u) after[b++] = "ACGT"[j];
        }
        printf("%s\t%llu\t%s\t%s\n", text, (unsigned long long)counts[i], before[0] ? before : "-", after[0] ? after : "-");
        ++shown;
    }
    free(words);
    free(counts);
    free(bytes);
    msbwt_rle_free(bwt);
    return 0;
}
