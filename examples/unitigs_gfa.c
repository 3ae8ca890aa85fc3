/* C host of the unitig links: reads in, GFA 1 out.  Builds the BWT of the reads on the device (one read a line over ACGTN; lines that
 * start with '>' or '@' are skipped, so a FASTA with unwrapped sequences will do), compacts its k-mer graph into unitigs WITH the link
 * table of the compacted graph, and prints a segment line a unitig -- KC:i: is the sum of its k-mers' counts -- and a link line per
 * edge, each edge once, k - 1 symbols of overlap.  --canonical: the strand-merged graph, a unitig and its reverse complement as one.
 *
 *   gcc -std=c11 -Iinclude examples/unitigs_gfa.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o unitigs_gfa
 *   ./unitigs_gfa --canonical reads.txt 31 2 > graph.gfa      (k = 31, k-mers and edges seen at least twice on both strands together)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

/* all lines of `in` that are reads, back to back, and where each starts; 0 when memory runs out */
static int read_lines(FILE *in, uint8_t **reads, uint64_t **offsets, size_t *n) {
    size_t cap = 1 << 16, cap_n = 1 << 10, used = 0, line_start = 0;
    int skip = 0, at_start = 1, c;
    *reads = malloc(cap);
    *offsets = malloc(cap_n * sizeof **offsets);
    *n = 0;
    if (!*reads || !*offsets) return 0;
    (*offsets)[0] = 0;
    while ((c = fgetc(in)) != EOF) {
        if (c == '\n') {
            if (!skip && used > line_start) {
                if (*n + 3 > cap_n && !(*offsets = realloc(*offsets, (cap_n *= 2) * sizeof **offsets))) return 0;
                (*offsets)[++*n] = used;
            }
            line_start = used, skip = 0, at_start = 1;
            continue;
        }
        if (at_start && (c == '>' || c == '@')) skip = 1;
        at_start = 0;
        if (skip || c == '\r') continue;
        if (used + 1 > cap && !(*reads = realloc(*reads, cap *= 2))) return 0;
        (*reads)[used++] = (uint8_t)c;
    }
    if (!skip && used > line_start) (*offsets)[++*n] = used; /* (room for it was made with the line before) */
    return 1;
}

int main(int argc, char **argv) {
    const int canonical = argc >= 2 && strcmp(argv[1], "--canonical") == 0, first = canonical ? 2 : 1;
    const long k = argc >= first + 2 ? strtol(argv[first + 1], NULL, 10) : 0, min_count = argc >= first + 3 ? strtol(argv[first + 2], NULL, 10) : 1;
    if (argc < first + 2 || argc > first + 3 || (argv[first][0] == '-' && argv[first][1]) || k < 1 || k > (canonical ? 31 : 32) || min_count < 1) {
        fprintf(stderr, "usage: %s [--canonical] READS.txt|- K [MIN_COUNT]   (one read a line; 1 <= K <= 32, 31 with --canonical; MIN_COUNT >= 1, default 1)\n", argv[0]);
        return 2;
    }
    FILE *in = strcmp(argv[first], "-") == 0 ? stdin : fopen(argv[first], "r");
    if (!in) {
        perror(argv[first]);
        return 1;
    }
    uint8_t *reads = NULL;
    uint64_t *read_offsets = NULL;
    size_t n_reads = 0;
    if (!read_lines(in, &reads, &read_offsets, &n_reads)) return 1;
    if (in != stdin) fclose(in);
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_reads(bwt, reads, read_offsets, n_reads, /*ascii=*/1);
    if (rc != MSBWT_OK) return fail(bwt, "load_reads", rc);
    free(reads);
    free(read_offsets);
    /* the two-call pattern: count, allocate, fill */
    int (*const call)(const msbwt_rle *, size_t, uint64_t, uint64_t, uint8_t *, uint64_t *, uint64_t *, uint8_t *, uint8_t *, uint64_t *, uint64_t *, uint64_t, uint64_t,
                      uint64_t, uint64_t *, uint64_t *, uint64_t *) = canonical ? msbwt_rle_enumerate_canonical_unitig_graph : msbwt_rle_enumerate_unitig_graph;
    uint64_t n = 0, total = 0, links = 0;
    if ((rc = call(bwt, (size_t)k, (uint64_t)min_count, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, &n, &total, &links)) != MSBWT_OK)
        return fail(bwt, "enumerate_unitig_graph", rc);
    uint8_t *symbols = malloc(total + 1), *flags = malloc(n + 1);
    uint64_t *offsets = malloc((n + 1) * sizeof *offsets), *sums = malloc((n + 1) * sizeof *sums);
    uint64_t *link_offsets = malloc((2 * n + 1) * sizeof *link_offsets), *targets = malloc((links + 1) * sizeof *targets);
    if (!symbols || !flags || !offsets || !sums || !link_offsets || !targets) return 1;
    offsets[0] = link_offsets[0] = 0;
    if (n && (rc = call(bwt, (size_t)k, (uint64_t)min_count, 0, symbols, offsets, sums, NULL, flags, link_offsets, targets, n, total, links, &n, &total, &links)) != MSBWT_OK)
        return fail(bwt, "enumerate_unitig_graph", rc);
    printf("H\tVN:Z:1.0\n");
    for (uint64_t u = 0; u < n; ++u) {
        printf("S\t%llu\t", (unsigned long long)u);
        for (uint64_t i = offsets[u]; i < offsets[u + 1]; ++i) putchar("$ACGNT"[symbols[i] % 6u]);
        printf("\tKC:i:%llu\n", (unsigned long long)sums[u]);
    }
    /* side a holds entry e; the same edge from its other end is (e ^ 1, a ^ 1), with bit 0 cleared for a unitig that is its own reverse
     * complement (flag bit 1): the record that is not above its mirror is printed */
    uint64_t written = 0;
    for (uint64_t a = 0; a < 2 * n; ++a)
        for (uint64_t i = link_offsets[a]; i < link_offsets[a + 1]; ++i) {
            const uint64_t e = targets[i];
            const uint64_t mirror_side = (flags[e >> 1] & 2u) ? (e ^ 1u) & ~(uint64_t)1 : e ^ 1u, mirror_entry = (flags[a >> 1] & 2u) ? (a ^ 1u) & ~(uint64_t)1 : a ^ 1u;
            if (a > mirror_side || (a == mirror_side && e > mirror_entry)) continue;
            printf("L\t%llu\t%c\t%llu\t%c\t%ldM\n", (unsigned long long)(a >> 1), (a & 1u) ? '-' : '+', (unsigned long long)(e >> 1), (e & 1u) ? '-' : '+', k - 1);
            ++written;
        }
    fprintf(stderr, "%llu unitigs of %llu symbols, %llu link entries, %llu edges written\n", (unsigned long long)n, (unsigned long long)total, (unsigned long long)links,
            (unsigned long long)written);
    free(symbols);
    free(flags);
    free(offsets);
    free(sums);
    free(link_offsets);
    free(targets);
    msbwt_rle_free(bwt);
    return 0;
}
