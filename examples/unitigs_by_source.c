/* C host of the unitigs by source: several read files in, one coloured GFA 1 out.  Builds the BWT of every input on the device (one
 * read a line over ACGTN; lines that start with '>' or '@' are skipped), merges them with their sources kept, compacts the k-mer graph
 * of the union into unitigs with the link table, and prints a segment line a unitig -- KC:i: the sum of its k-mers' counts, sc:Z: that
 * sum input by input, in the order of the files -- and a link line per edge, each edge once.  --canonical: the strand-merged graph.
 *
 *   gcc -std=c11 -Iinclude examples/unitigs_by_source.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o unitigs_by_source
 *   ./unitigs_by_source --canonical 31 2 normal.txt tumour.txt > graph.gfa     (sc:Z:0,<n> marks a unitig private to the tumour)
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
    const long k = argc >= first + 1 ? strtol(argv[first], NULL, 10) : 0, min_count = argc >= first + 2 ? strtol(argv[first + 1], NULL, 10) : 0;
    const int n_inputs = argc - first - 2;
    if (n_inputs < 2 || n_inputs > MSBWT_MERGE_MAX_INPUTS || k < 1 || k > (canonical ? 31 : 32) || min_count < 1) {
        fprintf(stderr, "usage: %s [--canonical] K MIN_COUNT READS_0.txt READS_1.txt [...]   (one read a line; 1 <= K <= 32, 31 with --canonical; MIN_COUNT >= 1; 2 to %d files)\n",
                argv[0], MSBWT_MERGE_MAX_INPUTS);
        return 2;
    }
    for (int i = 0; i < n_inputs; ++i) { /* every file is there before the device is asked for anything */
        FILE *in = fopen(argv[first + 2 + i], "r");
        if (!in) {
            perror(argv[first + 2 + i]);
            return 1;
        }
        fclose(in);
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    /* the RLE of every input, back to back */
    uint8_t *rle = NULL;
    uint64_t rle_offsets[MSBWT_MERGE_MAX_INPUTS + 1] = {0};
    int rc;
    for (int i = 0; i < n_inputs; ++i) {
        FILE *in = fopen(argv[first + 2 + i], "r");
        if (!in) {
            perror(argv[first + 2 + i]);
            return 1;
        }
        uint8_t *reads = NULL;
        uint64_t *read_offsets = NULL, length = 0;
        size_t n_reads = 0;
        if (!read_lines(in, &reads, &read_offsets, &n_reads)) return 1;
        fclose(in);
        const size_t cap = (size_t)read_offsets[n_reads] + n_reads + 1;
        if (!(rle = realloc(rle, (size_t)rle_offsets[i] + cap))) return 1;
        if (n_reads && (rc = msbwt_rle_build_from_reads(bwt, reads, read_offsets, n_reads, /*ascii=*/1, rle + rle_offsets[i], cap, &length)) != MSBWT_OK)
            return fail(bwt, "build_from_reads", rc);
        rle_offsets[i + 1] = rle_offsets[i] + length;
        free(reads);
        free(read_offsets);
    }
    if ((rc = msbwt_rle_load_merged_many_sources(bwt, rle, rle_offsets, (size_t)n_inputs)) != MSBWT_OK) return fail(bwt, "load_merged_many_sources", rc);
    free(rle);
    const uint64_t n_sources = (uint64_t)msbwt_rle_source_count(bwt);
    /* the two-call pattern: count, allocate, fill */
    int (*const call)(const msbwt_rle *, size_t, uint64_t, uint64_t, uint8_t *, uint64_t *, uint64_t *, uint8_t *, uint8_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t,
                      uint64_t, uint64_t, uint64_t *, uint64_t *, uint64_t *) =
        canonical ? msbwt_rle_enumerate_canonical_unitig_graph_by_source : msbwt_rle_enumerate_unitig_graph_by_source;
    uint64_t n = 0, total = 0, links = 0;
    if ((rc = call(bwt, (size_t)k, (uint64_t)min_count, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, &n, &total, &links)) != MSBWT_OK)
        return fail(bwt, "enumerate_unitig_graph_by_source", rc);
    uint8_t *symbols = malloc(total + 1), *flags = malloc(n + 1);
    uint64_t *offsets = malloc((n + 1) * sizeof *offsets), *sums = malloc((n + 1) * sizeof *sums);
    uint64_t *link_offsets = malloc((2 * n + 1) * sizeof *link_offsets), *targets = malloc((links + 1) * sizeof *targets);
    uint64_t *by_source = malloc((n * n_sources + 1) * sizeof *by_source);
    if (!symbols || !flags || !offsets || !sums || !link_offsets || !targets || !by_source) return 1;
    offsets[0] = link_offsets[0] = 0;
    if (n && (rc = call(bwt, (size_t)k, (uint64_t)min_count, 0, symbols, offsets, sums, NULL, flags, link_offsets, targets, by_source, n, total, links, &n, &total,
                        &links)) != MSBWT_OK)
        return fail(bwt, "enumerate_unitig_graph_by_source", rc);
    printf("H\tVN:Z:1.0\n");
    for (uint64_t u = 0; u < n; ++u) {
        printf("S\t%llu\t", (unsigned long long)u);
        for (uint64_t i = offsets[u]; i < offsets[u + 1]; ++i) putchar("$ACGNT"[symbols[i] % 6u]);
        printf("\tKC:i:%llu\tsc:Z:", (unsigned long long)sums[u]);
        for (uint64_t s = 0; s < n_sources; ++s) printf(s ? ",%llu" : "%llu", (unsigned long long)by_source[u * n_sources + s]);
        putchar('\n');
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
    fprintf(stderr, "%llu unitigs of %llu symbols over %llu inputs, %llu link entries, %llu edges written\n", (unsigned long long)n, (unsigned long long)total,
            (unsigned long long)n_sources, (unsigned long long)links, (unsigned long long)written);
    free(symbols);
    free(flags);
    free(offsets);
    free(sums);
    free(link_offsets);
    free(targets);
    free(by_source);
    msbwt_rle_free(bwt);
    return 0;
}
