/* C host of the bridges: a one-pass substitution corrector.  The reads given on the command line are loaded as an index and every k-mer
 * of every read is counted with the fused call.  A WEAK STRETCH is a maximal run of k-mers of a read below MIN_COUNT that has a solid
 * k-mer on both sides; with L k-mers in it, the solid k-mer behind it starts D = L + 1 symbols behind the one before it.  The two
 * flanks of every stretch go to msbwt_rle_bridge_kmers as one batch, each with the window of lengths D - D/10 .. D + D/10, which is the
 * widest of the batch (the call takes one window), and the report says per stretch how the exploration stopped and what it found.
 * Where exactly one bridge of the stretch's own length D exists, its symbols replace the read's, and the corrected read is printed.
 *
 *   gcc -std=c11 -Iinclude examples/bridge_kmers.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o bridge_kmers
 *   ./bridge_kmers 5 2 ACGTTGCATTAGGCA ACGTTGCATTAGGCA ACGTTGCCTTAGGCA
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

#define MAX_PATHS 4
#define MAX_LIVE 64

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

int main(int argc, char **argv) {
    static const char *const stops[] = {"", "EXHAUSTED", "FULL", "MAX_STEPS", "TOO_WIDE", "NO_SEED", "NO_TARGET", ""};
    char *end = NULL, *end2 = NULL;
    const unsigned long k_arg = argc >= 4 ? strtoul(argv[1], &end, 10) : 0, m_arg = argc >= 4 ? strtoul(argv[2], &end2, 10) : 0;
    if (argc < 4 || *end || *end2 || k_arg < 1 || k_arg > 31 || m_arg < 1) {
        fprintf(stderr, "usage: %s K MIN_COUNT READ [READ...]   (1 <= K <= 31, MIN_COUNT >= 1, reads over ACGTN)\n", argv[0]);
        return 2;
    }
    const size_t k = (size_t)k_arg, n_reads = (size_t)(argc - 3);
    const uint64_t min_count = (uint64_t)m_arg;
    uint64_t *offsets = (uint64_t *)calloc(n_reads + 1, sizeof(uint64_t));
    for (size_t r = 0; r < n_reads; ++r) offsets[r + 1] = offsets[r] + strlen(argv[3 + r]);
    uint8_t *reads = (uint8_t *)malloc(offsets[n_reads] + 1);
    for (size_t r = 0; r < n_reads; ++r) memcpy(reads + offsets[r], argv[3 + r], (size_t)(offsets[r + 1] - offsets[r]));

    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_reads(bwt, reads, offsets, n_reads, /*ascii=*/1);
    if (rc != MSBWT_OK) return fail(bwt, "load_reads", rc);

    /* every k-mer of every read, counted */
    uint64_t windows = 0;
    if ((rc = msbwt_rle_count_ragged_read_kmers(bwt, reads, offsets, n_reads, k, 1, NULL, NULL, &windows)) != MSBWT_OK) return fail(bwt, "count_ragged_read_kmers", rc);
    uint64_t *counts = (uint64_t *)calloc(windows + 1, sizeof(uint64_t));
    if ((rc = msbwt_rle_count_ragged_read_kmers(bwt, reads, offsets, n_reads, k, 1, counts, NULL, NULL)) != MSBWT_OK) return fail(bwt, "count_ragged_read_kmers", rc);

    /* the weak stretches: at most one every two k-mers */
    uint64_t *seeds = (uint64_t *)calloc(windows / 2 + 1, sizeof(uint64_t)), *targets = (uint64_t *)calloc(windows / 2 + 1, sizeof(uint64_t));
    uint64_t *read_of = (uint64_t *)calloc(windows / 2 + 1, sizeof(uint64_t)), *at = (uint64_t *)calloc(windows / 2 + 1, sizeof(uint64_t));
    uint64_t *own = (uint64_t *)calloc(windows / 2 + 1, sizeof(uint64_t));
    uint8_t *codes = (uint8_t *)malloc(k);
    size_t n = 0;
    uint64_t longest = 0, first_window = 0;
    for (size_t r = 0; r < n_reads; ++r) {
        const uint64_t len = offsets[r + 1] - offsets[r], w = len >= k ? len - k + 1 : 0;
        const uint64_t *c = counts + first_window;
        for (uint64_t i = 1; i < w; ++i) {
            if (c[i] >= min_count || c[i - 1] < min_count) continue; /* i: the first k-mer of a stretch behind a solid one */
            uint64_t j = i;
            while (j < w && c[j] < min_count) ++j;
            if (j == w) break; /* no solid k-mer behind it */
            msbwt_convert_stoi(reads + offsets[r] + i - 1, k, codes);
            msbwt_kmers_pack_2bit(codes, k, 1, seeds + n); /* (a solid k-mer holds no N) */
            msbwt_convert_stoi(reads + offsets[r] + j, k, codes);
            msbwt_kmers_pack_2bit(codes, k, 1, targets + n);
            read_of[n] = r;
            at[n] = i - 1;
            own[n] = j - i + 1;
            if (own[n] > longest) longest = own[n];
            ++n;
            i = j;
        }
        first_window += w;
    }
    printf("%zu reads, %llu k-mers, %zu weak stretches between solid k-mers\n", n_reads, (unsigned long long)windows, n);

    /* one batch: the window around the longest stretch holds every stretch's own length */
    uint64_t max_steps = longest + longest / 10, min_steps = 0;
    if (max_steps > MSBWT_BRIDGE_MAX_STEPS_CAP) max_steps = MSBWT_BRIDGE_MAX_STEPS_CAP;
    for (size_t i = 0; i < n; ++i)
        if (i == 0 || own[i] - own[i] / 10 < min_steps) min_steps = own[i] - own[i] / 10;
    uint8_t *symbols = (uint8_t *)calloc(n * MAX_PATHS * max_steps + 1, 1), *stop = (uint8_t *)calloc(n + 1, 1);
    uint64_t *lengths = (uint64_t *)calloc(n * MAX_PATHS + 1, sizeof(uint64_t)), *found = (uint64_t *)calloc(n + 1, sizeof(uint64_t));
    uint64_t *depths = (uint64_t *)calloc(n + 1, sizeof(uint64_t));
    rc = msbwt_rle_bridge_kmers(bwt, seeds, targets, k, n, min_count, /*min_edge=*/0, MSBWT_BRIDGE_RIGHT, min_steps, max_steps, MAX_PATHS, MAX_LIVE, symbols, lengths, NULL,
                                found, stop, depths, NULL);
    if (rc != MSBWT_OK) return fail(bwt, "bridge_kmers", rc);
    uint8_t *corrected = (uint8_t *)malloc(offsets[n_reads] + 1);
    uint8_t *changed = (uint8_t *)calloc(n_reads + 1, 1);
    memcpy(corrected, reads, offsets[n_reads]);
    for (size_t i = 0; i < n; ++i) {
        /* the bridges of the stretch's own length: all of them are known once the exploration has reached that length and lost no row */
        size_t same = 0, which = 0;
        for (size_t j = 0; j < MAX_PATHS; ++j)
            if (lengths[i * MAX_PATHS + j] == own[i]) {
                ++same;
                which = j;
            }
        const int sure = same == 1 && found[i] <= MAX_PATHS && depths[i] >= own[i];
        printf("read_%llu stretch at %llu, %llu steps: stop=%s found=%llu depth=%llu%s\n", (unsigned long long)read_of[i], (unsigned long long)at[i],
               (unsigned long long)own[i], stops[stop[i] & 7], (unsigned long long)found[i], (unsigned long long)depths[i], sure ? " corrected" : "");
        if (!sure) continue;
        uint8_t *to = corrected + offsets[read_of[i]] + at[i] + k;
        const uint8_t *row = symbols + (i * MAX_PATHS + which) * max_steps;
        for (uint64_t s = 0; s < own[i]; ++s) to[s] = (uint8_t)"$ACGNT"[row[s]];
        changed[read_of[i]] = 1;
    }
    for (size_t r = 0; r < n_reads; ++r)
        if (changed[r]) printf(">read_%zu corrected\n%.*s\n", r, (int)(offsets[r + 1] - offsets[r]), (const char *)corrected + offsets[r]);
    uint64_t info[MSBWT_BRIDGE_INFO_WORDS];
    if ((rc = msbwt_rle_bridge_info(bwt, info)) != MSBWT_OK) return fail(bwt, "bridge_info", rc);
    fprintf(stderr, "%llu pairs, %llu rounds, %llu queries searched, %llu walk-steps expanded, %llu bridges found\n", (unsigned long long)info[0],
            (unsigned long long)info[1], (unsigned long long)info[2], (unsigned long long)info[3], (unsigned long long)info[4]);
    free(changed);
    free(corrected);
    free(depths);
    free(found);
    free(lengths);
    free(stop);
    free(symbols);
    free(codes);
    free(own);
    free(at);
    free(read_of);
    free(targets);
    free(seeds);
    free(counts);
    free(reads);
    free(offsets);
    msbwt_rle_free(bwt);
    return 0;
}
