/* A plain-C translation unit over the construction entry points of include/msbwt_hip.h: it must compile as C11 with the
 * declared signatures, and its guards answer without a device.  Prints one line per check; exit status 0 when all hold. */
#include <stdio.h>
#include <string.h>

#include "msbwt_hip.h"

static int (*const build_fn)(msbwt_rle *, const uint8_t *, const uint64_t *, size_t, int, uint8_t *, size_t, uint64_t *) = msbwt_rle_build_from_reads;
static int (*const load_fn)(msbwt_rle *, const uint8_t *, const uint64_t *, size_t, int) = msbwt_rle_load_reads;
static int (*const piece_fn)(msbwt_rle *, uint64_t) = msbwt_rle_set_build_piece;
static int (*const plan_fn)(uint64_t, uint64_t, uint64_t, uint64_t *, uint64_t *) = msbwt_build_reads_plan;

static int checks = 0, failures = 0;
static void expect(const char *what, int got, int want) {
    ++checks;
    if (got != want) ++failures;
    printf("%s: %d (expected %d)%s\n", what, got, want, got == want ? "" : "  <-- MISMATCH");
}

int main(void) {
    msbwt_rle *bwt = msbwt_rle_new_on_device(8, 0);
    if (!bwt) return 1;
    const uint8_t codes[6] = {1, 2, 3, 5, 4, 1}, zero[3] = {1, 0, 2}, six[3] = {1, 6, 2};
    const uint64_t offsets[3] = {0, 4, 6}, decreasing[3] = {0, 4, 2}, one[2] = {0, 3};
    uint8_t out[16];
    uint64_t len = 77;
    expect("null handle", build_fn(NULL, codes, offsets, 2, 0, out, sizeof out, &len), MSBWT_ERR_INVALID_ARG);
    expect("null reads", build_fn(bwt, NULL, offsets, 2, 0, out, sizeof out, &len), MSBWT_ERR_INVALID_ARG);
    expect("null offsets", build_fn(bwt, codes, NULL, 2, 0, out, sizeof out, &len), MSBWT_ERR_INVALID_ARG);
    expect("null out_len", build_fn(bwt, codes, offsets, 2, 0, out, sizeof out, NULL), MSBWT_ERR_INVALID_ARG);
    expect("decreasing offsets", build_fn(bwt, codes, decreasing, 2, 0, out, sizeof out, &len), MSBWT_ERR_INVALID_ARG);
    expect("code 0", build_fn(bwt, zero, one, 1, 0, out, sizeof out, &len), MSBWT_ERR_INVALID_SYMBOL);
    expect("code 6", build_fn(bwt, six, one, 1, 0, out, sizeof out, &len), MSBWT_ERR_INVALID_SYMBOL);
    expect("'$' in ASCII mode", build_fn(bwt, (const uint8_t *)"AC$", one, 1, 1, out, sizeof out, &len), MSBWT_ERR_INVALID_SYMBOL);
    expect("load: decreasing offsets", load_fn(bwt, codes, decreasing, 2, 0), MSBWT_ERR_INVALID_ARG);
    expect("load: code 6", load_fn(bwt, six, one, 1, 0), MSBWT_ERR_INVALID_SYMBOL);
    expect("an error message is kept", strlen(msbwt_rle_last_error(bwt)) > 0, 1);
    len = 77;
    expect("no reads: the empty BWT", build_fn(bwt, NULL, NULL, 0, 0, out, sizeof out, &len), MSBWT_OK);
    expect("no reads: zero bytes", (int)len, 0);
    expect("set_build_piece", piece_fn(bwt, 1000), MSBWT_OK);
    expect("set_build_piece, null handle", piece_fn(NULL, 1000), MSBWT_ERR_INVALID_ARG);
    uint64_t piece = 0, bytes = 0;
    expect("plan", plan_fn(1000000, (uint64_t)1 << 34, 0, &piece, &bytes), MSBWT_OK);
    expect("plan: a piece", piece >= 1, 1);
    expect("plan: at least two bytes per symbol", bytes >= 2000000, 1);
    expect("plan: 2^40 symbols", plan_fn((uint64_t)1 << 40, (uint64_t)1 << 38, 0, &piece, &bytes), MSBWT_ERR_TOO_LARGE);
    msbwt_rle_free(bwt);
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
