/* A plain-C translation unit over the merge entry points of include/msbwt_hip.h: it must compile as C11 with the declared
 * signatures, and its guards answer without a device.  Prints one line per check; exit status 0 when all hold. */
#include <stdio.h>
#include <string.h>

#include "msbwt_hip.h"

static int (*const merge_fn)(msbwt_rle *, const uint8_t *, size_t, const uint8_t *, size_t, uint8_t *, size_t, uint64_t *, uint8_t *) = msbwt_rle_merge;
static int (*const load_fn)(msbwt_rle *, const uint8_t *, size_t, const uint8_t *, size_t) = msbwt_rle_load_merged;
static int (*const plan_fn)(uint64_t, uint64_t, uint64_t *) = msbwt_merge_plan;
static size_t (*const tile_fn)(void) = msbwt_merge_tile;
static int (*const info_fn)(const msbwt_rle *, uint64_t *, double *) = msbwt_rle_merge_info;

static int checks = 0, failures = 0;
static void expect(const char *what, int got, int want) {
    ++checks;
    if (got != want) ++failures;
    printf("%s: %d (expected %d)%s\n", what, got, want, got == want ? "" : "  <-- MISMATCH");
}

int main(void) {
    msbwt_rle *bwt = msbwt_rle_new_on_device(8, 0);
    if (!bwt) return 1;
    const uint8_t ok[2] = {1 | 3 << 3, 0 | 1 << 3}, six[2] = {1 | 1 << 3, 6 | 1 << 3}, seven[1] = {7 | 2 << 3};
    uint8_t huge[9], half[8]; /* 32^9 - 1 'A'; 2^39 'A' = digit 16 at 32^7 */
    memset(huge, 0xF9, sizeof huge);
    memset(half, 1, sizeof half);
    half[7] = 1 | 16 << 3;
    uint8_t out[16];
    uint64_t len = 77, iterations = 77;
    double ms[MSBWT_MERGE_STAGES];
    expect("null handle", merge_fn(NULL, ok, 2, ok, 2, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("load: null handle", load_fn(NULL, ok, 2, ok, 2), MSBWT_ERR_INVALID_ARG);
    expect("info: null handle", info_fn(NULL, &iterations, ms), MSBWT_ERR_INVALID_ARG);
    expect("null out_len", merge_fn(bwt, ok, 2, ok, 2, out, sizeof out, NULL, NULL), MSBWT_ERR_INVALID_ARG);
    expect("null first input with a length", merge_fn(bwt, NULL, 2, ok, 2, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("null second input with a length", merge_fn(bwt, ok, 2, NULL, 2, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("load: null input with a length", load_fn(bwt, ok, 2, NULL, 2), MSBWT_ERR_INVALID_ARG);
    expect("code 6 in the first input", merge_fn(bwt, six, 2, ok, 2, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_SYMBOL);
    expect("code 6 in the second input", merge_fn(bwt, ok, 2, six, 2, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_SYMBOL);
    expect("code 7 in the first input", merge_fn(bwt, seven, 1, ok, 2, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_SYMBOL);
    expect("code 7 in the second input", merge_fn(bwt, ok, 2, seven, 1, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_SYMBOL);
    expect("load: code 6", load_fn(bwt, ok, 2, six, 2), MSBWT_ERR_INVALID_SYMBOL);
    expect("a run of 32^9 - 1", merge_fn(bwt, huge, sizeof huge, ok, 2, out, sizeof out, &len, NULL), MSBWT_ERR_TOO_LARGE);
    expect("a run of 32^9 - 1, second", merge_fn(bwt, NULL, 0, huge, sizeof huge, out, sizeof out, &len, NULL), MSBWT_ERR_TOO_LARGE);
    expect("2^39 + 2^39 symbols", merge_fn(bwt, half, sizeof half, half, sizeof half, out, sizeof out, &len, NULL), MSBWT_ERR_TOO_LARGE);
    expect("load: 2^39 + 2^39 symbols", load_fn(bwt, half, sizeof half, half, sizeof half), MSBWT_ERR_TOO_LARGE);
    expect("an error message is kept", strlen(msbwt_rle_last_error(bwt)) > 0, 1);
    len = 77;
    expect("two empty inputs: the empty BWT", merge_fn(bwt, NULL, 0, NULL, 0, out, sizeof out, &len, NULL), MSBWT_OK);
    expect("two empty inputs: zero bytes", (int)len, 0);
    expect("info", info_fn(bwt, &iterations, ms), MSBWT_OK);
    expect("info: no iterations yet", (int)iterations, 0);
    expect("info: either output may be null", info_fn(bwt, NULL, NULL), MSBWT_OK);
    uint64_t bytes = 0;
    expect("plan", plan_fn(1000000, 2000000, &bytes), MSBWT_OK);
    expect("plan: at most 2.5 bytes per symbol and 64 MiB", bytes >= 3000000 && bytes <= 7500000 + ((uint64_t)64 << 20), 1);
    expect("plan: 2^40 symbols", plan_fn((uint64_t)1 << 39, (uint64_t)1 << 39, &bytes), MSBWT_ERR_TOO_LARGE);
    expect("plan: just below", plan_fn(((uint64_t)1 << 39) - 1, (uint64_t)1 << 39, NULL), MSBWT_OK);
    expect("tile", tile_fn() >= 64 && tile_fn() % 64 == 0, 1);
    msbwt_rle_free(bwt);
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
