/* A plain-C translation unit over the one-pass merge entry points of include/msbwt_hip.h: it must compile as C11 with the declared
 * signatures, and its guards answer without a device.  Prints one line per check; exit status 0 when all hold. */
#include <stdio.h>
#include <string.h>

#include "msbwt_hip.h"

static int (*const merge_fn)(msbwt_rle *, const uint8_t *, const uint64_t *, size_t, uint8_t *, size_t, uint64_t *, uint8_t *) = msbwt_rle_merge_many;
static int (*const load_fn)(msbwt_rle *, const uint8_t *, const uint64_t *, size_t) = msbwt_rle_load_merged_many;
static int (*const plan_fn)(const uint64_t *, size_t, uint64_t *) = msbwt_merge_many_plan;
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
    /* three inputs: "AAA$", "$", "CC"; then the same with code 6 in input 2 */
    const uint8_t ok[4] = {1 | 3 << 3, 0 | 1 << 3, 0 | 1 << 3, 2 | 2 << 3}, bad[4] = {1 | 3 << 3, 0 | 1 << 3, 0 | 1 << 3, 6 | 2 << 3};
    const uint64_t three[4] = {0, 2, 3, 4}, decreasing[4] = {0, 3, 2, 4};
    uint64_t many[MSBWT_MERGE_MAX_INPUTS + 2];
    memset(many, 0, sizeof many);
    uint8_t halves[24]; /* 2^39 'A' = digit 16 at 32^7, an empty input, 2^39 'A' */
    memset(halves, 1, sizeof halves);
    halves[7] = halves[15] = 1 | 16 << 3;
    const uint64_t halves_at[4] = {0, 8, 8, 16};
    uint8_t out[16];
    memset(out, 0xAB, sizeof out);
    uint64_t len = 77, iterations = 77;
    double ms[MSBWT_MERGE_STAGES];
    expect("null handle", merge_fn(NULL, ok, three, 3, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("load: null handle", load_fn(NULL, ok, three, 3), MSBWT_ERR_INVALID_ARG);
    expect("33 inputs", merge_fn(bwt, ok, many, MSBWT_MERGE_MAX_INPUTS + 1, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("load: 33 inputs", load_fn(bwt, ok, many, MSBWT_MERGE_MAX_INPUTS + 1), MSBWT_ERR_INVALID_ARG);
    expect("decreasing offsets", merge_fn(bwt, ok, decreasing, 3, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("load: decreasing offsets", load_fn(bwt, ok, decreasing, 3), MSBWT_ERR_INVALID_ARG);
    expect("null rle with bytes", merge_fn(bwt, NULL, three, 3, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("load: null rle with bytes", load_fn(bwt, NULL, three, 3), MSBWT_ERR_INVALID_ARG);
    expect("null offsets with inputs", merge_fn(bwt, ok, NULL, 3, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("null out_len", merge_fn(bwt, ok, three, 3, out, sizeof out, NULL, NULL), MSBWT_ERR_INVALID_ARG);
    expect("null out_rle with a capacity", merge_fn(bwt, ok, three, 3, NULL, sizeof out, &len, NULL), MSBWT_ERR_INVALID_ARG);
    expect("code 6 in input 2 of 3", merge_fn(bwt, bad, three, 3, out, sizeof out, &len, NULL), MSBWT_ERR_INVALID_SYMBOL);
    expect("the message names the input", strstr(msbwt_rle_last_error(bwt), "input 2") != NULL, 1);
    expect("load: code 6 in input 2 of 3", load_fn(bwt, bad, three, 3), MSBWT_ERR_INVALID_SYMBOL);
    expect("2^39 + 0 + 2^39 symbols", merge_fn(bwt, halves, halves_at, 3, out, sizeof out, &len, NULL), MSBWT_ERR_TOO_LARGE);
    expect("load: 2^39 + 0 + 2^39 symbols", load_fn(bwt, halves, halves_at, 3), MSBWT_ERR_TOO_LARGE);
    expect("an error message is kept", strlen(msbwt_rle_last_error(bwt)) > 0, 1);
    expect("nothing was written", out[0] == 0xAB && out[15] == 0xAB, 1);
    len = 77;
    expect("no input: the empty BWT", merge_fn(bwt, NULL, NULL, 0, out, sizeof out, &len, NULL), MSBWT_OK);
    expect("no input: zero bytes", (int)len, 0);
    len = 77;
    expect("32 empty inputs: the empty BWT", merge_fn(bwt, NULL, many, MSBWT_MERGE_MAX_INPUTS, out, sizeof out, &len, out), MSBWT_OK);
    expect("32 empty inputs: zero bytes", (int)len, 0);
    expect("info", info_fn(bwt, &iterations, ms), MSBWT_OK);
    expect("info: no iterations", (int)iterations, 0);
    uint64_t bytes = 0;
    const uint64_t totals[3] = {1000000, 0, 2000000}, big[3] = {(uint64_t)1 << 39, 0, (uint64_t)1 << 39}, below[3] = {((uint64_t)1 << 39) - 1, 0, (uint64_t)1 << 39};
    expect("plan", plan_fn(totals, 3, &bytes), MSBWT_OK);
    expect("plan: between 2 and 3.25 bytes per symbol and 64 MiB", bytes >= 6000000 && bytes <= 9750000 + ((uint64_t)64 << 20), 1);
    expect("plan: 2^40 symbols", plan_fn(big, 3, &bytes), MSBWT_ERR_TOO_LARGE);
    expect("plan: just below", plan_fn(below, 3, NULL), MSBWT_OK);
    expect("plan: 33 inputs", plan_fn(many, MSBWT_MERGE_MAX_INPUTS + 1, &bytes), MSBWT_ERR_INVALID_ARG);
    expect("plan: no input", plan_fn(NULL, 0, &bytes), MSBWT_OK);
    msbwt_rle_free(bwt);
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
