/* C host of the one-pass merge: two or more comp_msbwt.npy files in, the BWT of the union of their read sets out, merged on the
 * GPU in one call.
 *
 *   gcc -std=c11 -Iinclude examples/merge_many_bwts.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o merge_many_bwts
 *   ./merge_many_bwts lane1/comp_msbwt.npy lane2/comp_msbwt.npy lane3/comp_msbwt.npy merged/comp_msbwt.npy
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

/* the payload of a NumPy v1.0 file of bytes, appended to *all (of *used bytes): 10 bytes of magic, version and header length, the
 * header, the RLE bytes */
static int append_npy(const char *path, uint8_t **all, size_t *used) {
    FILE *f = fopen(path, "rb");
    unsigned char head[10];
    if (!f) return 0;
    if (fread(head, 1, sizeof head, f) != sizeof head || memcmp(head, "\x93NUMPY", 6) != 0 || head[6] != 1) {
        fclose(f);
        return 0;
    }
    const long start = 10 + (long)(head[8] | head[9] << 8);
    if (fseek(f, 0, SEEK_END) != 0 || ftell(f) < start) {
        fclose(f);
        return 0;
    }
    const size_t len = (size_t)(ftell(f) - start);
    uint8_t *grown = (uint8_t *)realloc(*all, *used + len + 1);
    if (grown) *all = grown;
    const int ok = grown && fseek(f, start, SEEK_SET) == 0 && fread(grown + *used, 1, len, f) == len;
    fclose(f);
    if (ok) *used += len;
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s IN1.npy IN2.npy [IN3.npy ...] MERGED.npy\n", argv[0]);
        return 2;
    }
    const size_t n = (size_t)argc - 2;
    if (n > MSBWT_MERGE_MAX_INPUTS) {
        fprintf(stderr, "%zu inputs, one merge takes at most %d\n", n, MSBWT_MERGE_MAX_INPUTS);
        return 1;
    }
    uint8_t *rle = NULL;
    uint64_t offsets[MSBWT_MERGE_MAX_INPUTS + 1] = {0};
    size_t used = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!append_npy(argv[1 + i], &rle, &used)) {
            fprintf(stderr, "cannot read %s\n", argv[1 + i]);
            return 1;
        }
        offsets[i + 1] = used;
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    size_t cap = used; /* enough for canonical inputs; the call says what it needs otherwise */
    uint8_t *out = (uint8_t *)malloc(cap + 1);
    uint64_t len = 0, iterations = 0;
    int rc = msbwt_rle_merge_many(bwt, rle, offsets, n, out, cap, &len, NULL);
    if (rc == MSBWT_ERR_INVALID_ARG && len > cap) {
        cap = (size_t)len;
        out = (uint8_t *)realloc(out, cap);
        rc = msbwt_rle_merge_many(bwt, rle, offsets, n, out, cap, &len, NULL);
    }
    if (rc != MSBWT_OK) {
        fprintf(stderr, "merge failed (%d): %s\n", rc, msbwt_rle_last_error(bwt));
        return 1;
    }
    double ms[MSBWT_MERGE_STAGES];
    msbwt_rle_merge_info(bwt, &iterations, ms);
    printf("%zu inputs: %llu RLE bytes after %llu iterations (%.1f ms)\n", n, (unsigned long long)len, (unsigned long long)iterations, ms[2]);
    if ((rc = msbwt_save_bwt_numpy(out, (size_t)len, argv[argc - 1])) != MSBWT_OK) {
        fprintf(stderr, "cannot write %s (%d)\n", argv[argc - 1], rc);
        return 1;
    }
    free(out);
    free(rle);
    msbwt_rle_free(bwt);
    return 0;
}
