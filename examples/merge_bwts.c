/* C host of the merge: two comp_msbwt.npy files in, the BWT of the union of their read sets out, merged on the GPU.
 *
 *   gcc -std=c11 -Iinclude examples/merge_bwts.c -Lrust-msbwt_amd -lmsbwt_hip -Wl,-rpath,$PWD/rust-msbwt_amd -o merge_bwts
 *   ./merge_bwts lane1/comp_msbwt.npy lane2/comp_msbwt.npy merged/comp_msbwt.npy
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

/* the payload of a NumPy v1.0 file of bytes: 10 bytes of magic, version and header length, the header, the RLE bytes */
static uint8_t *read_npy(const char *path, size_t *len) {
    FILE *f = fopen(path, "rb");
    unsigned char head[10];
    if (!f) return NULL;
    if (fread(head, 1, sizeof head, f) != sizeof head || memcmp(head, "\x93NUMPY", 6) != 0 || head[6] != 1) {
        fclose(f);
        return NULL;
    }
    const long start = 10 + (long)(head[8] | head[9] << 8);
    if (fseek(f, 0, SEEK_END) != 0 || ftell(f) < start) {
        fclose(f);
        return NULL;
    }
    *len = (size_t)(ftell(f) - start);
    uint8_t *bytes = (uint8_t *)malloc(*len + 1);
    const int ok = bytes && fseek(f, start, SEEK_SET) == 0 && fread(bytes, 1, *len, f) == *len;
    fclose(f);
    if (!ok) {
        free(bytes);
        return NULL;
    }
    return bytes;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s FIRST.npy SECOND.npy MERGED.npy\n", argv[0]);
        return 2;
    }
    size_t len0 = 0, len1 = 0;
    uint8_t *rle0 = read_npy(argv[1], &len0), *rle1 = read_npy(argv[2], &len1);
    if (!rle0 || !rle1) {
        fprintf(stderr, "cannot read %s\n", rle0 ? argv[2] : argv[1]);
        return 1;
    }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    size_t cap = len0 + len1; /* enough for canonical inputs; the call says what it needs otherwise */
    uint8_t *out = (uint8_t *)malloc(cap + 1);
    uint64_t len = 0, iterations = 0;
    int rc = msbwt_rle_merge(bwt, rle0, len0, rle1, len1, out, cap, &len, NULL);
    if (rc == MSBWT_ERR_INVALID_ARG && len > cap) {
        cap = (size_t)len;
        out = (uint8_t *)realloc(out, cap);
        rc = msbwt_rle_merge(bwt, rle0, len0, rle1, len1, out, cap, &len, NULL);
    }
    if (rc != MSBWT_OK) {
        fprintf(stderr, "merge failed (%d): %s\n", rc, msbwt_rle_last_error(bwt));
        return 1;
    }
    double ms[MSBWT_MERGE_STAGES];
    msbwt_rle_merge_info(bwt, &iterations, ms);
    printf("%llu RLE bytes after %llu iterations (%.1f ms)\n", (unsigned long long)len, (unsigned long long)iterations, ms[2]);
    if ((rc = msbwt_save_bwt_numpy(out, (size_t)len, argv[3])) != MSBWT_OK) {
        fprintf(stderr, "cannot write %s (%d)\n", argv[3], rc);
        return 1;
    }
    free(out);
    free(rle0);
    free(rle1);
    msbwt_rle_free(bwt);
    return 0;
}
