/* C host of the k-mer range and extension calls: load a comp_msbwt.npy, print the FM range of every k-mer given on the command
 * line and the counts of its six left extensions c . KMER ($ A C G N T), from the host forms, and check that the device forms
 * (one stream, buffers in HBM) return the same.
 *
 *   gcc -std=gnu11 -Iinclude -I/opt/rocm/include examples/kmer_extensions.c -Lrust-msbwt_amd -lmsbwt_hip -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/rust-msbwt_amd -Wl,-rpath,/opt/rocm/lib -o kmer_extensions
 *   ./kmer_extensions tests/golden/two_string.npy ACG CGT
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msbwt_hip.h"

#define CHECK_HIP(call)                                                           \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_));     \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static int fail(msbwt_rle *bwt, const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, msbwt_rle_last_error(bwt));
    return 1;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s comp_msbwt.npy KMER [KMER...]   (all k-mers of one length)\n", argv[0]);
        return 2;
    }
    const size_t n = (size_t)(argc - 2), k = strlen(argv[2]);
    for (size_t i = 0; i < n; ++i)
        if (strlen(argv[i + 2]) != k) {
            fprintf(stderr, "all k-mers must have the same length\n");
            return 2;
        }
    msbwt_rle *bwt = msbwt_rle_new(8);
    if (!bwt) return 1;
    int rc = msbwt_rle_load_numpy_file(bwt, argv[1]);
    if (rc != MSBWT_OK) return fail(bwt, "load", rc);
    uint8_t *codes = (uint8_t *)malloc(n * k > 0 ? n * k : 1);
    uint64_t *l = (uint64_t *)calloc(n, sizeof(uint64_t)), *h = (uint64_t *)calloc(n, sizeof(uint64_t));
    uint64_t *ext = (uint64_t *)calloc(6 * n, sizeof(uint64_t));
    uint64_t *dev_l = (uint64_t *)calloc(n, sizeof(uint64_t)), *dev_h = (uint64_t *)calloc(n, sizeof(uint64_t));
    uint64_t *dev_ext = (uint64_t *)calloc(6 * n, sizeof(uint64_t));
    for (size_t i = 0; i < n; ++i) msbwt_convert_stoi((const uint8_t *)argv[i + 2], k, codes + i * k);

    /* host forms */
    if ((rc = msbwt_rle_kmer_ranges(bwt, codes, k, n, l, h)) != MSBWT_OK) return fail(bwt, "kmer_ranges", rc);
    if ((rc = msbwt_rle_count_kmer_extensions(bwt, codes, k, n, ext)) != MSBWT_OK) return fail(bwt, "count_kmer_extensions", rc);

    /* device forms: asynchronous on one stream, reported by msbwt_rle_device_status */
    hipStream_t stream = NULL;
    void *d_codes = NULL, *d_l = NULL, *d_h = NULL, *d_ext = NULL;
    CHECK_HIP(hipStreamCreate(&stream));
    CHECK_HIP(hipMalloc(&d_codes, n * k > 0 ? n * k : 1));
    CHECK_HIP(hipMalloc(&d_l, n * sizeof(uint64_t)));
    CHECK_HIP(hipMalloc(&d_h, n * sizeof(uint64_t)));
    CHECK_HIP(hipMalloc(&d_ext, 6 * n * sizeof(uint64_t)));
    CHECK_HIP(hipMemcpy(d_codes, codes, n * k, hipMemcpyHostToDevice));
    if ((rc = msbwt_rle_kmer_ranges_device(bwt, d_codes, k, n, d_l, d_h, stream)) != MSBWT_OK) return fail(bwt, "kmer_ranges_device", rc);
    if ((rc = msbwt_rle_count_kmer_extensions_device(bwt, d_codes, k, n, d_ext, stream)) != MSBWT_OK)
        return fail(bwt, "count_kmer_extensions_device", rc);
    if ((rc = msbwt_rle_device_status(bwt, stream)) != MSBWT_OK) return fail(bwt, "device_status", rc);
    CHECK_HIP(hipMemcpy(dev_l, d_l, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(dev_h, d_h, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(dev_ext, d_ext, 6 * n * sizeof(uint64_t), hipMemcpyDeviceToHost));

    printf("total symbols: %llu\n", (unsigned long long)msbwt_rle_get_total_size(bwt));
    printf("kmer\tl\th\t$\tA\tC\tG\tN\tT\n");
    for (size_t i = 0; i < n; ++i) {
        printf("%s\t%llu\t%llu", argv[i + 2], (unsigned long long)l[i], (unsigned long long)h[i]);
        for (int c = 0; c < 6; ++c) printf("\t%llu", (unsigned long long)ext[6 * i + c]);
        printf("\n");
    }
    const int same = memcmp(l, dev_l, n * sizeof(uint64_t)) == 0 && memcmp(h, dev_h, n * sizeof(uint64_t)) == 0 &&
                     memcmp(ext, dev_ext, 6 * n * sizeof(uint64_t)) == 0;
    printf(same ? "device forms agree\n" : "device forms DIFFER\n");

    (void)hipFree(d_codes);
    (void)hipFree(d_l);
    (void)hipFree(d_h);
    (void)hipFree(d_ext);
    (void)hipStreamDestroy(stream);
    free(codes);
    free(l);
    free(h);
    free(ext);
    free(dev_l);
    free(dev_h);
    free(dev_ext);
    msbwt_rle_free(bwt);
    return same ? 0 : 1;
}
