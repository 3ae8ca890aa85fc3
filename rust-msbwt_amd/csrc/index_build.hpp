// The loader's boundary (index_build.cpp): the six functions through which the rest of the C API decides what sits in HBM -- a load, the
// two releases, and the three rebuilds a setter can ask for.  Everything else the loader defines is private to its unit.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/msbwt_hip.h"

namespace msbwt_capi __attribute__((visibility("hidden"))) {

int install(msbwt_rle *h, const uint8_t *rle, size_t n);
void release_index(msbwt_rle *h);
void release_sparse(msbwt_rle *h);
int rebuild_table(msbwt_rle *h);
int rebuild_pair_and_table(msbwt_rle *h);
int replan(msbwt_rle *h, uint64_t bytes);  // the optional structures under a new memory budget

}  // namespace msbwt_capi
