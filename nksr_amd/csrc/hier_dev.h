// Device-side reading of nksr_hier_t that several files share.  (Not in common.h: build.kernel_hash covers that file for the
// roofline kernels.)
#pragma once
#include "common.h"

// level of global unknown (= system row) `row`: the levels' unknowns are concatenated, lv[d].offset is where level d starts
__device__ __forceinline__ int row_level(const nksr_hier_t& h, int row) {
    int d = 0;
    while (d + 1 < h.depth && row >= h.lv[d + 1].offset) ++d;
    return d;
}
