// Shared by the kernels that place heights among a family of parallel planes (csrc/meshslice.hip, csrc/meshclip.hip): the one search
// that decides on which side of a plane a height lies, so that the slicer and the clipper cannot disagree about it.
#pragma once
#include "common.h"

#define SL_LDS_OFFSETS 2048         // offsets staged in LDS up to this many planes (16 KiB)

// the number of offsets <= x (offsets strictly ascending): the first plane that lies ABOVE height x
__device__ __forceinline__ int32_t sl_upper(const double* __restrict__ o, int32_t np, double x) {
    int32_t lo = 0, hi = np;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (o[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
