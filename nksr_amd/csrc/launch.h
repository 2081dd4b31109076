// One thread per element, 256 per workgroup, nothing launched for n <= 0: the launch of most entry points of hierarchy.hip,
// splat.hip, nn.hip and meshing.hip.  Returns the error code from the calling entry point when the launch fails.
#pragma once
#include "common.h"

#define LAUNCH1D(kern, n, stream, ...)                                                              \
    do {                                                                                            \
        if ((n) > 0) {                                                                              \
            hipLaunchKernelGGL(kern, dim3(nksr_blocks((n), 256)), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); \
            NKSR_CHECK_LAUNCH();                                                                    \
        }                                                                                           \
    } while (0)
