// Shared by the mesh kernels (csrc/metrics.hip, csrc/meshquery.hip, csrc/meshtopo.hip): the reader of an int32 or int64 face array
// (``faces_int64`` of their entry points).  What an index outside [0, nv) means is each caller's business (face_corners, tp_face).
#pragma once
#include "common.h"

__device__ __forceinline__ int64_t mesh_face_index(const void* faces, int is64, int64_t k) {
    return is64 ? ((const int64_t*)faces)[k] : (int64_t)((const int32_t*)faces)[k];
}
