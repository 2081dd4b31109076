// Shared by the mesh kernels (csrc/metrics.hip, csrc/meshquery.hip, csrc/meshtopo.hip, csrc/meshgeom.hip, csrc/meshsimp.hip, csrc/meshslice.hip, csrc/meshclip.hip, csrc/meshbound.hip): the reader
// of an int32 or int64 face array (``faces_int64`` of their entry points).  What an index outside [0, nv) means is each caller's
// business (face_corners); mesh_valid_face is the topology's notion, which the simplifier shares.  Below it what the entry points of
// meshtopo.hip, meshgeom.hip and meshsimp.hip share on the host: mesh_check_sizes and MESH_BLOCK / MESH_LAUNCH.
#pragma once
#include "common.h"

__device__ __forceinline__ int64_t mesh_face_index(const void* faces, int is64, int64_t k) {
    return is64 ? ((const int64_t*)faces)[k] : (int64_t)((const int32_t*)faces)[k];
}

// fp64 vectors of the geometry and simplification kernels (csrc/meshgeom.hip, csrc/meshsimp.hip)
struct gm_vec3 { double x, y, z; };
__device__ __forceinline__ gm_vec3 gm_sub(gm_vec3 a, gm_vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double gm_dot(gm_vec3 a, gm_vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ gm_vec3 gm_cross(gm_vec3 a, gm_vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// vertex i of an fp32 (v_f64 = 0) or fp64 position array
__device__ __forceinline__ gm_vec3 gm_pos(const void* v, int v_f64, int64_t i) {
    if (v_f64) { const double* p = (const double*)v + i * 3; return {p[0], p[1], p[2]}; }
    const float* p = (const float*)v + i * 3;
    return {(double)p[0], (double)p[1], (double)p[2]};
}

// the corners of face j and whether it is VALID: every index inside [0, nv) and no two equal
__device__ __forceinline__ bool mesh_valid_face(const void* faces, int is64, int64_t j, int64_t nv, int64_t c[3]) {
    c[0] = mesh_face_index(faces, is64, j * 3);
    c[1] = mesh_face_index(faces, is64, j * 3 + 1);
    c[2] = mesh_face_index(faces, is64, j * 3 + 2);
    return c[0] >= 0 && c[0] < nv && c[1] >= 0 && c[1] < nv && c[2] >= 0 && c[2] < nv && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

// ---- host side of the topology, geometry and simplification entry points: the limits of a mesh, one lane per item --------------
static inline int mesh_check_sizes(const char* who, int64_t nv, int64_t nf) {
    if (nv < 0 || nf < 0) return nksr_set_error(NKSR_ERR_ARG, "%s: negative size (nv=%lld, nf=%lld)", who, (long long)nv, (long long)nf);
    if (nv >= (1ll << 31)) return nksr_set_error(NKSR_ERR_ARG, "%s: nv=%lld, at most 2^31 - 1 vertices", who, (long long)nv);
    if (nf > NKSR_TOPO_MAX_FACES) return nksr_set_error(NKSR_ERR_ARG, "%s: %lld faces > 2^30", who, (long long)nf);
    return NKSR_OK;
}
#define MESH_BLOCK 256
#define MESH_LAUNCH(kernel, n, st, ...)                                                                                    \
    do {                                                                                                                   \
        hipLaunchKernelGGL(kernel, dim3(nksr_blocks((n), MESH_BLOCK)), dim3(MESH_BLOCK), 0, (st), __VA_ARGS__);             \
        NKSR_CHECK_LAUNCH();                                                                                               \
    } while (0)
