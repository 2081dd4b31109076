// Triangle-mesh queries (nksr_amd/mesh_query.py: MeshQuery, the o3d-iou of metrics.MeshEvaluator):
//   k_bvh_morton    Morton codes of face centroids (build) or of query points (query order), 21 bits per axis in a given box
//   k_bvh_nodes     internal nodes of the linear BVH (Karras, HPG 2012), equal codes split by their sorted position
//   k_bvh_refit     leaf records + bottom-up boxes; the second child to arrive at a node finishes it (integer flags, no float atomics)
//   k_mesh_occupancy  per query and ray: all crossings of the half-line (watertight predicate), inside = most rays odd
//   k_mesh_closest    exact closest point: nearer child first, boxes pruned by squared distance
// Layouts and the predicate: include/nksr_hip.h (mesh queries) and DESIGN.md section 3.9.
#include "common.h"
#include "mesh_dev.h"

#define BVH_BLOCK 64            // one wavefront per workgroup: the traversal stack is a per-lane column of LDS
#define BVH_LEAF_FLAG(k) (~(int32_t)(k))

__constant__ float c_bvh_dirs[NKSR_BVH_MAX_RAYS][3] = NKSR_BVH_RAY_DIRS;

// ---- build ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mq_quantise(float x, float lo, float scale) {
    const float q = (x - lo) * scale;
    return q > 0.f ? (q < 2097151.f ? (uint32_t)q : 2097151u) : 0u;      // (NaN -> 0)
}

// item i: the centroid of face i (faces != NULL) or point i; box6 = (lo xyz, hi xyz)
__global__ void __launch_bounds__(256) k_bvh_morton(const float* __restrict__ xyz, int64_t nv, const void* faces, int is64, int64_t n,
                                                    const float* __restrict__ box6, uint64_t* __restrict__ codes,
                                                    uint32_t* __restrict__ index) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float p[3] = {0.f, 0.f, 0.f};
    if (faces) {
        for (int c = 0; c < 3; ++c) {
            const int64_t vi = mesh_face_index(faces, is64, i * 3 + c);
            if (vi < 0 || vi >= nv) { p[0] = p[1] = p[2] = 0.f; break; }
            p[0] += xyz[vi * 3] * (1.f / 3.f);
            p[1] += xyz[vi * 3 + 1] * (1.f / 3.f);
            p[2] += xyz[vi * 3 + 2] * (1.f / 3.f);
        }
    } else {
        p[0] = xyz[i * 3]; p[1] = xyz[i * 3 + 1]; p[2] = xyz[i * 3 + 2];
    }
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ext = box6[3 + a] - box6[a];
        q[a] = mq_quantise(p[a], box6[a], ext > 0.f ? 2097152.f / ext : 0.f);
    }
    codes[i] = (uint64_t)morton_biased((int)q[0], (int)q[1], (int)q[2], 0);
    index[i] = (uint32_t)i;
}

// common prefix length of sorted codes i and j; equal codes continue with the bits of their positions (-1 outside [0, n))
__device__ __forceinline__ int mq_delta(const uint64_t* __restrict__ codes, int64_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t a = codes[i], b = codes[j];
    return a == b ? 64 + __clz((uint32_t)(i ^ j)) : __clzll((long long)(a ^ b));
}

// internal node i of n - 1; parent[c] = 2 * node + side for internal node c, parent[n - 1 + k] for leaf k (parent[0] = -1)
__global__ void __launch_bounds__(256) k_bvh_nodes(const uint64_t* __restrict__ codes, int n, float* __restrict__ nodes,
                                                   int32_t* __restrict__ parent) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    const int d = mq_delta(codes, n, i, i + 1) > mq_delta(codes, n, i, i - 1) ? 1 : -1;
    const int dmin = mq_delta(codes, n, i, i - d);
    int64_t lmax = 2;                                   // (int64: i + lmax d may pass 2^31 for n near 2^30)
    while (mq_delta(codes, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (mq_delta(codes, n, i, i + (l + t) * d) > dmin) l += (int)t;
    const int j = i + l * d;
    const int dnode = mq_delta(codes, n, i, j);
    int s = 0;
    for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (mq_delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
        if (t == 1) break;
    }
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int c0 = lo == gamma ? BVH_LEAF_FLAG(gamma) : gamma;
    const int c1 = hi == gamma + 1 ? BVH_LEAF_FLAG(gamma + 1) : gamma + 1;
    float* nd = nodes + (int64_t)i * NKSR_BVH_NODE_FLOATS;
    nd[12] = __int_as_float(c0);
    nd[13] = __int_as_float(c1);
    nd[14] = 0.f;
    nd[15] = 0.f;
    parent[c0 >= 0 ? c0 : (n - 1) + gamma] = 2 * i;
    parent[c1 >= 0 ? c1 : (n - 1) + gamma + 1] = 2 * i + 1;
    if (i == 0) parent[0] = -1;
}

// The boxes of a node's children travel through device memory between workgroups: they are written and read with agent-scope
// atomic stores / loads (coherent across the XCDs' L2s), and the flag increment (relaxed, agent scope) sits between two
// __threadfence()s: the first child's release before its increment, the second child's acquire after it.  min / max do not depend
// on the arrival order, so the tree is the same bit for bit on every run.
__device__ __forceinline__ void mq_store(float* p, float v) {
    __hip_atomic_store((unsigned int*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float mq_load(float* p) {
    return __uint_as_float(__hip_atomic_load((unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// thread k: leaf k (sorted position) = face order[k]; writes its record, then climbs while it is the second child to arrive
__global__ void __launch_bounds__(256) k_bvh_refit(const float* __restrict__ v, int64_t nv, const void* faces, int is64,
                                                   const uint32_t* __restrict__ order, int n, const int32_t* __restrict__ parent,
                                                   int32_t* __restrict__ flags, int32_t* __restrict__ height, float* __restrict__ nodes,
                                                   float* __restrict__ leaves, int32_t* __restrict__ depth_out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t face = order[k];
    float p[3][3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int64_t vi = mesh_face_index(faces, is64, face * 3 + c);
        if (vi < 0 || vi >= nv) { ok = false; vi = 0; }
#pragma unroll
        for (int a = 0; a < 3; ++a) p[c][a] = v[vi * 3 + a];
    }
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // (+ 0.f: -0 becomes +0, so that min / max cannot pick between the two zeros by arrival order)
        lo[a] = ok ? fminf(fminf(p[0][a], p[1][a]), p[2][a]) + 0.f : __int_as_float(0x7f800000);
        hi[a] = ok ? fmaxf(fmaxf(p[0][a], p[1][a]), p[2][a]) + 0.f : -__int_as_float(0x7f800000);
    }
    float* lf = leaves + (int64_t)k * NKSR_BVH_LEAF_FLOATS;
    const float qnan = __int_as_float(0x7fc00000);     // a face with an index outside [0, nv): never crossed, never nearest
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) lf[c * 3 + a] = ok ? p[c][a] : qnan;
    lf[9] = __int_as_float((int32_t)face);
    lf[10] = 0.f;
    lf[11] = 0.f;
    if (n == 1) { *depth_out = 0; return; }
    int code = parent[(n - 1) + k], h = 0;
    while (true) {
        const int node = code >> 1, side = code & 1;
        float* nd = nodes + (int64_t)node * NKSR_BVH_NODE_FLOATS;
#pragma unroll
        for (int a = 0; a < 3; ++a) { mq_store(nd + side * 6 + a, lo[a]); mq_store(nd + side * 6 + 3 + a, hi[a]); }
        __threadfence();                                                // release: the box above before the flag
        if (__hip_atomic_fetch_add(flags + node, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;   // first: the sibling finishes
        __threadfence();                                                // acquire: the sibling's box after its flag
        const int sib = __float_as_int(nd[12 + (side ^ 1)]);
        const int hs = sib >= 0 ? __hip_atomic_load(height + sib, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], mq_load(nd + (side ^ 1) * 6 + a));
            hi[a] = fmaxf(hi[a], mq_load(nd + (side ^ 1) * 6 + 3 + a));
        }
        h = 1 + (h > hs ? h : hs);
        __hip_atomic_store(height + node, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (node == 0) { *depth_out = h; return; }
        code = parent[node];
    }
}

// ---- the crossing predicate ------------------------------------------------------------------------------------------------------
// Watertight ray / triangle test (Woop, Benthin, Wald, JCGT 2013) for the ray (0, 0, +t) of the sheared frame, in which vertex X of
// the query O and direction d is  x = X'[kx] - d[kx] d[kz] X'[kz],  y = X'[ky] - d[ky] d[kz] X'[kz],  z = d[kz] X'[kz]  with
// X' = X - O (fp32) and |d[kz]| = 1, so every factor of the shear is exact.  The edge function of (P, Q) is e = Px Qy - Py Qx in fp32;
// fp32 rounding is monotone, so it is either exact in sign or 0, and a 0 is recomputed in fp64 from the fp32 coordinates (two exact
// products, exact sign).  An exact 0 (the ray meets the edge's line) takes the sign the edge function would have at the origin moved
// by (eps1, eps2), eps2 << eps1:  sign(Py - Qy), or sign(Qx - Px) when Py = Qy.  That is a top-left rule for the triangle's normalised
// winding, written per edge: e(Q, P) = -e(P, Q) in every case, so two triangles that share an edge never both count a transversal
// crossing and never both miss it, a vertex is claimed as by the perturbed origin, and the answer ignores the faces' orientation.
// The triangle counts when the three signs agree, det = U + V + W != 0, and the crossing lies on the half-line (T = U Az + V Bz + W Cz
// has the sign of the triangle).  No fp contraction: tests/mesh_query_ref.py restates the same operations in numpy.
__device__ __forceinline__ int mq_edge_sign(float px, float py, float qx, float qy, float& e) {
#pragma clang fp contract(off)
    e = px * qy - py * qx;
    if (e > 0.f) return 1;
    if (e < 0.f) return -1;
    const double e64 = (double)px * (double)qy - (double)py * (double)qx;
    if (e64 > 0.0) return 1;
    if (e64 < 0.0) return -1;
    if (py != qy) return py > qy ? 1 : -1;
    if (qx != px) return qx > px ? 1 : -1;
    return 0;                                           // (P = Q in the sheared plane, or a NaN corner)
}

struct mq_ray {
    float o[3];          // query (recentred fp32)
    float inv[3];        // 1 / d
    float sx, sy, sz;    // d[kx] d[kz], d[ky] d[kz], d[kz]
    int kx, ky, kz;
};

__device__ __forceinline__ int mq_crosses(const mq_ray& r, const float4 t0, const float4 t1, const float4 t2) {
#pragma clang fp contract(off)
    const float a[3] = {t0.x - r.o[0], t0.y - r.o[1], t0.z - r.o[2]};
    const float b[3] = {t0.w - r.o[0], t1.x - r.o[1], t1.y - r.o[2]};
    const float c[3] = {t1.z - r.o[0], t1.w - r.o[1], t2.x - r.o[2]};
    const float ax = a[r.kx] - r.sx * a[r.kz], ay = a[r.ky] - r.sy * a[r.kz];
    const float bx = b[r.kx] - r.sx * b[r.kz], by = b[r.ky] - r.sy * b[r.kz];
    const float cx = c[r.kx] - r.sx * c[r.kz], cy = c[r.ky] - r.sy * c[r.kz];
    float U, V, W;
    const int su = mq_edge_sign(bx, by, cx, cy, U);
    const int sv = mq_edge_sign(cx, cy, ax, ay, V);
    const int sw = mq_edge_sign(ax, ay, bx, by, W);
    if (su == 0 || su != sv || su != sw) return 0;
    const float det = U + V + W;
    if (det == 0.f) return 0;
    const float az = r.sz * a[r.kz], bz = r.sz * b[r.kz], cz = r.sz * c[r.kz];
    const float T = U * az + V * bz + W * cz;
    return (su > 0 ? T > 0.f : T < 0.f) ? 1 : 0;
}

// Conservative slab test (in the spirit of Ize, JCGT 2013): the box is widened by pad (2^-20 of the largest coordinate magnitude of
// mesh and query -- far above the few ulps by which the sheared, rounded corners of a counted triangle can leave its exact box) and
// tmax by 2 gamma(3).  A triangle the predicate counts is never culled, whatever the tree.
__device__ __forceinline__ bool mq_slab(const mq_ray& r, float pad, float lx, float ly, float lz, float hx, float hy, float hz) {
    const float t0x = (lx - r.o[0] - pad) * r.inv[0], t1x = (hx - r.o[0] + pad) * r.inv[0];
    const float t0y = (ly - r.o[1] - pad) * r.inv[1], t1y = (hy - r.o[1] + pad) * r.inv[1];
    const float t0z = (lz - r.o[2] - pad) * r.inv[2], t1z = (hz - r.o[2] + pad) * r.inv[2];
    const float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    const float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z)) * 1.0000004f;
    return tmin <= tmax && tmax >= 0.f;
}

__device__ __forceinline__ float mq_pad(float box_abs, const float o[3]) {
    const float m = fmaxf(box_abs, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2])));
    return m * 0x1p-20f + 0x1p-100f;
}

__device__ __forceinline__ float mq_box_abs(const float* __restrict__ box6) {
    float m = 0.f;
#pragma unroll
    for (int a = 0; a < 6; ++a) m = fmaxf(m, fabsf(box6[a]));
    return m;
}

__device__ __forceinline__ void mq_load_node(const float* __restrict__ nodes, int i, float4& n0, float4& n1, float4& n2, int& c0, int& c1) {
    const float4* p = reinterpret_cast<const float4*>(nodes + (int64_t)i * NKSR_BVH_NODE_FLOATS);
    n0 = p[0]; n1 = p[1]; n2 = p[2];
    const float4 n3 = p[3];
    c0 = __float_as_int(n3.x);
    c1 = __float_as_int(n3.y);
}

// one thread per query (in `order` when given, results scattered back to the query's own index); per ray the crossings of every
// triangle, the stack a column of LDS (NKSR_BVH_STACK entries: the host refuses a deeper tree)
__global__ void __launch_bounds__(BVH_BLOCK) k_mesh_occupancy(const float* __restrict__ nodes, const float* __restrict__ leaves, int nf,
                                                              const float* __restrict__ box6, const float* __restrict__ query, int64_t nq,
                                                              const uint32_t* __restrict__ order, int rays, uint8_t* __restrict__ inside,
                                                              int32_t* __restrict__ counts) {
    __shared__ int32_t stk[NKSR_BVH_STACK][BVH_BLOCK];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * BVH_BLOCK + lane;
    if (t >= nq) return;
    const int64_t qi = order ? (int64_t)order[t] : t;
    mq_ray r;
    r.o[0] = query[qi * 3]; r.o[1] = query[qi * 3 + 1]; r.o[2] = query[qi * 3 + 2];
    const float pad = mq_pad(mq_box_abs(box6), r.o);
    const int root = nf > 1 ? 0 : BVH_LEAF_FLAG(0);
    int odd = 0;
    for (int ray = 0; ray < rays; ++ray) {
        const float d[3] = {c_bvh_dirs[ray][0], c_bvh_dirs[ray][1], c_bvh_dirs[ray][2]};
        const float m0 = fabsf(d[0]), m1 = fabsf(d[1]), m2 = fabsf(d[2]);
        r.kz = m0 >= m1 && m0 >= m2 ? 0 : (m1 >= m2 ? 1 : 2);
        r.kx = r.kz == 2 ? 0 : r.kz + 1;
        r.ky = r.kx == 2 ? 0 : r.kx + 1;
        r.sz = d[r.kz];
        r.sx = d[r.kx] * r.sz;
        r.sy = d[r.ky] * r.sz;
        r.inv[0] = 1.f / d[0]; r.inv[1] = 1.f / d[1]; r.inv[2] = 1.f / d[2];
        int cnt = 0, sp = 0, node = root;
        while (nf > 0) {
            if (node >= 0) {
                float4 n0, n1, n2;
                int c0, c1;
                mq_load_node(nodes, node, n0, n1, n2, c0, c1);
                const bool h0 = mq_slab(r, pad, n0.x, n0.y, n0.z, n0.w, n1.x, n1.y);
                const bool h1 = mq_slab(r, pad, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w);
                if (h0 && h1) {
                    if (sp >= NKSR_BVH_STACK) { cnt = -1; break; }     // (unreachable: depth <= NKSR_BVH_STACK is checked before launch)
                    stk[sp++][lane] = c1;
                    node = c0;
                    continue;
                }
                if (h0 || h1) { node = h0 ? c0 : c1; continue; }
            } else {
                const float4* lf = reinterpret_cast<const float4*>(leaves + (int64_t)(~node) * NKSR_BVH_LEAF_FLOATS);
                cnt += mq_crosses(r, lf[0], lf[1], lf[2]);
            }
            if (sp == 0) break;
            node = stk[--sp][lane];
        }
        if (counts) counts[qi * rays + ray] = cnt;
        odd += cnt & 1;
    }
    inside[qi] = 2 * odd > rays ? 1 : 0;
}

// ---- closest point ---------------------------------------------------------------------------------------------------------------
// Ericson, Real-Time Collision Detection (2005) 5.1.5, fp32: the closest point of triangle (a, b, c) to p by Voronoi regions
__device__ __forceinline__ void mq_closest_on_triangle(const float p[3], const float a[3], const float b[3], const float c[3], float out[3]) {
#pragma clang fp contract(off)
    const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const float d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2], d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
    if (d1 <= 0.f && d2 <= 0.f) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
    const float bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const float d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2], d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
    if (d3 >= 0.f && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        const float s = d1 / (d1 - d3);
        for (int k = 0; k < 3; ++k) out[k] = a[k] + s * ab[k];
        return;
    }
    const float cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const float d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2], d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
    if (d6 >= 0.f && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return; }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        const float s = d2 / (d2 - d6);
        for (int k = 0; k < 3; ++k) out[k] = a[k] + s * ac[k];
        return;
    }
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        const float s = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int k = 0; k < 3; ++k) out[k] = b[k] + s * (c[k] - b[k]);
        return;
    }
    const float den = 1.f / (va + vb + vc), sv = vb * den, sw = vc * den;
    for (int k = 0; k < 3; ++k) out[k] = a[k] + ab[k] * sv + ac[k] * sw;
}

__device__ __forceinline__ float mq_box_d2(const float p[3], float pad, float lx, float ly, float lz, float hx, float hy, float hz) {
    const float dx = fmaxf(fmaxf(lx - pad - p[0], p[0] - hx - pad), 0.f);
    const float dy = fmaxf(fmaxf(ly - pad - p[1], p[1] - hy - pad), 0.f);
    const float dz = fmaxf(fmaxf(lz - pad - p[2], p[2] - hz - pad), 0.f);
    return dx * dx + dy * dy + dz * dz;
}

__global__ void __launch_bounds__(BVH_BLOCK) k_mesh_closest(const float* __restrict__ nodes, const float* __restrict__ leaves, int nf,
                                                            const float* __restrict__ box6, const float* __restrict__ query, int64_t nq,
                                                            const uint32_t* __restrict__ order, float* __restrict__ dist,
                                                            int64_t* __restrict__ face_out, float* __restrict__ point_out) {
    __shared__ int32_t stk[NKSR_BVH_STACK][BVH_BLOCK];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * BVH_BLOCK + lane;
    if (t >= nq) return;
    const int64_t qi = order ? (int64_t)order[t] : t;
    const float p[3] = {query[qi * 3], query[qi * 3 + 1], query[qi * 3 + 2]};
    const float pad = mq_pad(mq_box_abs(box6), p);
    float best = __int_as_float(0x7f800000), bp[3] = {0.f, 0.f, 0.f};
    int bface = -1, sp = 0, node = nf > 1 ? 0 : BVH_LEAF_FLAG(0);
    while (nf > 0) {
        if (node >= 0) {
            float4 n0, n1, n2;
            int c0, c1;
            mq_load_node(nodes, node, n0, n1, n2, c0, c1);
            const float d0 = mq_box_d2(p, pad, n0.x, n0.y, n0.z, n0.w, n1.x, n1.y);
            const float d1 = mq_box_d2(p, pad, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w);
            const bool v0 = d0 <= best, v1 = d1 <= best;     // (<=: a tie may still bring a smaller face index)
            if (v0 && v1) {
                if (sp >= NKSR_BVH_STACK) { bface = -2; break; }     // (unreachable: depth <= NKSR_BVH_STACK is checked before launch)
                const bool first0 = d0 <= d1;
                stk[sp++][lane] = first0 ? c1 : c0;
                node = first0 ? c0 : c1;
                continue;
            }
            if (v0 || v1) { node = v0 ? c0 : c1; continue; }
        } else {
            const float* lf = leaves + (int64_t)(~node) * NKSR_BVH_LEAF_FLOATS;
            const float4* l4 = reinterpret_cast<const float4*>(lf);
            const float4 t0 = l4[0], t1 = l4[1], t2 = l4[2];
            const float a[3] = {t0.x, t0.y, t0.z}, b[3] = {t0.w, t1.x, t1.y}, c[3] = {t1.z, t1.w, t2.x};
            float q[3];
            mq_closest_on_triangle(p, a, b, c, q);
            const float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
            const float d2 = ex * ex + ey * ey + ez * ez;
            const int fid = __float_as_int(t2.y);
            if (d2 < best || (d2 == best && (unsigned)fid < (unsigned)bface)) {
                best = d2; bface = fid; bp[0] = q[0]; bp[1] = q[1]; bp[2] = q[2];
            }
        }
        if (sp == 0) break;
        node = stk[--sp][lane];
    }
    if (dist) dist[qi] = sqrtf(best);
    if (face_out) face_out[qi] = bface;
    if (point_out) {
        point_out[qi * 3] = bp[0]; point_out[qi * 3 + 1] = bp[1]; point_out[qi * 3 + 2] = bp[2];
    }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
static int mq_check_bvh(const nksr_bvh_t* bvh, const char* who) {
    if (!bvh) return nksr_set_error(NKSR_ERR_ARG, "%s: NULL bvh", who);
    if (bvh->n_faces < 0 || bvh->n_faces > NKSR_BVH_MAX_FACES)
        return nksr_set_error(NKSR_ERR_ARG, "%s: n_faces=%lld outside [0, 2^30]", who, (long long)bvh->n_faces);
    if (bvh->n_faces > 0 && (!bvh->nodes || !bvh->leaves || !bvh->box)) return nksr_set_error(NKSR_ERR_ARG, "%s: NULL bvh arrays", who);
    return NKSR_OK;
}

extern "C" int nksr_bvh_morton(const float* xyz, int64_t nv, const void* faces, int faces_int64, int64_t n, const float* box6,
                               uint64_t* codes_out, uint32_t* index_out, void* stream) {
    if (nv < 0 || n < 0) return nksr_set_error(NKSR_ERR_ARG, "bvh morton: negative size (nv=%lld, n=%lld)", (long long)nv, (long long)n);
    if (n > NKSR_BVH_MAX_FACES && faces) return nksr_set_error(NKSR_ERR_ARG, "bvh morton: %lld faces > 2^30", (long long)n);
    if (n > 0xFFFFFFFFll) return nksr_set_error(NKSR_ERR_ARG, "bvh morton: %lld items do not fit 32-bit indices", (long long)n);
    if (!faces && n > nv) return nksr_set_error(NKSR_ERR_ARG, "bvh morton: %lld points of %lld", (long long)n, (long long)nv);
    if (n == 0) return NKSR_OK;
    if (!xyz || !box6 || !codes_out || !index_out) return nksr_set_error(NKSR_ERR_ARG, "bvh morton: NULL arrays");
    hipLaunchKernelGGL(k_bvh_morton, dim3(nksr_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, xyz, nv, faces, faces_int64, n, box6,
                       codes_out, index_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_bvh_nodes(const uint64_t* codes_sorted, int32_t* parent_work, const nksr_bvh_t* bvh, void* stream) {
    int rc = mq_check_bvh(bvh, "bvh nodes");
    if (rc) return rc;
    const int64_t n = bvh->n_faces;
    if (n < 2) return NKSR_OK;
    if (!codes_sorted || !parent_work) return nksr_set_error(NKSR_ERR_ARG, "bvh nodes: NULL arrays");
    hipLaunchKernelGGL(k_bvh_nodes, dim3(nksr_blocks(n - 1, 256)), dim3(256), 0, (hipStream_t)stream, codes_sorted, (int)n, bvh->nodes,
                       parent_work);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_bvh_refit(const float* v, int64_t nv, const void* faces, int faces_int64, const uint32_t* order,
                              const int32_t* parent_work, int32_t* flag_work, const nksr_bvh_t* bvh, void* stream) {
    int rc = mq_check_bvh(bvh, "bvh refit");
    if (rc) return rc;
    if (nv < 0) return nksr_set_error(NKSR_ERR_ARG, "bvh refit: negative size (nv=%lld)", (long long)nv);
    const int64_t n = bvh->n_faces;
    if (n == 0) return NKSR_OK;
    if (nv == 0) return nksr_set_error(NKSR_ERR_ARG, "bvh refit: %lld faces over zero vertices", (long long)n);
    if (!v || !faces || !order || !bvh->depth_dev || (n > 1 && (!parent_work || !flag_work)))
        return nksr_set_error(NKSR_ERR_ARG, "bvh refit: NULL arrays");
    hipStream_t st = (hipStream_t)stream;
    if (n > 1) NKSR_CHECK_HIP(hipMemsetAsync(flag_work, 0, sizeof(int32_t) * (size_t)(n - 1), st));
    hipLaunchKernelGGL(k_bvh_refit, dim3(nksr_blocks(n, 256)), dim3(256), 0, st, v, nv, faces, faces_int64, order, (int)n, parent_work,
                       flag_work, n > 1 ? flag_work + (n - 1) : nullptr, bvh->nodes, bvh->leaves, bvh->depth_dev);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

static int mq_check_query(const nksr_bvh_t* bvh, const float* query, int64_t nq, const char* who) {
    int rc = mq_check_bvh(bvh, who);
    if (rc) return rc;
    if (nq < 0) return nksr_set_error(NKSR_ERR_ARG, "%s: negative size (nq=%lld)", who, (long long)nq);
    if (nq > 0 && !query) return nksr_set_error(NKSR_ERR_ARG, "%s: NULL query", who);
    if (bvh->depth < 0 || bvh->depth > NKSR_BVH_STACK)
        return nksr_set_error(NKSR_ERR_CAPACITY, "%s: tree depth %d outside the traversal stack (%d entries)", who, (int)bvh->depth,
                              NKSR_BVH_STACK);
    return NKSR_OK;
}

extern "C" int nksr_mesh_occupancy(const nksr_bvh_t* bvh, const float* query, int64_t nq, const uint32_t* order, int rays,
                                   uint8_t* inside_out, int32_t* counts_out, void* stream) {
    int rc = mq_check_query(bvh, query, nq, "mesh occupancy");
    if (rc) return rc;
    if (rays < 1 || rays > NKSR_BVH_MAX_RAYS || rays % 2 == 0)
        return nksr_set_error(NKSR_ERR_ARG, "mesh occupancy: rays=%d is not an odd count in [1, %d]", rays, NKSR_BVH_MAX_RAYS);
    if (nq == 0) return NKSR_OK;
    if (!inside_out) return nksr_set_error(NKSR_ERR_ARG, "mesh occupancy: NULL output");
    hipLaunchKernelGGL(k_mesh_occupancy, dim3(nksr_blocks(nq, BVH_BLOCK)), dim3(BVH_BLOCK), 0, (hipStream_t)stream, bvh->nodes, bvh->leaves,
                       (int)bvh->n_faces, bvh->box, query, nq, order, rays, inside_out, counts_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}

extern "C" int nksr_mesh_closest(const nksr_bvh_t* bvh, const float* query, int64_t nq, const uint32_t* order, float* dist_out,
                                 int64_t* face_out, float* point_out, void* stream) {
    int rc = mq_check_query(bvh, query, nq, "mesh closest");
    if (rc) return rc;
    if (nq == 0) return NKSR_OK;
    if (!dist_out && !face_out && !point_out) return nksr_set_error(NKSR_ERR_ARG, "mesh closest: no output");
    hipLaunchKernelGGL(k_mesh_closest, dim3(nksr_blocks(nq, BVH_BLOCK)), dim3(BVH_BLOCK), 0, (hipStream_t)stream, bvh->nodes, bvh->leaves,
                       (int)bvh->n_faces, bvh->box, query, nq, order, dist_out, face_out, point_out);
    NKSR_CHECK_LAUNCH();
    return NKSR_OK;
}
