"""numpy / scipy restatement of nksr_amd/cloud.py in float64: k nearest neighbours, radius counts, the two outlier masks and voxel
downsampling.  Only the voxel of a point is computed in float32, exactly as the package defines it --
floor(fl32(x) * fl32(1 / voxel_size)) per axis -- since np.float32 multiply and floor reproduce that bit for bit."""
import numpy as np
from scipy.spatial import cKDTree


def cloud_a():
    """The standard input of tests/test_gpu_cloud.py: 20 000 noisy sphere samples with normals + 1 000 uniform stray points."""
    from nksr_amd import utils
    xyz, nrm = utils.synth_sphere(20000, 0.45, 0.002, 0)
    stray = np.random.RandomState(1).uniform(-0.6, 0.6, (1000, 3)).astype(np.float32)
    sn = np.random.RandomState(2).randn(1000, 3)
    sn = (sn / np.linalg.norm(sn, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([xyz, stray]).astype(np.float32), np.concatenate([nrm, sn]).astype(np.float32)


def knn(xyz, k, query=None, exclude_self=False):
    """(idx [Q, k + 1], dist [Q, k + 1]) float64, ascending: ONE neighbour more than asked for, so that a caller can see how
    far the k-th and the (k + 1)-th are apart (where the cloud has that many points; else k columns)."""
    x = np.asarray(xyz, np.float64)
    q = x if query is None else np.asarray(query, np.float64)
    kk = min(k + 1 + (1 if exclude_self else 0), len(x))
    d, j = cKDTree(x).query(q, k=kk)
    d, j = d.reshape(len(q), kk), j.reshape(len(q), kk)
    if exclude_self:
        # drop point i from row i (it is in the row unless more than kk points share its position: then any kk - 1 of the
        # others at distance 0 are as good, and the row is cut to its first kk - 1)
        keep = np.ones_like(j, bool)
        me = j == np.arange(len(q))[:, None]
        first = me.argmax(1)
        has = me.any(1)
        keep[np.arange(len(q))[has], first[has]] = False
        keep[~has, -1] = False
        d, j = d[keep].reshape(len(q), kk - 1), j[keep].reshape(len(q), kk - 1)
    return j, d


def radius_neighbors(xyz, radius, query=None):
    """per query the float64 distances of the cloud points within radius * (1 + 1e-4), ascending (the margin shows what sits AT the radius)"""
    x = np.asarray(xyz, np.float64)
    q = x if query is None else np.asarray(query, np.float64)
    tree = cKDTree(x)
    out = []
    for i, nb in enumerate(tree.query_ball_point(q, radius * (1 + 1e-4))):
        out.append(np.sort(np.linalg.norm(x[nb] - q[i], axis=1)))
    return out


def radius_count(xyz, radius, query=None, exclude_self=False, band=1e-5):
    """(count [Q], sure [Q]): points with d <= radius (the query's own point left out with exclude_self), and whether no neighbour lies
    within band * radius of the radius"""
    nb = radius_neighbors(xyz, radius, query)
    cnt = np.array([(d <= radius).sum() for d in nb]) - (1 if exclude_self else 0)
    sure = np.array([not (np.abs(d - radius) < band * radius).any() for d in nb])
    return cnt, sure


def mean_knn_distance(xyz, k):
    _, d = knn(xyz, k, exclude_self=True)
    return d[:, :k].mean(1)


def statistical_outlier(xyz, k=16, std_ratio=2.0):
    """(mask, m, threshold): keep iff m_i <= mean(m) + std_ratio * std(m, ddof=1)"""
    m = mean_knn_distance(xyz, k)
    thr = m.mean() + std_ratio * m.std(ddof=1)
    return m <= thr, m, thr


def voxel_ijk(xyz, voxel_size):
    inv = np.float32(1.0 / float(voxel_size))
    return np.floor(np.asarray(xyz, np.float32) * inv).astype(np.int64)


def voxel_downsample(xyz, voxel_size, attrs=()):
    """-> dict(ijk [V, 3] in ascending Morton-key order, inverse [N], count [V], xyz [V, 3] float64 means, attrs = list of [V, C] float64
    means, first [V] = lowest input index of every voxel)."""
    from oracle import spec
    ijk = voxel_ijk(xyz, voxel_size)
    keys = spec.morton_key(ijk, 0)
    uk, first, inverse, count = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)

    def mean(a):
        a = np.asarray(a, np.float64)
        s = np.zeros((len(uk), a.shape[1]))
        np.add.at(s, inverse, a)
        return s / count[:, None]
    return dict(ijk=ijk[first], inverse=inverse, count=count, xyz=mean(xyz), attrs=[mean(a) for a in attrs], first=first)


def unit_normals(mean_normal, first_normal):
    """mean normals scaled to unit length; one shorter than 1e-12 is replaced by the normal of the voxel's lowest-index point"""
    length = np.linalg.norm(mean_normal, axis=1, keepdims=True)
    return np.where(length < 1e-12, np.asarray(first_normal, np.float64), mean_normal / np.maximum(length, 1e-300))
