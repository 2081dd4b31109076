"""numpy / scipy restatement of point-cloud segmentation, written from the definitions (csrc/segment.hip's header comment), in float64
and integers.

DBSCAN.  j is a neighbour of i iff |x_j - x_i| <= eps (inclusive, a point its own neighbour); core = at least min_points neighbours;
clusters = connected components of the core-core neighbour graph; a non-core point with a core neighbour takes the lowest label among
its core neighbours, every other non-core point is noise (-1); labels 0 .. C - 1 ascend with the smallest index among each cluster's
core points.  Pairs come from a cKDTree with a margin and are then decided here: in integers for a lattice cloud (``lattice_pairs``),
in float64 for a real-valued one (``real_pairs``).

Plane RANSAC.  Triples from numpy.random.RandomState(seed).randint(0, N, (H, 3)); n = (p1 - p0) x (p2 - p0) scaled to unit length,
d = -n . p0, |n| <= 1e-12 before scaling: degenerate (score -1); the residual is ((a x + b y) + c z) + d in float64 (numpy rounds every
product and sum on its own); inlier iff |s| <= t; best = highest count, lowest iteration on a tie; refinement = the eigenvector of the
smallest eigenvalue of the inliers' covariance, signed so that the first non-zero of (n_z, n_y, n_x) is positive, d = -n . mean; the
inliers returned are those of the refined plane."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

UNIT = 2.0 ** -10           # the lattice: coordinates are integer multiples of it


# ---- DBSCAN ----------------------------------------------------------------------------------------------------------------------------
def lattice_pairs(k, r):
    """(pairs [P, 2] with i < j and |k_j - k_i|^2 <= r^2 decided in integers, number of pairs EXACTLY at the radius)"""
    k = np.asarray(k, np.int64)
    cand = cKDTree(k.astype(np.float64)).query_pairs(r + 0.5, output_type='ndarray').reshape(-1, 2)
    d = k[cand[:, 0]] - k[cand[:, 1]]
    d2 = (d * d).sum(1)
    return cand[d2 <= r * r], int((d2 == r * r).sum())


def real_pairs(xyz, eps):
    """pairs with i < j and float64 |x_j - x_i|^2 <= eps^2"""
    x = np.asarray(xyz, np.float64)
    cand = cKDTree(x).query_pairs(eps * (1.0 + 1e-9), output_type='ndarray').reshape(-1, 2)
    d = x[cand[:, 0]] - x[cand[:, 1]]
    return cand[(d * d).sum(1) <= eps * eps]


def pairs_in_band(xyz, eps, band=1e-5):
    """the number of pairs whose float64 distance lies in (eps (1 - band), eps (1 + band)]"""
    return len(real_pairs(xyz, eps * (1.0 + band))) - len(real_pairs(xyz, eps * (1.0 - band)))


def dbscan(n, pairs, min_points):
    """-> dict(labels int64 [n], core bool [n], n_clusters, sizes int64 [C]) from the neighbour pairs (i != j, each once)"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    degree = 1 + np.bincount(pairs.ravel(), minlength=n)                 # itself included
    core = degree >= min_points
    cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]]
    graph = coo_matrix((np.ones(len(cc), np.int8), (cc[:, 0], cc[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    labels = np.full(n, -1, np.int64)
    core_idx = np.nonzero(core)[0]
    if len(core_idx):
        # components of core points, numbered by their smallest core index: np.unique returns first occurrences in ascending index order
        _, first = np.unique(comp[core_idx], return_index=True)
        rank = np.empty(comp.max() + 1, np.int64)
        rank[comp[core_idx][np.sort(first)]] = np.arange(len(first))
        labels[core_idx] = rank[comp[core_idx]]
    n_clusters = int(labels.max()) + 1 if len(core_idx) else 0
    # border points: the lowest label among the core neighbours
    best = np.full(n, np.iinfo(np.int64).max)
    for a, b in ((0, 1), (1, 0)):
        m = ~core[pairs[:, a]] & core[pairs[:, b]]
        np.minimum.at(best, pairs[m, a], labels[pairs[m, b]])
    border = ~core & (best < np.iinfo(np.int64).max)
    labels[border] = best[border]
    sizes = np.bincount(labels[labels >= 0], minlength=n_clusters).astype(np.int64)
    return dict(labels=labels, core=core, n_clusters=n_clusters, sizes=sizes, border=border)


def dbscan_lattice(k, r, min_points):
    pairs, at_radius = lattice_pairs(k, r)
    out = dbscan(len(k), pairs, min_points)
    out['at_radius'] = at_radius
    return out


def dbscan_real(xyz, eps, min_points):
    return dbscan(len(xyz), real_pairs(xyz, eps), min_points)


def centroids(xyz, labels, n_clusters):
    """float64 [C, 3] means of every cluster's points"""
    x = np.asarray(xyz, np.float64)
    s = np.zeros((n_clusters, 3))
    m = labels >= 0
    np.add.at(s, labels[m], x[m])
    return s / np.maximum(np.bincount(labels[m], minlength=n_clusters), 1)[:, None]


def relabel_by_first_core(labels, core):
    """the labels of the CORE points renumbered in ascending order of each cluster's smallest core index (-1 elsewhere)"""
    out = np.full(len(labels), -1, np.int64)
    idx = np.nonzero(core)[0]
    if len(idx):
        _, first = np.unique(labels[idx], return_index=True)
        rank = np.empty(labels.max() + 1, np.int64)
        rank[labels[idx][np.sort(first)]] = np.arange(len(first))
        out[idx] = rank[labels[idx]]
    return out


LATTICE_CASES = ((5, 3), (13, 6), (25, 10), (25, 1), (50, 20))          # (r in lattice units, min_points)


def lattice_cloud():
    """int64 [N, 3] lattice coordinates, |k| <= 500, about 4 400 points: four Gaussian blobs (sigma 25 - 40 units, one of only 60
    points), a thin bridge of points 4 units apart joining two of them, 300 uniform strays and 50 exact duplicates, shuffled."""
    rs = np.random.RandomState(11)
    blobs = [((-250, -200, 0), 40, 1500), ((200, -150, 50), 30, 1300), ((150, 250, -100), 25, 1100), ((-300, 300, 200), 25, 60)]
    parts = [np.rint(rs.randn(n, 3) * s + np.array(c)) for c, s, n in blobs]
    a, b = np.array(blobs[0][0], float), np.array(blobs[1][0], float)
    steps = int(np.linalg.norm(b - a) / 4.0)
    parts.append(np.rint(a + (b - a) * (np.arange(steps + 1) / steps)[:, None]))
    parts.append(np.rint(rs.uniform(-500, 500, (300, 3))))
    k = np.clip(np.concatenate(parts), -500, 500).astype(np.int64)
    k = np.concatenate([k, k[rs.randint(0, len(k), 50)]])
    return k[rs.permutation(len(k))]


def lattice_xyz(k):
    """float32 coordinates of lattice points: exact"""
    return (np.asarray(k, np.float64) * UNIT).astype(np.float32)


# ---- plane RANSAC ----------------------------------------------------------------------------------------------------------------------
PLANE_NORMAL = np.array([-0.1, 0.05, 1.0]) / np.linalg.norm([-0.1, 0.05, 1.0])       # of z = 0.1 x - 0.05 y + 0.02
PLANE_D = -0.02 / np.linalg.norm([-0.1, 0.05, 1.0])
THRESHOLD = 0.006


def plane_scene():
    """(xyz float32 [16 500, 3], on_plane bool): 12 000 points on z = 0.1 x - 0.05 y + 0.02 with sigma = 0.002 noise along the normal,
    4 000 points on eight spheres of radius 0.06 above the plane, 500 uniform strays, shuffled."""
    rs = np.random.RandomState(21)
    xy = rs.uniform(-0.5, 0.5, (12000, 2))
    ground = np.concatenate([xy, (0.1 * xy[:, 0] - 0.05 * xy[:, 1] + 0.02)[:, None]], axis=1) + rs.randn(12000, 1) * 0.002 * PLANE_NORMAL
    centres = np.concatenate([rs.uniform(-0.4, 0.4, (8, 2)), np.zeros((8, 1))], axis=1)
    centres[:, 2] = 0.1 * centres[:, 0] - 0.05 * centres[:, 1] + 0.02 + rs.uniform(0.09, 0.2, 8)
    u = rs.randn(4000, 3)
    balls = centres[np.arange(4000) % 8] + 0.06 * u / np.linalg.norm(u, axis=1, keepdims=True)
    strays = rs.uniform(-0.5, 0.5, (500, 3))
    xyz = np.concatenate([ground, balls, strays]).astype(np.float32)
    on_plane = np.arange(len(xyz)) < 12000
    p = rs.permutation(len(xyz))
    return xyz[p], on_plane[p]


def sample_planes(xyz, num_iterations, seed=0):
    """(planes float64 [H, 4], degenerate bool [H])"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    tri = np.random.RandomState(seed).randint(0, len(x), (num_iterations, 3))
    p0, p1, p2 = x[tri[:, 0]], x[tri[:, 1]], x[tri[:, 2]]
    n = np.cross(p1 - p0, p2 - p0)
    length = np.sqrt((n * n).sum(1))
    bad = length <= 1e-12
    n = n / np.where(bad, 1.0, length)[:, None]
    planes = np.concatenate([n, -(n * p0).sum(1, keepdims=True)], axis=1)
    planes[bad] = 0.0
    return planes, bad


def residuals(xyz, plane):
    x = np.asarray(xyz, np.float32).astype(np.float64)
    return ((plane[0] * x[:, 0] + plane[1] * x[:, 1]) + plane[2] * x[:, 2]) + plane[3]


def plane_counts(xyz, planes, t, degenerate=None):
    """int64 [H]: inliers of every plane, -1 for a degenerate one (flagged, or a zero normal)"""
    planes = np.asarray(planes, np.float64)
    bad = (planes[:, :3] == 0.0).all(1) | ~np.isfinite(planes).all(1)
    if degenerate is not None:
        bad = bad | degenerate
    return np.array([-1 if b else int((np.abs(residuals(xyz, p)) <= t).sum()) for p, b in zip(planes, bad)], np.int64)


def sign_normal(plane):
    for a in (2, 1, 0):
        if plane[a] != 0.0:
            return plane if plane[a] > 0.0 else -plane
    return plane


def refine(xyz, mask):
    """the least-squares plane of the points flagged in ``mask``"""
    p = np.asarray(xyz, np.float32).astype(np.float64)[mask]
    mean = p.mean(0)
    q = p - mean
    val, vec = np.linalg.eigh(q.T @ q / len(p))
    n = vec[:, 0]
    return sign_normal(np.concatenate([n, [-n @ mean]])), val


def segment_plane(xyz, t, num_iterations, seed=0):
    """-> dict(best, counts, plane, inliers, margin = the smallest | |s| - t | over the points for the refined plane, eigenvalues)"""
    planes, bad = sample_planes(xyz, num_iterations, seed)
    counts = plane_counts(xyz, planes, t, bad)
    best = int(np.argmax(counts))
    plane, val = refine(xyz, np.abs(residuals(xyz, planes[best])) <= t)
    s = np.abs(residuals(xyz, plane))
    return dict(best=best, counts=counts, planes=planes, plane=plane, inliers=np.nonzero(s <= t)[0], margin=float(np.abs(s - t).min()),
                eigenvalues=val)
