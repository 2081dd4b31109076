"""A scene, not an object: a tilted ground, a few objects standing clear of it and stray returns, positions only.  The ground would
join every object into one cluster, so it goes first -- ``nksr.cloud.segment_plane`` --, then ``nksr.cloud.cluster_dbscan`` splits what
is left into its objects (the strays end as noise), and the largest object is reconstructed.

    python recons_segmented.py [points on the ground]

Prints the plane found, the cluster sizes and the mesh of the largest cluster."""
import sys

import numpy as np
import torch
from common import warning_on_low_memory
import nksr

VOXEL = 0.02
GROUND = np.array([-0.1, 0.05, 1.0, 0.45]) / np.linalg.norm([-0.1, 0.05, 1.0])         # z = 0.1 x - 0.05 y - 0.45


def scene(n_ground, seed=0):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(-1.0, 1.0, (n_ground, 2))
    ground = np.concatenate([xy, (0.1 * xy[:, 0] - 0.05 * xy[:, 1] - 0.45)[:, None]], axis=1) + rs.randn(n_ground, 1) * 0.002 * GROUND[:3]
    n = n_ground // 2
    torus, _ = nksr.utils.synth_torus(n, 0.32, 0.12, 0.002, seed=1)
    ball, _ = nksr.utils.synth_sphere(n // 3, 0.2, 0.002, seed=2)
    box, _ = nksr.utils.synth_rounded_box(n // 2, (0.15, 0.11, 0.08), 0.05, 0.002, seed=3)
    objects = [torus + [-0.45, -0.4, 0.0], ball + [0.55, 0.45, -0.1], box + [0.5, -0.55, -0.2]]
    strays = rs.uniform(-1.0, 1.0, (n_ground // 40, 3)) * [1.0, 1.0, 0.5]
    xyz = np.concatenate([ground] + objects + [strays]).astype(np.float32)
    return xyz[rs.permutation(len(xyz))]


if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    device = torch.device('cuda:0')
    n_ground = int(sys.argv[1]) if len(sys.argv) > 1 else 60000
    xyz = torch.from_numpy(scene(n_ground)).to(device)

    plane, inliers = nksr.cloud.segment_plane(xyz, 3 * 0.002, num_iterations=500, seed=0)
    angle = np.degrees(np.arccos(min(1.0, abs(float(plane[:3] @ GROUND[:3])))))
    print('plane %s: %d of %d points, %.3f deg from the ground it was sampled from' % (np.round(plane, 4), inliers.numel(), xyz.shape[0], angle))
    keep = torch.ones(xyz.shape[0], dtype=torch.bool, device=device)
    keep[inliers] = False
    rest = xyz[keep]

    clusters = nksr.cloud.cluster_dbscan(rest, eps=1.5 * VOXEL, min_points=10)
    sizes = clusters.sizes.tolist()
    print('%d clusters of sizes %s, %d noise points' % (clusters.n_clusters, sorted(sizes, reverse=True), int((clusters.labels < 0).sum())))
    largest = int(torch.argmax(clusters.sizes))
    obj = rest[clusters.labels == largest]
    print('largest cluster: label %d, %d points, centroid %s' % (largest, obj.shape[0], np.round(clusters.centroid[largest].cpu().numpy(), 3)))

    obj, normal = nksr.cloud.estimate_normals(obj, knn=32)
    field = nksr.Reconstructor(device).reconstruct(obj, normal, voxel_size=VOXEL)
    mesh = field.extract_dual_mesh(mise_iter=1)
    nksr.utils.write_ply_mesh('recons_segmented.ply', mesh.v, mesh.f)
    print('V=%d F=%d -> recons_segmented.ply' % (mesh.v.shape[0], mesh.f.shape[0]))
