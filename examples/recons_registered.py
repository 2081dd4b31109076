"""Two overlapping partial scans of one shape whose poses disagree: the second is off by a few degrees and a few voxels, as the sweeps
of a ScanNet or Waymo sequence are before their poses are refined.  Merged as they come, the solve sees two sheets where the scans
overlap; registered first -- ``nksr.cloud.icp_multiscale``, point-to-plane, coarse to fine -- it sees one.

    python recons_registered.py [points per scan]

Prints the pose error before and after, and the chamfer distance of both reconstructions to the analytic surface."""
import sys

import numpy as np
import torch
from common import warning_on_low_memory
import nksr

VOXEL = 0.02


def partial_scans(n, device):
    """the rounded box cut by the oblique plane x + y + z = 0, either half with a band of 0.1 beyond it: the overlap crosses all six
    faces, so it fixes all six parameters (a cut along an axis leaves the scans free to slide along it).  The second scan comes in a
    frame of its own."""
    a, _ = nksr.utils.synth_rounded_box(3 * n, seed=0)
    b, _ = nksr.utils.synth_rounded_box(3 * n, seed=1)
    side = np.ones(3) / np.sqrt(3.0)
    a, b = a[a @ side < 0.1][:n], b[b @ side > -0.1][:n]
    u, t = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.radians(4.0)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    pose = np.eye(4)                                            # scan 2 -> scan 1: what the registration should find
    pose[:3, :3] = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
    pose[:3, 3] = [2.0 * VOXEL, -1.5 * VOXEL, 1.0 * VOXEL]
    b = nksr.cloud.apply_transform(torch.from_numpy(b).to(device), np.linalg.inv(pose))
    return torch.from_numpy(a).to(device), b, pose


def reconstruct(reconstructor, xyz, normal):
    field = reconstructor.reconstruct(xyz, normal, voxel_size=VOXEL)
    return field.extract_dual_mesh(mise_iter=1)


if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    device = torch.device('cuda:0')
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
    scan1, scan2, pose = partial_scans(n, device)
    scan1, normal1 = nksr.cloud.estimate_normals(scan1, knn=32)
    scan2, normal2 = nksr.cloud.estimate_normals(scan2, knn=32)

    result = nksr.cloud.icp_multiscale(scan2, scan1, voxel_sizes=[4 * VOXEL, 2 * VOXEL, None],
                                       max_correspondence_distances=[5 * VOXEL, 3 * VOXEL, 1.5 * VOXEL], max_iterations=[30, 30, 30],
                                       method='plane', target_normal=normal1)
    found = result.transformation.numpy()

    def pose_error(T):
        dR = T[:3, :3] @ pose[:3, :3].T
        return np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), np.linalg.norm(T[:3, 3] - pose[:3, 3]) / VOXEL

    print('pose error before: %.2f deg, %.2f voxels; after %d iterations on the last level (fitness %.3f, rmse %.4f): %.3f deg, %.3f voxels' % (
        pose_error(np.eye(4)) + (result.iterations, result.fitness, result.inlier_rmse) + pose_error(found)))

    truth_xyz, truth_normal = nksr.utils.synth_rounded_box(100000, seed=7)
    evaluator = nksr.metrics.MeshEvaluator(n_points=100000, metric_names=['chamfer-L1'], device=device)
    reconstructor = nksr.Reconstructor(device)
    chamfer = {}
    for name, T in (('unregistered', np.eye(4)), ('registered', found)):
        moved, moved_normal = nksr.cloud.apply_transform(scan2, T, normal2)
        mesh = reconstruct(reconstructor, torch.cat([scan1, moved]), torch.cat([normal1, moved_normal]))
        chamfer[name] = evaluator.eval_mesh(mesh, truth_xyz, truth_normal)['chamfer-L1']
        nksr.utils.write_ply_mesh('recons_%s.ply' % name, mesh.v, mesh.f)
        print('%s: V=%d F=%d chamfer-L1=%.5f -> recons_%s.ply' % (name, mesh.v.shape[0], mesh.f.shape[0], chamfer[name], name))
    print('chamfer unregistered=%.6f registered=%.6f' % (chamfer['unregistered'], chamfer['registered']))
