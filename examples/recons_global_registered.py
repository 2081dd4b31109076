"""Two partial scans of one shape that share NO frame: the second comes 140 degrees and 0.9 away from the first, as two handheld
sweeps or two tiles of different sessions do.  ICP alone cannot bring them together (it refines a pose that is nearly right);
``nksr.cloud.register_global`` finds the pose from scratch -- FPFH features on the voxel-downsampled scans, matched by brute force,
RANSAC over the matched pairs -- and hands it to point-to-plane ICP on the full scans.  Merged in the pose found, the scans are
reconstructed as one surface.

    python recons_global_registered.py [points per scan]

Prints the pose error after RANSAC and after ICP, and the chamfer distance of the merged reconstruction -- unregistered and
registered -- to the analytic surface."""
import sys

import numpy as np
import torch
from common import warning_on_low_memory
import nksr

VOXEL = 0.02                # of the reconstruction
REGISTRATION_VOXEL = 0.04   # of the features: their radius is 3 voxels, which then holds about 32 points of the thinned scan

BOX_HALF, BOX_RADIUS = np.array([0.30, 0.22, 0.16]), 0.10
BALL_CENTRE, BALL_RADIUS = np.array([0.34, 0.20, 0.14]), 0.13
RING_CENTRE, RING_R, RING_r = np.array([-0.15, -0.05, 0.26]), 0.12, 0.04


def shape(n, seed):
    """(xyz, normal) on the surface of a rounded box with a ball through one corner and a ring half sunk into its top: nothing about
    it is symmetric, so one pose alone brings two scans of it together.  The parts of every solid inside another are left out."""
    def box(x):
        q = np.abs(x) - BOX_HALF
        return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0) - BOX_RADIUS

    def ball(x):
        return np.linalg.norm(x - BALL_CENTRE, axis=1) - BALL_RADIUS

    def ring(x):
        y = x - RING_CENTRE
        return np.hypot(np.hypot(y[:, 0], y[:, 1]) - RING_R, y[:, 2]) - RING_r

    parts = ((nksr.utils.synth_rounded_box(2 * n, BOX_HALF, BOX_RADIUS, seed=seed), (ball, ring)),
             (nksr.utils.synth_sphere(n // 2, BALL_RADIUS, seed=seed, center=BALL_CENTRE), (box, ring)),
             (nksr.utils.synth_torus(n // 2, RING_R, RING_r, seed=seed, center=RING_CENTRE), (box, ball)))
    xyz, normal = [], []
    for (x, nrm), others in parts:
        outside = np.all([sdf(x.astype(np.float64)) > 0.0 for sdf in others], axis=0)
        xyz.append(x[outside])
        normal.append(nrm[outside])
    xyz, normal = np.concatenate(xyz), np.concatenate(normal)
    order = np.random.RandomState(seed).permutation(len(xyz))
    return xyz[order].astype(np.float32), normal[order].astype(np.float32)


def partial_scans(n, device):
    """the shape cut by the oblique plane x + y + z = 0, either half with a band of 0.15 beyond it; the second scan in a frame of its
    own, with the normals its scanner measured there"""
    a, na = shape(3 * n, seed=0)
    b, nb = shape(3 * n, seed=1)
    side = np.ones(3) / np.sqrt(3.0)
    ka, kb = a @ side < 0.15, b @ side > -0.15
    a, na, b, nb = a[ka][:n], na[ka][:n], b[kb][:n], nb[kb][:n]
    u, t = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.radians(140.0)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    pose = np.eye(4)                                            # scan 2 -> scan 1: what the registration should find
    pose[:3, :3] = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
    pose[:3, 3] = [0.7, -0.4, 0.3]
    gpu = lambda x: torch.from_numpy(x).to(device)              # noqa: E731
    b, nb = nksr.cloud.apply_transform(gpu(b), np.linalg.inv(pose), gpu(nb))
    return gpu(a), gpu(na), b, nb, pose


if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    device = torch.device('cuda:0')
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
    scan1, normal1, scan2, normal2, pose = partial_scans(n, device)

    result = nksr.cloud.register_global(scan2, scan1, REGISTRATION_VOXEL, source_normal=normal2, target_normal=normal1)
    ransac = result.ransac

    def pose_error(T):
        dR = T[:3, :3] @ pose[:3, :3].T
        return np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), np.linalg.norm(T[:3, 3] - pose[:3, 3])

    print('before: %.1f deg, %.3f apart' % pose_error(np.eye(4)))
    print('RANSAC: %d matched pairs, %d of %d draws scored, best holds %d pairs -> %.3f deg, %.4f' % (
        (ransac.correspondence_set.shape[0], ransac.n_scored, ransac.n_drawn, ransac.best_count) + pose_error(ransac.transformation.numpy())))
    found = result.transformation.numpy()
    print('ICP: %d iterations, fitness %.3f, rmse %.4f -> %.4f deg, %.5f' % (
        (result.iterations, result.fitness, result.inlier_rmse) + pose_error(found)))

    truth_xyz, truth_normal = shape(60000, seed=7)
    evaluator = nksr.metrics.MeshEvaluator(n_points=100000, metric_names=['chamfer-L1'], device=device)
    reconstructor = nksr.Reconstructor(device)
    chamfer = {}
    for name, T in (('unregistered', np.eye(4)), ('registered', found)):
        moved, moved_normal = nksr.cloud.apply_transform(scan2, T, normal2)
        field = reconstructor.reconstruct(torch.cat([scan1, moved]), torch.cat([normal1, moved_normal]), voxel_size=VOXEL)
        mesh = field.extract_dual_mesh(mise_iter=1)
        chamfer[name] = evaluator.eval_mesh(mesh, truth_xyz, truth_normal)['chamfer-L1']
        nksr.utils.write_ply_mesh('recons_global_%s.ply' % name, mesh.v, mesh.f)
        print('%s: V=%d F=%d chamfer-L1=%.5f -> recons_global_%s.ply' % (name, mesh.v.shape[0], mesh.f.shape[0], chamfer[name], name))
    print('chamfer unregistered=%.6f registered=%.6f' % (chamfer['unregistered'], chamfer['registered']))
