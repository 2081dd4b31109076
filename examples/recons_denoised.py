"""Measurement noise taken out of the POINTS before the solve: a sphere sampled with ten times the noise of recons_noisy_scan.py (0.02, one
voxel: the reconstruction ripples visibly), reconstructed as it comes and through ``nksr.get_mls_smooth_preprocess_fn`` (moving-least-squares
projection, ``nksr.cloud.smooth_mls``), with the RMS radial error of the input points and of the mesh vertices both ways."""
import torch
from common import warning_on_low_memory
import nksr

RADIUS = 0.45


def rms_radial(p):
    return float((torch.linalg.norm(p.double(), dim=1) - RADIUS).pow(2).mean().sqrt())


if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    device = torch.device("cuda:0")
    xyz, nrm = nksr.utils.synth_sphere(200000, RADIUS, 0.02, seed=0)
    input_xyz, input_normal = torch.from_numpy(xyz).to(device), torch.from_numpy(nrm).to(device)

    # the radius spans ~600 neighbours and two and a half times the noise, wide enough to average it below what the solve averages itself
    denoise = nksr.get_mls_smooth_preprocess_fn(radius=0.05, order=2, iterations=2)
    moved, fitted, _ = denoise(input_xyz, input_normal, None)
    fit = nksr.cloud.mls_project(moved, 0.05, normal=fitted)
    print('%d points, RMS radial error %.5f as they come, %.5f after two projections (%d of them fitted, %.0f neighbours each, '
          'mean curvature of the moved cloud %.3f for 1 / r = %.3f)'
          % (input_xyz.shape[0], rms_radial(input_xyz), rms_radial(moved), int(fit.valid.sum()), float(fit.count.float().mean()),
             float(fit.mean_curvature[fit.valid].mean()), 1.0 / RADIUS))

    reconstructor = nksr.Reconstructor(device)
    for name, fn in (('as it comes', None), ('denoised', denoise)):
        field = reconstructor.reconstruct(input_xyz, input_normal, preprocess_fn=fn, voxel_size=0.02)
        mesh = field.extract_dual_mesh(mise_iter=1)
        print('%-12s mesh vertices: RMS radial error %.5f' % (name, rms_radial(mesh.v)))

    nksr.utils.write_ply_mesh('recons_denoised.ply', mesh.v, mesh.f, normals=mesh.vertex_normals())
    print('V=%d F=%d -> recons_denoised.ply' % (mesh.v.shape[0], mesh.f.shape[0]))
