"""A noisy scan cleaned on the GPU before the solve: a sphere sampled with noise plus uniform stray points, through
radius outlier filter -> voxel downsampling (``nksr.compose_preprocess_fns``), reconstructed and written out."""
import numpy as np
import torch
from common import warning_on_low_memory
import nksr

if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    device = torch.device("cuda:0")
    xyz, nrm = nksr.utils.synth_sphere(200000, 0.45, 0.002, seed=0)
    rs = np.random.RandomState(1)
    stray = rs.uniform(-0.6, 0.6, (4000, 3)).astype(np.float32)
    stray_n = rs.randn(4000, 3).astype(np.float32)
    input_xyz = torch.from_numpy(np.concatenate([xyz, stray])).to(device)
    input_normal = torch.from_numpy(np.concatenate([nrm, stray_n / np.linalg.norm(stray_n, axis=1, keepdims=True)])).to(device)

    clean = nksr.compose_preprocess_fns(nksr.get_radius_outlier_preprocess_fn(radius=0.02, min_neighbors=8),
                                        nksr.get_voxel_downsample_preprocess_fn(voxel_size=0.005))
    kept = clean(input_xyz, input_normal, None)[0]
    print('%d points in, %d after the filter and the downsampling' % (input_xyz.shape[0], kept.shape[0]))

    reconstructor = nksr.Reconstructor(device)
    field = reconstructor.reconstruct(input_xyz, input_normal, preprocess_fn=clean, voxel_size=0.02)
    mesh = field.extract_dual_mesh(mise_iter=1)
    mesh = mesh.smooth(5)                       # five Taubin pairs take the lattice-frequency ripple out without shrinking the sphere

    nksr.utils.write_ply_mesh('recons_noisy_scan.ply', mesh.v, mesh.f, normals=mesh.vertex_normals())
    r = torch.linalg.norm(mesh.v, dim=1)
    print('V=%d F=%d radius %.4f .. %.4f -> recons_noisy_scan.ply' % (mesh.v.shape[0], mesh.f.shape[0], float(r.min()), float(r.max())))
