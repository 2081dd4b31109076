"""A cloud that has positions only -- no normals, no sensor positions: the bunny with its normals thrown away, reconstructed through
``nksr.get_estimate_oriented_normal_preprocess_fn`` (kNN-PCA normals, signs propagated along the minimum spanning forest of the
kNN graph, the highest point looking up) and written out.

For a chunked reconstruction (``chunk_size > 0``) orient the WHOLE cloud first -- ``xyz, normal = nksr.cloud.estimate_normals(xyz)`` --
and pass ``normal=``: a preprocess_fn runs per chunk, and a chunk's open piece of surface cannot be signed on its own."""
import os

import numpy as np
import torch
from common import warning_on_low_memory
import nksr

if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    device = torch.device("cuda:0")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'bunny_10k.npz')
    if os.path.exists(path):
        data = np.load(path)
        xyz, true_normal = data['xyz'].astype(np.float32), data['normal'].astype(np.float32)
    else:
        xyz, true_normal = nksr.utils.synth_torus(10000, 0.32, 0.12, 0.0, seed=0)
    input_xyz = torch.from_numpy(xyz).to(device)

    estimate = nksr.get_estimate_oriented_normal_preprocess_fn(knn=32, orient_k=16)
    kept, normal, _ = estimate(input_xyz, None, None)
    if kept.shape[0] == input_xyz.shape[0]:
        agree = float(((normal * torch.from_numpy(true_normal).to(device)).sum(1) > 0).float().mean())
        print('%d points; %.1f %% of the estimated normals look the way the scanned ones do' % (kept.shape[0], 100.0 * agree))

    reconstructor = nksr.Reconstructor(device)
    field = reconstructor.reconstruct(input_xyz, preprocess_fn=estimate, detail_level=1.0)
    mesh = field.extract_dual_mesh(mise_iter=1)
    nksr.utils.write_ply_mesh('recons_unoriented.ply', mesh.v, mesh.f)
    t = mesh.topology()
    print('V=%d F=%d watertight=%s components=%d -> recons_unoriented.ply' % (mesh.v.shape[0], mesh.f.shape[0], t.is_watertight,
                                                                             t.components().n))
