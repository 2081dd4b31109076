"""Elevation contours of a reconstructed terrain (nksr_amd/mesh_slice.py): the stand-in of the configs[4] scene -- a wavy height field with
a box standing on it -- is reconstructed, cut at a fixed height interval on the GPU, and the ordered polylines are written as OBJ ``l``
elements.  Prints the number of polylines and the total length per level."""
import sys

import torch
from common import warning_on_low_memory
import nksr
from nksr_amd import utils

if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    interval = float(sys.argv[1]) if len(sys.argv) > 1 else 0.25
    device = torch.device('cuda:0')
    xyz, nrm = utils.synth_terrain_patch(200_000, seed=0)
    reconstructor = nksr.Reconstructor(device)
    field = reconstructor.reconstruct(torch.from_numpy(xyz).to(device), torch.from_numpy(nrm).to(device), detail_level=1.0)
    mesh = field.extract_dual_mesh(mise_iter=1)
    print('V=%d F=%d reconstructed' % (mesh.v.shape[0], mesh.f.shape[0]))

    r = mesh.contours(interval=interval)            # the multiples of the interval inside the height range; device tensors
    nksr.utils.write_obj_polylines('recons_contours.obj', r.points64, r.polyline_start, r.polyline_points, r.polyline_closed)
    start = r.plane_polyline_start.tolist()
    for j, (z, length, n_open) in enumerate(zip(r.offsets.tolist(), r.plane_length.tolist(), r.plane_open.tolist())):
        print('z=%+.3f  L=%d (%d open)  length=%.3f' % (z, start[j + 1] - start[j], n_open, length))
    print('N=%d S=%d L=%d on %d levels -> recons_contours.obj' % (r.n_points, r.n_segments, r.n_polylines, r.n_planes))
