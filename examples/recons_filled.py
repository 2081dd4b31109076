"""Closing the small holes of a reconstruction (nksr_amd/mesh_boundary.py): the stand-in of the configs[2] scene is reconstructed, its
small components are removed, and every closed boundary loop of at most ``max_edges`` edges is filled by a centroid star; the flat
patches are then faired by Taubin smoothing with every old vertex pinned.  The rim of an open surface is a loop like any other: the
threshold is what keeps it open.  Prints the boundary edges and loops before and after and writes the patches as an OBJ."""
import sys

import torch
from common import warning_on_low_memory
import nksr
from nksr_amd import utils

if __name__ == '__main__':
    warning_on_low_memory(4096.0)
    max_edges = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    device = torch.device('cuda:0')
    xyz, nrm = utils.synth_scene(1_000_000, seed=0, extent=(40.0, 40.0, 10.0), n_objects=8)
    reconstructor = nksr.Reconstructor(device)
    field = reconstructor.reconstruct(torch.from_numpy(xyz).to(device), torch.from_numpy(nrm).to(device), detail_level=1.0)
    mesh = field.extract_dual_mesh(mise_iter=1).remove_small_components(min_faces=64)
    print('V=%d F=%d reconstructed, small components removed' % (mesh.v.shape[0], mesh.f.shape[0]))

    loops = mesh.boundary_loops()
    print('before: %d boundary edges in %d loops (%d closed, %d of them with at most %d edges); the longest has %d edges' % (
        loops.n_boundary, loops.n_loops, int(loops.loop_closed.sum()), int(loops.select(max_edges=max_edges).sum()), max_edges,
        int(loops.loop_edges.max()) if loops.n_loops else 0))
    filled = mesh.fill_holes(max_edges=max_edges)               # 'centroid': one new vertex per hole, appended behind the old ones
    new_vertex = torch.arange(filled.v.shape[0], device=device) >= mesh.v.shape[0]
    faired = filled.smooth(10, fixed=~new_vertex)               # only the new vertices move
    after = faired.topology()
    print('after:  %d boundary edges, %d new vertices, %d new faces, moved by at most %.3g' % (
        after.boundary_edges, int(new_vertex.sum()), filled.f.shape[0] - mesh.f.shape[0],
        float((faired.v - filled.v).norm(dim=1).max()) if filled.v.shape[0] else 0.0))
    assert after.boundary_edges <= loops.n_boundary
    patches = faired.f[mesh.f.shape[0]:]                        # the new faces follow the old ones
    used, local = torch.unique(patches, return_inverse=True)
    nksr.utils.write_obj_mesh('recons_filled_patches.obj', faired.v[used], local)
    print('-> recons_filled_patches.obj (%d faces)' % patches.shape[0])
