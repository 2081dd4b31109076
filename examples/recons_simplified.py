"""examples/recons_simple.py followed by the mesh tools: floaters removed, then the mesh reduced by quadric vertex clustering on a grid of
four voxels (nksr_amd/mesh_simplify.py) -- flat parts lose their triangles, edges and corners keep their place."""
import torch
from common import load_bunny_example, warning_on_low_memory
import nksr

if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    device = torch.device("cuda:0")
    xyz, nrm = load_bunny_example()
    input_xyz = torch.from_numpy(xyz).float().to(device)
    input_normal = torch.from_numpy(nrm).float().to(device)

    reconstructor = nksr.Reconstructor(device)
    field = reconstructor.reconstruct(input_xyz, input_normal, detail_level=1.0)
    mesh = field.extract_dual_mesh(mise_iter=1)
    print('V=%d F=%d reconstructed' % (mesh.v.shape[0], mesh.f.shape[0]))

    voxel = reconstructor.hparams.voxel_size / field.scale          # the finest voxel in the cloud's units
    small = mesh.remove_small_components(min_area_ratio=0.01).simplify(cell_size=4 * voxel)
    nksr.utils.write_ply_mesh('recons_simplified.ply', small.v, small.f)
    print('V=%d F=%d -> recons_simplified.ply' % (small.v.shape[0], small.f.shape[0]))
