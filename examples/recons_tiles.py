"""A reconstructed terrain as a grid of tiles (nksr_amd/mesh_clip.py): the stand-in of the configs[4] scene -- a wavy height field with a box
standing on it -- is reconstructed, cut into square tiles on the GPU, every tile is simplified on its own and written as one OBJ.  Prints
the tile count and whether the border vertices of neighbouring tiles coincide bit for bit (before the simplification, which moves them)."""
import sys

import torch
from common import warning_on_low_memory
import nksr
from nksr_amd import utils

if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    tile_size = float(sys.argv[1]) if len(sys.argv) > 1 else 4.0
    n_points = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    device = torch.device('cuda:0')
    xyz, nrm = utils.synth_terrain_patch(n_points, seed=0)
    reconstructor = nksr.Reconstructor(device)
    field = reconstructor.reconstruct(torch.from_numpy(xyz).to(device), torch.from_numpy(nrm).to(device), detail_level=1.0)
    mesh = field.extract_dual_mesh(mise_iter=1)
    print('V=%d F=%d reconstructed' % (mesh.v.shape[0], mesh.f.shape[0]))

    tiles = mesh.tiles(tile_size)                   # a grid along x and y from the origin; device tensors
    nx, ny = tiles.shape
    nonempty = tiles.nonempty
    print('%d x %d tiles of %.2f, %d non-empty, %d faces' % (nx, ny, tile_size, len(nonempty), tiles.f.shape[0]))

    # neighbours along y share the cut points of the level between them: the same rows of the split mesh, hence the same bits
    start, src = tiles.part_vertex_start.tolist(), tiles.vertex_source
    same, shared = True, 0
    for j in nonempty:
        k = j + 1
        if k % ny and k in nonempty:
            a, b = src[start[j]:start[j + 1]], src[start[k]:start[k + 1]]
            ia = torch.isin(a, b).nonzero()[:, 0]
            ib = torch.searchsorted(b, a[ia])
            pa, pb = tiles.v64[start[j]:start[j + 1]][ia], tiles.v64[start[k]:start[k + 1]][ib]
            same = same and ia.numel() > 0 and torch.equal(pa.view(torch.int64), pb.view(torch.int64))
            shared += int(ia.numel())
    print('%d border vertices of neighbours coincide: %s' % (shared, same))

    for j, tile in zip(nonempty, tiles):
        small = tile.simplify(cell_size=0.25) if tile.f.shape[0] > 1000 else tile
        ix, iy = divmod(j, ny)
        utils.write_obj_mesh('recons_tiles_%02d_%02d.obj' % (ix, iy), small.v, small.f)
        print('tile (%d, %d): F=%d -> %d' % (ix, iy, tile.f.shape[0], small.f.shape[0]))
