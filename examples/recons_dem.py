"""A reconstructed terrain as a raster (nksr_amd/mesh_raster.py): the stand-in of the configs[4] scene -- a wavy height field with a box
standing on it -- is reconstructed and rasterised on the GPU into an elevation grid on the lattice the tiles and contours are cut at.
Writes the grid as an ESRI ASCII file (north-up, -9999 where no face covers a pixel) and prints the share of covered pixels, the largest
layer count and the range of slope and hillshade."""
import sys

import torch
from common import warning_on_low_memory
import nksr
from nksr_amd import utils

if __name__ == '__main__':
    warning_on_low_memory(1024.0)
    pixel_size = float(sys.argv[1]) if len(sys.argv) > 1 else 0.1
    n_points = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    device = torch.device('cuda:0')
    xyz, nrm = utils.synth_terrain_patch(n_points, seed=0)
    reconstructor = nksr.Reconstructor(device)
    field = reconstructor.reconstruct(torch.from_numpy(xyz).to(device), torch.from_numpy(nrm).to(device), detail_level=1.0)
    mesh = field.extract_dual_mesh(mise_iter=1)
    print('V=%d F=%d reconstructed' % (mesh.v.shape[0], mesh.f.shape[0]))

    hm = mesh.height_map(pixel_size)                # seen along z, the top surface; device tensors
    nx, ny = hm.shape
    covered = float(hm.valid.double().mean()) if nx * ny else 0.0
    print('%d x %d pixels of %.3f from (%.3f, %.3f): %.1f%% covered, at most %d layers, %d coverings of %d candidates'
          % (nx, ny, hm.pixel_size, hm.origin[0], hm.origin[1], 100.0 * covered, int(hm.count.max()) if nx * ny else 0, hm.n_hits, hm.n_candidates))
    slope, shade = hm.slope(), hm.hillshade()
    inner = ~torch.isnan(shade)
    if bool(inner.any()):
        print('slope up to %.1f degrees, hillshade in [%.3f, %.3f]' % (float(torch.rad2deg(slope[inner].max())), float(shade[inner].min()), float(shade[inner].max())))
    utils.write_ascii_grid('recons_dem.asc', hm.height, hm.origin, hm.pixel_size)
    print('wrote recons_dem.asc')
