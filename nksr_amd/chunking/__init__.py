"""Spatial chunking (``chunk_size=``), batched over all chunks of a rank, and its multi-GPU sharding.

Reference behaviour (call sites; the implementation is in the absent wheel): ``reconstruct(xyz,
normal, detail_level=None, chunk_size=50.0)`` examples/recons_by_chunk.py:29; solved chunks are
parked on ``chunk_tmp_device`` (:27); "Tuning detail_level / voxel_size is not supported if
chunk_size is provided" NKSR-USAGE.md:137.  Spec:
  * the bounding box is cut into a grid of ``chunk_size`` cubes; chunk c solves the points inside
    core_c +- band (ov = max(overlap_ratio*chunk_size, OV_FLOOR coarsest voxels), band = ov + BAND_EXTRA coarsest voxels)
  * the global field is the partition-of-unity blend  f = sum_c w_c f_c / sum_c w_c  with
    w_c(x) = prod_axis ramp((x - (lo-ov)) / 2ov) * ramp(((hi+ov) - x) / 2ov)  (linear ramps of
    neighbouring chunks add up to 1 inside the 2*ov band; a chunk's weight vanishes ov inside
    its data boundary, so it never contributes where its hierarchy is truncated)
  * every dual cell is meshed by the rank that owns the chunk whose core contains the cell's base voxel centre.

The reference runs its chunks one after the other (examples/recons_by_chunk.py:26-29).  Here ALL chunks of a rank are
ONE launch sequence: chunk c is moved into its own aligned cube ("slot") of an EXPLODED FRAME -- x' = x + T_c, T_c a
whole number of coarsest voxels, slots far enough apart that no kernel support reaches from one into another -- and the
union of the translated clouds is reconstructed like a single cloud.  Its system is block diagonal by construction (one
block per chunk); the PCG keeps per-chunk scalars and stopping tests (nksr_segments_t), every summation order of the
operator is chunk-relative, so a chunk's solution does not depend on its batch mates, and the slot of a chunk depends on
its grid position only: the same chunk gives the same bits on 1, 2 or 8 ranks.  A slot is an aligned cube of the Morton
lattice, hence one contiguous key range per level: the chunks are the segments of the batch.  The blend evaluates the
batch field at x + T_c for every chunk c that weighs at x.

Multi-GPU (one process per GPU): chunks are sharded over ranks (nksr_amd.dist) along a Morton curve; every rank is
given either the same full cloud or -- ``sharded_input=True`` -- only the points of its own chunks (+ band).  No
collective on the solve path, one all_gather of the chunk HALOS before meshing, one point-to-point gather of the
mesh pieces to rank 0 after it.
"""
from .residency import borrowed, spill_to_disk
from .geometry import (BAND_EXTRA, MIN_CHUNK_POINTS, OV_FLOOR, SLOT_GAP, ChunkFrame, chunk_geometry, chunk_grid, chunk_grid_struct,
                       chunk_index, chunk_pairs, exchange_band, halo_destinations, halo_inner, needed_chunks)
from .payload import ChunkPart, fields_from_payloads, pack_field, unpack_field
from .field import ChunkUnionMask, MultiChunkField
from .driver import ChunkTooSmall, plan_batches, reconstruct_by_chunk, select_chunk_points
