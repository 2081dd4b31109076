"""nksr_amd -- MI355X-native implementation of the NKSR solve-time hot path.

Exports the surface of the reference's ``nksr`` package that its examples and training glue
use: ``Reconstructor``, ``NKSRNetwork``, ``SparseFeatureHierarchy``,
``get_estimate_normal_preprocess_fn`` and the sub-modules ``fields``, ``svh``, ``configs``,
``utils``; beyond it the mesh and point-cloud tools (``metrics``, ``MeshTopology``, ``MeshGeometry``, ``MeshSimplifier``, ``MeshSlicer``, ``MeshClipper``, ``MeshRasterizer``, ``MeshBoundary``, ``cloud`` -- neighbour queries, voxel downsampling, outlier masks, normal
orientation, rigid registration (``cloud.icp`` / ``icp_multiscale`` / ``evaluate_registration`` / ``apply_transform``), global
registration of scans that share no frame (``cloud.compute_fpfh_feature`` / ``match_features`` /
``registration_ransac_based_on_feature_matching`` / ``register_global``), segmentation (``cloud.cluster_dbscan`` / ``segment_plane``) and
moving-least-squares projection (``cloud.mls_project`` / ``smooth_mls``) -- and the
``preprocess_fn`` makers on it).  ``import nksr`` resolves to this package through the top-level ``nksr`` shim.
"""
from . import cloud, configs, fields, metrics, svh, utils
from .mesh_boundary import MeshBoundary
from .mesh_clip import MeshClipper
from .mesh_geometry import MeshGeometry
from .mesh_raster import MeshRasterizer
from .mesh_simplify import MeshSimplifier
from .mesh_slice import MeshSlicer
from .mesh_topology import MeshTopology
from .nn.network import NKSRNetwork
from .preprocess import (compose_preprocess_fns, get_dbscan_preprocess_fn, get_estimate_normal_preprocess_fn,
                         get_estimate_oriented_normal_preprocess_fn, get_mls_smooth_preprocess_fn, get_radius_outlier_preprocess_fn,
                         get_remove_plane_preprocess_fn,
                         get_statistical_outlier_preprocess_fn, get_voxel_downsample_preprocess_fn)
from .reconstructor import Reconstructor
from .svh import SparseFeatureHierarchy

__all__ = ['Reconstructor', 'NKSRNetwork', 'SparseFeatureHierarchy', 'get_estimate_normal_preprocess_fn', 'MeshTopology', 'MeshGeometry', 'MeshSimplifier',
           'MeshSlicer', 'MeshClipper', 'MeshRasterizer', 'MeshBoundary', 'get_voxel_downsample_preprocess_fn', 'get_radius_outlier_preprocess_fn', 'get_statistical_outlier_preprocess_fn',
           'get_estimate_oriented_normal_preprocess_fn', 'get_dbscan_preprocess_fn', 'get_remove_plane_preprocess_fn', 'get_mls_smooth_preprocess_fn', 'compose_preprocess_fns',
           'fields', 'svh', 'configs', 'utils', 'metrics', 'cloud']
__version__ = '0.1.0'
