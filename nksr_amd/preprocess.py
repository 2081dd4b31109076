"""``preprocess_fn`` makers for ``Reconstructor.reconstruct(..., preprocess_fn=...)``: every one returns a function
``(xyz, normal, sensor) -> (xyz', normal', sensor')`` (``None`` passes through as ``None``).

``nksr.get_estimate_normal_preprocess_fn(knn, deg)`` (reference call sites
examples/recons_waymo.py:36, gis_app.py:41; CPU recipe examples/recons_waymo_cpu.py:21-41):
kNN-PCA normals, flipped towards the sensor, grazing (> deg) points dropped.

The cleaning steps in front of it (nksr_amd/cloud.py): voxel downsampling, the two outlier filters, plane removal, DBSCAN
cluster selection and moving-least-squares smoothing, chained with ``compose_preprocess_fns``.  The filters keep the input order of the points they keep; the
downsampler returns its voxels in ascending key order."""


def get_estimate_normal_preprocess_fn(knn=64, deg=85.0):
    def fn(xyz, normal, sensor):
        from .normals import estimate_normals_knn
        return estimate_normals_knn(xyz, normal, sensor, int(knn), float(deg))
    return fn


def get_estimate_oriented_normal_preprocess_fn(knn=64, orient_k=16, seed='+z', viewpoint=None):
    """For a cloud that has positions only: ``(xyz, None, sensor-or-None) -> (xyz', normal', None)`` by ``cloud.estimate_normals`` --
    kNN-PCA normals, oriented along the minimum spanning forest of the ``orient_k``-nearest-neighbour graph, every connected component
    signed by ``seed`` / ``viewpoint``; a sensor that is given is not used.  Orientation is a property of the WHOLE cloud: under
    ``reconstruct(..., chunk_size > 0)`` this function would run per chunk, and the open piece inside a chunk cannot be signed by the
    '+z' rule -- call ``cloud.estimate_normals`` on the whole cloud first and pass ``normal=``."""
    def fn(xyz, normal, sensor):
        from .orient import estimate_normals
        if normal is not None:
            raise RuntimeError('normal already exists')
        xyz, normal = estimate_normals(xyz, knn=knn, orient_k=orient_k, seed=seed, viewpoint=viewpoint)
        return xyz, normal, None
    return fn


def get_voxel_downsample_preprocess_fn(voxel_size, reduce='mean'):
    """One point per voxel of size ``voxel_size`` (``cloud.voxel_downsample``; colours do not fit the three slots: call it directly)."""
    def fn(xyz, normal, sensor):
        from .cloud import voxel_downsample
        r = voxel_downsample(xyz, voxel_size, normal=normal, sensor=sensor, reduce=reduce)
        return r.xyz, r.normal, r.sensor
    return fn


def _select(mask, xyz, normal, sensor):
    return xyz[mask], normal[mask] if normal is not None else None, sensor[mask] if sensor is not None else None


def get_radius_outlier_preprocess_fn(radius, min_neighbors):
    """Keeps the points with at least ``min_neighbors`` other points within ``radius`` (``cloud.radius_outlier_mask``)."""
    def fn(xyz, normal, sensor):
        from .cloud import radius_outlier_mask
        return _select(radius_outlier_mask(xyz, radius, min_neighbors), xyz, normal, sensor)
    return fn


def get_statistical_outlier_preprocess_fn(k=16, std_ratio=2.0):
    """Keeps the points whose mean distance to their k nearest neighbours is at most mean + std_ratio * std over the cloud
    (``cloud.statistical_outlier_mask``)."""
    def fn(xyz, normal, sensor):
        from .cloud import statistical_outlier_mask
        return _select(statistical_outlier_mask(xyz, k, std_ratio), xyz, normal, sensor)
    return fn


def get_dbscan_preprocess_fn(eps, min_points, min_cluster_size=None, keep_largest=None):
    """Keeps the points of the ``cloud.cluster_dbscan(eps, min_points)`` clusters with at least ``min_cluster_size`` points and / or of
    the ``keep_largest`` largest clusters (ties on size go to the lower label); noise is dropped, the input order is kept.  Clusters
    are a property of the WHOLE cloud: under ``reconstruct(..., chunk_size > 0)`` this function would run per chunk, where an object cut
    by a chunk boundary counts as two smaller ones -- call ``cloud.cluster_dbscan`` on the whole cloud first and pass what it keeps."""
    def fn(xyz, normal, sensor):
        from .cloud import cluster_dbscan
        r = cluster_dbscan(xyz, eps, min_points)
        return _select(r.point_mask(r.select(min_cluster_size, keep_largest)), xyz, normal, sensor)
    return fn


def get_remove_plane_preprocess_fn(distance_threshold, num_iterations=1000, seed=0):
    """Drops the inliers of the dominant plane (``cloud.segment_plane``: ground, floor, table); the input order is kept."""
    def fn(xyz, normal, sensor):
        import torch
        from .cloud import segment_plane
        _, inliers = segment_plane(xyz, distance_threshold, num_iterations=num_iterations, seed=seed)
        keep = torch.ones(xyz.shape[0], dtype=torch.bool, device=xyz.device)
        keep[inliers] = False
        return _select(keep, xyz, normal, sensor)
    return fn


def get_mls_smooth_preprocess_fn(radius, order=2, iterations=1, sigma=None):
    """Moves every point onto the moving-least-squares surface of the cloud (``cloud.smooth_mls``: ``iterations`` projections, a plane
    (``order=1``) or a quadric (``order=2``) fitted to the neighbours within ``radius``); normals that came in are replaced by the
    fit's, signed by them; the sensor passes through; the order and the number of points are kept.  A point with too few neighbours
    stays as it is.  The fit is a property of the WHOLE cloud: under ``reconstruct(..., chunk_size > 0)`` this function would run per
    chunk, where the points near a chunk face lose the neighbours beyond it and are pulled towards the inside -- call
    ``cloud.smooth_mls`` on the whole cloud first and pass what it returns."""
    from .mls import _check_args
    _check_args('get_mls_smooth_preprocess_fn', radius, order, sigma, None)
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 1:
        raise ValueError('get_mls_smooth_preprocess_fn: iterations must be an integer >= 1 (got %r)' % (iterations,))

    def fn(xyz, normal, sensor):
        from .cloud import smooth_mls
        moved, fitted = smooth_mls(xyz, radius, normal=normal, iterations=iterations, order=order, sigma=sigma)
        return moved, fitted if normal is not None else None, sensor
    return fn


def compose_preprocess_fns(*fns):
    """The given functions applied one after the other, e.g. outlier filter -> downsample -> get_estimate_normal_preprocess_fn."""
    def fn(xyz, normal, sensor):
        for f in fns:
            xyz, normal, sensor = f(xyz, normal, sensor)
        return xyz, normal, sensor
    return fn
