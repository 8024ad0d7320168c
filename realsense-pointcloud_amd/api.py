"""Host-side mirror of the PCL class surface the reference's schemes call, over the C ABI.

Method names and argument meaning follow the reference call sites:
``pcl::IterativeClosestPoint`` (src/incremental_icp.hpp:46-63), ``pcl::NormalDistributions
Transform`` (src/ndt_edge_based_registration.hpp:38-43,71-72,83,104), ``pcl::ApproximateVoxel
Grid`` (src/icp_edge_based_registration.hpp:47,59-60) and ``pcl::transformPointCloud``
(src/incremental_icp.hpp:63).  Transforms cross this layer as 4x4 numpy arrays in the usual
row/column maths convention; the column-major packing of the ABI is handled here.
"""
import ctypes as C
import sys

import numpy as np

from . import lib as _l
from .cloud import POINT_DTYPE, PointCloud

CONV_STATES = ["NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES",
               "FAILURE_AFTER_MAX_ITERATIONS"]


def _colmajor(T):
    if T is None:
        return None
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(4, 4).T).copy()


def _rowmajor(buf):
    return np.array(buf, dtype=np.float32).reshape(4, 4).T.copy()


def _records(a):
    """(keepalive, pointer, n, stride) for a PointCloud / structured array / (n,>=3) float32."""
    if isinstance(a, PointCloud):
        a = a.points
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return a, a.ctypes.data, a.shape[0], a.dtype.itemsize
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("points must be a PointCloud, a structured array or an (n, >=3) float32 array")
    return a, a.ctypes.data, a.shape[0], a.shape[1] * 4


def device_count():
    n = C.c_int(0)
    _l.check(_l.lib().rsreg_device_count(C.byref(n)))
    return n.value


class Context:
    """One (device, stream) execution context; not thread-safe (include/rsreg.h)."""

    def __init__(self, device=0, stream=None, profiling=False):
        h = C.c_void_p()
        _l.check(_l.lib().rsreg_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device
        # a context holds ONE ICP target index, ONE ICP source and ONE NDT voxel grid: who uploaded each last
        self.icp_target_owner = self.icp_source_owner = self.ndt_target_owner = None
        if profiling:
            self.set_profiling(True)

    def set_profiling(self, on):
        _l.check(_l.lib().rsreg_ctx_set_profiling(self.h, int(bool(on))), self.h)

    def synchronize(self):
        _l.check(_l.lib().rsreg_ctx_synchronize(self.h), self.h)

    def prepare(self, frame_bytes=0, model_bytes=0, side_streams=False):
        """What a frame loop is about to need -- streams, pinned staging for frames of `frame_bytes`, a device buffer a model
        can grow to `model_bytes` in -- made on a thread of the context while the caller goes on (rsreg_ctx_prepare)."""
        _l.check(_l.lib().rsreg_ctx_prepare(self.h, int(frame_bytes), int(model_bytes), 1 if side_streams else 0), self.h)

    def wait_downloads(self):
        """Every DeviceCloud.download_async of this context has landed in its host array when this returns."""
        _l.check(_l.lib().rsreg_ctx_wait_downloads(self.h), self.h)

    def close(self):
        if getattr(self, "h", None):
            _l.lib().rsreg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- N-GPU
    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_uint8 * _l.UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _l.check(_l.lib().rsreg_comm_init(self.h, buf, rank, nranks), self.h)

    def allreduce_f64(self, arr):
        arr = np.ascontiguousarray(arr, np.float64)
        _l.check(_l.lib().rsreg_comm_allreduce_f64(self.h, arr.ctypes.data, arr.size), self.h)
        return arr


def comm_unique_id():
    buf = (C.c_uint8 * _l.UNIQUE_ID_BYTES)()
    _l.check(_l.lib().rsreg_comm_unique_id(buf))
    return bytes(buf)


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# pcl::Normal: 32 bytes -- normal_x, normal_y, normal_z, 0.f, curvature, three words of padding
NORMAL_DTYPE = np.dtype({"names": ["normal_x", "normal_y", "normal_z", "data_n3", "curvature", "pad0", "pad1", "pad2"],
                         "formats": ["<f4", "<f4", "<f4", "<f4", "<f4", "<u4", "<u4", "<u4"], "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})


class NormalCloud:
    """width / height / is_dense / points like pcl::PointCloud<pcl::Normal>; points: NORMAL_DTYPE records."""

    def __init__(self, points, width, height, is_dense):
        self.points, self.width, self.height, self.is_dense = points, int(width), int(height), bool(is_dense)

    def __len__(self):
        return len(self.points)


FPFH_DTYPE = np.dtype([("histogram", np.float32, (33,))])   # pcl::FPFHSignature33


class FPFHCloud(NormalCloud):
    """width / height / is_dense / points like pcl::PointCloud<pcl::FPFHSignature33>; points: FPFH_DTYPE records."""


# pcl::Correspondence (rsreg_correspondence): 12 bytes; distance is the squared distance
CORRESPONDENCE_DTYPE = np.dtype([("index_query", np.int32), ("index_match", np.int32), ("distance", np.float32)])


class DeviceCloud:
    """A cloud resident in HBM (rsreg_cloud): whole records plus width / height / is_dense.  What the
    reference's frame loop hands from step to step (filter -> align -> transformPointCloud -> operator+,
    icp_edge_based_registration.hpp:75-120) without the records leaving the GPU."""

    def __init__(self, cloud=None, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        _l.check(_l.lib().rsreg_cloud_create(self.ctx.h, C.byref(h)), self.ctx.h)
        self.h = h
        if cloud is not None:
            self.upload(cloud)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            _l.lib().rsreg_cloud_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, cloud):
        pts = np.ascontiguousarray(cloud.points)
        _l.check(_l.lib().rsreg_cloud_upload(self.h, pts.ctypes.data, len(pts), pts.dtype.itemsize, cloud.width, cloud.height,
                                             int(cloud.is_dense)), self.ctx.h)
        return self

    def upload_async(self, cloud):
        """upload() that returns once the records are staged: the PCIe copy runs beside the main stream's work and
        whatever touches this cloud next waits for it (rsreg_cloud_upload_async)."""
        pts = np.ascontiguousarray(cloud.points)
        _l.check(_l.lib().rsreg_cloud_upload_async(self.h, pts.ctypes.data, len(pts), pts.dtype.itemsize, cloud.width, cloud.height,
                                                   int(cloud.is_dense)), self.ctx.h)
        return self

    def upload_deferred(self, cloud):
        """upload_async() that returns before the records have been read (rsreg_cloud_upload_deferred): a thread of the
        context stages them and queues their copy.  `cloud.points` must not change until a call that reads or rewrites
        this DeviceCloud has returned (the array itself is kept alive here)."""
        pts = np.ascontiguousarray(cloud.points)
        self._deferred_src = pts
        _l.check(_l.lib().rsreg_cloud_upload_deferred(self.h, pts.ctypes.data, len(pts), pts.dtype.itemsize, cloud.width, cloud.height,
                                                      int(cloud.is_dense)), self.ctx.h)
        return self

    def info(self):
        n, s = C.c_size_t(0), C.c_size_t(0)
        w, h, d = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        _l.check(_l.lib().rsreg_cloud_info(self.h, C.byref(n), C.byref(s), C.byref(w), C.byref(h), C.byref(d)), self.ctx.h)
        return n.value, s.value, w.value, h.value, bool(d.value)

    def __len__(self):
        return self.info()[0]

    @property
    def stamp(self):
        """(id, version): changes whenever the records in HBM are rewritten (upload, filter, transform, concat, align into it)."""
        import ctypes as C
        i, v = C.c_uint64(), C.c_uint64()
        _l.check(_l.lib().rsreg_cloud_version(self.h, C.byref(i), C.byref(v)))
        return (i.value, v.value)

    @property
    def device_ptr(self):
        """Address of the records in HBM (an int; 0 for a cloud without a buffer)."""
        return int(_l.lib().rsreg_cloud_device_ptr(self.h) or 0)

    def download(self):
        n, stride, w, h, dense = self.info()
        assert stride == POINT_DTYPE.itemsize or n == 0
        pts = np.zeros(n, POINT_DTYPE)
        _l.check(_l.lib().rsreg_cloud_download(self.h, pts.ctypes.data, n), self.ctx.h)
        return PointCloud(pts, width=w, height=h, is_dense=dense)

    def download_async(self, out, offset=0):
        """download() that returns at once (rsreg_cloud_download_async): this cloud's records, as they are when the
        context's stream gets here, go to out[offset:offset + len(self)] (a C-contiguous POINT_DTYPE array the caller
        keeps alive and does not touch until ctx.wait_downloads() has returned); the cloud may be rewritten or dropped
        right away.  Returns the number of records on their way."""
        n = self.info()[0]
        if not (isinstance(out, np.ndarray) and out.dtype == POINT_DTYPE and out.flags.c_contiguous and out.ndim == 1):
            raise ValueError("download_async needs a C-contiguous 1-D POINT_DTYPE array")
        if offset < 0 or offset + n > len(out):
            raise ValueError("download_async: %d records do not fit behind offset %d of %d" % (n, offset, len(out)))
        _l.check(_l.lib().rsreg_cloud_download_async(self.h, out.ctypes.data + offset * POINT_DTYPE.itemsize, n), self.ctx.h)
        return n

    def knn_mean_distance(self, mean_k):
        """StatisticalOutlierRemoval's first pass on its own (rsreg_cloud_knn_mean_distance): for every record the mean
        float distance to its mean_k nearest neighbours among the finite records (exact search), 0 for a non-finite record."""
        out = np.zeros(self.info()[0], np.float32)
        _l.check(_l.lib().rsreg_cloud_knn_mean_distance(self.ctx.h, self.h, int(mean_k), out.ctypes.data), self.ctx.h)
        return out

    def knn(self, k):
        """nearestKSearch of every record in its own cloud (rsreg_cloud_knn, exact): (idx, d2), each (n, k) -- int32 original
        record indices and float32 squared distances, ascending by (d2, index), ties: lowest index; the record itself and exact
        copies count.  A non-finite record's row is -1 / 0."""
        n = self.info()[0]
        idx = np.zeros((n, int(k)), np.int32)
        d2 = np.zeros((n, int(k)), np.float32)
        _l.check(_l.lib().rsreg_cloud_knn(self.ctx.h, self.h, int(k), idx.ctypes.data, d2.ctypes.data), self.ctx.h)
        return idx, d2

    def normals_cloud(self, k, viewpoint=None):
        """pcl::NormalEstimation with setKSearch(k) (rsreg_cloud_normals): a DeviceCloud of 32-byte pcl::Normal records."""
        out = DeviceCloud(ctx=self.ctx)
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(3)
        _l.check(_l.lib().rsreg_cloud_normals(self.ctx.h, self.h, int(k), None if vp is None else vp.ctypes.data, out.h), self.ctx.h)
        return out

    def normals(self, k, viewpoint=None):
        """(n, 4) float32: normal_x, normal_y, normal_z, curvature of every record (NaN for a non-finite one)."""
        out = self.normals_cloud(k, viewpoint)
        rec = out.download_normals().points
        out.close()
        return np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], axis=1)

    def gicp_covariances_cloud(self, k=20, epsilon=1e-3):
        """GeneralizedIterativeClosestPoint's computeCovariances (rsreg_cloud_gicp_covariances; include/rsreg.h holds the contract):
        a DeviceCloud of 48-byte records, six doubles (xx, xy, xz, yy, yz, zz) of I - (1 - epsilon) n n^T per record."""
        out = DeviceCloud(ctx=self.ctx)
        rc = _l.lib().rsreg_cloud_gicp_covariances(self.ctx.h, self.h, int(k), float(epsilon), out.h)
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return out

    def gicp_covariances(self, k=20, epsilon=1e-3):
        """(covariances (n, 6) float64 -- NaN rows for non-finite records --, is_dense of the result)."""
        out = self.gicp_covariances_cloud(k, epsilon)
        n, stride, _, _, dense = out.info()
        if n and stride != 48:
            raise ValueError("the device cloud does not hold 48-byte covariance records")
        cov = np.zeros((n, 6), np.float64)
        _l.check(_l.lib().rsreg_cloud_download(out.h, cov.ctypes.data, n), self.ctx.h)
        out.close()
        return cov, dense

    def lab_cloud(self):
        """RGB -> normalised CIE L*a*b* of every record (rsreg_cloud_lab; include/rsreg.h holds the formula): a DeviceCloud of
        16-byte records {L / 100, a / 120, b / 120, 0}."""
        out = DeviceCloud(ctx=self.ctx)
        rc = _l.lib().rsreg_cloud_lab(self.ctx.h, self.h, out.h)
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return out

    def lab(self):
        """(n, 3) float32: L', a', b' of every record."""
        out = self.lab_cloud()
        n, stride = out.info()[:2]
        if n and stride != 16:
            raise ValueError("the device cloud does not hold 16-byte colour records")
        rec = np.zeros((n, 4), np.float32)
        _l.check(_l.lib().rsreg_cloud_download(out.h, rec.ctypes.data, n), self.ctx.h)
        out.close()
        return rec[:, :3].copy()

    def _normals_on_device(self, normals):
        """(a DeviceCloud of this context that holds the normals, whether it was made here): a DeviceCloud as it is, a NormalCloud,
        a structured array that starts with normal_x, normal_y, normal_z, or an (n, >= 3) float32 array uploaded."""
        if isinstance(normals, DeviceCloud):
            return normals, False
        rec = normals.points if hasattr(normals, "points") else np.asarray(normals)
        if rec.dtype.names is None:
            rec = np.ascontiguousarray(rec, np.float32)
            if rec.ndim != 2 or rec.shape[1] < 3:
                raise ValueError("normals must be a DeviceCloud, a NormalCloud, a structured array that starts with normal_x or an (n, >=3) float32 array")
            rec = rec.view(np.dtype((np.void, rec.shape[1] * 4))).reshape(-1)
        elif rec.dtype.names[:3] != ("normal_x", "normal_y", "normal_z") or rec.dtype.fields["normal_x"][1] != 0:
            raise ValueError("the normals' records must start with normal_x, normal_y, normal_z")
        return DeviceCloud(NormalCloud(rec, len(rec), 1, True), ctx=self.ctx), True

    def fpfh_cloud(self, normals, k):
        """pcl::FPFHEstimation with setKSearch(k) (rsreg_cloud_fpfh; include/rsreg.h holds the contract): a DeviceCloud of 132-byte
        pcl::FPFHSignature33 records.  normals: see fpfh()."""
        nrm, made = self._normals_on_device(normals)
        out = DeviceCloud(ctx=self.ctx)
        rc = _l.lib().rsreg_cloud_fpfh(self.ctx.h, self.h, nrm.h, int(k), out.h)
        if made:
            nrm.close()
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return out

    def fpfh(self, normals, k):
        """(n, 33) float32: the Fast Point Feature Histogram of every record over its k nearest neighbours, three blocks of 11 bins
        that each sum to 100 (NaN for a record that is not finite or whose normal is not).  normals: a DeviceCloud of this context
        (what normals_cloud() returns), a NormalCloud, or an (n, >= 3) float32 array."""
        out = self.fpfh_cloud(normals, k)
        hist = out.download_fpfh().points["histogram"]
        out.close()
        return hist

    def spfh(self, normals, k):
        """(n, 33) float32: the Simplified Point Feature Histogram of every record (rsreg_cloud_spfh), the first pass of fpfh():
        zeros for a record that is not finite or whose normal is not."""
        nrm, made = self._normals_on_device(normals)
        out = np.zeros((self.info()[0], 33), np.float32)
        rc = _l.lib().rsreg_cloud_spfh(self.ctx.h, self.h, nrm.h, int(k), out.ctypes.data)
        if made:
            nrm.close()
        _l.check(rc, self.ctx.h)
        return out

    def fpfh_radius_cloud(self, normals, radius):
        """pcl::FPFHEstimationOMP with setRadiusSearch(radius) (rsreg_cloud_fpfh_radius; include/rsreg.h holds the contract): a
        DeviceCloud of 132-byte pcl::FPFHSignature33 records over the exact radius search, any number of neighbours.  normals: see
        fpfh()."""
        nrm, made = self._normals_on_device(normals)
        out = DeviceCloud(ctx=self.ctx)
        rc = _l.lib().rsreg_cloud_fpfh_radius(self.ctx.h, self.h, nrm.h, float(radius), out.h)
        if made:
            nrm.close()
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return out

    def fpfh_radius(self, normals, radius):
        """(n, 33) float32: the Fast Point Feature Histogram of every record over its neighbours within `radius`, three blocks of 11
        bins that each sum to 100 or are all zero (NaN for a record that is not finite or whose normal is not)."""
        out = self.fpfh_radius_cloud(normals, radius)
        hist = out.download_fpfh().points["histogram"]
        out.close()
        return hist

    def spfh_radius(self, normals, radius, counts=False):
        """(n, 33) float32: the Simplified Point Feature Histogram of every record over its neighbours within `radius`
        (rsreg_cloud_spfh_radius), the first pass of fpfh_radius(): zeros for a record that is not finite or whose normal is not.
        counts: (rows, m) with m (n,) uint32, every record's number of neighbours -- what radius_count() gives."""
        nrm, made = self._normals_on_device(normals)
        n = self.info()[0]
        out = np.zeros((n, 33), np.float32)
        m = np.zeros(n, np.uint32)
        rc = _l.lib().rsreg_cloud_spfh_radius(self.ctx.h, self.h, nrm.h, float(radius), out.ctypes.data, m.ctypes.data if counts else None)
        if made:
            nrm.close()
        _l.check(rc, self.ctx.h)
        return (out, m) if counts else out

    # ---- setSearchSurface: this cloud's records are the queries, `surface` (a DeviceCloud of this context; this one is allowed) is
    # searched (include/rsreg.h holds the contract)
    def radius_count_surface(self, surface, radius):
        """radiusSearch of every record of this cloud in `surface`, counted (rsreg_cloud_radius_count_surface, exact): uint32 per
        record, the finite surface records with float32 d2 < (float)(radius * radius), strictly; 0 for a non-finite record."""
        out = np.zeros(self.info()[0], np.uint32)
        _l.check(_l.lib().rsreg_cloud_radius_count_surface(self.ctx.h, self.h, surface.h, float(radius), out.ctypes.data), self.ctx.h)
        return out

    def normals_radius_surface_cloud(self, surface, radius, viewpoint=None):
        """pcl::NormalEstimation with setSearchSurface(surface) and setRadiusSearch(radius) (rsreg_cloud_normals_radius_surface): a
        DeviceCloud of one 32-byte pcl::Normal record per record of this cloud, from its neighbours in `surface`; fewer than three:
        NaNs."""
        out = DeviceCloud(ctx=self.ctx)
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(3)
        rc = _l.lib().rsreg_cloud_normals_radius_surface(self.ctx.h, self.h, surface.h, float(radius), None if vp is None else vp.ctypes.data, out.h)
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return out

    def normals_radius_surface(self, surface, radius, viewpoint=None):
        """(n, 4) float32: normal_x, normal_y, normal_z, curvature of every record of this cloud over its neighbours in `surface`."""
        out = self.normals_radius_surface_cloud(surface, radius, viewpoint)
        rec = out.download_normals().points
        out.close()
        return np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], axis=1)

    def fpfh_radius_surface_cloud(self, surface, normals, radius, n_spfh=False):
        """pcl::FPFHEstimationOMP with setSearchSurface(surface), setInputNormals(normals: the SURFACE's, see fpfh()) and
        setRadiusSearch(radius) (rsreg_cloud_fpfh_radius_surface): a DeviceCloud of one 132-byte pcl::FPFHSignature33 record per
        record of this cloud.  n_spfh: (cloud, the number of surface records whose SPFH row was computed)."""
        nrm, made = surface._normals_on_device(normals)
        out = DeviceCloud(ctx=self.ctx)
        n = C.c_uint64(0)
        rc = _l.lib().rsreg_cloud_fpfh_radius_surface(self.ctx.h, self.h, surface.h, nrm.h, float(radius), out.h, C.byref(n))
        if made:
            nrm.close()
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return (out, int(n.value)) if n_spfh else out

    def fpfh_radius_surface(self, surface, normals, radius):
        """(n, 33) float32: the Fast Point Feature Histogram of every record of this cloud over its neighbours in `surface` (NaN
        for a record that is not finite or has no neighbour)."""
        out = self.fpfh_radius_surface_cloud(surface, normals, radius)
        hist = out.download_fpfh().points["histogram"]
        out.close()
        return hist

    def spfh_radius_surface(self, surface, normals, radius):
        """(rows, needed, m): the (ns, 33) float32 SPFH rows of `surface` (rsreg_cloud_spfh_radius_surface) -- the rows
        surface.spfh_radius(normals, radius) gives where needed[j] (ns, uint32) is 1, a neighbour of a record of this cloud, zero
        elsewhere -- and m (n, uint32), every record's number of neighbours in `surface`."""
        nrm, made = surface._normals_on_device(normals)
        ns = surface.info()[0]
        out = np.zeros((ns, 33), np.float32)
        needed = np.zeros(ns, np.uint32)
        m = np.zeros(self.info()[0], np.uint32)
        rc = _l.lib().rsreg_cloud_spfh_radius_surface(self.ctx.h, self.h, surface.h, nrm.h, float(radius), out.ctypes.data, needed.ctypes.data,
                                                      m.ctypes.data)
        if made:
            nrm.close()
        _l.check(rc, self.ctx.h)
        return out, needed, m

    def download_fpfh(self):
        """download() of a cloud of pcl::FPFHSignature33 records (what FPFHEstimation.compute returns): an FPFHCloud."""
        n, stride, w, h, dense = self.info()
        if n and stride != FPFH_DTYPE.itemsize:
            raise ValueError("the device cloud does not hold 132-byte pcl::FPFHSignature33 records")
        rec = np.zeros(n, FPFH_DTYPE)
        _l.check(_l.lib().rsreg_cloud_download(self.h, rec.ctypes.data, n), self.ctx.h)
        return FPFHCloud(rec, w, h, dense)

    def feature_knn(self, target, k):
        """(index (ns, k) int32, sqr_dist (ns, k) float32): for every valid row of this descriptor cloud (records that start with 33
        floats, what fpfh_cloud() returns) the k valid rows of `target`, a DeviceCloud of this context, with the smallest float32
        squared distance, ascending by (d2, index) (rsreg_cloud_feature_knn, exact; include/rsreg.h holds the contract).  A row with
        a float that is not finite gets -1 and 0.  1 <= k <= 16."""
        ns = self.info()[0]
        k = int(k)
        idx = np.full((ns, max(k, 0)), -1, np.int32)
        d2 = np.zeros((ns, max(k, 0)), np.float32)
        _l.check(_l.lib().rsreg_cloud_feature_knn(self.ctx.h, self.h, target.h, k, idx.ctypes.data, d2.ctypes.data), self.ctx.h)
        return idx, d2

    def feature_correspondences(self, target, max_distance=None, reciprocal=False):
        """pcl::registration::CorrespondenceEstimation's determineCorrespondences (reciprocal: determineReciprocalCorrespondences)
        between this descriptor cloud and `target` (rsreg_cloud_feature_correspondences): a CORRESPONDENCE_DTYPE array ordered by
        index_query; distance is the squared distance.  max_distance None: DBL_MAX, PCL's default, which keeps every match."""
        ns = self.info()[0]
        out = np.zeros(ns, CORRESPONDENCE_DTYPE)
        found = C.c_size_t(0)
        md = sys.float_info.max if max_distance is None else float(max_distance)
        _l.check(_l.lib().rsreg_cloud_feature_correspondences(self.ctx.h, self.h, target.h, md, int(bool(reciprocal)), out.ctypes.data, ns,
                                                              C.byref(found)), self.ctx.h)
        return out[:found.value]

    def count_inliers(self, target, corr, transforms, threshold):
        """uint32 per transform: the pairs of `corr` (a CORRESPONDENCE_DTYPE array; index_query a record of this cloud, index_match
        one of `target`) within `threshold` of their match once the transform has moved the source point
        (rsreg_cloud_count_inliers; include/rsreg.h holds the arithmetic).  transforms: (H, 4, 4), or one 4 x 4."""
        corr = np.ascontiguousarray(corr, CORRESPONDENCE_DTYPE)
        t = np.asarray(transforms, np.float32)
        t = t.reshape(-1, 4, 4)
        packed = np.ascontiguousarray(t.transpose(0, 2, 1))   # column-major, one after the other
        out = np.zeros(len(t), np.uint32)
        _l.check(_l.lib().rsreg_cloud_count_inliers(self.ctx.h, self.h, target.h, corr.ctypes.data, len(corr), packed.ctypes.data, len(t), float(threshold),
                                                    out.ctypes.data), self.ctx.h)
        return out

    def estimate_rigid_svd(self, target, corr):
        """(T 4 x 4 float32, the 17 sums float64): TransformationEstimationSVD over the finite pairs of `corr`
        (rsreg_cloud_estimate_rigid_svd); T is umeyama_from_sums of the sums."""
        corr = np.ascontiguousarray(corr, CORRESPONDENCE_DTYPE)
        t, sums = np.zeros(16, np.float32), np.zeros(_l.NUM_SUMS, np.float64)
        _l.check(_l.lib().rsreg_cloud_estimate_rigid_svd(self.ctx.h, self.h, target.h, corr.ctypes.data, len(corr), t.ctypes.data, sums.ctypes.data), self.ctx.h)
        return _rowmajor(t), sums

    def sac_correspondences(self, target, corr, capacity=None, **params):
        """pcl::registration::CorrespondenceRejectorSampleConsensus over `corr` (rsreg_cloud_sac_correspondences): (the kept
        correspondences in input order, SacResult).  params: inlier_threshold, max_iterations, probability, refit_rounds,
        min_sample_distance, seed (sac_params()).  capacity: room for so many records (None: all); the result's n_out is the
        number kept, however many were written."""
        corr = np.ascontiguousarray(corr, CORRESPONDENCE_DTYPE)
        p = sac_params(**params)
        room = len(corr) if capacity is None else int(capacity)
        out = np.zeros(room, CORRESPONDENCE_DTYPE)
        found, res = C.c_size_t(0), _l.SacResult()
        _l.check(_l.lib().rsreg_cloud_sac_correspondences(self.ctx.h, self.h, target.h, corr.ctypes.data, len(corr), C.byref(p), out.ctypes.data, room,
                                                          C.byref(found), C.byref(res)), self.ctx.h)
        return out[:min(found.value, room)], SacResult(res, found.value)

    def score_transforms(self, target, transforms, max_range):
        """(counts uint32, sums float64), one of each per transform: the records of this cloud whose exact nearest record of `target`
        lies within `max_range` once the transform has moved them, and the sum of those squared distances
        (rsreg_cloud_score_transforms; include/rsreg.h holds the arithmetic and the order of the sum).  transforms: (H, 4, 4), or one
        4 x 4."""
        t = np.asarray(transforms, np.float32).reshape(-1, 4, 4)
        packed = np.ascontiguousarray(t.transpose(0, 2, 1))   # column-major, one after the other
        counts, sums = np.zeros(len(t), np.uint32), np.zeros(len(t), np.float64)
        _l.check(_l.lib().rsreg_cloud_score_transforms(self.ctx.h, self.h, target.h, packed.ctypes.data, len(t), float(max_range), counts.ctypes.data,
                                                       sums.ctypes.data), self.ctx.h)
        return counts, sums

    def prerejective(self, target, neighbor_index, capacity=None, **params):
        """pcl::SampleConsensusPrerejective (rsreg_cloud_prerejective): (the winner's inlier records of this cloud in ascending order,
        PrerejResult).  neighbor_index: (ns, k) int32, what source_features.feature_knn(target_features, k)[0] returned.  params:
        max_iterations, similarity_threshold, max_correspondence_distance, inlier_fraction, select_by_inliers, seed (prerej_params()).
        capacity: room for so many records (None: all); the result's n_out is the number of inliers, however many were written."""
        nbr = np.ascontiguousarray(neighbor_index, np.int32)
        ns = self.info()[0]
        if nbr.ndim != 2 or nbr.shape[0] != ns:
            raise ValueError("neighbor_index must be (%d, k) int32" % ns)
        p = prerej_params(**params)
        room = ns if capacity is None else int(capacity)
        out = np.zeros(room, np.int32)
        found, res = C.c_size_t(0), _l.PrerejResult()
        _l.check(_l.lib().rsreg_cloud_prerejective(self.ctx.h, self.h, target.h, nbr.ctypes.data, nbr.shape[1], C.byref(p), out.ctypes.data, room,
                                                   C.byref(found), C.byref(res)), self.ctx.h)
        return out[:min(found.value, room)], PrerejResult(res, found.value)

    def _scia_table(self, neighbor_index):
        nbr = np.ascontiguousarray(neighbor_index, np.int32)
        ns = self.info()[0]
        if nbr.ndim != 2 or nbr.shape[0] != ns:
            raise ValueError("neighbor_index must be (%d, k) int32" % ns)
        return nbr

    def error_transforms(self, target, transforms, error_function, max_correspondence_distance):
        """float64 per transform: SampleConsensusInitialAlignment's error of this cloud moved by it against `target`
        (rsreg_cloud_error_transforms; include/rsreg.h holds the terms and the order of the sum).  error_function: SCIA_TRUNCATED or
        SCIA_HUBER; max_correspondence_distance is compared, as a float, with the SQUARED distance.  transforms: (H, 4, 4), or one 4 x 4."""
        t = np.asarray(transforms, np.float32).reshape(-1, 4, 4)
        packed = np.ascontiguousarray(t.transpose(0, 2, 1))   # column-major, one after the other
        errors = np.zeros(len(t), np.float64)
        _l.check(_l.lib().rsreg_cloud_error_transforms(self.ctx.h, self.h, target.h, packed.ctypes.data, len(t), int(error_function),
                                                       float(max_correspondence_distance), errors.ctypes.data), self.ctx.h)
        return errors

    def initial_alignment_hypotheses(self, target, neighbor_index, first=0, count=1, **params):
        """(transforms (count, 4, 4) float32, valid (count,) bool, samples (count, 16) int32) of the hypotheses first .. first + count - 1
        of SampleConsensusInitialAlignment: the sampler and the fit alone (rsreg_cloud_initial_alignment_hypotheses).  An invalid
        hypothesis's transform is NaN; samples: the source records in [:, :8], their target records in [:, 8:], -1 where there is none."""
        nbr = self._scia_table(neighbor_index)
        p = scia_params(**params)
        t, valid, samples = np.zeros((count, 16), np.float32), np.zeros(count, np.int32), np.zeros((count, 16), np.int32)
        _l.check(_l.lib().rsreg_cloud_initial_alignment_hypotheses(self.ctx.h, self.h, target.h, nbr.ctypes.data, nbr.shape[1], C.byref(p), int(first), count,
                                                                   t.ctypes.data, valid.ctypes.data, samples.ctypes.data), self.ctx.h)
        return np.ascontiguousarray(t.reshape(count, 4, 4).transpose(0, 2, 1)), valid != 0, samples

    def initial_alignment(self, target, neighbor_index, guess=None, errors=False, **params):
        """pcl::SampleConsensusInitialAlignment (rsreg_cloud_initial_alignment): a SciaResult, or (SciaResult, the error of every
        hypothesis: max_iterations float64, NaN for an invalid or unused one) with errors=True.  neighbor_index: (ns, k) int32, what
        source_features.feature_knn(target_features, k)[0] returned.  guess: a 4 x 4 that is scored first and spends an iteration.
        params: max_correspondence_distance, min_sample_distance, nr_samples, error_function, max_iterations, seed (scia_params())."""
        nbr = self._scia_table(neighbor_index)
        p = scia_params(**params)
        g = None if guess is None else _colmajor(guess)
        errs = np.zeros(max(int(p.max_iterations), 0), np.float64) if errors else None
        res = _l.SciaResult()
        _l.check(_l.lib().rsreg_cloud_initial_alignment(self.ctx.h, self.h, target.h, nbr.ctypes.data, nbr.shape[1], C.byref(p), None if g is None else g.ctypes.data,
                                                        None if errs is None else errs.ctypes.data, C.byref(res)), self.ctx.h)
        return (SciaResult(res), errs) if errors else SciaResult(res)

    def radius_count(self, radius):
        """radiusSearch of every record in its own cloud, counted (rsreg_cloud_radius_count, exact): uint32 per record, its
        neighbours with float32 d2 < (float)(radius * radius) -- strictly, itself and exact copies among them; 0 for a non-finite
        record."""
        out = np.zeros(self.info()[0], np.uint32)
        _l.check(_l.lib().rsreg_cloud_radius_count(self.ctx.h, self.h, float(radius), out.ctypes.data), self.ctx.h)
        return out

    def radius_outlier_removal(self, radius, min_neighbors, negative=False, keep_organized=False, out=None):
        """pcl::RadiusOutlierRemoval (rsreg_cloud_radius_outlier_removal): a record is removed when its radius_count is
        <= min_neighbors (negative: when it is above).  out: None = a new DeviceCloud, or a DeviceCloud of this context (this one
        is allowed).  Returns (out, the number of kept records)."""
        made = out is None
        if made:
            out = DeviceCloud(ctx=self.ctx)
        kept = C.c_uint64(0)
        rc = _l.lib().rsreg_cloud_radius_outlier_removal(self.ctx.h, self.h, float(radius), int(min_neighbors), int(bool(negative)),
                                                         int(bool(keep_organized)), out.h, C.byref(kept))
        if rc and made:
            out.close()
        _l.check(rc, self.ctx.h)
        return out, int(kept.value)

    def euclidean_clusters(self, tolerance, min_size=1, max_size=2**31 - 1):
        """pcl::EuclideanClusterExtraction (rsreg_cloud_euclidean_clusters): the connected components of "float32 d2 < (float)(tolerance
        * tolerance)" with min_size <= records <= max_size, ranked by size descending (ties: the smallest record index first).
        Returns (labels, indices, offsets): labels (n,) int32, every record's rank or -1; indices (uint32) the records cluster by
        cluster, ascending inside one; offsets (n_clusters + 1,) uint32, cluster c is indices[offsets[c]:offsets[c + 1]]."""
        n = self.info()[0]
        p = cluster_params(tolerance, min_size, max_size)
        labels, indices, offsets = np.empty(n, np.int32), np.empty(n, np.uint32), np.empty(n + 1, np.uint32)
        count = C.c_uint32(0)
        _l.check(_l.lib().rsreg_cloud_euclidean_clusters(self.ctx.h, self.h, C.byref(p), labels.ctypes.data, indices.ctypes.data, offsets.ctypes.data,
                                                         n, C.byref(count)), self.ctx.h)
        offsets = offsets[:count.value + 1].copy()
        return labels, indices[:int(offsets[-1])].copy(), offsets

    def cluster_filter(self, tolerance, rank_lo=0, rank_hi=1, min_size=1, max_size=2**31 - 1, negative=False, keep_organized=False, out=None):
        """rsreg_cloud_cluster_filter: keeps the records whose cluster (euclidean_clusters) has a rank in [rank_lo, rank_hi) -- the
        default: the largest cluster only; negative: the other records.  out: None = a new DeviceCloud, or a DeviceCloud of this
        context (this one is allowed).  Returns (out, the number of kept records)."""
        made = out is None
        if made:
            out = DeviceCloud(ctx=self.ctx)
        p = cluster_params(tolerance, min_size, max_size)
        kept = C.c_uint64(0)
        rc = _l.lib().rsreg_cloud_cluster_filter(self.ctx.h, self.h, C.byref(p), int(rank_lo), int(rank_hi), int(bool(negative)),
                                                 int(bool(keep_organized)), out.h, C.byref(kept))
        if rc and made:
            out.close()
        _l.check(rc, self.ctx.h)
        return out, int(kept.value)

    def plane_count(self, coeffs, threshold):
        """uint32 per model: the finite records with float32 |((a x + b y) + c z) + d| < threshold, strictly (rsreg_cloud_plane_count;
        include/rsreg.h holds the arithmetic).  coeffs: (H, 4) float32, or one model."""
        m = np.ascontiguousarray(np.asarray(coeffs, np.float32).reshape(-1, 4))
        out = np.zeros(len(m), np.uint32)
        _l.check(_l.lib().rsreg_cloud_plane_count(self.ctx.h, self.h, m.ctypes.data, len(m), float(threshold), out.ctypes.data), self.ctx.h)
        return out

    def plane_hypotheses(self, first=0, count=1, **params):
        """(coeffs (count, 4) float32, samples (count, 4) int32, valid (count,) bool) of the plane hypotheses first .. first + count - 1:
        the sampler and the fit alone (rsreg_cloud_plane_hypotheses).  An invalid hypothesis's model is NaN; samples: the three
        records and the try that gave them, -1 after sixteen bad tries.  params: plane_params()."""
        p = plane_params(**params)
        coeffs, samples, valid = np.zeros((count, 4), np.float32), np.zeros((count, 4), np.int32), np.zeros(count, np.int32)
        _l.check(_l.lib().rsreg_cloud_plane_hypotheses(self.ctx.h, self.h, C.byref(p), int(first), count, coeffs.ctypes.data, samples.ctypes.data,
                                                       valid.ctypes.data), self.ctx.h)
        return coeffs, samples, valid != 0

    def segment_plane(self, capacity=None, **params):
        """pcl::SACSegmentation with a plane model and RANSAC (rsreg_cloud_plane_segment): (coefficients (4,) float32, the inliers'
        record indices int32 ascending, PlaneResult).  params: distance_threshold, max_iterations, probability,
        optimize_coefficients, axis, eps_angle, seed (plane_params()).  capacity: room for so many indices (None: all); the
        result's n_inliers is their number, however many were written."""
        p = plane_params(**params)
        room = self.info()[0] if capacity is None else int(capacity)
        coeff, idx = np.zeros(4, np.float32), np.zeros(room, np.int32)
        found, res = C.c_size_t(0), _l.PlaneResult()
        _l.check(_l.lib().rsreg_cloud_plane_segment(self.ctx.h, self.h, C.byref(p), coeff.ctypes.data, idx.ctypes.data if room else None, room,
                                                    C.byref(found), C.byref(res)), self.ctx.h)
        return coeff, idx[:min(found.value, room)], PlaneResult(res)

    def plane_filter(self, coeff, threshold, negative=False, keep_organized=False, out=None):
        """rsreg_cloud_plane_filter: keeps the inliers of the model `coeff` (a, b, c, d) at `threshold` -- negative: every other
        record.  out: None = a new DeviceCloud, or a DeviceCloud of this context (this one is allowed).  Returns (out, the number
        of kept records)."""
        made = out is None
        if made:
            out = DeviceCloud(ctx=self.ctx)
        m = np.ascontiguousarray(np.asarray(coeff, np.float32).reshape(4))
        kept = C.c_uint64(0)
        rc = _l.lib().rsreg_cloud_plane_filter(self.ctx.h, self.h, m.ctypes.data, float(threshold), int(bool(negative)), int(bool(keep_organized)),
                                               out.h, C.byref(kept))
        if rc and made:
            out.close()
        _l.check(rc, self.ctx.h)
        return out, int(kept.value)

    def extract_indices(self, indices, negative=False, out=None):
        """pcl::ExtractIndices (rsreg_cloud_extract_indices): the records `indices` names, in that order and with its repeats --
        negative: the records it does not name, in input order.  out: None = a new DeviceCloud, or a DeviceCloud of this context
        (this one is allowed).  Returns (out, the number of kept records)."""
        made = out is None
        if made:
            out = DeviceCloud(ctx=self.ctx)
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        kept = C.c_uint64(0)
        rc = _l.lib().rsreg_cloud_extract_indices(self.ctx.h, self.h, idx.ctypes.data if len(idx) else None, len(idx), int(bool(negative)), out.h,
                                                  C.byref(kept))
        if rc and made:
            out.close()
        _l.check(rc, self.ctx.h)
        return out, int(kept.value)

    def normals_radius_cloud(self, radius, viewpoint=None):
        """pcl::NormalEstimation with setRadiusSearch(radius) (rsreg_cloud_normals_radius): a DeviceCloud of 32-byte pcl::Normal
        records; fewer than three neighbours within the radius: NaNs."""
        out = DeviceCloud(ctx=self.ctx)
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(3)
        rc = _l.lib().rsreg_cloud_normals_radius(self.ctx.h, self.h, float(radius), None if vp is None else vp.ctypes.data, out.h)
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return out

    def normals_radius(self, radius, viewpoint=None):
        """(n, 4) float32: normal_x, normal_y, normal_z, curvature of every record (NaN for a non-finite one and for one with
        fewer than three neighbours within the radius)."""
        out = self.normals_radius_cloud(radius, viewpoint)
        rec = out.download_normals().points
        out.close()
        return np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], axis=1)

    def iss_saliency(self, **params):
        """The first pass of pcl::ISSKeypoint3D (rsreg_cloud_iss_saliency; params: the fields of iss_params(), salient_radius
        among them): (eig (n, 3) float64, the eigenvalues of every record's scatter over its neighbours within the salient radius,
        ascending; saliency (n,) float64, the smallest one where both ratios are below their gammas, else 0; counts (n,) uint32,
        what radius_count(salient_radius) gives).  Zeros for a non-finite record and for one below min_neighbors."""
        p = iss_params(**params)
        n = self.info()[0]
        eig, sal, m = np.zeros((n, 3), np.float64), np.zeros(n, np.float64), np.zeros(n, np.uint32)
        _l.check(_l.lib().rsreg_cloud_iss_saliency(self.ctx.h, self.h, C.byref(p), eig.ctypes.data, sal.ctypes.data, m.ctypes.data), self.ctx.h)
        return eig, sal, m

    def iss_non_max(self, saliency, radius, min_neighbors):
        """The second pass of pcl::ISSKeypoint3D over the caller's saliencies (rsreg_cloud_iss_non_max): (n,) bool, True where
        saliency[i] > 0, the record has min_neighbors or more neighbours within `radius`, and none of them has a larger saliency."""
        n = self.info()[0]
        sal = np.ascontiguousarray(saliency, np.float64).reshape(-1)
        if len(sal) != n:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "one saliency per record")
        out = np.zeros(n, np.uint8)
        _l.check(_l.lib().rsreg_cloud_iss_non_max(self.ctx.h, self.h, sal.ctypes.data, float(radius), int(min_neighbors), out.ctypes.data), self.ctx.h)
        return out.astype(bool)

    def iss_keypoints(self, **params):
        """pcl::ISSKeypoint3D (rsreg_cloud_iss_keypoints; params: the fields of iss_params()): (a DeviceCloud of the keypoints'
        records in ascending record index, their indices as an int32 array -- PCL's getKeypointsIndices)."""
        p = iss_params(**params)
        n = self.info()[0]
        idx = np.zeros(max(n, 1), np.int32)
        out = DeviceCloud(ctx=self.ctx)
        found = C.c_uint64(0)
        rc = _l.lib().rsreg_cloud_iss_keypoints(self.ctx.h, self.h, C.byref(p), out.h, idx.ctypes.data, n, C.byref(found))
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return out, idx[:int(found.value)].copy()

    def integral_normals_cloud(self, params=None, rect=False):
        """pcl::IntegralImageNormalEstimation of this organized cloud (rsreg_cloud_integral_normals; params: iin_params(),
        None = PCL's defaults): a DeviceCloud of 32-byte pcl::Normal records.  rect=True: (cloud, the window size of every
        record as a uint8 array, 0 = no window)."""
        out = DeviceCloud(ctx=self.ctx)
        sizes = np.zeros(self.info()[0], np.uint8) if rect else None
        rc = _l.lib().rsreg_cloud_integral_normals(self.ctx.h, self.h, None if params is None else C.byref(params), out.h,
                                                   sizes.ctypes.data if rect else None)
        if rc:
            out.close()
        _l.check(rc, self.ctx.h)
        return (out, sizes) if rect else out

    def integral_normals(self, params=None, rect=False):
        """(n, 4) float32: normal_x, normal_y, normal_z, curvature (always NaN: the method defines none) of every record, NaN
        where there is no normal; rect=True: (that, the window sizes)."""
        res = self.integral_normals_cloud(params, rect)
        out = res[0] if rect else res
        rec = out.download_normals().points
        out.close()
        four = np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], axis=1)
        return (four, res[1]) if rect else four

    def voxel_grid(self, leaf, downsample_all_data=True, min_points=0):
        """pcl::VoxelGrid::filter of this cloud (rsreg_cloud_voxel_grid): a new DeviceCloud with one centroid per occupied
        leaf, in leaf order.  leaf: one float or three."""
        f = VoxelGrid()
        f.setLeafSize(*np.broadcast_to(np.asarray(leaf, np.float32), (3,)))
        f.setDownsampleAllData(downsample_all_data)
        f.setMinimumPointsNumberPerVoxel(min_points)
        f.setInputCloud(self)
        return f.filter()

    @classmethod
    def from_depth(cls, ctx, depth, color, params, out=None):
        """The capture step in HBM (rsreg_cloud_from_depth; include/rsreg.h, "capture"): a DeviceCloud of PointXYZRGB records
        from a host depth image ((h, w) uint16) and a host colour image ((h, w, 3 or 4) uint8), rows may be padded -- the two
        images cross the link, not the records.  params: depth_params().  out: a DeviceCloud to rewrite instead of a new one."""
        ctx = ctx or default_context()
        dev = out if out is not None else cls(ctx=ctx)
        (keep_d, d_ptr, d_stride), (keep_c, c_ptr, c_stride) = _depth_image(depth), _color_image(color)
        rc = _l.lib().rsreg_cloud_from_depth(ctx.h, d_ptr, d_stride, c_ptr, c_stride, C.byref(params), dev.h)
        if rc and out is None:
            dev.close()
        _l.check(rc, ctx.h)
        return dev

    @classmethod
    def from_depth_device(cls, ctx, d_depth, depth_stride, d_color, color_stride, params, out=None):
        """from_depth with the two images already in HBM (rsreg_cloud_from_depth_device): device addresses (ints) and row
        strides in bytes; nothing crosses the link.  The context is synchronized before this returns, so the images may go."""
        ctx = ctx or default_context()
        dev = out if out is not None else cls(ctx=ctx)
        rc = _l.lib().rsreg_cloud_from_depth_device(ctx.h, int(d_depth), int(depth_stride), int(d_color), int(color_stride), C.byref(params), dev.h)
        if rc == 0:
            rc = _l.lib().rsreg_ctx_synchronize(ctx.h)
        if rc and out is None:
            dev.close()
        _l.check(rc, ctx.h)
        return dev

    def download_normals(self):
        """download() of a cloud of pcl::Normal records (what NormalEstimation.compute returns): a NormalCloud."""
        n, stride, w, h, dense = self.info()
        if n and stride != NORMAL_DTYPE.itemsize:
            raise ValueError("the device cloud does not hold 32-byte pcl::Normal records")
        rec = np.zeros(n, NORMAL_DTYPE)
        _l.check(_l.lib().rsreg_cloud_download(self.h, rec.ctypes.data, n), self.ctx.h)
        return NormalCloud(rec, w, h, dense)

    def copy(self):
        out = DeviceCloud(ctx=self.ctx)
        _l.check(_l.lib().rsreg_cloud_copy(self.ctx.h, self.h, out.h), self.ctx.h)
        return out

    def __add__(self, other):
        """PointCloud::operator+ in HBM: self's records followed by other's."""
        out = DeviceCloud(ctx=self.ctx)
        _l.check(_l.lib().rsreg_cloud_concat(self.ctx.h, self.h, other.h, out.h), self.ctx.h)
        return out

    def append(self, other):
        """PointCloud::operator+= in HBM (grows in place; the copy is of `other` only once there is room)."""
        _l.check(_l.lib().rsreg_cloud_concat(self.ctx.h, self.h, other.h, self.h), self.ctx.h)
        return self

    def prepend(self, other):
        """`*self = *other + *self` in HBM (icp_edge_based_registration.hpp:119: the new points go FIRST)."""
        _l.check(_l.lib().rsreg_cloud_concat(self.ctx.h, other.h, self.h, self.h), self.ctx.h)
        return self


def icp_params(reference=False, **kw):
    p = _l.IcpParams()
    (_l.lib().rsreg_icp_params_reference if reference else _l.lib().rsreg_icp_params_default)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def ndt_params(reference=False, **kw):
    p = _l.NdtParams()
    (_l.lib().rsreg_ndt_params_reference if reference else _l.lib().rsreg_ndt_params_default)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def iin_params(**kw):
    """rsreg_iin_params with PCL's defaults: AVERAGE_3D_GRADIENT, 0.02, 10.0, IGNORE, viewpoint (0, 0, 0)."""
    p = _l.IinParams()
    _l.lib().rsreg_iin_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "viewpoint":
            v = (C.c_float * 3)(*[float(x) for x in v])
        setattr(p, k, v)
    return p


def cluster_params(tolerance, min_size=1, max_size=2**31 - 1):
    """rsreg_cluster_params: PCL's defaults for the sizes (1, INT_MAX); the tolerance has none."""
    if not (0 <= int(min_size) < 2**32 and 0 <= int(max_size) < 2**32):
        raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "cluster sizes are counted in 32 bits")
    p = _l.ClusterParams()
    _l.lib().rsreg_cluster_params_default(C.byref(p))
    p.tolerance, p.min_cluster_size, p.max_cluster_size = float(tolerance), int(min_size), int(max_size)
    return p


def iss_params(**kw):
    """rsreg_iss_params with PCL's defaults: gamma_21 = gamma_32 = 0.975, min_neighbors 5; the two radii are 0 until set (refused)."""
    p = _l.IssParams()
    _l.lib().rsreg_iss_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "rsreg_iss_params has no field %r" % (k,))
        setattr(p, k, v)
    return p


def _depth_image(a):
    """(keepalive, pointer, row stride in bytes) of an (h, w) uint16 image; rows may be padded"""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype.kind not in "ui" or a.dtype.itemsize != 2:
        raise ValueError("the depth image must be an (h, w) uint16 array")
    if a.shape[0] > 1 and (a.strides[1] != 2 or a.strides[0] < 2 * a.shape[1]) or a.shape[0] <= 1 and not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    return a, a.ctypes.data, (a.strides[0] if a.shape[0] > 1 else 2 * a.shape[1])


def _color_image(a):
    """(keepalive, pointer, row stride in bytes) of an (h, w, 3 or 4) uint8 image; rows may be padded"""
    a = np.asarray(a)
    if a.ndim != 3 or a.dtype != np.uint8 or a.shape[2] not in (3, 4):
        raise ValueError("the colour image must be an (h, w, 3 or 4) uint8 array")
    bpp = a.shape[2]
    if a.shape[0] > 1 and (a.strides[2] != 1 or a.strides[1] != bpp or a.strides[0] < bpp * a.shape[1]) or a.shape[0] <= 1 and not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    return a, a.ctypes.data, (a.strides[0] if a.shape[0] > 1 else bpp * a.shape[1])


def _set_intrinsics(s, width, height, ppx, ppy, fx, fy, model=0, coeffs=(0, 0, 0, 0, 0)):
    s.width, s.height, s.ppx, s.ppy, s.fx, s.fy, s.model = int(width), int(height), float(ppx), float(ppy), float(fx), float(fy), int(model)
    for i in range(5):
        s.coeffs[i] = float(coeffs[i])


def depth_params(w, h, reference=False, depth=None, color=None, rotation=None, translation=None, **kw):
    """rsreg_depth_params for a w x h depth frame: the whole frame (convert_to_pcl_new), or with reference=True the reference's
    three-fifths centre crop (convert_to_pcl).  depth / color: dicts of width, height, ppx, ppy, fx, fy[, model, coeffs];
    rotation: 9 floats column-major, translation: 3; any other field of the struct by name."""
    p = _l.DepthParams()
    (_l.lib().rsreg_depth_params_reference if reference else _l.lib().rsreg_depth_params_default)(int(w), int(h), C.byref(p))
    if depth is not None:
        _set_intrinsics(p.depth, **depth)
    if color is not None:
        _set_intrinsics(p.color, **color)
    if rotation is not None:
        p.rotation = (C.c_float * 9)(*[float(v) for v in rotation])
    if translation is not None:
        p.translation = (C.c_float * 3)(*[float(v) for v in translation])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class DepthToCloud:
    """The capture step: rs2::pointcloud (map_to, calculate) + the reference's convert_to_pcl (src/capture.hpp:72-107; the whole
    frame: convert_to_pcl_new, src/capture_opencv.hpp:128-160) from a depth and a colour image (include/rsreg.h, "capture",
    states the contract).  With a context the cloud is built in HBM from the two images (rsreg_cloud_from_depth) and
    compute() returns a DeviceCloud; without one it runs the sequential host restatement (rsreg_depth_to_cloud) and returns a
    PointCloud: the same bytes from both."""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self._depth = self._color = None
        self._rotation, self._translation = (1, 0, 0, 0, 1, 0, 0, 0, 1), (0, 0, 0)
        self._scale, self._bpp, self._bgr, self._crop = 0.001, 3, True, False

    def setDepthIntrinsics(self, width, height, ppx, ppy, fx, fy, model=0, coeffs=(0, 0, 0, 0, 0)):
        self._depth = dict(width=width, height=height, ppx=ppx, ppy=ppy, fx=fx, fy=fy, model=model, coeffs=tuple(coeffs))

    def setColorIntrinsics(self, width, height, ppx, ppy, fx, fy, model=0, coeffs=(0, 0, 0, 0, 0)):
        self._color = dict(width=width, height=height, ppx=ppx, ppy=ppy, fx=fx, fy=fy, model=model, coeffs=tuple(coeffs))

    def setExtrinsics(self, rotation, translation):
        """depth -> colour (rs2_extrinsics): rotation 9 floats column-major, translation 3 (metres)"""
        self._rotation, self._translation = tuple(float(v) for v in rotation), tuple(float(v) for v in translation)

    def setDepthScale(self, scale):
        self._scale = float(scale)

    def setColorLayout(self, bytes_per_pixel=3, bgr=True):
        self._bpp, self._bgr = int(bytes_per_pixel), bool(bgr)

    def setReferenceCrop(self, on):
        """True: the reference's three-fifths centre crop with its shape and is_dense = 1 (convert_to_pcl); False: the frame"""
        self._crop = bool(on)

    def params(self, depth_shape, color_shape):
        """the rsreg_depth_params compute() uses for images of these shapes (an intrinsics that was not set: the placeholder)"""
        h, w = (self._depth["height"], self._depth["width"]) if self._depth else depth_shape[:2]
        color = self._color
        if color is None and tuple(color_shape[:2]) != (h, w):
            ch, cw = color_shape[:2]
            color = dict(width=cw, height=ch, ppx=cw / 2, ppy=ch / 2, fx=cw, fy=cw)
        return depth_params(w, h, reference=self._crop, depth=self._depth, color=color, rotation=self._rotation, translation=self._translation,
                            depth_scale=self._scale, color_bytes_per_pixel=self._bpp, color_bgr=int(self._bgr))

    def compute(self, depth, color, out=None):
        p = self.params(depth.shape, color.shape)
        if tuple(depth.shape[:2]) != (p.depth.height, p.depth.width) or tuple(color.shape) != (p.color.height, p.color.width, p.color_bytes_per_pixel):
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "the images do not have the shapes of the intrinsics and the colour layout")
        if self.ctx is not None:
            return DeviceCloud.from_depth(self.ctx, depth, color, p, out=out)
        (keep_d, d_ptr, d_stride), (keep_c, c_ptr, c_stride) = _depth_image(depth), _color_image(color)
        n = p.out_width * p.out_height
        pts = np.zeros(n, POINT_DTYPE)
        w, h, dense = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        _l.check(_l.lib().rsreg_depth_to_cloud(d_ptr, d_stride, c_ptr, c_stride, C.byref(p), pts.ctypes.data, n, C.byref(w), C.byref(h), C.byref(dense)))
        return PointCloud(pts, width=w.value, height=h.value, is_dense=bool(dense.value))


def _own_alignment(reg, owns):
    """getFitnessScore belongs to the last alignment of THIS object: the context's state may be another object's since."""
    if reg.result is None or not owns:
        raise _l.RsregError(_l.RSREG_ERR_STATE, "getFitnessScore before this object's align()")


class CorrespondenceRejector:
    """pcl::registration::CorrespondenceRejector as an entry of an ICP object's chain (include/rsreg.h: rsreg_icp_set_rejectors):
    a kind and a value.  The rejectors run inside the alignment, on the GPU; the objects only carry their settings."""
    kind = 0

    def __init__(self, value=0.0):
        self.value = float(value)
        self._stat = None   # (n_in, n_out, median d2) of the last search of the ICP object that holds it: rejector_stats()


class CorrespondenceRejectorMedianDistance(CorrespondenceRejector):
    kind = _l.REJECTOR_MEDIAN_DISTANCE

    def __init__(self, factor=1.0):
        super().__init__(factor)

    def setMedianFactor(self, factor):
        self.value = float(factor)

    def getMedianFactor(self):
        return self.value

    def getMedianDistance(self):
        """The median squared distance of the last search (after IterativeClosestPoint.rejector_stats())."""
        return self._stat[2] if self._stat else 0.0


class CorrespondenceRejectorOneToOne(CorrespondenceRejector):
    kind = _l.REJECTOR_ONE_TO_ONE


class CorrespondenceRejectorSurfaceNormal(CorrespondenceRejector):
    kind = _l.REJECTOR_SURFACE_NORMAL

    def __init__(self, threshold=1.0):
        super().__init__(threshold)

    def setThreshold(self, threshold):
        self.value = float(threshold)

    def getThreshold(self):
        return self.value


class CorrespondenceRejectorTrimmed(CorrespondenceRejector):
    kind = _l.REJECTOR_TRIMMED

    def __init__(self, overlap_ratio=0.5):
        super().__init__(overlap_ratio)

    def setOverlapRatio(self, ratio):
        self.value = float(ratio)

    def getOverlapRatio(self):
        return self.value


class IterativeClosestPoint:
    """pcl::IterativeClosestPoint<PointXYZRGB, PointXYZRGB> on the MI355X."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.params = icp_params()
        self.reuse_target_index = False   # engine extra, see _sync_inputs; PCL rebuilds its kd-tree at every setInputTarget
        self._src = self._tgt = None
        self._tgt_dirty = True
        self._src_dirty = True
        self._quiet_search = False   # run_sharded_icp: skip the per-iteration D2H of the correspondences
        self.result = None
        self._rejectors = []         # Registration::correspondence_rejectors_
        self._src_normals = None     # setInputSourceNormals: what a CorrespondenceRejectorSurfaceNormal compares
        self._src_normals_dirty = True
        self._normals = None         # setInputTargetNormals: the other side of that comparison (and point-to-plane ICP's planes)
        self._normals_dirty = True

    # Registration::addCorrespondenceRejector and its companions: the chain runs in this order in every iteration, behind
    # setUseReciprocalCorrespondences / setTrimmedRejectorOverlapRatio (include/rsreg.h: rsreg_icp_set_rejectors)
    def addCorrespondenceRejector(self, rejector):
        if not isinstance(rejector, CorrespondenceRejector) or rejector.kind == 0:
            raise ValueError("addCorrespondenceRejector takes a CorrespondenceRejectorMedianDistance, ...OneToOne, ...SurfaceNormal or ...Trimmed")
        if len(self._rejectors) >= _l.MAX_REJECTORS:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "a rejector chain has at most %d entries" % _l.MAX_REJECTORS)
        self._rejectors.append(rejector)

    def getCorrespondenceRejectors(self):
        return list(self._rejectors)

    def removeCorrespondenceRejector(self, i):
        if not 0 <= i < len(self._rejectors):
            return False
        del self._rejectors[i]
        return True

    def clearCorrespondenceRejectors(self):
        self._rejectors = []

    def setInputSourceNormals(self, normals):
        """The source's normals, one per record (a NormalCloud / NORMAL_DTYPE array, an (n, >= 3) float32 array or a DeviceCloud
        of pcl::Normal records); a POINT_NORMAL_DTYPE source carries its own.  Read by CorrespondenceRejectorSurfaceNormal."""
        self._src_normals = normals
        self._src_normals_dirty = True

    def setInputTargetNormals(self, normals):
        """The target's normals, one per record, in the forms setInputSourceNormals takes; a POINT_NORMAL_DTYPE target carries its own."""
        self._normals = normals
        self._normals_dirty = True

    def _needs_target_normals(self):
        return any(r.kind == _l.REJECTOR_SURFACE_NORMAL for r in self._rejectors)

    def _sync_target_normals(self, rebuilt):
        if not (rebuilt or self._normals_dirty):   # (a new target index drops the normals of the one before)
            return
        L, h = _l.lib(), self.ctx.h
        nrm = self._normals
        if nrm is None:
            pts = getattr(self._tgt, "points", self._tgt)
            if not (isinstance(pts, np.ndarray) and pts.dtype.names and "normal_x" in pts.dtype.names):
                raise _l.RsregError(_l.RSREG_ERR_STATE, "%s: the target has no normals (setInputTargetNormals)" % type(self).__name__)
            pts = np.ascontiguousarray(pts)
            _l.check(L.rsreg_icp_set_target_normals(h, pts.ctypes.data + pts.dtype.fields["normal_x"][1], len(pts), pts.dtype.itemsize), h)
        elif isinstance(nrm, DeviceCloud):
            _l.check(L.rsreg_icp_set_target_normals_cloud(h, nrm.h), h)
            self._nrm_stamp = nrm.stamp
        else:
            rec = np.ascontiguousarray(getattr(nrm, "points", nrm))
            if rec.dtype.names:
                off = rec.dtype.fields["normal_x"][1]
                _l.check(L.rsreg_icp_set_target_normals(h, rec.ctypes.data + off, len(rec), rec.dtype.itemsize), h)
            else:
                if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] < 3:
                    raise ValueError("normals must be a NormalCloud, a structured array with normal_x or an (n, >=3) float32 array")
                _l.check(L.rsreg_icp_set_target_normals(h, rec.ctypes.data, rec.shape[0], rec.shape[1] * 4), h)
        self._normals_dirty = False

    def _sync_rejectors(self, source_loaded):
        """The object's chain onto the context (another object's may be there), and the source's normals if the chain reads them."""
        L, h = _l.lib(), self.ctx.h
        n = len(self._rejectors)
        arr = (_l.Rejector * max(n, 1))()
        for k, r in enumerate(self._rejectors):
            arr[k].kind, arr[k].value = r.kind, r.value
        _l.check(L.rsreg_icp_set_rejectors(h, C.cast(arr, C.c_void_p) if n else None, n), h)
        if not any(r.kind == _l.REJECTOR_SURFACE_NORMAL for r in self._rejectors):
            return
        nrm = self._src_normals
        if isinstance(nrm, DeviceCloud) and getattr(self, "_src_nrm_stamp", None) != nrm.stamp:
            self._src_normals_dirty = True
        if not (source_loaded or self._src_normals_dirty):
            return
        if nrm is None:
            pts = getattr(self._src, "points", self._src)
            if not (isinstance(pts, np.ndarray) and pts.dtype.names and "normal_x" in pts.dtype.names):
                raise _l.RsregError(_l.RSREG_ERR_STATE, "CorrespondenceRejectorSurfaceNormal: the source has no normals (setInputSourceNormals)")
            pts = np.ascontiguousarray(pts)
            _l.check(L.rsreg_icp_set_source_normals(h, pts.ctypes.data + pts.dtype.fields["normal_x"][1], len(pts), pts.dtype.itemsize), h)
        elif isinstance(nrm, DeviceCloud):
            _l.check(L.rsreg_icp_set_source_normals_cloud(h, nrm.h), h)
            self._src_nrm_stamp = nrm.stamp
        else:
            rec = np.ascontiguousarray(getattr(nrm, "points", nrm))
            if rec.dtype.names:
                _l.check(L.rsreg_icp_set_source_normals(h, rec.ctypes.data + rec.dtype.fields["normal_x"][1], len(rec), rec.dtype.itemsize), h)
            else:
                if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] < 3:
                    raise ValueError("normals must be a NormalCloud, a structured array with normal_x or an (n, >=3) float32 array")
                _l.check(L.rsreg_icp_set_source_normals(h, rec.ctypes.data, rec.shape[0], rec.shape[1] * 4), h)
        self._src_normals_dirty = False

    def rejector_stats(self):
        """[(n_in, n_out, median d2)] per rejector of the chain for the last search (rsreg_icp_rejector_stats); also left on the
        rejector objects (getMedianDistance)."""
        n = len(self._rejectors)
        st = (_l.RejectorStat * max(n, 1))()
        got = C.c_int32(0)
        _l.check(_l.lib().rsreg_icp_rejector_stats(self.ctx.h, C.cast(st, C.c_void_p), n, C.byref(got)), self.ctx.h)
        out = [(int(st[k].n_in), int(st[k].n_out), float(st[k].median_distance)) for k in range(min(n, got.value))]
        for r, s in zip(self._rejectors, out):
            r._stat = s
        return out

    # setters the reference calls (incremental_icp.hpp:46-49)
    def setMaximumIterations(self, n):
        self.params.max_iterations = int(n)

    def setMaxCorrespondenceDistance(self, d):
        if d != self.params.max_correspondence_distance:
            self._tgt_dirty = True  # the grid cell size derives from the gate
        self.params.max_correspondence_distance = float(d)

    def setTransformationEpsilon(self, e):
        self.params.transformation_epsilon = float(e)

    def setTransformationRotationEpsilon(self, e):
        self.params.transformation_rotation_epsilon = float(e)

    def setEuclideanFitnessEpsilon(self, e):
        self.params.euclidean_fitness_epsilon = float(e)

    # optional correspondence filters of pcl::IterativeClosestPoint (off by default and in the reference)
    def setUseReciprocalCorrespondences(self, on):
        self.params.use_reciprocal_correspondences = int(bool(on))

    def setTrimmedRejectorOverlapRatio(self, ratio):
        """addCorrespondenceRejector(CorrespondenceRejectorTrimmed with setOverlapRatio(ratio)); <= 0 or >= 1: none."""
        self.params.trim_overlap_ratio = float(ratio)

    # engine knobs (not in PCL)
    def setCriteriaMode(self, mode):
        self.params.criteria_mode = int(mode)

    def setPipelineMode(self, mode):
        self.params.pipeline_mode = int(mode)

    def setInputSource(self, cloud):
        self._src = cloud
        self._src_dirty = True

    def setInputTarget(self, cloud):
        self._tgt = cloud
        self._tgt_dirty = True  # PCL rebuilds the kd-tree whenever the target is set

    # clouds already resident in HBM (e.g. torch tensors): (device pointer, count, stride)
    def setInputSourceDevice(self, ptr, n, stride):
        self._src = ("device", int(ptr), int(n), int(stride))
        self._src_dirty = True

    def setInputTargetDevice(self, ptr, n, stride):
        self._tgt = ("device", int(ptr), int(n), int(stride))
        self._tgt_dirty = True

    def _sync_inputs(self):
        L, h = _l.lib(), self.ctx.h
        if self._tgt is None or self._src is None:
            raise ValueError("setInputSource / setInputTarget not called")
        rebuilt = self._tgt_dirty or self.ctx.icp_target_owner is not self or getattr(self, "_tgt_gate", None) != self.params.max_correspondence_distance
        if isinstance(self._tgt, DeviceCloud) and getattr(self, "_tgt_stamp", None) != self._tgt.stamp:
            rebuilt = True
        if isinstance(self._normals, DeviceCloud) and getattr(self, "_nrm_stamp", None) != self._normals.stamp:
            self._normals_dirty = True
        # the source first, as the reference does (incremental_icp.hpp:57-58): the library loads it on a stream of its own,
        # beside the target's index build
        # a device cloud rewritten in place since it was loaded (filter(x, x), +=, a transform or an alignment into it) is
        # loaded again, as PCL would see the new points through its pointer
        if isinstance(self._src, DeviceCloud) and getattr(self, "_src_stamp", None) != self._src.stamp:
            self._src_dirty = True
        if isinstance(self._tgt, DeviceCloud) and getattr(self, "_tgt_stamp", None) != self._tgt.stamp:
            self._tgt_dirty = True
        if self._src_dirty or self.ctx.icp_source_owner is not self:
            if isinstance(self._src, DeviceCloud):
                _l.check(L.rsreg_icp_set_source_cloud(h, self._src.h), h)
                n = len(self._src)
                self._src_stamp = self._src.stamp
            elif isinstance(self._src, tuple):
                _, p, n, s = self._src
                _l.check(L.rsreg_icp_set_source_device(h, p, n, s, 0), h)
            else:
                keep, p, n, s = _records(self._src)
                dense = int(getattr(self._src, "is_dense", False))
                _l.check(L.rsreg_icp_set_source(h, p, n, s, dense), h)
            self._n_src = n
            self._src_dirty = False
            self.ctx.icp_source_owner = self
            self._src_loaded = True   # (the library dropped the source normals of the load before: _sync_rejectors)
        # the index's cell size derives from the gate: a gate that has changed since the build -- through the setter or by assigning
        # `params` -- means a new index (PCL lets the caller change it between two aligns of the same target)
        if getattr(self, "_tgt_gate", None) != self.params.max_correspondence_distance:
            self._tgt_dirty = True
        if self._tgt_dirty or self.ctx.icp_target_owner is not self:
            self._tgt_gate = self.params.max_correspondence_distance
            if isinstance(self._tgt, DeviceCloud):
                # (reuse_target_index: another ICP object of this context has just built the index of this very cloud)
                if not (self.reuse_target_index and L.rsreg_icp_target_is_cloud(h, self._tgt.h, self.params.max_correspondence_distance)):
                    _l.check(L.rsreg_icp_set_target_cloud(h, self._tgt.h, self.params.max_correspondence_distance), h)
                self._tgt_stamp = self._tgt.stamp
            elif isinstance(self._tgt, tuple):
                _, p, n, s = self._tgt
                _l.check(L.rsreg_icp_set_target_device(h, p, n, s, 0, self.params.max_correspondence_distance), h)
            else:
                keep, p, n, s = _records(self._tgt)
                dense = int(getattr(self._tgt, "is_dense", False))
                _l.check(L.rsreg_icp_set_target(h, p, n, s, dense, self.params.max_correspondence_distance), h)
            self._tgt_dirty = False
            self.ctx.icp_target_owner = self
        if self._needs_target_normals():
            self._sync_target_normals(rebuilt)
        loaded, self._src_loaded = getattr(self, "_src_loaded", False), False
        self._sync_rejectors(loaded)

    def align(self, guess=None):
        """icp.align(out[, guess]): returns the aligned cloud (source colours, xyz <- final * xyz)."""
        self._sync_inputs()
        g = _colmajor(guess)
        res = _l.IcpResult()
        if isinstance(self._src, DeviceCloud):   # the aligned cloud stays in HBM too
            out = DeviceCloud(ctx=self.ctx)
            _l.check(_l.lib().rsreg_icp_align_cloud(self.ctx.h, g.ctypes.data if g is not None else None, C.byref(self.params),
                                                    C.byref(res), out.h), self.ctx.h)
            self.result = res
            return out
        if isinstance(self._src, PointCloud) and len(self._src.points):
            # `output = input` is made inside the call (rsreg_icp_align_records), by the host threads that write the aligned positions
            recs = np.ascontiguousarray(self._src.points)
            out = np.empty(len(recs), recs.dtype)
            _l.check(_l.lib().rsreg_icp_align_records(self.ctx.h, g.ctypes.data if g is not None else None, C.byref(self.params),
                                                      C.byref(res), recs.ctypes.data, out.ctypes.data, out.dtype.itemsize), self.ctx.h)
        else:
            out = self._src.points.copy() if isinstance(self._src, PointCloud) else np.zeros(self._n_src, POINT_DTYPE)
            _l.check(_l.lib().rsreg_icp_align(self.ctx.h, g.ctypes.data if g is not None else None, C.byref(self.params),
                                              C.byref(res), out.ctypes.data, out.dtype.itemsize), self.ctx.h)
        self.result = res
        src = self._src if isinstance(self._src, PointCloud) else None
        return PointCloud(out, width=src.width if src else len(out), height=src.height if src else 1,
                          is_dense=src.is_dense if src else False)

    def hasConverged(self):
        return bool(self.result.converged)

    def getFinalTransformation(self):
        return _rowmajor(self.result.transform)

    def getConvergenceState(self):
        return CONV_STATES[self.result.state]

    # ---- step-wise form (parity tests, sharded runs)
    def begin(self, guess=None):
        self._sync_inputs()
        g = _colmajor(guess)
        _l.check(_l.lib().rsreg_icp_begin(self.ctx.h, g.ctypes.data if g is not None else None, C.byref(self.params)),
                 self.ctx.h)

    def search(self, want_output=True):
        if not want_output:
            _l.check(_l.lib().rsreg_icp_search(self.ctx.h, None, None), self.ctx.h)
            return None
        idx = np.empty(self._n_src, np.int32)
        d2 = np.empty(self._n_src, np.float32)
        _l.check(_l.lib().rsreg_icp_search(self.ctx.h, idx.ctypes.data, d2.ctypes.data), self.ctx.h)
        return idx, d2

    def sums(self):
        s = np.zeros(_l.NUM_SUMS, np.float64)
        _l.check(_l.lib().rsreg_icp_sums(self.ctx.h, s.ctypes.data), self.ctx.h)
        return s

    def update(self, sums):
        sums = np.ascontiguousarray(sums, np.float64)
        t = np.zeros(16, np.float32)
        done = C.c_int(0)
        _l.check(_l.lib().rsreg_icp_update(self.ctx.h, sums.ctypes.data, t.ctypes.data, C.byref(done)), self.ctx.h)
        return _rowmajor(t), bool(done.value)

    def end(self, want_aligned=False):
        res = _l.IcpResult()
        out = np.zeros((self._n_src, 4), np.float32) if want_aligned else None
        _l.check(_l.lib().rsreg_icp_end(self.ctx.h, C.byref(res), out.ctypes.data if want_aligned else None, 16),
                 self.ctx.h)
        self.result = res
        return (res, out) if want_aligned else res

    def getFitnessScore(self, max_range=sys.float_info.max):
        """Registration::getFitnessScore(max_range) of the last alignment: the mean squared distance from every finite source
        record at the final pose to its nearest target point, over the records whose SQUARED distance is <= max_range (PCL's
        quirk: the range is compared with d^2); sys.float_info.max when none is (rsreg_icp_fitness_score).  With a communicator
        of more than one rank the mean is over all ranks' records."""
        return self.fitnessScore(max_range)[0]

    def fitnessScore(self, max_range=sys.float_info.max):
        """(score, records in range) -- getFitnessScore with the count."""
        _own_alignment(self, self.ctx.icp_source_owner is self and self.ctx.icp_target_owner is self and not self._src_dirty and not self._tgt_dirty)
        score, nr = C.c_double(0), C.c_uint64(0)
        _l.check(_l.lib().rsreg_icp_fitness_score(self.ctx.h, float(max_range), C.byref(score), C.byref(nr)), self.ctx.h)
        return score.value, nr.value

    def fitness_sums(self, max_range=sys.float_info.max):
        """This rank's (count, sum of d^2) of getFitnessScore, never all-reduced (rsreg_icp_fitness_sums): sharded.py adds them up."""
        _own_alignment(self, self.ctx.icp_source_owner is self and self.ctx.icp_target_owner is self and not self._src_dirty and not self._tgt_dirty)
        s = np.zeros(2, np.float64)
        _l.check(_l.lib().rsreg_icp_fitness_sums(self.ctx.h, float(max_range), s.ctypes.data), self.ctx.h)
        return s

    def grid_info(self):
        gi = _l.GridInfo()
        _l.check(_l.lib().rsreg_icp_grid_info(self.ctx.h, C.byref(gi)), self.ctx.h)
        return gi


# pcl::PointXYZRGBNormal: 48 bytes -- data[4], data_n[4], then rgb, curvature and two words of padding
POINT_NORMAL_DTYPE = np.dtype({"names": ["x", "y", "z", "w", "normal_x", "normal_y", "normal_z", "data_n3", "rgba", "curvature", "pad0", "pad1"],
                               "formats": ["<f4"] * 8 + ["<u4", "<f4", "<u4", "<u4"], "offsets": list(range(0, 48, 4)), "itemsize": 48})


class IterativeClosestPointWithNormals(IterativeClosestPoint):
    """pcl::IterativeClosestPointWithNormals on the MI355X: point-to-plane ICP with PCL's default estimator,
    TransformationEstimationPointToPlaneLLS (include/rsreg.h: rsreg_estimation, RSREG_NUM_PLANE_SUMS).  The target's normals
    come with the target -- setInputTarget(cloud, normals) or setInputTargetNormals(normals), a NormalCloud / NORMAL_DTYPE
    array, an (n, >= 3) float32 array or a DeviceCloud of pcl::Normal records (NormalEstimation.compute of a DeviceCloud) --
    or inside it: a POINT_NORMAL_DTYPE array as the target hands over xyz at stride 48 and the normals at byte 16.  The
    aligned cloud's own normals, if its records carry any, are copied, not rotated."""

    def __init__(self, ctx=None):
        super().__init__(ctx)
        self.params.estimation = _l.ESTIMATION_POINT_TO_PLANE_LLS

    def setInputTarget(self, cloud, normals=None):
        super().setInputTarget(cloud)
        self._normals = normals
        self._normals_dirty = True

    def _needs_target_normals(self):
        return True

    # ---- step-wise form: begin -> { search -> plane_sums -> update_plane } -> end
    def plane_sums(self):
        s = np.zeros(_l.NUM_PLANE_SUMS, np.float64)
        _l.check(_l.lib().rsreg_icp_plane_sums(self.ctx.h, s.ctypes.data), self.ctx.h)
        return s

    def update_plane(self, sums):
        sums = np.ascontiguousarray(sums, np.float64)
        if sums.size != _l.NUM_PLANE_SUMS:
            raise ValueError("update_plane takes the 32 plane sums")
        t = np.zeros(16, np.float32)
        done = C.c_int(0)
        _l.check(_l.lib().rsreg_icp_update_plane(self.ctx.h, sums.ctypes.data, t.ctypes.data, C.byref(done)), self.ctx.h)
        return _rowmajor(t), bool(done.value)

    def plane_sums_last(self):
        s = np.zeros(_l.NUM_PLANE_SUMS, np.float64)
        _l.check(_l.lib().rsreg_icp_plane_sums_last(self.ctx.h, s.ctypes.data), self.ctx.h)
        return s


def gicp_params(**kw):
    p = _l.GicpParams()
    _l.lib().rsreg_gicp_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _colmajor64(X):
    return None if X is None else np.ascontiguousarray(np.asarray(X, np.float64).reshape(4, 4).T).copy()


def gicp_step_from_sums(sums, scale=1.0):
    """(x (6,), Delta(x) 4x4 float64, rank): x = scale * pinv(H) b of the 32 GICP sums (rsreg_gicp_step_from_sums, host only)."""
    sums = np.ascontiguousarray(sums, np.float64)
    if sums.size != _l.NUM_GICP_SUMS:
        raise ValueError("gicp_step_from_sums takes the 32 GICP sums")
    x, d, rank = np.zeros(6), np.zeros(16), C.c_int(0)
    _l.check(_l.lib().rsreg_gicp_step_from_sums(sums.ctypes.data, float(scale), x.ctypes.data, d.ctypes.data, C.byref(rank)))
    return x, d.reshape(4, 4).T.copy(), rank.value


class GeneralizedIterativeClosestPoint(IterativeClosestPoint):
    """pcl::GeneralizedIterativeClosestPoint on the MI355X (plane-to-plane ICP; include/rsreg.h: the rsreg_gicp_* section holds the
    contract and the stated deviations from PCL).  Covariances: setSourceCovariances / setTargetCovariances take an (n, 6) float64
    array (xx, xy, xz, yy, yz, zz per record) or a DeviceCloud of such records (DeviceCloud.gicp_covariances_cloud); a cloud without
    them gets its own from rsreg_cloud_gicp_covariances with setCorrespondenceRandomness' k, as PCL computes them."""

    def __init__(self, ctx=None):
        super().__init__(ctx)
        self.gparams = gicp_params()
        self.params.max_correspondence_distance = self.gparams.max_correspondence_distance   # (the target index's gate)
        self._cov = {"source": None, "target": None}
        self._cov_dirty = {"source": True, "target": True}

    def setCorrespondenceRandomness(self, k):
        self.gparams.k_correspondences = int(k)
        self._cov_dirty = {"source": True, "target": True}

    def setRotationEpsilon(self, e):
        self.gparams.rotation_epsilon = float(e)

    def setTransformationEpsilon(self, e):
        self.gparams.transformation_epsilon = float(e)

    def setMaximumOptimizerIterations(self, n):
        self.gparams.max_inner_iterations = int(n)

    def setMaximumIterations(self, n):
        self.gparams.max_iterations = int(n)

    def setMaxCorrespondenceDistance(self, d):
        super().setMaxCorrespondenceDistance(d)
        self.gparams.max_correspondence_distance = float(d)

    def setInputSource(self, cloud):
        super().setInputSource(cloud)
        self._cov["source"], self._cov_dirty["source"] = None, True

    def setInputTarget(self, cloud):
        super().setInputTarget(cloud)
        self._cov["target"], self._cov_dirty["target"] = None, True

    def setSourceCovariances(self, cov):
        self._cov["source"], self._cov_dirty["source"] = cov, True

    def setTargetCovariances(self, cov):
        self._cov["target"], self._cov_dirty["target"] = cov, True

    def _set_covariances(self, which, cloud):
        L, h = _l.lib(), self.ctx.h
        cov = self._cov[which]
        set_host = getattr(L, "rsreg_gicp_set_%s_covariances" % which)
        set_cloud = getattr(L, "rsreg_gicp_set_%s_covariances_cloud" % which)
        if cov is None:   # PCL: computeCovariances of the cloud itself
            dev, made = (cloud, False) if isinstance(cloud, DeviceCloud) else (DeviceCloud(cloud, ctx=self.ctx), True)
            out = dev.gicp_covariances_cloud(self.gparams.k_correspondences, self.gparams.gicp_epsilon)
            rc = set_cloud(h, out.h)
            out.close()
            if made:
                dev.close()
            _l.check(rc, h)
        elif isinstance(cov, DeviceCloud):
            _l.check(set_cloud(h, cov.h), h)
        else:
            a = np.ascontiguousarray(cov, np.float64)
            if a.ndim != 2 or a.shape[1] < 6:
                raise ValueError("covariances must be a DeviceCloud or an (n, >= 6) float64 array")
            _l.check(set_host(h, a.ctypes.data, a.shape[0], a.shape[1] * 8), h)
        self._cov_dirty[which] = False

    def _sync_inputs(self):
        self.params.max_correspondence_distance = self.gparams.max_correspondence_distance
        src_new = self._src_dirty or self.ctx.icp_source_owner is not self
        tgt_new = self._tgt_dirty or self.ctx.icp_target_owner is not self or getattr(self, "_tgt_gate", None) != self.params.max_correspondence_distance
        if isinstance(self._src, DeviceCloud) and getattr(self, "_src_stamp", None) != self._src.stamp:
            src_new = True
        if isinstance(self._tgt, DeviceCloud) and getattr(self, "_tgt_stamp", None) != self._tgt.stamp:
            tgt_new = True
        super()._sync_inputs()
        # (a new source or target drops the covariances of the one before)
        if src_new or self._cov_dirty["source"]:
            self._set_covariances("source", self._src)
        if tgt_new or self._cov_dirty["target"]:
            self._set_covariances("target", self._tgt)

    def align(self, guess=None):
        """gicp.align(out[, guess]): the aligned cloud, as IterativeClosestPoint.align returns it."""
        self._sync_inputs()
        g = _colmajor(guess)
        gp = g.ctypes.data if g is not None else None
        res = _l.GicpResult()
        if isinstance(self._src, DeviceCloud):
            out = DeviceCloud(ctx=self.ctx)
            _l.check(_l.lib().rsreg_gicp_align_cloud(self.ctx.h, gp, C.byref(self.gparams), C.byref(res), out.h), self.ctx.h)
            self.result = res
            return out
        out = self._src.points.copy() if isinstance(self._src, PointCloud) else np.zeros(self._n_src, POINT_DTYPE)
        _l.check(_l.lib().rsreg_gicp_align(self.ctx.h, gp, C.byref(self.gparams), C.byref(res), out.ctypes.data if len(out) else None,
                                           out.dtype.itemsize), self.ctx.h)
        self.result = res
        src = self._src if isinstance(self._src, PointCloud) else None
        return PointCloud(out, width=src.width if src else len(out), height=src.height if src else 1, is_dense=src.is_dense if src else False)

    # ---- step-wise form: begin -> { search -> gicp_sums(X) ... -> update(X, sums, evaluations) } -> end
    def begin(self, guess=None):
        self._sync_inputs()
        g = _colmajor(guess)
        _l.check(_l.lib().rsreg_gicp_begin(self.ctx.h, g.ctypes.data if g is not None else None, C.byref(self.gparams)), self.ctx.h)

    def search(self, want_output=True):
        idx = np.empty(self._n_src, np.int32) if want_output else None
        d2 = np.empty(self._n_src, np.float32) if want_output else None
        _l.check(_l.lib().rsreg_gicp_search(self.ctx.h, idx.ctypes.data if want_output else None, d2.ctypes.data if want_output else None), self.ctx.h)
        return (idx, d2) if want_output else None

    def gicp_sums(self, X=None):
        """The 32 sums (RSREG_NUM_GICP_SUMS) of the last search at the increment X (4x4 float64, None: the identity)."""
        s = np.zeros(_l.NUM_GICP_SUMS, np.float64)
        Xc = _colmajor64(X)
        _l.check(_l.lib().rsreg_gicp_sums(self.ctx.h, Xc.ctypes.data if Xc is not None else None, s.ctypes.data), self.ctx.h)
        return s

    def sums(self):
        raise _l.RsregError(_l.RSREG_ERR_STATE, "GICP alignment: gicp_sums(X)")

    def update(self, X, sums, inner_evaluations=0):
        """Compose T = float(X T) and test PCL's criterion: True when the loop must stop."""
        sums = np.ascontiguousarray(sums, np.float64)
        if sums.size != _l.NUM_GICP_SUMS:
            raise ValueError("update takes the 32 GICP sums")
        Xc = _colmajor64(X)
        done = C.c_int(0)
        _l.check(_l.lib().rsreg_gicp_update(self.ctx.h, Xc.ctypes.data if Xc is not None else None, sums.ctypes.data, int(inner_evaluations),
                                            C.byref(done)), self.ctx.h)
        return bool(done.value)

    def end(self, want_aligned=False):
        res = _l.GicpResult()
        out = np.zeros((self._n_src, 4), np.float32) if want_aligned else None
        _l.check(_l.lib().rsreg_gicp_end(self.ctx.h, C.byref(res), out.ctypes.data if want_aligned else None, 16), self.ctx.h)
        self.result = res
        return (res, out) if want_aligned else res


def lab_tables():
    """(S (256,), F (4000,)) float32: the sRGB -> linear and CIE f() tables the library converts colours with (rsreg_lab_tables)."""
    S, F = np.zeros(256, np.float32), np.zeros(4000, np.float32)
    _l.check(_l.lib().rsreg_lab_tables(S.ctypes.data, F.ctypes.data))
    return S, F


def rgb_to_lab(rgba):
    """(n, 3) float32 L', a', b' of n packed rgb words (rsreg_rgb_to_lab, host only)."""
    w = np.ascontiguousarray(rgba, np.uint32).reshape(-1)
    out = np.zeros((len(w), 3), np.float32)
    _l.check(_l.lib().rsreg_rgb_to_lab(w.ctypes.data, len(w), out.ctypes.data))
    return out


class GeneralizedIterativeClosestPoint6D(GeneralizedIterativeClosestPoint):
    """pcl::GeneralizedIterativeClosestPoint6D on the MI355X: GICP whose correspondences are nearest neighbours in
    (x, y, z, w L', w a', w b') (include/rsreg.h: the GICP6D section).  The colours come from the clouds themselves
    (rsreg_cloud_lab) unless setSourceLab / setTargetLab hand them in: an (n, >= 3) float32 array or a DeviceCloud of such records."""

    def __init__(self, ctx=None, lab_weight=0.032):
        super().__init__(ctx)
        self.lab_weight = float(lab_weight)
        self._lab = {"source": None, "target": None}
        self._lab_dirty = {"source": True, "target": True}

    def setInputSource(self, cloud):
        super().setInputSource(cloud)
        self._lab["source"], self._lab_dirty["source"] = None, True

    def setInputTarget(self, cloud):
        super().setInputTarget(cloud)
        self._lab["target"], self._lab_dirty["target"] = None, True

    def setSourceLab(self, lab):
        self._lab["source"], self._lab_dirty["source"] = lab, True

    def setTargetLab(self, lab):
        self._lab["target"], self._lab_dirty["target"] = lab, True

    def _set_lab(self, which, cloud):
        L, h = _l.lib(), self.ctx.h
        lab = self._lab[which]
        set_host = getattr(L, "rsreg_gicp_set_%s_lab" % which)
        set_cloud = getattr(L, "rsreg_gicp_set_%s_lab_cloud" % which)
        if lab is None:   # the colours of the cloud itself
            if isinstance(cloud, tuple):
                raise ValueError("a cloud given by its device pointer needs setSourceLab / setTargetLab")
            dev, made = (cloud, False) if isinstance(cloud, DeviceCloud) else (DeviceCloud(cloud, ctx=self.ctx), True)
            out = dev.lab_cloud()
            rc = set_cloud(h, out.h)
            out.close()
            if made:
                dev.close()
            _l.check(rc, h)
        elif isinstance(lab, DeviceCloud):
            _l.check(set_cloud(h, lab.h), h)
        else:
            a = np.ascontiguousarray(lab, np.float32)
            if a.ndim != 2 or a.shape[1] < 3:
                raise ValueError("colours must be a DeviceCloud or an (n, >= 3) float32 array")
            _l.check(set_host(h, a.ctypes.data, a.shape[0], a.shape[1] * 4), h)
        self._lab_dirty[which] = False

    def _sync_inputs(self):
        src_new = self._src_dirty or self.ctx.icp_source_owner is not self
        tgt_new = self._tgt_dirty or self.ctx.icp_target_owner is not self or getattr(self, "_tgt_gate", None) != self.gparams.max_correspondence_distance
        if isinstance(self._src, DeviceCloud) and getattr(self, "_src_stamp", None) != self._src.stamp:
            src_new = True
        if isinstance(self._tgt, DeviceCloud) and getattr(self, "_tgt_stamp", None) != self._tgt.stamp:
            tgt_new = True
        super()._sync_inputs()
        # (a new source or target drops the colours of the one before)
        if src_new or self._lab_dirty["source"]:
            self._set_lab("source", self._src)
        if tgt_new or self._lab_dirty["target"]:
            self._set_lab("target", self._tgt)

    def align(self, guess=None):
        """gicp6d.align(out[, guess]): the aligned cloud, as IterativeClosestPoint.align returns it."""
        self._sync_inputs()
        g = _colmajor(guess)
        gp = g.ctypes.data if g is not None else None
        res = _l.GicpResult()
        if isinstance(self._src, DeviceCloud):
            out = DeviceCloud(ctx=self.ctx)
            _l.check(_l.lib().rsreg_gicp6d_align_cloud(self.ctx.h, gp, C.byref(self.gparams), self.lab_weight, C.byref(res), out.h), self.ctx.h)
            self.result = res
            return out
        out = self._src.points.copy() if isinstance(self._src, PointCloud) else np.zeros(self._n_src, POINT_DTYPE)
        _l.check(_l.lib().rsreg_gicp6d_align(self.ctx.h, gp, C.byref(self.gparams), self.lab_weight, C.byref(res), out.ctypes.data if len(out) else None,
                                             out.dtype.itemsize), self.ctx.h)
        self.result = res
        src = self._src if isinstance(self._src, PointCloud) else None
        return PointCloud(out, width=src.width if src else len(out), height=src.height if src else 1, is_dense=src.is_dense if src else False)

    def begin(self, guess=None):
        self._sync_inputs()
        g = _colmajor(guess)
        _l.check(_l.lib().rsreg_gicp6d_begin(self.ctx.h, g.ctypes.data if g is not None else None, C.byref(self.gparams), self.lab_weight), self.ctx.h)


class NormalDistributionsTransform:
    """pcl::NormalDistributionsTransform<PointXYZRGB, PointXYZRGB> on the MI355X."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.params = ndt_params()
        self._src = self._tgt = None
        self._tgt_dirty = True
        self.result = None
        self._pcl_centroids = False
        self._fit_fresh = False   # the last align() is of the current source and target (getFitnessScore)

    def setPclCentroids(self, on):
        """Engine extra: search the voxels by PCL's own centroid arithmetic (a float running sum per voxel in input order,
        rsreg_ndt_set_centroid_mode) instead of the rounded f64 mean."""
        if bool(on) != self._pcl_centroids:
            self._tgt_dirty = True
        self._pcl_centroids = bool(on)

    def centroids(self):
        n = C.c_int32(0)
        _l.check(_l.lib().rsreg_ndt_get_voxels(self.ctx.h, C.byref(n), None, None, 0), self.ctx.h)
        out = np.zeros((n.value, 3), np.float32)
        _l.check(_l.lib().rsreg_ndt_get_centroids(self.ctx.h, out.ctypes.data, n.value), self.ctx.h)
        return out

    def setTransformationEpsilon(self, e):
        self.params.transformation_epsilon = float(e)

    def setStepSize(self, s):
        self.params.step_size = float(s)

    def setResolution(self, r):
        if r != self.params.resolution:
            self._tgt_dirty = True
        self.params.resolution = float(r)

    def setMaximumIterations(self, n):
        self.params.max_iterations = int(n)

    def setInputSource(self, cloud):
        self._src = cloud
        self._fit_fresh = False

    def setInputTarget(self, cloud):
        self._tgt = cloud
        self._tgt_dirty = True
        self._fit_fresh = False

    def _sync_target(self):
        if self._tgt is None or self._src is None:
            raise ValueError("setInputSource / setInputTarget not called")
        if isinstance(self._tgt, DeviceCloud) and getattr(self, "_tgt_stamp", None) != self._tgt.stamp:
            self._tgt_dirty = True   # (rewritten in place since the voxel grid was built)
        if self._tgt_dirty or self.ctx.ndt_target_owner is not self:
            _l.check(_l.lib().rsreg_ndt_set_centroid_mode(self.ctx.h, 1 if self._pcl_centroids else 0), self.ctx.h)
            if isinstance(self._tgt, DeviceCloud):
                _l.check(_l.lib().rsreg_ndt_set_target_cloud(self.ctx.h, self._tgt.h, self.params.resolution), self.ctx.h)
                self._tgt_stamp = self._tgt.stamp
            else:
                keep, p, n, s = _records(self._tgt)
                _l.check(_l.lib().rsreg_ndt_set_target(self.ctx.h, p, n, s, int(getattr(self._tgt, "is_dense", False)),
                                                       self.params.resolution), self.ctx.h)
            self._tgt_dirty = False
            self.ctx.ndt_target_owner = self

    def align(self, guess=None):
        self._sync_target()
        g = _colmajor(guess)
        res = _l.NdtResult()
        if isinstance(self._src, DeviceCloud):
            out = DeviceCloud(ctx=self.ctx)
            _l.check(_l.lib().rsreg_ndt_align_cloud(self.ctx.h, self._src.h, g.ctypes.data if g is not None else None,
                                                    C.byref(self.params), C.byref(res), out.h), self.ctx.h)
            self.result = res
            self._fit_fresh = True
            return out
        keep, p, n, s = _records(self._src)
        out = self._src.points.copy() if isinstance(self._src, PointCloud) else np.zeros(n, POINT_DTYPE)
        _l.check(_l.lib().rsreg_ndt_align(self.ctx.h, p, n, s, int(getattr(self._src, "is_dense", False)),
                                          g.ctypes.data if g is not None else None, C.byref(self.params),
                                          C.byref(res), out.ctypes.data, out.dtype.itemsize), self.ctx.h)
        self.result = res
        self._fit_fresh = True
        src = self._src if isinstance(self._src, PointCloud) else None
        return PointCloud(out, width=src.width if src else n, height=src.height if src else 1,
                          is_dense=src.is_dense if src else False)

    def hasConverged(self):
        return bool(self.result.converged)

    def getFinalTransformation(self):
        return _rowmajor(self.result.transform)

    def getTransformationProbability(self):
        return self.result.trans_probability

    def getFitnessScore(self, max_range=sys.float_info.max):
        """Registration::getFitnessScore(max_range) of the last alignment, against the target's POINTS as PCL scores NDT
        (rsreg_ndt_fitness_score); the squared-range quirk and the sys.float_info.max of IterativeClosestPoint.getFitnessScore."""
        return self.fitnessScore(max_range)[0]

    def fitnessScore(self, max_range=sys.float_info.max):
        """(score, records in range) -- getFitnessScore with the count."""
        _own_alignment(self, self.ctx.ndt_target_owner is self and self._fit_fresh)
        score, nr = C.c_double(0), C.c_uint64(0)
        _l.check(_l.lib().rsreg_ndt_fitness_score(self.ctx.h, float(max_range), C.byref(score), C.byref(nr)), self.ctx.h)
        return score.value, nr.value

    def derivatives(self, pose):
        self._sync_target()
        keep, p, n, s = _records(self._src)
        pose = np.ascontiguousarray(pose, np.float64)
        score = C.c_double(0)
        g = np.zeros(6)
        h = np.zeros((6, 6))
        _l.check(_l.lib().rsreg_ndt_derivatives(self.ctx.h, p, n, s, 0, pose.ctypes.data, C.byref(score),
                                                g.ctypes.data, h.ctypes.data), self.ctx.h)
        return score.value, g, h

    def voxels(self):
        self._sync_target()
        n = C.c_int32(0)
        _l.check(_l.lib().rsreg_ndt_get_voxels(self.ctx.h, C.byref(n), None, None, 0), self.ctx.h)
        m = np.zeros((n.value, 21), np.float64)
        c = np.zeros(n.value, np.int32)
        _l.check(_l.lib().rsreg_ndt_get_voxels(self.ctx.h, C.byref(n), m.ctypes.data, c.ctypes.data, n.value), self.ctx.h)
        return m, c


class ApproximateVoxelGrid:
    """pcl::ApproximateVoxelGrid<PointXYZRGB>.  Without a context: the sequential host filter
    (csrc/voxel_host.cpp); with one: the GPU filter (csrc/voxel.hip), same records in the same order."""

    def __init__(self, ctx=None):
        self.leaf = np.ones(3, np.float32)  # PCL default leaf: 1 m (IncrementalICP never sets it)
        self._in = None
        self.ctx = ctx

    def setLeafSize(self, lx, ly, lz):
        self.leaf = np.array([lx, ly, lz], np.float32)

    def setInputCloud(self, cloud):
        self._in = cloud

    def filter_async(self):
        """filter() of a device cloud queued by a thread of the context on a stream of its own: returns at once; whatever
        takes the result next waits for its size and its records (rsreg_cloud_filter_async).  The input -- which may be
        the not-yet-complete result of extract_edge_features_async -- must stay alive and unchanged until then."""
        out = DeviceCloud(ctx=self._in.ctx)
        _l.check(_l.lib().rsreg_cloud_filter_async(self._in.ctx.h, self._in.h, self.leaf.ctypes.data, out.h), self._in.ctx.h)
        out._filtered_from = self._in   # (keeps the input alive)
        return out

    def filter(self):
        if isinstance(self._in, DeviceCloud):
            out = DeviceCloud(ctx=self._in.ctx)
            _l.check(_l.lib().rsreg_cloud_filter(self._in.ctx.h, self._in.h, self.leaf.ctypes.data, out.h), self._in.ctx.h)
            return out
        pts = np.ascontiguousarray(self._in.points)
        out = np.zeros_like(pts)
        n_out = C.c_size_t(0)
        if self.ctx is not None:
            _l.check(_l.lib().rsreg_approx_voxel_grid_gpu(self.ctx.h, pts.ctypes.data, len(pts), pts.dtype.itemsize,
                                                          self.leaf.ctypes.data, out.ctypes.data, C.byref(n_out)), self.ctx.h)
        else:
            _l.check(_l.lib().rsreg_approx_voxel_grid(pts.ctypes.data, len(pts), pts.dtype.itemsize,
                                                      self.leaf.ctypes.data, out.ctypes.data, C.byref(n_out)))
        out = out[: n_out.value].copy()
        return PointCloud(out, width=len(out), height=1, is_dense=False)


class VoxelGrid:
    """pcl::VoxelGrid<PointXYZRGB>: one centroid per occupied leaf, in ascending leaf index, a leaf's points added in ascending
    input index (include/rsreg.h states the contract).  A DeviceCloud is filtered in HBM (rsreg_cloud_voxel_grid); a host cloud
    on the GPU when a context was given (rsreg_voxel_grid_gpu), else by the sequential host restatement (rsreg_voxel_grid):
    the same bytes from all three.  `info` holds the last filter()'s rsreg_voxel_grid_info.  Not built: the filter-field
    limits (run PassThrough first) and the saved leaf layout."""

    def __init__(self, ctx=None):
        self.params = _l.VoxelGridParams()
        _l.lib().rsreg_voxel_grid_params_default(C.byref(self.params))
        self.info = None
        self._in = None
        self.ctx = ctx

    def setLeafSize(self, lx, ly=None, lz=None):
        """setLeafSize(lx, ly, lz), or setLeafSize(l) for a cubic leaf"""
        ly, lz = (lx, lx) if ly is None else (ly, lz)
        self.params.leaf[0], self.params.leaf[1], self.params.leaf[2] = float(lx), float(ly), float(lz)

    def getLeafSize(self):
        return np.array(self.params.leaf[:], np.float32)

    def setDownsampleAllData(self, on):
        self.params.downsample_all_data = int(bool(on))

    def getDownsampleAllData(self):
        return bool(self.params.downsample_all_data)

    def setMinimumPointsNumberPerVoxel(self, n):
        self.params.min_points_per_voxel = int(n)

    def getMinimumPointsNumberPerVoxel(self):
        return int(self.params.min_points_per_voxel)

    def setInputCloud(self, cloud):
        self._in = cloud

    def getMinBoxCoordinates(self):
        return np.array(self.info.min_b[:], np.int32)

    def getMaxBoxCoordinates(self):
        return np.array(self.info.max_b[:], np.int32)

    def getNrDivisions(self):
        return np.array(self.info.div_b[:], np.int32)

    def getDivisionMultiplier(self):
        return np.array(self.info.divb_mul[:], np.int32)

    def filter(self):
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        info = _l.VoxelGridInfo()
        if isinstance(self._in, DeviceCloud):
            out = DeviceCloud(ctx=self._in.ctx)
            rc = _l.lib().rsreg_cloud_voxel_grid(self._in.ctx.h, self._in.h, C.byref(self.params), out.h, C.byref(info))
            if rc:
                out.close()
            _l.check(rc, self._in.ctx.h)
            self.info = info
            return out
        pts = np.ascontiguousarray(self._in.points)
        out = np.zeros_like(pts)
        n_out = C.c_size_t(0)
        if self.ctx is not None:
            _l.check(_l.lib().rsreg_voxel_grid_gpu(self.ctx.h, pts.ctypes.data, len(pts), pts.dtype.itemsize, C.byref(self.params),
                                                   out.ctypes.data, C.byref(n_out), C.byref(info)), self.ctx.h)
        else:
            _l.check(_l.lib().rsreg_voxel_grid(pts.ctypes.data, len(pts), pts.dtype.itemsize, self.params.leaf, self.params.downsample_all_data,
                                               self.params.min_points_per_voxel, out.ctypes.data, C.byref(n_out), C.byref(info)))
        self.info = info
        out = out[: n_out.value].view(np.uint8).copy().view(out.dtype)   # (byte for byte: .copy() of padded records drops the padding)
        if info.overflowed:   # PCL: "leaf size is too small", the output is the input
            return PointCloud(out, width=self._in.width, height=self._in.height, is_dense=self._in.is_dense)
        return PointCloud(out, width=len(out), height=1, is_dense=True)


def _filter_io(cloud, ctx, run):
    """run(in, out) on device clouds: a DeviceCloud goes in as it is, a host PointCloud through a temporary one."""
    if isinstance(cloud, DeviceCloud):
        out = DeviceCloud(ctx=cloud.ctx)
        run(cloud, out)
        return out
    tmp = DeviceCloud(cloud, ctx=ctx or default_context())
    run(tmp, tmp)
    out = tmp.download()
    tmp.close()
    return out


class PassThrough:
    """pcl::PassThrough<PointXYZRGB> on the GPU (csrc/filters.hip, rsreg_cloud_passthrough) for the fields x, y and z.  A
    record with a non-finite coordinate is always removed.  Any other field name raises (PCL warns and returns an empty
    cloud)."""
    FIELDS = {"x": 0, "y": 1, "z": 2}

    def __init__(self, ctx=None):
        self.field = None
        self.lo, self.hi = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)   # FLT_MIN, FLT_MAX
        self.negative = False
        self.keep_organized = False
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setFilterFieldName(self, name):
        self.field = name

    def setFilterLimits(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def setNegative(self, negative):
        self.negative = bool(negative)

    setFilterLimitsNegative = setNegative

    def setKeepOrganized(self, keep):
        self.keep_organized = bool(keep)

    def filter(self):
        if self.field not in self.FIELDS:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "PassThrough filters on x, y or z, not %r" % (self.field,))
        field = self.FIELDS[self.field]

        def run(cin, cout):
            _l.check(_l.lib().rsreg_cloud_passthrough(cin.ctx.h, cin.h, field, self.lo, self.hi, int(self.negative), int(self.keep_organized),
                                                      cout.h), cin.ctx.h)
        return _filter_io(self._in, self.ctx, run)


class StatisticalOutlierRemoval:
    """pcl::StatisticalOutlierRemoval<PointXYZRGB> on the GPU with an exact k-nearest-neighbour search (csrc/filters.hip,
    rsreg_cloud_sor).  PCL's defaults: mean_k = 1, stddev_mult = 0.  `stats` holds the last call's rsreg_sor_stats."""

    def __init__(self, ctx=None):
        self.mean_k = 1
        self.stddev_mult = 0.0
        self.negative = False
        self.stats = None
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setMeanK(self, k):
        self.mean_k = int(k)

    def setStddevMulThresh(self, m):
        self.stddev_mult = float(m)

    def setNegative(self, negative):
        self.negative = bool(negative)

    def filter(self):
        st = _l.SorStats()

        def run(cin, cout):
            _l.check(_l.lib().rsreg_cloud_sor(cin.ctx.h, cin.h, self.mean_k, self.stddev_mult, int(self.negative), cout.h, C.byref(st)),
                     cin.ctx.h)
        out = _filter_io(self._in, self.ctx, run)
        self.stats = st
        return out


class RadiusOutlierRemoval:
    """pcl::RadiusOutlierRemoval<PointXYZRGB> on the GPU over an exact radius search (csrc/radius_kernels.hpp,
    rsreg_cloud_radius_outlier_removal): a record is removed when it has min_neighbors or fewer neighbours within the radius,
    itself counted, the compare at the radius strict.  PCL's defaults: radius 0 (filter() refuses it), min_neighbors 1.
    `n_kept` holds the last call's number of kept records."""

    def __init__(self, ctx=None):
        self.radius = 0.0
        self.min_neighbors = 1
        self.negative = False
        self.keep_organized = False
        self.n_kept = None
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setRadiusSearch(self, radius):
        self.radius = float(radius)

    def getRadiusSearch(self):
        return self.radius

    def setMinNeighborsInRadius(self, m):
        self.min_neighbors = int(m)

    def getMinNeighborsInRadius(self):
        return self.min_neighbors

    def setNegative(self, negative):
        self.negative = bool(negative)

    def setKeepOrganized(self, keep):
        self.keep_organized = bool(keep)

    def filter(self):
        def run(cin, cout):
            _, self.n_kept = cin.radius_outlier_removal(self.radius, self.min_neighbors, self.negative, self.keep_organized, out=cout)
        return _filter_io(self._in, self.ctx, run)


class EuclideanClusterExtraction:
    """pcl::EuclideanClusterExtraction<PointXYZRGB> on the GPU over the exact radius search (csrc/cluster_kernels.hpp,
    rsreg_cloud_euclidean_clusters; include/rsreg.h holds the contract).  PCL's defaults: tolerance 0 (extract() refuses it),
    sizes 1 .. INT_MAX.  extract() gives a list of int32 arrays, a cluster's record indices each, ascending, the largest cluster
    first.  No setIndices, no setSearchMethod."""

    def __init__(self, ctx=None):
        self.tolerance = 0.0
        self.min_cluster_size = 1
        self.max_cluster_size = 2**31 - 1
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setClusterTolerance(self, tolerance):
        self.tolerance = float(tolerance)

    def getClusterTolerance(self):
        return self.tolerance

    def setMinClusterSize(self, m):
        self.min_cluster_size = int(m)

    def getMinClusterSize(self):
        return self.min_cluster_size

    def setMaxClusterSize(self, m):
        self.max_cluster_size = int(m)

    def getMaxClusterSize(self):
        return self.max_cluster_size

    def extract(self):
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        on_device = isinstance(self._in, DeviceCloud)
        dev = self._in if on_device else DeviceCloud(self._in, ctx=self.ctx or default_context())
        try:
            _, indices, offsets = dev.euclidean_clusters(self.tolerance, self.min_cluster_size, self.max_cluster_size)
        finally:
            if not on_device:
                dev.close()
        return [indices[offsets[c]:offsets[c + 1]].astype(np.int32) for c in range(len(offsets) - 1)]


SACMODEL_PLANE, SACMODEL_PERPENDICULAR_PLANE = 0, 9    # pcl::SacModel
SAC_RANSAC = 0                                         # pcl::SAC_RANSAC


def plane_params(**kw):
    """rsreg_plane_params: the defaults (rsreg_plane_params_default) with the given fields replaced; axis: three numbers."""
    p = _l.PlaneParams()
    _l.lib().rsreg_plane_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(p._fields_):
            raise TypeError("rsreg_plane_params has no field %r" % k)
        if k == "axis":
            v = (C.c_double * 3)(*[float(a) for a in v])
        setattr(p, k, v)
    return p


class PlaneResult:
    """rsreg_plane_result: found, best_hypothesis, sample, iterations, skipped, refined, n_inliers, cos_eps, unrefined (4,), sums (10,)"""

    def __init__(self, r):
        self.found, self.best_hypothesis, self.sample = bool(r.found), int(r.best_hypothesis), tuple(r.sample)
        self.iterations, self.skipped, self.refined, self.n_inliers = int(r.iterations), int(r.skipped), bool(r.refined), int(r.n_inliers)
        self.cos_eps = float(r.cos_eps)
        self.unrefined = np.array(list(r.unrefined), np.float32)
        self.sums = np.array(list(r.sums), np.float64)


def plane_from_sums(sums, p0, prior):
    """rsreg_plane_from_sums (host only): the refined model (4,) float32 from the ten sums relative to p0, its normal on the side
    of `prior`'s; None when there are fewer than three inliers or the covariance is not finite."""
    s = np.ascontiguousarray(sums, np.float64).reshape(_l.NUM_PLANE_SEG_SUMS)
    q, m = np.ascontiguousarray(p0, np.float32).reshape(3), np.ascontiguousarray(prior, np.float32).reshape(4)
    out = np.zeros(4, np.float32)
    rc = _l.lib().rsreg_plane_from_sums(s.ctypes.data, q.ctypes.data, m.ctypes.data, out.ctypes.data)
    return None if rc else out


class SACSegmentation:
    """pcl::SACSegmentation<PointXYZRGB> on the GPU for SACMODEL_PLANE and SACMODEL_PERPENDICULAR_PLANE with SAC_RANSAC: batches of
    plane hypotheses, each scored against every record (csrc/plane_seg_kernels.hpp, rsreg_cloud_plane_segment; include/rsreg.h holds
    the contract and the stated deviations from PCL).  PCL's defaults: max_iterations 50, probability 0.99, optimize_coefficients
    on, distance_threshold 0.  segment() gives (the inliers' record indices int32 ascending, the coefficients (4,) float32) -- an
    empty list and zeros when no model was found; `result` holds the last call's PlaneResult.  setSeed is the one addition."""

    def __init__(self, ctx=None):
        self.params = plane_params()
        self.model_type = SACMODEL_PLANE
        self.method_type = SAC_RANSAC
        self.result = None
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setModelType(self, model):
        if model not in (SACMODEL_PLANE, SACMODEL_PERPENDICULAR_PLANE):
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "SACSegmentation fits SACMODEL_PLANE and SACMODEL_PERPENDICULAR_PLANE only")
        self.model_type = model

    def setMethodType(self, method):
        if method != SAC_RANSAC:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "SACSegmentation runs SAC_RANSAC only")
        self.method_type = method

    def setDistanceThreshold(self, threshold):
        self.params.distance_threshold = float(threshold)

    def getDistanceThreshold(self):
        return self.params.distance_threshold

    def setMaxIterations(self, n):
        self.params.max_iterations = int(n)

    def getMaxIterations(self):
        return self.params.max_iterations

    def setProbability(self, p):
        self.params.probability = float(p)

    def getProbability(self):
        return self.params.probability

    def setOptimizeCoefficients(self, on):
        self.params.optimize_coefficients = int(bool(on))

    def getOptimizeCoefficients(self):
        return bool(self.params.optimize_coefficients)

    def setAxis(self, axis):
        self.params.axis = (C.c_double * 3)(*[float(a) for a in axis])

    def getAxis(self):
        return tuple(self.params.axis)

    def setEpsAngle(self, eps):
        self.params.eps_angle = float(eps)

    def getEpsAngle(self):
        return self.params.eps_angle

    def setSeed(self, seed):
        self.params.seed = int(seed)

    def segment(self):
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        prm = {k: getattr(self.params, k) for k, _ in self.params._fields_}
        if self.model_type == SACMODEL_PLANE:   # (PCL's plain plane model ignores the axis)
            prm["axis"], prm["eps_angle"] = (0.0, 0.0, 0.0), 0.0
        on_device = isinstance(self._in, DeviceCloud)
        dev = self._in if on_device else DeviceCloud(self._in, ctx=self.ctx or default_context())
        try:
            coeff, inliers, self.result = dev.segment_plane(**prm)
        finally:
            if not on_device:
                dev.close()
        return inliers, coeff


class ExtractIndices:
    """pcl::ExtractIndices<PointXYZRGB> on the GPU (rsreg_cloud_extract_indices): the records an index list names, in its order and
    with its repeats; setNegative(True): the records it does not name, in input order.  `n_kept` holds the last call's number of
    kept records."""

    def __init__(self, ctx=None):
        self.indices = np.zeros(0, np.int32)
        self.negative = False
        self.n_kept = None
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setIndices(self, indices):
        self.indices = np.ascontiguousarray(indices, np.int32).reshape(-1)

    def setNegative(self, negative):
        self.negative = bool(negative)

    def getNegative(self):
        return self.negative

    def filter(self):
        def run(cin, cout):
            _, self.n_kept = cin.extract_indices(self.indices, self.negative, out=cout)
        return _filter_io(self._in, self.ctx, run)


class ISSKeypoint3D:
    """pcl::ISSKeypoint3D<PointXYZRGB, PointXYZRGB> on the GPU over the exact radius search (csrc/iss_kernels.hpp,
    rsreg_cloud_iss_keypoints; include/rsreg.h holds the contract): the records whose scatter over the salient radius has
    eigenvalue ratios below gamma_21 and gamma_32 and whose smallest eigenvalue no neighbour within the non-max radius exceeds.
    PCL's defaults: both radii 0 (compute() refuses them), thresholds 0.975, min_neighbors 5.  Border estimation (setBorderRadius,
    setNormalRadius above 0) is not built and compute() says so; no setIndices, no setSearchSurface.  compute() of a DeviceCloud
    gives a DeviceCloud of the keypoints, of a host cloud a PointCloud; getKeypointsIndices() their record indices."""

    def __init__(self, ctx=None):
        self.salient_radius = 0.0
        self.non_max_radius = 0.0
        self.gamma_21 = 0.975
        self.gamma_32 = 0.975
        self.min_neighbors = 5
        self.border_radius = 0.0
        self.normal_radius = 0.0
        self._indices = np.zeros(0, np.int32)
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setSalientRadius(self, radius):
        self.salient_radius = float(radius)

    def setNonMaxRadius(self, radius):
        self.non_max_radius = float(radius)

    def setThreshold21(self, gamma):
        self.gamma_21 = float(gamma)

    def setThreshold32(self, gamma):
        self.gamma_32 = float(gamma)

    def setMinNeighbors(self, m):
        self.min_neighbors = int(m)

    def setBorderRadius(self, radius):
        self.border_radius = float(radius)

    def setNormalRadius(self, radius):
        self.normal_radius = float(radius)

    def getKeypointsIndices(self):
        return self._indices

    def compute(self):
        if self.border_radius > 0.0 or self.normal_radius > 0.0:   # (before any device call)
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "ISSKeypoint3D: border estimation (setBorderRadius / setNormalRadius) is not built")
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        on_device = isinstance(self._in, DeviceCloud)
        dev = self._in if on_device else DeviceCloud(self._in, ctx=self.ctx or default_context())
        try:
            out, self._indices = dev.iss_keypoints(salient_radius=self.salient_radius, non_max_radius=self.non_max_radius, gamma_21=self.gamma_21,
                                                   gamma_32=self.gamma_32, min_neighbors=self.min_neighbors)
            if on_device:
                return out
            host = out.download()
            out.close()
            return host
        finally:
            if not on_device:
                dev.close()


def _compute_over_surface(est, run, download):
    """compute() of an estimator with an input cloud (est._in) and an optional search surface (est._surface), each a host cloud or
    a DeviceCloud: run(input on the device, surface on the device or None) gives the DeviceCloud of the rows; a DeviceCloud input
    gets it as it is, a host input gets download(rows).  What was uploaded here is released here."""
    ctx = next((c.ctx for c in (est._in, est._surface) if isinstance(c, DeviceCloud)), None) or est.ctx or default_context()
    made = []

    def on_device(cloud):
        if cloud is None or isinstance(cloud, DeviceCloud):
            return cloud
        made.append(DeviceCloud(cloud, ctx=ctx))
        return made[-1]

    try:
        dev_in, dev_surface = on_device(est._in), on_device(est._surface)
        rows = run(dev_in, dev_surface) if dev_surface is not None else run(dev_in)
        if isinstance(est._in, DeviceCloud):
            return rows
        out = download(rows)
        rows.close()
        return out
    finally:
        for d in made:
            d.close()


class NormalEstimation:
    """pcl::NormalEstimation<PointXYZRGB, Normal> on the GPU: with setKSearch over an exact k-nearest-neighbour search
    (csrc/normals_kernels.hpp, rsreg_cloud_normals), 3 <= k <= 64, or with setRadiusSearch over an exact radius search
    (csrc/radius_kernels.hpp, rsreg_cloud_normals_radius), any number of neighbours.  As in PCL exactly one of the two is set:
    compute() refuses both and neither; setKSearch(0) / setRadiusSearch(0) unset them.  The covariance is the one the formula
    defines, in double about the query point: PCL's float accumulation about the origin is not reproduced (include/rsreg.h).
    setSearchSurface (with setRadiusSearch only): the neighbours come from another cloud (csrc/surface_kernels.hpp,
    rsreg_cloud_normals_radius_surface).  compute() of a DeviceCloud gives a DeviceCloud of pcl::Normal records, of a host cloud a NormalCloud."""

    def __init__(self, ctx=None):
        self.k = 0                                   # PCL's default: no search set
        self.radius = 0.0
        self.viewpoint = (0.0, 0.0, 0.0)
        self._in = None
        self._surface = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setKSearch(self, k):
        self.k = int(k)

    def getKSearch(self):
        return self.k

    def setRadiusSearch(self, radius):
        self.radius = float(radius)

    def getRadiusSearch(self):
        return self.radius

    def setViewPoint(self, vx, vy, vz):
        self.viewpoint = (float(vx), float(vy), float(vz))

    def getViewPoint(self):
        return self.viewpoint

    def setSearchSurface(self, surface):
        """The cloud the neighbours are taken from (a host cloud or a DeviceCloud; None: the input cloud itself, PCL's default).
        With a surface only setRadiusSearch is built."""
        self._surface = surface

    def _normals_cloud(self, dev, surface=None):
        if surface is not None:
            return dev.normals_radius_surface_cloud(surface, self.radius, self.viewpoint)
        return dev.normals_radius_cloud(self.radius, self.viewpoint) if self.radius != 0.0 else dev.normals_cloud(self.k, self.viewpoint)

    def compute(self):
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        if self.k != 0 and self.radius != 0.0:   # (before any device call, as PCL's initCompute)
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "both setKSearch and setRadiusSearch are set: set one of them to 0")
        if self.k == 0 and self.radius == 0.0:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "neither setKSearch nor setRadiusSearch is set")
        if self._surface is not None and self.k != 0:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "NormalEstimation: setKSearch with setSearchSurface is not built; use setRadiusSearch")
        return _compute_over_surface(self, self._normals_cloud, lambda dev: dev.download_normals())


class FPFHEstimation:
    """pcl::FPFHEstimation<PointXYZRGB, Normal, FPFHSignature33> on the GPU with setKSearch, 2 <= k <= 64, over the exact
    k-nearest-neighbour search (csrc/fpfh_kernels.hpp, rsreg_cloud_fpfh; include/rsreg.h holds the contract).  PCL's two quirks are
    kept -- the weight is 1 / squared distance, the record's own SPFH does not enter -- and the pair features are computed in
    double, not in float.  setRadiusSearch and setSearchSurface are refused here: FPFHEstimationOMP, below, takes either search
    and, with a radius, a search surface.  setIndices is not built.  compute() of a DeviceCloud gives a DeviceCloud of pcl::FPFHSignature33 records, of a host cloud an
    FPFHCloud."""

    def __init__(self, ctx=None):
        self.k = 0                                   # PCL's default: no search set
        self._in = None
        self._normals = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setInputNormals(self, normals):
        self._normals = normals

    def setKSearch(self, k):
        self.k = int(k)

    def getKSearch(self):
        return self.k

    def setRadiusSearch(self, radius):
        if float(radius) != 0.0:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "FPFHEstimation: setRadiusSearch is not built; use setKSearch")

    def setSearchSurface(self, surface):
        if surface is not None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "FPFHEstimation: setSearchSurface is not built; use FPFHEstimationOMP with setRadiusSearch")

    def compute(self):
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        if self._normals is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputNormals not called")
        if self.k == 0:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setKSearch not called")
        if isinstance(self._in, DeviceCloud):
            return self._in.fpfh_cloud(self._normals, self.k)
        tmp = DeviceCloud(self._in, ctx=self.ctx or default_context())
        try:
            dev = tmp.fpfh_cloud(self._normals, self.k)
            out = dev.download_fpfh()
            dev.close()
        finally:
            tmp.close()
        return out


class FPFHEstimationOMP:
    """pcl::FPFHEstimationOMP<PointXYZRGB, Normal, FPFHSignature33> on the GPU: with setKSearch, 2 <= k <= 64, the bytes of
    FPFHEstimation (rsreg_cloud_fpfh); with setRadiusSearch over the exact radius search (csrc/fpfh_radius_kernels.hpp,
    rsreg_cloud_fpfh_radius; include/rsreg.h holds the contract), any number of neighbours, the histogram sums in double.  As in
    PCL exactly one of the two is set: compute() refuses both and neither before any device call; setKSearch(0) /
    setRadiusSearch(0) unset them.  setNumberOfThreads is accepted and ignored.  setSearchSurface (with setRadiusSearch only): the
    descriptors of the input cloud's records over another cloud and that cloud's normals (csrc/surface_kernels.hpp,
    rsreg_cloud_fpfh_radius_surface).  compute() of a DeviceCloud gives a DeviceCloud of
    pcl::FPFHSignature33 records, of a host cloud an FPFHCloud."""

    def __init__(self, ctx=None):
        self.k = 0                                   # PCL's default: no search set
        self.radius = 0.0
        self.threads = 0
        self._in = None
        self._surface = None
        self._normals = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setInputNormals(self, normals):
        self._normals = normals

    def setKSearch(self, k):
        self.k = int(k)

    def getKSearch(self):
        return self.k

    def setRadiusSearch(self, radius):
        self.radius = float(radius)

    def getRadiusSearch(self):
        return self.radius

    def setNumberOfThreads(self, threads=0):
        self.threads = int(threads)

    def setSearchSurface(self, surface):
        """The cloud the neighbours are taken from (a host cloud or a DeviceCloud; None: the input cloud itself, PCL's default).
        With a surface setInputNormals must hold the SURFACE's normals, as in PCL, and only setRadiusSearch is built."""
        self._surface = surface

    def _fpfh_cloud(self, dev, surface=None):
        if surface is not None:
            return dev.fpfh_radius_surface_cloud(surface, self._normals, self.radius)
        return dev.fpfh_radius_cloud(self._normals, self.radius) if self.radius != 0.0 else dev.fpfh_cloud(self._normals, self.k)

    def compute(self):
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        if self._normals is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputNormals not called")
        if self.k != 0 and self.radius != 0.0:   # (before any device call, as PCL's initCompute)
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "both setKSearch and setRadiusSearch are set: set one of them to 0")
        if self.k == 0 and self.radius == 0.0:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "neither setKSearch nor setRadiusSearch is set")
        if self._surface is not None and self.k != 0:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "FPFHEstimationOMP: setKSearch with setSearchSurface is not built; use setRadiusSearch")
        return _compute_over_surface(self, self._fpfh_cloud, lambda dev: dev.download_fpfh())


class CorrespondenceEstimation:
    """pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33> on the GPU: every valid source descriptor's
    nearest valid target descriptor by an exact brute-force search (csrc/feature_kernels.hpp,
    rsreg_cloud_feature_correspondences; include/rsreg.h holds the contract).  setInputSource / setInputTarget take a DeviceCloud
    of descriptor records (what FPFHEstimation.compute returns for a DeviceCloud) or a host FPFHCloud, which is uploaded into a
    temporary.  Both calls return a CORRESPONDENCE_DTYPE array ordered by index_query; distance is the squared distance, a match AT
    max_distance is kept.  setIndices and the rejectors are not built."""

    def __init__(self, ctx=None):
        self._src = None
        self._tgt = None
        self.ctx = ctx

    def setInputSource(self, cloud):
        self._src = cloud

    def setInputTarget(self, cloud):
        self._tgt = cloud

    def _run(self, max_distance, reciprocal):
        if self._src is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputSource not called")
        if self._tgt is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputTarget not called")
        ctx = next((c.ctx for c in (self._src, self._tgt) if isinstance(c, DeviceCloud)), None) or self.ctx or default_context()
        made = []
        try:
            pair = []
            for c in (self._src, self._tgt):
                if not isinstance(c, DeviceCloud):
                    c = DeviceCloud(c, ctx=ctx)
                    made.append(c)
                pair.append(c)
            return pair[0].feature_correspondences(pair[1], max_distance, reciprocal)
        finally:
            for c in made:
                c.close()

    def determineCorrespondences(self, max_distance=sys.float_info.max):
        return self._run(max_distance, False)

    def determineReciprocalCorrespondences(self, max_distance=sys.float_info.max):
        return self._run(max_distance, True)


def sac_params(**kw):
    """rsreg_sac_params: PCL's defaults (rsreg_sac_params_default) with the given fields replaced."""
    p = _l.SacParams()
    _l.lib().rsreg_sac_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(p._fields_):
            raise TypeError("rsreg_sac_params has no field %r" % k)
        setattr(p, k, v)
    return p


class SacResult:
    """rsreg_sac_result: transform (4 x 4), found, best_hypothesis, sample, iterations, n_inliers, refit_rounds_run, sums; n_out: the
    correspondences kept (which may exceed the capacity that was given)."""

    def __init__(self, r, n_out):
        self.transform = _rowmajor(list(r.transform))
        self.found, self.best_hypothesis, self.sample = bool(r.found), int(r.best_hypothesis), tuple(r.sample)
        self.iterations, self.n_inliers, self.refit_rounds_run = int(r.iterations), int(r.n_inliers), int(r.refit_rounds_run)
        self.sums = np.array(list(r.sums), np.float64)
        self.n_out = int(n_out)


def _as_device_pair(src, tgt, ctx):
    """(source, target, made): both as DeviceClouds of one context; made: the temporaries uploaded for host clouds"""
    ctx = next((c.ctx for c in (src, tgt) if isinstance(c, DeviceCloud)), None) or ctx or default_context()
    pair, made = [], []
    for c in (src, tgt):
        if not isinstance(c, DeviceCloud):
            c = DeviceCloud(c, ctx=ctx)
            made.append(c)
        pair.append(c)
    return pair[0], pair[1], made


class CorrespondenceRejectorSampleConsensus:
    """pcl::registration::CorrespondenceRejectorSampleConsensus on the GPU: RANSAC over a correspondence list, thousands of
    hypotheses each scored against every pair (csrc/sac_kernels.hpp, rsreg_cloud_sac_correspondences; include/rsreg.h holds the
    contract and the stated deviations from PCL).  setInputSource / setInputTarget take a DeviceCloud or a host PointCloud (uploaded
    into a temporary).  setRefineModel(True) is one refit round over the inliers, not PCL's refineModel."""

    def __init__(self, ctx=None):
        self._src = self._tgt = self._corr = None
        self.ctx = ctx
        self.params = sac_params()
        self._result = None

    def setInputSource(self, cloud):
        self._src = cloud

    def setInputTarget(self, cloud):
        self._tgt = cloud

    def setInlierThreshold(self, threshold):
        self.params.inlier_threshold = float(threshold)

    def getInlierThreshold(self):
        return self.params.inlier_threshold

    def setMaximumIterations(self, n):
        self.params.max_iterations = int(n)

    def getMaximumIterations(self):
        return self.params.max_iterations

    def setRefineModel(self, on):
        self.params.refit_rounds = 1 if on else 0

    def setInputCorrespondences(self, corr):
        self._corr = np.ascontiguousarray(corr, CORRESPONDENCE_DTYPE)

    def getRemainingCorrespondences(self, corr):
        """The correspondences of `corr` that RANSAC keeps, in input order; getBestTransformation() is theirs afterwards."""
        if self._src is None or self._tgt is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputSource / setInputTarget not called")
        src, tgt, made = _as_device_pair(self._src, self._tgt, self.ctx)
        try:
            kept, self._result = src.sac_correspondences(tgt, corr, **{k: getattr(self.params, k) for k, _ in self.params._fields_})
        finally:
            for c in made:
                c.close()
        return kept

    def getCorrespondences(self):
        if self._corr is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCorrespondences not called")
        return self.getRemainingCorrespondences(self._corr)

    def getBestTransformation(self):
        return np.eye(4, dtype=np.float32) if self._result is None else self._result.transform

    @property
    def result(self):
        return self._result


def prerej_params(**kw):
    """rsreg_prerej_params: the defaults (rsreg_prerej_params_default) with the given fields replaced."""
    p = _l.PrerejParams()
    _l.lib().rsreg_prerej_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(p._fields_):
            raise TypeError("rsreg_prerej_params has no field %r" % k)
        setattr(p, k, v)
    return p


class PrerejResult:
    """rsreg_prerej_result: transform (4 x 4), found, best_hypothesis, sample (source records), match (target records), n_valid,
    n_inliers, fitness; n_out: the winner's inliers (which may exceed the capacity that was given)."""

    def __init__(self, r, n_out):
        self.transform = _rowmajor(list(r.transform))
        self.found, self.best_hypothesis = bool(r.found), int(r.best_hypothesis)
        self.sample, self.match = tuple(r.sample), tuple(r.match)
        self.n_valid, self.n_inliers, self.fitness = int(r.n_valid), int(r.n_inliers), float(r.fitness)
        self.n_out = int(n_out)


class SampleConsensusPrerejective:
    """pcl::SampleConsensusPrerejective on the GPU: poses from three source records and a random one of each one's k nearest
    descriptors, pre-rejected on their edge lengths, the survivors scored against the whole target cloud by an exact nearest-point
    search (csrc/prerej_kernels.hpp, rsreg_cloud_prerejective; include/rsreg.h holds the contract and the stated deviations from
    PCL).  The clouds are DeviceClouds or host PointClouds, the features DeviceClouds of descriptor records (what
    FPFHEstimation.compute returns for a DeviceCloud) or host FPFHClouds; host inputs are uploaded into temporaries.  align() makes two
    calls, rsreg_cloud_feature_knn and rsreg_cloud_prerejective, and returns the source moved by the final transformation.
    params.select_by_inliers = 1 and params.seed are this library's own."""

    def __init__(self, ctx=None):
        self._src = self._tgt = self._src_feat = self._tgt_feat = None
        self.ctx = ctx
        self.params = prerej_params()
        self.k = 2                                   # PCL's default correspondence randomness
        self._result = None
        self._inliers = np.zeros(0, np.int32)

    def setInputSource(self, cloud):
        self._src = cloud

    def setInputTarget(self, cloud):
        self._tgt = cloud

    def setSourceFeatures(self, features):
        self._src_feat = features

    def setTargetFeatures(self, features):
        self._tgt_feat = features

    def setMaximumIterations(self, n):
        self.params.max_iterations = int(n)

    def setNumberOfSamples(self, n):
        if int(n) != 3:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "SampleConsensusPrerejective: only three samples are built")

    def getNumberOfSamples(self):
        return 3

    def setCorrespondenceRandomness(self, k):
        self.k = int(k)

    def getCorrespondenceRandomness(self):
        return self.k

    def setSimilarityThreshold(self, t):
        self.params.similarity_threshold = float(t)

    def getSimilarityThreshold(self):
        return self.params.similarity_threshold

    def setMaxCorrespondenceDistance(self, d):
        self.params.max_correspondence_distance = float(d)

    def setInlierFraction(self, f):
        self.params.inlier_fraction = float(f)

    def getInlierFraction(self):
        return self.params.inlier_fraction

    def align(self):
        for what, v in (("setInputSource", self._src), ("setInputTarget", self._tgt), ("setSourceFeatures", self._src_feat),
                        ("setTargetFeatures", self._tgt_feat)):
            if v is None:
                raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, what + " not called")
        ctx = next((c.ctx for c in (self._src, self._tgt, self._src_feat, self._tgt_feat) if isinstance(c, DeviceCloud)), None) or self.ctx or default_context()
        src, tgt, made = _as_device_pair(self._src, self._tgt, ctx)
        try:
            fs, ft, more = _as_device_pair(self._src_feat, self._tgt_feat, ctx)
            made += more
            nbr, _ = fs.feature_knn(ft, self.k)
            self._inliers, self._result = src.prerejective(tgt, nbr, **{k: getattr(self.params, k) for k, _ in self.params._fields_})
            moved = transformPointCloud(src, self._result.transform)
            if isinstance(self._src, DeviceCloud):
                return moved
            out = moved.download()
            moved.close()
            return out
        finally:
            for c in made:
                c.close()

    def hasConverged(self):
        return self._result is not None and self._result.found

    def getFinalTransformation(self):
        return np.eye(4, dtype=np.float32) if self._result is None else self._result.transform

    def getInliers(self):
        return self._inliers

    def getFitnessScore(self):
        """the winner's error, sum of its inliers' squared distances / their number (0.0 without a winner)"""
        return 0.0 if self._result is None else self._result.fitness

    @property
    def result(self):
        return self._result


SCIA_TRUNCATED, SCIA_HUBER = _l.SCIA_TRUNCATED, _l.SCIA_HUBER


def scia_params(**kw):
    """rsreg_scia_params: the defaults (rsreg_scia_params_default) with the given fields replaced."""
    p = _l.SciaParams()
    _l.lib().rsreg_scia_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(p._fields_):
            raise TypeError("rsreg_scia_params has no field %r" % k)
        setattr(p, k, v)
    return p


class SciaResult:
    """rsreg_scia_result: transform (4 x 4), found (a hypothesis won, not the guess), best_hypothesis, sample (source records) and
    match (target records), -1 behind nr_samples, n_valid, error."""

    def __init__(self, r):
        self.transform = _rowmajor(list(r.transform))
        self.found, self.best_hypothesis = bool(r.found), int(r.best_hypothesis)
        self.sample, self.match = tuple(r.sample), tuple(r.match)
        self.n_valid, self.error = int(r.n_valid), float(r.error)


class SampleConsensusInitialAlignment:
    """pcl::SampleConsensusInitialAlignment on the GPU: poses from nr_samples source records that keep a minimum distance from one
    another and a random one of each one's k nearest descriptors; none is thrown away, every one is scored over every source record
    by a bounded penalty of its exact nearest-point distance (csrc/scia_kernels.hpp, rsreg_cloud_initial_alignment; include/rsreg.h
    holds the contract and the stated deviations from PCL).  Clouds and features as SampleConsensusPrerejective takes them.  align()
    makes two calls, rsreg_cloud_feature_knn and rsreg_cloud_initial_alignment, and returns the source moved by the final
    transformation.  As in PCL, setMaxCorrespondenceDistance is compared with the SQUARED distance.  params.seed is this library's own."""

    def __init__(self, ctx=None):
        self._src = self._tgt = self._src_feat = self._tgt_feat = None
        self.ctx = ctx
        self.params = scia_params()
        self.k = 10                                  # PCL's default k_correspondences_
        self._result = None

    def setInputSource(self, cloud):
        self._src = cloud

    def setInputTarget(self, cloud):
        self._tgt = cloud

    def setSourceFeatures(self, features):
        self._src_feat = features

    def setTargetFeatures(self, features):
        self._tgt_feat = features

    def setMaximumIterations(self, n):
        self.params.max_iterations = int(n)

    def setNumberOfSamples(self, n):
        self.params.nr_samples = int(n)

    def getNumberOfSamples(self):
        return self.params.nr_samples

    def setCorrespondenceRandomness(self, k):
        self.k = int(k)

    def getCorrespondenceRandomness(self):
        return self.k

    def setMinSampleDistance(self, d):
        self.params.min_sample_distance = float(d)

    def getMinSampleDistance(self):
        return self.params.min_sample_distance

    def setMaxCorrespondenceDistance(self, d):
        self.params.max_correspondence_distance = float(d)

    def setErrorFunction(self, f):
        self.params.error_function = int(f)

    def setSeed(self, seed):
        self.params.seed = int(seed)

    def align(self, guess=None):
        for what, v in (("setInputSource", self._src), ("setInputTarget", self._tgt), ("setSourceFeatures", self._src_feat),
                        ("setTargetFeatures", self._tgt_feat)):
            if v is None:
                raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, what + " not called")
        ctx = next((c.ctx for c in (self._src, self._tgt, self._src_feat, self._tgt_feat) if isinstance(c, DeviceCloud)), None) or self.ctx or default_context()
        src, tgt, made = _as_device_pair(self._src, self._tgt, ctx)
        try:
            fs, ft, more = _as_device_pair(self._src_feat, self._tgt_feat, ctx)
            made += more
            nbr, _ = fs.feature_knn(ft, self.k)
            self._result = src.initial_alignment(tgt, nbr, guess=guess, **{k: getattr(self.params, k) for k, _ in self.params._fields_})
            moved = transformPointCloud(src, self._result.transform)
            if isinstance(self._src, DeviceCloud):
                return moved
            out = moved.download()
            moved.close()
            return out
        finally:
            for c in made:
                c.close()

    def hasConverged(self):
        return self._result is not None and self._result.found

    def getFinalTransformation(self):
        return np.eye(4, dtype=np.float32) if self._result is None else self._result.transform

    def getFitnessScore(self):
        """the winner's error (+inf before align(), or when nothing was scored)"""
        return float("inf") if self._result is None else self._result.error

    @property
    def result(self):
        return self._result


class TransformationEstimationSVD:
    """pcl::registration::TransformationEstimationSVD with a correspondence list (rsreg_cloud_estimate_rigid_svd): the fit over
    the finite pairs, the sums in double in a fixed order on the GPU."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def estimateRigidTransformation(self, source, target, correspondences):
        src, tgt, made = _as_device_pair(source, target, self.ctx)
        try:
            return src.estimate_rigid_svd(tgt, correspondences)[0]
        finally:
            for c in made:
                c.close()


class IntegralImageNormalEstimation:
    """pcl::IntegralImageNormalEstimation<PointXYZRGB, Normal> on the GPU for organized clouds (csrc/iinormals_kernels.hpp,
    rsreg_cloud_integral_normals) as src/edge_extractor.hpp:9-15 sets it up: AVERAGE_3D_GRADIENT, the IGNORE border policy,
    no depth-dependent smoothing; anything else is refused.  The window sums are the double sums of the window's elements,
    not differences of PCL's table (include/rsreg.h states the deviation).  compute() of a DeviceCloud gives a DeviceCloud of
    pcl::Normal records, of a host cloud a NormalCloud."""
    COVARIANCE_MATRIX, AVERAGE_3D_GRADIENT, AVERAGE_DEPTH_CHANGE, SIMPLE_3D_GRADIENT = 0, 1, 2, 3
    BORDER_POLICY_IGNORE, BORDER_POLICY_MIRROR = 0, 1

    def __init__(self, ctx=None):
        self.params = iin_params()
        self._in = None
        self.ctx = ctx

    def setInputCloud(self, cloud):
        self._in = cloud

    def setNormalEstimationMethod(self, method):
        self.params.method = int(method)

    def setMaxDepthChangeFactor(self, factor):
        self.params.max_depth_change_factor = float(factor)

    def setNormalSmoothingSize(self, size):
        self.params.normal_smoothing_size = float(size)

    def setDepthDependentSmoothing(self, on):
        self.params.depth_dependent_smoothing = int(bool(on))

    def setBorderPolicy(self, policy):
        self.params.border_policy = int(policy)

    def setViewPoint(self, vx, vy, vz):
        self.params.viewpoint = (C.c_float * 3)(float(vx), float(vy), float(vz))

    def getViewPoint(self):
        return tuple(self.params.viewpoint)

    def compute(self):
        if self._in is None:
            raise _l.RsregError(_l.RSREG_ERR_INVALID_ARG, "setInputCloud not called")
        if isinstance(self._in, DeviceCloud):
            return self._in.integral_normals_cloud(self.params)
        tmp = DeviceCloud(self._in, ctx=self.ctx or default_context())
        try:
            dev = tmp.integral_normals_cloud(self.params)
            out = dev.download_normals()
            dev.close()
        finally:
            tmp.close()
        return out


def transformPointCloud(cloud, T, ctx=None):
    """pcl::transformPointCloud(in, out, Matrix4f): returns the transformed copy."""
    if isinstance(cloud, DeviceCloud):
        out = DeviceCloud(ctx=cloud.ctx)
        t = _colmajor(T)
        _l.check(_l.lib().rsreg_cloud_transform(cloud.ctx.h, cloud.h, t.ctypes.data, out.h), cloud.ctx.h)
        return out
    ctx = ctx or default_context()
    pts = np.ascontiguousarray(cloud.points)
    out = np.empty_like(pts)
    t = _colmajor(T)
    _l.check(_l.lib().rsreg_transform_cloud(ctx.h, pts.ctypes.data, out.ctypes.data, len(pts), pts.dtype.itemsize,
                                            int(cloud.is_dense), t.ctypes.data), ctx.h)
    return PointCloud(out, width=cloud.width, height=cloud.height, is_dense=cloud.is_dense)


def extract_edge_features_async(cloud):
    """extract_edge_features of a DeviceCloud queued by a thread of the context on a stream of its own
    (rsreg_cloud_edge_features_async): returns at once; the result is complete when a call that takes it has waited for
    it (every one does).  `cloud` -- which may still be uploading -- must stay as it is until then."""
    out = DeviceCloud(ctx=cloud.ctx)
    _l.check(_l.lib().rsreg_cloud_edge_features_async(cloud.ctx.h, cloud.h, out.h), cloud.ctx.h)
    out._features_of = cloud   # (keeps the input alive)
    return out


def extract_edge_features(cloud, ctx=None, want_indices=False):
    """extract_edge_features(cloud) of the reference (src/edge_extractor.hpp:7-39): the RGB-Canny edge points
    of an ORGANIZED cloud, in index order.  A DeviceCloud in gives a DeviceCloud out."""
    if isinstance(cloud, DeviceCloud):
        out = DeviceCloud(ctx=cloud.ctx)
        _l.check(_l.lib().rsreg_cloud_edge_features(cloud.ctx.h, cloud.h, out.h), cloud.ctx.h)
        return out
    ctx = ctx or default_context()
    pts = np.ascontiguousarray(cloud.points)
    if cloud.width * cloud.height != len(pts):
        raise ValueError("edge extraction needs an organized cloud (width x height points)")
    out = np.zeros_like(pts)
    idx = np.zeros(len(pts), np.int32)
    n_out = C.c_size_t(0)
    _l.check(_l.lib().rsreg_extract_edge_features(ctx.h, pts.ctypes.data, cloud.width, cloud.height, pts.dtype.itemsize,
                                                  out.ctypes.data, idx.ctypes.data, C.byref(n_out)), ctx.h)
    n = n_out.value
    res = PointCloud(out[:n].copy(), width=n, height=1, is_dense=cloud.is_dense)
    return (res, idx[:n].copy()) if want_indices else res


def umeyama_from_sums(sums):
    sums = np.ascontiguousarray(sums, np.float64)
    t = np.zeros(16, np.float32)
    _l.check(_l.lib().rsreg_umeyama_from_sums(sums.ctypes.data, t.ctypes.data))
    return _rowmajor(t)


def plane_solve_from_sums(sums, want_rank=False):
    """TransformationEstimationPointToPlaneLLS from the 32 plane sums (rsreg_plane_solve_from_sums, host only): the 4x4
    increment, with want_rank also the number of eigen-directions of AtA that carried data."""
    sums = np.ascontiguousarray(sums, np.float64)
    if sums.size != _l.NUM_PLANE_SUMS:
        raise ValueError("plane_solve_from_sums takes the 32 plane sums")
    t = np.zeros(16, np.float32)
    rank = C.c_int(0)
    _l.check(_l.lib().rsreg_plane_solve_from_sums(sums.ctypes.data, t.ctypes.data, C.byref(rank)))
    return (_rowmajor(t), rank.value) if want_rank else _rowmajor(t)
