"""Host-side mirror of the PCL `Registration` protocol the reference drives, on top of the C-ABI.

The reference calls (identically at /root/reference/src/icpslam/icp_odometer.cpp:188-201 and
src/icpslam/octree_mapper.cpp:104-117):

    icp.setMaximumIterations(ICP_MAX_ITERS); icp.setTransformationEpsilon(ICP_EPSILON);
    icp.setMaxCorrespondenceDistance(ICP_MAX_CORR_DIST); icp.setRANSACIterations(0);
    icp.setInputSource(curr); icp.setInputTarget(prev); icp.align(out);
    T = icp.getFinalTransformation(); icp.hasConverged(); icp.getFitnessScore()

`IterativeClosestPoint` below keeps those method names, argument meaning and error behaviour
(failure = hasConverged() False, never an exception on the data path) so the parity tests read like
a PCL caller.  `Context` is the thin 1:1 wrapper over include/icpgpu.h used by bench.py.
The C++ twin of this class is include/icpgpu_registration.hpp.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import IcpGpuError, Params, Profile, Rejector, Result


FPFH_BINS = 33  # ICPGPU_FPFH_BINS: pcl::FPFHSignature33
SEGMENT_RECORD = np.dtype(_lib.SegmentRecord)  # icpgpu_segment_record as a NumPy structured dtype


def _as_cloud(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("cloud must be (N, 4) float32: the pcl::PointXYZ layout x, y, z, pad")
    return a


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _colmajor16(T) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(4, 4).T).reshape(16)


FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)  # pcl::PassThrough's default limits


def crop_box_matrix(transform=None, translation=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """icpgpu_crop_box_matrix: pcl::CropBox's transform, translation and rotation (rx, ry, rz) as the ONE 4 x 4 float32 matrix
    Context.crop_box applies to a row before the box test."""
    L = _lib.load()
    out = np.zeros(16, np.float32)
    Tb = None if transform is None else _colmajor16(transform)
    tr, ro = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (translation, rotation))
    rc = L.icpgpu_crop_box_matrix(None if Tb is None else _fp(Tb), _fp(tr), _fp(ro), _fp(out))
    if rc != 0:
        raise IcpGpuError(rc, "icpgpu_crop_box_matrix")
    return out.reshape(4, 4).T.copy()


def seeded_first_row(cloud, seed: int) -> int:
    """FarthestPointSampling.setSeed's first row: the plane segmentation's generator (splitmix64 of the rule's counter, t = 0, c = 0) over
    the cloud's n rows, advanced cyclically to the next finite row; -1 when no row is finite."""
    cloud = _as_cloud(cloud)
    n = cloud.shape[0]
    if n == 0:
        return -1
    M = (1 << 64) - 1
    z = (int(seed) + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    start = ((z >> 32) * n) >> 32
    finite = np.flatnonzero(np.isfinite(cloud[:, :3]).all(axis=1))
    if finite.size == 0:
        return -1
    at = np.searchsorted(finite, start)
    return int(finite[at] if at < finite.size else finite[0])


class Context:
    """One icpgpu_ctx: one device, one HIP stream, reusable scratch."""

    def __init__(self, device_id: int = 0):
        self._L = _lib.load()
        h = C.c_void_p()
        rc = self._L.icpgpu_create(C.byref(h), int(device_id))
        if rc != 0:
            raise IcpGpuError(rc, self._L.icpgpu_last_error(None).decode())
        self._h = h
        self.n_source = 0
        self.n_target = 0
        self._scp_last = (0, 3, 0)  # (max_iterations, nr_samples, n_inliers) of the last scp_align_raw call: what scp_fetch sizes its arrays by
        self._sac_last = (0, 0)  # (n_inliers, iterations) of the last sac_segment_raw call: what sac_fetch sizes its arrays by

    def close(self):
        if getattr(self, "_h", None):
            self._L.icpgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise IcpGpuError(rc, self._L.icpgpu_last_error(self._h).decode())

    # parameters -----------------------------------------------------------------------------------------
    def default_params(self) -> Params:
        p = Params()
        self._L.icpgpu_default_params(C.byref(p))
        return p

    def get_params(self) -> Params:
        p = Params()
        self._check(self._L.icpgpu_get_params(self._h, C.byref(p)))
        return p

    def set_params(self, p: Params | None = None, **kw):
        p = p or self.get_params()
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        self._check(self._L.icpgpu_set_params(self._h, C.byref(p)))

    # inputs ----------------------------------------------------------------------------------------------
    def set_source(self, cloud):
        cloud = _as_cloud(cloud)
        self._check(self._L.icpgpu_set_source(self._h, _fp(cloud), cloud.shape[0]))
        self.n_source = cloud.shape[0]

    def set_target(self, cloud):
        cloud = _as_cloud(cloud)
        self._check(self._L.icpgpu_set_target(self._h, _fp(cloud), cloud.shape[0]))
        # the library may have recognised the context's current SOURCE in `cloud` and taken the promote path (icpgpu.h)
        ns, nt = C.c_size_t(), C.c_size_t()
        self._check(self._L.icpgpu_cloud_sizes(self._h, C.byref(ns), C.byref(nt)))
        self.n_source, self.n_target = int(ns.value), int(nt.value)

    def set_source_device(self, ptr: int, n: int):
        self._check(self._L.icpgpu_set_source_device(self._h, C.c_void_p(ptr), n))
        self.n_source = n

    def set_target_device(self, ptr: int, n: int):
        self._check(self._L.icpgpu_set_target_device(self._h, C.c_void_p(ptr), n))
        self.n_target = n

    def promote_source_to_target(self):
        self._check(self._L.icpgpu_promote_source_to_target(self._h))
        self.n_target, self.n_source = self.n_source, 0

    # the mapper's map (octree_mapper.cpp:55-90) -----------------------------------------------
    def map_set_search(self, pcl_approx: bool):
        """False: exact nearest map point (default); True: PCL's approxNearestSearch as octree_mapper.cpp:84 calls it."""
        self._check(self._L.icpgpu_map_set_search(self._h, 1 if pcl_approx else 0))

    def map_reset(self, resolution: float = 0.5):
        """resetMap(): empty one-point-per-voxel map (octree_resolution_, octree_mapper.cpp:41)."""
        self._check(self._L.icpgpu_map_reset(self._h, float(resolution)))

    def map_add_points(self, cloud, pose=None) -> int:
        """addPointsToMap(transformCloudToPoseFrame(cloud, pose)); returns the number of points appended."""
        cloud = _as_cloud(cloud)
        n = C.c_size_t()
        g = _fp(_colmajor16(pose)) if pose is not None else None
        self._check(self._L.icpgpu_map_add_points(self._h, _fp(cloud), cloud.shape[0], g, C.byref(n)))
        return int(n.value)

    def map_add_source(self, pose=None) -> int:
        n = C.c_size_t()
        g = _fp(_colmajor16(pose)) if pose is not None else None
        self._check(self._L.icpgpu_map_add_source(self._h, g, C.byref(n)))
        return int(n.value)

    def map_size(self) -> int:
        n = C.c_size_t()
        self._check(self._L.icpgpu_map_size(self._h, C.byref(n)))
        return int(n.value)

    def map_points(self) -> np.ndarray:
        n = self.map_size()
        out = np.empty((n, 4), np.float32)
        m = C.c_size_t()
        self._check(self._L.icpgpu_map_get_points(self._h, _fp(out) if n else None, n, C.byref(m)))
        return out

    def map_nn_target(self, pose, pose_inv, want_cloud: bool = True):
        """approxNearestNeighbors(cloud_in_map) moved by pose_inv becomes the target (exact NN); returns the nn cloud."""
        out = np.empty((self.n_source, 4), np.float32) if want_cloud else None
        n = C.c_size_t()
        self._check(self._L.icpgpu_map_nn_target(self._h, _fp(_colmajor16(pose)), _fp(_colmajor16(pose_inv)),
                                                 _fp(out) if out is not None and self.n_source else None, C.byref(n)))
        self.n_target = int(n.value)
        return out[: n.value] if out is not None else None

    # hot path ---------------------------------------------------------------------------------------------
    def align(self, guess=None, want_cloud: bool = False, want_fitness: bool = False):
        res = Result()
        g = None
        if guess is not None:
            gbuf = _colmajor16(guess)
            g = _fp(gbuf)
        out = np.empty((self.n_source, 4), np.float32) if want_cloud else None
        self._check(self._L.icpgpu_align(self._h, g, _fp(out) if out is not None else None, int(want_fitness),
                                         C.byref(res)))
        return result_dict(res, out)

    def align_view(self, guess=None, want_fitness: bool = False):
        """icpgpu_align_view: align with the aligned cloud taken from the context's staging buffer (copied here: the view lives until
        the context's next call)."""
        res = Result()
        g = None
        if guess is not None:
            gbuf = _colmajor16(guess)
            g = _fp(gbuf)
        view = C.POINTER(C.c_float)()
        n_out = C.c_size_t()
        self._check(self._L.icpgpu_align_view(self._h, g, int(want_fitness), C.byref(res), C.byref(view), C.byref(n_out)))
        out = np.ctypeslib.as_array(view, shape=(n_out.value, 4)).copy() if n_out.value else np.empty((0, 4), np.float32)
        return result_dict(res, out)

    def fitness(self, max_range: float = float(np.finfo(np.float64).max)) -> float:
        v = C.c_double()
        self._check(self._L.icpgpu_fitness(self._h, float(max_range), C.byref(v)))
        return v.value

    def align_batch(self, sources, targets, want_fitness: bool = False):
        n = len(sources)
        srcs = [_as_cloud(s) for s in sources]
        tgts = [_as_cloud(t) for t in targets]
        FP = C.POINTER(C.c_float)
        sp = (FP * n)(*[_fp(s) for s in srcs])
        tp = (FP * n)(*[_fp(t) for t in tgts])
        ns = (C.c_size_t * n)(*[s.shape[0] for s in srcs])
        nt = (C.c_size_t * n)(*[t.shape[0] for t in tgts])
        res = (Result * n)()
        self._check(self._L.icpgpu_align_batch(self._h, n, sp, ns, tp, nt, int(want_fitness), res))
        return [result_dict(r, None) for r in res]

    # correspondence rejectors (pcl::Registration::addCorrespondenceRejector) ------------------------------------------
    def set_correspondence_rejectors(self, chain=()):
        """The context's chain, in order: (kind, value[, min_correspondences]) tuples or _lib.Rejector structs; () clears it."""
        items = []
        for r in chain:
            if not isinstance(r, Rejector):
                r = tuple(r)
                r = Rejector(int(r[0]), int(r[2]) if len(r) > 2 else 0, float(r[1]) if len(r) > 1 else 0.0)
            items.append(r)
        arr = (Rejector * max(1, len(items)))(*items)
        self._check(self._L.icpgpu_set_correspondence_rejectors(self._h, arr, len(items)))

    def get_correspondence_rejectors(self):
        arr = (Rejector * _lib.MAX_REJECTORS)()
        n = C.c_size_t(0)
        self._check(self._L.icpgpu_get_correspondence_rejectors(self._h, arr, C.byref(n)))
        return [(int(r.kind), float(r.value), int(r.min_correspondences)) for r in arr[:n.value]]

    def correspondences(self, T=np.eye(4)):
        """What one iteration at T hands to the solve: (idx, d2) per source point, idx = -1 where the gate, the reciprocal test or
        the chain removed the pair."""
        idx = np.empty(self.n_source, np.int32)
        d2 = np.empty(self.n_source, np.float32)
        Tb = _colmajor16(T)
        self._check(self._L.icpgpu_correspondences(self._h, _fp(Tb), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fp(d2)))
        return idx, d2

    def rejector_stats(self):
        """Per stage of the chain's last run: dict(pairs_in, pairs_out, cut) (cut: float32 d2)."""
        cap = _lib.MAX_REJECTORS
        a, b = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        cut = np.zeros(cap, np.float32)
        n = C.c_size_t(0)
        u32 = C.POINTER(C.c_uint32)
        self._check(self._L.icpgpu_rejector_stats(self._h, cap, a.ctypes.data_as(u32), b.ctypes.data_as(u32), _fp(cut), C.byref(n)))
        return [dict(pairs_in=int(a[s]), pairs_out=int(b[s]), cut=np.float32(cut[s])) for s in range(n.value)]

    # the sample-consensus rejector (pcl::registration::CorrespondenceRejectorSampleConsensus) --------------------------
    def set_rejector_sac_seed(self, seed: int):
        """The seed of the chain's sample-consensus stages (default 12345), used afresh in every iteration."""
        self._check(self._L.icpgpu_set_rejector_sac_seed(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1))))

    def get_rejector_sac_seed(self) -> int:
        v = C.c_uint64(0)
        self._check(self._L.icpgpu_get_rejector_sac_seed(self._h, C.byref(v)))
        return int(v.value)

    def reject_sample_consensus(self, source, target, index_query, index_match, inlier_threshold: float = 0.05, max_iterations: int = 1000,
                                seed: int = 12345, want_flags: bool = True) -> dict:
        """RANSAC over the pairs (source[index_query[r]], target[index_match[r]]): dict(kept (bool per pair, or None), n_kept,
        best_T (4x4, getBestTransformation())).  Everything else of the run: rejector_sac_fetch()."""
        src, tgt = _as_cloud(source), _as_cloud(target)
        iq = np.ascontiguousarray(index_query, dtype=np.int32).reshape(-1)
        im = np.ascontiguousarray(index_match, dtype=np.int32).reshape(-1)
        if iq.size != im.size:
            raise ValueError("index_query and index_match must have the same length")
        ip = C.POINTER(C.c_int32)
        kept = np.zeros(max(1, iq.size), np.int32) if want_flags else None
        n_kept = C.c_size_t(0)
        T = np.zeros(16, np.float32)
        self._check(self._L.icpgpu_correspondence_rejector_sample_consensus(
            self._h, _fp(src), len(src), _fp(tgt), len(tgt), iq.ctypes.data_as(ip), im.ctypes.data_as(ip), iq.size, float(inlier_threshold),
            int(max_iterations), C.c_uint64(int(seed) & (2 ** 64 - 1)), kept.ctypes.data_as(ip) if want_flags else None, C.byref(n_kept), _fp(T)))
        return dict(kept=kept[:iq.size].astype(bool) if want_flags else None, n_kept=int(n_kept.value), best_T=T.reshape(4, 4).T.copy())

    def rejector_sac_fetch(self, per_hypothesis: bool = True) -> dict:
        """The last run of the sample-consensus core on this context (the call, correspondences(), or the last iteration of the last
        alignment with such a stage): m, sample_d2, moments9, iterations, status, counts, ranks (iterations x 3), transforms
        (iterations x 4 x 4), best_t, best_T, n_kept, host_waits."""
        ip = C.POINTER(C.c_int32)
        m, it, status, best_t, waits = (C.c_int32(0) for _ in range(5))
        d2 = C.c_double(0.0)
        mom = np.zeros(9, np.float64)
        T = np.zeros(16, np.float32)
        n_kept = C.c_size_t(0)
        dp = C.POINTER(C.c_double)
        self._check(self._L.icpgpu_rejector_sac_fetch(self._h, 0, C.byref(m), C.byref(d2), mom.ctypes.data_as(dp), C.byref(it), C.byref(status), None,
                                                      None, None, C.byref(best_t), _fp(T), C.byref(n_kept), C.byref(waits)))
        out = dict(m=int(m.value), sample_d2=float(d2.value), moments9=mom, iterations=int(it.value), status=int(status.value),
                   best_t=int(best_t.value), best_T=T.reshape(4, 4).T.copy(), n_kept=int(n_kept.value), host_waits=int(waits.value))
        if per_hypothesis:
            n = out["iterations"]
            counts = np.zeros(max(1, n), np.int32)
            ranks = np.zeros((max(1, n), 3), np.int32)
            tr = np.zeros((max(1, n), 16), np.float32)
            self._check(self._L.icpgpu_rejector_sac_fetch(self._h, n, None, None, None, None, None, counts.ctypes.data_as(ip), ranks.ctypes.data_as(ip),
                                                          _fp(tr), None, None, None, None))
            out.update(counts=counts[:n], ranks=ranks[:n], transforms=tr[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy())
        return out

    # reciprocal correspondences (pcl::Registration::setUseReciprocalCorrespondences) -----------------------------------
    def set_reciprocal_correspondences(self, on: bool):
        """P2P_SVD / P2PLANE: keep a pair only if the target point's nearest transformed source point is the pair's own (the
        lowest source index among equally near ones); in front of the rejector chain.  GICP and NDT ignore it."""
        self._check(self._L.icpgpu_set_reciprocal_correspondences(self._h, 1 if on else 0))

    def get_reciprocal_correspondences(self) -> bool:
        on = C.c_int(0)
        self._check(self._L.icpgpu_get_reciprocal_correspondences(self._h, C.byref(on)))
        return bool(on.value)

    def reciprocal_stats(self):
        """The reciprocal stage's last run: dict(pairs_in (past the gate), pairs_out (reciprocal)); zeroes when the flag was off."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.icpgpu_reciprocal_stats(self._h, C.byref(a), C.byref(b)))
        return dict(pairs_in=int(a.value), pairs_out=int(b.value))

    # kernel-level entry points ------------------------------------------------------------------------------
    def nn(self, T=np.eye(4)):
        idx = np.empty(self.n_source, np.int32)
        d2 = np.empty(self.n_source, np.float32)
        Tb = _colmajor16(T)
        self._check(self._L.icpgpu_nn(self._h, _fp(Tb), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fp(d2)))
        return idx, d2

    def reduce(self, T, max_dist: float) -> np.ndarray:
        sums = np.zeros(17, np.float64)
        Tb = _colmajor16(T)
        self._check(self._L.icpgpu_reduce(self._h, _fp(Tb), float(max_dist), sums.ctypes.data_as(C.POINTER(C.c_double))))
        return sums

    def sweep_sums(self, T=None, max_dist: float = 1.0) -> np.ndarray:
        """icpgpu_sweep_sums: the (17,) sums of one P2P_SVD sweep at T by the alignment's own path -- its opening, then what an
        iteration launches (the fused grid sweep where the grid serves max_dist); reduce()'s layout.  For tests."""
        sums = np.zeros(17, np.float64)
        Tb = None if T is None else _colmajor16(T)
        self._check(self._L.icpgpu_sweep_sums(self._h, None if Tb is None else _fp(Tb), float(max_dist),
                                              sums.ctypes.data_as(C.POINTER(C.c_double))))
        return sums

    def solve(self, sums) -> np.ndarray:
        sums = np.ascontiguousarray(sums, np.float64)
        Tk = np.zeros(16, np.float64)
        dp = C.POINTER(C.c_double)
        rc = self._L.icpgpu_solve(sums.ctypes.data_as(dp), Tk.ctypes.data_as(dp))
        if rc != 0:
            raise IcpGpuError(rc, "solve failed (n < 1 or non-finite sums)")
        return Tk.reshape(4, 4).T.copy()

    def transform(self, T) -> np.ndarray:
        out = np.empty((self.n_source, 4), np.float32)
        Tb = _colmajor16(T)
        self._check(self._L.icpgpu_transform(self._h, _fp(Tb), _fp(out)))
        return out

    def gicp_covariances(self, of_target: bool = False) -> np.ndarray:
        """(n, 3, 3) regularised neighbourhood covariances of the source (or target) cloud -- GICP row a11."""
        n = self.n_target if of_target else self.n_source
        out = np.zeros((n, 6), np.float64)
        self._check(self._L.icpgpu_gicp_covariances(self._h, int(of_target), out.ctypes.data_as(C.POINTER(C.c_double))))
        full = np.empty((n, 3, 3))
        full[:, 0, 0], full[:, 0, 1], full[:, 0, 2] = out[:, 0], out[:, 1], out[:, 2]
        full[:, 1, 0], full[:, 1, 1], full[:, 1, 2] = out[:, 1], out[:, 3], out[:, 4]
        full[:, 2, 0], full[:, 2, 1], full[:, 2, 2] = out[:, 2], out[:, 4], out[:, 5]
        return full

    # point-to-plane mode (method P2PLANE) ----------------------------------------------------------------------
    def set_target_normals(self, normals):
        """icpgpu_set_target_normals: (n_target, 4) float32 {nx, ny, nz, pad} -- the target's normals as a PointNormal cloud carries
        them (PCL's semantics exactly); dropped whenever the target changes."""
        normals = _as_cloud(normals)
        self._check(self._L.icpgpu_set_target_normals(self._h, _fp(normals), normals.shape[0]))

    def set_source_normals(self, normals):
        """icpgpu_set_source_normals: (n_source, 4) float32 {nx, ny, nz, pad} -- read by the symmetric objective and the
        surface-normal rejector; dropped whenever the source is replaced, moved to the target by promote_source_to_target()."""
        normals = _as_cloud(normals)
        self._check(self._L.icpgpu_set_source_normals(self._h, _fp(normals), normals.shape[0]))

    def set_p2plane_symmetric(self, on: bool, enforce_same_direction: bool = True):
        """icpgpu_set_p2plane_symmetric: setUseSymmetricObjective / setEnforceSameDirectionNormals of the P2PLANE method."""
        self._check(self._L.icpgpu_set_p2plane_symmetric(self._h, int(bool(on)), int(bool(enforce_same_direction))))

    def get_p2plane_symmetric(self) -> tuple:
        """(on, enforce_same_direction)"""
        on, enforce = C.c_int(0), C.c_int(0)
        self._check(self._L.icpgpu_get_p2plane_symmetric(self._h, C.byref(on), C.byref(enforce)))
        return bool(on.value), bool(enforce.value)

    def reduce_symmetric_point_to_plane(self, T, max_dist: float, enforce_same_direction: bool = True) -> np.ndarray:
        """icpgpu_reduce_symmetric_point_to_plane over the last nn() sweep: (29,) float64 in reduce_point_to_plane's layout over
        v = ((p + q) x n, n), r = (q - p) . n."""
        sums = np.zeros(29, np.float64)
        Tb = _colmajor16(T)
        self._check(self._L.icpgpu_reduce_symmetric_point_to_plane(self._h, _fp(Tb), float(max_dist), int(bool(enforce_same_direction)),
                                                                   sums.ctypes.data_as(C.POINTER(C.c_double))))
        return sums

    def solve_symmetric_point_to_plane(self, sums):
        """icpgpu_solve_symmetric_point_to_plane: the 4x4 incremental transform R Tr R from the 29 sums, or None when singular."""
        return solve_symmetric_point_to_plane(sums)

    def normals(self, of_target: bool = True) -> np.ndarray:
        """(n, 4) float32: the normals the point-to-plane mode uses for the target or the source (the caller's, else
        estimated); NaN rows for points without a neighbourhood (include/icpgpu.h, ICPGPU_P2PLANE)."""
        n = self.n_target if of_target else self.n_source
        out = np.zeros((n, 4), np.float32)
        self._check(self._L.icpgpu_normals(self._h, int(of_target), _fp(out) if n else None))
        return out

    def reduce_point_to_plane(self, T, max_dist: float) -> np.ndarray:
        """icpgpu_reduce_point_to_plane over the last nn() sweep: (29,) float64 = n, sum d2, the 21 upper-triangle entries of A^T A
        over (a, b, c, nx, ny, nz), the 6 of A^T r."""
        sums = np.zeros(29, np.float64)
        Tb = _colmajor16(T)
        self._check(self._L.icpgpu_reduce_point_to_plane(self._h, _fp(Tb), float(max_dist), sums.ctypes.data_as(C.POINTER(C.c_double))))
        return sums

    def solve_point_to_plane(self, sums):
        """icpgpu_solve_point_to_plane: the 4x4 incremental transform from the 29 sums, or None for a singular system."""
        return solve_point_to_plane(sums)

    # NDT mode (method NDT) -------------------------------------------------------------------------------------
    def set_ndt_params(self, resolution: float = 1.0, step_size: float = 0.1, outlier_ratio: float = 0.55, line_search: int | None = None):
        """icpgpu_set_ndt_params: setResolution / setStepSize / setOulierRatio (PCL's defaults); line_search (None: unchanged) =
        icpgpu_set_ndt_line_search's mode, NDT_LINE_SEARCH_PCL18 or NDT_LINE_SEARCH_MORE_THUENTE."""
        self._check(self._L.icpgpu_set_ndt_params(self._h, float(resolution), float(step_size), float(outlier_ratio)))
        if line_search is not None:
            self.set_ndt_line_search(line_search)

    def set_ndt_line_search(self, mode: int):
        """icpgpu_set_ndt_line_search: the NDT step rule, NDT_LINE_SEARCH_PCL18 (default) or NDT_LINE_SEARCH_MORE_THUENTE."""
        self._check(self._L.icpgpu_set_ndt_line_search(self._h, int(mode)))

    def get_ndt_line_search(self) -> int:
        v = C.c_int32()
        self._check(self._L.icpgpu_get_ndt_line_search(self._h, C.byref(v)))
        return v.value

    def ndt_gradient(self, p) -> np.ndarray:
        """icpgpu_ndt_gradient: the line search's trial pass at p -- (8,) float64 = pairs, score, gradient (6), the bits of
        ndt_derivatives(p)[:8]."""
        p = np.ascontiguousarray(p, np.float64).reshape(6)
        sums = np.zeros(8, np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._L.icpgpu_ndt_gradient(self._h, p.ctypes.data_as(dp), sums.ctypes.data_as(dp)))
        return sums

    def ndt_line_search_trace(self) -> dict:
        """icpgpu_ndt_line_search_trace: the last NDT alignment's More-Thuente trials -- iteration (n,) int32, step, phi, d_phi (n,)."""
        n = C.c_size_t()
        self._check(self._L.icpgpu_ndt_line_search_trace(self._h, 0, None, None, None, None, C.byref(n)))
        k = n.value
        it = np.zeros(k, np.int32)
        a, phi, dphi = (np.zeros(k, np.float64) for _ in range(3))
        dp = C.POINTER(C.c_double)
        self._check(self._L.icpgpu_ndt_line_search_trace(self._h, k, it.ctypes.data_as(C.POINTER(C.c_int32)), a.ctypes.data_as(dp),
                                                         phi.ctypes.data_as(dp), dphi.ctypes.data_as(dp), C.byref(n)))
        return dict(iteration=it, step=a, phi=phi, d_phi=dphi)

    def get_ndt_params(self) -> dict:
        v = [C.c_double(), C.c_double(), C.c_double()]
        self._check(self._L.icpgpu_get_ndt_params(self._h, *[C.byref(x) for x in v]))
        return dict(resolution=v[0].value, step_size=v[1].value, outlier_ratio=v[2].value)

    def ndt_transformation_probability(self) -> float:
        """getTransformationProbability(): the last NDT alignment's score / the number of source points."""
        out = C.c_double()
        self._check(self._L.icpgpu_ndt_transformation_probability(self._h, C.byref(out)))
        return out.value

    def ndt_cells(self) -> dict:
        """icpgpu_ndt_cells: the target's valid NDT cells in key order -- centroid (n, 4) float32, mean (n, 3), icov (n, 3, 3),
        n_points (n,) int32."""
        n = C.c_size_t()
        self._check(self._L.icpgpu_ndt_cells(self._h, 0, None, None, None, None, C.byref(n)))
        k = n.value
        cent = np.zeros((k, 4), np.float32)
        mean = np.zeros((k, 3), np.float64)
        ic6 = np.zeros((k, 6), np.float64)
        npts = np.zeros(k, np.int32)
        dp = C.POINTER(C.c_double)
        self._check(self._L.icpgpu_ndt_cells(self._h, k, _fp(cent), mean.ctypes.data_as(dp), ic6.ctypes.data_as(dp),
                                             npts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        icov = ic6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(k, 3, 3)
        return dict(centroid=cent, mean=mean, icov=icov, n_points=npts)

    def ndt_derivatives(self, p) -> np.ndarray:
        """icpgpu_ndt_derivatives: (29,) float64 = pairs, score, gradient (6), Hessian upper triangle row by row (21) at
        p = (tx, ty, tz, roll, pitch, yaw)."""
        p = np.ascontiguousarray(p, np.float64).reshape(6)
        sums = np.zeros(29, np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._L.icpgpu_ndt_derivatives(self._h, p.ctypes.data_as(dp), sums.ctypes.data_as(dp)))
        return sums

    def gicp_quadratic_sums(self, T=None) -> np.ndarray:
        """(75, 2) the sums of GICP's quadratic inner objective at transform T as (hi, lo) pairs (icp_gicp_quadratic.h) -- the
        device half of params.gicp_inner = GICP_INNER_QUADRATIC, for tests."""
        out = np.zeros((75, 2), np.float64)
        Tb = None if T is None else _colmajor16(T)
        self._check(self._L.icpgpu_gicp_quadratic_sums(self._h, None if Tb is None else _fp(Tb), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # the step before the path (icp_odometer.cpp:96-101) ---------------------------------------------------------
    def voxel_grid(self, cloud, leaf: float) -> np.ndarray:
        cloud = _as_cloud(cloud)
        out = np.empty_like(cloud)
        n_out = C.c_size_t()
        self._check(self._L.icpgpu_voxel_grid(self._h, _fp(cloud), cloud.shape[0], float(leaf), _fp(out), C.byref(n_out)))
        return out[: n_out.value].copy()

    def voxel_grid_view(self, cloud, leaf: float) -> np.ndarray:
        """icpgpu_voxel_grid_view: the filtered cloud copied out of the context's staging buffer (one host copy; the view itself is
        only valid until the context's next call)."""
        cloud = _as_cloud(cloud)
        view = C.POINTER(C.c_float)()
        n_out = C.c_size_t()
        self._check(self._L.icpgpu_voxel_grid_view(self._h, _fp(cloud), cloud.shape[0], float(leaf), C.byref(view), C.byref(n_out)))
        if n_out.value == 0:
            return np.empty((0, 4), np.float32)
        return np.ctypeslib.as_array(view, shape=(n_out.value, 4)).copy()

    def set_source_voxel_filtered(self, cloud, leaf: float) -> int:
        cloud = _as_cloud(cloud)
        n_out = C.c_size_t()
        self._check(self._L.icpgpu_set_source_voxel_filtered(self._h, _fp(cloud), cloud.shape[0], float(leaf), C.byref(n_out)))
        self.n_source = int(n_out.value)
        return self.n_source

    # outlier removal (pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval; rules: include/icpgpu.h) -------------
    def _outlier(self, view: bool, fn, cloud, *args) -> np.ndarray:
        cloud = _as_cloud(cloud)
        n_out = C.c_size_t()
        if view:
            ptr = C.POINTER(C.c_float)()
            self._check(fn(self._h, _fp(cloud), cloud.shape[0], *args, C.byref(ptr), C.byref(n_out)))
            if n_out.value == 0:
                return np.empty((0, 4), np.float32)
            return np.ctypeslib.as_array(ptr, shape=(n_out.value, 4)).copy()
        out = np.empty_like(cloud)
        self._check(fn(self._h, _fp(cloud), cloud.shape[0], *args, _fp(out), C.byref(n_out)))
        return out[: n_out.value].copy()

    def statistical_outlier_removal(self, cloud, mean_k: int, stddev_mult: float, negative: bool = False, view: bool = False) -> np.ndarray:
        """The kept points in input order (view: through icpgpu_statistical_outlier_removal_view, copied out of the staging buffer)."""
        fn = self._L.icpgpu_statistical_outlier_removal_view if view else self._L.icpgpu_statistical_outlier_removal
        return self._outlier(view, fn, cloud, int(mean_k), float(stddev_mult), int(bool(negative)))

    def radius_outlier_removal(self, cloud, radius: float, min_pts: int, negative: bool = False, view: bool = False) -> np.ndarray:
        fn = self._L.icpgpu_radius_outlier_removal_view if view else self._L.icpgpu_radius_outlier_removal
        return self._outlier(view, fn, cloud, float(radius), int(min_pts), int(bool(negative)))

    def outlier_stats(self) -> dict:
        """mean, stddev, threshold (float64) and n_valid of the context's last statistical filter call."""
        m, s, t, nv = C.c_double(), C.c_double(), C.c_double(), C.c_size_t()
        self._check(self._L.icpgpu_outlier_stats(self._h, C.byref(m), C.byref(s), C.byref(t), C.byref(nv)))
        return {"mean": m.value, "stddev": s.value, "threshold": t.value, "n_valid": int(nv.value)}

    def outlier_fetch(self) -> dict:
        """The last outlier filter call's measure per input point (SOR: dist; ROR: k as float32) and the kept / removed indices."""
        n_in, n_kept = C.c_size_t(), C.c_size_t()
        self._check(self._L.icpgpu_outlier_fetch(self._h, 0, None, None, C.byref(n_in), C.byref(n_kept)))  # (both NULL: the sizes alone)
        measure = np.zeros(n_in.value, np.float32)
        kept = np.zeros(n_kept.value, np.int32)
        self._check(self._L.icpgpu_outlier_fetch(self._h, n_in.value, _fp(measure), kept.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_in),
                                                 C.byref(n_kept)))
        mask = np.ones(n_in.value, bool)
        mask[kept] = False
        return {"measure": measure, "kept": kept, "removed": np.flatnonzero(mask).astype(np.int32)}

    # cropping and sampling filters (pcl::PassThrough / CropBox / UniformSampling / FarthestPointSampling; rules: include/icpgpu.h) ----
    def pass_through(self, cloud, field: int = -1, lo: float = FLT_MIN, hi: float = FLT_MAX, negative: bool = False, view: bool = False) -> np.ndarray:
        """The kept rows in input order.  field: 0, 1, 2 = x, y, z; -1 = none (only the non-finite rows go)."""
        fn = self._L.icpgpu_pass_through_view if view else self._L.icpgpu_pass_through
        return self._outlier(view, fn, cloud, int(field), float(lo), float(hi), int(bool(negative)))

    def crop_box(self, cloud, min3, max3, T=None, negative: bool = False, view: bool = False) -> np.ndarray:
        """The kept rows in input order.  T: a 4 x 4 matrix applied to every row before the box test (crop_box_matrix makes PCL's), or None."""
        fn = self._L.icpgpu_crop_box_view if view else self._L.icpgpu_crop_box
        mn, mx = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (min3, max3))
        Tb = None if T is None else _colmajor16(T)
        return self._outlier(view, fn, cloud, _fp(mn), _fp(mx), None if Tb is None else _fp(Tb), int(bool(negative)))

    def uniform_sampling(self, cloud, leaf: float, view: bool = False) -> np.ndarray:
        """One input row per occupied cell of side `leaf`, the one closest to the cell's centre, in input order."""
        fn = self._L.icpgpu_uniform_sampling_view if view else self._L.icpgpu_uniform_sampling
        return self._outlier(view, fn, cloud, float(leaf))

    def farthest_point_sampling(self, cloud, n_samples: int, first_index: int = -1, view: bool = False) -> np.ndarray:
        """n_samples input rows in selection order, from row first_index (-1: the lowest finite row)."""
        fn = self._L.icpgpu_farthest_point_sampling_view if view else self._L.icpgpu_farthest_point_sampling
        return self._outlier(view, fn, cloud, int(n_samples), int(first_index))

    def subset_fetch_raw(self, capacity: int, want=("kept", "measure")) -> tuple:
        """icpgpu_subset_fetch as it is: (rc, kept, measure, n_in, n_kept) with arrays of `capacity` entries (None where not wanted)."""
        kept = np.full(capacity, -1, np.int32) if "kept" in want else None
        measure = np.full(capacity, -1.0, np.float32) if "measure" in want else None
        n_in, n_kept = C.c_size_t(), C.c_size_t()
        rc = self._L.icpgpu_subset_fetch(self._h, int(capacity), None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int32)),
                                         None if measure is None else _fp(measure), C.byref(n_in), C.byref(n_kept))
        return rc, kept, measure, int(n_in.value), int(n_kept.value)

    def subset_removed_raw(self, capacity: int, want: bool = True) -> tuple:
        """icpgpu_subset_removed as it is: (rc, removed, n_removed)."""
        removed = np.full(capacity, -1, np.int32) if want else None
        n_removed = C.c_size_t()
        rc = self._L.icpgpu_subset_removed(self._h, int(capacity), None if removed is None else removed.ctypes.data_as(C.POINTER(C.c_int32)),
                                           C.byref(n_removed))
        return rc, removed, int(n_removed.value)

    def subset_fetch(self) -> dict:
        """The last cropping or sampling call's kept indices (ascending; farthest point sampling: selection order), the removed ones
        (ascending), one measure per kept row and the input's size."""
        rc, _, _, n_in, n_kept = self.subset_fetch_raw(0, want=())
        self._check(rc)
        rc, kept, measure, _, _ = self.subset_fetch_raw(n_kept)
        self._check(rc)
        rc, removed, _ = self.subset_removed_raw(n_in - n_kept)
        self._check(rc)
        return {"kept": kept, "removed": removed, "measure": measure, "n_in": n_in}

    def subset_stats(self) -> dict:
        v = [C.c_int32() for _ in range(4)]
        self._check(self._L.icpgpu_subset_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("kind", "host_waits", "launches", "path"), (int(x.value) for x in v)))

    # neighbour search (pcl::search::KdTree / pcl::KdTreeFLANN; rules: include/icpgpu.h) --------------------------------
    def search_set_input(self, cloud) -> None:
        """setInputCloud: the context's search cloud (its own buffer and k-NN grid, apart from source, target and the filters)."""
        cloud = _as_cloud(cloud)
        self._check(self._L.icpgpu_search_set_input(self._h, _fp(cloud), cloud.shape[0]))

    def search_size(self) -> tuple:
        """(points, finite points) of the search cloud."""
        n, nf = C.c_size_t(), C.c_size_t()
        self._check(self._L.icpgpu_search_size(self._h, C.byref(n), C.byref(nf)))
        return int(n.value), int(nf.value)

    def _search_queries(self, queries, n_q):
        if queries is None:
            return None, (self.search_size()[0] if n_q is None else int(n_q))
        queries = _as_cloud(queries)
        return queries, queries.shape[0]

    def search_knn(self, queries, k: int, n_q: int | None = None):
        """(idx (n_q, k) int32, d2 (n_q, k) float32, n_found (n_q,) int32): every query's k nearest cloud points, ascending by
        (d2, index), padded with -1 / +inf.  queries None: the search cloud's own points (n_q: only to test the refusal)."""
        queries, n_q = self._search_queries(queries, n_q)
        kk = max(int(k), 0)
        idx = np.empty((n_q, kk), np.int32)
        d2 = np.empty((n_q, kk), np.float32)
        n_found = np.empty(n_q, np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self._L.icpgpu_search_knn(self._h, None if queries is None else _fp(queries), n_q, int(k), idx.ctypes.data_as(ip), _fp(d2),
                                              n_found.ctypes.data_as(ip)))
        return idx, d2, n_found

    def search_radius_raw(self, queries, radius: float, max_nn: int, capacity: int, n_q: int | None = None):
        """One icpgpu_search_radius call with room for `capacity` neighbours: (rc, row_start, idx, d2, n_total); rc is the status
        code (ERR_INVALID_ARG when the rows did not fit: row_start and n_total are valid, idx / d2 untouched)."""
        queries, n_q = self._search_queries(queries, n_q)
        row_start = np.full(n_q + 1, -1, np.int64)
        idx = np.full(capacity, -2, np.int32)
        d2 = np.full(capacity, np.nan, np.float32)
        n_total = C.c_size_t()
        rc = self._L.icpgpu_search_radius(self._h, None if queries is None else _fp(queries), n_q, float(radius), int(max_nn), int(capacity),
                                          row_start.ctypes.data_as(C.POINTER(C.c_int64)), idx.ctypes.data_as(C.POINTER(C.c_int32)) if capacity else None,
                                          _fp(d2) if capacity else None, C.byref(n_total))
        return rc, row_start, idx, d2, int(n_total.value)

    def search_radius(self, queries, radius: float, max_nn: int = 0, n_q: int | None = None):
        """(row_start (n_q + 1,) int64, idx, d2): CSR rows of every query's neighbours with d2 < float32(radius^2), ascending by
        (d2, index), at most max_nn each when max_nn > 0.  Two calls: the first sizes the arrays."""
        rc, row_start, idx, d2, total = self.search_radius_raw(queries, radius, max_nn, 0, n_q)
        if rc == 0 or rc != _lib.ERR_INVALID_ARG or total == 0:
            self._check(rc)
            return row_start, idx, d2
        rc, row_start, idx, d2, total = self.search_radius_raw(queries, radius, max_nn, total, n_q)
        self._check(rc)
        return row_start, idx, d2

    # normal estimation (pcl::NormalEstimation; rules: include/icpgpu.h) ------------------------------------------------
    def normal_estimation(self, queries, k: int = 0, radius: float = 0.0, viewpoint=(0.0, 0.0, 0.0), want_moments: bool = False,
                          n_q: int | None = None):
        """(normals (n_q, 4) float32 {nx, ny, nz, curvature}, n_neighbours (n_q,) int32[, moments (n_q, 9) float32]): the surface
        normal of every query from its k nearest points of the search cloud, or from those within `radius` (exactly one of the
        two), turned towards `viewpoint`; NaN rows where fewer than three neighbours were found.  queries None: the search cloud's
        own points (n_q: only to test the refusal)."""
        queries, n_q = self._search_queries(queries, n_q)
        normals = np.empty((n_q, 4), np.float32)
        count = np.empty(n_q, np.int32)
        moments = np.empty((n_q, 9), np.float32) if want_moments else None
        vp = None if viewpoint is None else np.ascontiguousarray(np.asarray(viewpoint, np.float32).reshape(3))
        self._check(self._L.icpgpu_normal_estimation(self._h, None if queries is None else _fp(queries), n_q, int(k), float(radius),
                                                     None if vp is None else _fp(vp), _fp(normals), count.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     None if moments is None else _fp(moments)))
        return (normals, count, moments) if want_moments else (normals, count)

    # fast point feature histograms (pcl::FPFHEstimation; rules: include/icpgpu.h) ---------------------------------------
    def fpfh_estimation(self, normals, queries, k: int = 0, radius: float = 0.0, want_spfh: bool = False, n_q: int | None = None):
        """(fpfh (n_q, 33) float32, n_neighbours (n_q,) int32[, spfh (n, 33) float32]): pcl::FPFHSignature33 of every query from its
        k nearest points of the search cloud, or from those within `radius` (exactly one of the two).  normals: the search cloud's,
        (n, 4) float32 as normal_estimation returns them.  queries None: the search cloud's own points (n_q: only to test the
        refusal).  NaN rows for non-finite queries."""
        queries, n_q = self._search_queries(queries, n_q)
        n = self.search_size()[0]
        if normals is not None:
            normals = _as_cloud(normals)
        fpfh = np.empty((n_q, FPFH_BINS), np.float32)
        count = np.empty(n_q, np.int32)
        spfh = np.empty((n, FPFH_BINS), np.float32) if want_spfh else None
        self._check(self._L.icpgpu_fpfh_estimation(self._h, None if normals is None else _fp(normals), None if queries is None else _fp(queries), n_q,
                                                   int(k), float(radius), _fp(fpfh), count.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   None if spfh is None else _fp(spfh)))
        return (fpfh, count, spfh) if want_spfh else (fpfh, count)

    # boundary estimation (pcl::BoundaryEstimation; rules: include/icpgpu.h) ---------------------------------------------
    def boundary_estimation_raw(self, normals, queries, k: int = 0, radius: float = 0.0, angle_threshold: float = math.pi / 2,
                                n_q: int | None = None, want=("n_neighbours", "n_directions", "witness")) -> tuple:
        """One icpgpu_boundary_estimation call into arrays pre-filled with 0xFE / -2: (rc, dict of boundary and the outputs named in
        `want`; the others get NULL).  normals / queries may be None and n_q given (only to test the refusals)."""
        queries, n_q = self._search_queries(queries, n_q)
        if normals is not None:
            normals = _as_cloud(normals)
        out = {"boundary": np.full(n_q, 0xFE, np.uint8)}
        out.update({name: np.full(n_q, -2, np.int32) for name in ("n_neighbours", "n_directions", "witness") if name in want})
        ip = C.POINTER(C.c_int32)

        def ptr(name):
            return out[name].ctypes.data_as(ip) if name in out else None

        rc = self._L.icpgpu_boundary_estimation(self._h, None if normals is None else _fp(normals), None if queries is None else _fp(queries), n_q,
                                                int(k), float(radius), float(angle_threshold), out["boundary"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                                ptr("n_neighbours"), ptr("n_directions"), ptr("witness"))
        return rc, out

    def boundary_estimation(self, normals, queries, k: int = 0, radius: float = 0.0, angle_threshold: float = math.pi / 2,
                            n_q: int | None = None) -> dict:
        """dict(boundary (n_q,) uint8, n_neighbours, n_directions, witness (n_q,) int32): which queries lie on the rim of the search
        cloud's surface, from their k nearest points of the search cloud or from those within `radius` (exactly one of the two).
        normals: the QUERIES' normals, (n_q, 4) float32 as normal_estimation returns them.  queries None: the search cloud's own
        points.  witness: the lowest cloud index among the neighbours whose sector of `angle_threshold` radians is empty, else -1."""
        rc, out = self.boundary_estimation_raw(normals, queries, k, radius, angle_threshold, n_q)
        self._check(rc)
        return out

    # feature-space k-nearest (pcl::KdTreeFLANN<FPFHSignature33>; rules: include/icpgpu.h) --------------------------------------
    def feature_knn_raw(self, target_feat, query_feat, k: int, n_t: int | None = None, n_q: int | None = None) -> tuple:
        """One icpgpu_feature_knn call into arrays pre-filled with -2 / NaN: (rc, idx, d2, n_found).  target_feat / query_feat may be
        None and n_t / n_q given (only to test the refusals)."""
        tf = None if target_feat is None else np.ascontiguousarray(target_feat, np.float32).reshape(-1, FPFH_BINS)
        qf = None if query_feat is None else np.ascontiguousarray(query_feat, np.float32).reshape(-1, FPFH_BINS)
        n_t = (0 if tf is None else tf.shape[0]) if n_t is None else int(n_t)
        n_q = (0 if qf is None else qf.shape[0]) if n_q is None else int(n_q)
        kk = max(int(k), 0)
        idx = np.full((n_q, kk), -2, np.int32)
        d2 = np.full((n_q, kk), np.nan, np.float32)
        n_found = np.full(n_q, -2, np.int32)
        ip = C.POINTER(C.c_int32)
        rc = self._L.icpgpu_feature_knn(self._h, None if tf is None else _fp(tf), n_t, None if qf is None else _fp(qf), n_q, int(k),
                                        idx.ctypes.data_as(ip), _fp(d2), n_found.ctypes.data_as(ip))
        return rc, idx, d2, n_found

    def feature_knn(self, target_feat, query_feat, k: int):
        """(idx (n_q, k) int32, d2 (n_q, k) float32, n_found (n_q,) int32): every query descriptor's k nearest target descriptors
        (rows of 33 floats, as fpfh_estimation returns them), ascending by (d2, index), padded with -1 / +inf.  Rows with a
        non-finite component are never neighbours and find nothing."""
        rc, idx, d2, n_found = self.feature_knn_raw(target_feat, query_feat, k)
        self._check(rc)
        return idx, d2, n_found

    # sample-consensus alignment (pcl::SampleConsensusPrerejective; rules: include/icpgpu.h) ------------------------------------
    def scp_align_raw(self, source, source_feat, target_feat, nr_samples: int = 3, k_correspondences: int = 2, similarity_threshold: float = 0.9,
                      max_correspondence_distance: float = 1.0, inlier_fraction: float = 0.25, max_iterations: int = 1000, seed: int = 0,
                      want_cloud: bool = True) -> tuple:
        """One icpgpu_scp_align call over the search cloud (the target): (rc, T (4, 4) float32, n_inliers, fitness, converged, aligned
        cloud or None); the result stays in the context.  source / source_feat / target_feat may be None (only to test the refusals)."""
        src = None if source is None else _as_cloud(source)
        sf = None if source_feat is None else np.ascontiguousarray(source_feat, np.float32).reshape(-1, FPFH_BINS)
        tf = None if target_feat is None else np.ascontiguousarray(target_feat, np.float32).reshape(-1, FPFH_BINS)
        n_s = 0 if src is None else src.shape[0]
        if sf is not None and sf.shape[0] != n_s:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"scp_align: {sf.shape[0]} descriptors for {n_s} source points")
        if tf is not None and tf.shape[0] != self.search_size()[0]:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"scp_align: {tf.shape[0]} descriptors for a search cloud of {self.search_size()[0]} points")
        T = np.full(16, -2, np.float32)
        out = np.full((n_s, 4), np.nan, np.float32) if want_cloud else None
        n_in, fit, conv = C.c_size_t(), C.c_float(), C.c_int32()
        rc = self._L.icpgpu_scp_align(self._h, None if src is None else _fp(src), n_s, None if sf is None else _fp(sf), None if tf is None else _fp(tf),
                                      int(nr_samples), int(k_correspondences), float(similarity_threshold), float(max_correspondence_distance),
                                      float(inlier_fraction), int(max_iterations), int(seed) & (2**64 - 1), _fp(T), C.byref(n_in), C.byref(fit),
                                      C.byref(conv), None if out is None else _fp(out))
        self._scp_last = (max(int(max_iterations), 0), int(nr_samples), int(n_in.value))
        return rc, T.reshape(4, 4).T.copy(), int(n_in.value), float(fit.value), int(conv.value), out

    def scp_fetch_raw(self, capacity_hypotheses: int, capacity_inliers: int, nr_samples: int) -> tuple:
        """One icpgpu_scp_fetch call into arrays pre-filled with -2: (rc, dict of everything the fetch hands out)."""
        ip = C.POINTER(C.c_int32)
        h, nr = int(capacity_hypotheses), int(nr_samples)
        status, counts = np.full(h, -2, np.int32), np.full(h, -2, np.int32)
        sidx, tidx = np.full((h, nr), -2, np.int32), np.full((h, nr), -2, np.int32)
        transforms = np.full((h, 16), -2, np.float32)
        sums, errors = np.full(h, -2, np.float64), np.full(h, -2, np.float32)
        inliers = np.full(int(capacity_inliers), -2, np.int32)
        best_t = C.c_int32(-2)
        rc = self._L.icpgpu_scp_fetch(self._h, h, int(capacity_inliers), status.ctypes.data_as(ip), sidx.ctypes.data_as(ip), tidx.ctypes.data_as(ip),
                                      _fp(transforms), counts.ctypes.data_as(ip), sums.ctypes.data_as(C.POINTER(C.c_double)), _fp(errors),
                                      C.byref(best_t), inliers.ctypes.data_as(ip))
        return rc, {"status": status, "source_idx": sidx, "target_idx": tidx, "transforms": transforms, "count": counts, "sum": sums, "error": errors,
                    "best_t": int(best_t.value), "inliers": inliers}

    def scp_align(self, source, source_feat, target_feat, **kw) -> dict:
        """The pose of `source` in the search cloud without a guess: dict(T (4, 4) float32, converged, fitness, inliers (ascending int32),
        cloud (the aligned source)).  Keywords as scp_align_raw."""
        rc, T, n_in, fit, conv, cloud = self.scp_align_raw(source, source_feat, target_feat, **kw)
        self._check(rc)
        inliers = np.empty(n_in, np.int32)                     # the inliers alone: no per-hypothesis array is allocated or copied
        self._check(self._L.icpgpu_scp_fetch(self._h, 0, n_in, None, None, None, None, None, None, None, None,
                                             inliers.ctypes.data_as(C.POINTER(C.c_int32))))
        return {"T": T, "converged": bool(conv), "fitness": fit, "inliers": inliers, "cloud": cloud}

    def scp_fetch(self) -> dict:
        """Everything icpgpu_scp_fetch hands out of the last alignment: per hypothesis status, source_idx, target_idx, transforms (16,
        column-major), count, sum, error; best_t and the inliers."""
        it, nr, n_in = self._scp_last
        rc, out = self.scp_fetch_raw(it, n_in, nr)
        self._check(rc)
        return out

    def scp_stats(self) -> dict:
        """host_waits, evaluated hypotheses and the host's solve time (ms) of the last alignment (icpgpu_scp_stats)."""
        w, e, ms = C.c_int32(), C.c_int32(), C.c_double()
        self._check(self._L.icpgpu_scp_stats(self._h, C.byref(w), C.byref(e), C.byref(ms)))
        return {"host_waits": int(w.value), "evaluated": int(e.value), "host_solve_ms": float(ms.value)}

    # euclidean clustering (pcl::EuclideanClusterExtraction; rules: include/icpgpu.h) --------------------------------------
    def cluster_extract_raw(self, tolerance: float, min_size: int, max_size: int) -> tuple:
        """One icpgpu_euclidean_cluster_extraction call: (rc, n_clusters, n_clustered); the result stays in the context."""
        nc, np_ = C.c_size_t(), C.c_size_t()
        rc = self._L.icpgpu_euclidean_cluster_extraction(self._h, float(tolerance), int(min_size), int(max_size), C.byref(nc), C.byref(np_))
        return rc, int(nc.value), int(np_.value)

    def cluster_fetch_raw(self, capacity_clusters: int, capacity_indices: int, want_labels: bool = True, want_component: bool = True) -> tuple:
        """One icpgpu_cluster_fetch call into arrays pre-filled with -2: (rc, cluster_start, indices, labels, component)."""
        n_c = C.c_size_t()
        self._L.icpgpu_search_size(self._h, C.byref(n_c), None)  # (0 without a search cloud)
        n = int(n_c.value)
        start = np.full(capacity_clusters + 1, -2, np.int64)
        indices = np.full(capacity_indices, -2, np.int32)
        labels = np.full(n, -2, np.int32) if want_labels else None
        component = np.full(n, -2, np.int32) if want_component else None
        ip = C.POINTER(C.c_int32)
        rc = self._L.icpgpu_cluster_fetch(self._h, int(capacity_clusters), int(capacity_indices), start.ctypes.data_as(C.POINTER(C.c_int64)),
                                          indices.ctypes.data_as(ip), None if labels is None else labels.ctypes.data_as(ip),
                                          None if component is None else component.ctypes.data_as(ip))
        return rc, start, indices, labels, component

    def euclidean_cluster_extraction(self, tolerance: float, min_size: int = 1, max_size: int = 2**31 - 1) -> tuple:
        """(cluster_start (n_clusters + 1,) int64, indices (n_clustered,) int32, labels (n,) int32, component (n,) int32): the
        connected components of the search cloud's graph d2 < float32(tolerance^2) with min_size .. max_size points, by size
        descending (the lowest index first among equal sizes), indices ascending inside a cluster; labels / component -1 where none."""
        rc, n_clusters, n_clustered = self.cluster_extract_raw(tolerance, min_size, max_size)
        self._check(rc)
        rc, start, indices, labels, component = self.cluster_fetch_raw(n_clusters, n_clustered)
        self._check(rc)
        return start, indices, labels, component

    # region growing (pcl::RegionGrowing by the order-free rule of include/icpgpu.h, "region growing") ----------------------------
    def region_growing_raw(self, normals, k: int, smoothness_cos: float, curvature_threshold: float, min_size: int, max_size: int) -> tuple:
        """One icpgpu_region_growing call: (rc, n_regions, n_in_regions); the result stays in the context.  normals: (n, 4) float32
        {nx, ny, nz, curvature} or None (a null pointer)."""
        nr, ni = C.c_size_t(), C.c_size_t()
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
        rc = self._L.icpgpu_region_growing(self._h, None if nrm is None else _fp(nrm), int(k), float(smoothness_cos), float(curvature_threshold),
                                           int(min_size), int(max_size), C.byref(nr), C.byref(ni))
        return rc, int(nr.value), int(ni.value)

    def region_fetch_raw(self, capacity_regions: int, capacity_indices: int, want=("labels", "region", "kind", "anchor")) -> tuple:
        """One icpgpu_region_fetch call into arrays pre-filled with -2: (rc, region_start, indices, labels, region, kind, anchor); the
        per-point arrays not named in `want` are passed as NULL and come back as None."""
        n_c = C.c_size_t()
        self._L.icpgpu_search_size(self._h, C.byref(n_c), None)  # (0 without a search cloud)
        n = int(n_c.value)
        start = np.full(capacity_regions + 1, -2, np.int64)
        indices = np.full(capacity_indices, -2, np.int32)
        per_point = [np.full(n, -2, np.int32) if name in want else None for name in ("labels", "region", "kind", "anchor")]
        ip = C.POINTER(C.c_int32)
        rc = self._L.icpgpu_region_fetch(self._h, int(capacity_regions), int(capacity_indices), start.ctypes.data_as(C.POINTER(C.c_int64)),
                                         indices.ctypes.data_as(ip), *[None if a is None else a.ctypes.data_as(ip) for a in per_point])
        return (rc, start, indices, *per_point)

    def region_growing(self, normals, k: int = 30, smoothness: float = math.radians(30.0), curvature_threshold: float = 0.05,
                       min_size: int = 1, max_size: int = 2**31 - 1, smoothness_cos=None) -> tuple:
        """(region_start (n_regions + 1,) int64, indices (n_in_regions,) int32, labels, region, kind, anchor (n,) int32 each): the
        search cloud's smooth regions of min_size .. max_size points by size descending (the lowest name first among equal sizes),
        indices ascending inside a region.  smoothness: PCL's theta in radians; smoothness_cos, when given, is used as it is."""
        cos = np.float32(math.cos(float(smoothness))) if smoothness_cos is None else smoothness_cos
        rc, n_regions, n_in = self.region_growing_raw(normals, k, cos, curvature_threshold, min_size, max_size)
        self._check(rc)
        rc, *arrays = self.region_fetch_raw(n_regions, n_in)
        self._check(rc)
        return tuple(arrays)

    # segment moments (pcl::MomentOfInertiaEstimation for every segment at once; rules: include/icpgpu.h, "segment moments") --------
    def segment_moments_raw(self, source: int, n_segments: int, segment_start=None, indices=None, sizeof_record=None, null_out: bool = False) -> tuple:
        """One icpgpu_segment_moments call into n_segments records pre-filled with the byte 0xAB: (rc, records).  segment_start /
        indices: int64 / int32 arrays or None (null pointers); sizeof_record: the record's size unless given; null_out: out = NULL."""
        records = np.frombuffer(bytearray(b"\xab" * (int(n_segments) * SEGMENT_RECORD.itemsize)), SEGMENT_RECORD)
        start = None if segment_start is None else np.ascontiguousarray(segment_start, np.int64)
        idx = None if indices is None else np.ascontiguousarray(indices, np.int32)
        rc = self._L.icpgpu_segment_moments(self._h, int(source), int(n_segments),
                                            None if start is None else start.ctypes.data_as(C.POINTER(C.c_int64)),
                                            None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                            SEGMENT_RECORD.itemsize if sizeof_record is None else int(sizeof_record),
                                            None if null_out or records.size == 0 else records.ctypes.data)
        return rc, records

    def segment_moments(self, segment_start=None, indices=None, source: str = "host", n_segments=None) -> np.ndarray:
        """One record per segment of the search cloud (a NumPy structured array of SEGMENT_RECORD: count, status, first, K, moments,
        centroid, cov, eigenvalues, axes, aabb_min, aabb_max, obb_lo, obb_hi, obb_position, obb_dims).  source "host": the CSR
        segment_start (n_segments + 1) / indices; "clusters" / "regions": the last euclidean_cluster_extraction / region_growing
        result over this search cloud, read where it lies on the device (n_segments: its count, checked by the library)."""
        if source == "host":
            if segment_start is None:
                raise IcpGpuError(_lib.ERR_INVALID_ARG, "segment_moments: a host source needs segment_start")
            n_seg = len(segment_start) - 1
            code = _lib.SEGMENTS_HOST
        elif source in ("clusters", "regions"):
            if segment_start is not None or indices is not None:
                raise IcpGpuError(_lib.ERR_INVALID_ARG, f"segment_moments: source {source!r} takes no segment_start or indices")
            if n_segments is None:
                raise IcpGpuError(_lib.ERR_INVALID_ARG, f"segment_moments: source {source!r} needs n_segments, the result's count")
            n_seg = int(n_segments)
            code = _lib.SEGMENTS_CLUSTERS if source == "clusters" else _lib.SEGMENTS_REGIONS
        else:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"segment_moments: unknown source {source!r}")
        rc, records = self.segment_moments_raw(code, n_seg, segment_start, indices)
        self._check(rc)
        return records

    def segment_stats(self) -> dict:
        """host_waits of the last segment_moments call (icpgpu_segment_stats)."""
        w = C.c_int32()
        self._check(self._L.icpgpu_segment_stats(self._h, C.byref(w)))
        return {"host_waits": int(w.value)}

    # ISS keypoints (pcl::ISSKeypoint3D; the _border calls with border estimation; rules: include/icpgpu.h) -------------------------
    def iss_keypoints_raw(self, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                          min_neighbors: int = 5) -> tuple:
        """One icpgpu_iss_keypoints call: (rc, n_keypoints); the result stays in the context."""
        nk = C.c_size_t()
        rc = self._L.icpgpu_iss_keypoints(self._h, float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32),
                                          int(min_neighbors), C.byref(nk))
        return rc, int(nk.value)

    def iss_fetch_raw(self, capacity_keypoints: int, want=("keypoint_index", "keypoints", "n_salient", "scatter6", "eigenvalues3", "saliency")) -> tuple:
        """One icpgpu_iss_fetch call into arrays pre-filled with -2: (rc, dict of the outputs named in `want`; the others get NULL)."""
        n_c = C.c_size_t()
        self._L.icpgpu_search_size(self._h, C.byref(n_c), None)  # (0 without a search cloud)
        n, cap = int(n_c.value), int(capacity_keypoints)
        shapes = {"keypoint_index": ((cap,), np.int32), "keypoints": ((cap, 4), np.float32), "n_salient": ((n,), np.int32),
                  "scatter6": ((n, 6), np.float64), "eigenvalues3": ((n, 3), np.float64), "saliency": ((n,), np.float64)}
        out = {name: np.full(shape, -2, dtype) for name, (shape, dtype) in shapes.items() if name in want}
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

        def ptr(name, kind):
            return out[name].ctypes.data_as(kind) if name in out else None

        rc = self._L.icpgpu_iss_fetch(self._h, cap, ptr("keypoint_index", ip), ptr("keypoints", C.POINTER(C.c_float)), ptr("n_salient", ip),
                                      ptr("scatter6", dp), ptr("eigenvalues3", dp), ptr("saliency", dp))
        return rc, out

    def iss_stats(self) -> int:
        """The host waits of the last iss_keypoints call."""
        waits = C.c_int32(-1)
        self._check(self._L.icpgpu_iss_stats(self._h, C.byref(waits)))
        return int(waits.value)

    def iss_keypoints(self, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                      min_neighbors: int = 5) -> dict:
        """The search cloud's ISS keypoints: dict(n_keypoints, keypoint_index (m,) int32 ascending, keypoints (m, 4) float32,
        n_salient (n,) int32, scatter6 (n, 6), eigenvalues3 (n, 3) descending, saliency (n,) float64)."""
        rc, m = self.iss_keypoints_raw(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
        self._check(rc)
        rc, out = self.iss_fetch_raw(m)
        self._check(rc)
        out["n_keypoints"] = m
        return out

    def iss_keypoints_border_raw(self, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                                 min_neighbors: int = 5, border_radius: float = 0.0, angle_threshold: float = math.pi / 2, normals=None,
                                 normal_radius: float = 0.0) -> tuple:
        """One icpgpu_iss_keypoints_border call: (rc, n_keypoints); the result stays in the context."""
        nk = C.c_size_t()
        if normals is not None:
            normals = _as_cloud(normals)
        rc = self._L.icpgpu_iss_keypoints_border(self._h, float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32),
                                                 int(min_neighbors), float(border_radius), float(angle_threshold),
                                                 None if normals is None else _fp(normals), float(normal_radius), C.byref(nk))
        return rc, int(nk.value)

    def iss_fetch_border_raw(self, want=("edge", "border")) -> tuple:
        """One icpgpu_iss_fetch_border call into arrays pre-filled with -2: (rc, dict of the outputs named in `want`)."""
        n_c = C.c_size_t()
        self._L.icpgpu_search_size(self._h, C.byref(n_c), None)
        out = {name: np.full(int(n_c.value), -2, np.int32) for name in ("edge", "border") if name in want}
        ip = C.POINTER(C.c_int32)
        rc = self._L.icpgpu_iss_fetch_border(self._h, out["edge"].ctypes.data_as(ip) if "edge" in out else None,
                                             out["border"].ctypes.data_as(ip) if "border" in out else None)
        return rc, out

    def iss_keypoints_border(self, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                             min_neighbors: int = 5, border_radius: float = 0.0, angle_threshold: float = math.pi / 2, normals=None,
                             normal_radius: float = 0.0) -> dict:
        """iss_keypoints with PCL's border estimation: its dict plus edge and border (n,) int32.  A point within border_radius of an
        edge point -- a boundary point of the cloud by boundary_estimation's rule over the border radius's rows -- is no keypoint.
        normals: the cloud's, (n, 4) float32, or None to have them computed from normal_radius.  border_radius 0: iss_keypoints."""
        rc, m = self.iss_keypoints_border_raw(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, border_radius, angle_threshold,
                                              normals, normal_radius)
        self._check(rc)
        rc, out = self.iss_fetch_raw(m)
        self._check(rc)
        rc, more = self.iss_fetch_border_raw()
        self._check(rc)
        out.update(more)
        out["n_keypoints"] = m
        return out

    # moving least squares (pcl::MovingLeastSquares, UpsamplingMethod NONE; rules: include/icpgpu.h) ---------------------------------
    def moving_least_squares_raw(self, queries, radius: float, order: int = 2, sqr_gauss_param: float = 0.0, n_q=None,
                                 want_normals: bool = True) -> tuple:
        """One icpgpu_moving_least_squares call into arrays of n_q entries pre-filled with -2: (rc, n_out, points (n_q, 4) float32,
        normals (n_q, 4) float32 or None, index (n_q,) int32); the per-query record stays in the context.  queries None: the search
        cloud's own points (n_q then defaults to its size)."""
        q = None if queries is None else _as_cloud(queries)
        if n_q is None and q is None:
            n_c = C.c_size_t()
            self._L.icpgpu_search_size(self._h, C.byref(n_c), None)  # (0 without a search cloud)
            n_q = n_c.value
        n_q = q.shape[0] if n_q is None else int(n_q)
        points = np.full((n_q, 4), -2, np.float32)
        normals = np.full((n_q, 4), -2, np.float32) if want_normals else None
        index = np.full(n_q, -2, np.int32)
        n_out = C.c_size_t()
        rc = self._L.icpgpu_moving_least_squares(self._h, None if q is None else _fp(q), n_q, float(radius), int(order), float(sqr_gauss_param),
                                                 _fp(points), None if normals is None else _fp(normals),
                                                 index.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_out))
        return rc, int(n_out.value), points, normals, index

    def mls_fetch_raw(self, capacity: int, want=("status", "n_neighbours", "plane7", "coeff10")) -> tuple:
        """One icpgpu_mls_fetch call into arrays of `capacity` entries pre-filled with -2: (rc, dict of the outputs named in `want`; the
        others get NULL)."""
        cap = int(capacity)
        shapes = {"status": ((cap,), np.int32), "n_neighbours": ((cap,), np.int32), "plane7": ((cap, 7), np.float64),
                  "coeff10": ((cap, 10), np.float64)}
        out = {name: np.full(shape, -2, dtype) for name, (shape, dtype) in shapes.items() if name in want}
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

        def ptr(name, kind):
            return out[name].ctypes.data_as(kind) if name in out else None

        rc = self._L.icpgpu_mls_fetch(self._h, cap, ptr("status", ip), ptr("n_neighbours", ip), ptr("plane7", dp), ptr("coeff10", dp))
        return rc, out

    def mls_stats(self) -> int:
        """The host waits of the last moving_least_squares call."""
        waits = C.c_int32(-1)
        self._check(self._L.icpgpu_mls_stats(self._h, C.byref(waits)))
        return int(waits.value)

    def moving_least_squares(self, radius: float, order: int = 2, sqr_gauss_param: float = 0.0, queries=None, want_record: bool = False):
        """The queries (None: the search cloud's own points) projected onto a polynomial of `order` fitted to their radius neighbourhood
        in the search cloud: (points (m, 4) float32, normals (m, 4) float32 {nx, ny, nz, curvature}, index (m,) int32 -- the kept
        queries, in order).  want_record: a fourth item, dict(status, n_neighbours, plane7, coeff10) per query (icpgpu_mls_fetch)."""
        rc, m, points, normals, index = self.moving_least_squares_raw(queries, radius, order, sqr_gauss_param)
        self._check(rc)
        if not want_record:
            return points[:m].copy(), normals[:m].copy(), index[:m].copy()
        rc, record = self.mls_fetch_raw(len(index))
        self._check(rc)
        return points[:m].copy(), normals[:m].copy(), index[:m].copy(), record

    # plane segmentation (pcl::SACSegmentation, pcl::ExtractIndices; rules: include/icpgpu.h) ----------------------------------
    def sac_segment_raw(self, distance_threshold: float, max_iterations: int = 50, probability: float = 0.99, seed: int = 0,
                        optimize_coefficients: bool = True, axis=None, eps_angle: float = 0.0) -> tuple:
        """One icpgpu_sac_plane_segmentation call: (rc, coefficients (4,) float32, n_inliers, iterations, found); the result stays
        in the context."""
        coeff = np.full(4, -2, np.float32)
        n_in, it, found = C.c_size_t(), C.c_int32(), C.c_int32()
        ax = None if axis is None else (C.c_double * 3)(*[float(v) for v in axis])
        rc = self._L.icpgpu_sac_plane_segmentation(self._h, float(distance_threshold), int(max_iterations), float(probability),
                                                   int(seed) & (2**64 - 1), int(bool(optimize_coefficients)), ax, float(eps_angle), _fp(coeff),
                                                   C.byref(n_in), C.byref(it), C.byref(found))
        self._sac_last = (int(n_in.value), int(it.value))
        return rc, coeff, int(n_in.value), int(it.value), int(found.value)

    def sac_fetch_raw(self, capacity_inliers: int, capacity_counts: int) -> tuple:
        """One icpgpu_sac_fetch call into arrays pre-filled with -2: (rc, dict of everything the fetch hands out)."""
        ip = C.POINTER(C.c_int32)
        inliers = np.full(capacity_inliers, -2, np.int32)
        counts = np.full(capacity_counts, -2, np.int32)
        sample = np.full(3, -2, np.int32)
        best_t, n_unref = C.c_int32(-2), C.c_size_t(0)
        coeff = np.full(4, -2, np.float32)
        moments = np.full(9, -2, np.float64)
        rc = self._L.icpgpu_sac_fetch(self._h, int(capacity_inliers), int(capacity_counts), inliers.ctypes.data_as(ip), counts.ctypes.data_as(ip),
                                      sample.ctypes.data_as(ip), C.byref(best_t), _fp(coeff), moments.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(n_unref))
        return rc, {"inliers": inliers, "counts": counts, "sample": sample, "best_t": int(best_t.value), "coeff_unrefined": coeff,
                    "moments": moments, "n_unrefined": int(n_unref.value)}

    def sac_plane_segmentation(self, distance_threshold: float, max_iterations: int = 50, probability: float = 0.99, seed: int = 0,
                               optimize_coefficients: bool = True, axis=None, eps_angle: float = 0.0) -> tuple:
        """(inliers (m,) int32 ascending, coefficients (4,) float32, iterations, found) of the dominant plane of the search cloud:
        RANSAC over counter-based samples (seed), PCL's refinement when optimize_coefficients; axis: SACMODEL_PERPENDICULAR_PLANE."""
        rc, coeff, n_in, it, found = self.sac_segment_raw(distance_threshold, max_iterations, probability, seed, optimize_coefficients, axis,
                                                          eps_angle)
        self._check(rc)
        return self.sac_fetch(n_in, it)["inliers"], coeff, it, found

    def sac_fetch(self, n_inliers: int | None = None, n_counts: int | None = None) -> dict:
        """Everything icpgpu_sac_fetch hands out of the last segmentation: inliers, counts (one per iteration), sample, best_t,
        coeff_unrefined, moments (the refinement's nine sums), n_unrefined.  Sizes that are not given are the last call's."""
        n_inliers = self._sac_last[0] if n_inliers is None else n_inliers
        n_counts = self._sac_last[1] if n_counts is None else n_counts
        rc, out = self.sac_fetch_raw(n_inliers, n_counts)
        self._check(rc)
        return out

    def sac_extract(self, negative: bool = False, view: bool = False) -> np.ndarray:
        """pcl::ExtractIndices over the last segmentation: the search cloud's points in (negative: not in) the inliers, in order."""
        n_out = C.c_size_t()
        if view:
            ptr = C.POINTER(C.c_float)()
            self._check(self._L.icpgpu_sac_extract_view(self._h, int(bool(negative)), C.byref(ptr), C.byref(n_out)))
            if n_out.value == 0:
                return np.empty((0, 4), np.float32)
            return np.ctypeslib.as_array(ptr, shape=(n_out.value, 4)).copy()
        out = np.empty((self.search_size()[0], 4), np.float32)
        self._check(self._L.icpgpu_sac_extract(self._h, int(bool(negative)), _fp(out), C.byref(n_out)))
        return out[: n_out.value].copy()

    def sac_host_waits(self) -> int:
        """The host waits of the last segmentation (icpgpu_sac_stats)."""
        w = C.c_int32()
        self._check(self._L.icpgpu_sac_stats(self._h, C.byref(w)))
        return int(w.value)

    # segmentation from normals (pcl::SACSegmentationFromNormals; rules: include/icpgpu.h) --------------------------------------
    def sac_segmentation_from_normals_raw(self, model: int, normals, distance_threshold: float, normal_distance_weight: float = 0.1,
                                          radius_min: float = 0.0, radius_max: float = 0.0, max_iterations: int = 50, probability: float = 0.99,
                                          seed: int = 0, optimize_coefficients: bool = True, axis=None, eps_angle: float = 0.0) -> tuple:
        """One icpgpu_sac_segmentation_from_normals call: (rc, coefficients (7,) float32, n_coeff, n_inliers, iterations, found); the
        result stays in the context.  normals: (n, 4) float32 rows (nx, ny, nz, curvature) of the search cloud, or None (NULL)."""
        coeff = np.full(7, -2, np.float32)
        n_in, it, found, n_coeff = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32()
        ax = None if axis is None else (C.c_double * 3)(*[float(v) for v in axis])
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32)
        rc = self._L.icpgpu_sac_segmentation_from_normals(self._h, int(model), None if nrm is None else _fp(nrm), float(distance_threshold),
                                                          float(normal_distance_weight), float(radius_min), float(radius_max), int(max_iterations),
                                                          float(probability), int(seed) & (2**64 - 1), int(bool(optimize_coefficients)), ax,
                                                          float(eps_angle), _fp(coeff), C.byref(n_coeff), C.byref(n_in), C.byref(it), C.byref(found))
        self._sac_last = (int(n_in.value), int(it.value))
        return rc, coeff, int(n_coeff.value), int(n_in.value), int(it.value), int(found.value)

    def sac_normals_fetch_raw(self, capacity_inliers: int, capacity_counts: int) -> tuple:
        """One icpgpu_sac_normals_fetch call into arrays pre-filled with -2: (rc, dict of everything the fetch hands out)."""
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        inliers = np.full(capacity_inliers, -2, np.int32)
        counts = np.full(capacity_counts, -2, np.int32)
        sample = np.full(3, -2, np.int32)
        best_t, n_unref, passes, stop = C.c_int32(-2), C.c_size_t(0), C.c_int32(-2), C.c_int32(-2)
        coeff = np.full(7, -2, np.float32)
        moments = np.full(9, -2, np.float64)
        sums = np.full((_lib.SAC_CYLINDER_ITERATIONS, 21), -2, np.float64)
        rc = self._L.icpgpu_sac_normals_fetch(self._h, int(capacity_inliers), int(capacity_counts), inliers.ctypes.data_as(ip),
                                              counts.ctypes.data_as(ip), sample.ctypes.data_as(ip), C.byref(best_t), _fp(coeff), C.byref(n_unref),
                                              moments.ctypes.data_as(dp), sums.ctypes.data_as(dp), C.byref(passes), C.byref(stop))
        return rc, {"inliers": inliers, "counts": counts, "sample": sample, "best_t": int(best_t.value), "coeff_unrefined": coeff,
                    "n_unrefined": int(n_unref.value), "moments": moments, "cylinder_sums": sums, "cylinder_passes": int(passes.value),
                    "cylinder_stop": int(stop.value)}

    def sac_segmentation_from_normals(self, model: int, normals, distance_threshold: float, normal_distance_weight: float = 0.1,
                                      radius_min: float = 0.0, radius_max: float = 0.0, max_iterations: int = 50, probability: float = 0.99,
                                      seed: int = 0, optimize_coefficients: bool = True, axis=None, eps_angle: float = 0.0) -> tuple:
        """(inliers (m,) int32 ascending, coefficients (4,) or (7,) float32, iterations, found) of the search cloud's dominant
        normal-aware plane (SACMODEL_NORMAL_PLANE) or cylinder (SACMODEL_CYLINDER: point on the axis, direction, radius)."""
        rc, coeff, n_coeff, n_in, it, found = self.sac_segmentation_from_normals_raw(model, normals, distance_threshold, normal_distance_weight,
                                                                                     radius_min, radius_max, max_iterations, probability, seed,
                                                                                     optimize_coefficients, axis, eps_angle)
        self._check(rc)
        return self.sac_normals_fetch(n_in, it)["inliers"], coeff[:n_coeff].copy(), it, found

    def sac_normals_fetch(self, n_inliers: int | None = None, n_counts: int | None = None) -> dict:
        """Everything icpgpu_sac_normals_fetch hands out of the last segmentation from normals.  Sizes that are not given are the
        last call's."""
        n_inliers = self._sac_last[0] if n_inliers is None else n_inliers
        n_counts = self._sac_last[1] if n_counts is None else n_counts
        rc, out = self.sac_normals_fetch_raw(n_inliers, n_counts)
        self._check(rc)
        return out

    def sac_normals_host_waits(self) -> int:
        """The host waits of the last segmentation from normals (icpgpu_sac_normals_stats)."""
        w = C.c_int32()
        self._check(self._L.icpgpu_sac_normals_stats(self._h, C.byref(w)))
        return int(w.value)

    # ground filter (pcl::applyMorphologicalOperator, pcl::ProgressiveMorphologicalFilter; rules: include/icpgpu.h) --------------
    def morphological_operator_raw(self, resolution: float, op: int) -> tuple:
        """One icpgpu_morphological_operator call: (rc, z (n,) float32, pre-filled with -2)."""
        n_c = C.c_size_t()
        self._L.icpgpu_search_size(self._h, C.byref(n_c), None)  # (0 without a search cloud)
        out = np.full(int(n_c.value), -2, np.float32)
        rc = self._L.icpgpu_morphological_operator(self._h, float(resolution), int(op), _fp(out))
        return rc, out

    def morphological_operator(self, resolution: float, op: int) -> np.ndarray:
        """z (n,) float32 of the search cloud after MORPH_ERODE / DILATE / OPEN / CLOSE over xy boxes of side `resolution`; non-finite
        rows keep their own z."""
        rc, out = self.morphological_operator_raw(resolution, op)
        self._check(rc)
        return out

    def pmf_filter_raw(self, max_window_size: int = 33, slope: float = 0.7, initial_distance: float = 0.15, max_distance: float = 10.0,
                       cell_size: float = 1.0, base: float = 2.0, exponential: bool = True) -> tuple:
        """One icpgpu_progressive_morphological_filter call: (rc, n_ground, n_passes); the result stays in the context."""
        n_ground, n_passes = C.c_size_t(), C.c_int32()
        rc = self._L.icpgpu_progressive_morphological_filter(self._h, int(max_window_size), float(slope), float(initial_distance), float(max_distance),
                                                             float(cell_size), float(base), int(bool(exponential)), C.byref(n_ground),
                                                             C.byref(n_passes))
        self._pmf_last = (int(n_ground.value), int(n_passes.value))
        return rc, int(n_ground.value), int(n_passes.value)

    def pmf_fetch_raw(self, capacity_ground: int, capacity_passes: int, want=("ground", "windows", "thresholds", "ground_after", "removed_at")) -> tuple:
        """One icpgpu_pmf_fetch call into arrays pre-filled with -2 (those not in `want` are handed over as NULL): (rc, dict)."""
        ip = C.POINTER(C.c_int32)
        n_c = C.c_size_t()
        self._L.icpgpu_search_size(self._h, C.byref(n_c), None)  # (0 without a search cloud)
        out = {"ground": np.full(capacity_ground, -2, np.int32), "windows": np.full(capacity_passes, -2, np.float32),
               "thresholds": np.full(capacity_passes, -2, np.float32), "ground_after": np.full(capacity_passes, -2, np.int32),
               "removed_at": np.full(int(n_c.value), -2, np.int32)}
        ptr = {k: (None if k not in want else _fp(v) if v.dtype == np.float32 else v.ctypes.data_as(ip)) for k, v in out.items()}
        rc = self._L.icpgpu_pmf_fetch(self._h, int(capacity_ground), int(capacity_passes), ptr["ground"], ptr["windows"], ptr["thresholds"],
                                      ptr["ground_after"], ptr["removed_at"])
        return rc, out

    def pmf_stats(self) -> tuple:
        """(host waits of the last filter or operator call, exact point tests of the last filter call's rim scans): icpgpu_pmf_stats."""
        w, t = C.c_int32(), C.c_uint64()
        self._check(self._L.icpgpu_pmf_stats(self._h, C.byref(w), C.byref(t)))
        return int(w.value), int(t.value)

    def progressive_morphological_filter(self, max_window_size: int = 33, slope: float = 0.7, initial_distance: float = 0.15,
                                         max_distance: float = 10.0, cell_size: float = 1.0, base: float = 2.0, exponential: bool = True) -> dict:
        """The ground of the search cloud: ground (int32 ascending), windows and thresholds (the schedule), ground_after (per pass),
        removed_at (per point: the pass that removed it, -1 ground, -2 non-finite) and host_waits."""
        rc, n_ground, n_passes = self.pmf_filter_raw(max_window_size, slope, initial_distance, max_distance, cell_size, base, exponential)
        self._check(rc)
        rc, out = self.pmf_fetch_raw(n_ground, n_passes)
        self._check(rc)
        out["host_waits"] = self.pmf_stats()[0]
        return out

    def pmf_extract(self, negative: bool = False, view: bool = False) -> np.ndarray:
        """pcl::ExtractIndices over the last ground filter: the search cloud's points in (negative: not in) the ground, in order."""
        n_out = C.c_size_t()
        if view:
            ptr = C.POINTER(C.c_float)()
            self._check(self._L.icpgpu_pmf_extract_view(self._h, int(bool(negative)), C.byref(ptr), C.byref(n_out)))
            if n_out.value == 0:
                return np.empty((0, 4), np.float32)
            return np.ctypeslib.as_array(ptr, shape=(n_out.value, 4)).copy()
        out = np.empty((self.search_size()[0], 4), np.float32)
        self._check(self._L.icpgpu_pmf_extract(self._h, int(bool(negative)), _fp(out), C.byref(n_out)))
        return out[: n_out.value].copy()

    # measurement -----------------------------------------------------------------------------------------------
    def calibrate(self) -> int:
        """icpgpu_calibrate: time GICP's two inner solvers on the clouds this context holds and keep the faster (GICP_SOLVER_*)."""
        v = C.c_int()
        self._check(self._L.icpgpu_calibrate(self._h, C.byref(v)))
        return int(v.value)

    def profile_reset(self):
        self._check(self._L.icpgpu_profile_reset(self._h))

    def profile_sampling(self, every: int):
        """Time one correspondence sweep in `every` (library default 7; 1 = all of them, at 6-7 us per iteration)."""
        self._check(self._L.icpgpu_profile_set_sampling(self._h, int(every)))

    def profile(self) -> Profile:
        p = Profile()
        self._check(self._L.icpgpu_profile_get(self._h, C.byref(p)))
        return p

    def synchronize(self):
        self._check(self._L.icpgpu_synchronize(self._h))

    def count_candidates(self, enable: bool = True):
        """Counting runs: target points evaluated by the grid sweeps (see icpgpu_count_candidates)."""
        self._check(self._L.icpgpu_count_candidates(self._h, int(enable)))

    def candidates(self) -> int:
        v = C.c_uint64()
        self._check(self._L.icpgpu_count_candidates_read(self._h, C.byref(v)))
        return int(v.value)


def ndt_step(sums, p, step_size: float, eps: float):
    """icpgpu_ndt_step (host only): one Newton step of the NDT loop -> (status, p_out (6,), step, T_out 4x4 float32);
    status 0 = a step, 1 = |delta| is 0, 2 = delta is NaN."""
    L = _lib.load()
    sums = np.ascontiguousarray(sums, np.float64).reshape(29)
    p = np.ascontiguousarray(p, np.float64).reshape(6)
    p_out = np.zeros(6, np.float64)
    step = C.c_double()
    T = np.zeros(16, np.float32)
    dp = C.POINTER(C.c_double)
    rc = L.icpgpu_ndt_step(sums.ctypes.data_as(dp), p.ctypes.data_as(dp), float(step_size), float(eps), p_out.ctypes.data_as(dp),
                           C.byref(step), _fp(T))
    if rc < 0:
        raise IcpGpuError(rc, "ndt_step: bad argument")
    return rc, p_out, step.value, T.reshape(4, 4).T.copy()


def ndt_line_search_replay(phi_0: float, d_phi_0: float, step_init: float, step_max: float, step_min: float, phi=(), d_phi=()):
    """icpgpu_ndt_line_search_replay (host only): the More-Thuente search replayed from its trials' observations ->
    (status, step, trial): status MT_TRIAL with the next trial's step and index, or the exit (MT_WOLFE ...) with the accepted step
    and trial."""
    L = _lib.load()
    phi = np.ascontiguousarray(phi, np.float64).reshape(-1)
    d_phi = np.ascontiguousarray(d_phi, np.float64).reshape(-1)
    if len(phi) != len(d_phi):
        raise ValueError("phi and d_phi differ in length")
    step = C.c_double()
    trial = C.c_int32()
    dp = C.POINTER(C.c_double)
    rc = L.icpgpu_ndt_line_search_replay(float(phi_0), float(d_phi_0), float(step_init), float(step_max), float(step_min),
                                         phi.ctypes.data_as(dp), d_phi.ctypes.data_as(dp), len(phi), C.byref(step), C.byref(trial))
    if rc < 0:
        raise IcpGpuError(rc, "ndt_line_search_replay: bad argument")
    return rc, step.value, trial.value


def _solve29(name, sums):
    L = _lib.load()
    sums = np.ascontiguousarray(sums, np.float64)
    if sums.shape != (29,):
        raise ValueError("sums must be the 29 float64 terms of icpgpu_reduce_point_to_plane")
    Tk = np.zeros(16, np.float64)
    dp = C.POINTER(C.c_double)
    if getattr(L, name)(sums.ctypes.data_as(dp), Tk.ctypes.data_as(dp)) != 0:
        return None
    return Tk.reshape(4, 4).T.copy()


def solve_point_to_plane(sums):
    """icpgpu_solve_point_to_plane (host only): (AᵀA)⁻¹Aᵀr -> constructTransformationMatrix, 4x4 float64; None when singular."""
    return _solve29("icpgpu_solve_point_to_plane", sums)


def solve_symmetric_point_to_plane(sums):
    """icpgpu_solve_symmetric_point_to_plane (host only): the same x -> R Tr R, 4x4 float64; None when singular."""
    return _solve29("icpgpu_solve_symmetric_point_to_plane", sums)


def result_dict(res: Result, cloud):
    return dict(T=np.array(res.T, dtype=np.float32).reshape(4, 4).T.copy(), converged=bool(res.converged),
                iterations=int(res.iterations), state=int(res.convergence_state), n_corr=int(res.n_correspondences),
                mse=float(res.mse_last), fitness=float(res.fitness), cloud=cloud, t_total_ms=float(res.t_total_ms),
                t_device_ms=float(res.t_device_ms), gicp_solver=int(res.gicp_solver))


class CorrespondenceRejector:
    """pcl::registration::CorrespondenceRejector-shaped base of the five rejectors a registration object's chain may hold
    (addCorrespondenceRejector).  The objects carry parameters only: the stages run on the device inside align()."""

    KIND = 0

    def getClassName(self) -> str:
        return type(self).__name__

    def _entry(self) -> Rejector:
        return Rejector(self.KIND, 0, 0.0)


class CorrespondenceRejectorMedianDistance(CorrespondenceRejector):
    KIND = _lib.REJECT_MEDIAN_DISTANCE

    def __init__(self):
        self._factor = 1.0
        self._median = 0.0

    def setMedianFactor(self, factor):
        self._factor = float(factor)

    def getMedianFactor(self) -> float:
        return self._factor

    def getMedianDistance(self) -> float:
        """The median squared distance of the last iteration of the last align() this rejector took part in."""
        return self._median

    def _entry(self) -> Rejector:
        return Rejector(self.KIND, 0, self._factor)


class CorrespondenceRejectorTrimmed(CorrespondenceRejector):
    KIND = _lib.REJECT_TRIMMED

    def __init__(self):
        self._ratio = 0.5
        self._min = 0

    def setOverlapRatio(self, ratio):
        self._ratio = float(np.float32(ratio))      # (PCL holds a float)

    def getOverlapRatio(self) -> float:
        return self._ratio

    def setMinCorrespondences(self, n):
        self._min = int(n)

    def getMinCorrespondences(self) -> int:
        return self._min

    def _entry(self) -> Rejector:
        return Rejector(self.KIND, self._min, self._ratio)


class CorrespondenceRejectorOneToOne(CorrespondenceRejector):
    KIND = _lib.REJECT_ONE_TO_ONE


class CorrespondenceRejectorSurfaceNormal(CorrespondenceRejector):
    """A pair stays iff the dot of the source's normal (rotated by the iteration's transform) and the target's is above the
    threshold, the cosine of the largest accepted angle (PCL's default 1.0).  The normals are the registration object's
    (setSourceNormals / setTargetNormals) or estimated on the device."""

    KIND = _lib.REJECT_SURFACE_NORMAL

    def __init__(self):
        self._threshold = 1.0

    def setThreshold(self, threshold):
        self._threshold = float(threshold)

    def getThreshold(self) -> float:
        return self._threshold

    def _entry(self) -> Rejector:
        return Rejector(self.KIND, 0, self._threshold)


class CorrespondenceRejectorSampleConsensus(CorrespondenceRejector):
    """RANSAC over the pairs with a rigid transform as the model: a pair stays iff it is an inlier of the best hypothesis.  In a
    registration object's chain it runs inside align() (and waits on the host there); alone -- setInputSource, setInputTarget,
    setInputCorrespondences, getRemainingCorrespondences -- it filters a pair list, e.g. descriptor matches, on a context of its
    own.  setRefineModel(True) is not provided."""

    KIND = _lib.REJECT_SAMPLE_CONSENSUS

    def __init__(self, ctx: "Context | None" = None):
        self._threshold = 0.05
        self._max_iterations = 1000
        self._best_T = np.eye(4, dtype=np.float32)
        self._ctx = ctx
        self._source = self._target = None
        self._pairs = (np.zeros(0, np.int32), np.zeros(0, np.int32))
        self._seed = 12345

    def setInlierThreshold(self, threshold):
        self._threshold = float(threshold)

    def getInlierThreshold(self) -> float:
        return self._threshold

    def setMaximumIterations(self, n):
        self._max_iterations = int(n)

    def getMaximumIterations(self) -> int:
        return self._max_iterations

    def setRefineModel(self, on: bool):
        if on:
            raise NotImplementedError("CorrespondenceRejectorSampleConsensus.setRefineModel(True) is not provided")

    def getRefineModel(self) -> bool:
        return False

    def setInputSource(self, cloud):
        self._source = _as_cloud(cloud)

    def setInputTarget(self, cloud):
        self._target = _as_cloud(cloud)

    def setInputCorrespondences(self, index_query, index_match):
        self._pairs = (np.ascontiguousarray(index_query, np.int32).reshape(-1), np.ascontiguousarray(index_match, np.int32).reshape(-1))

    def getRemainingCorrespondences(self):
        """(index_query, index_match) of the pairs that stay, in their order."""
        if self._source is None or self._target is None:
            raise RuntimeError("CorrespondenceRejectorSampleConsensus: setInputSource and setInputTarget first")
        if self._ctx is None:
            self._ctx = Context()
        r = self._ctx.reject_sample_consensus(self._source, self._target, self._pairs[0], self._pairs[1], self._threshold, self._max_iterations,
                                              self._seed)
        self._best_T = r["best_T"]
        return self._pairs[0][r["kept"]], self._pairs[1][r["kept"]]

    getCorrespondences = getRemainingCorrespondences

    def getBestTransformation(self) -> np.ndarray:
        """The best hypothesis' transform: of the last getRemainingCorrespondences(), or of the last iteration of the last
        align() this rejector took part in."""
        return self._best_T

    def _entry(self) -> Rejector:
        return Rejector(self.KIND, self._max_iterations, self._threshold)


class _OutlierFilter:
    """What pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval share: the input cloud, `negative`, the removed indices."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._cloud = np.empty((0, 4), np.float32)
        self._negative = False
        self._removed = np.empty(0, np.int32)

    def setInputCloud(self, cloud):
        self._cloud = _as_cloud(cloud)

    def setNegative(self, negative: bool):
        self._negative = bool(negative)

    def getNegative(self) -> bool:
        return self._negative

    def getRemovedIndices(self) -> np.ndarray:
        return self._removed

    def _run(self, cloud) -> np.ndarray:
        raise NotImplementedError

    def filter(self) -> np.ndarray:
        """The filtered cloud; a refused call returns an empty one, as PCL's error path leaves `output`."""
        self._removed = np.empty(0, np.int32)
        try:
            out = self._run(self._cloud)
        except IcpGpuError:
            return np.empty((0, 4), np.float32)
        self._removed = self._ctx.outlier_fetch()["removed"]
        return out


class StatisticalOutlierRemoval(_OutlierFilter):
    """pcl::StatisticalOutlierRemoval<PointXYZ> (PCL's defaults: mean_k 1, stddev_mult 0)."""

    def __init__(self, device_id: int = 0):
        super().__init__(device_id)
        self._mean_k = 1
        self._stddev_mult = 0.0

    def setMeanK(self, k: int):
        self._mean_k = int(k)

    def getMeanK(self) -> int:
        return self._mean_k

    def setStddevMulThresh(self, m: float):
        self._stddev_mult = float(m)

    def getStddevMulThresh(self) -> float:
        return self._stddev_mult

    def _run(self, cloud) -> np.ndarray:
        return self._ctx.statistical_outlier_removal(cloud, self._mean_k, self._stddev_mult, self._negative, view=True)


class RadiusOutlierRemoval(_OutlierFilter):
    """pcl::RadiusOutlierRemoval<PointXYZ> (PCL's defaults: radius 0, min_pts 1)."""

    def __init__(self, device_id: int = 0):
        super().__init__(device_id)
        self._radius = 0.0
        self._min_pts = 1

    def setRadiusSearch(self, r: float):
        self._radius = float(r)

    def getRadiusSearch(self) -> float:
        return self._radius

    def setMinNeighborsInRadius(self, n: int):
        self._min_pts = int(n)

    def getMinNeighborsInRadius(self) -> int:
        return self._min_pts

    def _run(self, cloud) -> np.ndarray:
        return self._ctx.radius_outlier_removal(cloud, self._radius, self._min_pts, self._negative, view=True)


class _SubsetFilter:
    """What pcl::PassThrough, CropBox, UniformSampling and FarthestPointSampling share here: the input cloud, filter() as the kept
    rows or (indices=True: PCL's filter(indices)) their indices, and the removed indices."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._cloud = np.empty((0, 4), np.float32)
        self._removed = np.empty(0, np.int32)

    def setInputCloud(self, cloud):
        self._cloud = _as_cloud(cloud)

    def getRemovedIndices(self) -> np.ndarray:
        return self._removed

    def _run(self, cloud) -> np.ndarray:
        raise NotImplementedError

    def filter(self, indices: bool = False) -> np.ndarray:
        """The filtered cloud (indices: the kept rows' indices); a refused call returns an empty one, as PCL's error path does."""
        self._removed = np.empty(0, np.int32)
        try:
            out = self._run(self._cloud)
        except IcpGpuError:
            return np.empty(0, np.int32) if indices else np.empty((0, 4), np.float32)
        res = self._ctx.subset_fetch()
        self._removed = res["removed"]
        return res["kept"] if indices else out


class PassThrough(_SubsetFilter):
    """pcl::PassThrough<PointXYZ> (PCL's defaults: no field, FLT_MIN .. FLT_MAX, not negative)."""

    def __init__(self, device_id: int = 0):
        super().__init__(device_id)
        self._field, self._lo, self._hi, self._negative = -1, FLT_MIN, FLT_MAX, False

    def setFilterFieldName(self, name: str):
        if name not in ("x", "y", "z"):
            raise ValueError(f"PassThrough: field {name!r} is not one of x, y, z")
        self._field = "xyz".index(name)

    def getFilterFieldName(self) -> str:
        return "" if self._field < 0 else "xyz"[self._field]

    def setFilterLimits(self, lo: float, hi: float):
        self._lo, self._hi = float(lo), float(hi)

    def getFilterLimits(self) -> tuple:
        return self._lo, self._hi

    def setNegative(self, negative: bool):
        self._negative = bool(negative)

    def getNegative(self) -> bool:
        return self._negative

    def _run(self, cloud) -> np.ndarray:
        return self._ctx.pass_through(cloud, self._field, self._lo, self._hi, self._negative, view=True)


class CropBox(_SubsetFilter):
    """pcl::CropBox<PointXYZ> (PCL's defaults: the box -1 .. 1, no translation, rotation or transform, not negative)."""

    def __init__(self, device_id: int = 0):
        super().__init__(device_id)
        self._min, self._max = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
        self._translation, self._rotation = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._transform = None
        self._negative = False

    def setMin(self, min_pt):
        self._min = np.asarray(min_pt, np.float32).reshape(-1)[:3].copy()

    def setMax(self, max_pt):
        self._max = np.asarray(max_pt, np.float32).reshape(-1)[:3].copy()

    def setTranslation(self, translation):
        self._translation = np.asarray(translation, np.float32).reshape(3).copy()

    def setRotation(self, rotation):
        self._rotation = np.asarray(rotation, np.float32).reshape(3).copy()

    def setTransform(self, transform):
        self._transform = None if transform is None else np.asarray(transform, np.float32).reshape(4, 4).copy()

    def setNegative(self, negative: bool):
        self._negative = bool(negative)

    def getNegative(self) -> bool:
        return self._negative

    def _run(self, cloud) -> np.ndarray:
        plain = self._transform is None and not self._translation.any() and not self._rotation.any()
        T = None if plain else crop_box_matrix(self._transform, self._translation, self._rotation)
        return self._ctx.crop_box(cloud, self._min, self._max, T, self._negative, view=True)


class UniformSampling(_SubsetFilter):
    """pcl::UniformSampling<PointXYZ>: setRadiusSearch is the leaf size."""

    def __init__(self, device_id: int = 0):
        super().__init__(device_id)
        self._leaf = 0.0

    def setRadiusSearch(self, radius: float):
        self._leaf = float(radius)

    def getRadiusSearch(self) -> float:
        return self._leaf

    def _run(self, cloud) -> np.ndarray:
        return self._ctx.uniform_sampling(cloud, self._leaf, view=True)


class FarthestPointSampling(_SubsetFilter):
    """pcl::FarthestPointSampling<PointXYZ> (PCL 1.12): setSample rows in selection order; setSeed picks the first row
    (seeded_first_row), not mt19937's."""

    def __init__(self, device_id: int = 0):
        super().__init__(device_id)
        self._sample, self._seed = 0, 0

    def setSample(self, sample: int):
        self._sample = int(sample)

    def getSample(self) -> int:
        return self._sample

    def setSeed(self, seed: int):
        self._seed = int(seed)

    def getSeed(self) -> int:
        return self._seed

    def _run(self, cloud) -> np.ndarray:
        return self._ctx.farthest_point_sampling(cloud, self._sample, seeded_first_row(cloud, self._seed), view=True)


class KdTree:
    """pcl::search::KdTree<PointXYZ> / pcl::KdTreeFLANN<PointXYZ>-shaped front end: exact k-nearest and radius search over one cloud
    (include/icpgpu.h, "neighbour search": results ascending by (d2, index)).  A query is a point (x, y, z[, w]) or an index into the
    input cloud; the batched forms take a whole query cloud (None: the input cloud's own points) and are what a GPU user should
    call."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._cloud = np.empty((0, 4), np.float32)

    def setInputCloud(self, cloud):
        self._cloud = _as_cloud(cloud).copy()
        self._ctx.search_set_input(self._cloud)

    def getInputCloud(self) -> np.ndarray:
        return self._cloud

    def _query(self, point) -> np.ndarray:
        if isinstance(point, (int, np.integer)):
            return self._cloud[int(point):int(point) + 1]
        q = np.ones((1, 4), np.float32)
        p = np.asarray(point, np.float32).reshape(-1)
        q[0, :min(p.size, 4)] = p[:4]
        return q

    def nearestKSearch(self, point, k: int):
        """(indices, squared distances) of the k nearest; their number is len(indices), as PCL's return value."""
        idx, d2, n = self._ctx.search_knn(self._query(point), k)
        return idx[0, :n[0]].copy(), d2[0, :n[0]].copy()

    def radiusSearch(self, point, radius: float, max_nn: int = 0):
        _, idx, d2 = self._ctx.search_radius(self._query(point), radius, max_nn)
        return idx, d2

    def nearestKSearchBatch(self, queries, k: int):
        """(idx (n_q, k), d2 (n_q, k), n_found (n_q,)) for a whole query cloud (None: the input cloud's own points)."""
        return self._ctx.search_knn(queries, k)

    def radiusSearchBatch(self, queries, radius: float, max_nn: int = 0):
        """(row_start (n_q + 1,), idx, d2): CSR rows for a whole query cloud (None: the input cloud's own points)."""
        return self._ctx.search_radius(queries, radius, max_nn)


KdTreeFLANN = KdTree


class NormalEstimation:
    """pcl::NormalEstimation<PointXYZ, Normal>-shaped front end (include/icpgpu.h, "normal estimation"): setInputCloud, optionally
    setSearchSurface (the default is the input cloud), setKSearch or setRadiusSearch, setViewPoint, compute() -> (n, 4) float32
    {normal_x, normal_y, normal_z, curvature}, NaN rows where PCL clears is_dense.  What compute() returns can be handed to
    IterativeClosestPointWithNormals.setInputTarget(cloud, normals) as it is."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._surface = None
        self._k = 0
        self._radius = 0.0
        self._viewpoint = (0.0, 0.0, 0.0)
        self._n_neighbours = np.empty(0, np.int32)

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setSearchSurface(self, cloud):
        self._surface = None if cloud is None else _as_cloud(cloud).copy()

    def setSearchMethod(self, tree=None):
        """Accepted and ignored: the search is the library's own (exact, ascending by (d2, index))."""

    def setKSearch(self, k: int):
        self._k = int(k)

    def getKSearch(self) -> int:
        return self._k

    def setRadiusSearch(self, radius: float):
        self._radius = float(radius)

    def getRadiusSearch(self) -> float:
        return self._radius

    def setViewPoint(self, vpx: float, vpy: float, vpz: float):
        self._viewpoint = (float(vpx), float(vpy), float(vpz))

    def getViewPoint(self) -> tuple:
        return self._viewpoint

    def getNeighbourCounts(self) -> np.ndarray:
        """How many neighbours the last compute() used for every point (not PCL's)."""
        return self._n_neighbours

    def compute(self) -> np.ndarray:
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "compute: setInputCloud first")
        if self._surface is None:
            self._ctx.search_set_input(self._input)
            queries = None
        else:
            self._ctx.search_set_input(self._surface)
            queries = self._input
        normals, self._n_neighbours = self._ctx.normal_estimation(queries, self._k, self._radius, self._viewpoint)
        return normals


class FPFHEstimation:
    """pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33>-shaped front end (include/icpgpu.h, "fast point feature histograms"):
    setInputCloud, setInputNormals (the normals of the search surface -- of the input cloud when no surface is set -- as
    NormalEstimation.compute() returns them), optionally setSearchSurface, setKSearch or setRadiusSearch, compute() -> (n, 33)
    float32, NaN rows for non-finite input points."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._normals = None
        self._surface = None
        self._k = 0
        self._radius = 0.0
        self._n_neighbours = np.empty(0, np.int32)

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setInputNormals(self, normals):
        self._normals = _as_cloud(normals).copy()

    def setSearchSurface(self, cloud):
        self._surface = None if cloud is None else _as_cloud(cloud).copy()

    def setSearchMethod(self, tree=None):
        """Accepted and ignored: the search is the library's own (exact, ascending by (d2, index))."""

    def setKSearch(self, k: int):
        self._k = int(k)

    def getKSearch(self) -> int:
        return self._k

    def setRadiusSearch(self, radius: float):
        self._radius = float(radius)

    def getRadiusSearch(self) -> float:
        return self._radius

    def getNeighbourCounts(self) -> np.ndarray:
        """How many neighbours the last compute() found for every point (not PCL's)."""
        return self._n_neighbours

    def compute(self) -> np.ndarray:
        if self._input is None or self._normals is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "compute: setInputCloud and setInputNormals first")
        surface = self._input if self._surface is None else self._surface
        if self._normals.shape[0] != surface.shape[0]:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"compute: {self._normals.shape[0]} normals for a search surface of {surface.shape[0]} points")
        self._ctx.search_set_input(surface)
        fpfh, self._n_neighbours = self._ctx.fpfh_estimation(self._normals, None if self._surface is None else self._input, self._k, self._radius)
        return fpfh


class BoundaryEstimation:
    """pcl::BoundaryEstimation<PointXYZ, Normal, Boundary>-shaped front end (include/icpgpu.h, "boundary estimation"): setInputCloud,
    setInputNormals (the INPUT cloud's normals, as NormalEstimation.compute() returns them), optionally setSearchSurface, setKSearch
    or setRadiusSearch, setAngleThreshold (default pi / 2), compute() -> (n,) uint8, pcl::Boundary's boundary_point."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._normals = None
        self._surface = None
        self._k = 0
        self._radius = 0.0
        self._angle = math.pi / 2
        self._last = None

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setInputNormals(self, normals):
        self._normals = _as_cloud(normals).copy()

    def setSearchSurface(self, cloud):
        self._surface = None if cloud is None else _as_cloud(cloud).copy()

    def setSearchMethod(self, tree=None):
        """Accepted and ignored: the search is the library's own (exact, ascending by (d2, index))."""

    def setKSearch(self, k: int):
        self._k = int(k)

    def getKSearch(self) -> int:
        return self._k

    def setRadiusSearch(self, radius: float):
        self._radius = float(radius)

    def getRadiusSearch(self) -> float:
        return self._radius

    def setAngleThreshold(self, angle: float):
        self._angle = float(angle)

    def getAngleThreshold(self) -> float:
        return self._angle

    def getLastResult(self):
        """Everything the last compute() produced (Context.boundary_estimation's dict; not PCL's)."""
        return self._last

    def compute(self) -> np.ndarray:
        if self._input is None or self._normals is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "compute: setInputCloud and setInputNormals first")
        if self._normals.shape[0] != self._input.shape[0]:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"compute: {self._normals.shape[0]} normals for an input of {self._input.shape[0]} points")
        self._ctx.search_set_input(self._input if self._surface is None else self._surface)
        self._last = self._ctx.boundary_estimation(self._normals, None if self._surface is None else self._input, self._k, self._radius, self._angle)
        return self._last["boundary"]


class FeatureKdTree:
    """pcl::KdTreeFLANN<pcl::FPFHSignature33>-shaped front end (include/icpgpu.h, "feature-space k-nearest"): setInputCloud with
    (n, 33) descriptors, nearestKSearch(queries, k) -> (idx (n_q, k) int32, d2 (n_q, k) float32), padded with -1 / +inf."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None

    def setInputCloud(self, features):
        self._input = np.ascontiguousarray(features, np.float32).reshape(-1, FPFH_BINS).copy()

    def nearestKSearch(self, queries, k: int):
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "nearestKSearch: setInputCloud first")
        idx, d2, _ = self._ctx.feature_knn(self._input, np.ascontiguousarray(queries, np.float32).reshape(-1, FPFH_BINS), k)
        return idx, d2


class SampleConsensusPrerejective:
    """pcl::SampleConsensusPrerejective<PointXYZ, PointXYZ, FPFHSignature33>-shaped front end (include/icpgpu.h, "sample-consensus
    alignment"): setInputSource, setSourceFeatures, setInputTarget, setTargetFeatures, setNumberOfSamples, setCorrespondenceRandomness,
    setSimilarityThreshold, setMaxCorrespondenceDistance, setInlierFraction, setMaximumIterations, our own setSeed, align() -> the
    aligned source, hasConverged, getFinalTransformation, getInliers, getFitnessScore.  The defaults are PCL's (3 samples, randomness
    2, similarity 0.9, inlier fraction 0; Registration's 10 iterations and sqrt(DBL_MAX) distance are replaced by 1000 and 1.0: the
    call refuses a distance whose square is not a float).  A guess is not provided."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._source = self._target = self._sf = self._tf = None
        self._nr, self._k, self._sim, self._dist, self._frac, self._it, self._seed = 3, 2, 0.9, 1.0, 0.0, 1000, 0
        self._T = np.eye(4, dtype=np.float32)
        self._converged = False
        self._fitness = float(np.finfo(np.float32).max)
        self._inliers = np.empty(0, np.int32)

    def setInputSource(self, cloud):
        self._source = _as_cloud(cloud).copy()

    def setSourceFeatures(self, features):
        self._sf = np.ascontiguousarray(features, np.float32).reshape(-1, FPFH_BINS).copy()

    def setInputTarget(self, cloud):
        self._target = _as_cloud(cloud).copy()

    def setTargetFeatures(self, features):
        self._tf = np.ascontiguousarray(features, np.float32).reshape(-1, FPFH_BINS).copy()

    def setNumberOfSamples(self, nr_samples: int):
        self._nr = int(nr_samples)

    def getNumberOfSamples(self) -> int:
        return self._nr

    def setCorrespondenceRandomness(self, k: int):
        self._k = int(k)

    def getCorrespondenceRandomness(self) -> int:
        return self._k

    def setSimilarityThreshold(self, similarity_threshold: float):
        self._sim = float(similarity_threshold)

    def getSimilarityThreshold(self) -> float:
        return self._sim

    def setMaxCorrespondenceDistance(self, distance: float):
        self._dist = float(distance)

    def getMaxCorrespondenceDistance(self) -> float:
        return self._dist

    def setInlierFraction(self, inlier_fraction: float):
        self._frac = float(inlier_fraction)

    def getInlierFraction(self) -> float:
        return self._frac

    def setMaximumIterations(self, max_iterations: int):
        self._it = int(max_iterations)

    def getMaximumIterations(self) -> int:
        return self._it

    def setSeed(self, seed: int):
        """The seed of the counter-based generator the samples come from (not PCL's, whose samples come from rand())."""
        self._seed = int(seed)

    def align(self) -> np.ndarray:
        if self._source is None or self._target is None or self._sf is None or self._tf is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "align: setInputSource, setSourceFeatures, setInputTarget and setTargetFeatures first")
        self._ctx.search_set_input(self._target)
        r = self._ctx.scp_align(self._source, self._sf, self._tf, nr_samples=self._nr, k_correspondences=self._k, similarity_threshold=self._sim,
                                max_correspondence_distance=self._dist, inlier_fraction=self._frac, max_iterations=self._it, seed=self._seed)
        self._T, self._converged, self._fitness, self._inliers = r["T"], r["converged"], r["fitness"], r["inliers"]
        return r["cloud"]

    def hasConverged(self) -> bool:
        return self._converged

    def getFinalTransformation(self) -> np.ndarray:
        return self._T

    def getInliers(self) -> np.ndarray:
        return self._inliers

    def getFitnessScore(self) -> float:
        return self._fitness


class EuclideanClusterExtraction:
    """pcl::EuclideanClusterExtraction<PointXYZ>-shaped front end (include/icpgpu.h, "euclidean clustering"): setInputCloud,
    setClusterTolerance, setMinClusterSize, setMaxClusterSize, extract() -> a list of int32 index arrays, the largest cluster first,
    ascending inside a cluster.  The defaults are PCL's constructor's (0, 1, INT_MAX).  setIndices is not provided."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._tolerance = 0.0
        self._min = 1
        self._max = 2**31 - 1
        self._labels = np.empty(0, np.int32)

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setSearchMethod(self, tree=None):
        """Accepted and ignored: the search is the library's own (exact)."""

    def setClusterTolerance(self, tolerance: float):
        self._tolerance = float(tolerance)

    def getClusterTolerance(self) -> float:
        return self._tolerance

    def setMinClusterSize(self, min_cluster_size: int):
        self._min = int(min_cluster_size)

    def getMinClusterSize(self) -> int:
        return self._min

    def setMaxClusterSize(self, max_cluster_size: int):
        self._max = int(max_cluster_size)

    def getMaxClusterSize(self) -> int:
        return self._max

    def getLabels(self) -> np.ndarray:
        """The last extract()'s cluster rank of every input point, -1 where it is in none (not PCL's)."""
        return self._labels

    def extract(self) -> list:
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "extract: setInputCloud first")
        self._ctx.search_set_input(self._input)
        start, indices, self._labels, _ = self._ctx.euclidean_cluster_extraction(self._tolerance, self._min, self._max)
        return [indices[start[r]:start[r + 1]].copy() for r in range(start.size - 1)]


class RegionGrowing:
    """pcl::RegionGrowing<PointXYZ, Normal>-shaped front end (include/icpgpu.h, "region growing": an order-free rule, not PCL's seed
    queue): setInputCloud, setInputNormals (as NormalEstimation.compute() returns them), setNumberOfNeighbours, setSmoothnessThreshold
    (radians), setCurvatureThreshold, setCurvatureTestFlag, setMinClusterSize, setMaxClusterSize, extract() -> a list of int32 index
    arrays, the largest region first, ascending inside a region; getSegmentFromPoint(index).  The defaults are PCL's constructor's
    (30 neighbours, 30 degrees, 0.05, sizes 1 .. INT_MAX).  setIndices, setSmoothModeFlag(False) and setResidualTestFlag(True) raise."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._normals = None
        self._k = 30
        self._theta = 30.0 / 180.0 * math.pi
        self._curvature = 0.05
        self._curvature_test = True
        self._min = 1
        self._max = 2**31 - 1
        self._result = None

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()
        self._result = None

    def setInputNormals(self, normals):
        self._normals = _as_cloud(normals).copy()
        self._result = None

    def setSearchMethod(self, tree=None):
        """Accepted and ignored: the search is the library's own (exact, ascending by (d2, index))."""

    def setIndices(self, indices):
        raise IcpGpuError(_lib.ERR_UNSUPPORTED, "RegionGrowing.setIndices is not provided")

    def setSmoothModeFlag(self, value: bool):
        if not value:
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "RegionGrowing.setSmoothModeFlag(False) is not provided")

    def setResidualTestFlag(self, value: bool):
        if value:
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "RegionGrowing.setResidualTestFlag(True) is not provided")

    def setNumberOfNeighbours(self, k: int):
        self._k = int(k)

    def getNumberOfNeighbours(self) -> int:
        return self._k

    def setSmoothnessThreshold(self, theta: float):
        self._theta = float(theta)

    def getSmoothnessThreshold(self) -> float:
        return self._theta

    def setCurvatureThreshold(self, curvature: float):
        self._curvature = float(curvature)

    def getCurvatureThreshold(self) -> float:
        return self._curvature

    def setCurvatureTestFlag(self, value: bool):
        self._curvature_test = bool(value)

    def getCurvatureTestFlag(self) -> bool:
        return self._curvature_test

    def setMinClusterSize(self, min_cluster_size: int):
        self._min = int(min_cluster_size)

    def getMinClusterSize(self) -> int:
        return self._min

    def setMaxClusterSize(self, max_cluster_size: int):
        self._max = int(max_cluster_size)

    def getMaxClusterSize(self) -> int:
        return self._max

    def getLabels(self) -> np.ndarray:
        """The last extract()'s region rank of every input point, -1 where it is in none (not PCL's)."""
        return np.empty(0, np.int32) if self._result is None else self._result[2]

    def extract(self) -> list:
        if self._input is None or self._normals is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "extract: setInputCloud and setInputNormals first")
        if len(self._normals) != len(self._input):
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"extract: {len(self._normals)} normals for {len(self._input)} points")
        self._ctx.search_set_input(self._input)
        threshold = self._curvature if self._curvature_test else math.inf
        self._result = self._ctx.region_growing(self._normals, self._k, self._theta, threshold, self._min, self._max)
        start, indices = self._result[:2]
        return [indices[start[r]:start[r + 1]].copy() for r in range(start.size - 1)]

    def getSegmentFromPoint(self, index: int) -> np.ndarray:
        """The emitted region the point lies in (extract() runs first if it has not), empty when it is in none."""
        if self._result is None:
            self.extract()
        start, indices, labels = self._result[:3]
        if not 0 <= int(index) < labels.size:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"getSegmentFromPoint: index {index} outside the cloud")
        r = int(labels[int(index)])
        return np.empty(0, np.int32) if r < 0 else indices[start[r]:start[r + 1]].copy()


class MomentOfInertiaEstimation:
    """pcl::MomentOfInertiaEstimation<PointXYZ>-shaped front end (include/icpgpu.h, "segment moments"): setInputCloud, setIndices (ONE
    segment; the whole cloud without), compute(), getAABB() -> (min, max), getOBB() -> (min, max, position, rotation) as PCL hands them
    out (min / max relative to the box's centre, the rotation's COLUMNS the major, middle and minor axis), getEigenValues() -> (major,
    middle, minor), getEigenVectors() -> three vectors, getMassCenter().  Beyond PCL, every segment of a segmentation in one call:
    compute_segments(list of index arrays), compute_clusters(EuclideanClusterExtraction) and compute_regions(RegionGrowing) -- the
    last two read the extractor's unfetched result on the device -- each returning the records (Context.segment_moments).
    getMomentOfInertia, getEccentricity, setAngleStep and setIndices on top of a segment list raise."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._indices = None
        self._records = None

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()
        self._records = None

    def setIndices(self, indices):
        self._indices = np.ascontiguousarray(indices, np.int32).copy()
        self._records = None

    def setAngleStep(self, step: float):
        raise IcpGpuError(_lib.ERR_UNSUPPORTED, "MomentOfInertiaEstimation.setAngleStep: the moment-of-inertia sweep is not provided")

    def getMomentOfInertia(self):
        raise IcpGpuError(_lib.ERR_UNSUPPORTED, "MomentOfInertiaEstimation.getMomentOfInertia is not provided")

    def getEccentricity(self):
        raise IcpGpuError(_lib.ERR_UNSUPPORTED, "MomentOfInertiaEstimation.getEccentricity is not provided")

    def compute(self):
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "compute: setInputCloud first")
        indices = np.arange(len(self._input), dtype=np.int32) if self._indices is None else self._indices
        self.compute_segments([indices])

    def compute_segments(self, segments) -> np.ndarray:
        """One record per index array of `segments` over the input cloud; the getters then describe the first."""
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "compute_segments: setInputCloud first")
        if self._indices is not None and not (len(segments) == 1 and segments[0] is self._indices):
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "MomentOfInertiaEstimation: setIndices on top of a segment list is not provided")
        lists = [np.ascontiguousarray(s, np.int32).reshape(-1) for s in segments]
        start = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(s) for s in lists], out=start[1:])
        self._ctx.search_set_input(self._input)
        self._records = self._ctx.segment_moments(start, np.concatenate(lists) if lists else np.empty(0, np.int32))
        return self._records

    def _compute_extractor(self, extractor, source: str) -> np.ndarray:
        if self._indices is not None:
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "MomentOfInertiaEstimation: setIndices on top of a segment list is not provided")
        segments = extractor.extract()  # (its context holds the search cloud and the result this call reads on the device)
        self._records = extractor._ctx.segment_moments(source=source, n_segments=len(segments))
        return self._records

    def compute_clusters(self, extractor: "EuclideanClusterExtraction") -> np.ndarray:
        """extractor.extract(), then one record per cluster in emitted order, read from the device-resident result."""
        return self._compute_extractor(extractor, "clusters")

    def compute_regions(self, extractor: "RegionGrowing") -> np.ndarray:
        """extractor.extract(), then one record per region in emitted order, read from the device-resident result."""
        return self._compute_extractor(extractor, "regions")

    def _first(self):
        if self._records is None or self._records.size == 0:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "MomentOfInertiaEstimation: compute first")
        return self._records[0]

    def getAABB(self) -> tuple:
        r = self._first()
        return r["aabb_min"].copy(), r["aabb_max"].copy()

    def getOBB(self) -> tuple:
        r = self._first()
        half = r["obb_dims"] / 2.0
        return -half, half, r["obb_position"].copy(), r["axes"].reshape(3, 3).T.copy()

    def getEigenValues(self) -> tuple:
        return tuple(float(v) for v in self._first()["eigenvalues"])

    def getEigenVectors(self) -> tuple:
        axes = self._first()["axes"].reshape(3, 3)
        return axes[0].copy(), axes[1].copy(), axes[2].copy()

    def getMassCenter(self) -> np.ndarray:
        return self._first()["centroid"].copy()


class ISSKeypoint3D:
    """pcl::ISSKeypoint3D<PointXYZ, PointXYZ>-shaped front end (include/icpgpu.h, "ISS keypoints"): setInputCloud, setSalientRadius,
    setNonMaxRadius, setThreshold21, setThreshold32, setMinNeighbors, compute() -> the keypoint cloud, getKeypointsIndices().  The
    defaults are PCL's constructor's (radii 0, gammas 0.975, 5 neighbours), so compute() refuses until both radii are set.  Border
    estimation is ISSKeypoint3DBorder's, below: on this class setBorderRadius with a radius above 0 raises; setNormalRadius and
    setNumberOfThreads are stored and have no effect.  setIndices and setSearchSurface are not provided."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._salient = 0.0
        self._non_max = 0.0
        self._gamma_21 = 0.975
        self._gamma_32 = 0.975
        self._min_neighbors = 5
        self._border = 0.0
        self._normal_radius = 0.0
        self._threads = 0
        self._indices = np.empty(0, np.int32)
        self._last = None

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setSearchMethod(self, tree=None):
        """Accepted and ignored: the search is the library's own (exact)."""

    def setSalientRadius(self, salient_radius: float):
        self._salient = float(salient_radius)

    def setNonMaxRadius(self, non_max_radius: float):
        self._non_max = float(non_max_radius)

    def setThreshold21(self, gamma_21: float):
        self._gamma_21 = float(gamma_21)

    def setThreshold32(self, gamma_32: float):
        self._gamma_32 = float(gamma_32)

    def setMinNeighbors(self, min_neighbors: int):
        self._min_neighbors = int(min_neighbors)

    def setBorderRadius(self, border_radius: float):
        if float(border_radius) > 0.0:
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "setBorderRadius: border estimation is not provided")
        self._border = float(border_radius)

    def setNormalRadius(self, normal_radius: float):
        """Stored; without border estimation it has no effect."""
        self._normal_radius = float(normal_radius)

    def setNumberOfThreads(self, nr_threads: int = 0):
        """Stored; the kernels' parallelism is the device's."""
        self._threads = int(nr_threads)

    def getKeypointsIndices(self) -> np.ndarray:
        """The last compute()'s keypoints as ascending indices into the input cloud."""
        return self._indices

    def getLastResult(self):
        """Everything the last compute() produced (Context.iss_keypoints' dict; not PCL's)."""
        return self._last

    def compute(self) -> np.ndarray:
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "compute: setInputCloud first")
        self._ctx.search_set_input(self._input)
        self._last = self._ctx.iss_keypoints(self._salient, self._non_max, self._gamma_21, self._gamma_32, self._min_neighbors)
        self._indices = self._last["keypoint_index"]
        return self._last["keypoints"]


class ISSKeypoint3DBorder(ISSKeypoint3D):
    """ISSKeypoint3D with PCL's border estimation: setBorderRadius, setNormalRadius, setNormals and setAngleThreshold work as in
    pcl::ISSKeypoint3D, and compute() refuses every keypoint within the border radius of a boundary point of the cloud.  Beyond PCL:
    getEdgePoints() and getBorderPoints().  It is a class of its own, and not ISSKeypoint3D itself, because the tests of the change
    that added ISSKeypoint3D pin that its setBorderRadius(r > 0) raises; folding the two is left to a change that may edit them."""

    def __init__(self, device_id: int = 0):
        super().__init__(device_id)
        self._angle = math.pi / 2
        self._normals = None

    def setBorderRadius(self, border_radius: float):
        self._border = float(border_radius)

    def setNormalRadius(self, normal_radius: float):
        self._normal_radius = float(normal_radius)

    def setNormals(self, normals):
        self._normals = None if normals is None else _as_cloud(normals).copy()

    def setAngleThreshold(self, angle: float):
        self._angle = float(angle)

    def getEdgePoints(self) -> np.ndarray:
        """The last compute()'s boundary points as ascending indices into the input cloud (not PCL's)."""
        return np.flatnonzero(self._last["edge"]).astype(np.int32) if self._last else np.empty(0, np.int32)

    def getBorderPoints(self) -> np.ndarray:
        """The points the last compute() skipped for lying within the border radius of an edge point (not PCL's)."""
        return np.flatnonzero(self._last["border"]).astype(np.int32) if self._last else np.empty(0, np.int32)

    def compute(self) -> np.ndarray:
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "compute: setInputCloud first")
        self._ctx.search_set_input(self._input)
        self._last = self._ctx.iss_keypoints_border(self._salient, self._non_max, self._gamma_21, self._gamma_32, self._min_neighbors, self._border,
                                                    self._angle, self._normals, self._normal_radius)
        self._indices = self._last["keypoint_index"]
        return self._last["keypoints"]


class SACSegmentation:
    """pcl::SACSegmentation<PointXYZ>-shaped front end (include/icpgpu.h, "plane segmentation"): setInputCloud, setModelType
    (SACMODEL_PLANE, SACMODEL_PERPENDICULAR_PLANE), setMethodType (SAC_RANSAC: anything else raises), setDistanceThreshold,
    setMaxIterations, setProbability, setOptimizeCoefficients, setAxis, setEpsAngle, our own setSeed, and
    segment() -> (inliers int32 ascending, coefficients (4,) float32; both empty when no model was found).  The defaults are PCL's
    (threshold 0, 50 iterations, probability 0.99, optimize true).  setIndices is not provided."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._model = _lib.SACMODEL_PLANE
        self._threshold = 0.0
        self._max_iterations = 50
        self._probability = 0.99
        self._optimize = True
        self._axis = (0.0, 0.0, 0.0)
        self._eps_angle = 0.0
        self._seed = 0
        self.iterations = 0

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setModelType(self, model: int):
        if model not in (_lib.SACMODEL_PLANE, _lib.SACMODEL_PERPENDICULAR_PLANE):
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "setModelType: SACMODEL_PLANE or SACMODEL_PERPENDICULAR_PLANE")
        self._model = int(model)

    def getModelType(self) -> int:
        return self._model

    def setMethodType(self, method: int):
        if method != _lib.SAC_RANSAC:
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "setMethodType: SAC_RANSAC is the only method")

    def getMethodType(self) -> int:
        return _lib.SAC_RANSAC

    def setDistanceThreshold(self, threshold: float):
        self._threshold = float(threshold)

    def getDistanceThreshold(self) -> float:
        return self._threshold

    def setMaxIterations(self, max_iterations: int):
        self._max_iterations = int(max_iterations)

    def getMaxIterations(self) -> int:
        return self._max_iterations

    def setProbability(self, probability: float):
        self._probability = float(probability)

    def getProbability(self) -> float:
        return self._probability

    def setOptimizeCoefficients(self, optimize: bool):
        self._optimize = bool(optimize)

    def getOptimizeCoefficients(self) -> bool:
        return self._optimize

    def setAxis(self, axis):
        self._axis = tuple(float(v) for v in np.asarray(axis, np.float64).reshape(3))

    def getAxis(self) -> tuple:
        return self._axis

    def setEpsAngle(self, eps_angle: float):
        self._eps_angle = float(eps_angle)

    def getEpsAngle(self) -> float:
        return self._eps_angle

    def setSeed(self, seed: int):
        """NOT a PCL method: the counter-based generator's seed (PCL seeds rand() with a constant)."""
        self._seed = int(seed)

    def segment(self) -> tuple:
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "segment: setInputCloud first")
        self._ctx.search_set_input(self._input)
        axis = self._axis if self._model == _lib.SACMODEL_PERPENDICULAR_PLANE else None
        inliers, coeff, self.iterations, found = self._ctx.sac_plane_segmentation(self._threshold, self._max_iterations, self._probability,
                                                                                 self._seed, self._optimize, axis, self._eps_angle)
        if not found:
            return np.empty(0, np.int32), np.empty(0, np.float32)
        return inliers, coeff


class SACSegmentationFromNormals:
    """pcl::SACSegmentationFromNormals<PointXYZ, Normal>-shaped front end (include/icpgpu.h, "segmentation from normals"):
    setInputCloud, setInputNormals ((n, 4) rows nx, ny, nz, curvature: NormalEstimation's output), setModelType
    (SACMODEL_NORMAL_PLANE, SACMODEL_CYLINDER), setMethodType (SAC_RANSAC: anything else raises), setDistanceThreshold,
    setNormalDistanceWeight, setRadiusLimits, setMaxIterations, setProbability, setOptimizeCoefficients, setAxis, setEpsAngle, our
    own setSeed, and segment() -> (inliers int32 ascending, coefficients (4,) or (7,) float32; both empty when no model was found).
    The defaults are PCL's (threshold 0, weight 0.1, limits 0 / 0, 50 iterations, probability 0.99, optimize true).  An axis of zero
    length (the default) means none, as in PCL.  After a segment, extractCloud(negative) is pcl::ExtractIndices over it."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._normals = None
        self._model = _lib.SACMODEL_NORMAL_PLANE
        self._threshold = 0.0
        self._weight = 0.1
        self._radius = (0.0, 0.0)
        self._max_iterations = 50
        self._probability = 0.99
        self._optimize = True
        self._axis = (0.0, 0.0, 0.0)
        self._eps_angle = 0.0
        self._seed = 0
        self.iterations = 0

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setInputNormals(self, normals):
        self._normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 4).copy()

    def setModelType(self, model: int):
        if model not in (_lib.SACMODEL_NORMAL_PLANE, _lib.SACMODEL_CYLINDER):
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "setModelType: SACMODEL_NORMAL_PLANE or SACMODEL_CYLINDER")
        self._model = int(model)

    def getModelType(self) -> int:
        return self._model

    def setMethodType(self, method: int):
        if method != _lib.SAC_RANSAC:
            raise IcpGpuError(_lib.ERR_UNSUPPORTED, "setMethodType: SAC_RANSAC is the only method")

    def getMethodType(self) -> int:
        return _lib.SAC_RANSAC

    def setDistanceThreshold(self, threshold: float):
        self._threshold = float(threshold)

    def getDistanceThreshold(self) -> float:
        return self._threshold

    def setNormalDistanceWeight(self, weight: float):
        self._weight = float(weight)

    def getNormalDistanceWeight(self) -> float:
        return self._weight

    def setRadiusLimits(self, radius_min: float, radius_max: float):
        self._radius = (float(radius_min), float(radius_max))

    def getRadiusLimits(self) -> tuple:
        return self._radius

    def setMaxIterations(self, max_iterations: int):
        self._max_iterations = int(max_iterations)

    def getMaxIterations(self) -> int:
        return self._max_iterations

    def setProbability(self, probability: float):
        self._probability = float(probability)

    def getProbability(self) -> float:
        return self._probability

    def setOptimizeCoefficients(self, optimize: bool):
        self._optimize = bool(optimize)

    def getOptimizeCoefficients(self) -> bool:
        return self._optimize

    def setAxis(self, axis):
        self._axis = tuple(float(v) for v in np.asarray(axis, np.float64).reshape(3))

    def getAxis(self) -> tuple:
        return self._axis

    def setEpsAngle(self, eps_angle: float):
        self._eps_angle = float(eps_angle)

    def getEpsAngle(self) -> float:
        return self._eps_angle

    def setSeed(self, seed: int):
        """NOT a PCL method: the counter-based generator's seed (PCL seeds rand() with a constant)."""
        self._seed = int(seed)

    def segment(self) -> tuple:
        if self._input is None or self._normals is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "segment: setInputCloud and setInputNormals first")
        if self._normals.shape[0] != self._input.shape[0]:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, "segment: %d normals for %d points" % (self._normals.shape[0], self._input.shape[0]))
        self._ctx.search_set_input(self._input)
        axis = self._axis if self._model == _lib.SACMODEL_CYLINDER and any(v != 0.0 for v in self._axis) else None
        inliers, coeff, self.iterations, found = self._ctx.sac_segmentation_from_normals(
            self._model, self._normals, self._threshold, self._weight, self._radius[0], self._radius[1], self._max_iterations, self._probability,
            self._seed, self._optimize, axis, self._eps_angle)
        if not found:
            return np.empty(0, np.int32), np.empty(0, np.float32)
        return inliers, coeff

    def extractCloud(self, negative: bool = False) -> np.ndarray:
        """NOT a PCL method: the input's inliers (negative: the others) of the last segment(), in cloud order."""
        return self._ctx.sac_extract(negative)


class ProgressiveMorphologicalFilter:
    """pcl::ProgressiveMorphologicalFilter<PointXYZ>-shaped front end (include/icpgpu.h, "ground filter"): setInputCloud,
    setMaxWindowSize, setSlope, setMaxDistance, setInitialDistance, setCellSize, setBase, setExponential and
    extract() -> the ground's indices (int32, ascending).  The defaults are PCL's (33, 0.7, 10.0, 0.15, 1.0, 2.0, true).  After an
    extract, `last` holds everything Context.progressive_morphological_filter returned and extractCloud(negative) is
    pcl::ExtractIndices over it.  setIndices is not provided."""

    def __init__(self, device_id: int = 0):
        self._ctx = Context(device_id)
        self._input = None
        self._max_window_size = 33
        self._slope = 0.7
        self._max_distance = 10.0
        self._initial_distance = 0.15
        self._cell_size = 1.0
        self._base = 2.0
        self._exponential = True
        self.last = None

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setMaxWindowSize(self, max_window_size: int):
        self._max_window_size = int(max_window_size)

    def getMaxWindowSize(self) -> int:
        return self._max_window_size

    def setSlope(self, slope: float):
        self._slope = float(slope)

    def getSlope(self) -> float:
        return self._slope

    def setMaxDistance(self, max_distance: float):
        self._max_distance = float(max_distance)

    def getMaxDistance(self) -> float:
        return self._max_distance

    def setInitialDistance(self, initial_distance: float):
        self._initial_distance = float(initial_distance)

    def getInitialDistance(self) -> float:
        return self._initial_distance

    def setCellSize(self, cell_size: float):
        self._cell_size = float(cell_size)

    def getCellSize(self) -> float:
        return self._cell_size

    def setBase(self, base: float):
        self._base = float(base)

    def getBase(self) -> float:
        return self._base

    def setExponential(self, exponential: bool):
        self._exponential = bool(exponential)

    def getExponential(self) -> bool:
        return self._exponential

    def extract(self) -> np.ndarray:
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "extract: setInputCloud first")
        self._ctx.search_set_input(self._input)
        self.last = self._ctx.progressive_morphological_filter(self._max_window_size, self._slope, self._initial_distance, self._max_distance,
                                                               self._cell_size, self._base, self._exponential)
        return self.last["ground"]

    def extractCloud(self, negative: bool = False) -> np.ndarray:
        """NOT a PCL method: the input's ground points (negative: the others) of the last extract(), in cloud order."""
        if self.last is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "extractCloud: extract first")
        return self._ctx.pmf_extract(negative)


class ExtractIndices:
    """pcl::ExtractIndices<PointXYZ>-shaped front end: setInputCloud, setIndices, setNegative, filter() -> the cloud's points whose
    index is (negative: is not) among the indices, in cloud order.  A plain host selection."""

    def __init__(self):
        self._input = None
        self._indices = np.empty(0, np.int64)
        self._negative = False

    def setInputCloud(self, cloud):
        self._input = _as_cloud(cloud).copy()

    def setIndices(self, indices):
        self._indices = np.asarray(indices, np.int64).reshape(-1)

    def setNegative(self, negative: bool):
        self._negative = bool(negative)

    def getNegative(self) -> bool:
        return self._negative

    def filter(self) -> np.ndarray:
        if self._input is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "filter: setInputCloud first")
        n = self._input.shape[0]
        if self._indices.size and (self._indices.min() < 0 or self._indices.max() >= n):
            raise IcpGpuError(_lib.ERR_INVALID_ARG, "filter: an index outside the cloud")
        mask = np.zeros(n, bool)
        mask[self._indices] = True
        return self._input[~mask if self._negative else mask].copy()


class IterativeClosestPoint:
    """pcl::IterativeClosestPoint<PointXYZ, PointXYZ>-shaped front end (same method names as the reference uses):
    point-to-point ICP, the solver BASELINE.json's north_star specifies.  The class the reference literally instantiates
    is GeneralizedIterativeClosestPoint below; each mirror keeps the semantics of the PCL class it is named after."""

    _shared_ctx: dict = {}
    METHOD = _lib.P2P_SVD

    def __init__(self, device_id: int = 0, method: int | None = None):
        method = self.METHOD if method is None else method
        # the reference builds a fresh registration object per scan (icp_odometer.cpp:188); the GPU context is
        # cached per device so that doing the same here costs nothing
        ctx = IterativeClosestPoint._shared_ctx.get(device_id)
        if ctx is None or ctx._h is None:
            ctx = Context(device_id)
            IterativeClosestPoint._shared_ctx[device_id] = ctx
        self._ctx = ctx
        self._params = ctx.default_params()
        self._params.method = method
        self._source = None
        self._target = None
        self._result = None
        self._fitness = None
        self._rejectors = []
        self._reciprocal = False
        self._source_normals = None
        self._target_normals = None

    # setters used by the reference -----------------------------------------------------------------------------
    def setMaximumIterations(self, n):           # icp_odometer.cpp:189 (passes a double constant)
        self._params.max_iterations = int(n)

    def setTransformationEpsilon(self, eps):     # icp_odometer.cpp:190
        self._params.transformation_epsilon = float(eps)

    def setMaxCorrespondenceDistance(self, d):   # icp_odometer.cpp:191
        self._params.max_correspondence_distance = float(d)

    def setRANSACIterations(self, n):            # icp_odometer.cpp:192 -- always 0 in the reference
        if int(n) != 0:
            raise NotImplementedError("RANSAC outlier rejection is not on the reference's path (always 0)")

    def setEuclideanFitnessEpsilon(self, eps):
        self._params.euclidean_fitness_epsilon = float(eps)

    # pcl::Registration's rejector chain (the library ignores it for GICP and NDT, as PCL's classes do)
    def addCorrespondenceRejector(self, rejector):
        if len(self._rejectors) >= _lib.MAX_REJECTORS:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, f"at most {_lib.MAX_REJECTORS} correspondence rejectors")
        self._rejectors.append(rejector)

    def getCorrespondenceRejectors(self):
        return list(self._rejectors)

    def removeCorrespondenceRejector(self, i) -> bool:
        if i >= len(self._rejectors):
            return False
        del self._rejectors[i]
        return True

    def clearCorrespondenceRejectors(self):
        self._rejectors = []

    # pcl::Registration::setUseReciprocalCorrespondences (read by IterativeClosestPoint and ...WithNormals only, as in PCL: the
    # GICP and NDT mirrors store the flag and the library ignores it for their methods)
    def setUseReciprocalCorrespondences(self, on: bool):
        self._reciprocal = bool(on)

    def getUseReciprocalCorrespondences(self) -> bool:
        return self._reciprocal

    def _set_chain(self):
        self._ctx.set_correspondence_rejectors([r._entry() for r in self._rejectors])
        self._ctx.set_reciprocal_correspondences(self._reciprocal)

    def _take_rejector_stats(self):
        for r, s in zip(self._rejectors, self._ctx.rejector_stats()):
            if isinstance(r, CorrespondenceRejectorMedianDistance):
                r._median = float(s["cut"])
        sac = [r for r in self._rejectors if isinstance(r, CorrespondenceRejectorSampleConsensus)]
        if sac:  # (the fetch is of the LAST such stage's last run)
            try:
                sac[-1]._best_T = self._ctx.rejector_sac_fetch(per_hypothesis=False)["best_T"]
            except IcpGpuError:  # (GICP and NDT ignore the chain: no run)
                pass

    def setInputSource(self, cloud):             # icp_odometer.cpp:193
        self._source = _as_cloud(cloud)
        self._source_normals = None

    def setInputTarget(self, cloud):             # icp_odometer.cpp:194
        self._target = _as_cloud(cloud)
        self._target_normals = None

    # the clouds' normals as PointNormal clouds carry them (after setInputSource / setInputTarget: a new cloud drops the normals it
    # had); read by the surface-normal rejector and by IterativeClosestPointWithNormals, estimated on the device where missing
    def setSourceNormals(self, normals):
        self._source_normals = None if normals is None else _as_cloud(normals)

    def setTargetNormals(self, normals):
        self._target_normals = None if normals is None else _as_cloud(normals)

    def _upload(self):
        self._ctx.set_params(self._params)
        self._ctx.set_source(self._source)
        self._ctx.set_target(self._target)
        if self._source_normals is not None:
            self._ctx.set_source_normals(self._source_normals)
        if self._target_normals is not None:
            self._ctx.set_target_normals(self._target_normals)   # (after set_target: a new target drops the normals it had)

    # the call ------------------------------------------------------------------------------------------------------
    def align(self, guess=None) -> np.ndarray:   # icp_odometer.cpp:198; returns the aligned source cloud
        if self._source is None or self._target is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "align: setInputSource/setInputTarget first")
        self._upload()
        self._set_chain()
        self._result = self._ctx.align(guess=guess, want_cloud=True)
        self._take_rejector_stats()
        self._ctx._last_user = self          # objects of one device share the cached context (see getFitnessScore)
        return self._result["cloud"]

    def getFinalTransformation(self) -> np.ndarray:   # icp_odometer.cpp:199
        return np.eye(4, dtype=np.float32) if self._result is None else self._result["T"]

    def hasConverged(self) -> bool:                   # icp_odometer.cpp:201
        return bool(self._result and self._result["converged"])

    def getFitnessScore(self, max_range: float = float(np.finfo(np.float64).max)) -> float:   # icp_odometer.cpp:201
        if self._result is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "getFitnessScore before align")
        if getattr(self._ctx, "_last_user", None) is not self:
            # another registration object used the shared context since this one's align: put this object's clouds back
            # and evaluate under ITS transform (kernel-level entry points), not under whatever the context did last
            self._ctx.set_params(self._params)
            self._ctx.set_source(self._source)
            self._ctx.set_target(self._target)
            self._ctx.nn(self._result["T"])
            s = self._ctx.reduce(self._result["T"], 1e18 if max_range >= 1e36 else float(np.sqrt(max_range)))
            self._ctx._last_user = None
            return float(s[16] / s[0]) if s[0] > 0 else float(np.finfo(np.float64).max)
        return self._ctx.fitness(max_range)

    @property
    def result(self):
        return self._result


class GeneralizedIterativeClosestPoint(IterativeClosestPoint):
    """pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ>-shaped front end: the class the reference instantiates at
    icp_odometer.cpp:188 and octree_mapper.cpp:104 (plane-to-plane cost, BFGS inner solver, PCL's constructor defaults)."""

    METHOD = _lib.GICP

    def setQuadraticInnerSolver(self, on: bool):
        """NOT a PCL method (the C++ shim has the same one): the inner minimisation on the quadratic form of each outer iteration,
        icpgpu_params.gicp_inner -- faster, within tolerance of the default's result instead of on its bits (include/icpgpu.h)."""
        self._params.gicp_inner = _lib.GICP_INNER_QUADRATIC if on else _lib.GICP_INNER_EXACT


class NormalDistributionsTransform(IterativeClosestPoint):
    """pcl::NormalDistributionsTransform<PointXYZ, PointXYZ>-shaped front end: the target's points in cells of `resolution` with one
    Gaussian each, a Newton loop on the Gauss-fitted score (include/icpgpu.h, ICPGPU_NDT).  PCL's constructor defaults: resolution 1.0,
    step size 0.1, outlier ratio 0.55, 35 iterations, transformation epsilon 0.1."""

    METHOD = _lib.NDT

    def __init__(self, device_id: int = 0, method: int | None = None):
        super().__init__(device_id, method)
        self._params.max_iterations = 35
        self._params.transformation_epsilon = 0.1
        self._ndt = dict(resolution=1.0, step_size=0.1, outlier_ratio=0.55, line_search=_lib.NDT_LINE_SEARCH_PCL18)
        self._probability = float("nan")

    def setMoreThuenteLineSearch(self, on: bool):
        """NOT a PCL method (the C++ shim has the same one): the More-Thuente line search with its loop running instead of PCL 1.8's
        clamped Newton step (icpgpu_set_ndt_line_search; include/icpgpu.h)."""
        self._ndt["line_search"] = _lib.NDT_LINE_SEARCH_MORE_THUENTE if on else _lib.NDT_LINE_SEARCH_PCL18

    def getMoreThuenteLineSearch(self) -> bool:
        return self._ndt["line_search"] == _lib.NDT_LINE_SEARCH_MORE_THUENTE

    def setResolution(self, r):
        self._ndt["resolution"] = float(r)

    def getResolution(self) -> float:
        return self._ndt["resolution"]

    def setStepSize(self, s):
        self._ndt["step_size"] = float(s)

    def getStepSize(self) -> float:
        return self._ndt["step_size"]

    def setOulierRatio(self, r):                 # (PCL's spelling)
        self._ndt["outlier_ratio"] = float(r)

    def getOulierRatio(self) -> float:
        return self._ndt["outlier_ratio"]

    def align(self, guess=None) -> np.ndarray:
        if self._source is None or self._target is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "align: setInputSource/setInputTarget first")
        self._ctx.set_ndt_params(**self._ndt)
        out = super().align(guess)
        self._probability = self._ctx.ndt_transformation_probability()
        return out

    def getTransformationProbability(self) -> float:
        return self._probability

    def getFinalNumIteration(self) -> int:
        return 0 if self._result is None else int(self._result["iterations"])


class IterativeClosestPointWithNormals(IterativeClosestPoint):
    """pcl::IterativeClosestPointWithNormals<PointNormal, PointNormal>-shaped front end (TransformationEstimationPointToPlaneLLS): the
    point-to-point loop with the linearised point-to-plane solve.  setInputTarget(cloud, normals) hands the target's normals over as
    a PointNormal cloud carries them; without them the target's normals are estimated on the device (GICP's plane: include/icpgpu.h,
    ICPGPU_P2PLANE -- not pcl::NormalEstimation's: the NormalEstimation class above computes those)."""

    METHOD = _lib.P2PLANE

    def __init__(self, device_id: int = 0, method: int | None = None):
        super().__init__(device_id, method)
        self._symmetric = False
        self._enforce_same_direction = True

    def setInputTarget(self, cloud, normals=None):
        super().setInputTarget(cloud)
        self.setTargetNormals(normals)

    # TransformationEstimationSymmetricPointToPlaneLLS in place of ...PointToPlaneLLS (PCL >= 1.10)
    def setUseSymmetricObjective(self, on: bool):
        self._symmetric = bool(on)

    def getUseSymmetricObjective(self) -> bool:
        return self._symmetric

    def setEnforceSameDirectionNormals(self, on: bool):
        self._enforce_same_direction = bool(on)

    def getEnforceSameDirectionNormals(self) -> bool:
        return self._enforce_same_direction

    def _upload(self):
        super()._upload()
        self._ctx.set_p2plane_symmetric(self._symmetric, self._enforce_same_direction)

    def getFitnessScore(self, max_range: float = float(np.finfo(np.float64).max)) -> float:
        if self._result is not None and getattr(self._ctx, "_last_user", None) is not self:
            self._upload()                       # the base class puts the clouds back; the normals go with the target
            self._ctx._last_user = None
            self._ctx.nn(self._result["T"])
            s = self._ctx.reduce(self._result["T"], 1e18 if max_range >= 1e36 else float(np.sqrt(max_range)))
            return float(s[16] / s[0]) if s[0] > 0 else float(np.finfo(np.float64).max)
        return super().getFitnessScore(max_range)
