"""MI355X-native scan-matching core behind the reference's VoxelGrid /
CloudMatcher / Pose3D interface (vovo-4K/lidar_odometry_demo:
src/voxel_grid.h, src/cloud_matcher.h, src/pose_3d.h).

Python mirror of the reference classes over the C ABI of
include/lidar_odometry_amd.h -- same names, argument meaning and error
behaviour, so parity tests read like the reference's own tests.  All compute
runs in the HIP library; there is no CPU path in this package.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import LomError  # noqa: F401

__all__ = ["Pose3D", "VoxelGrid", "CloudMatcher", "ScanContext", "LidarOdometry", "transform_points", "pointTimeNormalize",
           "transformNonRigid", "rangeFilter", "classify", "loadPCDFile", "fromROSMsg", "toROSMsg", "estimateNormals", "FrontEnd", "classifyNeighbourhood", "neighbourhoodParams", "carveParams", "voteParams", "LomError", "capi", "quality_report",
           "quality_report_batch", "pose_lattice", "PoseGraph", "graphParams", "graph_information_from_quality"]


class Pose3D:
    """reference src/pose_3d.h:10-59 (f32 translation + wxyz quaternion)."""

    def __init__(self, translation=(0, 0, 0), rotation_wxyz=(1, 0, 0, 0)):
        self.translation = np.asarray(translation, dtype=np.float32).copy()
        self.rotation = np.asarray(rotation_wxyz, dtype=np.float32).copy()

    def _c(self):
        return capi.Pose(capi.f3(self.translation), capi.f4(self.rotation))

    @staticmethod
    def _from(c):
        return Pose3D(np.array(c.t[:], np.float32), np.array(c.q[:], np.float32))

    def compose(self, another):          # pose_3d.h:29-32
        o = capi.Pose()
        capi.lib().lom_pose_compose(C.byref(self._c()), C.byref(another._c()), C.byref(o))
        return Pose3D._from(o)

    def inverse(self):                   # pose_3d.h:34-39
        o = capi.Pose()
        capi.lib().lom_pose_inverse(C.byref(self._c()), C.byref(o))
        return Pose3D._from(o)

    def relativeTo(self, target):        # pose_3d.h:23-27
        o = capi.Pose()
        capi.lib().lom_pose_relative_to(C.byref(self._c()), C.byref(target._c()), C.byref(o))
        return Pose3D._from(o)

    def rotationMatrix(self):            # pose_3d.h:41-43
        R = (C.c_float * 9)()
        capi.lib().lom_pose_rotation_matrix(C.byref(self._c()), R)
        return np.array(R[:], np.float32).reshape(3, 3)

    def __repr__(self):
        return f"Pose3D(t={self.translation.tolist()}, q_wxyz={self.rotation.tolist()})"


def transform_points(pose, xyz, normals=None):
    """CloudTransformer::transform / transformWithNormals (src/utils/cloud_transform.h:43-97)."""
    xyz = capi.xyz_array(xyz)
    out = np.empty_like(xyz)
    nout = None
    if normals is not None:
        normals = capi.xyz_array(normals)
        nout = np.empty_like(normals)
    capi.check(capi.lib().lom_transform_points(
        C.byref(pose._c()), xyz.ctypes.data, normals.ctypes.data if normals is not None else None,
        len(xyz), 12, out.ctypes.data, nout.ctypes.data if normals is not None else None, 12))
    return (out, nout) if normals is not None else out


class VoxelGrid:
    """reference src/voxel_grid.h:17-257, device-resident."""

    def __init__(self, voxel_size=0.5, max_points=10, capacity_hint=0, device=0):
        h = C.c_void_p()
        rc = capi.lib().lom_map_create(float(voxel_size), int(max_points), int(capacity_hint), int(device),
                                       C.byref(h))
        if rc != 0:
            capi.check(rc, None)
        self._h = h
        self.max_points = int(max_points)
        self.device = int(device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and capi is not None:          # at interpreter shutdown the module may already be gone
            capi.lib().lom_map_destroy(h)
            self._h = None

    close = __del__

    @property
    def handle(self):
        return self._h

    def setOption(self, option, value):
        """lom_map_set_option: run-time switches of the handle (capi.OPT_*)."""
        capi.check(capi.lib().lom_map_set_option(self._h, int(option), int(value)), self._h)

    def debugCounter(self, which=capi.COUNTER_GRID_REDOS):
        return capi.check(capi.lib().lom_map_debug_counter(self._h, int(which)), self._h)

    def replayedIterations(self):
        """Outer iterations of the last device-resident align on this grid that the replay fold (capi.OPT_REPLAY_FOLD)
        accounted for without running them."""
        return capi.replayed_iterations(self._h)

    def setMaxPoints(self, max_points):                    # voxel_grid.h:56-59
        capi.check(capi.lib().lom_map_set_max_points(self._h, int(max_points)), self._h)
        self.max_points = int(max_points)

    def setVoxelSize(self, voxel_size):                    # voxel_grid.h:61-66 (clears)
        capi.check(capi.lib().lom_map_clear(self._h, float(voxel_size)), self._h)

    def addCloud(self, xyz, normals):                      # voxel_grid.h:77-93
        xyz, normals = capi.xyz_array(xyz), capi.xyz_array(normals)
        if len(xyz) != len(normals):
            raise ValueError("xyz and normals differ in length")
        capi.check(capi.lib().lom_map_add_points(self._h, xyz.ctypes.data, normals.ctypes.data, len(xyz), 12),
                   self._h)

    def addCloudInterleaved(self, records, stride_bytes, normal_offset_bytes=None):
        """pcl-style records (e.g. 48-byte PointNormal: xyz at 0, normal at 16) without repacking."""
        buf = np.ascontiguousarray(records)
        n = buf.nbytes // stride_bytes
        base = buf.ctypes.data
        nrm = base + normal_offset_bytes if normal_offset_bytes is not None else None
        capi.check(capi.lib().lom_map_add_points(self._h, base, nrm, n, stride_bytes), self._h)

    def addCloudWithoutNormals(self, xyz):                 # voxel_grid.h:95-110
        xyz = capi.xyz_array(xyz)
        capi.check(capi.lib().lom_map_add_points(self._h, xyz.ctypes.data, None, len(xyz), 12), self._h)

    def addCloudDevice(self, d_xyz_ptr, d_nrm_ptr, n, stride_bytes=12):
        capi.check(capi.lib().lom_map_add_points_device(self._h, d_xyz_ptr, d_nrm_ptr, int(n), int(stride_bytes)),
                   self._h)

    def assemble(self, archive, ids, poses, centre=None, radius=0.0):
        """lom_map_assemble: the scans `ids` of the ScanArchive at `poses` ((n, 7) float64: t, then q wxyz) into this map
        in call order, as one addCloud of their concatenation; with radius > 0 only the points within it of `centre`.
        Returns the stats as a dict."""
        ids, p = _assemble_args(ids, poses)
        prm = None
        if centre is not None or radius > 0.0:
            prm = capi.AssembleParams(capi.f3((0, 0, 0) if centre is None else centre), float(radius))
        st = capi.AssembleStats()
        rc = capi.lib().lom_map_assemble(self._h, archive.handle, ids.ctypes.data, p.ctypes.data, len(ids),
                                         C.byref(prm) if prm is not None else None, C.byref(st))
        if rc != 0:
            text = capi.lib().lom_archive_last_error(archive.handle)
            raise LomError(int(rc), text.decode() if text else "lom_map_assemble")
        return st.asdict()

    def size(self):                                        # voxel_grid.h:248-251
        return int(capi.check(capi.lib().lom_map_size(self._h), self._h))

    def pointCount(self):
        return int(capi.check(capi.lib().lom_map_point_count(self._h), self._h))

    def _export(self, mode, want_normals):
        n = capi.check(capi.lib().lom_map_export(self._h, mode, None, None, 0), self._h)
        xyz = np.empty((n, 3), np.float32)
        nrm = np.empty((n, 3), np.float32) if want_normals else None
        if n:
            capi.check(capi.lib().lom_map_export(self._h, mode, xyz.ctypes.data,
                                                 nrm.ctypes.data if want_normals else None, n), self._h)
        return xyz, nrm

    def getCloud(self):                                    # voxel_grid.h:112-130
        return self._export(capi.EXPORT_FULL, True)

    def getCloudWithoutNormals(self):                      # voxel_grid.h:133-147
        return self._export(capi.EXPORT_FULL_NO_NORMALS, False)[0]

    def getSparseCloudWithoutNormals(self):                # voxel_grid.h:150-162
        return self._export(capi.EXPORT_FIRST_PER_VOXEL, False)[0]

    def downsample(self, xyz, normals, voxel_size):
        """VoxelGrid(voxel_size, 1).addCloud(...).getCloud() in one fused pass (lidar_odometry.cpp:37-47);
        this grid is only the workspace and is left empty."""
        xyz = capi.xyz_array(xyz)
        normals = capi.xyz_array(normals) if normals is not None else None
        oxyz = np.empty_like(xyz)
        onrm = np.empty_like(xyz)
        n = capi.check(capi.lib().lom_voxel_downsample(
            self._h, float(voxel_size), xyz.ctypes.data, normals.ctypes.data if normals is not None else None,
            len(xyz), 12, oxyz.ctypes.data, onrm.ctypes.data, len(xyz)), self._h)
        return oxyz[:n].copy(), onrm[:n].copy()

    def radiusCleanup(self, point, radius):                # voxel_grid.h:236-246
        capi.check(capi.lib().lom_map_radius_cleanup(self._h, capi.f3(point), float(radius)), self._h)

    def radiusCleanupAfterAlign(self, radius):
        """Arm the next align on this grid to enqueue the scan of radiusCleanup(<its result translation>, radius) behind
        itself (lidar_odometry.cpp:65-67's pattern); the radiusCleanup that follows takes it if its arguments match."""
        capi.check(capi.lib().lom_map_radius_cleanup_after_align(self._h, float(radius)), self._h)

    def carveRays(self, origin, xyz, params, device_ptr=None, n=None, stride_bytes=12):
        """lom_map_carve_rays ("ray carving" in the header; not in the reference): erase the voxels that at least
        params.min_crossings rays origin -> xyz[i] of this call pass through and no xyz[i] falls into.  Returns the call's
        capi.CarveStats as a dict.  device_ptr / n: the endpoints are in device memory (lom_map_carve_rays_device)."""
        p = carveParams(params)
        st = capi.CarveStats()
        if device_ptr is not None:
            rc = capi.lib().lom_map_carve_rays_device(self._h, capi.f3(origin), device_ptr, int(n), int(stride_bytes),
                                                      C.byref(p), C.byref(st))
        else:
            xyz = capi.xyz_array(xyz)
            rc = capi.lib().lom_map_carve_rays(self._h, capi.f3(origin), xyz.ctypes.data, len(xyz), 12, C.byref(p),
                                               C.byref(st))
        capi.check(rc, self._h)
        return st.asdict()

    def carveCounts(self, origin, xyz, params):
        """lom_map_carve_counts: what carveRays would decide on, nothing erased -- (cross uint32, hit uint8) per live
        voxel in the export's order."""
        p = carveParams(params)
        xyz = capi.xyz_array(xyz)
        nv = self.size()
        cross, hit = np.zeros(nv, np.uint32), np.zeros(nv, np.uint8)
        got = capi.check(capi.lib().lom_map_carve_counts(self._h, capi.f3(origin), xyz.ctypes.data, len(xyz), 12,
                                                         C.byref(p), cross.ctypes.data, hit.ctypes.data, nv), self._h)
        if got != nv:
            raise LomError(capi.ERR_STATE, "lom_map_carve_counts: voxel count changed")
        return cross, hit

    def carveScans(self, archive, ids, poses, params):
        """lom_map_carve_scans ("scan votes" in the header; not in the reference): the scans `ids` of the ScanArchive at
        `poses` vote on this map's voxels -- seen, or seen through -- and the voxels with at least params.min_free_scans
        free votes and free >= params.free_per_seen * seen are erased.  Returns capi.VoteStats as a dict."""
        p = voteParams(params)
        ids, g = _assemble_args(ids, poses)
        st = capi.VoteStats()
        capi.check(capi.lib().lom_map_carve_scans(self._h, archive.handle, ids.ctypes.data, g.ctypes.data, len(ids),
                                                  C.byref(p), C.byref(st)), self._h)
        return st.asdict()

    def scanVotes(self, archive, ids, poses, params):
        """lom_map_scan_votes: what carveScans would decide on, nothing erased -- (free uint32, seen uint32) per live
        voxel in the export's order."""
        p = voteParams(params)
        ids, g = _assemble_args(ids, poses)
        nv = self.size()
        free, seen = np.zeros(nv, np.uint32), np.zeros(nv, np.uint32)
        got = capi.check(capi.lib().lom_map_scan_votes(self._h, archive.handle, ids.ctypes.data, g.ctypes.data, len(ids),
                                                       C.byref(p), free.ctypes.data, seen.ctypes.data, nv), self._h)
        if got != nv:
            raise LomError(capi.ERR_STATE, "lom_map_scan_votes: voxel count changed")
        return free, seen

    def findMatchingPairs(self, xyz, transform, max_correspondence_distance=0.3):
        """voxel_grid.h:206-234; one entry per source point in source order (index < 0: no match)."""
        xyz = capi.xyz_array(xyz)
        out = np.zeros(len(xyz), capi.CORR_DTYPE)
        capi.check(capi.lib().lom_match_find_pairs(
            self._h, xyz.ctypes.data, len(xyz), 12, capi.f3(transform.translation), capi.f4(transform.rotation),
            float(max_correspondence_distance), out.ctypes.data), self._h)
        return out

    def findMatchingPairsSq(self, xyz, transform, max_correspondence_distance_sq):
        """The search with the squared threshold as getCorrespondence takes it (voxel_grid.h:164: a double)."""
        xyz = capi.xyz_array(xyz)
        out = np.zeros(len(xyz), capi.CORR_DTYPE)
        capi.check(capi.lib().lom_match_find_pairs_sq(
            self._h, xyz.ctypes.data, len(xyz), 12, capi.f3(transform.translation), capi.f4(transform.rotation),
            float(max_correspondence_distance_sq), out.ctypes.data), self._h)
        return out

    def findMatchingPairsAfter(self, xyz, previous_transform, transform, max_correspondence_distance=0.3):
        """Parity entry: the search at `transform` with the temporal pruning bound taken from a search at
        `previous_transform` (what outer iterations >= 2 of an align run); equals findMatchingPairs(xyz, transform)."""
        xyz = capi.xyz_array(xyz)
        out = np.zeros(len(xyz), capi.CORR_DTYPE)
        capi.check(capi.lib().lom_debug_find_pairs_after(
            self._h, xyz.ctypes.data, len(xyz), 12, capi.f3(previous_transform.translation),
            capi.f4(previous_transform.rotation), capi.f3(transform.translation), capi.f4(transform.rotation),
            float(max_correspondence_distance), out.ctypes.data), self._h)
        return out

    def getCorrespondence(self, query, max_correspondence_distance_sq):
        """voxel_grid.h:164-204 for a single already-transformed f32 query point; the threshold is the reference's
        `double max_correspondence_distance_sq`, handed over as it is."""
        return self.findMatchingPairsSq(np.asarray(query, np.float32).reshape(1, 3), Pose3D(), max_correspondence_distance_sq)[0]

    def profileMatch(self, d_src_ptr, n, transform, max_correspondence_distance=0.3, reps=20, stride_bytes=12):
        """(average k_match launch duration [us] over a back-to-back train under one event pair, algorithmic
        bytes per launch, bytes the kernel requests per launch, average of the same launches with one event
        pair each [us])."""
        us, by, rq, pr = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        capi.check(capi.lib().lom_profile_match(
            self._h, d_src_ptr, int(n), int(stride_bytes), capi.f3(transform.translation),
            capi.f4(transform.rotation), float(max_correspondence_distance), int(reps), C.byref(us), C.byref(by),
            C.byref(rq), C.byref(pr)), self._h)
        return us.value, by.value, rq.value, pr.value

    def profileInsert(self, d_xyz_ptr, d_nrm_ptr, n, stride_bytes=12):
        """addCloud of device-resident points, all kernels of the insert under one HIP event pair: microseconds."""
        us = C.c_double()
        capi.check(capi.lib().lom_profile_insert(self._h, d_xyz_ptr, d_nrm_ptr, int(n), int(stride_bytes), C.byref(us)),
                   self._h)
        return us.value

    def quality(self, xyz, transform, max_correspondence_distance=0.3, min_eig_t=0.0, min_eig_r=0.0, residuals=False):
        """lom_match_quality: see quality_report()."""
        return quality_report(self, xyz, transform, max_correspondence_distance, min_eig_t, min_eig_r, residuals)

    def qualityBatch(self, clouds_or_cloud, poses, max_correspondence_distance=0.3, min_eig_t=0.0, min_eig_r=0.0,
                     sums_only=False):
        """lom_match_quality_batch: see quality_report_batch()."""
        return quality_report_batch(self, clouds_or_cloud, poses, max_correspondence_distance, min_eig_t, min_eig_r,
                                    sums_only)

    def setProfiling(self, period):
        """HIP event pairs around the correspondence launches of every `period`-th align (True = 1, False = 0)."""
        capi.check(capi.lib().lom_map_set_profiling(self._h, int(period)), self._h)


class ScanContext:
    """lom_scan: what a further caller of ONE keyframe owns (stream, per-scan buffers, solve state) -- the reference's
    search and align take the grid by const reference (voxel_grid.h:206, cloud_matcher.h:15), so several threads may
    align against one keyframe at a time.  Pass it to CloudMatcher.align / alignDevice / align_repeat in place of the
    grid.  One caller per context; nobody changes the grid while contexts are in use."""

    def __init__(self, keyframe, partition=None):
        """partition = (index, count): the context's stream runs on that slice of the GPU's compute units
        (lom_scan_create_on_partition) -- for `count` callers side by side."""
        h = C.c_void_p()
        if partition is None:
            capi.check(capi.lib().lom_scan_create(keyframe.handle, C.byref(h)), keyframe.handle)
        else:
            capi.check(capi.lib().lom_scan_create_on_partition(keyframe.handle, int(partition[0]), int(partition[1]),
                                                               C.byref(h)), keyframe.handle)
        self._h = h
        self.keyframe = keyframe          # keeps the grid alive

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and capi is not None:
            capi.lib().lom_scan_destroy(h)
            self._h = None

    close = __del__

    @property
    def handle(self):
        return self._h

    def setOption(self, option, value):
        if capi.lib().lom_scan_set_option(self._h, int(option), int(value)) != 0:
            raise LomError(-1, "lom_scan_set_option")

    def _check(self, rc):
        if rc < 0:
            text = capi.lib().lom_scan_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "")
        return rc

    def quality(self, xyz, transform, max_correspondence_distance=0.3, min_eig_t=0.0, min_eig_r=0.0, residuals=False):
        """lom_scan_quality: see quality_report()."""
        return quality_report(self, xyz, transform, max_correspondence_distance, min_eig_t, min_eig_r, residuals)

    def qualityBatch(self, clouds_or_cloud, poses, max_correspondence_distance=0.3, min_eig_t=0.0, min_eig_r=0.0,
                     sums_only=False):
        """lom_scan_quality_batch: see quality_report_batch()."""
        return quality_report_batch(self, clouds_or_cloud, poses, max_correspondence_distance, min_eig_t, min_eig_r,
                                    sums_only)


def _align_entry(keyframe, name):
    """(function, checker) for a grid or a scan context"""
    L = capi.lib()
    if isinstance(keyframe, ScanContext):
        return getattr(L, "lom_scan_" + name), keyframe._check
    return getattr(L, "lom_match_" + name), (lambda rc: capi.check(rc, keyframe.handle))


def quality_report(keyframe, xyz, transform, max_correspondence_distance=0.3, min_eig_t=0.0, min_eig_r=0.0,
                   residuals=False, raw=False):
    """How good is `transform` for `xyz` against `keyframe` (a VoxelGrid or a ScanContext)?  One search at the pose as
    given, one evaluation of the align's residuals and Jacobians over its winners (lom_match_quality): a dict of the
    fields of lom_quality_report -- counts, overlap, rmse, the 6x6 information matrix (rotation first, half-angle
    tangent), the spectra of its translation and rotation blocks with the number of eigenvalues below the caller's
    thresholds, and the 6x6 covariance in nav_msgs order (zeros and covariance_valid = 0 where the geometry is
    degenerate).  residuals=True adds "residuals": the signed point-to-plane residual per source point, NaN where it
    has no correspondence.  raw=True returns the ctypes struct instead (its bytes compare exactly)."""
    xyz = capi.xyz_array(xyz)
    rep = capi.QualityReport()
    res = np.empty(len(xyz), np.float32) if residuals else None
    fn, chk = _align_entry(keyframe, "quality")
    chk(fn(keyframe.handle, xyz.ctypes.data if len(xyz) else None, len(xyz), 12, capi.f3(transform.translation),
           capi.f4(transform.rotation), float(max_correspondence_distance), float(min_eig_t), float(min_eig_r),
           C.byref(rep), res.ctypes.data if residuals and len(xyz) else None))
    if raw:
        return (rep, res) if residuals else rep
    out = rep.asdict()
    if residuals:
        out["residuals"] = res
    return out


def quality_problems(items):
    """A lom_quality_problem array from [(pointer or None, n, stride_bytes, pose), ...] (host or device pointers)."""
    problems = (capi.QualityProblem * max(len(items), 1))()
    for p, (ptr, n, stride_bytes, pose) in zip(problems, items):
        p.xyz = ptr
        p.n = int(n)
        p.stride_bytes = int(stride_bytes)
        p.t[:] = [float(v) for v in np.asarray(pose.translation, np.float32)]
        p.q_wxyz[:] = [float(v) for v in np.asarray(pose.rotation, np.float32)]
    return problems


def quality_report_batch(keyframe, clouds_or_cloud, poses, max_correspondence_distance=0.3, min_eig_t=0.0, min_eig_r=0.0,
                         sums_only=False, raw=False):
    """quality_report() for K candidates in ONE call (lom_match_quality_batch): one host wait whatever K is.
    `clouds_or_cloud`: one (n, 3) array scored at every pose of `poses` (the pose-lattice case: uploaded once), or a list
    of K arrays, one per pose (an array that appears several times is uploaded once).  Returns (reports, best): a list of
    K dicts as quality_report() returns them (raw=True: the ctypes array) and the index of the best candidate -- most
    valid correspondences, then lowest cost; -1 for K == 0.  sums_only=True: the (K, 36) array of the reduced values
    instead of the reports (lom_match_quality_batch_sums), best from them.  `keyframe`: a VoxelGrid or a ScanContext."""
    if isinstance(clouds_or_cloud, np.ndarray) and clouds_or_cloud.ndim == 2:
        one = capi.xyz_array(clouds_or_cloud)
        arrays = [one] * len(poses)
    else:
        if len(clouds_or_cloud) != len(poses):
            raise ValueError("one pose per cloud")
        arrays = [c if isinstance(c, np.ndarray) and c.dtype == np.float32 and c.ndim == 2 and c.shape[1] == 3 and
                  c.flags.c_contiguous else capi.xyz_array(c) for c in clouds_or_cloud]
    count = len(arrays)
    problems = quality_problems([(a.ctypes.data if len(a) else None, len(a), 12, g) for a, g in zip(arrays, poses)])
    if sums_only:
        sums = np.zeros((count, capi.NQSUMS), np.float64)
        fn, chk = _align_entry(keyframe, "quality_batch_sums")
        chk(fn(keyframe.handle, problems if count else None, count, float(max_correspondence_distance),
               sums.ctypes.data_as(C.POINTER(C.c_double)) if count else None))
        reps = (capi.QualityReport * max(count, 1))()
        for i in range(count):
            capi.check(capi.lib().lom_quality_from_sums(sums[i].ctypes.data_as(C.POINTER(C.c_double)), len(arrays[i]), 0.0,
                                                        0.0, C.byref(reps[i])))
        return sums, int(capi.lib().lom_quality_batch_best(reps, count))
    reps = (capi.QualityReport * max(count, 1))()
    best = C.c_int(-1)
    fn, chk = _align_entry(keyframe, "quality_batch")
    chk(fn(keyframe.handle, problems if count else None, count, float(max_correspondence_distance), float(min_eig_t),
           float(min_eig_r), reps if count else None, C.byref(best)))
    del arrays
    if raw:
        return reps, best.value
    return [reps[i].asdict() for i in range(count)], best.value


def pose_lattice(centre, half_extent_xyz, step_xyz, half_extent_yaw=0.0, step_yaw=0.0):
    """lom_pose_lattice: the poses of a lattice around `centre` -- per axis 2 * floor(half_extent / step) + 1 nodes (one
    where the step is <= 0 or the extent below it), translation offsets in the world frame, yaw about world Z applied
    from the left (radians); order: yaw outermost, then x, y, and z innermost, each ascending."""
    L = capi.lib()
    c = centre._c()
    he, st = capi.f3(half_extent_xyz), capi.f3(step_xyz)
    n = L.lom_pose_lattice(C.byref(c), he, st, float(half_extent_yaw), float(step_yaw), None, 0)
    if n < 0:
        raise LomError(int(n), "lom_pose_lattice")
    out = (capi.Pose * max(n, 1))()
    capi.check(L.lom_pose_lattice(C.byref(c), he, st, float(half_extent_yaw), float(step_yaw), out, n))
    return [Pose3D._from(out[i]) for i in range(n)]


def align_repeat(keyframe, d_src_ptr, n, position_guess, reps, stride_bytes=12):
    """`reps` back-to-back aligns of a device-resident scan issued from compiled code
    (lom_match_align_repeat): (pose of the last one, accumulated stats)."""
    ot, oq = (C.c_float * 3)(), (C.c_float * 4)()
    st = capi.AlignStats()
    fn, chk = _align_entry(keyframe, "align_repeat")
    chk(fn(keyframe.handle, d_src_ptr, int(n), int(stride_bytes), capi.f3(position_guess.translation),
           capi.f4(position_guess.rotation), int(reps), ot, oq, C.byref(st)))
    return Pose3D(np.array(ot[:], np.float32), np.array(oq[:], np.float32)), st.asdict()


def debug_lm_policy(form, solves):
    """One form of the LM policy on given sums (lom_debug_lm_policy): form 0 = lm_core.hpp on the host, 1-3 = the wave
    forms of lm_wave.hpp on the GPU, all solves in one launch.  `solves`: [(x0[7], prior_b[3], sums[n_evals][32]), ...]
    with 1 <= n_evals <= 5.  Returns per solve a dict: `actions` (1 evaluate / 0 done, one per evaluation replayed),
    `points` (the candidate, or the solution with a 0), `recorded`, `evaluations`, `last_step_norm`, `cost`."""
    n = len(solves)
    ne = np.array([len(s[2]) for s in solves], np.int32)
    x0 = np.ascontiguousarray([np.asarray(s[0], np.float64) for s in solves], np.float64).reshape(n, 7)
    pb = np.ascontiguousarray([np.asarray(s[1], np.float64) for s in solves], np.float64).reshape(n, 3)
    sums = np.zeros((n, 5, 32), np.float64)
    for i, s in enumerate(solves):
        sums[i, :len(s[2])] = np.asarray(s[2], np.float64).reshape(-1, 32)[:5]
    act = np.empty((n, 5), np.int32)
    pts = np.empty((n, 5, 7), np.float64)
    rec, ev = np.empty(n, np.int32), np.empty(n, np.int32)
    lsn, cost = np.empty(n, np.float64), np.empty(n, np.float64)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    capi.check(capi.lib().lom_debug_lm_policy(
        int(form), n, ne.ctypes.data_as(ip), x0.ctypes.data_as(dp), pb.ctypes.data_as(dp), sums.ctypes.data_as(dp),
        act.ctypes.data_as(ip), pts.ctypes.data_as(dp), rec.ctypes.data_as(ip), ev.ctypes.data_as(ip),
        lsn.ctypes.data_as(dp), cost.ctypes.data_as(dp)))
    out = []
    for i in range(n):
        k = int(np.sum(act[i] >= 0))
        out.append({"actions": act[i, :k].tolist(), "points": pts[i, :k].copy(), "recorded": int(rec[i]),
                    "evaluations": int(ev[i]), "last_step_norm": float(lsn[i]), "cost": float(cost[i])})
    return out


class CloudMatcher:
    """reference src/cloud_matcher.h:13-17 / src/cloud_matcher.cpp:105-178."""

    def __init__(self):
        self.stats = None
        self.batch_stats = None
        self.best = None

    def align(self, keyframe, planar_cloud, position_guess):
        xyz = capi.xyz_array(planar_cloud)
        ot, oq = (C.c_float * 3)(), (C.c_float * 4)()
        st = capi.AlignStats()
        fn, chk = _align_entry(keyframe, "align")
        chk(fn(keyframe.handle, xyz.ctypes.data, len(xyz), 12, capi.f3(position_guess.translation),
               capi.f4(position_guess.rotation), ot, oq, C.byref(st)))
        self.stats = st.asdict()
        return Pose3D(np.array(ot[:], np.float32), np.array(oq[:], np.float32))

    def debugEvalSums(self, keyframe, planar_cloud, transform, q=None, t=None):
        """One search at the f32 pose `transform`, then the LOM_NSUMS reduced sums of
        PointToPlaneErrorAnalytic::Evaluate (cloud_matcher.cpp:38-103) at the f64 point (q, t)
        (default: the widened pose) -- parity entry, host-driven path's kernels."""
        xyz = capi.xyz_array(planar_cloud)
        q = np.asarray(transform.rotation if q is None else q, np.float64)
        t = np.asarray(transform.translation if t is None else t, np.float64)
        out = (C.c_double * 32)()
        capi.check(capi.lib().lom_debug_eval_sums(
            keyframe.handle, xyz.ctypes.data, len(xyz), 12, capi.f3(transform.translation), capi.f4(transform.rotation),
            (C.c_double * 4)(*q), (C.c_double * 3)(*t), out), keyframe.handle)
        return np.array(out[:], np.float64)

    def debugLmTrace(self, keyframe, planar_cloud, position_guess, outer_index=0):
        """align() on the device-resident path plus what k_lm's policy saw in outer iteration
        `outer_index`: [(x[7], sums[32]), ...] per evaluation.  Returns (pose, trace)."""
        xyz = capi.xyz_array(planar_cloud)
        ot, oq = (C.c_float * 3)(), (C.c_float * 4)()
        st = capi.AlignStats()
        raw = (C.c_double * 200)()
        ne = C.c_int()
        capi.check(capi.lib().lom_debug_lm_trace(
            keyframe.handle, xyz.ctypes.data, len(xyz), 12, capi.f3(position_guess.translation),
            capi.f4(position_guess.rotation), int(outer_index), raw, C.byref(ne), ot, oq, C.byref(st)), keyframe.handle)
        self.stats = st.asdict()
        a = np.array(raw[:], np.float64).reshape(5, 40)
        trace = [(a[e, :7].copy(), a[e, 8:40].copy()) for e in range(ne.value)]
        return Pose3D(np.array(ot[:], np.float32), np.array(oq[:], np.float32)), trace

    def _batch(self, keyframe, problems, count, keep, device):
        res = (capi.AlignResult * max(count, 1))()
        best = C.c_int(-1)
        fn, chk = _align_entry(keyframe, "align_batch_device" if device else "align_batch")
        chk(fn(keyframe.handle, problems if count else None, count, res, C.byref(best)))
        del keep
        self.batch_stats = [dict(res[i].stats.asdict(), round=res[i].round) for i in range(count)]
        self.best = best.value
        return [Pose3D(np.array(res[i].t[:], np.float32), np.array(res[i].q_wxyz[:], np.float32)) for i in range(count)]

    @staticmethod
    def _problem(p, ptr, n, guess, stride_bytes):
        p.xyz = ptr
        p.n = int(n)
        p.stride_bytes = int(stride_bytes)
        p.guess_t[:] = [float(v) for v in np.asarray(guess.translation, np.float32)]
        p.guess_q_wxyz[:] = [float(v) for v in np.asarray(guess.rotation, np.float32)]

    def alignBatch(self, keyframe, clouds, guesses):
        """K (cloud, guess) problems against one keyframe in ONE call (lom_match_align_batch): the K solves run side by
        side on the device.  Returns the poses align() would return, bit for bit; per-problem stats in `batch_stats`,
        the best problem's index (most valid correspondences, then lowest cost) in `best`.  `keyframe`: a VoxelGrid or a
        ScanContext."""
        if len(clouds) != len(guesses):
            raise ValueError("one guess per cloud")
        arrays = [capi.xyz_array(c) for c in clouds]
        problems = (capi.AlignProblem * max(len(arrays), 1))()
        for i, (xyz, g) in enumerate(zip(arrays, guesses)):
            self._problem(problems[i], xyz.ctypes.data if len(xyz) else None, len(xyz), g, 12)
        return self._batch(keyframe, problems, len(arrays), arrays, False)

    def alignBatchDevice(self, keyframe, items, stride_bytes=12):
        """alignBatch with device-resident clouds: items = [(device pointer, n, guess), ...]."""
        problems = (capi.AlignProblem * max(len(items), 1))()
        for i, (ptr, n, g) in enumerate(items):
            self._problem(problems[i], ptr, n, g, stride_bytes)
        return self._batch(keyframe, problems, len(items), None, True)

    def _multi(self, runner, problems, count, keep, device):
        res = (capi.AlignResult * max(count, 1))()
        best = C.c_int(-1)
        L = capi.lib()
        fn = L.lom_match_align_multi_device if device else L.lom_match_align_multi
        capi.check(fn(runner.handle, problems if count else None, count, res, C.byref(best)), runner.handle)
        del keep
        self.batch_stats = [dict(res[i].stats.asdict(), round=res[i].round) for i in range(count)]
        self.best = best.value
        return [Pose3D(np.array(res[i].t[:], np.float32), np.array(res[i].q_wxyz[:], np.float32)) for i in range(count)]

    @staticmethod
    def _multi_problems(keyframes, items):
        problems = (capi.AlignMultiProblem * max(len(items), 1))()
        for i, (kf, (ptr, n, g, stride_bytes)) in enumerate(zip(keyframes, items)):
            if not isinstance(kf, VoxelGrid):
                raise TypeError("alignMulti: every keyframe must be a VoxelGrid")
            problems[i].map = kf.handle
            CloudMatcher._problem(problems[i], ptr, n, g, stride_bytes)
        return problems

    def alignMulti(self, keyframes, clouds, guesses, runner=None):
        """K (cloud, guess) problems, problem i against keyframes[i], in ONE call (lom_match_align_multi): the K solves
        run side by side on the device.  Returns the poses align(keyframes[i], ...) would return, bit for bit; per-problem
        stats in `batch_stats`, the best problem's index in `best`.  `runner` (a VoxelGrid, default keyframes[0]) carries
        the device chain."""
        if not (len(keyframes) == len(clouds) == len(guesses)):
            raise ValueError("one keyframe and one guess per cloud")
        arrays = [capi.xyz_array(c) for c in clouds]
        items = [(a.ctypes.data if len(a) else None, len(a), g, 12) for a, g in zip(arrays, guesses)]
        runner = runner if runner is not None else (keyframes[0] if keyframes else None)
        if runner is None:
            raise ValueError("alignMulti of no problems needs a runner")
        return self._multi(runner, self._multi_problems(keyframes, items), len(items), arrays, False)

    def alignMultiDevice(self, keyframes, items, runner=None, stride_bytes=12):
        """alignMulti with device-resident clouds: items = [(device pointer, n, guess), ...], one per keyframe."""
        if len(keyframes) != len(items):
            raise ValueError("one keyframe per item")
        runner = runner if runner is not None else (keyframes[0] if keyframes else None)
        if runner is None:
            raise ValueError("alignMultiDevice of no problems needs a runner")
        full = [(ptr, n, g, stride_bytes) for ptr, n, g in items]
        return self._multi(runner, self._multi_problems(keyframes, full), len(items), None, True)

    def quality(self, keyframe, planar_cloud, pose, max_correspondence_distance=0.3, min_eig_t=0.0, min_eig_r=0.0,
                residuals=False):
        """The quality report of `pose` (e.g. what align() returned) for this cloud and keyframe: quality_report()."""
        return quality_report(keyframe, planar_cloud, pose, max_correspondence_distance, min_eig_t, min_eig_r, residuals)

    def qualityBatch(self, keyframe, clouds_or_cloud, poses, max_correspondence_distance=0.3, min_eig_t=0.0,
                     min_eig_r=0.0, sums_only=False):
        """K candidate poses scored in one call: quality_report_batch(); the best candidate's index also in `best`."""
        out, self.best = quality_report_batch(keyframe, clouds_or_cloud, poses, max_correspondence_distance, min_eig_t,
                                              min_eig_r, sums_only)
        return out, self.best

    def alignDevice(self, keyframe, d_src_ptr, n, position_guess, stride_bytes=12):
        """Source cloud already resident in HBM (device pointer, e.g. torch tensor.data_ptr())."""
        ot, oq = (C.c_float * 3)(), (C.c_float * 4)()
        st = capi.AlignStats()
        fn, chk = _align_entry(keyframe, "align_device")
        chk(fn(keyframe.handle, d_src_ptr, int(n), int(stride_bytes), capi.f3(position_guess.translation),
               capi.f4(position_guess.rotation), ot, oq, C.byref(st)))
        self.stats = st.asdict()
        return Pose3D(np.array(ot[:], np.float32), np.array(oq[:], np.float32))


# ---- callers of the path: host code in the library over the C ABI --------

def _cloud(points):
    a = np.ascontiguousarray(points, dtype=capi.POINT_XYZIRT)
    if a.ndim != 1:
        raise ValueError("expected a 1-d array of POINT_XYZIRT records")
    return a


def pointTimeNormalize(points):
    """utils::pointTimeNormalize (src/utils/point_time_normalize.h:15-39)."""
    a = _cloud(points)
    out = np.empty_like(a)
    capi.lib().lom_point_time_normalize(a.ctypes.data, len(a), out.ctypes.data)
    return out


def transformNonRigid(points, start_pose, end_pose):
    """CloudTransformer::transformNonRigid (src/utils/cloud_transform.h:15-40)."""
    a = _cloud(points)
    out = np.empty_like(a)
    capi.lib().lom_transform_non_rigid(a.ctypes.data, len(a), C.byref(start_pose._c()), C.byref(end_pose._c()),
                                       out.ctypes.data)
    return out


def rangeFilter(xyz, normals, min_range, max_range):
    """utils::rangeFilter (src/utils/range_filter.h:13-28) on packed xyz (+ normals)."""
    xyz = capi.xyz_array(xyz)
    normals = capi.xyz_array(normals) if normals is not None else None
    oxyz = np.empty_like(xyz)
    onrm = np.empty_like(xyz) if normals is not None else None
    n = capi.lib().lom_range_filter(xyz.ctypes.data, normals.ctypes.data if normals is not None else None, len(xyz),
                                    float(min_range), float(max_range), oxyz.ctypes.data,
                                    onrm.ctypes.data if normals is not None else None)
    return (oxyz[:n], onrm[:n]) if normals is not None else oxyz[:n]


def classify(points):
    """CloudClassifier::classify (src/utils/cloud_classifier.h:19-168):
    (planar xyz, planar normals, number of unclassified points, (height, width) of the organised cloud)."""
    a = _cloud(points)
    xyz = np.empty((max(len(a), 1), 3), np.float32)
    nrm = np.empty((max(len(a), 1), 3), np.float32)
    nu = C.c_size_t()
    grid = (C.c_size_t * 2)()
    n = capi.lib().lom_cloud_classify(a.ctypes.data, len(a), xyz.ctypes.data, nrm.ctypes.data, C.byref(nu), grid)
    return xyz[:n].copy(), nrm[:n].copy(), int(nu.value), (int(grid[0]), int(grid[1]))


def estimateNormals(xyz, radius, device=0, with_counts=False):
    """pcl::NormalEstimation with setRadiusSearch(radius), viewpoint (0, 0, 0) (test/test.cpp:196-205) on the
    device: (n, 3) float32 normals, NaN where fewer than 3 neighbours exist."""
    xyz = capi.xyz_array(xyz)
    nrm = np.empty_like(xyz)
    cnt = np.empty(len(xyz), np.uint32) if with_counts else None
    capi.check(capi.lib().lom_estimate_normals(xyz.ctypes.data, len(xyz), 12, float(radius), int(device), nrm.ctypes.data,
                                               cnt.ctypes.data if with_counts else None))
    return (nrm, cnt) if with_counts else nrm


def neighbourhoodParams(params):
    """capi.NeighbourhoodParams from one, from a dict with its five fields, or from a 5-tuple in the struct's order
    (radius, index_cap, min_neighbours, max_variation, min_spread).  There are no defaults."""
    if isinstance(params, capi.NeighbourhoodParams):
        return params
    names = [k for k, _ in capi.NeighbourhoodParams._fields_]
    if isinstance(params, dict):
        if sorted(params) != sorted(names):
            raise TypeError(f"neighbourhood parameters: exactly {names}")
        return capi.NeighbourhoodParams(**params)
    vals = tuple(params)
    if len(vals) != len(names):
        raise TypeError(f"neighbourhood parameters: exactly {names}")
    return capi.NeighbourhoodParams(*vals)


def carveParams(params):
    """capi.CarveParams from one, from a dict with its four fields, or from a 4-tuple in the struct's order (margin,
    min_range, max_range, min_crossings).  There are no defaults."""
    if isinstance(params, capi.CarveParams):
        return params
    names = [k for k, _ in capi.CarveParams._fields_]
    if isinstance(params, dict):
        if sorted(params) != sorted(names):
            raise TypeError(f"carve parameters: exactly {names}")
        return capi.CarveParams(**params)
    vals = tuple(params)
    if len(vals) != len(names):
        raise TypeError(f"carve parameters: exactly {names}")
    return capi.CarveParams(*vals)


def voteParams(params):
    """capi.VoteParams from one, from a dict with its six fields, or from a 6-tuple in the struct's order (margin,
    min_range, max_range, clearance, min_free_scans, free_per_seen).  There are no defaults."""
    if isinstance(params, capi.VoteParams):
        return params
    names = [k for k, _ in capi.VoteParams._fields_]
    if isinstance(params, dict):
        if sorted(params) != sorted(names):
            raise TypeError(f"vote parameters: exactly {names}")
        return capi.VoteParams(**params)
    vals = tuple(params)
    if len(vals) != len(names):
        raise TypeError(f"vote parameters: exactly {names}")
    return capi.VoteParams(*vals)


def _struct_from(cls, params, what):
    if isinstance(params, cls):
        return params
    names = [k for k, _ in cls._fields_]
    if isinstance(params, dict):
        if sorted(params) != sorted(names):
            raise TypeError(f"{what}: exactly {names}")
        return cls(**params)
    vals = tuple(params)
    if len(vals) != len(names):
        raise TypeError(f"{what}: exactly {names}")
    return cls(*vals)


def occupancyRayParams(params):
    """capi.OccupancyRayParams from one, from a dict with its five fields, or from a 5-tuple in the struct's order (z_lo,
    z_hi, margin, min_range, max_range).  There are no defaults."""
    return _struct_from(capi.OccupancyRayParams, params, "occupancy ray parameters")


def occupancyRule(rule):
    """capi.OccupancyRule from one, from a dict with its three fields, or from a 3-tuple in the struct's order
    (min_free_scans, free_per_seen, min_seen_scans)."""
    return _struct_from(capi.OccupancyRule, rule, "occupancy rule")


def elevationPointParams(params):
    """capi.ElevationPointParams from one, from a dict with its four fields, or from a 4-tuple in the struct's order (z_lo,
    z_hi, min_range, max_range).  There are no defaults."""
    return _struct_from(capi.ElevationPointParams, params, "elevation point parameters")


def elevationLayerParams(params):
    """capi.ElevationLayerParams from one, from a dict, or from a 2-tuple (min_points, window)."""
    return _struct_from(capi.ElevationLayerParams, params, "elevation layer parameters")


def elevationCostParams(params):
    """capi.ElevationCostParams from one, from a dict, or from a 4-tuple (max_slope, max_step, max_rough, max_span)."""
    return _struct_from(capi.ElevationCostParams, params, "elevation cost parameters")


def clearanceParams(params):
    """capi.ClearanceParams from one, from a dict with its four fields, or from a 4-tuple in the struct's order
    (inflation_radius, inscribed_radius, decay, flags).  There are no defaults."""
    return _struct_from(capi.ClearanceParams, params, "clearance parameters")


def navfieldParams(params):
    """capi.NavFieldParams from one, from a dict with its five fields, or from a 5-tuple in the struct's order (neutral,
    factor, unknown_cost, max_passable, flags).  There are no defaults."""
    return _struct_from(capi.NavFieldParams, params, "navigation field parameters")


def navfieldWaypointParams(params):
    """capi.NavFieldWaypointParams from one, from a dict with its four fields, or from a 4-tuple in the struct's order
    (max_cell_cost, lookahead, route_cap, flags).  There are no defaults."""
    return _struct_from(capi.NavFieldWaypointParams, params, "navigation field waypoint parameters")


def regionsParams(params):
    """capi.RegionsParams from one, from a dict with its seven fields, or from a 7-tuple in the struct's order (kind, lo, hi,
    max_cost, min_cells, rank, flags).  There are no defaults."""
    return _struct_from(capi.RegionsParams, params, "region parameters")


def visibilityParams(params):
    """capi.VisibilityParams from one, from a dict with its five fields, or from a 5-tuple in the struct's order (beams,
    range_cells, block_min, unknown_depth, flags).  There are no defaults."""
    return _struct_from(capi.VisibilityParams, params, "visibility parameters")


def visibilitySelectParams(params):
    """capi.VisibilitySelectParams from one, from a dict with its four fields, or from a 4-tuple in the struct's order (n,
    gain_weight, cost_shift, min_gain).  There are no defaults."""
    return _struct_from(capi.VisibilitySelectParams, params, "visibility select parameters")


def classifyNeighbourhood(points, params, details=False, frontend=None):
    """The neighbourhood classifier alone (lom_classify_neighbourhood) on POINT_XYZIRT records whose `ring` is not read:
    (planar xyz, normals) in input order, and with details=True a third array of capi.NEIGHBOURHOOD_DETAIL records, one
    per input point.  `frontend`: the FrontEnd whose stream and workspace it uses (default: one made for the call)."""
    a = _cloud(points)
    fe = frontend if frontend is not None else FrontEnd()
    p = neighbourhoodParams(params)
    xyz = np.empty((max(len(a), 1), 3), np.float32)
    nrm = np.empty((max(len(a), 1), 3), np.float32)
    det = np.zeros(len(a), capi.NEIGHBOURHOOD_DETAIL) if details else None
    n = fe._check(capi.lib().lom_classify_neighbourhood(fe._h, a.ctypes.data, len(a), C.byref(p), xyz.ctypes.data,
                                                        nrm.ctypes.data, det.ctypes.data if details else None))
    out = (xyz[:n].copy(), nrm[:n].copy())
    return out + (det,) if details else out


class _Handle:
    """A handle of the family lom_<_family>_*: its creation, destruction and last error."""

    _family = None
    _create_failed = None  # the text of a failed create; None: lom_<_family>_last_error(NULL), why it failed

    def _call(self, name, *args):
        return getattr(capi.lib(), f"lom_{self._family}_{name}")(*args)

    def _create(self, *args):
        """lom_<_family>_create(*args, &handle)"""
        h = C.c_void_p()
        rc = self._call("create", *args, C.byref(h))
        if rc != 0:
            if self._create_failed:
                raise LomError(int(rc), self._create_failed)
            text = self._call("last_error", None)
            raise LomError(int(rc), text.decode() if text else f"lom_{self._family}_create")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and capi is not None:          # at interpreter shutdown the module may already be gone
            self._call("destroy", h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def _check(self, rc):
        if rc < 0:
            text = self._call("last_error", self._h)
            raise LomError(int(rc), text.decode() if text else "")
        return rc


class FrontEnd(_Handle):
    """The per-frame front end on the device (csrc/frontend.hip): pointTimeNormalize + transformNonRigid +
    CloudClassifier::classify + rangeFilter, results left in HBM."""

    _family, _create_failed = "frontend", "lom_frontend_create failed"

    def __init__(self, device=0):
        self._create(int(device), None)

    def setClassifier(self, kind, params=None):
        """capi.CLASSIFIER_RINGS (the default) or capi.CLASSIFIER_NEIGHBOURHOOD (params required) for the frames that follow."""
        p = neighbourhoodParams(params) if params is not None else None
        self._check(capi.lib().lom_frontend_set_classifier(self._h, int(kind), C.byref(p) if p is not None else None))

    def setOption(self, option, value):
        self._check(capi.lib().lom_frontend_set_option(self._h, int(option), int(value)))

    def debugCounter(self, which=capi.COUNTER_GRID_REDOS):
        return int(capi.lib().lom_frontend_debug_counter(self._h, int(which)))

    def process(self, points, start_pose, end_pose, min_range, max_range):
        """Returns dict(deskewed, planar_points, xyz, normals, grid, redo_on_host)."""
        a = _cloud(points)
        L = capi.lib()
        self._check(L.lom_frontend_process(self._h, a.ctypes.data, len(a), C.byref(start_pose._c()),
                                           C.byref(end_pose._c()), float(min_range), float(max_range)))
        counts = (C.c_uint32 * 4)()
        redo = self._check(L.lom_frontend_wait(self._h, counts))
        desk = np.empty(len(a), capi.POINT_XYZIRT)
        self._check(L.lom_frontend_fetch(self._h, 0, desk.ctypes.data, None, len(a)))
        nf = int(counts[1])
        xyz, nrm = np.empty((nf, 3), np.float32), np.empty((nf, 3), np.float32)
        self._check(L.lom_frontend_fetch(self._h, 1, xyz.ctypes.data, nrm.ctypes.data, nf))
        return dict(deskewed=desk, planar_points=int(counts[0]), xyz=xyz, normals=nrm,
                    grid=(int(counts[2]), int(counts[3])), redo_on_host=bool(redo))

    def sinf(self, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        self._check(capi.lib().lom_debug_sinf(self._h, x.ctypes.data, x.size, out.ctypes.data))
        return out


def placeParams(params):
    """capi.PlaceParams from one, from a dict with its four fields, or from a 4-tuple in the struct's order
    (rings, sectors, max_range, z_floor).  There are no defaults."""
    if isinstance(params, capi.PlaceParams):
        return params
    names = [k for k, _ in capi.PlaceParams._fields_]
    if isinstance(params, dict):
        if sorted(params) != sorted(names):
            raise TypeError(f"place parameters: exactly {names}")
        return capi.PlaceParams(**params)
    vals = tuple(params)
    if len(vals) != len(names):
        raise TypeError(f"place parameters: exactly {names}")
    return capi.PlaceParams(*vals)


def _place_cloud(cloud):
    """(pointer owner, n, stride) of an (n, 3) float array or of POINT_XYZIRT records"""
    a = np.asarray(cloud)
    if a.dtype == capi.POINT_XYZIRT:
        a = np.ascontiguousarray(a)
        return a, len(a), 32
    a = capi.xyz_array(a.reshape(-1, 3) if a.size == 0 else a)
    return a, len(a), 12


class PlaceDatabase(_Handle):
    """Scan descriptors (a polar height image in the style of Scan Context) and a database of them in HBM
    (lom_place_db_*, include/lidar_odometry_amd.h): query() names, for each query descriptor, the k nearest entries and
    the column shift against each; shiftYaw() turns a shift into the yaw of a pose guess.  numpy in and out."""

    _family = "place_db"

    def __init__(self, params, capacity_hint=0, device=0):
        self.params = placeParams(params)
        self._create(C.byref(self.params), int(device), int(capacity_hint))
        self.shape = (int(self.params.rings), int(self.params.sectors))

    def __len__(self):
        return int(self._check(capi.lib().lom_place_db_size(self._h)))

    def clear(self):
        self._check(capi.lib().lom_place_db_clear(self._h))

    def _desc(self, desc, count=None):
        d = np.ascontiguousarray(desc, np.float32)
        cells = self.shape[0] * self.shape[1]
        if d.size % cells or d.size == 0 or (count is not None and d.size != count * cells):
            raise ValueError(f"expected descriptors of shape {self.shape}")
        return d

    def describe(self, cloud):
        """The raw (rings, sectors) descriptor of an (n, 3) cloud or of POINT_XYZIRT records; the database is unchanged."""
        a, n, stride = _place_cloud(cloud)
        out = np.empty(self.shape, np.float32)
        self._check(capi.lib().lom_place_describe(self._h, a.ctypes.data if n else None, n, stride, out.ctypes.data))
        return out

    def add(self, desc):
        """A raw descriptor becomes a new entry; returns its id (0, 1, 2 ... in order of arrival)."""
        d = self._desc(desc, 1)
        return int(self._check(capi.lib().lom_place_db_add(self._h, d.ctypes.data)))

    def addCloud(self, cloud):
        """describe + add with the descriptor staying in HBM; returns the id."""
        a, n, stride = _place_cloud(cloud)
        return int(self._check(capi.lib().lom_place_db_add_cloud(self._h, a.ctypes.data if n else None, n, stride)))

    def get(self, id):
        out = np.empty(self.shape, np.float32)
        self._check(capi.lib().lom_place_db_get(self._h, int(id), out.ctypes.data))
        return out

    def query(self, desc, k=1, id_begin=0, id_end=None, all_dist=False):
        """desc: one (rings, sectors) descriptor or a stack of Q of them.  Returns a (Q, k) array of capi.PLACE_MATCH
        (id, distance, shift; nearest first; id -1 / distance inf in slots beyond the entries searched), and with
        all_dist=True also the (Q, id_end - id_begin) distances to every entry of the range."""
        d = self._desc(desc)
        q = d.size // (self.shape[0] * self.shape[1])
        if id_end is None:
            id_end = len(self)
        out = np.zeros((q, max(int(k), 1)), capi.PLACE_MATCH)
        n = max(int(id_end) - int(id_begin), 0)
        alld = np.empty((q, n), np.float32) if all_dist else None
        self._check(capi.lib().lom_place_db_query(self._h, d.ctypes.data, q, int(id_begin), int(id_end), int(k),
                                                  out.ctypes.data, alld.ctypes.data if all_dist else None))
        return (out, alld) if all_dist else out

    def shiftYaw(self, shift):
        """psi = ((S - shift) mod S) 2 pi / S: the rotation about z that takes the entry's cloud onto the query's; the
        query sensor's rotation in the entry's frame is Rz(-psi)."""
        return float(capi.lib().lom_place_shift_yaw(C.byref(self.params), int(shift)))


def graphParams(params):
    """capi.GraphParams from one, or from a dict with exactly its six fields (lambda0, gtol, xtol, pcg_rtol, max_outer,
    max_pcg).  There are no defaults."""
    if isinstance(params, capi.GraphParams):
        return params
    names = [k for k, _ in capi.GraphParams._fields_]
    if not isinstance(params, dict) or sorted(params) != sorted(names):
        raise TypeError(f"pose graph parameters: exactly {names}")
    return capi.GraphParams(**params)


def graph_information_from_quality(report, with_prior=True):
    """lom_graph_information_from_quality: the 6x6 Omega of an edge (rotation in radians, then translation) from the
    quality report (capi.QualityReport) of the align that measured it."""
    out = np.empty((6, 6), np.float64)
    rc = capi.lib().lom_graph_information_from_quality(C.byref(report), int(bool(with_prior)), out.ctypes.data)
    if rc != 0:
        raise LomError(int(rc), "a quality report with fewer than 7 correspondences carries no information matrix")
    return out


def _graph_poses(poses):
    """capi.GRAPH_POSE records from such records, from an (n, 7) array (t, then q wxyz) or from one pose of 7 values"""
    a = np.asarray(poses)
    if a.dtype == capi.GRAPH_POSE:
        return np.ascontiguousarray(a).reshape(-1)
    if isinstance(poses, Pose3D):
        a = np.concatenate([poses.translation, poses.rotation])
    a = np.ascontiguousarray(a, np.float64).reshape(-1, 7)
    out = np.empty(len(a), capi.GRAPH_POSE)
    out["t"], out["q_wxyz"] = a[:, :3], a[:, 3:]
    return out


def graph_pose_rotation_matrix(pose):
    """lom_graph_pose_rotation_matrix: the 3x3 float64 rotation matrix the map assembly uses for a pose (7 values: t,
    then the quaternion w x y z, normalised first)."""
    p = _graph_poses(pose)
    if len(p) != 1:
        raise TypeError("one pose of 7 values")
    out = np.empty((3, 3), np.float64)
    rc = capi.lib().lom_graph_pose_rotation_matrix(p.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise LomError(int(rc), "a pose with a non-finite value or a zero quaternion")
    return out


class ScanArchive(_Handle):
    """Clouds with normals kept in HBM in their own sensor frame (lom_archive_*, include/lidar_odometry_amd.h "scan
    archive and map assembly"); VoxelGrid.assemble puts any of them, at float64 poses, into a map in one call."""

    _family = "archive"

    def __init__(self, point_hint=0, scan_hint=0, device=0):
        self._create(int(device), int(point_hint), int(scan_hint))

    def __len__(self):
        return int(self._check(capi.lib().lom_archive_scan_count(self._h)))

    def pointCount(self):
        return int(self._check(capi.lib().lom_archive_point_count(self._h)))

    def scanSize(self, id):
        return int(self._check(capi.lib().lom_archive_scan_size(self._h, int(id))))

    def clear(self):
        self._check(capi.lib().lom_archive_clear(self._h))

    def waitEvent(self, hip_event):
        self._check(capi.lib().lom_archive_wait_event(self._h, hip_event))

    def add(self, xyz, normals):
        """a new scan from host arrays; returns its id"""
        xyz, nrm = capi.xyz_array(xyz), capi.xyz_array(normals)
        if len(xyz) != len(nrm):
            raise ValueError("points and normals differ in length")
        return int(self._check(capi.lib().lom_archive_add(self._h, xyz.ctypes.data, nrm.ctypes.data, len(xyz), 12)))

    def addDevice(self, d_xyz_ptr, d_nrm_ptr, n, stride_bytes=12, hip_event=None):
        """a new scan from device memory, read behind `hip_event` (a hipEvent_t) or the archive's own stream"""
        return int(self._check(capi.lib().lom_archive_add_device(self._h, d_xyz_ptr, d_nrm_ptr, int(n), int(stride_bytes),
                                                                hip_event)))

    def addPoints(self, xyz):
        """lom_archive_add_points: a new scan without normals (zeros are stored); returns its id"""
        xyz = capi.xyz_array(xyz)
        return int(self._check(capi.lib().lom_archive_add_points(self._h, xyz.ctypes.data, len(xyz), 12)))

    def addPointsDevice(self, d_xyz_ptr, n, stride_bytes=12, hip_event=None):
        """the same from device memory, read behind `hip_event` (a hipEvent_t) or the archive's own stream"""
        return int(self._check(capi.lib().lom_archive_add_points_device(self._h, d_xyz_ptr, int(n), int(stride_bytes), hip_event)))

    def get(self, id):
        """(points, normals) of a scan, (n, 3) float32 each"""
        n = self.scanSize(id)
        xyz, nrm = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        self._check(capi.lib().lom_archive_get(self._h, int(id), xyz.ctypes.data, nrm.ctypes.data, n))
        return xyz, nrm


def _assemble_args(ids, poses):
    ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
    p = _graph_poses(poses) if len(ids) else np.empty(0, capi.GRAPH_POSE)
    if len(p) != len(ids):
        raise ValueError("one pose per id")
    return ids, p


class _Grid(_Handle):
    """What every dense 2-D grid shares: a geometry structure (_geometry) it is created from and gives back, options, an
    event for its stream to wait on, and a clear."""

    _geometry = capi.OccupancyGeometry

    def _create_grid(self, geo, device):
        self._create(C.byref(geo), int(device))
        self.width, self.height = int(geo.width), int(geo.height)

    def geometry(self):
        geo = self._geometry()
        self._check(self._call("get_geometry", self._h, C.byref(geo)))
        return geo.asdict()

    def setOption(self, option, value):
        self._check(self._call("set_option", self._h, int(option), int(value)))

    def waitEvent(self, hip_event):
        self._check(self._call("wait_event", self._h, hip_event))

    def clear(self):
        self._check(self._call("clear", self._h))

    def shift(self, dx, dy):
        """lom_<family>_shift: the window moves by (dx, dy) whole cells by the rule of grid_shift_geometry.  An occupancy or
        elevation grid keeps what still overlaps and clears what enters; a planning grid is left as its clear() leaves it."""
        self._check(self._call("shift", self._h, int(dx), int(dy)))


def _occupancy_geometry(geometry):
    """capi.OccupancyGeometry of one, of a grid's geometry() dict (an elevation grid's too), or of the 5-tuple (resolution,
    origin_x, origin_y, width, height)"""
    if isinstance(geometry, capi.OccupancyGeometry):
        return geometry
    if isinstance(geometry, dict):
        geometry = [geometry[k] for k in ("resolution", "origin_x", "origin_y", "width", "height")]
    return capi.OccupancyGeometry(*geometry)


def grid_shift_geometry(geometry, dx, dy):
    """lom_grid_shift_geometry: the geometry moved by (dx, dy) whole cells, as a capi.OccupancyGeometry; origin' =
    f32(f64(origin) + dx * f64(resolution)).  Needs no device."""
    out = capi.OccupancyGeometry()
    rc = capi.lib().lom_grid_shift_geometry(C.byref(_occupancy_geometry(geometry)), int(dx), int(dy), C.byref(out))
    if rc != 0:
        raise LomError(rc, "grid shift: a valid geometry and an origin that stays finite")
    return out


def grid_follow(geometry, x, y, margin_cells, quantum_cells):
    """lom_grid_follow: the shift (dx, dy), in multiples of quantum_cells, that brings a robot at (x, y) metres back towards
    the middle once its cell leaves [margin_cells, n - margin_cells) on an axis; (0, 0) while it is inside.  Needs no device."""
    dx, dy = C.c_int32(), C.c_int32()
    rc = capi.lib().lom_grid_follow(C.byref(_occupancy_geometry(geometry)), float(x), float(y), int(margin_cells), int(quantum_cells),
                                    C.byref(dx), C.byref(dy))
    if rc != 0:
        raise LomError(rc, "grid follow: a valid geometry, a finite position, quantum >= 1, margin + quantum <= side / 2, "
                           "a position within 2^40 cells")
    return int(dx.value), int(dy.value)


class _PosedScanGrid(_Grid):
    """What OccupancyGrid and ElevationGrid share (csrc/grid_handle.hpp): a dense 2-D grid that integrates posed scans.  A
    family names its geometry and stats structures (_geometry, _stats) and the converter of its parameters (_params)."""

    def _integrate(self, archive, ids, poses, params):
        """lom_<family>_integrate: the scans `ids` of the ScanArchive at `poses` (n x 7 float64, t then q wxyz); returns the
        family's stats (capi.OccupancyStats / capi.ElevationStats) as a dict"""
        p = self._params(params)
        ids, g = _assemble_args(ids, poses)
        st = self._stats()
        self._check(self._call("integrate", self._h, archive.handle, ids.ctypes.data, g.ctypes.data, len(ids), C.byref(p),
                               C.byref(st)))
        return st.asdict()

    def _integrate_cloud(self, xyz, pose, params, device_ptr=None, n=None, stride_bytes=12, hip_event=None):
        """lom_<family>_integrate_cloud: one scan that is not in an archive, a host array (n, 3) -- or, with device_ptr,
        lom_<family>_integrate_cloud_device: n records of stride_bytes in HBM behind `hip_event`"""
        p = self._params(params)
        g = _graph_poses(np.asarray(pose, np.float64).reshape(1, 7))
        st = self._stats()
        if device_ptr is not None:
            rc = self._call("integrate_cloud_device", self._h, device_ptr, int(n), int(stride_bytes), g.ctypes.data, C.byref(p),
                            hip_event, C.byref(st))
        else:
            xyz = capi.xyz_array(xyz)
            rc = self._call("integrate_cloud", self._h, xyz.ctypes.data, len(xyz), 12, g.ctypes.data, C.byref(p), C.byref(st))
        self._check(rc)
        return st.asdict()


class OccupancyGrid(_PosedScanGrid):
    """A dense 2-D grid of free / seen scan counts on the device (lom_occupancy_*, include/lidar_odometry_amd.h
    "occupancy grid"): posed scans vote once per cell, and classify() turns the counts into the int8 values of
    nav_msgs/OccupancyGrid (0 free, 100 occupied, -1 unknown), shape (height, width)."""

    _family, _geometry, _stats = "occupancy", capi.OccupancyGeometry, capi.OccupancyStats
    _params = staticmethod(occupancyRayParams)

    def __init__(self, resolution, origin_xy, width, height, device=0):
        self._create_grid(capi.OccupancyGeometry(float(resolution), float(origin_xy[0]), float(origin_xy[1]), int(width),
                                                 int(height)), device)

    def integrate(self, archive, ids, poses, ray_params):
        """lom_occupancy_integrate: the scans `ids` of the ScanArchive at `poses` (n x 7 float64, t then q wxyz) vote;
        returns capi.OccupancyStats as a dict"""
        return self._integrate(archive, ids, poses, ray_params)

    def integrateCloud(self, xyz, pose, ray_params, device_ptr=None, n=None, stride_bytes=12, hip_event=None):
        """lom_occupancy_integrate_cloud: one scan that is not in an archive, a host array (n, 3) -- or, with device_ptr,
        lom_occupancy_integrate_cloud_device: n records of stride_bytes in HBM behind `hip_event`"""
        return self._integrate_cloud(xyz, pose, ray_params, device_ptr, n, stride_bytes, hip_event)

    def counts(self):
        """(free, seen): uint32 arrays of shape (height, width)"""
        free, seen = np.zeros((self.height, self.width), np.uint32), np.zeros((self.height, self.width), np.uint32)
        self._check(capi.lib().lom_occupancy_counts(self._h, free.ctypes.data, seen.ctypes.data, free.size))
        return free, seen

    def classify(self, rule):
        """(int8 array of shape (height, width), summary dict) by lom_occupancy_rule"""
        r = occupancyRule(rule)
        out = np.empty((self.height, self.width), np.int8)
        sm = capi.OccupancySummary()
        self._check(capi.lib().lom_occupancy_classify(self._h, C.byref(r), out.ctypes.data, out.size, C.byref(sm)))
        return out, sm.asdict()


class ElevationGrid(_PosedScanGrid):
    """A dense 2-D grid of height accumulators on the device (lom_elevation_*, include/lidar_odometry_amd.h "elevation
    grid"): every point of a posed scan that is an occupancy hit adds its quantised height to its cell; layers() derives
    ground height, slope, roughness and step, cost() the int8 values of a costmap (-1 unknown, 0 .. 99, 100 lethal).  All
    arrays have the shape (height, width)."""

    LAYERS = ("min", "max", "mean", "slope", "rough", "step")
    _family, _geometry, _stats = "elevation", capi.ElevationGeometry, capi.ElevationStats
    _params = staticmethod(elevationPointParams)

    def __init__(self, resolution, origin_xy, width, height, z_ref=0.0, device=0):
        self._create_grid(capi.ElevationGeometry(float(resolution), float(origin_xy[0]), float(origin_xy[1]), int(width),
                                                 int(height), float(z_ref)), device)

    def integrate(self, archive, ids, poses, point_params):
        """lom_elevation_integrate: the scans `ids` of the ScanArchive at `poses` (n x 7 float64, t then q wxyz); returns
        capi.ElevationStats as a dict"""
        return self._integrate(archive, ids, poses, point_params)

    def integrateCloud(self, xyz, pose, point_params, device_ptr=None, n=None, stride_bytes=12, hip_event=None):
        """lom_elevation_integrate_cloud: one scan that is not in an archive, a host array (n, 3) -- or, with device_ptr,
        lom_elevation_integrate_cloud_device: n records of stride_bytes in HBM behind `hip_event`"""
        return self._integrate_cloud(xyz, pose, point_params, device_ptr, n, stride_bytes, hip_event)

    def cells(self):
        """(count uint32, zmin int32, zmax int32, sum int64): the accumulators, in quanta of 2^-8 m relative to z_ref"""
        shape = (self.height, self.width)
        count, zmin, zmax = np.zeros(shape, np.uint32), np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        total = np.zeros(shape, np.int64)
        self._check(capi.lib().lom_elevation_cells(self._h, count.ctypes.data, zmin.ctypes.data, zmax.ctypes.data,
                                                   total.ctypes.data, count.size))
        return count, zmin, zmax, total

    def layers(self, layer_params):
        """dict of the six float32 layers (min, max, mean, slope, rough, step) by lom_elevation_layer_params"""
        lp = elevationLayerParams(layer_params)
        out = {k: np.empty((self.height, self.width), np.float32) for k in self.LAYERS}
        self._check(capi.lib().lom_elevation_layers(self._h, C.byref(lp), *[out[k].ctypes.data for k in self.LAYERS],
                                                    self.width * self.height))
        return out

    def cost(self, layer_params, cost_params):
        """(int8 array, summary dict) by lom_elevation_layer_params and lom_elevation_cost_params"""
        lp, cp = elevationLayerParams(layer_params), elevationCostParams(cost_params)
        out = np.empty((self.height, self.width), np.int8)
        sm = capi.ElevationSummary()
        self._check(capi.lib().lom_elevation_cost(self._h, C.byref(lp), C.byref(cp), out.ctypes.data, out.size, C.byref(sm)))
        return out, sm.asdict()


class _PlaneGrid(_Grid):
    """What ClearanceGrid, NavField, NavFieldSet, PoseField, RegionGrid, VisibilityGrid and RolloutGrid share (csrc/plane_handle.hpp): a dense 2-D grid of one
    lom_occupancy_geometry that takes planes of shape (height, width)."""

    _shape_text = "expected an int8 array of shape (height, width)"

    def __init__(self, resolution, origin_xy, width, height, device=0):
        self._create_grid(capi.OccupancyGeometry(float(resolution), float(origin_xy[0]), float(origin_xy[1]), int(width),
                                                 int(height)), device)

    def _plane(self, a, dtype):
        """a host plane as a contiguous array of `dtype`"""
        a = np.ascontiguousarray(a, dtype)
        if a.shape != (self.height, self.width):
            raise ValueError(self._shape_text)
        return a

    def _optional_plane(self, a, dtype):
        return None if a is None else self._plane(a, dtype)


class ClearanceGrid(_PlaneGrid):
    """Obstacle distance and inflated cost on the device (lom_clearance_*, include/lidar_odometry_amd.h "clearance grid"):
    update() merges an occupancy and an elevation plane (int8 arrays of shape (height, width), either may be None),
    computes the exact truncated squared distance to the nearest obstacle and the int8 cost of a costmap (-1 unknown,
    0 .. 98, 99 inscribed, 100 lethal).  A window is (x0, y0, width, height) in cells.  All arrays have the shape
    (height, width)."""

    _family = "clearance"

    @staticmethod
    def _window(window):
        return None if window is None else C.byref(capi.ClearanceWindow(*[int(v) for v in window]))

    def update(self, occ, elev, params, window=None, device=False, hip_event=None):
        """lom_clearance_update: host planes -- or, with device=True, lom_clearance_update_device: occ and elev are device
        pointers to planes in HBM, complete when `hip_event` is.  Returns capi.ClearanceSummary as a dict."""
        p, sm = clearanceParams(params), capi.ClearanceSummary()
        if device:
            rc = self._call("update_device", self._h, occ, elev, hip_event, C.byref(p), self._window(window), C.byref(sm))
        else:
            occ, elev = self._optional_plane(occ, np.int8), self._optional_plane(elev, np.int8)
            rc = self._call("update", self._h, None if occ is None else occ.ctypes.data, None if elev is None else elev.ctypes.data,
                            C.byref(p), self._window(window), C.byref(sm))
        self._check(rc)
        return sm.asdict()

    def updateFromGrids(self, occupancy, rule, elevation, layer_params, cost_params, params, window=None):
        """lom_clearance_update_from_grids: the planes of an OccupancyGrid (by `rule`) and an ElevationGrid (by
        `layer_params`, `cost_params`) of this geometry, left in HBM; either grid may be None"""
        p, sm = clearanceParams(params), capi.ClearanceSummary()
        r = None if occupancy is None else C.byref(occupancyRule(rule))
        lp = None if elevation is None else C.byref(elevationLayerParams(layer_params))
        cp = None if elevation is None else C.byref(elevationCostParams(cost_params))
        self._check(self._call("update_from_grids", self._h, None if occupancy is None else occupancy.handle, r,
                               None if elevation is None else elevation.handle, lp, cp, C.byref(p), self._window(window),
                               C.byref(sm)))
        return sm.asdict()

    def cost(self):
        """(int8 array, summary dict of the whole plane)"""
        out, sm = np.empty((self.height, self.width), np.int8), capi.ClearanceSummary()
        self._check(self._call("cost", self._h, out.ctypes.data, out.size, C.byref(sm)))
        return out, sm.asdict()

    def distanceSq(self):
        """uint16 array: the squared distance to the nearest obstacle in cells, capi.CLEAR_FAR beyond the radius"""
        out = np.empty((self.height, self.width), np.uint16)
        self._check(self._call("distance_sq", self._h, out.ctypes.data, out.size))
        return out

    def distance(self):
        """float32 array: that distance in metres, +inf beyond the radius"""
        out = np.empty((self.height, self.width), np.float32)
        self._check(self._call("distance", self._h, out.ctypes.data, out.size))
        return out

    def query(self, xy):
        """(distance in metres float32, cost int8) of the cells of the points xy (n, 2), in the grid's frame; NaN and -1
        outside the grid"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        dist, cost = np.empty(len(xy), np.float32), np.empty(len(xy), np.int8)
        self._check(self._call("query", self._h, xy.ctypes.data, len(xy), dist.ctypes.data, cost.ctypes.data))
        return dist, cost


def clearanceCostTable(params, resolution):
    """lom_clearance_cost_table: the uint8 cost per squared distance, R^2 + 1 entries; needs no device"""
    p = clearanceParams(params)
    geo = capi.OccupancyGeometry(float(resolution), 0.0, 0.0, 1, 1)
    n = capi.lib().lom_clearance_cost_table(C.byref(p), C.byref(geo), None, 0)
    if n < 0:
        raise LomError(int(n), "clearance cost table: bad parameters")
    out = np.empty(n, np.uint8)
    capi.lib().lom_clearance_cost_table(C.byref(p), C.byref(geo), out.ctypes.data, n)
    return out


class NavField(_PlaneGrid):
    """The navigation field on the device (lom_navfield_*, include/lidar_odometry_amd.h "navigation field"): solve() takes
    an int8 cost plane of shape (height, width) in the value range ClearanceGrid.cost() writes, and goals, and leaves per
    cell the least total cost to reach a goal (uint32, capi.NAV_UNREACHED where there is no route); paths() walks down it,
    query() reads it at points in metres.  Goals and starts are (n, 2) arrays: integers are cells (ix, iy), with
    metres=True floats are (x, y) in the grid's frame."""

    _family = "navfield"

    @staticmethod
    def _points(points, metres):
        """(kind, contiguous (n, 2) array)"""
        if metres:
            return capi.NAV_METRES, np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        return capi.NAV_CELLS, np.ascontiguousarray(points, np.int32).reshape(-1, 2)

    def solve(self, plane, params, goals, metres=False, device=False, hip_event=None):
        """lom_navfield_solve: a host plane -- or, with device=True, lom_navfield_solve_device: `plane` is a device pointer to
        a plane in HBM, complete when `hip_event` is.  Returns capi.NavFieldSummary as a dict."""
        p, sm = navfieldParams(params), capi.NavFieldSummary()
        kind, g = self._points(goals, metres)
        if device:
            rc = self._call("solve_device", self._h, plane, hip_event, C.byref(p), kind, g.ctypes.data, len(g), C.byref(sm))
        else:
            plane = self._plane(plane, np.int8)
            rc = self._call("solve", self._h, plane.ctypes.data, C.byref(p), kind, g.ctypes.data, len(g), C.byref(sm))
        self._check(rc)
        return sm.asdict()

    def solveFromClearance(self, clearance, params, goals, metres=False):
        """lom_navfield_solve_from_clearance: the cost plane a ClearanceGrid of this geometry left in HBM"""
        p, sm = navfieldParams(params), capi.NavFieldSummary()
        kind, g = self._points(goals, metres)
        self._check(self._call("solve_from_clearance", self._h, clearance.handle, C.byref(p), kind, g.ctypes.data, len(g), C.byref(sm)))
        return sm.asdict()

    def resolve(self, plane, window=None, device=False, hip_event=None):
        """lom_navfield_resolve: the field of the kept plane with the cells of `window` ((x0, y0, width, height) in cells,
        None: the whole grid) taken from the host plane `plane`, for the goals the last solve used -- or, with device=True,
        lom_navfield_resolve_device: `plane` is a device pointer to a plane in HBM, complete when `hip_event` is.  Returns
        capi.NavFieldSummary as a dict."""
        sm = capi.NavFieldSummary()
        if device:
            rc = self._call("resolve_device", self._h, plane, hip_event, ClearanceGrid._window(window), C.byref(sm))
        else:
            plane = self._plane(plane, np.int8)
            rc = self._call("resolve", self._h, plane.ctypes.data, ClearanceGrid._window(window), C.byref(sm))
        self._check(rc)
        return sm.asdict()

    def resolveFromClearance(self, clearance, window=None):
        """lom_navfield_resolve_from_clearance: the window of the cost plane a ClearanceGrid of this geometry left in HBM"""
        sm = capi.NavFieldSummary()
        self._check(self._call("resolve_from_clearance", self._h, clearance.handle, ClearanceGrid._window(window), C.byref(sm)))
        return sm.asdict()

    def resolveStats(self):
        """capi.NavFieldResolveCounters of the last re-solve as a dict: cells_changed, cells_raised, raise_launches,
        relax_launches, waits, tiles_marked"""
        st = capi.NavFieldResolveCounters()
        self._check(self._call("resolve_stats", self._h, C.byref(st)))
        return st.asdict()

    def shiftResolve(self, dx, dy, plane, window=None, device=False, hip_event=None):
        """lom_navfield_shift_resolve: the geometry moves by (dx, dy) cells, the field and the kept plane move with the
        world, the entered cells and the cells of `window` take the bytes of the host plane `plane` (in the new geometry's
        cells), and the field is re-solved for the goals that are still in the grid -- or, with device=True,
        lom_navfield_shift_resolve_device: `plane` is a device pointer to a plane in HBM, complete when `hip_event` is.
        Returns capi.NavFieldSummary as a dict."""
        sm = capi.NavFieldSummary()
        if device:
            rc = self._call("shift_resolve_device", self._h, int(dx), int(dy), plane, hip_event, ClearanceGrid._window(window), C.byref(sm))
        else:
            plane = self._plane(plane, np.int8)
            rc = self._call("shift_resolve", self._h, int(dx), int(dy), plane.ctypes.data, ClearanceGrid._window(window), C.byref(sm))
        self._check(rc)
        return sm.asdict()

    def shiftResolveFromClearance(self, dx, dy, clearance, window=None):
        """lom_navfield_shift_resolve_from_clearance: the cost plane a ClearanceGrid left in HBM after it was shifted by
        the same (dx, dy) and updated"""
        sm = capi.NavFieldSummary()
        self._check(self._call("shift_resolve_from_clearance", self._h, int(dx), int(dy), clearance.handle,
                               ClearanceGrid._window(window), C.byref(sm)))
        return sm.asdict()

    def shiftStats(self):
        """capi.NavFieldShiftCounters of the last shift with a re-solve as a dict: cells_kept, cells_entered, goals_left"""
        st = capi.NavFieldShiftCounters()
        self._check(self._call("shift_stats", self._h, C.byref(st)))
        return st.asdict()

    def potential(self):
        """uint32 array of shape (height, width): P per cell, capi.NAV_UNREACHED where no goal is reached"""
        out = np.empty((self.height, self.width), np.uint32)
        self._check(self._call("potential", self._h, out.ctypes.data, out.size))
        return out

    def paths(self, starts, cap, metres=False):
        """(cells uint16 (K, cap, 2), lengths uint32 (K,)): the walk from each start down the field, (ix, iy) per cell; a
        length counts start and goal, is 0 for a start outside the grid or unreached, and may exceed cap"""
        kind, s = self._points(starts, metres)
        cells, lengths = np.zeros((len(s), int(cap), 2), np.uint16), np.zeros(len(s), np.uint32)
        self._check(self._call("paths", self._h, kind, s.ctypes.data, len(s), cells.ctypes.data, int(cap), lengths.ctypes.data))
        return cells, lengths

    def query(self, xy):
        """uint32 P of the cells of the points xy (n, 2), in the grid's frame; capi.NAV_UNREACHED outside the grid"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty(len(xy), np.uint32)
        self._check(self._call("query", self._h, xy.ctypes.data, len(xy), out.ctypes.data))
        return out

    def visible(self, pairs, max_cell_cost=0):
        """uint8 per pair of cells (x0, y0, x1, y1), an (n, 4) integer array: 1 where the second cell is in line of sight of
        the first over cells of cost at most `max_cell_cost` (0: any passable cell), under the last solve's parameters"""
        q = np.ascontiguousarray(pairs, np.int32).reshape(-1, 4)
        out = np.zeros(len(q), np.uint8)
        self._check(self._call("visible", self._h, q.ctypes.data, len(q), int(max_cell_cost), out.ctypes.data))
        return out

    def waypoints(self, starts, params, wp_cap, metres=False):
        """(cells uint16 (K, wp_cap, 2), counts uint32 (K,), lengths uint32 (K,)): the walk from each start down the field,
        cut to any-angle waypoints by line-of-sight shortcuts.  `params`: navfieldWaypointParams (max_cell_cost, lookahead,
        route_cap, flags).  A count is the full number of waypoints and may exceed wp_cap; a length is the full length of
        the walk and may exceed route_cap, of which only the first route_cap cells are cut."""
        p = navfieldWaypointParams(params)
        kind, s = self._points(starts, metres)
        cells = np.zeros((len(s), int(wp_cap), 2), np.uint16)
        counts, lengths = np.zeros(len(s), np.uint32), np.zeros(len(s), np.uint32)
        self._check(self._call("waypoints", self._h, kind, s.ctypes.data, len(s), C.byref(p), cells.ctypes.data, int(wp_cap),
                               counts.ctypes.data, lengths.ctypes.data))
        return cells, counts, lengths

    def waypointsMetres(self, cells):
        """float64 (..., 2): the centres of cells (ix, iy) in the grid's frame, origin + (i + 0.5) * resolution"""
        g = self.geometry()
        return np.array([g["origin_x"], g["origin_y"]]) + (np.asarray(cells, np.float64) + 0.5) * g["resolution"]

    def polylineLength(self, cells, count=None):
        """the length in metres of the polyline through the first `count` (default: all) cells of an (n, 2) array"""
        xy = self.waypointsMetres(np.asarray(cells).reshape(-1, 2)[:count])
        return float(np.sqrt((np.diff(xy, axis=0) ** 2).sum(axis=1)).sum())

    def stats(self):
        """capi.NavFieldSolveStats of the last solve as a dict: launches, waits, tiles"""
        st = capi.NavFieldSolveStats()
        self._check(self._call("stats", self._h, C.byref(st)))
        return st.asdict()

    def adopt(self, fieldset, i):
        """lom_navfield_adopt: this field becomes what solve() of the plane, parameters and goals of field `i` of a
        NavFieldSet of this geometry would have left; paths(), waypoints(), resolve() and the consumers that take a NavField
        then read it.  Returns capi.NavFieldSummary as a dict."""
        sm = capi.NavFieldSummary()
        self._check(self._call("adopt", self._h, fieldset.handle, int(i), C.byref(sm)))
        return sm.asdict()


class NavFieldSet(_PlaneGrid):
    """N navigation fields over one cost plane, solved in one call (lom_navset_*, include/lidar_odometry_amd.h "navigation
    field set"): solve() takes a plane, one parameter set and a list of goal arrays, one per field; field i and its summary
    are byte for byte what NavField.solve() gives for goals_per_field[i].  gather() reads every field at points (with the
    goals as points: the travel-cost matrix), nearest() gives the partition of the grid by nearest goal, paths() walks down a
    named field, NavField.adopt() makes one field a NavField.  Goals, starts and points are as NavField's."""

    _family = "navset"

    def __init__(self, resolution, origin_xy, width, height, max_fields, device=0):
        geo = capi.OccupancyGeometry(float(resolution), float(origin_xy[0]), float(origin_xy[1]), int(width), int(height))
        self._create(C.byref(geo), int(device), int(max_fields))
        self.width, self.height, self.max_fields = int(geo.width), int(geo.height), int(max_fields)

    @staticmethod
    def _goals(goals_per_field, metres):
        """(kind, contiguous (n, 2) array of all goals, uint32 offsets (n_fields + 1,))"""
        per = [NavField._points(g, metres)[1] for g in goals_per_field]
        offsets = np.zeros(len(per) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(g) for g in per])
        kind, empty = NavField._points(np.zeros((0, 2)), metres)
        return kind, np.ascontiguousarray(np.concatenate(per)) if per else empty, offsets

    def _solve(self, name, head, params, goals_per_field, metres):
        p = navfieldParams(params)
        kind, g, offsets = self._goals(goals_per_field, metres)
        n = len(offsets) - 1
        sm = (capi.NavFieldSummary * max(n, 1))()
        self._check(self._call(name, self._h, *head, C.byref(p), kind, g.ctypes.data, offsets.ctypes.data, n, sm))
        return [sm[i].asdict() for i in range(n)]

    def solve(self, plane, params, goals_per_field, metres=False):
        """lom_navset_solve: a host plane and one goal array per field.  Returns a list of capi.NavFieldSummary dicts."""
        plane = self._plane(plane, np.int8)
        return self._solve("solve", (plane.ctypes.data,), params, goals_per_field, metres)

    def solveDevice(self, d_plane, params, goals_per_field, metres=False, hip_event=None):
        """lom_navset_solve_device: `d_plane` is a device pointer to a plane in HBM, complete when `hip_event` is"""
        return self._solve("solve_device", (d_plane, hip_event), params, goals_per_field, metres)

    def solveFromClearance(self, clearance, params, goals_per_field, metres=False):
        """lom_navset_solve_from_clearance: the cost plane a ClearanceGrid of this geometry left in HBM"""
        return self._solve("solve_from_clearance", (clearance.handle,), params, goals_per_field, metres)

    def fieldCount(self):
        """the fields of the last solve; 0 after create, clear() or shift()"""
        return int(self._call("field_count", self._h))

    def potential(self, i):
        """uint32 array of shape (height, width): P of field i"""
        out = np.empty((self.height, self.width), np.uint32)
        self._check(self._call("potential", self._h, int(i), out.ctypes.data, out.size))
        return out

    def potentialDevice(self, i):
        """the device pointer of field i, valid until the next solve(), clear() or shift()"""
        p = C.c_void_p()
        self._check(self._call("potential_device", self._h, int(i), C.byref(p)))
        return p.value

    def gather(self, points, metres=False):
        """uint32 (fieldCount(), n): P of every field at every point, capi.NAV_UNREACHED outside the grid.  With the goals
        as the points this is the travel-cost matrix; a step pays for the cell it leaves, so it need not be symmetric."""
        kind, q = NavField._points(points, metres)
        out = np.empty((self.fieldCount(), len(q)), np.uint32)
        self._check(self._call("gather", self._h, kind, q.ctypes.data, len(q), out.ctypes.data))
        return out

    def nearest(self):
        """(owner uint16 (height, width), potential uint32 (height, width), cells_owned uint64 (fieldCount(),)): per cell the
        least P over the fields and the least field index that attains it, capi.NAVSET_NO_OWNER where none reaches it"""
        owner, potential = np.empty((self.height, self.width), np.uint16), np.empty((self.height, self.width), np.uint32)
        owned = np.zeros(self.fieldCount(), np.uint64)
        self._check(self._call("nearest", self._h, owner.ctypes.data, potential.ctypes.data, owned.ctypes.data))
        return owner, potential, owned

    def paths(self, field_of_start, starts, cap, metres=False):
        """(cells uint16 (K, cap, 2), lengths uint32 (K,)): NavField.paths()' walk, start k down field field_of_start[k]"""
        kind, s = NavField._points(starts, metres)
        which = np.ascontiguousarray(field_of_start, np.int32).reshape(-1)
        if len(which) != len(s):
            raise ValueError("one field index per start")
        cells, lengths = np.zeros((len(s), int(cap), 2), np.uint16), np.zeros(len(s), np.uint32)
        self._check(self._call("paths", self._h, which.ctypes.data, kind, s.ctypes.data, len(s), cells.ctypes.data, int(cap),
                               lengths.ctypes.data))
        return cells, lengths

    def stats(self):
        """capi.NavSetSolveStats of the last solve as a dict: launches, waits, tiles (workgroups per launch), fields"""
        st = capi.NavSetSolveStats()
        self._check(self._call("stats", self._h, C.byref(st)))
        return st.asdict()


class PoseField(_PlaneGrid):
    """The pose field on the device (lom_posefield_*, include/lidar_odometry_amd.h "pose field"): solve() takes an int8 cost
    plane of shape (height, width), a footprint -- (F, 2) int32 samples in 1/256 cell in the robot's frame, what
    rolloutFootprintRectangle gives -- and goals, (n, 3) int32 triples (ix, iy, h) with h = -1 for every passable heading of
    the cell, and leaves per cell and heading the least total cost to reach a goal state (uint32, capi.NAV_UNREACHED where
    there is no way).  Heading h of 0 .. 7 points along E, NE, N, NW, W, SW, S, SE.  floor() is the least over the headings,
    in NavField.potential()'s form; paths() walks down the field, query() reads it at points in metres."""

    _family = "posefield"

    @staticmethod
    def _triples(a):
        return np.ascontiguousarray(a, np.int32).reshape(-1, 3)

    def _solve(self, name, head, params, footprint, goals):
        p, sm = posefieldParams(params), capi.PoseFieldSummary()
        fp, g = np.ascontiguousarray(footprint, np.int32).reshape(-1, 2), self._triples(goals)
        self._check(self._call(name, self._h, *head, C.byref(p), fp.ctypes.data, len(fp), g.ctypes.data, len(g), C.byref(sm)))
        return sm.asdict()

    def solve(self, plane, params, footprint, goals, device=False, hip_event=None):
        """lom_posefield_solve: a host plane -- or, with device=True, lom_posefield_solve_device: `plane` is a device pointer
        to a plane in HBM, complete when `hip_event` is.  Returns capi.PoseFieldSummary as a dict."""
        if device:
            return self._solve("solve_device", (plane, hip_event), params, footprint, goals)
        plane = self._plane(plane, np.int8)
        return self._solve("solve", (plane.ctypes.data,), params, footprint, goals)

    def solveFromClearance(self, clearance, params, footprint, goals):
        """lom_posefield_solve_from_clearance: the cost plane a ClearanceGrid of this geometry left in HBM"""
        return self._solve("solve_from_clearance", (clearance.handle,), params, footprint, goals)

    def resolve(self, plane, window=None, device=False, hip_event=None):
        """lom_posefield_resolve: the pose field of the kept plane with the cells of `window` ((x0, y0, width, height) in
        cells, None: the whole grid) taken from the host plane `plane`, for the footprint, parameters and goal states of the
        last solve -- or, with device=True, lom_posefield_resolve_device: `plane` is a device pointer to a plane in HBM,
        complete when `hip_event` is.  Returns capi.PoseFieldSummary as a dict."""
        sm = capi.PoseFieldSummary()
        if device:
            rc = self._call("resolve_device", self._h, plane, hip_event, ClearanceGrid._window(window), C.byref(sm))
        else:
            plane = self._plane(plane, np.int8)
            rc = self._call("resolve", self._h, plane.ctypes.data, ClearanceGrid._window(window), C.byref(sm))
        self._check(rc)
        return sm.asdict()

    def resolveFromClearance(self, clearance, window=None):
        """lom_posefield_resolve_from_clearance: the window of the cost plane a ClearanceGrid of this geometry left in HBM"""
        sm = capi.PoseFieldSummary()
        self._check(self._call("resolve_from_clearance", self._h, clearance.handle, ClearanceGrid._window(window), C.byref(sm)))
        return sm.asdict()

    def resolveStats(self):
        """capi.PoseFieldResolveCounters of the last re-solve as a dict: cells_changed, states_changed, states_raised,
        raise_launches, relax_launches, waits, tiles_marked"""
        st = capi.PoseFieldResolveCounters()
        self._check(self._call("resolve_stats", self._h, C.byref(st)))
        return st.asdict()

    def potential(self):
        """uint32 array of shape (8, height, width): P per heading and cell"""
        out = np.empty((capi.POSE_HEADINGS, self.height, self.width), np.uint32)
        self._check(self._call("potential", self._h, out.ctypes.data, out.size))
        return out

    def potentialDevice(self):
        """the device pointer of P, valid until the next solve(), clear() or shift()"""
        p = C.c_void_p()
        self._check(self._call("potential_device", self._h, C.byref(p)))
        return p.value

    def layers(self):
        """uint32 array of shape (8, height, width): L per heading and cell, 0 where the footprint does not fit"""
        out = np.empty((capi.POSE_HEADINGS, self.height, self.width), np.uint32)
        self._check(self._call("layers", self._h, out.ctypes.data, out.size))
        return out

    def floor(self):
        """(floor uint32 (height, width), heading uint8 (height, width)): the least P over the headings and the least
        heading that attains it, 8 where none is reached"""
        fl, fh = np.empty((self.height, self.width), np.uint32), np.empty((self.height, self.width), np.uint8)
        self._check(self._call("floor", self._h, fl.ctypes.data, fh.ctypes.data, fl.size))
        return fl, fh

    def floorDevice(self):
        """(floor, heading) device pointers, valid as potentialDevice()'s; the floor is a potential plane for
        RolloutGrid.evaluate(..., device=True)"""
        fl, fh = C.c_void_p(), C.c_void_p()
        self._check(self._call("floor_device", self._h, C.byref(fl), C.byref(fh)))
        return fl.value, fh.value

    def paths(self, starts, cap):
        """(states uint16 (K, cap, 3), lengths uint32 (K,)): the walk from each start (ix, iy, h), h = -1 for the floor's
        heading, down the field; a length counts start and goal, is 0 for a start that is not walked, and may exceed cap"""
        s = self._triples(starts)
        states, lengths = np.zeros((len(s), int(cap), 3), np.uint16), np.zeros(len(s), np.uint32)
        self._check(self._call("paths", self._h, s.ctypes.data, len(s), states.ctypes.data, int(cap), lengths.ctypes.data))
        return states, lengths

    def query(self, xy, headings):
        """uint32 P of the states at the points xy (n, 2) in the grid's frame with one heading each, -1 for the floor;
        capi.NAV_UNREACHED outside the grid"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        h = np.ascontiguousarray(headings, np.int32).reshape(-1)
        if len(h) != len(xy):
            raise ValueError("one heading per point")
        out = np.empty(len(xy), np.uint32)
        self._check(self._call("query", self._h, xy.ctypes.data, h.ctypes.data, len(xy), out.ctypes.data))
        return out

    def stats(self):
        """capi.PoseFieldSolveStats of the last solve as a dict: launches, waits, tiles"""
        st = capi.PoseFieldSolveStats()
        self._check(self._call("stats", self._h, C.byref(st)))
        return st.asdict()


def posefieldParams(params):
    """capi.PoseFieldParams from one, from a dict with its five fields, or from a 5-tuple in the struct's order (nav,
    turn_cost, spin_cost, reverse_cost, flags); nav is whatever navfieldParams takes.  There are no defaults."""
    if isinstance(params, capi.PoseFieldParams):
        return params
    names = [k for k, _ in capi.PoseFieldParams._fields_]
    if isinstance(params, dict):
        if sorted(params) != sorted(names):
            raise TypeError(f"pose field parameters: exactly {names}")
        vals = [params[k] for k in names]
    else:
        vals = list(params)
        if len(vals) != len(names):
            raise TypeError(f"pose field parameters: exactly {names}")
    return capi.PoseFieldParams(navfieldParams(vals[0]), *[int(v) for v in vals[1:]])


posefield_params = posefieldParams


def posefieldStencils(footprint):
    """lom_posefield_stencils: a list of eight (n_h, 2) int32 arrays, the (dx, dy) cell offsets the footprint covers at
    heading h, sorted by (dy, dx); needs no device"""
    fp = np.ascontiguousarray(footprint, np.int32).reshape(-1, 2)
    counts = np.zeros(capi.POSE_HEADINGS, np.uint32)
    rc = capi.lib().lom_posefield_stencils(fp.ctypes.data, len(fp), None, 0, counts.ctypes.data)
    if rc != 0:
        raise LomError(int(rc), "pose field stencils: a footprint of 1 .. 1024 samples with |fx|, |fy| <= 16384")
    cells = np.zeros((int(counts.sum()), 2), np.int32)
    capi.lib().lom_posefield_stencils(fp.ctypes.data, len(fp), cells.ctypes.data, len(cells), counts.ctypes.data)
    return np.split(cells, np.cumsum(counts)[:-1].astype(np.int64))


def posefieldHeadingOfAngle(angle):
    """lom_posefield_heading_of_angle: the heading 0 .. 7 of an angle in 1/65536 turn; needs no device"""
    return int(capi.lib().lom_posefield_heading_of_angle(int(angle) & 0xFFFFFFFF))


def navfieldCellCosts(params):
    """lom_navfield_cell_costs: the uint32 cost of a cell per cost byte (index: the byte read as unsigned), 0 = impassable;
    needs no device"""
    p = navfieldParams(params)
    out = np.empty(256, np.uint32)
    rc = capi.lib().lom_navfield_cell_costs(C.byref(p), out.ctypes.data)
    if rc != 0:
        raise LomError(int(rc), "navigation field cell costs: bad parameters")
    return out


class RegionGrid(_PlaneGrid):
    """Connected regions of a grid plane on the device (lom_regions_*, include/lidar_odometry_amd.h "frontier regions"):
    extract() takes an int8 plane of shape (height, width) -- what OccupancyGrid.classify() writes -- and optionally a cost
    plane and a NavField potential, labels the regions of the frontier cells (or of a byte range) with the least linear
    index of each, and leaves a record per region and a ranked list; goals() gives the list's centre or entry cells in the
    form NavField.solve() takes."""

    _family = "regions"
    _shape_text = "expected an array of shape (height, width)"

    def extract(self, plane, params, cost=None, potential=None, device=False, hip_event=None):
        """lom_regions_extract: host planes (int8, int8 or None, uint32 or None) -- or, with device=True,
        lom_regions_extract_device: device pointers to planes in HBM, complete when `hip_event` is.  Returns
        capi.RegionsSummary as a dict."""
        p, sm = regionsParams(params), capi.RegionsSummary()
        if device:
            rc = self._call("extract_device", self._h, plane, cost, potential, hip_event, C.byref(p), C.byref(sm))
        else:
            plane, cost = self._optional_plane(plane, np.int8), self._optional_plane(cost, np.int8)
            potential = self._optional_plane(potential, np.uint32)
            rc = self._call("extract", self._h, None if plane is None else plane.ctypes.data, None if cost is None else cost.ctypes.data,
                            None if potential is None else potential.ctypes.data, C.byref(p), C.byref(sm))
        self._check(rc)
        return sm.asdict()

    def extractFromGrids(self, occupancy, rule, clearance, navfield, params):
        """lom_regions_extract_from_grids: the planes an OccupancyGrid (by `rule`), a ClearanceGrid (or None) and a NavField
        (or None) of this geometry left in HBM"""
        p, sm = regionsParams(params), capi.RegionsSummary()
        self._check(self._call("extract_from_grids", self._h, occupancy.handle, C.byref(occupancyRule(rule)),
                               None if clearance is None else clearance.handle, None if navfield is None else navfield.handle,
                               C.byref(p), C.byref(sm)))
        return sm.asdict()

    def labels(self):
        """uint32 array of shape (height, width): the least linear index of a member's region, capi.REGIONS_NONE elsewhere"""
        out = np.empty((self.height, self.width), np.uint32)
        self._check(self._call("labels", self._h, out.ctypes.data, out.size))
        return out

    def list(self):
        """the list of the last extract: an array of capi.REGIONS_RECORD in rank order"""
        n = C.c_size_t()
        self._check(self._call("list", self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, capi.REGIONS_RECORD)
        self._check(self._call("list", self._h, out.ctypes.data, len(out), None))
        return out

    def goals(self, which=capi.REGIONS_GOAL_CENTRE):
        """int32 array (n, 2): the centre cells (or, with capi.REGIONS_GOAL_ENTRY, the entry cells) of the list, in list order"""
        n = C.c_size_t()
        self._check(self._call("goals", self._h, int(which), None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), np.int32)
        self._check(self._call("goals", self._h, int(which), out.ctypes.data, len(out), None))
        return out

    def query(self, xy):
        """uint32 label of the cells of the points xy (n, 2), in the grid's frame; capi.REGIONS_NONE outside the grid"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty(len(xy), np.uint32)
        self._check(self._call("query", self._h, xy.ctypes.data, len(xy), out.ctypes.data))
        return out

    def stats(self):
        """capi.RegionsExtractStats of the last extract as a dict: launches, waits, tiles"""
        st = capi.RegionsExtractStats()
        self._check(self._call("stats", self._h, C.byref(st)))
        return st.asdict()


class VisibilityGrid(_PlaneGrid):
    """Rays cast over a grid plane from many viewpoints at once (lom_visibility_*, include/lidar_odometry_amd.h "visibility
    grid"): cast() takes an int8 plane of shape (height, width) -- what OccupancyGrid.classify() or ClearanceGrid.cost()
    writes -- and (K, 2) int32 viewpoints (ix, iy), what RegionGrid.goals() returns, and leaves a record per viewpoint: the
    distinct cells its beams see, by class.  beams() gives the simulated scans, windows() the unknown cells each viewpoint
    sees, select() the greedy next-best views, gain against travel cost."""

    _family = "visibility"
    _beams = _range = 0  # of the last cast

    def _cast(self, name, head, viewpoints, params):
        p, sm = visibilityParams(params), capi.VisibilitySummary()
        vp = np.ascontiguousarray(viewpoints, np.int32).reshape(-1, 2)
        self._check(self._call(name, self._h, *head, vp.ctypes.data if len(vp) else None, len(vp), C.byref(p), C.byref(sm)))
        self._beams, self._range = int(p.beams), int(p.range_cells)
        return sm.asdict()

    def cast(self, plane, viewpoints, params, device=False, hip_event=None):
        """lom_visibility_cast: a host plane -- or, with device=True, lom_visibility_cast_device: `plane` is a device pointer
        to a plane in HBM, complete when `hip_event` is.  Returns capi.VisibilitySummary as a dict."""
        if device:
            return self._cast("cast_device", (plane, hip_event), viewpoints, params)
        return self._cast("cast", (self._plane(plane, np.int8).ctypes.data,), viewpoints, params)

    def castFromOccupancy(self, occupancy, rule, viewpoints, params):
        """lom_visibility_cast_from_occupancy: the plane an OccupancyGrid of this geometry classifies by `rule`, in HBM"""
        return self._cast("cast_from_occupancy", (occupancy.handle, C.byref(occupancyRule(rule))), viewpoints, params)

    def records(self):
        """the records of the last cast: an array of capi.VISIBILITY_RECORD, one per viewpoint"""
        n = C.c_size_t()
        self._check(self._call("records", self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, capi.VISIBILITY_RECORD)
        self._check(self._call("records", self._h, out.ctypes.data, len(out), None))
        return out

    def beams(self):
        """uint32 array (K, B) of the last cast under capi.VIS_KEEP_BEAMS: d2 in the low 24 bits, the end reason in the high 8"""
        n = C.c_size_t()
        self._check(self._call("records", self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, self._beams), np.uint32)
        self._check(self._call("beams", self._h, out.ctypes.data, out.size))
        return out

    def windowsDevice(self):
        """(device pointer, words per window) of the last cast's windows under capi.VIS_KEEP_WINDOWS"""
        d, words = C.c_void_p(), C.c_size_t()
        self._check(self._call("windows_device", self._h, C.byref(d), C.byref(words)))
        return d.value, int(words.value)

    def windows(self):
        """uint32 array (K, 2R + 1, words per row): the unknown cells each viewpoint of the last cast sees, read back"""
        n, words = C.c_size_t(), C.c_size_t()
        self._check(self._call("records", self._h, None, 0, C.byref(n)))
        self._check(self._call("windows", self._h, None, 0, C.byref(words)))
        side = 2 * self._range + 1
        out = np.zeros((n.value, side, words.value // side), np.uint32)
        self._check(self._call("windows", self._h, out.ctypes.data, out.size, None))
        return out

    def _select(self, name, head, select):
        s = visibilitySelectParams(select)
        out, n = np.zeros(max(int(s.n), 1), capi.VISIBILITY_PICK), C.c_size_t()
        self._check(self._call(name, self._h, *head, out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def select(self, select, cost=None):
        """lom_visibility_select: the picks (capi.VISIBILITY_PICK: k, gain, score) in the order picked; cost: K uint32 or None"""
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.uint32)
        return self._select("select", (C.byref(visibilitySelectParams(select)), None if cost is None else cost.ctypes.data), select)

    def selectFromNavfield(self, navfield, select):
        """lom_visibility_select_from_navfield: the costs are a NavField's potential at the viewpoints' cells, read in HBM"""
        return self._select("select_from_navfield", (navfield.handle, C.byref(visibilitySelectParams(select))), select)

    def stats(self):
        """capi.VisibilityCallStats of the last cast or select as a dict: launches, waits"""
        st = capi.VisibilityCallStats()
        self._check(self._call("stats", self._h, C.byref(st)))
        return st.asdict()


def visibilityTable(beams):
    """lom_visibility_table: the int32 (dx, dy) of each of `beams` beams, shape (beams, 2); needs no device"""
    out = np.zeros((max(int(beams), 0), 2), np.int32)
    rc = capi.lib().lom_visibility_table(int(beams) & 0xFFFFFFFF, out.ctypes.data)
    if rc != 0:
        raise LomError(int(rc), "visibility table: 4 <= beams <= 8192")
    return out


class RolloutGrid(_PlaneGrid):
    """Candidate command sequences rolled out from many start states at once (lom_rollout_*, include/lidar_odometry_amd.h
    "trajectory rollouts"): evaluate() takes an int8 cost plane of shape (height, width) -- what ClearanceGrid.cost() writes
    -- an optional uint32 potential (NavField.potential()), M states (capi.ROLLOUT_STATE, or an (M, 3) array of x, y, a), K
    candidates of L (v, w) int16 commands as an array (K, L, 2), and F footprint samples (F, 2) int32, and returns the pick
    per state (capi.ROLLOUT_PICK) and the summary.  records() gives the record per state and candidate."""

    _family = "rollout"

    @staticmethod
    def _states(states):
        s = np.asarray(states)
        if s.dtype != capi.ROLLOUT_STATE:
            s = np.asarray(states, np.int64).reshape(-1, 3)
            out = np.zeros(len(s), capi.ROLLOUT_STATE)
            if np.any(s[:, :2] < -2**31) or np.any(s[:, :2] >= 2**31) or np.any(s[:, 2] < 0) or np.any(s[:, 2] >= 2**32):
                raise ValueError("rollout states: x, y int32 and a uint32")
            out["x"], out["y"], out["a"] = s[:, 0], s[:, 1], s[:, 2]
            s = out
        return np.ascontiguousarray(s.reshape(-1))

    def _evaluate(self, name, head, states, commands, footprint, params):
        p, sm = rolloutParams(params), capi.RolloutSummary()
        st = self._states(states)
        cmd = np.ascontiguousarray(commands, np.int16)
        per = 2 * max(int(p.segments), 1)  # int16 words of a candidate
        # the library judges the parameters and, with `segments` out of range, reads no command; within it, it reads k * per
        if 1 <= int(p.segments) <= 8 and ((cmd.ndim == 3 and cmd.shape[1:] != (per // 2, 2)) or cmd.size % per):
            raise ValueError("rollout commands: (K, segments, 2) int16, or K * segments * 2 of them")
        k = len(cmd) if cmd.ndim == 3 else cmd.size // per
        fp = np.ascontiguousarray(footprint, np.int32).reshape(-1, 2)
        picks = np.zeros(len(st), capi.ROLLOUT_PICK)
        self._check(self._call(name, self._h, *head, st.ctypes.data if len(st) else None, len(st), cmd.ctypes.data if k else None,
                               k, fp.ctypes.data if len(fp) else None, len(fp), C.byref(p),
                               picks.ctypes.data if len(st) else None, C.byref(sm)))
        return picks, sm.asdict()

    def evaluate(self, cost_plane, potential, states, commands, footprint, params, device=False, cost_event=None,
                 potential_event=None):
        """lom_rollout_evaluate: host planes (potential may be None) -- or, with device=True, lom_rollout_evaluate_device:
        the planes are device pointers, each complete when its event is.  Returns (picks, summary dict)."""
        if device:
            return self._evaluate("evaluate_device", (cost_plane, cost_event, potential, potential_event), states, commands,
                                  footprint, params)
        cost, pot = self._plane(cost_plane, np.int8), self._optional_plane(potential, np.uint32)
        return self._evaluate("evaluate", (cost.ctypes.data, None if pot is None else pot.ctypes.data), states, commands, footprint,
                              params)

    def evaluateFromGrids(self, clearance, navfield, states, commands, footprint, params):
        """lom_rollout_evaluate_from_grids: the cost of a ClearanceGrid and the potential of a NavField (or None) of this
        geometry, read in HBM"""
        return self._evaluate("evaluate_from_grids", (clearance.handle, None if navfield is None else navfield.handle), states,
                              commands, footprint, params)

    def records(self):
        """the records of the last evaluation under capi.ROLLOUT_KEEP_RECORDS: an array of capi.ROLLOUT_RECORD, state-major"""
        n = C.c_size_t()
        self._check(self._call("records", self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, capi.ROLLOUT_RECORD)
        self._check(self._call("records", self._h, out.ctypes.data if len(out) else None, len(out), None))
        return out

    def stats(self):
        """capi.RolloutCallStats of the last evaluation as a dict: launches, waits"""
        st = capi.RolloutCallStats()
        self._check(self._call("stats", self._h, C.byref(st)))
        return st.asdict()


def rolloutParams(params):
    """capi.RolloutParams from one, from a dict with its nine fields, or from a 9-tuple in the struct's order (segments,
    steps_per_segment, lethal_min, unknown_cost, min_steps, progress_weight, cost_weight, truncation_weight, flags).  There
    are no defaults."""
    return _struct_from(capi.RolloutParams, params, "rollout parameters")


def rolloutFootprintRectangle(front, back, half_width, spacing, perimeter_only=False):
    """lom_rollout_footprint_rectangle: the (F, 2) int32 samples of a rectangle, all in 1/256 cell; needs no device"""
    n = C.c_size_t()
    args = (int(front), int(back), int(half_width), int(spacing), int(bool(perimeter_only)))
    if capi.lib().lom_rollout_footprint_rectangle(*args, None, 0, C.byref(n)) != 0:
        raise LomError(-1, "rollout footprint: 0 <= front, back, half_width <= 16384, spacing >= 1, at most 1024 samples")
    out = np.zeros((n.value, 2), np.int32)
    capi.lib().lom_rollout_footprint_rectangle(*args, out.ctypes.data, len(out), C.byref(n))
    return out


def rolloutStateFromPose(geometry, x_m, y_m, yaw):
    """lom_rollout_state_from_pose: (x, y, a) of a pose in metres and radians on a grid given as capi.OccupancyGeometry or
    its 5-tuple (resolution, origin_x, origin_y, width, height); needs no device"""
    geo = geometry if isinstance(geometry, capi.OccupancyGeometry) else capi.OccupancyGeometry(*geometry)
    out = np.zeros(1, capi.ROLLOUT_STATE)
    if capi.lib().lom_rollout_state_from_pose(C.byref(geo), float(x_m), float(y_m), float(yaw), out.ctypes.data) != 0:
        raise LomError(-1, "rollout state: a valid geometry, a finite pose, -2^29 <= x, y < 2^29 in Q15 cells")
    return int(out["x"][0]), int(out["y"][0]), int(out["a"][0])


def rolloutPoses(params, state, commands):
    """lom_rollout_poses: the (S + 1, 3) int64 poses (x, y, a) of one candidate of L (v, w) commands; needs no device"""
    p = rolloutParams(params)
    st = RolloutGrid._states([state])
    cmd = np.ascontiguousarray(commands, np.int16).reshape(-1, 2)
    S = int(p.segments) * int(p.steps_per_segment)
    out = np.zeros(max(S, 0) + 1 if S <= 1024 else 1, capi.ROLLOUT_STATE)
    if len(cmd) != int(p.segments) or capi.lib().lom_rollout_poses(C.byref(p), st.ctypes.data, cmd.ctypes.data, out.ctypes.data) != 0:
        raise LomError(-1, "rollout poses: valid parameters, a valid state, `segments` commands")
    return np.stack([out["x"].astype(np.int64), out["y"].astype(np.int64), out["a"].astype(np.int64)], axis=1)


class PoseGraph(_Handle):
    """Keyframe poses and the relative poses measured between them, in HBM, optimised on the device (lom_graph_*,
    include/lidar_odometry_amd.h "pose graph").  Poses are (n, 7) float64 arrays: t, then the quaternion w x y z; an
    edge's measurement is the pose of node j in node i's frame.  numpy in and out."""

    _family = "graph"

    def __init__(self, node_hint=0, edge_hint=0, device=0):
        self._create(int(device), int(node_hint), int(edge_hint))

    def clear(self):
        self._check(capi.lib().lom_graph_clear(self._h))

    def nodeCount(self):
        return int(self._check(capi.lib().lom_graph_node_count(self._h)))

    def edgeCount(self):
        return int(self._check(capi.lib().lom_graph_edge_count(self._h)))

    def addNode(self, pose, fixed=False):
        p = _graph_poses(pose)
        return int(self._check(capi.lib().lom_graph_add_node(self._h, p.ctypes.data, int(bool(fixed)))))

    def addNodes(self, poses, fixed):
        """Returns the first id; fixed: one flag per node."""
        p = _graph_poses(poses)
        f = np.ascontiguousarray(np.asarray(fixed) != 0, np.int32)
        if len(f) != len(p):
            raise ValueError("one fixed flag per pose")
        return int(self._check(capi.lib().lom_graph_add_nodes(self._h, p.ctypes.data, f.ctypes.data, len(p))))

    def addEdge(self, i, j, measurement, information, delta):
        """information: the 6x6 Omega (rotation in radians, then translation), or the capi.QualityReport of the align that
        measured the edge (taken with the align's translation prior: graph_information_from_quality)."""
        if isinstance(information, capi.QualityReport):
            information = graph_information_from_quality(information, True)
        z = _graph_poses(measurement)
        om = np.ascontiguousarray(information, np.float64).reshape(36)
        return int(self._check(capi.lib().lom_graph_add_edge(self._h, int(i), int(j), z.ctypes.data, om.ctypes.data,
                                                             float(delta))))

    def addEdges(self, ij, measurements, informations, deltas):
        """Returns the first id.  ij: (n, 2); measurements: (n, 7); informations: (n, 6, 6); deltas: n."""
        e = np.ascontiguousarray(ij, np.int32).reshape(-1, 2)
        z = _graph_poses(measurements)
        om = np.ascontiguousarray(informations, np.float64).reshape(-1, 36)
        d = np.ascontiguousarray(deltas, np.float64).reshape(-1)
        if not len(e) == len(z) == len(om) == len(d):
            raise ValueError("one measurement, information and delta per edge")
        return int(self._check(capi.lib().lom_graph_add_edges(self._h, e.ctypes.data, z.ctypes.data, om.ctypes.data,
                                                              d.ctypes.data, len(e))))

    def poses(self, first=0, n=None):
        """(n, 7) float64: t, then q wxyz"""
        if n is None:
            n = self.nodeCount() - int(first)
        out = np.empty(max(int(n), 0), capi.GRAPH_POSE)
        self._check(capi.lib().lom_graph_get_poses(self._h, int(first), int(n), out.ctypes.data))
        return np.concatenate([out["t"], out["q_wxyz"]], axis=1)

    def setPose(self, id, pose):
        self._check(capi.lib().lom_graph_set_pose(self._h, int(id), _graph_poses(pose).ctypes.data))

    def setFixed(self, id, fixed):
        self._check(capi.lib().lom_graph_set_fixed(self._h, int(id), int(bool(fixed))))

    def optimize(self, params):
        """Levenberg-Marquardt on the device from the poses the graph holds; returns the stats as a dict."""
        st = capi.GraphStats()
        self._check(capi.lib().lom_graph_optimize(self._h, C.byref(graphParams(params)), C.byref(st)))
        return st.asdict()

    def evaluate(self, lam=0.0):
        """One linearisation at the current poses: dict of e (m, 6), w (m), cost, g (n, 6), hdiag (n, 6, 6) -- the diagonal
        blocks of H_ff + lam D; a fixed node's g and block read 0."""
        n, m = self.nodeCount(), self.edgeCount()
        e, w, cost = np.zeros((m, 6)), np.zeros(m), C.c_double()
        g, hd = np.zeros((n, 6)), np.zeros((n, 6, 6))
        self._check(capi.lib().lom_graph_evaluate(self._h, float(lam), e.ctypes.data, w.ctypes.data, C.addressof(cost),
                                                  g.ctypes.data, hd.ctypes.data))
        return {"e": e, "w": w, "cost": cost.value, "g": g, "hdiag": hd}

    def matvec(self, lam, p):
        """lom_graph_debug_matvec: (H_ff + lam D) p, (n, 6) in and out"""
        p = np.ascontiguousarray(p, np.float64)
        if p.shape != (self.nodeCount(), 6):
            raise ValueError("p: 6 values per node")
        y = np.zeros_like(p)
        self._check(capi.lib().lom_graph_debug_matvec(self._h, float(lam), p.ctypes.data, y.ctypes.data))
        return y

    def chi2(self, first=0, n=None):
        """s = e^T Omega e per edge at the current poses"""
        if n is None:
            n = self.edgeCount() - int(first)
        out = np.zeros(max(int(n), 0))
        self._check(capi.lib().lom_graph_edge_chi2(self._h, int(first), int(n), out.ctypes.data))
        return out


def loadPCDFile(path, with_normals=False):
    """pcl::io::loadPCDFile<pcl::PointXYZ> (test/test.cpp:194) without PCL: (n, 3) float32 xyz
    (and normals when asked; zeros if the file has none)."""
    info = capi.PcdInfo()
    n = capi.lib().lom_pcd_read(str(path).encode(), None, None, 0, C.byref(info))
    if n < 0:
        raise LomError(int(n), capi.lib().lom_pcd_last_error().decode())
    xyz = np.empty((n, 3), np.float32)
    nrm = np.empty((n, 3), np.float32) if with_normals else None
    m = capi.lib().lom_pcd_read(str(path).encode(), xyz.ctypes.data, nrm.ctypes.data if with_normals else None, n, None)
    if m < 0:
        raise LomError(int(m), capi.lib().lom_pcd_last_error().decode())
    return (xyz, nrm) if with_normals else xyz


# sensor_msgs/msg/PointField datatypes
PF_INT8, PF_UINT8, PF_INT16, PF_UINT16, PF_INT32, PF_UINT32, PF_FLOAT32, PF_FLOAT64 = range(1, 9)


def fromROSMsg(data, fields, width, height=1, point_step=None, row_step=None, is_bigendian=False):
    """pcl::fromROSMsg into PointCloud<PointXYZIRT> (src/lidar_odometry_node.cpp:47-48) on the members of a
    sensor_msgs/PointCloud2: `data` the payload bytes, `fields` a list of (name, offset, datatype, count).
    Returns (POINT_XYZIRT records, names of the point type's fields the message did not carry)."""
    buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).ravel()
    arr = (capi.Pc2Field * max(len(fields), 1))()
    for i, (name, offset, datatype, count) in enumerate(fields):
        arr[i] = capi.Pc2Field(name.encode(), offset, datatype, count)
    if point_step is None:
        raise ValueError("point_step is required")
    view = capi.Pc2View(height, width, arr, len(fields), 1 if is_bigendian else 0, point_step,
                        row_step if row_step is not None else width * point_step, buf.ctypes.data, buf.size)
    missing = C.c_uint32(0)
    n = capi.lib().lom_pointcloud2_unpack(C.byref(view), None, 0, C.byref(missing))
    if n < 0:
        raise LomError(int(n), capi.lib().lom_pointcloud2_last_error().decode())
    out = np.empty(n, capi.POINT_XYZIRT)
    m = capi.lib().lom_pointcloud2_unpack(C.byref(view), out.ctypes.data, n, None)
    if m < 0:
        raise LomError(int(m), capi.lib().lom_pointcloud2_last_error().decode())
    names = ("x", "y", "z", "intensity", "ring", "time")
    return out, [names[k] for k in range(6) if missing.value >> k & 1]


def toROSMsg(cloud):
    """pcl::toROSMsg (src/lidar_odometry_node.cpp:61,71): an (n, 3) float32 array becomes a PointCloud<PointXYZ>
    message, POINT_XYZIRT records a PointCloud<PointXYZIRT> one.  Returns a dict of the PointCloud2 members."""
    arr = (capi.Pc2Field * 6)()
    step = C.c_uint32(0)
    cloud = np.asarray(cloud)
    if cloud.dtype == capi.POINT_XYZIRT:
        nf = capi.lib().lom_pointcloud2_layout(1, arr, C.byref(step))
        data = np.ascontiguousarray(cloud).tobytes()
        n = len(cloud)
    else:
        xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        nf = capi.lib().lom_pointcloud2_layout(0, arr, C.byref(step))
        n = len(xyz)
        out = np.empty(16 * n, np.uint8)
        w = capi.lib().lom_pointcloud2_pack_xyz(xyz.ctypes.data, n, 12, out.ctypes.data, out.size)
        if w < 0:
            raise LomError(int(w), capi.lib().lom_pointcloud2_last_error().decode())
        data = out.tobytes()
    return {"height": 1, "width": n, "fields": [(arr[i].name.decode(), arr[i].offset, arr[i].datatype, arr[i].count) for i in range(nf)],
            "is_bigendian": False, "point_step": step.value, "row_step": step.value * n, "data": data, "is_dense": True}


class LidarOdometry:
    """reference src/lidar_odometry.{h,cpp}; `params` overrides LidarOdometry::Params defaults by name."""

    def __init__(self, device=0, **params):
        p = capi.OdometryParams()
        capi.lib().lom_odometry_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown parameter {k}")
            setattr(p, k, v)
        h = C.c_void_p()
        rc = capi.lib().lom_odometry_create(C.byref(p), int(device), C.byref(h))
        if rc != 0:
            capi.check(rc, None)
        self._h = h
        self.params = p

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and capi is not None:
            capi.lib().lom_odometry_destroy(h)
            self._h = None

    def setOption(self, option, value):
        """lom_odometry_set_option: switches of the pipeline and of its keyframe handle (capi.OPT_*)."""
        rc = capi.lib().lom_odometry_set_option(self._h, int(option), int(value))
        if rc != 0:
            raise LomError(int(rc), "lom_odometry_set_option")

    def debugCounter(self, which=capi.COUNTER_GRID_REDOS):
        return int(capi.lib().lom_odometry_debug_counter(self._h, int(which)))

    def setClassifier(self, kind, params=None):
        """lom_odometry_set_classifier: capi.CLASSIFIER_RINGS (the reference's, the default) or
        capi.CLASSIFIER_NEIGHBOURHOOD for clouds without rings (params required: neighbourhoodParams)."""
        p = neighbourhoodParams(params) if params is not None else None
        rc = capi.lib().lom_odometry_set_classifier(self._h, int(kind), C.byref(p) if p is not None else None)
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_set_classifier")

    def setCarve(self, params=None):
        """lom_odometry_set_carve: with parameters (carveParams), every keyframe update carves free space along the
        frame's rays before it inserts them; None (the default) launches nothing."""
        p = carveParams(params) if params is not None else None
        rc = capi.lib().lom_odometry_set_carve(self._h, C.byref(p) if p is not None else None)
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_set_carve")

    def carveStats(self):
        """The last keyframe update's carve (capi.CarveStats as a dict); None while none has run."""
        st = capi.CarveStats()
        rc = capi.lib().lom_odometry_get_carve_stats(self._h, C.byref(st))
        if rc == capi.ERR_STATE:
            return None
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_get_carve_stats")
        return st.asdict()

    def setRebuildVotes(self, params=None):
        """lom_odometry_set_rebuild_votes: with parameters (voteParams), rebuildKeyframe lets the scans vote the movers
        out of the keyframe it has assembled (VoxelGrid.carveScans); None (the default) changes nothing."""
        p = voteParams(params) if params is not None else None
        rc = capi.lib().lom_odometry_set_rebuild_votes(self._h, C.byref(p) if p is not None else None)
        if rc != 0:
            raise LomError(int(rc), "lom_odometry_set_rebuild_votes")

    def rebuildVoteStats(self):
        """The last rebuild's votes (capi.VoteStats as a dict); None while none has run."""
        st = capi.VoteStats()
        rc = capi.lib().lom_odometry_get_rebuild_vote_stats(self._h, C.byref(st))
        if rc == capi.ERR_STATE:
            return None
        if rc != 0:
            raise LomError(int(rc), "lom_odometry_get_rebuild_vote_stats")
        return st.asdict()

    def processCloud(self, input_cloud):                   # lidar_odometry.cpp:22-77
        a = _cloud(input_cloud)
        rc = capi.lib().lom_odometry_process_cloud(self._h, a.ctypes.data, len(a))
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "")

    def hintNext(self, cloud):
        """The frame that will come after the next processCloud (lom_odometry_hint_next): its upload is sent ahead while
        that call's align runs.  The array is kept alive here until the hint is replaced."""
        self._hinted = _cloud(cloud)
        rc = capi.lib().lom_odometry_hint_next(self._h, self._hinted.ctypes.data, len(self._hinted))
        if rc != 0:
            raise LomError(int(rc), "lom_odometry_hint_next")
        return self._hinted

    def processSequence(self, clouds):
        """processCloud of every frame of `clouds`, in order, issued from compiled code (lom_odometry_process_sequence): the
        reference's caller is the C++ node -- no interpreter between two frames."""
        arrs = [_cloud(c) for c in clouds]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        ns = (C.c_size_t * len(arrs))(*[len(a) for a in arrs])
        done = C.c_size_t(0)
        rc = capi.lib().lom_odometry_process_sequence(self._h, ptrs, ns, len(arrs), C.byref(done))
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), (text.decode() if text else "") + f" (frame {done.value} of the sequence)")

    @staticmethod
    def processBatch(odometries, clouds):
        """One frame for each of several distinct odometries on one device (lom_odometry_process_batch): for each exactly
        what processCloud would do, with the aligns of all streams run as one call.  Raises LomError if any stream failed
        (its `statuses` holds the per-stream codes); the other streams have still advanced."""
        if len(odometries) != len(clouds):
            raise ValueError("one cloud per odometry")
        k = len(odometries)
        arrs = [_cloud(c) for c in clouds]
        hs = (C.c_void_p * max(k, 1))(*[o._h for o in odometries])
        ptrs = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in arrs])
        ns = (C.c_size_t * max(k, 1))(*[len(a) for a in arrs])
        st = (C.c_int * max(k, 1))()
        rc = capi.lib().lom_odometry_process_batch(hs, ptrs, ns, k, st)
        if rc != 0:
            codes = [int(st[i]) for i in range(k)] if rc != capi.ERR_ARG or any(st[i] for i in range(k)) else [int(rc)] * k
            bad = [i for i, c in enumerate(codes) if c != 0]
            texts = []
            for i in bad:
                t = capi.lib().lom_odometry_last_error(odometries[i]._h)
                texts.append(f"stream {i}: {t.decode() if t else ''}")
            err = LomError(int(rc), "; ".join(texts))
            err.statuses = codes
            raise err

    def setQualityReport(self, on, min_eig_t=0.0, min_eig_r=0.0):
        """LOM_OPT_QUALITY_REPORT: every frame that aligns also gets a quality report (getQuality)."""
        rc = capi.lib().lom_odometry_set_quality_thresholds(self._h, float(min_eig_t), float(min_eig_r))
        if rc != 0:
            raise LomError(int(rc), "lom_odometry_set_quality_thresholds")
        self.setOption(capi.OPT_QUALITY_REPORT, 1 if on else 0)

    def getQuality(self, raw=False):
        """The report of the last frame that aligned (a dict as quality_report() returns; raw=True: the ctypes struct).
        LomError(LOM_ERR_STATE) before the first aligned frame or with the option off."""
        rep = capi.QualityReport()
        rc = capi.lib().lom_odometry_get_quality(self._h, C.byref(rep))
        if rc != 0:
            raise LomError(int(rc), "no quality report: the option is off or no frame has aligned yet")
        return rep if raw else rep.asdict()

    def getCurrentPose(self):                              # lidar_odometry.cpp:87-89
        p = capi.Pose()
        capi.check(capi.lib().lom_odometry_get_pose(self._h, C.byref(p)))
        return Pose3D._from(p)

    def getTempCloud(self):                                # lidar_odometry.h:73-75
        """The deskewed input cloud of the last processCloud (None before the first frame)."""
        n = capi.check(capi.lib().lom_odometry_get_temp_cloud(self._h, None, 0))
        if n == 0:
            return None
        out = np.empty(n, capi.POINT_XYZIRT)
        capi.check(capi.lib().lom_odometry_get_temp_cloud(self._h, out.ctypes.data, n))
        return out

    def placeDescriptor(self, db, add=False):
        """lom_odometry_place_descriptor: the place descriptor of the last frame's deskewed cloud (getTempCloud) through
        the PlaceDatabase `db`; add=True also stores it and returns (descriptor, id).  LomError(LOM_ERR_STATE) before the
        first frame."""
        out = np.empty(db.shape, np.float32)
        id_ = C.c_int64(-1)
        rc = capi.lib().lom_odometry_place_descriptor(self._h, db.handle, 1 if add else 0, out.ctypes.data, C.byref(id_))
        if rc != 0:
            text = capi.lib().lom_place_db_last_error(db.handle)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_place_descriptor")
        return (out, int(id_.value)) if add else out

    def archiveScan(self, archive):
        """lom_odometry_archive_scan: the last frame's update cloud becomes a new scan of the ScanArchive; returns its
        id.  LomError(LOM_ERR_STATE) before the first frame."""
        id_ = C.c_int64(-1)
        rc = capi.lib().lom_odometry_archive_scan(self._h, archive.handle, C.byref(id_))
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_archive_scan")
        return int(id_.value)

    def archiveDeskewed(self, archive):
        """lom_odometry_archive_deskewed: the last frame's deskewed cloud (getTempCloud), every point and no normals,
        becomes a new scan of the ScanArchive; returns its id.  LomError(LOM_ERR_STATE) before the first frame."""
        id_ = C.c_int64(-1)
        rc = capi.lib().lom_odometry_archive_deskewed(self._h, archive.handle, C.byref(id_))
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_archive_deskewed")
        return int(id_.value)

    def occupancyScan(self, grid, ray_params):
        """lom_odometry_occupancy_scan: that cloud at the current pose votes on the OccupancyGrid; returns the stats."""
        p = occupancyRayParams(ray_params)
        st = capi.OccupancyStats()
        rc = capi.lib().lom_odometry_occupancy_scan(self._h, grid.handle, C.byref(p), C.byref(st))
        if rc != 0:
            text = capi.lib().lom_occupancy_last_error(grid.handle)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_occupancy_scan")
        return st.asdict()

    def elevationScan(self, grid, point_params):
        """lom_odometry_elevation_scan: that cloud at the current pose into the ElevationGrid; returns the stats."""
        p = elevationPointParams(point_params)
        st = capi.ElevationStats()
        rc = capi.lib().lom_odometry_elevation_scan(self._h, grid.handle, C.byref(p), C.byref(st))
        if rc != 0:
            text = capi.lib().lom_elevation_last_error(grid.handle)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_elevation_scan")
        return st.asdict()

    def rebuildKeyframe(self, archive, ids, poses, new_current):
        """lom_odometry_rebuild_keyframe: the keyframe again from the archive's scans `ids` at `poses`, culled at
        keyframe_cleanup_range around `new_current` (a Pose3D), which becomes the current pose; returns the stats."""
        ids, p = _assemble_args(ids, poses)
        st = capi.AssembleStats()
        rc = capi.lib().lom_odometry_rebuild_keyframe(self._h, archive.handle, ids.ctypes.data, p.ctypes.data, len(ids),
                                                      C.byref(new_current._c()), C.byref(st))
        if rc != 0:
            text = capi.lib().lom_odometry_last_error(self._h)
            raise LomError(int(rc), text.decode() if text else "lom_odometry_rebuild_keyframe")
        return st.asdict()

    def debugSetState(self, previous, current, keyframe_xyz=None, keyframe_normals=None):
        """Test hook: overwrite the two poses and, if given, rebuild the keyframe from a full export
        (creation order, insertion order inside a voxel: re-inserting it reproduces the map)."""
        if keyframe_xyz is not None:
            kf = capi.lib().lom_odometry_keyframe(self._h)
            xyz, nrm = capi.xyz_array(keyframe_xyz), capi.xyz_array(keyframe_normals)
            capi.check(capi.lib().lom_map_clear(kf, float(self.params.keyframe_voxel_size)), kf)
            capi.check(capi.lib().lom_map_add_points(kf, xyz.ctypes.data, nrm.ctypes.data, len(xyz), 12), kf)
        capi.check(capi.lib().lom_odometry_debug_set_state(self._h, C.byref(previous._c()), C.byref(current._c())))

    def getFullKeyFrameCloudWithNormals(self):
        kf = capi.lib().lom_odometry_keyframe(self._h)
        n = capi.check(capi.lib().lom_map_export(kf, capi.EXPORT_FULL, None, None, 0), kf)
        xyz, nrm = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        if n:
            capi.check(capi.lib().lom_map_export(kf, capi.EXPORT_FULL, xyz.ctypes.data, nrm.ctypes.data, n), kf)
        return xyz, nrm

    def _keyframe_export(self, mode):
        kf = capi.lib().lom_odometry_keyframe(self._h)
        n = capi.check(capi.lib().lom_map_export(kf, mode, None, None, 0), kf)
        xyz = np.empty((n, 3), np.float32)
        if n:
            capi.check(capi.lib().lom_map_export(kf, mode, xyz.ctypes.data, None, n), kf)
        return xyz

    def getKeyFrameCloud(self):                            # lidar_odometry.cpp:79-81
        return self._keyframe_export(capi.EXPORT_FIRST_PER_VOXEL)

    def getFullKeyFrameCloud(self):                        # lidar_odometry.cpp:83-85
        return self._keyframe_export(capi.EXPORT_FULL_NO_NORMALS)

    @property
    def stats(self):
        s = capi.OdometryFrameStats()
        capi.check(capi.lib().lom_odometry_get_stats(self._h, C.byref(s)))
        return s.asdict()
