"""ctypes binding of include/pvlm.h.  Thin: argument marshalling and error translation only."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

POINT2PLANE_METER, POINT2PLANE_ANGLE, POINT2LINE_METER, POINT2LINE_ANGLE, PLANE2PLANE_GLOBAL, PLANE_IOU = range(6)
ERR_CAPACITY = -5            # pvlm_status PVLM_ERR_CAPACITY
FLAG_NORMALIZE_DISTANCE = 1
FLAG_ASSOC_KEEP_INDICES = 0x100   # pvlm_assoc_point2plane: keep query / neighbour indices for pvlm_assoc_point2plane_debug
FLAG_ASSOC_EXACT_FIT = 0x200      # pvlm_assoc_point2plane: the reference's QR for every query (bit-identical records)
LOSS_NONE, LOSS_HUBER = 0, 1
BA_KINDS = {"angle1": 0, "angle2": 1, "pixel": 2}    # pvlm_ba_kind (K31)
FILTER_MODES = {"pixel": 0, "angle": 1}              # pvlm_filter_mode (K31)
PAIR_BLOCK = 121
STRIDE = {0: 7, 1: 7, 2: 9, 3: 9, 4: 10, 5: 12}

# every symbol include/pvlm.h declares (tests/test_abi.py checks the header and the .so against it)
ABI_SYMBOLS = [
    "pvlm_create", "pvlm_destroy", "pvlm_last_error", "pvlm_version", "pvlm_set_stream", "pvlm_use_own_stream", "pvlm_synchronize",
    "pvlm_timer_start", "pvlm_timer_stop", "pvlm_device_info", "pvlm_profile_enable", "pvlm_profile_read", "pvlm_set_poses", "pvlm_set_poses_dev",
    "pvlm_resset_upload", "pvlm_resset_destroy", "pvlm_resset_info", "pvlm_resset_download", "pvlm_eval",
    "pvlm_eval_dev", "pvlm_eval_pair_blocks", "pvlm_eval_pair_blocks_dev", "pvlm_neq_create", "pvlm_neq_destroy",
    "pvlm_neq_size", "pvlm_neq_accumulate_dev", "pvlm_neq_accumulate", "pvlm_neq_accumulate_async", "pvlm_neq_accumulate_sets", "pvlm_resset_set_pose_ids", "pvlm_comm_unique_id", "pvlm_comm_create",
    "pvlm_comm_destroy", "pvlm_allreduce_sum_f64", "pvlm_scan_upload", "pvlm_scan_upload_batch", "pvlm_scan_destroy",
    "pvlm_knn", "pvlm_centre_orders", "pvlm_assoc_point2plane", "pvlm_assoc_point2plane_debug", "pvlm_line2line_votes",
    "pvlm_cam_to_image_f32", "pvlm_cam_to_image_f64", "pvlm_image_to_cam_f32", "pvlm_image_to_cam_f64",
    "pvlm_cam_lidar_votes", "pvlm_line2line_votes_batch", "pvlm_line2line_best_batch", "pvlm_cam_lidar_votes_batch", "pvlm_cam_lidar_votes_batch_sparse",
    "pvlm_cam_to_image_f32_dev", "pvlm_image_to_cam_f32_dev", "pvlm_project_lidar_depth", "pvlm_spd_solve", "pvlm_spd_solve_blocks", "pvlm_mvs_init_conf_map", "pvlm_mvs_filter_depth", "pvlm_mvs_filter_depth_refine", "pvlm_mvs_propagate", "pvlm_mvs_propagate_sequential", "pvlm_mvs_views_estimate_sequential", "pvlm_mvs_views_estimate_sequential_batch", "pvlm_mvs_views_create", "pvlm_mvs_views_destroy", "pvlm_mvs_views_upload", "pvlm_mvs_views_download",
    "pvlm_mvs_views_snapshot_depth", "pvlm_mvs_views_estimate", "pvlm_mvs_views_filter_refine",
    "pvlm_ba_create", "pvlm_ba_destroy", "pvlm_ba_structure", "pvlm_ba_packed_size", "pvlm_ba_get_points", "pvlm_ba_set_points", "pvlm_ba_set_constant",
    "pvlm_ba_eval", "pvlm_ba_reduce", "pvlm_ba_step", "pvlm_ba_cost", "pvlm_ba_accept",
    "pvlm_reserve", "pvlm_reserve_staging", "pvlm_preload", "pvlm_trim", "pvlm_mem_info", "pvlm_graph_begin", "pvlm_graph_end", "pvlm_graph_launch", "pvlm_graph_destroy",
    "pvlm_allreduce_sum_f64_host", "pvlm_host_alloc", "pvlm_host_free", "pvlm_eval_host_async", "pvlm_eval_wrench_host_async", "pvlm_eval_force_host_async", "pvlm_line2line_residuals", "pvlm_mvs_init_depth_normal", "pvlm_mvs_remove_small_segments", "pvlm_mvs_depth_to_cloud", "pvlm_mvs_views_depth_to_cloud",
    "pvlm_spd_plan_info", "pvlm_spd_plan_schedule", "pvlm_spd_plan_tail", "pvlm_spd_one_launch", "pvlm_spd_plan_prefetch", "pvlm_spd_plan_prefetch_hits", "pvlm_line_grow_batch", "pvlm_line_grow_begin", "pvlm_line_grow_finish", "pvlm_line_grow_scan", "pvlm_line_grow_destroy", "pvlm_ring_extract_batch", "pvlm_ring_extract_batch_picks", "pvlm_ring_debug_sort", "pvlm_undistort_batch", "pvlm_assoc_point2plane_stats", "pvlm_assoc_point2plane_stats2", "pvlm_scan_transform_batch", "pvlm_scan_set_pose", "pvlm_scan_cloud_info", "pvlm_scan_cloud_fetch", "pvlm_ring_batch_scan", "pvlm_ring_batch_fetch", "pvlm_ring_batch_timing", "pvlm_ring_batch_destroy",
    "pvlm_fuse_scans", "pvlm_fuse_scans_dev",
    "pvlm_colorize_scans", "pvlm_colorize_scans_dev", "pvlm_colorize_debug_hsv",
    "pvlm_ba_create_kind", "pvlm_ba_info", "pvlm_filter_tracks",
    "pvlm_triangulate_tracks", "pvlm_filter_tracks_far",
    "pvlm_descset_create", "pvlm_descset_destroy", "pvlm_match_knn2", "pvlm_match_pairs",
    "pvlm_essential_acransac", "pvlm_filter_image_pairs",
    "pvlm_vlad_kmeans", "pvlm_vlad_embed", "pvlm_vladset_read", "pvlm_vlad_neighbors", "pvlm_vladset_destroy",
    "pvlm_resset_plane_runs", "pvlm_resset_point_table", "pvlm_resset_point_table_debug",
    "pvlm_refine_relative_poses", "pvlm_relpose_workgroup_size",
    "pvlm_transavg_dlt", "pvlm_transavg_solve", "pvlm_transavg_group_size", "pvlm_transavg_bata", "pvlm_bata_group_size",
    "pvlm_rotavg_l1", "pvlm_rotavg_l2", "pvlm_rotavg_group_size", "pvlm_rotavg_least_square",
    "pvlm_transavg_chordal", "pvlm_transavg_lud", "pvlm_transdir_group_size",
    "pvlm_transavg_l1", "pvlm_translp_group_size",
    "pvlm_triplets_find", "pvlm_triplets_filter", "pvlm_triplet_group_size",
    "pvlm_mvs_select_neighbors_sfm", "pvlm_mvs_neighbor_sfm_score_row", "pvlm_neighbor_sfm_tile_cols",
    "pvlm_depth_completion", "pvlm_compute_depth_images",
    "pvlm_depthset_compute", "pvlm_depthset_create", "pvlm_depthset_upload", "pvlm_depthset_info", "pvlm_depthset_read", "pvlm_depthset_destroy",
    "pvlm_set_translation_scales", "pvlm_scale_workgroup_size",
    "pvlm_sift_extract", "pvlm_sift_pyramid_debug",
]


class PvlmError(RuntimeError):
    pass


def lib_path():
    # PVLM_LIB selects another build of the same library (measured kernel variants); never a different implementation
    return os.environ.get("PVLM_LIB") or os.path.join(_HERE, "libpvlm.so")


_LIB = None


def load_library():
    """Loads libpvlm.so.  Raises if it has not been built (python -m panovlm_amd.build): the HIP
    extension IS the product, nothing else can stand in for it."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise PvlmError("libpvlm.so is missing (%s): build it with `python -m panovlm_amd.build` "
                        "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
    try:
        # PyTorch ships its own libamdhip64 with the same SONAME; when it is in the process it must
        # be loaded first so that one HIP runtime serves both.
        import sys
        if "torch" in sys.modules or os.environ.get("PVLM_PRELOAD_TORCH", "0") == "1":
            import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    lib.pvlm_last_error.restype = C.c_char_p
    lib.pvlm_version.restype = C.c_char_p
    lib.pvlm_neq_size.restype = C.c_int64
    lib.pvlm_ba_packed_size.restype = C.c_int64
    _LIB = lib
    return lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


class Graph:
    """A captured step (pvlm_graph_*): launch() replays it on the context's stream."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle

    def launch(self):
        self.ctx._check(self.ctx.lib.pvlm_graph_launch(self.ctx._h, self._h), "pvlm_graph_launch")

    def close(self):
        if self._h and self.ctx._h:
            self.ctx.lib.pvlm_graph_destroy(self.ctx._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, device=0):
        self.lib = load_library()
        self._h = C.c_void_p()
        rc = self.lib.pvlm_create(C.c_int(device), C.byref(self._h))
        if rc != 0:
            raise PvlmError("pvlm_create(device=%d) failed with status %d: no usable HIP device "
                            "(this package has no CPU path)" % (device, rc))
        self.device = device
        self._bound_stream = None      # the hipStream_t handle set_stream bound last; None = the context's own stream

    def _check(self, rc, what):
        if rc != 0:
            raise PvlmError("%s failed (%d): %s" % (what, rc, self.lib.pvlm_last_error(self._h).decode()))

    def close(self):
        if self._h:
            self.lib.pvlm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        """Issue all kernels on this hipStream_t (0 / None = HIP's default stream, e.g. torch's default stream)."""
        self._check(self.lib.pvlm_set_stream(self._h, C.c_void_p(stream_handle or 0)), "pvlm_set_stream")
        self._bound_stream = int(stream_handle or 0)

    def use_own_stream(self):
        self._check(self.lib.pvlm_use_own_stream(self._h), "pvlm_use_own_stream")
        self._bound_stream = None

    def synchronize(self):
        self._check(self.lib.pvlm_synchronize(self._h), "pvlm_synchronize")

    def reserve(self, nbytes):
        """One free range of `nbytes` in the context's device pool (hipMalloc is 40-70 ms per GB: pay it at set-up)."""
        self._check(self.lib.pvlm_reserve(self._h, C.c_int64(int(nbytes))), "pvlm_reserve")

    def trim(self):
        self._check(self.lib.pvlm_trim(self._h), "pvlm_trim")

    def mem_info(self):
        r, u, p, n = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.pvlm_mem_info(self._h, C.byref(r), C.byref(u), C.byref(p), C.byref(n)), "pvlm_mem_info")
        return dict(reserved=r.value, in_use=u.value, peak=p.value, device_allocs=n.value)

    def comm_unique_id(self):
        """128-byte RCCL id (rank 0 creates it, the launcher carries it to the other ranks)."""
        buf = (C.c_ubyte * 128)()
        self._check(self.lib.pvlm_comm_unique_id(self._h, buf), "pvlm_comm_unique_id")
        return bytes(buf)

    def host_alloc(self, nbytes):
        """Page-locked host memory (pvlm_host_alloc) as a numpy float64 array; free with host_free(array)."""
        p = C.c_void_p()
        self._check(self.lib.pvlm_host_alloc(self._h, C.c_int64(int(nbytes)), C.byref(p)), "pvlm_host_alloc")
        n = max(int(nbytes) // 8, 1)
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(n,))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def host_free(self, array):
        p = getattr(self, "_pinned", {}).pop(array.ctypes.data, None)
        if p is not None:
            self._check(self.lib.pvlm_host_free(self._h, p), "pvlm_host_free")

    def graph_begin(self):
        self._check(self.lib.pvlm_graph_begin(self._h), "pvlm_graph_begin")

    def graph_end(self):
        g = C.c_void_p()
        self._check(self.lib.pvlm_graph_end(self._h, C.byref(g)), "pvlm_graph_end")
        return Graph(self, g)

    def timer_start(self):
        self._check(self.lib.pvlm_timer_start(self._h), "pvlm_timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._check(self.lib.pvlm_timer_stop(self._h, C.byref(ms)), "pvlm_timer_stop")
        return float(ms.value)

    def device_info(self):
        cu = C.c_int(); hbm = C.c_int64(); name = C.create_string_buffer(64)
        self._check(self.lib.pvlm_device_info(self._h, C.byref(cu), C.byref(hbm), name, C.c_int(64)), "pvlm_device_info")
        return dict(cu_count=cu.value, hbm_bytes=hbm.value, arch=name.value.decode())

    def profile_enable(self, on=True):
        self._check(self.lib.pvlm_profile_enable(self._h, C.c_int(1 if on else 0)), "pvlm_profile_enable")

    def profile_read(self, which=0):
        ms = C.c_double(); n = C.c_int64()
        self._check(self.lib.pvlm_profile_read(self._h, C.c_int(which), C.byref(ms), C.byref(n)), "pvlm_profile_read")
        return float(ms.value), int(n.value)

    def set_poses(self, angle_axis, translation):
        aa = _f64(angle_axis).reshape(-1, 3); t = _f64(translation).reshape(-1, 3)
        assert aa.shape == t.shape
        self._check(self.lib.pvlm_set_poses(self._h, C.c_int(aa.shape[0]), _p(aa, C.c_double), _p(t, C.c_double)), "pvlm_set_poses")

    def set_poses_dev(self, n, d_aa_ptr, d_t_ptr):
        self._check(self.lib.pvlm_set_poses_dev(self._h, C.c_int(n), C.c_void_p(d_aa_ptr), C.c_void_p(d_t_ptr)), "pvlm_set_poses_dev")

    # --- equirectangular -------------------------------------------------------------------------
    def cam_to_image(self, rows, cols, cam):
        cam = np.ascontiguousarray(cam)
        n = cam.shape[0]
        if cam.dtype == np.float32:
            px = np.empty((n, 2), np.float32)
            self._check(self.lib.pvlm_cam_to_image_f32(self._h, C.c_int(rows), C.c_int(cols), C.c_int64(n), _p(cam, C.c_float), _p(px, C.c_float)), "pvlm_cam_to_image_f32")
        else:
            cam = _f64(cam); px = np.empty((n, 2), np.float64)
            self._check(self.lib.pvlm_cam_to_image_f64(self._h, C.c_int(rows), C.c_int(cols), C.c_int64(n), _p(cam, C.c_double), _p(px, C.c_double)), "pvlm_cam_to_image_f64")
        return px

    def image_to_cam(self, rows, cols, px, r=1.0):
        px = np.ascontiguousarray(px)
        n = px.shape[0]
        if px.dtype == np.float32:
            cam = np.empty((n, 3), np.float32)
            self._check(self.lib.pvlm_image_to_cam_f32(self._h, C.c_int(rows), C.c_int(cols), C.c_int64(n), _p(px, C.c_float), C.c_float(r), _p(cam, C.c_float)), "pvlm_image_to_cam_f32")
        else:
            px = _f64(px); cam = np.empty((n, 3), np.float64)
            self._check(self.lib.pvlm_image_to_cam_f64(self._h, C.c_int(rows), C.c_int(cols), C.c_int64(n), _p(px, C.c_double), C.c_double(r), _p(cam, C.c_double)), "pvlm_image_to_cam_f64")
        return cam

    def cam_lidar_votes(self, rows, cols, lines, lidar_scan, T_cl):
        lines = _f32(lines).reshape(-1, 4); T = _f64(T_cl).reshape(16)
        votes = np.zeros((lines.shape[0], max(1, lidar_scan.n_segments)), np.int32)
        self._check(self.lib.pvlm_cam_lidar_votes(self._h, C.c_int(rows), C.c_int(cols), _p(lines, C.c_float), C.c_int(lines.shape[0]),
                                                  lidar_scan._h, _p(T, C.c_double), _p(votes, C.c_int32)), "pvlm_cam_lidar_votes")
        return votes[:, :lidar_scan.n_segments]

    def cam_to_image_f32_dev(self, rows, cols, n, d_cam_ptr, d_px_ptr):
        self._check(self.lib.pvlm_cam_to_image_f32_dev(self._h, C.c_int(rows), C.c_int(cols), C.c_int64(n), C.c_void_p(d_cam_ptr), C.c_void_p(d_px_ptr)),
                    "pvlm_cam_to_image_f32_dev")

    def image_to_cam_f32_dev(self, rows, cols, n, d_px_ptr, r, d_cam_ptr):
        self._check(self.lib.pvlm_image_to_cam_f32_dev(self._h, C.c_int(rows), C.c_int(cols), C.c_int64(n), C.c_void_p(d_px_ptr), C.c_float(r),
                                                       C.c_void_p(d_cam_ptr)), "pvlm_image_to_cam_f32_dev")

    def spd_solve(self, A, B):
        """Dense SPD solve on the GPU (blocked Cholesky kernels of libpvlm.so): returns (X, info)."""
        A = _f64(A); n = A.shape[0]
        B2 = np.asfortranarray(np.asarray(B, np.float64).reshape(n, -1))
        info = C.c_int()
        self._check(self.lib.pvlm_spd_solve(self._h, C.c_int(n), C.c_int(B2.shape[1]), _p(A, C.c_double),
                                            B2.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info)), "pvlm_spd_solve")
        return np.ascontiguousarray(B2).reshape(np.shape(B)), info.value

    def spd_solve_blocks(self, n, row_idx, col_idx, mirror, blocks, scale, diag_add, rhs):
        row_idx = _i32(row_idx).reshape(-1, 6); col_idx = _i32(col_idx).reshape(-1, 6); blocks = _f64(blocks).reshape(-1, 36); mirror = _i32(mirror)
        x = _f64(rhs).copy(); info = C.c_int()
        self._check(self.lib.pvlm_spd_solve_blocks(self._h, C.c_int(n), C.c_int(len(blocks)), _p(row_idx, C.c_int), _p(col_idx, C.c_int), _p(mirror, C.c_int),
                                                   _p(blocks, C.c_double), _p(_f64(scale), C.c_double), _p(_f64(diag_add), C.c_double),
                                                   _p(x, C.c_double), C.byref(info)), "pvlm_spd_solve_blocks")
        return x, info.value

    def line_grow_batch(self, clouds, two_halves=False):
        """pvlm_line_grow_batch (K27): the line segments upstream's walk keeps for every edge cloud (n x >= 3 float32 each).  Returns one dict per cloud:
        status, seg_task, seg_offset, members, coeffs (n_segments x 6); the last call's kernel_ms / tasks_run under those keys of the first dict.
        two_halves: through pvlm_line_grow_begin / _finish."""
        class _Cloud(C.Structure):
            _fields_ = [("xyz", C.POINTER(C.c_float)), ("n", C.c_int), ("stride_floats", C.c_int)]

        class _Result(C.Structure):
            _fields_ = [("status", C.c_int), ("n_points", C.c_int), ("n_segments", C.c_int), ("seg_task", C.POINTER(C.c_int)), ("seg_offset", C.POINTER(C.c_int)),
                        ("members", C.POINTER(C.c_int)), ("coeffs", C.POINTER(C.c_double)), ("kernel_ms", C.c_double), ("tasks_run", C.c_longlong)]
        arrs = [np.ascontiguousarray(c, np.float32).reshape(len(c), -1) if len(c) else np.zeros((0, 3), np.float32) for c in clouds]
        descs = (_Cloud * max(len(arrs), 1))()
        for k, a in enumerate(arrs):
            descs[k].xyz = a.ctypes.data_as(C.POINTER(C.c_float)); descs[k].n = len(a); descs[k].stride_floats = a.shape[1] if len(a) else 3
        h = C.c_void_p()
        if two_halves:
            self._check(self.lib.pvlm_line_grow_begin(self._h, C.c_int(len(arrs)), descs, C.byref(h)), "pvlm_line_grow_begin")
            st = self.lib.pvlm_line_grow_finish(self._h, h)
            if st:
                self.lib.pvlm_line_grow_destroy(self._h, h)
                self._check(st, "pvlm_line_grow_finish")
        else:
            self._check(self.lib.pvlm_line_grow_batch(self._h, C.c_int(len(arrs)), descs, C.byref(h)), "pvlm_line_grow_batch")
        out = []
        try:
            for k in range(len(arrs)):
                r = _Result()
                self._check(self.lib.pvlm_line_grow_scan(h, C.c_int(k), C.byref(r)), "pvlm_line_grow_scan")
                ns = r.n_segments
                off = np.ctypeslib.as_array(r.seg_offset, (ns + 1,)).copy() if ns else np.zeros(1, np.int32)
                mem = np.ctypeslib.as_array(r.members, (int(off[-1]),))[int(off[0]):].copy() if ns else np.zeros(0, np.int32)
                out.append(dict(status=r.status, seg_task=np.ctypeslib.as_array(r.seg_task, (ns,)).copy() if ns else np.zeros(0, np.int32), seg_offset=off - off[0], members=mem,
                                coeffs=np.ctypeslib.as_array(r.coeffs, (ns, 6)).copy() if ns else np.zeros((0, 6)), kernel_ms=r.kernel_ms, tasks_run=r.tasks_run))
        finally:
            self.lib.pvlm_line_grow_destroy(self._h, h)
        return out

    def spd_plan_prefetch(self, n, row_idx, col_idx, mirror):
        """pvlm_spd_plan_prefetch: the host half of the plan of this structure starts on a thread of the library; the next spd_solve_blocks with exactly these lists takes it."""
        row_idx = _i32(row_idx).reshape(-1, 6); col_idx = _i32(col_idx).reshape(-1, 6); mirror = _i32(mirror)
        self._check(self.lib.pvlm_spd_plan_prefetch(self._h, C.c_int(n), C.c_int(len(mirror)), _p(row_idx, C.c_int), _p(col_idx, C.c_int), _p(mirror, C.c_int)), "pvlm_spd_plan_prefetch")

    def spd_plan_prefetch_hits(self):
        h = C.c_longlong()
        self._check(self.lib.pvlm_spd_plan_prefetch_hits(self._h, C.byref(h)), "pvlm_spd_plan_prefetch_hits")
        return h.value

    def centre_orders(self, xyz):
        """pvlm_centre_orders: for every centre the positions of all centres ordered by (float squared distance, position) — (n, n) uint16."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); n = len(xyz)
        out = np.zeros((n, n), np.uint16)
        self._check(self.lib.pvlm_centre_orders(self._h, C.c_int(n), _p(xyz, C.c_float), _p(out, C.c_uint16)), "pvlm_centre_orders")
        return out

    def spd_one_launch(self, enable=None):
        """pvlm_spd_one_launch: enable / disable the one-launch form of the tile-sparse factorisation (None: query only); returns the number of solves this context has
        redone with the level launches."""
        fb = C.c_longlong()
        self._check(self.lib.pvlm_spd_one_launch(self._h, C.c_int(-1 if enable is None else (int(enable) if isinstance(enable, int) and not isinstance(enable, bool) else int(bool(enable)))), C.byref(fb)),
                    "pvlm_spd_one_launch")
        return fb.value

    def spd_plan(self):
        """How the last spd_solve_blocks structure is factorised: tile_sparse, update_fraction (pvlm_spd_plan_info) and the schedule (pvlm_spd_plan_schedule):
        levels (0 = column by column), block_columns, padded_rows."""
        ts, lv, bc, pr = C.c_int(), C.c_int(), C.c_int(), C.c_int(); fr = C.c_double()
        self._check(self.lib.pvlm_spd_plan_info(self._h, C.byref(ts), C.byref(fr)), "pvlm_spd_plan_info")
        self._check(self.lib.pvlm_spd_plan_schedule(self._h, C.byref(lv), C.byref(bc), C.byref(pr)), "pvlm_spd_plan_schedule")
        tc, ll = C.c_int(), C.c_int()
        self._check(self.lib.pvlm_spd_plan_tail(self._h, C.byref(tc), C.byref(ll)), "pvlm_spd_plan_tail")
        return dict(tile_sparse=bool(ts.value), update_fraction=fr.value, levels=lv.value, block_columns=bc.value, padded_rows=pr.value, tail_block_columns=tc.value,
                    launched_levels=ll.value)

    def mvs_init_conf_map(self, ref_gray, nei_grays, R_nr, t_nr, depth, normal, half_window=3, step=1, conf=None, nei_depths=None):
        """MVS::InitPatchMap + InitConfMap(use_geometry=False) on the GPU: returns (conf, depth, normal) copies."""
        ref = np.ascontiguousarray(ref_gray, np.uint8); rows, cols = ref.shape
        neis = [np.ascontiguousarray(g, np.uint8) for g in nei_grays]
        ptrs = (C.POINTER(C.c_ubyte) * max(len(neis), 1))(*[g.ctypes.data_as(C.POINTER(C.c_ubyte)) for g in neis])
        R = _f32(R_nr).reshape(-1); t = _f32(t_nr).reshape(-1)
        d = np.array(depth, np.float32, copy=True); nrm = np.array(normal, np.float32, copy=True)
        c = np.zeros((rows, cols), np.float32) if conf is None else np.array(conf, np.float32, copy=True)
        dptrs = None
        if nei_depths is not None:
            nd = [np.ascontiguousarray(x, np.float32) for x in nei_depths]
            dptrs = (C.POINTER(C.c_float) * max(len(nd), 1))(*[x.ctypes.data_as(C.POINTER(C.c_float)) for x in nd])
        self._check(self.lib.pvlm_mvs_init_conf_map(self._h, C.c_int(rows), C.c_int(cols), C.c_int(half_window), C.c_int(step), _p(ref, C.c_ubyte),
                                                    C.c_int(len(neis)), ptrs, _p(R, C.c_float), _p(t, C.c_float), _p(d, C.c_float), _p(nrm, C.c_float),
                                                    _p(c, C.c_float), dptrs), "pvlm_mvs_init_conf_map")
        return c, d, nrm

    def mvs_init_depth_normal(self, rows, cols, lidar_depth16=None, mask=None, min_depth=0.1, max_depth=20.0, keep_lidar_constant=True, seed=1):
        """MVS::InitDepthNormal on the GPU: returns (depth, normal, depth_constant uint8)."""
        l16 = None if lidar_depth16 is None else np.ascontiguousarray(lidar_depth16, np.uint16)
        m = None if mask is None else np.ascontiguousarray(mask, np.float32)
        d = np.zeros((rows, cols), np.float32); n = np.zeros((rows, cols, 3), np.float32); c = np.zeros((rows, cols), np.uint8)
        self._check(self.lib.pvlm_mvs_init_depth_normal(self._h, C.c_int(rows), C.c_int(cols), _p(l16, C.c_uint16), _p(m, C.c_float), C.c_float(min_depth),
                                                        C.c_float(max_depth), C.c_int(1 if keep_lidar_constant else 0), C.c_ulonglong(seed), _p(d, C.c_float),
                                                        _p(n, C.c_float), _p(c, C.c_ubyte)), "pvlm_mvs_init_depth_normal")
        return d, n, c

    def mvs_remove_small_segments(self, depth, normal, conf, depth_diff_threshold=0.01, min_segment=100):
        """MVS::RemoveSmallSegments (host, sequential by construction): returns (depth, normal, conf, removed)."""
        d = np.array(depth, np.float32, copy=True); n = np.array(normal, np.float32, copy=True); c = np.array(conf, np.float32, copy=True)
        rows, cols = d.shape
        k = C.c_int64()
        self._check(self.lib.pvlm_mvs_remove_small_segments(self._h, C.c_int(rows), C.c_int(cols), C.c_float(depth_diff_threshold), C.c_int(min_segment),
                                                            _p(d, C.c_float), _p(n, C.c_float), _p(c, C.c_float), C.byref(k)), "pvlm_mvs_remove_small_segments")
        return d, n, c, int(k.value)

    def mvs_propagate(self, ref_gray, nei_grays, R_nr, t_nr, depth, normal, conf, half_window=3, step=1, nei_depths=None, depth_constant=None, min_depth=0.1,
                      max_depth=20.0, seed=1, max_iter=1, conf_threshold=-1.0, sequential=False):
        """MVS::EstimateDepthMapSingle on the GPU — checkerboard PatchMatch, or (sequential=True) the raster-order sweep the Room /
        Floor configs select, run anti-diagonal by anti-diagonal: returns (depth, normal, conf) copies."""
        ref = np.ascontiguousarray(ref_gray, np.uint8); rows, cols = ref.shape
        neis = [np.ascontiguousarray(g, np.uint8) for g in nei_grays]
        ptrs = (C.POINTER(C.c_ubyte) * max(len(neis), 1))(*[g.ctypes.data_as(C.POINTER(C.c_ubyte)) for g in neis])
        R = _f32(R_nr).reshape(-1); t = _f32(t_nr).reshape(-1)
        d = np.array(depth, np.float32, copy=True); nrm = np.array(normal, np.float32, copy=True); c = np.array(conf, np.float32, copy=True)
        dptrs = None
        if nei_depths is not None:
            nd = [np.ascontiguousarray(x, np.float32) for x in nei_depths]
            dptrs = (C.POINTER(C.c_float) * max(len(nd), 1))(*[x.ctypes.data_as(C.POINTER(C.c_float)) for x in nd])
        dc = None if depth_constant is None else np.ascontiguousarray(depth_constant, np.uint8)
        fn = self.lib.pvlm_mvs_propagate_sequential if sequential else self.lib.pvlm_mvs_propagate
        self._check(fn(self._h, C.c_int(rows), C.c_int(cols), C.c_int(half_window), C.c_int(step), _p(ref, C.c_ubyte), C.c_int(len(neis)),
                       ptrs, _p(R, C.c_float), _p(t, C.c_float), _p(d, C.c_float), _p(nrm, C.c_float), _p(c, C.c_float), dptrs,
                       _p(dc, C.c_ubyte), C.c_float(min_depth), C.c_float(max_depth), C.c_ulonglong(seed), C.c_int(max_iter),
                       C.c_float(conf_threshold)), "pvlm_mvs_propagate_sequential" if sequential else "pvlm_mvs_propagate")
        return d, nrm, c

    def mvs_filter_depth(self, nei_depths, R_nr, t_nr, depth, conf=None, depth_constant=None, thr=0.01):
        """MVS::FilterDepthImage on the GPU: returns (depth_filter, conf_filter)."""
        d = np.ascontiguousarray(depth, np.float32); rows, cols = d.shape
        nd = [np.ascontiguousarray(x, np.float32) for x in nei_depths]
        dptrs = (C.POINTER(C.c_float) * max(len(nd), 1))(*[x.ctypes.data_as(C.POINTER(C.c_float)) for x in nd])
        R = _f32(R_nr).reshape(-1); t = _f32(t_nr).reshape(-1)
        cf = None if conf is None else np.ascontiguousarray(conf, np.float32)
        dc = None if depth_constant is None else np.ascontiguousarray(depth_constant, np.uint8)
        out_d = np.zeros((rows, cols), np.float32); out_c = np.zeros((rows, cols), np.float32)
        self._check(self.lib.pvlm_mvs_filter_depth(self._h, C.c_int(rows), C.c_int(cols), C.c_int(len(nd)), dptrs, _p(R, C.c_float), _p(t, C.c_float),
                                                   _p(d, C.c_float), _p(cf, C.c_float), _p(dc, C.c_ubyte), C.c_float(thr), _p(out_d, C.c_float),
                                                   _p(out_c, C.c_float) if cf is not None else None), "pvlm_mvs_filter_depth")
        return out_d, out_c

    def mvs_depth_to_cloud(self, depth, bgr, T_wc, max_depth=20.0, filter_sky=True, normal=None):
        """MVS::DepthImageToCloud (normal None) / DepthNormalToCloud (normal given; pass filter_sky=False for the reference's behaviour) on the GPU:
        (xyz n x 3 float32, rgb n x 3 uint8[, normal n x 3 float32]) in raster order."""
        d = np.ascontiguousarray(depth, np.float32); rows, cols = d.shape
        c = np.ascontiguousarray(bgr, np.uint8); assert c.shape == (rows, cols, 3)
        T = np.ascontiguousarray(np.asarray(T_wc, np.float64).reshape(-1)[:12])
        nin = None if normal is None else np.ascontiguousarray(normal, np.float32)
        assert nin is None or nin.shape == (rows, cols, 3)
        xyz = np.empty((rows * cols, 3), np.float32); rgb = np.empty((rows * cols, 3), np.uint8)
        nout = None if nin is None else np.empty((rows * cols, 3), np.float32)
        n = C.c_longlong(0)
        self._check(self.lib.pvlm_mvs_depth_to_cloud(self._h, C.c_int(rows), C.c_int(cols), _p(d, C.c_float), _p(c, C.c_ubyte), _p(nin, C.c_float), _p(T, C.c_double),
                                                     C.c_float(max_depth), C.c_int(1 if filter_sky else 0), _p(xyz, C.c_float), _p(rgb, C.c_ubyte), _p(nout, C.c_float),
                                                     C.byref(n)), "pvlm_mvs_depth_to_cloud")
        k = n.value
        return (xyz[:k].copy(), rgb[:k].copy()) if nout is None else (xyz[:k].copy(), rgb[:k].copy(), nout[:k].copy())

    def mvs_filter_depth_refine(self, nei_depths, nei_confs, R_nr, t_nr, depth, conf, depth_constant=None, thr=0.01, min_depth=0.1, max_depth=20.0):
        """MVS::FilterDepthImageRefine on the GPU: returns (depth_filter, conf_filter, conf) — conf = the reference frame's
        conf_map after the call (zeroed where depth <= 0)."""
        d = np.ascontiguousarray(depth, np.float32); rows, cols = d.shape
        nd = [np.ascontiguousarray(x, np.float32) for x in nei_depths]
        nc = [np.ascontiguousarray(x, np.float32) for x in nei_confs]
        assert len(nd) == len(nc)
        dptrs = (C.POINTER(C.c_float) * max(len(nd), 1))(*[x.ctypes.data_as(C.POINTER(C.c_float)) for x in nd])
        cptrs = (C.POINTER(C.c_float) * max(len(nc), 1))(*[x.ctypes.data_as(C.POINTER(C.c_float)) for x in nc])
        R = _f32(R_nr).reshape(-1); t = _f32(t_nr).reshape(-1)
        cf = np.array(conf, np.float32, copy=True, order="C")
        dc = None if depth_constant is None else np.ascontiguousarray(depth_constant, np.uint8)
        out_d = np.zeros((rows, cols), np.float32); out_c = np.zeros((rows, cols), np.float32)
        self._check(self.lib.pvlm_mvs_filter_depth_refine(self._h, C.c_int(rows), C.c_int(cols), C.c_int(len(nd)), dptrs, cptrs, _p(R, C.c_float),
                                                          _p(t, C.c_float), _p(d, C.c_float), _p(cf, C.c_float), _p(dc, C.c_ubyte), C.c_float(thr),
                                                          C.c_float(min_depth), C.c_float(max_depth), _p(out_d, C.c_float), _p(out_c, C.c_float)),
                    "pvlm_mvs_filter_depth_refine")
        return out_d, out_c, cf

    def project_lidar_depth(self, rows, cols, xyz, T_cl, size=3):
        xyz = _f32(xyz).reshape(-1, 3); T = _f64(T_cl).reshape(16)
        out = np.zeros((rows, cols), np.uint16)
        self._check(self.lib.pvlm_project_lidar_depth(self._h, C.c_int(rows), C.c_int(cols), C.c_int64(xyz.shape[0]), _p(xyz, C.c_float),
                                                      _p(T, C.c_double), C.c_uint(size), _p(out, C.c_uint16)), "pvlm_project_lidar_depth")
        return out

    def depth_completion(self, sparse, max_depth, want_f32=True, want_u16=False):
        """pvlm_depth_completion (K37): DepthCompletion (util/DepthCompletion.cpp:154-316) of one rows x cols image or a batch n x rows x cols.  sparse: uint16
        (depth * 256) or float32 (metres; a negative or non-finite value is refused).  Returns (dense float32 or None, dense uint16 or None, stats dict), shaped as
        the input."""
        sparse = np.asarray(sparse)
        if sparse.dtype not in (np.uint16, np.float32) or sparse.ndim not in (2, 3):
            raise PvlmError("depth_completion: a uint16 or float32 image (rows x cols) or batch (n x rows x cols)")
        if not (want_f32 or want_u16):
            raise PvlmError("depth_completion: no output")
        sparse = np.ascontiguousarray(sparse)
        n = 1 if sparse.ndim == 2 else sparse.shape[0]
        rows, cols = sparse.shape[-2:]
        f32 = np.zeros(sparse.shape, np.float32) if want_f32 else None
        u16 = np.zeros(sparse.shape, np.uint16) if want_u16 else None
        st = DepthfillStats()
        is16 = sparse.dtype == np.uint16
        self._check(self.lib.pvlm_depth_completion(self._h, C.c_int(rows), C.c_int(cols), C.c_int(n), _p(sparse if is16 else None, C.c_uint16),
                                                   _p(None if is16 else sparse, C.c_float), C.c_float(max_depth), _p(f32, C.c_float), _p(u16, C.c_uint16),
                                                   C.byref(st)), "pvlm_depth_completion")
        return f32, u16, _depthfill_stats(st)

    def compute_depth_images(self, rows, cols, clouds, T_cl, size, max_depth):
        """pvlm_compute_depth_images (K37): the loop body of SfM::ComputeDepthImage (sfm/SfM.cpp:170-226) for every cloud (n x 3 float32, LiDAR frame) in one call:
        the splat of project_lidar_depth(rows, cols, cloud, T_cl, size), DepthCompletion, x 256, uint16.  Returns (n_scans x rows x cols uint16, stats dict)."""
        clouds = [_f32(c).reshape(-1, 3) for c in clouds]
        first = np.zeros(len(clouds) + 1, np.int64)
        first[1:] = np.cumsum([len(c) for c in clouds])
        xyz = np.ascontiguousarray(np.concatenate(clouds + [np.zeros((1, 3), np.float32)]))
        return self.compute_depth_images_flat(rows, cols, first, xyz, T_cl, size, max_depth)

    def compute_depth_images_flat(self, rows, cols, first_point, xyz, T_cl, size, max_depth):
        """compute_depth_images on the call's own arrays: scan s is the points first_point[s] .. first_point[s + 1] of xyz."""
        first = _i64(first_point); xyz = _f32(xyz).reshape(-1, 3); T = _f64(T_cl).reshape(16)
        n = max(len(first) - 1, 0)
        out = np.zeros((n, rows, cols), np.uint16)
        st = DepthfillStats()
        self._check(self.lib.pvlm_compute_depth_images(self._h, C.c_int(rows), C.c_int(cols), C.c_int(n), _p(first, C.c_longlong), _p(xyz, C.c_float), _p(T, C.c_double),
                                                       C.c_uint(size), C.c_float(max_depth), _p(out, C.c_uint16), C.byref(st)), "pvlm_compute_depth_images")
        return out, _depthfill_stats(st)

    def cam_lidar_votes_batch(self, rows, cols, lines_list, lidar_scans, T_cl_list):
        """One launch for many (image lines, LiDAR-local scan, T_cl) triples; returns the list of vote matrices."""
        n = len(lidar_scans)
        assert len(lines_list) == n and len(T_cl_list) == n
        ls = [_f32(l).reshape(-1, 4) for l in lines_list]
        off = _i64(np.concatenate([[0], np.cumsum([len(l) for l in ls])]))
        flat = _f32(np.concatenate(ls) if n and off[-1] else np.zeros((0, 4)))
        T = _f64(np.array([np.asarray(t, np.float64).reshape(16) for t in T_cl_list]).reshape(-1))
        hs = (C.c_void_p * max(n, 1))(*[s._h for s in lidar_scans])
        voff = np.zeros(n + 1, np.int64)
        args = (self._h, C.c_int(n), C.c_int(rows), C.c_int(cols), _p(off, C.c_int64), _p(flat, C.c_float), hs, _p(T, C.c_double), _p(voff, C.c_int64))
        self._check(self.lib.pvlm_cam_lidar_votes_batch(*args, None, C.c_int64(0)), "pvlm_cam_lidar_votes_batch")
        votes = np.zeros(max(int(voff[-1]), 1), np.int32)
        self._check(self.lib.pvlm_cam_lidar_votes_batch(*args, _p(votes, C.c_int32), C.c_int64(len(votes))), "pvlm_cam_lidar_votes_batch")
        return [votes[voff[p]:voff[p + 1]].reshape(len(ls[p]), lidar_scans[p].n_segments) for p in range(n)]

    def cam_lidar_votes_batch_sparse(self, rows, cols, lines_list, lidar_scans, T_cl_list):
        """The same launch, the votes returned sparse: (vote_offsets [n + 1], nz_index, nz_count) — the non-zero counters of the dense
        layout in ascending position (pvlm_cam_lidar_votes_batch_sparse)."""
        n = len(lidar_scans)
        assert len(lines_list) == n and len(T_cl_list) == n
        ls = [_f32(l).reshape(-1, 4) for l in lines_list]
        off = _i64(np.concatenate([[0], np.cumsum([len(l) for l in ls])]))
        flat = _f32(np.concatenate(ls) if n and off[-1] else np.zeros((0, 4)))
        T = _f64(np.array([np.asarray(t, np.float64).reshape(16) for t in T_cl_list]).reshape(-1))
        hs = (C.c_void_p * max(n, 1))(*[s._h for s in lidar_scans])
        voff = np.zeros(n + 1, np.int64)
        nnz = C.c_int64(0)
        cap = max(1, int(sum(len(l) for l in ls)) * 4)          # a line rarely collects votes for more than a few segments
        import time as _time
        while True:
            idx = np.empty(cap, np.int64); cnt = np.empty(cap, np.int32)
            t0 = _time.perf_counter()
            rc = self.lib.pvlm_cam_lidar_votes_batch_sparse(self._h, C.c_int(n), C.c_int(rows), C.c_int(cols), _p(off, C.c_int64), _p(flat, C.c_float), hs,
                                                             _p(T, C.c_double), _p(voff, C.c_int64), _p(idx, C.c_int64), _p(cnt, C.c_int32), C.c_int64(cap), C.byref(nnz))
            self.last_call_s = _time.perf_counter() - t0      # the C ABI call alone (the lists above are this wrapper's)
            if rc == ERR_CAPACITY and nnz.value > cap:
                cap = int(nnz.value)
                continue
            self._check(rc, "pvlm_cam_lidar_votes_batch_sparse")
            return voff, idx[:nnz.value], cnt[:nnz.value]

    # --- association -------------------------------------------------------------------------------
    def knn(self, scan, queries, k, max_dist, which=0):
        q = _f32(queries).reshape(-1, 3)
        idx = np.empty((q.shape[0], k), np.int32); sqd = np.empty((q.shape[0], k), np.float32)
        self._check(self.lib.pvlm_knn(self._h, scan._h, C.c_int(which), _p(q, C.c_float), C.c_int(q.shape[0]), C.c_int(k),
                                      C.c_float(max_dist), _p(idx, C.c_int32), _p(sqd, C.c_float)), "pvlm_knn")
        return idx, sqd

    def assoc_point2plane(self, refs, neis, plane_tolerance, dist_threshold, kind=POINT2PLANE_ANGLE,
                          flags=FLAG_NORMALIZE_DISTANCE, weight=1.0):
        n = len(refs)
        assert n == len(neis)
        ra = (C.c_void_p * max(n, 1))(*[s._h for s in refs])
        na = (C.c_void_p * max(n, 1))(*[s._h for s in neis])
        h = C.c_void_p()
        self._check(self.lib.pvlm_assoc_point2plane(self._h, C.c_int(n), ra, na, C.c_double(plane_tolerance), C.c_float(dist_threshold),
                                                    C.c_int(kind), C.c_uint(flags), C.c_double(weight), C.byref(h)), "pvlm_assoc_point2plane")
        return ResidualSet(self, h)

    def line2line_votes(self, ref, nei, dist_threshold):
        votes = np.zeros((max(1, nei.n_segments), max(1, ref.n_segments)), np.int32)
        self._check(self.lib.pvlm_line2line_votes(self._h, ref._h, nei._h, C.c_float(dist_threshold), _p(votes, C.c_int32)), "pvlm_line2line_votes")
        return votes[:nei.n_segments, :ref.n_segments]


    def line2line_votes_batch(self, refs, neis, dist_threshold):
        """One launch for many (ref, nei) pairs; returns the list of n_nei_seg x n_ref_seg vote matrices."""
        n = len(refs)
        assert len(neis) == n
        hr = (C.c_void_p * max(n, 1))(*[s._h for s in refs]); hn = (C.c_void_p * max(n, 1))(*[s._h for s in neis])
        voff = np.zeros(n + 1, np.int64)
        self._check(self.lib.pvlm_line2line_votes_batch(self._h, C.c_int(n), hr, hn, C.c_float(dist_threshold), _p(voff, C.c_int64), None, C.c_int64(0)),
                    "pvlm_line2line_votes_batch")
        votes = np.zeros(max(int(voff[-1]), 1), np.int32)
        self._check(self.lib.pvlm_line2line_votes_batch(self._h, C.c_int(n), hr, hn, C.c_float(dist_threshold), _p(voff, C.c_int64), _p(votes, C.c_int32),
                                                        C.c_int64(len(votes))), "pvlm_line2line_votes_batch")
        return [votes[voff[p]:voff[p + 1]].reshape(neis[p].n_segments, refs[p].n_segments) for p in range(n)]


    def line2line_best_batch(self, refs, neis, dist_threshold):
        """pvlm_line2line_best_batch: per pair and neighbour segment (a row of the vote block) the reference segment with the most votes — the first of equals — and
        that count.  Returns (row_offsets, best_col, best_count); a pair without reference segments has no rows."""
        n = len(refs)
        assert len(neis) == n
        hr = (C.c_void_p * max(n, 1))(*[s._h for s in refs]); hn = (C.c_void_p * max(n, 1))(*[s._h for s in neis])
        roff = np.zeros(n + 1, np.int64)
        self._check(self.lib.pvlm_line2line_best_batch(self._h, C.c_int(n), hr, hn, C.c_float(dist_threshold), _p(roff, C.c_int64), None, None, C.c_int64(0)), "pvlm_line2line_best_batch")
        col = np.zeros(max(int(roff[-1]), 1), np.int32); cnt = np.zeros_like(col)
        self._check(self.lib.pvlm_line2line_best_batch(self._h, C.c_int(n), hr, hn, C.c_float(dist_threshold), _p(roff, C.c_int64), _p(col, C.c_int32), _p(cnt, C.c_int32),
                                                       C.c_int64(len(col))), "pvlm_line2line_best_batch")
        return roff, col[:int(roff[-1])], cnt[:int(roff[-1])]


class MvsViews:
    """Resident set of equally sized MVS views (pvlm_mvs_views_*): maps stay on the GPU between the scoring pass, the
    PatchMatch sweeps and the fusion filter."""

    def __init__(self, ctx, rows, cols, n_views):
        self.ctx, self.rows, self.cols, self.n = ctx, rows, cols, n_views
        self._h = C.c_void_p()
        ctx._check(ctx.lib.pvlm_mvs_views_create(ctx._h, C.c_int(rows), C.c_int(cols), C.c_int(n_views), C.byref(self._h)), "pvlm_mvs_views_create")

    def close(self):
        if self._h:
            self.ctx.lib.pvlm_mvs_views_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, view, gray=None, depth=None, normal=None, conf=None):
        g = None if gray is None else np.ascontiguousarray(gray, np.uint8)
        d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        n = None if normal is None else np.ascontiguousarray(normal, np.float32)
        c = None if conf is None else np.ascontiguousarray(conf, np.float32)
        for a, shape in ((g, (self.rows, self.cols)), (d, (self.rows, self.cols)), (n, (self.rows, self.cols, 3)), (c, (self.rows, self.cols))):
            assert a is None or a.shape == shape
        self.ctx._check(self.ctx.lib.pvlm_mvs_views_upload(self.ctx._h, self._h, C.c_int(view), _p(g, C.c_ubyte), _p(d, C.c_float), _p(n, C.c_float),
                                                           _p(c, C.c_float)), "pvlm_mvs_views_upload")

    def download(self, view, what=("depth", "normal", "conf", "depth_filter", "conf_filter")):
        out = {k: np.zeros((self.rows, self.cols, 3) if k == "normal" else (self.rows, self.cols), np.float32) for k in what}
        ptr = lambda k: _p(out[k], C.c_float) if k in out else None
        self.ctx._check(self.ctx.lib.pvlm_mvs_views_download(self.ctx._h, self._h, C.c_int(view), ptr("depth"), ptr("normal"), ptr("conf"), ptr("depth_filter"),
                                                             ptr("conf_filter")), "pvlm_mvs_views_download")
        return out

    def snapshot_depth(self, view):
        self.ctx._check(self.ctx.lib.pvlm_mvs_views_snapshot_depth(self.ctx._h, self._h, C.c_int(view)), "pvlm_mvs_views_snapshot_depth")

    def _nb(self, nei, R_nr, t_nr):
        ids = _i32(np.asarray(nei, np.int32).reshape(-1))
        return ids, _f32(R_nr).reshape(-1), _f32(t_nr).reshape(-1)

    def estimate(self, ref, nei, R_nr, t_nr, half_window=3, step=1, use_geometry=False, depth_constant=None, min_depth=0.1, max_depth=20.0, seed=1, max_iter=-1,
                 conf_threshold=-1.0, sequential=False):
        """max_iter < 0: InitConfMap; otherwise EstimateDepthMapSingle with max_iter iterations (checkerboard, or the sequential sweep)."""
        ids, R, t = self._nb(nei, R_nr, t_nr)
        dc = None if depth_constant is None else np.ascontiguousarray(depth_constant, np.uint8)
        fn = self.ctx.lib.pvlm_mvs_views_estimate_sequential if (sequential and max_iter >= 0) else self.ctx.lib.pvlm_mvs_views_estimate
        self.ctx._check(fn(self.ctx._h, self._h, C.c_int(ref), C.c_int(len(ids)), _p(ids, C.c_int), _p(R, C.c_float), _p(t, C.c_float),
                                                             C.c_int(half_window), C.c_int(step), C.c_int(1 if use_geometry else 0), _p(dc, C.c_ubyte),
                                                             C.c_float(min_depth), C.c_float(max_depth), C.c_ulonglong(seed), C.c_int(max_iter),
                                                             C.c_float(conf_threshold)), "pvlm_mvs_views_estimate")

    def estimate_sequential_batch(self, jobs, half_window=3, step=1, use_geometry=False, min_depth=0.1, max_depth=20.0, max_iter=1, conf_threshold=-1.0):
        """jobs: list of dicts (ref, nei, R_nr, t_nr, seed[, depth_constant]) with distinct refs: the sequential sweep of all of them, one
        launch per anti-diagonal for the whole batch (pvlm_mvs_views_estimate_sequential_batch)."""
        n = len(jobs)
        refs = _i32([j["ref"] for j in jobs]); cnt = _i32([len(j["nei"]) for j in jobs])
        ids = _i32([b for j in jobs for b in j["nei"]]) if int(cnt.sum()) else np.zeros(1, np.int32)
        R = _f32(np.concatenate([np.asarray(j["R_nr"], np.float32).reshape(-1) for j in jobs])) if int(cnt.sum()) else np.zeros(9, np.float32)
        t = _f32(np.concatenate([np.asarray(j["t_nr"], np.float32).reshape(-1) for j in jobs])) if int(cnt.sum()) else np.zeros(3, np.float32)
        seeds = np.ascontiguousarray([int(j.get("seed", 1)) for j in jobs], np.uint64)
        dcs = [None if j.get("depth_constant") is None else np.ascontiguousarray(j["depth_constant"], np.uint8) for j in jobs]
        dptr = None
        if any(d is not None for d in dcs):
            dptr = (C.POINTER(C.c_ubyte) * max(n, 1))(*[None if d is None else d.ctypes.data_as(C.POINTER(C.c_ubyte)) for d in dcs])
        self.ctx._check(self.ctx.lib.pvlm_mvs_views_estimate_sequential_batch(
            self.ctx._h, self._h, C.c_int(n), _p(refs, C.c_int), _p(cnt, C.c_int), _p(ids, C.c_int), _p(R, C.c_float), _p(t, C.c_float), C.c_int(half_window), C.c_int(step),
            C.c_int(1 if use_geometry else 0), dptr, C.c_float(min_depth), C.c_float(max_depth), seeds.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.c_int(max_iter),
            C.c_float(conf_threshold)), "pvlm_mvs_views_estimate_sequential_batch")

    def depth_to_cloud(self, view, bgr, T_wc, max_depth=20.0, filter_sky=True, use_filtered_depth=True, with_normal=False):
        """MVS::DepthImageToCloud / DepthNormalToCloud of a resident view (its depth_filter or depth map, its normal map)."""
        c = np.ascontiguousarray(bgr, np.uint8); assert c.shape == (self.rows, self.cols, 3)
        T = np.ascontiguousarray(np.asarray(T_wc, np.float64).reshape(-1)[:12])
        npix = self.rows * self.cols
        xyz = np.empty((npix, 3), np.float32); rgb = np.empty((npix, 3), np.uint8)
        nout = np.empty((npix, 3), np.float32) if with_normal else None
        n = C.c_longlong(0)
        self.ctx._check(self.ctx.lib.pvlm_mvs_views_depth_to_cloud(self.ctx._h, self._h, C.c_int(view), C.c_int(1 if use_filtered_depth else 0), _p(c, C.c_ubyte),
                                                                   _p(T, C.c_double), C.c_float(max_depth), C.c_int(1 if filter_sky else 0), _p(xyz, C.c_float),
                                                                   _p(rgb, C.c_ubyte), _p(nout, C.c_float), C.byref(n)), "pvlm_mvs_views_depth_to_cloud")
        k = n.value
        return (xyz[:k].copy(), rgb[:k].copy()) if nout is None else (xyz[:k].copy(), rgb[:k].copy(), nout[:k].copy())

    def filter_refine(self, ref, nei, R_nr, t_nr, depth_constant=None, thr=0.01, min_depth=0.1, max_depth=20.0):
        ids, R, t = self._nb(nei, R_nr, t_nr)
        dc = None if depth_constant is None else np.ascontiguousarray(depth_constant, np.uint8)
        self.ctx._check(self.ctx.lib.pvlm_mvs_views_filter_refine(self.ctx._h, self._h, C.c_int(ref), C.c_int(len(ids)), _p(ids, C.c_int), _p(R, C.c_float),
                                                                  _p(t, C.c_float), _p(dc, C.c_ubyte), C.c_float(thr), C.c_float(min_depth),
                                                                  C.c_float(max_depth)), "pvlm_mvs_views_filter_refine")


class ResidualSet:
    def __init__(self, ctx, handle):
        self.ctx = ctx
        self._h = handle
        n = C.c_int64(); p = C.c_int(); k = C.c_int(); f = C.c_uint()
        ctx._check(ctx.lib.pvlm_resset_info(self._h, C.byref(n), C.byref(p), C.byref(k), C.byref(f)), "pvlm_resset_info")
        self.n, self.n_pairs, self.kind, self.flags = n.value, p.value, k.value, f.value

    @classmethod
    def upload(cls, ctx, kind, rows, pair_offsets, pair_ref, pair_nei, flags=0, weight=1.0):
        stride = STRIDE.get(kind, np.shape(rows)[-1] if np.ndim(rows) == 2 else 1)   # unknown kinds are rejected by the library
        rows = _f64(rows).reshape(-1, stride) if np.size(rows) else np.zeros((0, stride))
        po = _i64(pair_offsets); pr = _i32(pair_ref); pn = _i32(pair_nei)
        h = C.c_void_p()
        ctx._check(ctx.lib.pvlm_resset_upload(ctx._h, C.c_int(kind), C.c_uint(flags), C.c_double(weight), C.c_int64(rows.shape[0]),
                                              C.c_int(len(pr)), _p(po, C.c_int64), _p(pr, C.c_int), _p(pn, C.c_int),
                                              _p(rows, C.c_double), C.c_int(stride), C.byref(h)), "pvlm_resset_upload")
        return cls(ctx, h)

    def close(self):
        if self._h:
            self.ctx.lib.pvlm_resset_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def download(self):
        po = np.empty(self.n_pairs + 1, np.int64); pr = np.empty(max(self.n_pairs, 1), np.int32); pn = np.empty(max(self.n_pairs, 1), np.int32)
        rows = np.empty((max(self.n, 1), STRIDE[self.kind]), np.float64)
        self.ctx._check(self.ctx.lib.pvlm_resset_download(self.ctx._h, self._h, _p(po, C.c_int64), _p(pr, C.c_int), _p(pn, C.c_int),
                                                          _p(rows, C.c_double)), "pvlm_resset_download")
        return po, pr[:self.n_pairs], pn[:self.n_pairs], rows[:self.n]

    def plane_runs(self):
        """Point-to-plane sets: whether the fused evaluation reads the plane-run table, and the runs of equal consecutive planes counted at finalize."""
        u, r = C.c_int(0), C.c_int64(0)
        self.ctx._check(self.ctx.lib.pvlm_resset_plane_runs(self._h, C.byref(u), C.byref(r)), "pvlm_resset_plane_runs")
        return dict(in_use=bool(u.value), runs=int(r.value))

    def point_table(self):
        """Sets of the association: whether the fused evaluation reads the point from the per-neighbour table, the tables, and the fused kernel's grid."""
        u, t, g = C.c_int(0), C.c_int(0), C.c_int(0)
        self.ctx._check(self.ctx.lib.pvlm_resset_point_table(self._h, C.byref(u), C.byref(t), C.byref(g)), "pvlm_resset_point_table")
        return dict(in_use=bool(u.value), tables=int(t.value), positions=int(g.value))

    def point_table_debug(self):
        """Per residual block (compact order): the stored 16-bit query number and the table entry (3 doubles) it names."""
        q = np.empty(max(self.n, 1), np.uint16); pts = np.empty((max(self.n, 1), 3), np.float64)
        self.ctx._check(self.ctx.lib.pvlm_resset_point_table_debug(self.ctx._h, self._h, _p(q, C.c_uint16), _p(pts, C.c_double)),
                        "pvlm_resset_point_table_debug")
        return q[:self.n], pts[:self.n]

    def set_pose_ids(self, pair_ref, pair_nei):
        """Renumbers the segments' poses (one pose table for every set of a problem)."""
        pr = _i32(pair_ref); pn = _i32(pair_nei)
        assert len(pr) == self.n_pairs and len(pn) == self.n_pairs
        self.ctx._check(self.ctx.lib.pvlm_resset_set_pose_ids(self.ctx._h, self._h, _p(pr, C.c_int), _p(pn, C.c_int)), "pvlm_resset_set_pose_ids")

    def eval(self, jac=True):
        r = np.empty(max(self.n, 1), np.float64)
        J = np.empty((max(self.n, 1), 12), np.float64) if jac else None
        self.ctx._check(self.ctx.lib.pvlm_eval(self.ctx._h, self._h, _p(r, C.c_double), _p(J, C.c_double)), "pvlm_eval")
        return r[:self.n], (J[:self.n] if jac else None)

    def eval_dev(self, d_r_ptr, d_J_ptr):
        self.ctx._check(self.ctx.lib.pvlm_eval_dev(self.ctx._h, self._h, C.c_void_p(d_r_ptr), C.c_void_p(d_J_ptr or 0)), "pvlm_eval_dev")

    def pair_blocks(self, loss=LOSS_NONE, loss_a=0.0):
        out = np.empty((max(self.n_pairs, 1), PAIR_BLOCK), np.float64)
        self.ctx._check(self.ctx.lib.pvlm_eval_pair_blocks(self.ctx._h, self._h, C.c_int(loss), C.c_double(loss_a), _p(out, C.c_double)),
                        "pvlm_eval_pair_blocks")
        return out[:self.n_pairs]

    def pair_blocks_dev(self, d_out_ptr, loss=LOSS_NONE, loss_a=0.0):
        self.ctx._check(self.ctx.lib.pvlm_eval_pair_blocks_dev(self.ctx._h, self._h, C.c_int(loss), C.c_double(loss_a), C.c_void_p(d_out_ptr)),
                        "pvlm_eval_pair_blocks_dev")

    def eval_host_async(self, r_host, J_host=None):
        """pvlm_eval_host_async into (preferably pinned) host arrays; complete after ctx.synchronize()."""
        self.ctx._check(self.ctx.lib.pvlm_eval_host_async(self.ctx._h, self._h, C.c_void_p(r_host.ctypes.data),
                                                          C.c_void_p(J_host.ctypes.data if J_host is not None else 0)), "pvlm_eval_host_async")

    def eval_wrench_host_async(self, w_host, tab_host):
        self.ctx._check(self.ctx.lib.pvlm_eval_wrench_host_async(self.ctx._h, self._h, C.c_void_p(w_host.ctypes.data), C.c_void_p(tab_host.ctypes.data)),
                        "pvlm_eval_wrench_host_async")

    def eval_force_host_async(self, f_host, tab_host):
        """[r | g(3)] rows (32 B per block, point functors) + pair tables into page-locked arrays (Context.host_alloc); complete after synchronize()."""
        self.ctx._check(self.ctx.lib.pvlm_eval_force_host_async(self.ctx._h, self._h, _p(f_host, C.c_double), _p(tab_host, C.c_double)), "pvlm_eval_force_host_async")

    def assoc_exact_fits(self):
        """Queries of the association whose plane came from the exact QR because the certified fast fit refused."""
        n = C.c_int64(0)
        self.ctx._check(self.ctx.lib.pvlm_assoc_point2plane_stats(self._h, C.byref(n)), "pvlm_assoc_point2plane_stats")
        return int(n.value)

    def assoc_stats(self):
        n, b, e = C.c_int64(0), C.c_int(0), C.c_int(0)
        self.ctx._check(self.ctx.lib.pvlm_assoc_point2plane_stats2(self._h, C.byref(n), C.byref(b), C.byref(e)), "pvlm_assoc_point2plane_stats2")
        return dict(exact_fits=int(n.value), batches=b.value, exact_kernel_batches=e.value)

    def assoc_debug(self):
        q = np.empty(max(self.n, 1), np.int32); nn = np.empty((max(self.n, 1), 10), np.int32)
        self.ctx._check(self.ctx.lib.pvlm_assoc_point2plane_debug(self.ctx._h, self._h, _p(q, C.c_int32), _p(nn, C.c_int32)),
                        "pvlm_assoc_point2plane_debug")
        return q[:self.n], nn[:self.n]


class NormalEq:
    def __init__(self, ctx, n_poses, upair_i, upair_j):
        self.ctx = ctx
        ui = _i32(upair_i); uj = _i32(upair_j)
        self._h = C.c_void_p()
        ctx._check(ctx.lib.pvlm_neq_create(ctx._h, C.c_int(n_poses), C.c_int(len(ui)), _p(ui, C.c_int), _p(uj, C.c_int), C.byref(self._h)),
                   "pvlm_neq_create")
        self.n_poses, self.n_upairs = n_poses, len(ui)
        self.size = int(ctx.lib.pvlm_neq_size(self._h))

    def close(self):
        if self._h:
            self.ctx.lib.pvlm_neq_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate(self, rs, loss=LOSS_NONE, loss_a=0.0, packed=None):
        zero_first = packed is None
        buf = np.zeros(self.size, np.float64) if packed is None else _f64(packed)
        self.ctx._check(self.ctx.lib.pvlm_neq_accumulate(self.ctx._h, self._h, rs._h, C.c_int(loss), C.c_double(loss_a),
                                                         C.c_int(1 if zero_first else 0), _p(buf, C.c_double)), "pvlm_neq_accumulate")
        return buf

    def accumulate_dev(self, rs, d_packed_ptr, loss=LOSS_NONE, loss_a=0.0, zero_first=True):
        self.ctx._check(self.ctx.lib.pvlm_neq_accumulate_dev(self.ctx._h, self._h, rs._h, C.c_int(loss), C.c_double(loss_a),
                                                             C.c_int(1 if zero_first else 0), C.c_void_p(d_packed_ptr)), "pvlm_neq_accumulate_dev")

    def accumulate_async(self, rs, packed, loss=LOSS_NONE, loss_a=0.0):
        """Queues the linearisation of `rs` into this structure's own device buffer and its copy into `packed` (float64 array of
        `size` elements that must stay alive); complete after ctx.synchronize().  One call per residual set of a problem, one
        synchronisation for all of them."""
        assert packed.dtype == np.float64 and packed.flags["C_CONTIGUOUS"] and packed.size == self.size
        self.ctx._check(self.ctx.lib.pvlm_neq_accumulate_async(self.ctx._h, self._h, rs._h, C.c_int(loss), C.c_double(loss_a),
                                                               packed.ctypes.data_as(C.POINTER(C.c_double))), "pvlm_neq_accumulate_async")

    @staticmethod
    def accumulate_sets(ctx, neqs, sets, losses, loss_as, packed):
        """All sets linearised and summed on the device into neqs[0]'s buffer (identical structures), one queued copy into `packed`;
        complete after ctx.synchronize()."""
        n = len(neqs)
        assert packed.dtype == np.float64 and packed.flags["C_CONTIGUOUS"] and packed.size == neqs[0].size
        qa = (C.c_void_p * n)(*[q._h for q in neqs]); ra = (C.c_void_p * n)(*[r._h for r in sets])
        la = (C.c_int * n)(*[int(l) for l in losses]); aa = (C.c_double * n)(*[float(a) for a in loss_as])
        ctx._check(ctx.lib.pvlm_neq_accumulate_sets(ctx._h, C.c_int(n), qa, ra, la, aa, packed.ctypes.data_as(C.POINTER(C.c_double))), "pvlm_neq_accumulate_sets")

    def unpack(self, packed):
        n, u = self.n_poses, self.n_upairs
        Hd = packed[:n * 36].reshape(n, 6, 6); Ho = packed[n * 36:(n + u) * 36].reshape(u, 6, 6)
        g = packed[(n + u) * 36:(n + u) * 36 + n * 6].reshape(n, 6)
        return Hd, Ho, g, float(packed[-1])


class BundleSet:
    """Reprojection blocks with the 3-D points resident on the GPU and eliminated there (pvlm_ba_* of include/pvlm.h).
    Camera poses come from Context.set_poses (angleAxis_cw, t_cw).  kind = "angle1" (PanoramaReprojResidual_1Angle: bearings
    n x 3), "angle2" (_2Angle: n x 2 sphere angles) or "pixel" (_Pixel: n x 2 keypoint pixels, rows / cols = image size);
    the two-row kinds give 2 residual rows per observation (pvlm_ba_create_kind, K31)."""

    def __init__(self, ctx, point_offsets, cam_ids, bearings, points, weight=1.0, kind="angle1", rows=0, cols=0):
        self.ctx = ctx
        if kind not in BA_KINDS:
            raise ValueError("kind must be one of %s" % sorted(BA_KINDS))
        self.kind = kind
        self.rows_per_obs = 1 if kind == "angle1" else 2
        off = _i64(point_offsets); cam = _i32(cam_ids); b = _f64(bearings); X = _f64(points)
        if len(cam) and b.reshape(len(cam), -1).shape[1] != (3 if kind == "angle1" else 2):
            raise ValueError("observations must be n x %d for kind %r" % (3 if kind == "angle1" else 2, kind))
        self._h = C.c_void_p()
        if kind == "angle1":
            ctx._check(ctx.lib.pvlm_ba_create(ctx._h, C.c_int(len(off) - 1), C.c_int64(len(cam)), _p(off, C.c_int64), _p(cam, C.c_int),
                                              _p(b, C.c_double), _p(X, C.c_double), C.c_double(weight), C.byref(self._h)), "pvlm_ba_create")
        else:
            ctx._check(ctx.lib.pvlm_ba_create_kind(ctx._h, C.c_int(BA_KINDS[kind]), C.c_int(rows), C.c_int(cols), C.c_int(len(off) - 1), C.c_int64(len(cam)),
                                                   _p(off, C.c_int64), _p(cam, C.c_int), _p(b, C.c_double), _p(X, C.c_double), C.c_double(weight),
                                                   C.byref(self._h)), "pvlm_ba_create_kind")
        npts = C.c_int(); nobs = C.c_int64(); ncam = C.c_int(); nup = C.c_int()
        ctx.lib.pvlm_ba_structure(self._h, C.byref(npts), C.byref(nobs), C.byref(ncam), C.byref(nup), None, None)
        self.n_points, self.n_obs, self.n_cams, self.n_upairs = npts.value, nobs.value, ncam.value, nup.value
        self.ui = np.zeros(self.n_upairs, np.int32); self.uj = np.zeros(self.n_upairs, np.int32)
        ctx.lib.pvlm_ba_structure(self._h, None, None, None, None, _p(self.ui, C.c_int), _p(self.uj, C.c_int))
        self.size = int(ctx.lib.pvlm_ba_packed_size(self._h))

    def close(self):
        if self._h:
            self.ctx.lib.pvlm_ba_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def points(self, candidate=False):
        X = np.zeros((self.n_points, 3), np.float64)
        self.ctx._check(self.ctx.lib.pvlm_ba_get_points(self.ctx._h, self._h, C.c_int(1 if candidate else 0), _p(X, C.c_double)), "pvlm_ba_get_points")
        return X

    def set_points(self, X):
        X = _f64(X)
        assert X.shape == (self.n_points, 3)
        self.ctx._check(self.ctx.lib.pvlm_ba_set_points(self.ctx._h, self._h, _p(X, C.c_double)), "pvlm_ba_set_points")

    def set_constant(self, mask):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        assert m is None or m.shape == (self.n_points,)
        self.ctx._check(self.ctx.lib.pvlm_ba_set_constant(self.ctx._h, self._h, _p(m, C.c_ubyte)), "pvlm_ba_set_constant")

    def evaluate(self, jac=True):
        """r: n_obs x rows_per_obs residual rows (flat), J: (n_obs x rows_per_obs) x 9 rows [aa_cw | t_cw | X]."""
        r = np.zeros(self.n_obs * self.rows_per_obs, np.float64)
        J = np.zeros((self.n_obs * self.rows_per_obs, 9), np.float64) if jac else None
        self.ctx._check(self.ctx.lib.pvlm_ba_eval(self.ctx._h, self._h, _p(r, C.c_double), _p(J, C.c_double)), "pvlm_ba_eval")
        return r, J

    def reduce(self, loss=LOSS_NONE, loss_a=0.0, init_scale=False, radius=1e4, min_diag=1e-6, max_diag=1e32):
        packed = np.zeros(self.size, np.float64)
        self.ctx._check(self.ctx.lib.pvlm_ba_reduce(self.ctx._h, self._h, C.c_int(loss), C.c_double(loss_a), C.c_int(1 if init_scale else 0),
                                                    C.c_double(radius), C.c_double(min_diag), C.c_double(max_diag), _p(packed, C.c_double)), "pvlm_ba_reduce")
        return packed

    def step(self, dcam, loss=LOSS_NONE, loss_a=0.0):
        d = _f64(dcam)
        assert d.shape == (self.n_cams, 6)
        out3 = np.zeros(3, np.float64)
        self.ctx._check(self.ctx.lib.pvlm_ba_step(self.ctx._h, self._h, C.c_int(loss), C.c_double(loss_a), _p(d, C.c_double), _p(out3, C.c_double)), "pvlm_ba_step")
        return out3

    def cost(self, loss=LOSS_NONE, loss_a=0.0, candidate=False):
        c = C.c_double()
        self.ctx._check(self.ctx.lib.pvlm_ba_cost(self.ctx._h, self._h, C.c_int(loss), C.c_double(loss_a), C.c_int(1 if candidate else 0), C.byref(c)), "pvlm_ba_cost")
        return c.value

    def accept(self):
        self.ctx._check(self.ctx.lib.pvlm_ba_accept(self.ctx._h, self._h), "pvlm_ba_accept")


class Comm:
    """RCCL communicator of the C ABI (for hosts without their own collective layer)."""

    def __init__(self, ctx, world_size, rank, unique_id=None):
        self.ctx = ctx
        if unique_id is None:
            buf = (C.c_ubyte * 128)()
            ctx._check(ctx.lib.pvlm_comm_unique_id(ctx._h, buf), "pvlm_comm_unique_id")
            unique_id = bytes(buf)
        self.unique_id = unique_id
        self._h = C.c_void_p()
        ctx._check(ctx.lib.pvlm_comm_create(ctx._h, C.c_int(world_size), C.c_int(rank), (C.c_ubyte * 128).from_buffer_copy(unique_id),
                                            C.byref(self._h)), "pvlm_comm_create")

    def allreduce_sum_f64(self, d_ptr, count):
        self.ctx._check(self.ctx.lib.pvlm_allreduce_sum_f64(self.ctx._h, self._h, C.c_void_p(d_ptr), C.c_int64(count)), "pvlm_allreduce_sum_f64")

    def close(self):
        if self._h:
            self.ctx.lib.pvlm_comm_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()


class ScanDesc(C.Structure):
    _fields_ = [
        ("id", C.c_int), ("R_wl", C.POINTER(C.c_double)), ("t_wl", C.POINTER(C.c_double)),
        ("n_surf_flat", C.c_int), ("surf_flat_xyz", C.POINTER(C.c_float)), ("surf_flat_tag", C.POINTER(C.c_float)),
        ("n_surf_less_flat", C.c_int), ("surf_less_flat_xyz", C.POINTER(C.c_float)), ("surf_less_flat_tag", C.POINTER(C.c_float)),
        ("n_corner", C.c_int), ("corner_xyz", C.POINTER(C.c_float)),
        ("p2s_offsets", C.POINTER(C.c_int)), ("p2s_ids", C.POINTER(C.c_int)),
        ("n_segments", C.c_int), ("segment_size", C.POINTER(C.c_int)),
        ("segment_coeffs", C.POINTER(C.c_double)), ("end_points", C.POINTER(C.c_double)),
        ("seg_points_xyz", C.POINTER(C.c_float)), ("point_stride_floats", C.c_int),
    ]


class Scan:
    """Device-resident feature clouds of one LiDAR scan (the sensors/Velodyne.h:80-91 contract).
    `scan` is a dict: id, R_wl, t_wl, flat_xyz, flat_tag, less_xyz, less_tag, corner_xyz, p2s,
    seg_size, seg_coeffs, end_points (all optional except the pose)."""

    @staticmethod
    def _describe(scan):
        """ScanDesc of a scan dict + the arrays it points into (to be kept alive across the call)."""
        g = scan.get
        R = _f64(g("R_wl", np.eye(3))).reshape(9); t = _f64(g("t_wl", np.zeros(3)))
        flat = _f32(g("flat_xyz", np.zeros((0, 3)))); flat_tag = _f32(g("flat_tag", np.ones(len(flat))))
        less = _f32(g("less_xyz", np.zeros((0, 3)))); less_tag = _f32(g("less_tag", np.ones(len(less))))
        corner = _f32(g("corner_xyz", np.zeros((0, 3))))
        p2s = g("p2s", None)
        if p2s is None:
            p2s = [[] for _ in range(len(corner))]
        off = np.zeros(len(p2s) + 1, np.int32)
        for i, l in enumerate(p2s):
            off[i + 1] = off[i] + len(l)
        ids = _i32([v for l in p2s for v in l]) if off[-1] > 0 else np.zeros(1, np.int32)
        seg_size = _i32(g("seg_size", np.zeros(0)))
        seg_coeffs = _f64(g("seg_coeffs", np.zeros((len(seg_size), 6))))
        end_points = _f64(g("end_points", np.zeros((len(seg_size), 6))))
        d = ScanDesc()
        d.id = int(g("id", 0)); d.R_wl = _p(R, C.c_double); d.t_wl = _p(t, C.c_double)
        d.n_surf_flat = len(flat); d.surf_flat_xyz = _p(flat, C.c_float); d.surf_flat_tag = _p(flat_tag, C.c_float)
        d.n_surf_less_flat = len(less); d.surf_less_flat_xyz = _p(less, C.c_float); d.surf_less_flat_tag = _p(less_tag, C.c_float)
        d.n_corner = len(corner); d.corner_xyz = _p(corner, C.c_float)
        d.p2s_offsets = _p(off, C.c_int); d.p2s_ids = _p(ids, C.c_int)
        d.n_segments = len(seg_size); d.segment_size = _p(seg_size, C.c_int)
        d.segment_coeffs = _p(seg_coeffs, C.c_double); d.end_points = _p(end_points, C.c_double)
        seg_xyz = g("seg_points_xyz", None)          # optional: the points of every segment, concatenated (world frame)
        seg_xyz = _f32(seg_xyz).reshape(-1, 3) if seg_xyz is not None else None
        if seg_xyz is not None:
            assert len(seg_xyz) == int(seg_size.sum())
        d.seg_points_xyz = _p(seg_xyz, C.c_float) if seg_xyz is not None and len(seg_xyz) else None
        keep = (R, t, flat, flat_tag, less, less_tag, corner, off, ids, seg_size, seg_coeffs, end_points, seg_xyz)
        if g("point_records", False):
            # the clouds handed over as pcl::PointXYZI-style records {x, y, z, intensity} (point_stride_floats = 4): xyz and tag point INTO one n x 4 array per cloud
            rec = [np.ascontiguousarray(np.concatenate([xyz, tag[:, None]], axis=1), np.float32) if len(xyz) else np.zeros((0, 4), np.float32)
                   for xyz, tag in ((flat, flat_tag), (less, less_tag), (corner, np.zeros(len(corner), np.float32)))]
            at = lambda a, k: C.cast(a.ctypes.data + 4 * k, C.POINTER(C.c_float)) if len(a) else None
            d.point_stride_floats = 4
            d.surf_flat_xyz, d.surf_flat_tag = at(rec[0], 0), at(rec[0], 3)
            d.surf_less_flat_xyz, d.surf_less_flat_tag = at(rec[1], 0), at(rec[1], 3)
            d.corner_xyz = at(rec[2], 0)
            keep = keep + tuple(rec)
        return d, keep

    def _adopt(self, ctx, d, handle):
        self.ctx = ctx
        self._h = handle
        self.id = d.id
        self.n_segments = d.n_segments
        self.n_flat, self.n_less, self.n_corner = d.n_surf_flat, d.n_surf_less_flat, d.n_corner

    def __init__(self, ctx, scan):
        d, keep = self._describe(scan)
        h = C.c_void_p()
        self._h = None
        ctx._check(ctx.lib.pvlm_scan_upload(ctx._h, C.byref(d), C.byref(h)), "pvlm_scan_upload")
        self._adopt(ctx, d, h)

    @classmethod
    def upload_batch(cls, ctx, scans):
        """pvlm_scan_upload_batch: every scan of `scans` (dicts) in one staging copy / one device slab / one grid build."""
        pairs = [cls._describe(s) for s in scans]
        n = len(pairs)
        descs = (ScanDesc * max(n, 1))()
        for k, (d, _) in enumerate(pairs):
            descs[k] = d
        handles = (C.c_void_p * max(n, 1))()
        ctx._check(ctx.lib.pvlm_scan_upload_batch(ctx._h, n, descs, handles), "pvlm_scan_upload_batch")
        out = []
        for k, (d, _) in enumerate(pairs):
            o = cls.__new__(cls)
            o._adopt(ctx, d, C.c_void_p(handles[k]))
            out.append(o)
        return out

    @staticmethod
    def transform_batch(ctx, scans, T, rebuild_grids=True):
        """pvlm_scan_transform_batch: scan k's resident float clouds are replaced by T[k] (3x4 or 4x4, [R | t]) applied as
        pcl::transformPointCloud applies an Eigen::Matrix4d; rebuild_grids: the voxel grids follow."""
        n = len(scans)
        T12 = np.ascontiguousarray(np.stack([np.asarray(t, np.float64)[:3, :4] for t in T]).reshape(n, 12)) if n else np.zeros((0, 12))
        handles = (C.c_void_p * max(n, 1))(*[s._h for s in scans])
        ctx._check(ctx.lib.pvlm_scan_transform_batch(ctx._h, n, handles, _p(T12, C.c_double), 1 if rebuild_grids else 0), "pvlm_scan_transform_batch")

    def set_pose(self, R_wl, t_wl):
        R = _f64(R_wl).reshape(9); t = _f64(t_wl).reshape(3)
        self.ctx._check(self.ctx.lib.pvlm_scan_set_pose(self.ctx._h, self._h, _p(R, C.c_double), _p(t, C.c_double)), "pvlm_scan_set_pose")

    def cloud_info(self, which):
        info = GridInfo()
        self.ctx._check(self.ctx.lib.pvlm_scan_cloud_info(self._h, int(which), C.byref(info)), "pvlm_scan_cloud_info")
        return info

    def fetch_cloud(self, which, grid=False):
        """The resident floats of cloud `which` (0 surfFlat, 1 surfLessFlat, 2 cornerLessSharp, 3 segment points) and, with grid=True, a
        CANONICAL form of its voxel grid: the plan and the cell-sorted records ordered by (cell — dense: cell index, hashed: 64-bit key —, original
        index): cell_key, index, points — independent of the slot / in-cell order the atomics of a build produce."""
        info = self.cloud_info(which)
        xyz = np.zeros((info.n, 3), np.float32)
        if not grid or not info.has_grid:
            self.ctx._check(self.ctx.lib.pvlm_scan_cloud_fetch(self.ctx._h, self._h, int(which), _p(xyz, C.c_float), None, None, None, None), "pvlm_scan_cloud_fetch")
            return xyz if not grid else (xyz, None)
        T = info.table_size
        count = np.zeros(T, np.int32); start = np.zeros(T, np.int32); keys = np.zeros(T, np.uint64); srt = np.zeros((info.n, 4), np.float32)
        self.ctx._check(self.ctx.lib.pvlm_scan_cloud_fetch(self.ctx._h, self._h, int(which), _p(xyz, C.c_float), _p(count, C.c_int), _p(start, C.c_int),
                                                           _p(keys, C.c_uint64) if not info.dense else None, _p(srt, C.c_float)), "pvlm_scan_cloud_fetch")
        plan = dict(n=info.n, dense=info.dense, nx=info.nx, ny=info.ny, nz=info.nz, xf=info.xf, table_size=T, cell=np.float32(info.cell).tobytes(),
                    origin=np.asarray(list(info.origin), np.float32).tobytes(), stale=info.stale)
        # per sorted position the key of its cell: the occupied slots in order of their start cover [0, n) without gaps
        slots = np.nonzero(count)[0]
        slots = slots[np.argsort(start[slots], kind="stable")]
        assert int(count[slots].sum()) == info.n and np.array_equal(start[slots], np.concatenate([[0], np.cumsum(count[slots])[:-1]]))
        cell_key = np.repeat(slots.astype(np.uint64) if info.dense else keys[slots], count[slots])
        idx = srt[:, 3].view(np.int32)
        order = np.lexsort((idx, cell_key))
        return xyz, dict(plan=plan, cell_key=cell_key[order], index=idx[order].copy(), points=srt[order, :3].copy())

    def close(self):
        if self._h:
            self.ctx.lib.pvlm_scan_destroy(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GridInfo(C.Structure):
    _fields_ = [("n", C.c_int), ("has_grid", C.c_int), ("stale", C.c_int), ("dense", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("xf", C.c_int), ("table_size", C.c_int), ("cell", C.c_float), ("origin", C.c_float * 3)]


class UndistortScanDesc(C.Structure):
    _fields_ = [("xyzi", C.POINTER(C.c_float)), ("n", C.c_int), ("stride_floats", C.c_int), ("R_wl", C.POINTER(C.c_double)), ("t_wl", C.POINTER(C.c_double)),
                ("R_we", C.POINTER(C.c_double)), ("t_we", C.POINTER(C.c_double))]


def undistort_batch(ctx, clouds, start_poses, end_poses, inplace=False):
    """pvlm_undistort_batch: clouds — list of n x 4 float32 arrays; start_poses / end_poses — lists of (R 3x3, t 3), world <- sensor.  Returns the
    motion-compensated copies (Velodyne::UndistortCloud); inplace=True: the arrays themselves (C-contiguous float32 n x 4) are updated, as the C call does."""
    if inplace:
        out = list(clouds)
        for c in out:
            assert c.dtype == np.float32 and c.flags["C_CONTIGUOUS"] and c.ndim == 2 and c.shape[1] == 4
    else:
        out = [np.ascontiguousarray(c, np.float32).reshape(-1, 4).copy() for c in clouds]
    keep = []
    descs = (UndistortScanDesc * max(len(out), 1))()
    for k, c in enumerate(out):
        arrs = [_f64(start_poses[k][0]).reshape(9), _f64(start_poses[k][1]).reshape(3), _f64(end_poses[k][0]).reshape(9), _f64(end_poses[k][1]).reshape(3)]
        keep.append(arrs)
        descs[k].xyzi = _p(c, C.c_float); descs[k].n = len(c); descs[k].stride_floats = 4
        descs[k].R_wl, descs[k].t_wl, descs[k].R_we, descs[k].t_we = (_p(a, C.c_double) for a in arrs)
    ctx._check(ctx.lib.pvlm_undistort_batch(ctx._h, C.c_int(len(out)), descs), "pvlm_undistort_batch")
    return out


class FuseScanDesc(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("intensity", C.c_void_p), ("n", C.c_int), ("stride_floats", C.c_int), ("T_wl", C.POINTER(C.c_double))]


def _pose16(pose):
    """A 4x4 world <- sensor matrix or an (R 3x3, t 3) pair -> 16 contiguous doubles, row-major."""
    if isinstance(pose, (tuple, list)) and len(pose) == 2:
        T = np.eye(4)
        T[:3, :3] = np.asarray(pose[0], np.float64).reshape(3, 3); T[:3, 3] = np.asarray(pose[1], np.float64).reshape(3)
        return _f64(T).reshape(16)
    return _f64(pose).reshape(16).copy()


def _fuse_descs(clouds, poses, intensity_at, addr_of):
    if len(clouds) != len(poses):
        raise ValueError("fuse: one pose per cloud")
    cols = [intensity_at] * len(clouds) if np.isscalar(intensity_at) else list(intensity_at)
    keep = [_pose16(p) for p in poses]
    descs = (FuseScanDesc * max(len(clouds), 1))()
    for k, c in enumerate(clouds):
        n, stride = int(c.shape[0]), int(c.shape[1])
        if stride < 3 or not (0 <= cols[k] < stride):
            raise ValueError("fuse: cloud %d has %d columns, intensity at %d" % (k, stride, cols[k]))
        base = addr_of(c)
        descs[k].xyz = base; descs[k].intensity = base + 4 * int(cols[k]); descs[k].n = n; descs[k].stride_floats = stride
        descs[k].T_wl = _p(keep[k], C.c_double)
    return descs, keep


def fuse_scans(ctx, clouds, poses, min_range, max_range, intensity_at=3, capacity=None):
    """pvlm_fuse_scans (K29, the body of LidarOdometry::FuseLidar over the given scans): clouds — list of n x stride float32 arrays (x, y, z in columns 0..2,
    intensity in column `intensity_at`: 3 for packed x y z i, 4 for pcl::PointXYZI's 8-float layout; an int or one per cloud); poses — 4x4 world <- sensor
    matrices or (R, t) pairs.  Returns (kept points, m x 4 float32 in scan order then point order; per-scan counts, int64).  capacity (points, default: every
    input point) below the kept count raises PvlmError."""
    clouds = [np.ascontiguousarray(c, np.float32) for c in clouds]
    if any(c.ndim != 2 for c in clouds):
        raise ValueError("fuse_scans: n x stride arrays")
    descs, keep = _fuse_descs(clouds, poses, intensity_at, lambda c: c.ctypes.data)
    total = int(sum(len(c) for c in clouds))
    cap = total if capacity is None else int(capacity)
    out = np.zeros((max(cap, 1), 4), np.float32)
    n_out = C.c_longlong(0)
    per = np.zeros(max(len(clouds), 1), np.int64)
    rc = ctx.lib.pvlm_fuse_scans(ctx._h, C.c_int(len(clouds)), descs, C.c_double(min_range), C.c_double(max_range), _p(out, C.c_float), C.c_longlong(cap),
                                 C.byref(n_out), _p(per, C.c_longlong))
    ctx._check(rc, "pvlm_fuse_scans (%d points kept)" % n_out.value)
    return out[:n_out.value], per[:len(clouds)]


def fuse_scans_dev(ctx, tensors, poses, min_range, max_range, intensity_at=3, out=None, capacity=None):
    """pvlm_fuse_scans_dev on torch tensors (float32, C-contiguous n x stride on the context's device), queued on torch's current stream without a host
    synchronisation.  The context is bound to that stream (Context.set_stream) only when it is not bound to it already: that first binding waits for what the
    context had queued on the stream it was bound to before, and it lasts — later calls on this context run on torch's stream until Context.use_own_stream.
    out: a float32 (capacity x 4) device tensor, 16-byte aligned (default: room for every input point).  Returns (out, per-scan counts (int64 device tensor),
    kept count (int64 device tensor of one element, the full count even past capacity)): out[:min(count, capacity)] holds the points."""
    import torch
    dev = tensors[0].device if len(tensors) else torch.device("cuda", ctx.device)
    for t in tensors:
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.device != dev:
            raise ValueError("fuse_scans_dev: float32, 2-D, C-contiguous tensors on one device")
    descs, keep = _fuse_descs(tensors, poses, intensity_at, lambda t: t.data_ptr())
    total = int(sum(int(t.shape[0]) for t in tensors))
    if out is None:
        out = torch.empty((max(total if capacity is None else int(capacity), 1), 4), dtype=torch.float32, device=dev)
    cap = int(out.shape[0]) if capacity is None else int(capacity)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev or cap < 0 or out.numel() < 4 * cap or out.data_ptr() % 16:
        raise ValueError("fuse_scans_dev: out must be a contiguous, 16-byte aligned float32 tensor of at least capacity x 4 on the clouds' device")
    per = torch.zeros(max(len(tensors), 1), dtype=torch.int64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if ctx._bound_stream != int(stream or 0):
        ctx.set_stream(stream)
    ctx._check(ctx.lib.pvlm_fuse_scans_dev(ctx._h, C.c_int(len(tensors)), descs, C.c_double(min_range), C.c_double(max_range), C.c_void_p(out.data_ptr()),
                                           C.c_longlong(cap), C.c_void_p(n.data_ptr()), C.c_void_p(per.data_ptr())), "pvlm_fuse_scans_dev")
    return out, per[:len(tensors)], n


class ColorizePairDesc(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("n", C.c_int), ("stride_floats", C.c_int), ("T_cl", C.POINTER(C.c_double)), ("bgr", C.c_void_p), ("rows", C.c_int),
                ("cols", C.c_int), ("row_bytes", C.c_longlong)]


def _colorize_descs(clouds, T_cl, images, addr_of, shape_of):
    """T_cl[k] None: pair k is left out (a pose is invalid; it gets no points).  Otherwise 12 (rows 0..2) or 16 doubles, or a 3x4 / 4x4 matrix."""
    if not (len(clouds) == len(T_cl) == len(images)):
        raise ValueError("colorize: one T_cl and one image per cloud")
    keep, descs = [], (ColorizePairDesc * max(len(clouds), 1))()
    for k, (c, T, im) in enumerate(zip(clouds, T_cl, images)):
        n, stride = int(c.shape[0]), int(c.shape[1])
        if stride < 3:
            raise ValueError("colorize: cloud %d has %d columns" % (k, stride))
        if T is None or n == 0:
            continue
        t = _f64(T).reshape(-1)[:12].copy()
        if t.size != 12:
            raise ValueError("colorize: T_cl %d needs rows 0..2 of a 4x4 transform" % k)
        rows, cols, ch = shape_of(im)
        if ch != 3:
            raise ValueError("colorize: image %d is not rows x cols x 3 BGR" % k)
        keep.append(t)
        descs[k].xyz = addr_of(c); descs[k].n = n; descs[k].stride_floats = stride; descs[k].T_cl = _p(t, C.c_double)
        descs[k].bgr = addr_of(im); descs[k].rows = rows; descs[k].cols = cols; descs[k].row_bytes = 3 * cols
    return descs, keep


def colorize_scans(ctx, clouds, T_cl, images, min_dist, max_dist, capacity=None):
    """pvlm_colorize_scans (K30, the colour stage of Texture::ColorizeLidarPointCloud): clouds — list of n x stride float32 arrays (x, y, z in columns 0..2;
    pcl::PointXYZI's layout is stride 8); T_cl — camera <- LiDAR transforms (rows 0..2 used; None = the pair is skipped); images — rows x cols x 3 uint8 BGR
    arrays (host memory; they never go to the device).  Returns (records, m x 4 float32: x y z of the LiDAR-frame point and the bits of the colour word
    b | g << 8 | r << 16 | 255 << 24, in pair order then point order; per-pair counts, int64)."""
    clouds = [np.ascontiguousarray(c, np.float32) for c in clouds]
    images = [np.ascontiguousarray(im, np.uint8) for im in images]
    if any(c.ndim != 2 for c in clouds) or any(im.ndim != 3 for im in images):
        raise ValueError("colorize_scans: n x stride clouds and rows x cols x 3 images")
    descs, keep = _colorize_descs(clouds, T_cl, images, lambda a: a.ctypes.data, lambda im: im.shape)
    total = int(sum(len(c) for c, T in zip(clouds, T_cl) if T is not None))
    cap = total if capacity is None else int(capacity)
    out = np.zeros((max(cap, 1), 4), np.float32)
    n_out = C.c_longlong(0)
    per = np.zeros(max(len(clouds), 1), np.int64)
    rc = ctx.lib.pvlm_colorize_scans(ctx._h, C.c_int(len(clouds)), descs, C.c_double(min_dist), C.c_double(max_dist), _p(out, C.c_float), C.c_longlong(cap),
                                     C.byref(n_out), _p(per, C.c_longlong))
    ctx._check(rc, "pvlm_colorize_scans (%d points kept)" % n_out.value)
    return out[:n_out.value], per[:len(clouds)]


def colorize_scans_dev(ctx, clouds, T_cl, images, min_dist, max_dist, out=None, capacity=None):
    """pvlm_colorize_scans_dev on torch tensors: clouds float32 n x stride, images uint8 rows x cols x 3 (BGR), all C-contiguous on the context's device; queued
    on torch's current stream without a host synchronisation.  The context is bound to that stream only when it is not bound to it already (as fuse_scans_dev).
    Returns (out (capacity x 4 float32, 16-byte aligned; out[:min(count, capacity)] holds the records), per-pair counts (int64 device tensor), kept count
    (int64 device tensor of one element, the full count even past capacity))."""
    import torch
    dev = clouds[0].device if len(clouds) else torch.device("cuda", ctx.device)
    for t in clouds:
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.device != dev:
            raise ValueError("colorize_scans_dev: float32, 2-D, C-contiguous clouds on one device")
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or not im.is_contiguous() or im.device != dev:
            raise ValueError("colorize_scans_dev: uint8 rows x cols x 3, C-contiguous images on the clouds' device")
    descs, keep = _colorize_descs(clouds, T_cl, images, lambda t: t.data_ptr(), lambda im: tuple(int(v) for v in im.shape))
    total = int(sum(int(c.shape[0]) for c, T in zip(clouds, T_cl) if T is not None))
    if out is None:
        out = torch.empty((max(total if capacity is None else int(capacity), 1), 4), dtype=torch.float32, device=dev)
    cap = int(out.shape[0]) if capacity is None else int(capacity)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev or cap < 0 or out.numel() < 4 * cap or out.data_ptr() % 16:
        raise ValueError("colorize_scans_dev: out must be a contiguous, 16-byte aligned float32 tensor of at least capacity x 4 on the clouds' device")
    per = torch.zeros(max(len(clouds), 1), dtype=torch.int64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if ctx._bound_stream != int(stream or 0):
        ctx.set_stream(stream)
    ctx._check(ctx.lib.pvlm_colorize_scans_dev(ctx._h, C.c_int(len(clouds)), descs, C.c_double(min_dist), C.c_double(max_dist), C.c_void_p(out.data_ptr()),
                                               C.c_longlong(cap), C.c_void_p(n.data_ptr()), C.c_void_p(per.data_ptr())), "pvlm_colorize_scans_dev")
    return out, per[:len(clouds)], n


def colorize_debug_hsv(ctx, bgr):
    """pvlm_colorize_debug_hsv: the device's OpenCV 8-bit BGR -> HSV of n x 3 uint8 pixels (tests)."""
    bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
    hsv = np.zeros_like(bgr)
    ctx._check(ctx.lib.pvlm_colorize_debug_hsv(ctx._h, C.c_longlong(len(bgr)), _p(bgr, C.c_ubyte), _p(hsv, C.c_ubyte)), "pvlm_colorize_debug_hsv")
    return hsv


def filter_tracks(ctx, mode, rows, cols, point_offsets, frame_ids, keypoints, points, T_cw, threshold):
    """pvlm_filter_tracks (K31): FilterTracksPixelResidual (mode "pixel") / FilterTracksAngleResidual (mode "angle") as a keep mask.
    point_offsets: tracks + 1 (int64), frame_ids / keypoints (float32 n x 2): one per observation, points: tracks x 3, T_cw: frames x 3 x 4
    (zeros for frames without a valid pose).  Returns a uint8 mask, 1 = the track survives."""
    off = _i64(point_offsets); fid = _i32(frame_ids); kp = _f32(keypoints); X = _f64(points); T = _f64(T_cw)
    n = len(off) - 1
    keep = np.zeros(n, np.uint8)
    ctx._check(ctx.lib.pvlm_filter_tracks(ctx._h, C.c_int(FILTER_MODES[mode]), C.c_int(rows), C.c_int(cols), C.c_int(n), _p(off, C.c_int64), _p(fid, C.c_int),
                                          _p(kp, C.c_float), _p(X, C.c_double), C.c_int(T.reshape(-1, 12).shape[0]), _p(T, C.c_double), C.c_double(threshold),
                                          _p(keep, C.c_ubyte)), "pvlm_filter_tracks")
    return keep


def triangulate_tracks(ctx, rows, cols, track_offsets, frame_ids, T_cw, frame_valid=None, keypoints=None, bearings=None):
    """pvlm_triangulate_tracks (K32): TriangulateNView per track.  track_offsets: tracks + 1 (int64); frame_ids: one per observation; T_cw: frames x 3 x 4;
    frame_valid: frames (uint8) or None; exactly one of keypoints (float32 n x 2 pixels) and bearings (float32 n x 3).  Returns (points tracks x 3 float64,
    status uint8: 0 triangulated, 1 dropped by the inf rule, 2 an observation in an invalid frame)."""
    off = _i64(track_offsets); fid = _i32(frame_ids); T = _f64(T_cw)
    kp = None if keypoints is None else _f32(keypoints)
    br = None if bearings is None else _f32(bearings)
    fv = None if frame_valid is None else np.ascontiguousarray(frame_valid, np.uint8)
    n = len(off) - 1
    X = np.zeros((max(n, 0), 3), np.float64); status = np.zeros(max(n, 0), np.uint8)
    ctx._check(ctx.lib.pvlm_triangulate_tracks(ctx._h, C.c_int(rows), C.c_int(cols), C.c_int(n), _p(off, C.c_int64), _p(fid, C.c_int),
                                               None if kp is None else _p(kp, C.c_float), None if br is None else _p(br, C.c_float),
                                               C.c_int(T.reshape(-1, 12).shape[0]), _p(T, C.c_double), None if fv is None else _p(fv, C.c_ubyte),
                                               _p(X, C.c_double), _p(status, C.c_ubyte)), "pvlm_triangulate_tracks")
    return X, status


def filter_tracks_far(ctx, track_offsets, frame_ids, points, t_wc, threshold, frame_valid=None):
    """pvlm_filter_tracks_far (K32): FilterTracksToFar as a keep mask.  points: tracks x 3; t_wc: frames x 3 camera centres; frame_valid: frames (uint8) or
    None.  Returns a uint8 mask, 1 = the track survives (threshold * baseline >= average distance, or the comparison involves a NaN)."""
    off = _i64(track_offsets); fid = _i32(frame_ids); X = _f64(points); t = _f64(t_wc)
    fv = None if frame_valid is None else np.ascontiguousarray(frame_valid, np.uint8)
    n = len(off) - 1
    keep = np.zeros(max(n, 0), np.uint8)
    ctx._check(ctx.lib.pvlm_filter_tracks_far(ctx._h, C.c_int(n), _p(off, C.c_int64), _p(fid, C.c_int), _p(X, C.c_double), C.c_int(t.reshape(-1, 3).shape[0]),
                                              _p(t, C.c_double), None if fv is None else _p(fv, C.c_ubyte), C.c_double(threshold), _p(keep, C.c_ubyte)),
               "pvlm_filter_tracks_far")
    return keep


FLAG_MATCH_EXACT = 0x400


class MatchStats(C.Structure):
    _fields_ = [("queries", C.c_longlong), ("fallback_queries", C.c_longlong), ("batches", C.c_int)]


MATCH_DTYPE = np.dtype([("query", np.int32), ("train", np.int32), ("distance", np.float32)])


class DescSet:
    """pvlm_descset (K33): the SIFT descriptors of a set of frames, resident on the device.  descs: one array of rows x 128 float32 per frame (rows may be 0)."""

    def __init__(self, ctx, descs):
        self.ctx = ctx
        self._h = C.c_void_p()
        arrs = [np.ascontiguousarray(d, np.float32) for d in descs]
        arrs = [a if a.ndim == 2 else a.reshape(-1, 128) for a in arrs]
        widths = set(a.shape[1] for a in arrs)
        width = widths.pop() if len(widths) == 1 else (128 if not widths else -1)
        self.rows = np.array([a.shape[0] for a in arrs], np.int32)
        ptrs = (C.POINTER(C.c_float) * max(len(arrs), 1))(*[_p(a, C.c_float) if a.shape[0] else None for a in arrs])
        ctx._check(ctx.lib.pvlm_descset_create(ctx._h, C.c_int(len(arrs)), _p(self.rows, C.c_int), C.c_int(width), ptrs, C.byref(self._h)), "pvlm_descset_create")

    def close(self):
        if self._h and self.ctx._h:
            self.ctx.lib.pvlm_descset_destroy(self.ctx._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_knn2(ctx, descset, src, tgt, flags=0):
    """pvlm_match_knn2 (K33): the raw knnMatch(d[src], d[tgt], 2) of every pair.  Returns (idx queries x 2 int32, -1 where absent; dist queries x 2 float32, +inf where
    absent; stats dict), the queries of all pairs one pair after the other."""
    src = _i32(src); tgt = _i32(tgt)
    nq = int(descset.rows[src].sum()) if len(src) else 0
    idx = np.zeros((nq, 2), np.int32); dist = np.zeros((nq, 2), np.float32)
    st = MatchStats()
    ctx._check(ctx.lib.pvlm_match_knn2(ctx._h, descset._h, C.c_int(len(src)), _p(src, C.c_int), _p(tgt, C.c_int), C.c_uint(flags), _p(idx, C.c_int), _p(dist, C.c_float),
                                       C.byref(st)), "pvlm_match_knn2")
    return idx, dist, dict(queries=st.queries, fallback_queries=st.fallback_queries, batches=st.batches)


MATCH_GUARD = 8      # sentinel records match_pairs keeps behind the capacity it passes on


def match_pairs(ctx, descset, src, tgt, ratio, matches_threshold, flags=0, capacity=None):
    """pvlm_match_pairs (K33): MatchSIFT and the pair filter of SfM::MatchImagePairs for every pair.  Returns a dict: keep (uint8 per pair), offsets (int64, pairs + 1),
    matches (MATCH_DTYPE records of the surviving pairs in pair order, then query order; the first `capacity` of them when overflow), needed, stats, overflow (True
    when `capacity` records were too few), guard_intact (the MATCH_GUARD sentinel records kept behind `capacity` were not written)."""
    src = _i32(src); tgt = _i32(tgt)
    cap = int(descset.rows[src].sum()) if capacity is None and len(src) else int(capacity or 0)
    keep = np.zeros(len(src), np.uint8); off = np.zeros(len(src) + 1, np.int64)
    out = np.zeros(cap + MATCH_GUARD, MATCH_DTYPE)
    out["query"] = -7; out["train"] = -7; out["distance"] = -7.0
    needed = C.c_longlong(0); st = MatchStats()
    rc = ctx.lib.pvlm_match_pairs(ctx._h, descset._h, C.c_int(len(src)), _p(src, C.c_int), _p(tgt, C.c_int), C.c_float(ratio), C.c_int(matches_threshold), C.c_uint(flags),
                                  _p(keep, C.c_ubyte), _p(off, C.c_longlong), out.ctypes.data_as(C.c_void_p), C.c_longlong(cap), C.byref(needed), C.byref(st))
    if rc != -5:
        ctx._check(rc, "pvlm_match_pairs")
    g = out[cap:]
    return dict(keep=keep, offsets=off, matches=out[:min(needed.value, cap)], needed=needed.value, overflow=rc == -5,
                guard_intact=bool(np.all(g["query"] == -7) and np.all(g["train"] == -7) and np.all(g["distance"] == -7.0)),
                stats=dict(queries=st.queries, fallback_queries=st.fallback_queries, batches=st.batches))


class DepthfillStats(C.Structure):
    _fields_ = [("images", C.c_longlong), ("batches", C.c_longlong), ("valid_in", C.c_longlong), ("valid_out", C.c_longlong), ("splat_ms", C.c_double), ("fill_ms", C.c_double)]


def _depthfill_stats(st):
    return dict(images=st.images, batches=st.batches, valid_in=st.valid_in, valid_out=st.valid_out, splat_ms=st.splat_ms, fill_ms=st.fill_ms)


class VladStats(C.Structure):
    _fields_ = [("queries", C.c_longlong), ("fallback_queries", C.c_longlong), ("iterations", C.c_int), ("dead_centres", C.c_int), ("batches", C.c_int)]


def _vlad_stats(st):
    return dict(queries=st.queries, fallback_queries=st.fallback_queries, iterations=st.iterations, dead_centres=st.dead_centres, batches=st.batches)


def vlad_kmeans(ctx, descset, train_frames, book_size, max_iterations, init_rows, flags=0):
    """pvlm_vlad_kmeans (K35): the k-means codebook of sfm/VLAD.cpp over the rows of the train frames.  init_rows: book_size indices into the concatenation of the train
    frames' rows, in list order.  Returns (codebook book_size x 128 float32, alive uint8, assign int32 per training row, stats dict)."""
    tf = _i32(train_frames); init = _i64(init_rows)
    ok = (tf >= 0) & (tf < len(descset.rows))
    n = int(descset.rows[tf[ok]].sum()) if len(tf) else 0
    if len(init) != book_size:
        raise PvlmError("vlad_kmeans: %d init_rows for %d centres" % (len(init), book_size))
    codebook = np.zeros((max(book_size, 0), 128), np.float32); alive = np.zeros(max(book_size, 0), np.uint8); assign = np.zeros(n, np.int32)
    st = VladStats()
    ctx._check(ctx.lib.pvlm_vlad_kmeans(ctx._h, descset._h, C.c_int(len(tf)), _p(tf, C.c_int), C.c_int(book_size), C.c_int(max_iterations), _p(init, C.c_longlong),
                                        C.c_uint(flags), _p(codebook, C.c_float), _p(alive, C.c_ubyte), _p(assign, C.c_int), C.byref(st)), "pvlm_vlad_kmeans")
    return codebook, alive, assign, _vlad_stats(st)


class VladSet:
    """pvlm_vladset (K35): the VLAD vectors of the frames of a DescSet, resident on the device."""

    def __init__(self, ctx, handle, n_frames, book_size, stats):
        self.ctx, self._h, self.n_frames, self.book_size, self.stats = ctx, handle, n_frames, book_size, stats

    def read(self):
        out = np.zeros((self.n_frames, 128 * self.book_size), np.float32)
        self.ctx._check(self.ctx.lib.pvlm_vladset_read(self.ctx._h, self._h, _p(out, C.c_float)), "pvlm_vladset_read")
        return out

    def close(self):
        if self._h and self.ctx._h:
            self.ctx.lib.pvlm_vladset_destroy(self.ctx._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vlad_embed(ctx, descset, codebook, alive=None, normalization=2, flags=0):
    """pvlm_vlad_embed (K35): the VLAD vector of every frame of the set (normalization 0, 1, 2 as VLAD.h).  Returns a VladSet (read(), close(), stats)."""
    cb = np.ascontiguousarray(codebook, np.float32).reshape(-1, 128)
    a = None if alive is None else np.ascontiguousarray(alive, np.uint8)
    h = C.c_void_p(); st = VladStats()
    ctx._check(ctx.lib.pvlm_vlad_embed(ctx._h, descset._h, C.c_int(len(cb)), _p(cb, C.c_float), None if a is None else _p(a, C.c_ubyte), C.c_int(normalization),
                                       C.c_uint(flags), C.byref(h), C.byref(st)), "pvlm_vlad_embed")
    return VladSet(ctx, h, len(descset.rows), len(cb), _vlad_stats(st))


def vlad_neighbors(ctx, vladset, neighbor_size, want_sim=False):
    """pvlm_vlad_neighbors (K35): per frame its min(neighbor_size, n) most similar frames by inner product (itself included).  Returns (neighbors int32, sim float64
    n x n or None)."""
    n = vladset.n_frames
    nb = np.zeros((n, max(min(neighbor_size, n), 0)), np.int32)
    sim = np.zeros((n, n), np.float64) if want_sim else None
    ctx._check(ctx.lib.pvlm_vlad_neighbors(ctx._h, vladset._h, C.c_int(neighbor_size), _p(nb, C.c_int), None if sim is None else _p(sim, C.c_double)), "pvlm_vlad_neighbors")
    return nb, sim


class DepthSet:
    """pvlm_depthset (K37 / K39): the uint16 depth maps of a set of frames, resident on the device.  compute / compute_flat make one from LiDAR scans
    (pvlm_depthset_compute: what Context.compute_depth_images computes, left on the device); create makes one of empty frames for upload."""

    def __init__(self, ctx, handle, n_frames, stats=None):
        self.ctx, self._h, self.n_frames, self.stats = ctx, handle, n_frames, stats

    @classmethod
    def compute(cls, ctx, rows, cols, clouds, T_cl, size, max_depth):
        clouds = [_f32(c).reshape(-1, 3) for c in clouds]
        first = np.zeros(len(clouds) + 1, np.int64)
        first[1:] = np.cumsum([len(c) for c in clouds])
        xyz = np.ascontiguousarray(np.concatenate(clouds + [np.zeros((1, 3), np.float32)]))
        return cls.compute_flat(ctx, rows, cols, first, xyz, T_cl, size, max_depth)

    @classmethod
    def compute_flat(cls, ctx, rows, cols, first_point, xyz, T_cl, size, max_depth):
        first = _i64(first_point); xyz = _f32(xyz).reshape(-1, 3); T = _f64(T_cl).reshape(16)
        n = max(len(first) - 1, 0)
        h = C.c_void_p(); st = DepthfillStats()
        ctx._check(ctx.lib.pvlm_depthset_compute(ctx._h, C.c_int(rows), C.c_int(cols), C.c_int(n), _p(first, C.c_longlong), _p(xyz, C.c_float), _p(T, C.c_double),
                                                 C.c_uint(size), C.c_float(max_depth), C.byref(h), C.byref(st)), "pvlm_depthset_compute")
        return cls(ctx, h, n, _depthfill_stats(st))

    @classmethod
    def create(cls, ctx, n_frames):
        h = C.c_void_p()
        ctx._check(ctx.lib.pvlm_depthset_create(ctx._h, C.c_int(n_frames), C.byref(h)), "pvlm_depthset_create")
        return cls(ctx, h, n_frames)

    def _live(self, what):
        if not self._h or not self.ctx._h:
            raise PvlmError(what + ": the depth set was closed")

    def upload(self, frame, depth_u16):
        self._live("DepthSet.upload")
        d = np.ascontiguousarray(depth_u16, np.uint16)
        if d.ndim != 2:
            raise PvlmError("DepthSet.upload: a rows x cols uint16 map")
        self.ctx._check(self.ctx.lib.pvlm_depthset_upload(self.ctx._h, self._h, C.c_int(frame), C.c_int(d.shape[0]), C.c_int(d.shape[1]), _p(d, C.c_uint16)),
                        "pvlm_depthset_upload")

    def info(self, frame):
        """(rows, cols) of the frame's map; (0, 0) for an empty frame"""
        self._live("DepthSet.info")
        r = C.c_int(0); c = C.c_int(0)
        self.ctx._check(self.ctx.lib.pvlm_depthset_info(self._h, C.c_int(frame), C.byref(r), C.byref(c)), "pvlm_depthset_info")
        return r.value, c.value

    def read(self, frame):
        self._live("DepthSet.read")
        rows, cols = self.info(frame)
        out = np.zeros((rows, cols), np.uint16)
        if rows and cols:
            self.ctx._check(self.ctx.lib.pvlm_depthset_read(self.ctx._h, self._h, C.c_int(frame), _p(out, C.c_uint16)), "pvlm_depthset_read")
        return out

    def close(self):
        if self._h and self.ctx._h:
            self.ctx.lib.pvlm_depthset_destroy(self.ctx._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScaleStats(C.Structure):
    _fields_ = [("pairs_mean", C.c_longlong), ("pairs_median", C.c_longlong), ("pairs_unscaled", C.c_longlong), ("points_tested", C.c_longlong),
                ("points_scaled", C.c_longlong), ("batches", C.c_longlong)]


def scale_workgroup_size():
    """pvlm_scale_workgroup_size (K39): the lanes of the workgroup that scales one pair."""
    return int(load_library().pvlm_scale_workgroup_size())


def set_translation_scales(ctx, depthset, eq_rows, eq_cols, frame_rows, src, tgt, point_offsets, R_21, t_21, triangulated, points_with_depth=None, upper_scale=None,
                           lower_scale=None, check=True):
    """pvlm_set_translation_scales (K39): SfM::SetTranslationScaleDepthMap(eq, pair) for every pair on the maps of a DepthSet.  points_with_depth / upper_scale /
    lower_scale: what the pairs hold before the call (default 0, -1, -1: util/MatchPair.h's constructors).  The inputs are not modified.  Returns a dict: t_21
    (pairs x 3), triangulated (points x 3), ok (uint8), points_with_depth (int32), upper_scale, lower_scale, stats, rc.  An argument the library refuses raises
    PvlmError; with check=False the dict comes back with its rc (the outputs then hold the inputs)."""
    if not depthset._h:
        raise PvlmError("set_translation_scales: the depth set was closed")
    fr = _i32(frame_rows); src = _i32(src); tgt = _i32(tgt); off = _i64(point_offsets)
    npairs = len(src); npts = int(np.asarray(triangulated).size // 3)
    R = np.zeros((npairs + 1, 3, 3)); R[:npairs] = np.asarray(R_21, np.float64).reshape(npairs, 3, 3)
    t = np.zeros((npairs + 1, 3)); t[:npairs] = np.asarray(t_21, np.float64).reshape(npairs, 3)
    tri = np.zeros((npts + 1, 3)); tri[:npts] = np.asarray(triangulated, np.float64).reshape(npts, 3)
    ok = np.full(npairs + 1, 0xA5, np.uint8)
    pwd = np.zeros(npairs + 1, np.int32); up = np.full(npairs + 1, -1.0); lo = np.full(npairs + 1, -1.0)
    if points_with_depth is not None:
        pwd[:npairs] = points_with_depth
    if upper_scale is not None:
        up[:npairs] = upper_scale
    if lower_scale is not None:
        lo[:npairs] = lower_scale
    st = ScaleStats()
    rc = ctx.lib.pvlm_set_translation_scales(ctx._h, depthset._h, C.c_int(eq_rows), C.c_int(eq_cols), _p(fr, C.c_int), C.c_int(npairs), _p(src, C.c_int), _p(tgt, C.c_int),
                                             _p(off, C.c_longlong), _p(R, C.c_double), _p(t, C.c_double), _p(tri, C.c_double), _p(ok, C.c_ubyte), _p(pwd, C.c_int),
                                             _p(up, C.c_double), _p(lo, C.c_double), C.byref(st))
    if check:
        ctx._check(rc, "pvlm_set_translation_scales")
    return dict(t_21=t[:npairs], triangulated=tri[:npts], ok=ok[:npairs], points_with_depth=pwd[:npairs], upper_scale=up[:npairs], lower_scale=lo[:npairs],
                stats={k: getattr(st, k) for k, _ in ScaleStats._fields_}, rc=int(rc))


class EssentialParams(C.Structure):
    _fields_ = [("n_runs", C.c_int), ("max_iterations", C.c_int), ("triangulation_num_threshold", C.c_int), ("seed", C.c_ulonglong)]


class EssentialStats(C.Structure):
    _fields_ = [("chains", C.c_longlong), ("hypotheses", C.c_longlong), ("lds_chains", C.c_longlong), ("fallback_chains", C.c_longlong)]


FLAG_ESSENTIAL_FRESH_SAMPLE = 0x800
ESSENTIAL_GUARD = 8      # sentinel records the two K34 calls keep behind the capacity they pass on


def _essential_inputs(bearings, src, tgt, match_offsets, matches):
    arrs = [np.ascontiguousarray(b, np.float32).reshape(-1, 3) for b in bearings]
    rows = np.array([a.shape[0] for a in arrs], np.int32)
    ptrs = (C.POINTER(C.c_float) * max(len(arrs), 1))(*[_p(a, C.c_float) if a.shape[0] else None for a in arrs])
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    return arrs, rows, ptrs, _i32(src), _i32(tgt), _i64(match_offsets), m


def _essential_stats(st):
    return dict(chains=st.chains, hypotheses=st.hypotheses, lds_chains=st.lds_chains, fallback_chains=st.fallback_chains)


def essential_acransac(ctx, bearings, src, tgt, match_offsets, matches, n_runs=40, max_iterations=300, seed=0, flags=0, capacity=None):
    """pvlm_essential_acransac (K34): the raw result of every AC-RANSAC run of every pair.  bearings: one rows x 3 float32 array per frame; the matches of pair p are
    matches[match_offsets[p]:match_offsets[p + 1]] (MATCH_DTYPE).  Returns a dict: E (pairs x runs x 3 x 3, zero = no model), nfa (pairs x runs), offsets (int64, pairs *
    runs + 1), inliers (the runs' inlier sets one after the other, the first `capacity` of them when overflow), needed, overflow, guard_intact, stats."""
    arrs, rows, ptrs, src, tgt, off, m = _essential_inputs(bearings, src, tgt, match_offsets, matches)
    npairs = len(src)
    cap = int(len(m) * n_runs) if capacity is None else int(capacity)
    E = np.zeros((npairs, max(n_runs, 0), 3, 3)); nfa = np.zeros((npairs, max(n_runs, 0))); ioff = np.zeros(npairs * max(n_runs, 0) + 1, np.int64)
    inl = np.full(cap + ESSENTIAL_GUARD, -7, np.int32)
    prm = EssentialParams(n_runs, max_iterations, 0, seed); needed = C.c_longlong(0); st = EssentialStats()
    rc = ctx.lib.pvlm_essential_acransac(ctx._h, C.c_int(len(arrs)), ptrs, _p(rows, C.c_int), C.c_int(npairs), _p(src, C.c_int), _p(tgt, C.c_int), _p(off, C.c_longlong),
                                         m.ctypes.data_as(C.c_void_p), C.byref(prm), C.c_uint(flags), _p(E, C.c_double), _p(nfa, C.c_double), _p(ioff, C.c_longlong),
                                         _p(inl, C.c_int), C.c_longlong(cap), C.byref(needed), C.byref(st))
    if rc != -5:
        ctx._check(rc, "pvlm_essential_acransac")
    return dict(E=E, nfa=nfa, offsets=ioff, inliers=inl[:min(needed.value, cap)], needed=needed.value, overflow=rc == -5, guard_intact=bool(np.all(inl[cap:] == -7)),
                stats=_essential_stats(st))


def filter_image_pairs(ctx, bearings, src, tgt, match_offsets, matches, triangulation_num_threshold, n_runs=40, max_iterations=300, seed=0, flags=0, capacity=None):
    """pvlm_filter_image_pairs (K34): the loop body of SfM::FilterImagePairs up to RefineRelativePose.  Returns a dict: keep (uint8 per pair), R_21 (pairs x 3 x 3), t_21
    (pairs x 3), offsets (int64, pairs + 1), inlier_idx (indices into the pair's matches) and triangulated (x 3) of the kept pairs' winning runs, needed, overflow,
    guard_intact, stats."""
    arrs, rows, ptrs, src, tgt, off, m = _essential_inputs(bearings, src, tgt, match_offsets, matches)
    npairs = len(src)
    cap = int(len(m)) if capacity is None else int(capacity)
    keep = np.zeros(npairs, np.uint8); R = np.zeros((npairs, 3, 3)); t = np.zeros((npairs, 3)); ioff = np.zeros(npairs + 1, np.int64)
    idx = np.full(cap + ESSENTIAL_GUARD, -7, np.int32); tri = np.full((cap + ESSENTIAL_GUARD, 3), -7.0)
    prm = EssentialParams(n_runs, max_iterations, triangulation_num_threshold, seed); needed = C.c_longlong(0); st = EssentialStats()
    rc = ctx.lib.pvlm_filter_image_pairs(ctx._h, C.c_int(len(arrs)), ptrs, _p(rows, C.c_int), C.c_int(npairs), _p(src, C.c_int), _p(tgt, C.c_int), _p(off, C.c_longlong),
                                         m.ctypes.data_as(C.c_void_p), C.byref(prm), C.c_uint(flags), _p(keep, C.c_ubyte), _p(R, C.c_double), _p(t, C.c_double),
                                         _p(ioff, C.c_longlong), _p(idx, C.c_int), _p(tri, C.c_double), C.c_longlong(cap), C.byref(needed), C.byref(st))
    if rc != -5:
        ctx._check(rc, "pvlm_filter_image_pairs")
    k = min(needed.value, cap)
    return dict(keep=keep, R_21=R, t_21=t, offsets=ioff, inlier_idx=idx[:k], triangulated=tri[:k], needed=needed.value, overflow=rc == -5,
                guard_intact=bool(np.all(idx[cap:] == -7) and np.all(tri[cap:] == -7.0)), stats=_essential_stats(st))


class RelposeParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("max_num_iterations", C.c_int)]


RELPOSE_SUMMARY_DTYPE = np.dtype([("initial_cost", np.float64), ("final_cost", np.float64), ("successful_steps", np.int32), ("unsuccessful_steps", np.int32),
                                  ("termination", np.int32)], align=True)
RELPOSE_TERMINATIONS = ("max iterations", "function tolerance", "gradient tolerance", "parameter tolerance", "trust region collapsed", "initial cost not finite",
                        "no inliers")
RELPOSE_GUARD = 8      # sentinel records refine_relative_poses keeps behind every output


def relpose_workgroup_size():
    """pvlm_relpose_workgroup_size (K36): the lanes of the workgroup that refines one pair."""
    return int(load_library().pvlm_relpose_workgroup_size())


def refine_relative_poses(ctx, keypoints, img_rows, img_cols, src, tgt, match_offsets, matches, inlier_offsets, inlier_idx, R_21, t_21, triangulated, kind="pixel",
                          max_num_iterations=50, check=True):
    """pvlm_refine_relative_poses (K36): SfM::RefineRelativePose for every pair.  keypoints: one rows x 2 float32 array of pixels per frame; img_rows / img_cols: the
    frames' image sizes; the other inputs are what filter_image_pairs takes and returns.  The inputs are not modified.  Returns a dict: R_21 (pairs x 3 x 3), t_21
    (pairs x 3, unit), triangulated (inliers x 3), ok (uint8 per pair), summaries (RELPOSE_SUMMARY_DTYPE per pair), guard_intact (the RELPOSE_GUARD sentinel records
    kept behind each output were not written), rc (the pvlm_status).  An argument the library refuses raises PvlmError; with check=False the dict comes back with
    its rc instead (the outputs then hold the inputs: the library touches nothing it refuses)."""
    arrs = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    rows_kp = np.array([a.shape[0] for a in arrs], np.int32)
    ptrs = (C.POINTER(C.c_float) * max(len(arrs), 1))(*[_p(a, C.c_float) if a.shape[0] else None for a in arrs])
    ir = _i32(img_rows); ic = _i32(img_cols); src = _i32(src); tgt = _i32(tgt); moff = _i64(match_offsets); ioff = _i64(inlier_offsets)
    m = np.ascontiguousarray(matches, MATCH_DTYPE); idx = _i32(inlier_idx)
    npairs = len(src); nin = len(idx); G = RELPOSE_GUARD
    R = np.full((npairs + G, 3, 3), -7.0); R[:npairs] = np.asarray(R_21, np.float64).reshape(npairs, 3, 3)
    t = np.full((npairs + G, 3), -7.0); t[:npairs] = np.asarray(t_21, np.float64).reshape(npairs, 3)
    tri = np.full((nin + G, 3), -7.0); tri[:nin] = np.asarray(triangulated, np.float64).reshape(nin, 3)
    ok = np.full(npairs + G, 0xA5, np.uint8)
    sm = np.zeros(npairs + G, RELPOSE_SUMMARY_DTYPE); sm["termination"][npairs:] = -7
    prm = RelposeParams(BA_KINDS[kind] if isinstance(kind, str) else int(kind), max_num_iterations)
    rc = ctx.lib.pvlm_refine_relative_poses(ctx._h, C.c_int(len(arrs)), ptrs, _p(rows_kp, C.c_int), _p(ir, C.c_int), _p(ic, C.c_int), C.c_int(npairs), _p(src, C.c_int),
                                            _p(tgt, C.c_int), _p(moff, C.c_longlong), m.ctypes.data_as(C.c_void_p), _p(ioff, C.c_longlong), _p(idx, C.c_int),
                                            _p(R, C.c_double), _p(t, C.c_double), _p(tri, C.c_double), C.byref(prm), _p(ok, C.c_ubyte), sm.ctypes.data_as(C.c_void_p))
    if check:
        ctx._check(rc, "pvlm_refine_relative_poses")
    intact = bool(np.all(R[npairs:] == -7.0) and np.all(t[npairs:] == -7.0) and np.all(tri[nin:] == -7.0) and np.all(ok[npairs:] == 0xA5) and
                  np.all(sm["termination"][npairs:] == -7))
    return dict(R_21=R[:npairs], t_21=t[:npairs], triangulated=tri[:nin], ok=ok[:npairs], summaries=sm[:npairs], guard_intact=intact, rc=int(rc))


class TransavgParams(C.Structure):
    _fields_ = [("loss_a", C.c_double), ("upper_scale_ratio", C.c_double), ("lower_scale_ratio", C.c_double), ("max_num_iterations", C.c_int)]


class TransavgSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("successful_steps", C.c_int), ("unsuccessful_steps", C.c_int), ("termination", C.c_int)]


TRANSAVG_TERMINATIONS = ("max iterations", "function tolerance", "gradient tolerance", "parameter tolerance", "trust region collapsed", "initial cost not finite",
                         "no pairs")
TRANSAVG_GUARD = 8     # sentinel records the two wrappers keep behind every output


def transavg_group_size():
    """pvlm_transavg_group_size (K42): the lanes that share one camera's gather."""
    return int(load_library().pvlm_transavg_group_size())


def transavg_dlt(ctx, n_cameras, first, second, R_21, t_21, check=True):
    """pvlm_transavg_dlt (K42): TranslationAveragingDLT with camera 0 fixed at zero.  Returns a dict: translations (cameras x 3; -7 everywhere when the library wrote
    nothing), info (0, or k > 0: not positive definite), guard_intact, rc.  An argument the library refuses raises PvlmError; with check=False the dict comes back
    with its rc."""
    first = _i32(first); second = _i32(second); P = len(first); G = TRANSAVG_GUARD
    R = _f64(np.asarray(R_21, np.float64).reshape(P, 9)); t21 = _f64(np.asarray(t_21, np.float64).reshape(P, 3))
    out = np.full((n_cameras + G, 3), -7.0); info = C.c_int(-7)
    rc = ctx.lib.pvlm_transavg_dlt(ctx._h, C.c_int(n_cameras), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(R, C.c_double), _p(t21, C.c_double),
                                   _p(out, C.c_double), C.byref(info))
    if check:
        ctx._check(rc, "pvlm_transavg_dlt")
    return dict(translations=out[:n_cameras], info=int(info.value), guard_intact=bool(np.all(out[n_cameras:] == -7.0)), rc=int(rc))


def transavg_solve(ctx, first, second, R_21, t_21, scales, origin_idx, translations, weight=None, loss_a=0.01, upper_scale_ratio=1.3, lower_scale_ratio=1.0,
                   max_num_iterations=50, check=True):
    """pvlm_transavg_solve (K42): TranslationAveragingL2 under SoftLOneLoss(loss_a) (no loss when loss_a < 0).  The inputs are not modified.  Returns a dict:
    translations (cameras x 3), scales, weight (pairs), initial_cost, final_cost, successful_steps (accepted), unsuccessful_steps, termination
    (TRANSAVG_TERMINATIONS), guard_intact (the TRANSAVG_GUARD sentinel records kept behind each output were not written), rc.  An argument the library refuses
    raises PvlmError; with check=False the dict comes back with its rc (the outputs then hold the inputs: the library touches nothing it refuses)."""
    first = _i32(first); second = _i32(second); P = len(first); G = TRANSAVG_GUARD
    R = _f64(np.asarray(R_21, np.float64).reshape(P, 9)); t21 = _f64(np.asarray(t_21, np.float64).reshape(P, 3))
    t_in = np.asarray(translations, np.float64).reshape(-1, 3); F = len(t_in)
    t = np.full((F + G, 3), -7.0); t[:F] = t_in
    s = np.full(P + G, -7.0); s[:P] = np.asarray(scales, np.float64).reshape(P)
    w = np.full(P + G, -7.0); w[:P] = 1.0 if weight is None else np.asarray(weight, np.float64).reshape(P)
    prm = TransavgParams(loss_a, upper_scale_ratio, lower_scale_ratio, max_num_iterations)
    sm = TransavgSummary(-7.0, -7.0, -7, -7, -7)
    rc = ctx.lib.pvlm_transavg_solve(ctx._h, C.c_int(F), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(R, C.c_double), _p(t21, C.c_double), _p(s, C.c_double),
                                     C.c_int(origin_idx), _p(t, C.c_double), _p(w, C.c_double), C.byref(prm), C.byref(sm))
    if check:
        ctx._check(rc, "pvlm_transavg_solve")
    intact = bool(np.all(t[F:] == -7.0) and np.all(s[P:] == -7.0) and np.all(w[P:] == -7.0))
    return dict(translations=t[:F], scales=s[:P], weight=w[:P], initial_cost=sm.initial_cost, final_cost=sm.final_cost, successful_steps=sm.successful_steps,
                unsuccessful_steps=sm.unsuccessful_steps, termination=sm.termination, guard_intact=intact, rc=int(rc))


class TransdirChordalParams(C.Structure):
    _fields_ = [("loss_a", C.c_double), ("max_num_iterations", C.c_int)]


class TransdirLudParams(C.Structure):
    _fields_ = [("upper_scale_ratio", C.c_double), ("lower_scale_ratio", C.c_double), ("max_num_iterations", C.c_int)]


TRANSDIR_GUARD = 8     # sentinel records the two wrappers keep behind every output


def transdir_group_size():
    """pvlm_transdir_group_size (K46): the lanes that share one camera's gather."""
    return int(load_library().pvlm_transdir_group_size())


def transavg_chordal(ctx, first, second, directions, origin_idx, centres, loss_a=0.5, max_num_iterations=300, check=True):
    """pvlm_transavg_chordal (K46): TranslationAveragingL2Chordal on unit world-frame directions (pairs x 3) from the start `centres` (cameras x 3, zero at
    origin_idx) under HuberLoss(loss_a).  The cost does not fix the overall scale: the result keeps roughly the scale of its start.  The inputs are not modified.
    Returns a dict: centres, initial_cost, final_cost, successful_steps, unsuccessful_steps, termination (TRANSAVG_TERMINATIONS; 5 leaves the centres as they came),
    guard_intact (the TRANSDIR_GUARD sentinel records behind the output were not written), rc.  An argument the library refuses raises PvlmError; with check=False
    the dict comes back with its rc (the outputs then hold the inputs)."""
    first = _i32(first); second = _i32(second); P = len(first); G = TRANSDIR_GUARD
    d = _f64(np.asarray(directions, np.float64).reshape(P, 3))
    c_in = np.asarray(centres, np.float64).reshape(-1, 3); F = len(c_in)
    c = np.full((F + G, 3), -7.0); c[:F] = c_in
    prm = TransdirChordalParams(loss_a, max_num_iterations)
    sm = TransavgSummary(-7.0, -7.0, -7, -7, -7)
    rc = ctx.lib.pvlm_transavg_chordal(ctx._h, C.c_int(F), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(d, C.c_double), C.c_int(origin_idx), _p(c, C.c_double),
                                       C.byref(prm), C.byref(sm))
    if check:
        ctx._check(rc, "pvlm_transavg_chordal")
    return dict(centres=c[:F], initial_cost=sm.initial_cost, final_cost=sm.final_cost, successful_steps=sm.successful_steps, unsuccessful_steps=sm.unsuccessful_steps,
                termination=sm.termination, guard_intact=bool(np.all(c[F:] == -7.0)), rc=int(rc))


def transavg_lud(ctx, first, second, directions, scales, weight, origin_idx, centres, upper_scale_ratio=1.3, lower_scale_ratio=0.9, max_num_iterations=50, check=True):
    """pvlm_transavg_lud (K46): one solve of TranslationAveragingLUD's loop on unit world-frame directions, start scales (1 = a pair without a length) and the
    weights w_p > 0 of the residuals (None: all 1).  The inputs are not modified.  Returns a dict: centres (cameras x 3), scales, weight (the NEXT weights
    (|e| + 1e-2)^-1/2), sum_e (the sum of |e|; -7 when the library wrote none), the summary fields of transavg_chordal, guard_intact, rc.  An argument the library
    refuses raises PvlmError; with check=False the dict comes back with its rc (the outputs then hold the inputs)."""
    first = _i32(first); second = _i32(second); P = len(first); G = TRANSDIR_GUARD
    d = _f64(np.asarray(directions, np.float64).reshape(P, 3))
    c_in = np.asarray(centres, np.float64).reshape(-1, 3); F = len(c_in)
    c = np.full((F + G, 3), -7.0); c[:F] = c_in
    s = np.full(P + G, -7.0); s[:P] = np.asarray(scales, np.float64).reshape(P)
    w = np.full(P + G, -7.0); w[:P] = 1.0 if weight is None else np.asarray(weight, np.float64).reshape(P)
    prm = TransdirLudParams(upper_scale_ratio, lower_scale_ratio, max_num_iterations)
    sm = TransavgSummary(-7.0, -7.0, -7, -7, -7); sum_e = (C.c_double * 2)(-7.0, -7.0)
    rc = ctx.lib.pvlm_transavg_lud(ctx._h, C.c_int(F), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(d, C.c_double), _p(s, C.c_double), _p(w, C.c_double),
                                   C.c_int(origin_idx), _p(c, C.c_double), C.byref(prm), sum_e, C.byref(sm))
    if check:
        ctx._check(rc, "pvlm_transavg_lud")
    intact = bool(np.all(c[F:] == -7.0) and np.all(s[P:] == -7.0) and np.all(w[P:] == -7.0) and sum_e[1] == -7.0)
    return dict(centres=c[:F], scales=s[:P], weight=w[:P], sum_e=float(sum_e[0]), initial_cost=sm.initial_cost, final_cost=sm.final_cost, successful_steps=sm.successful_steps,
                unsuccessful_steps=sm.unsuccessful_steps, termination=sm.termination, guard_intact=intact, rc=int(rc))


class TranslpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("gap_tol", C.c_double), ("feas_tol", C.c_double)]


class TranslpSummary(C.Structure):
    _fields_ = [("gamma", C.c_double), ("dual_objective", C.c_double), ("gap", C.c_double), ("primal_residual", C.c_double), ("dual_residual", C.c_double),
                ("iterations", C.c_int), ("bumps", C.c_int), ("n_components", C.c_int), ("n_loose", C.c_int), ("termination", C.c_int)]


TRANSLP_GUARD = 8     # sentinel records the wrapper keeps behind every output
TRANSLP_TERMINATIONS = {0: "converged", 1: "iteration limit", 2: "factorisation lost", 3: "not finite", 6: "no triplets"}


def translp_group_size():
    """pvlm_translp_group_size (K47): the lanes that share one camera's or one pair's gather."""
    return int(load_library().pvlm_translp_group_size())


def transavg_l1(ctx, first, second, R_21, t_21, triplet_pairs, origin_idx, translations, max_iterations=60, gap_tol=1e-9, feas_tol=1e-9, want_duals=True, check=True):
    """pvlm_transavg_l1 (K47): TranslationAveragingL1, the triplet minimax programme, by an interior-point method.  triplet_pairs (triplets x 3): per triplet
    i < j < k the indices of its pairs (i,j), (j,k), (i,k).  translations (cameras x 3, zero at origin_idx) only has to be finite: the call starts from zero.  The
    inputs are not modified.  Returns a dict: translations, duals (triplets x 19, or None), gamma, dual_objective, gap, primal_residual, dual_residual, iterations,
    bumps, n_components, n_loose, termination (TRANSLP_TERMINATIONS; only 0 and 1 write translations and duals), guard_intact (the TRANSLP_GUARD sentinel records
    behind the outputs were not written), rc.  gamma, feasibility and the duals are the contract, the translation values are not (see pvlm.h).  An argument the
    library refuses raises PvlmError; with check=False the dict comes back with its rc (the outputs then hold what went in, duals -7)."""
    first = _i32(first); second = _i32(second); P = len(first); G = TRANSLP_GUARD
    R = _f64(np.asarray(R_21, np.float64).reshape(-1, 9)); t21 = _f64(np.asarray(t_21, np.float64).reshape(-1, 3))
    tp = _i32(np.asarray(triplet_pairs, np.int32).reshape(-1, 3)); T = len(tp)
    t_in = np.asarray(translations, np.float64).reshape(-1, 3); F = len(t_in)
    t = np.full((F + G, 3), -7.0); t[:F] = t_in
    duals = np.full((T + G, 19), -7.0) if want_duals else None
    prm = TranslpParams(max_iterations, gap_tol, feas_tol)
    sm = TranslpSummary(-7.0, -7.0, -7.0, -7.0, -7.0, -7, -7, -7, -7, -7)
    rc = ctx.lib.pvlm_transavg_l1(ctx._h, C.c_int(F), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(R, C.c_double), _p(t21, C.c_double), C.c_int(T),
                                  _p(tp, C.c_int), C.c_int(origin_idx), _p(t, C.c_double), _p(duals, C.c_double), C.byref(prm), C.byref(sm))
    if check:
        ctx._check(rc, "pvlm_transavg_l1")
    intact = bool(np.all(t[F:] == -7.0) and (duals is None or np.all(duals[T:] == -7.0)))
    out = dict(translations=t[:F], duals=None if duals is None else duals[:T], guard_intact=intact, rc=int(rc))
    for name, _ in TranslpSummary._fields_:
        out[name] = getattr(sm, name)
    return out


class TripletStats(C.Structure):
    _fields_ = [("n_triplets", C.c_longlong), ("n_kept_triplets", C.c_longlong), ("n_uncertain", C.c_longlong), ("n_kept_pairs", C.c_longlong)]


TRIPLET_GUARD = 8     # sentinel records the wrapper keeps behind every output


def triplet_group_size():
    """pvlm_triplet_group_size (K48): the lanes that share one pair's candidates."""
    return int(load_library().pvlm_triplet_group_size())


def triplets_find(ctx, n_cameras, first, second, want_triplets=True, want_pairs=True, capacity=None, check=True):
    """pvlm_triplets_find (K48): the triplets (i < j < k) of the pair graph in lexicographic order and, per triplet, the caller's list indices of its pairs (i,j),
    (j,k), (i,k).  capacity None sizes ONE call by 8 triplets per pair and repeats it once with the reported count on PVLM_ERR_CAPACITY (calls == 2), as sift_extract
    does; a given capacity is used as it is.  Returns a dict: triplets and triplet_pairs (n x 3 int32, or None), needed, pair_counts (int64 per pair), overflow,
    calls, guard_intact (the TRIPLET_GUARD sentinel records behind the outputs were not written), rc.  An argument the library refuses raises PvlmError; with
    check=False the dict comes back with its rc (needed and pair_counts then hold -7)."""
    first = _i32(first); second = _i32(second); P = len(first); G = TRIPLET_GUARD
    want = want_triplets or want_pairs

    def call(cap):
        t = np.full((cap + G, 3), -7, np.int32) if want_triplets else None
        tp = np.full((cap + G, 3), -7, np.int32) if want_pairs else None
        pc = np.full(P + G, -7, np.int64); needed = C.c_longlong(-7)
        rc = ctx.lib.pvlm_triplets_find(ctx._h, C.c_int(n_cameras), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(t, C.c_int), _p(tp, C.c_int),
                                        C.c_longlong(cap), C.byref(needed), _p(pc, C.c_longlong))
        return rc, t, tp, pc, needed.value

    cap = int(capacity) if capacity is not None else (8 * P if want else 0)
    rc, t, tp, pc, needed = call(cap)
    calls = 1
    if capacity is None and rc == ERR_CAPACITY:
        cap = needed
        rc, t, tp, pc, needed = call(cap)
        calls = 2
    if check and rc != ERR_CAPACITY:
        ctx._check(rc, "pvlm_triplets_find")
    n = max(0, min(needed, cap))
    intact = bool((t is None or np.all(t[cap:] == -7)) and (tp is None or np.all(tp[cap:] == -7)) and np.all(pc[P:] == -7))
    return dict(triplets=None if t is None else t[:n], triplet_pairs=None if tp is None else tp[:n], needed=needed, pair_counts=pc[:P], overflow=rc == ERR_CAPACITY,
                calls=calls, guard_intact=intact, rc=int(rc))


def triplets_filter(ctx, n_cameras, first, second, R_21, angle_threshold_deg, check=True):
    """pvlm_triplets_filter (K48): SfM::FilterByTriplet's test.  keep[p] = 1 when pair p lies in a triplet whose loop measure acos(trace(R_13 R_32 R_21) / 3) in
    degrees is below the threshold.  Returns a dict: keep (uint8 per pair), n_triplets, n_kept_triplets, n_uncertain (decided on the host by the literal chain),
    n_kept_pairs, guard_intact, rc.  An argument the library refuses raises PvlmError; with check=False the dict comes back with its rc (keep then holds 7s)."""
    first = _i32(first); second = _i32(second); P = len(first); G = TRIPLET_GUARD
    R = _f64(np.asarray(R_21, np.float64).reshape(-1, 9))
    keep = np.full(P + G, 7, np.uint8)
    st = TripletStats(-7, -7, -7, -7)
    rc = ctx.lib.pvlm_triplets_filter(ctx._h, C.c_int(n_cameras), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(R, C.c_double), C.c_double(angle_threshold_deg),
                                      _p(keep, C.c_ubyte), C.byref(st))
    if check:
        ctx._check(rc, "pvlm_triplets_filter")
    out = dict(keep=keep[:P], guard_intact=bool(np.all(keep[P:] == 7)), rc=int(rc))
    for name, _ in TripletStats._fields_:
        out[name] = int(getattr(st, name))
    return out


class NeighborSfmStats(C.Structure):
    _fields_ = [("n_candidates", C.c_longlong), ("n_contributions", C.c_longlong), ("n_repeat_tracks", C.c_longlong), ("n_uncertain", C.c_longlong)]


NEIGHBOR_GUARD = 4     # sentinel slots the wrapper keeps behind every output


def neighbor_sfm_tile_cols():
    """pvlm_neighbor_sfm_tile_cols (K49): the columns of a score row the accumulation holds in LDS at once (PVLM_NEIGHBOR_TILE lowers it)."""
    return int(load_library().pvlm_neighbor_sfm_tile_cols())


def _neighbor_inputs(T_wc, pose_valid, track_offsets, view_ids, points):
    T_wc = _f64(np.asarray(T_wc, np.float64).reshape(-1, 12)); F = len(T_wc)
    valid = np.ascontiguousarray(pose_valid, np.uint8)
    off = _i64(track_offsets); T = len(off) - 1
    views = _i32(np.concatenate([np.asarray(view_ids, np.int64).reshape(-1), [0]]))      # never empty
    pts = _f64(np.asarray(points, np.float64).reshape(-1, 3))
    if len(valid) != F or len(pts) != T:
        raise ValueError("pose_valid needs one entry per view and points one row per track")
    return F, T, T_wc, valid, off, views, pts


def mvs_select_neighbors_sfm(ctx, T_wc, pose_valid, track_offsets, view_ids, points, neighbor_size, sq_distance_threshold, check=True):
    """pvlm_mvs_select_neighbors_sfm (K49): MVS::SelectNeighborSFM.  T_wc: F x 3 x 4 poses; the tracks in CSR form (track_offsets T + 1, view_ids ascending inside a
    track, points T x 3).  Returns a dict: n_neighbors (F), ids (F x neighbor_size, -1 in the unused slots), R_nr (F x neighbor_size x 3 x 3 float32), t_nr
    (.. x 3), scores (F x neighbor_size), n_candidates, n_contributions, n_repeat_tracks, n_uncertain (rows redone on the host by the literal loop), guard_intact, rc.
    The norm of t_nr is compared with sq_distance_threshold as it is (upstream's test).  An argument the library refuses raises PvlmError; with check=False the dict
    comes back with its rc (the outputs then hold -7)."""
    F, T, T_wc, valid, off, views, pts = _neighbor_inputs(T_wc, pose_valid, track_offsets, view_ids, points)
    K = int(neighbor_size); n = F * max(K, 0); G = NEIGHBOR_GUARD
    nn = np.full(F + G, -7, np.int32); ids = np.full(n + G, -7, np.int32); R = np.full(9 * (n + G), -7, np.float32); t = np.full(3 * (n + G), -7, np.float32)
    sc = np.full(n + G, -7, np.float32)
    st = NeighborSfmStats(-7, -7, -7, -7)
    rc = ctx.lib.pvlm_mvs_select_neighbors_sfm(ctx._h, C.c_int(F), _p(T_wc, C.c_double), _p(valid, C.c_ubyte), C.c_int(T), _p(off, C.c_int64), _p(views, C.c_int),
                                               _p(pts, C.c_double), C.c_int(K), C.c_double(sq_distance_threshold), _p(nn, C.c_int), _p(ids, C.c_int), _p(R, C.c_float),
                                               _p(t, C.c_float), _p(sc, C.c_float), C.byref(st))
    if check:
        ctx._check(rc, "pvlm_mvs_select_neighbors_sfm")
    intact = bool(np.all(nn[F:] == -7) and np.all(ids[n:] == -7) and np.all(R[9 * n:] == -7) and np.all(t[3 * n:] == -7) and np.all(sc[n:] == -7))
    out = dict(n_neighbors=nn[:F], ids=ids[:n].reshape(F, max(K, 0)), R_nr=R[:9 * n].reshape(F, max(K, 0), 3, 3), t_nr=t[:3 * n].reshape(F, max(K, 0), 3),
               scores=sc[:n].reshape(F, max(K, 0)), guard_intact=intact, rc=int(rc))
    for name, _ in NeighborSfmStats._fields_:
        out[name] = int(getattr(st, name))
    return out


def mvs_neighbor_sfm_score_row(ctx, T_wc, pose_valid, track_offsets, view_ids, points, row):
    """pvlm_mvs_neighbor_sfm_score_row (K49): one row of the device's score matrix and the contribution counts of its cells (float32 F, int32 F); for the tests."""
    F, T, T_wc, valid, off, views, pts = _neighbor_inputs(T_wc, pose_valid, track_offsets, view_ids, points)
    s = np.full(F + NEIGHBOR_GUARD, -7, np.float32); n = np.full(F + NEIGHBOR_GUARD, -7, np.int32)
    rc = ctx.lib.pvlm_mvs_neighbor_sfm_score_row(ctx._h, C.c_int(F), _p(T_wc, C.c_double), _p(valid, C.c_ubyte), C.c_int(T), _p(off, C.c_int64), _p(views, C.c_int),
                                                 _p(pts, C.c_double), C.c_int(row), _p(s, C.c_float), _p(n, C.c_int))
    ctx._check(rc, "pvlm_mvs_neighbor_sfm_score_row")
    if not (np.all(s[F:] == -7) and np.all(n[F:] == -7)):
        raise PvlmError("pvlm_mvs_neighbor_sfm_score_row wrote past its outputs")
    return s[:F], n[:F]


class BataParams(C.Structure):
    _fields_ = [("delta", C.c_double), ("init_iteration", C.c_int), ("inner_iteration", C.c_int), ("outer_iteration", C.c_int), ("robust_threshold", C.c_double)]


BATA_GUARD = 8     # sentinel records the wrapper keeps behind every output


def bata_group_size():
    """pvlm_bata_group_size (K44): the lanes that share one camera's gather."""
    return int(load_library().pvlm_bata_group_size())


def bata_solve(ctx, n_cameras, first, second, directions, scales0, delta=1e-6, init_iteration=10, inner_iteration=10, outer_iteration=10, robust_threshold=0.1,
               check=True):
    """pvlm_transavg_bata (K44): BATA translation averaging (a revised-LUD start, then the bilinear IRLS) on unit directions (pairs x 3) and positive start scales.
    The cameras are F = max_id - min_id + 1, the ids shifted by min_id.  Returns a dict: centres and lud_centres (F x 3, camera 0 zero), scales (pairs), F, info (0;
    k > 0: not positive definite; -1: not finite; -2: no pairs), untouched (the library wrote none of the outputs: they still hold -7), guard_intact (the BATA_GUARD
    sentinel records behind each output were not written), rc.  An argument the library refuses raises PvlmError; with check=False the dict comes back with its rc."""
    first = _i32(first); second = _i32(second); P = len(first); G = BATA_GUARD
    d = _f64(np.asarray(directions, np.float64).reshape(P, 3)); s0 = _f64(np.asarray(scales0, np.float64).reshape(P))
    F = int(max(first.max(), second.max()) - min(first.min(), second.min()) + 1) if P else 0
    rows = max(int(n_cameras), F, 0)
    cen = np.full((rows + G, 3), -7.0); lud = np.full((rows + G, 3), -7.0); s = np.full(P + G, -7.0); info = C.c_int(-7)
    prm = BataParams(delta, init_iteration, inner_iteration, outer_iteration, robust_threshold)
    rc = ctx.lib.pvlm_transavg_bata(ctx._h, C.c_int(n_cameras), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(d, C.c_double), _p(s0, C.c_double), C.byref(prm),
                                    _p(cen, C.c_double), _p(lud, C.c_double), _p(s, C.c_double), C.byref(info))
    if check:
        ctx._check(rc, "pvlm_transavg_bata")
    untouched = bool(np.all(cen == -7.0) and np.all(lud == -7.0) and np.all(s == -7.0))
    intact = bool(np.all(cen[F:] == -7.0) and np.all(lud[F:] == -7.0) and np.all(s[P:] == -7.0))
    return dict(centres=cen[:F], lud_centres=lud[:F], scales=s[:P], F=F, info=int(info.value), untouched=untouched, guard_intact=intact, rc=int(rc))


class RotavgL1Summary(C.Structure):
    _fields_ = [("l1_iterations", C.c_int), ("admm_iterations", C.c_int), ("irls_iterations", C.c_int), ("info", C.c_int)]


class RotavgL2Params(C.Structure):
    _fields_ = [("loss_a", C.c_double), ("max_num_iterations", C.c_int)]


ROTAVG_GUARD = 8     # sentinel cameras the two wrappers keep behind the rotations


def rotavg_group_size():
    """pvlm_rotavg_group_size (K40): the lanes that share one camera's gather."""
    return int(load_library().pvlm_rotavg_group_size())


def _rotavg_inputs(first, second, R_21, rotations):
    first = _i32(first); second = _i32(second); P = len(first)
    R21 = _f64(np.asarray(R_21, np.float64).reshape(P, 9))
    r_in = np.asarray(rotations, np.float64).reshape(-1, 9); F = len(r_in)
    rot = np.full((F + ROTAVG_GUARD, 9), -7.0); rot[:F] = r_in
    return first, second, P, R21, F, rot


def rotavg_l1(ctx, first, second, R_21, start_idx, rotations, check=True):
    """pvlm_rotavg_l1 (K40): RotationAveragingRefineL1, the L1 (ADMM) stage and the IRLS stage, from `rotations` (cameras x 3 x 3, R_cw, the identity at start_idx).
    The inputs are not modified.  Returns a dict: rotations (cameras x 3 x 3), l1_iterations, admm_iterations, irls_iterations, info (0, or k > 0: an IRLS system
    was not finite or not positive definite), guard_intact, rc.  An argument the library refuses raises PvlmError; with check=False the dict comes back with its rc
    (the rotations then hold the input: the library touches nothing it refuses)."""
    first, second, P, R21, F, rot = _rotavg_inputs(first, second, R_21, rotations)
    sm = RotavgL1Summary(-7, -7, -7, -7)
    rc = ctx.lib.pvlm_rotavg_l1(ctx._h, C.c_int(F), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(R21, C.c_double), C.c_int(start_idx), _p(rot, C.c_double),
                                C.byref(sm))
    if check:
        ctx._check(rc, "pvlm_rotavg_l1")
    return dict(rotations=rot[:F].reshape(F, 3, 3), l1_iterations=sm.l1_iterations, admm_iterations=sm.admm_iterations, irls_iterations=sm.irls_iterations, info=sm.info,
                guard_intact=bool(np.all(rot[F:] == -7.0)), rc=int(rc))


def rotavg_l2(ctx, first, second, R_21, rotations, loss_a=0.07, max_num_iterations=50, check=True):
    """pvlm_rotavg_l2 (K40): RotationAveragingL2 under SoftLOneLoss(loss_a) (no loss when loss_a < 0).  The inputs are not modified.  Returns a dict: rotations
    (cameras x 3 x 3), initial_cost, final_cost, successful_steps (accepted), unsuccessful_steps, termination (TRANSAVG_TERMINATIONS), guard_intact, rc.  An argument
    the library refuses raises PvlmError; with check=False the dict comes back with its rc."""
    first, second, P, R21, F, rot = _rotavg_inputs(first, second, R_21, rotations)
    prm = RotavgL2Params(loss_a, max_num_iterations)
    sm = TransavgSummary(-7.0, -7.0, -7, -7, -7)
    rc = ctx.lib.pvlm_rotavg_l2(ctx._h, C.c_int(F), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(R21, C.c_double), _p(rot, C.c_double), C.byref(prm),
                                C.byref(sm))
    if check:
        ctx._check(rc, "pvlm_rotavg_l2")
    return dict(rotations=rot[:F].reshape(F, 3, 3), initial_cost=sm.initial_cost, final_cost=sm.final_cost, successful_steps=sm.successful_steps,
                unsuccessful_steps=sm.unsuccessful_steps, termination=sm.termination, guard_intact=bool(np.all(rot[F:] == -7.0)), rc=int(rc))


class RotavgLsqParams(C.Structure):
    _fields_ = [("shift_rel", C.c_double), ("tol", C.c_double), ("max_iterations", C.c_int)]


class RotavgLsqSummary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("solves", C.c_int), ("info", C.c_int), ("residual", C.c_double), ("theta", C.c_double * 3)]


def rotavg_least_square(ctx, first, second, R_21, rotations, shift_rel=1e-9, tol=1e-12, max_iterations=100, check=True):
    """pvlm_rotavg_least_square (K45): RotationAveragingLeastSquare, the start of the L2 method, by shift-and-invert subspace iteration from `rotations` (cameras x
    3 x 3: the spanning-tree start, or any 3 F x 3 matrix of full rank).  The inputs are not modified.  Returns a dict: rotations (cameras x 3 x 3, R_cw with camera 0
    the identity; the input when info is not 0), iterations, solves, info (0; k > 0: not positive definite; -1: not finite; -2: max_iterations reached; -3: a
    singular block or Gram matrix), residual (the last, over the largest degree), theta (the three Ritz values), guard_intact, rc.  An argument the library refuses
    raises PvlmError; with check=False the dict comes back with its rc (the summary then holds the sentinel -7: the library touches nothing it refuses)."""
    first, second, P, R21, F, rot = _rotavg_inputs(first, second, R_21, rotations)
    prm = RotavgLsqParams(shift_rel, tol, max_iterations)
    sm = RotavgLsqSummary(-7, -7, -7, -7.0, (C.c_double * 3)(-7.0, -7.0, -7.0))
    rc = ctx.lib.pvlm_rotavg_least_square(ctx._h, C.c_int(F), C.c_int(P), _p(first, C.c_int), _p(second, C.c_int), _p(R21, C.c_double), _p(rot, C.c_double),
                                          C.byref(prm), C.byref(sm))
    if check:
        ctx._check(rc, "pvlm_rotavg_least_square")
    return dict(rotations=rot[:F].reshape(F, 3, 3), iterations=sm.iterations, solves=sm.solves, info=sm.info, residual=sm.residual, theta=np.array(list(sm.theta)),
                guard_intact=bool(np.all(rot[F:] == -7.0)), rc=int(rc))


def device_sort(ctx, keys):
    """pvlm_ring_debug_sort: the permutation the device's std::sort restatement leaves for uint32 keys (tests)."""
    keys = np.ascontiguousarray(keys, np.uint32)
    order = np.zeros(len(keys), np.int32)
    ctx._check(ctx.lib.pvlm_ring_debug_sort(ctx._h, _p(keys, C.c_uint), C.c_int(len(keys)), _p(order, C.c_int)), "pvlm_ring_debug_sort")
    return order


class RawScanDesc(C.Structure):
    _fields_ = [("xyzi", C.POINTER(C.c_float)), ("n", C.c_int), ("stride_floats", C.c_int)]


class RingResultDesc(C.Structure):
    _fields_ = [("n_raw", C.c_int), ("n_reordered", C.c_int), ("n_kept", C.c_int), ("resolved_points", C.c_int), ("resolved_edges", C.c_int), ("replayed", C.c_int),
                ("ring_count_reordered", C.POINTER(C.c_int)), ("ring_count", C.POINTER(C.c_int)), ("source", C.POINTER(C.c_int)), ("ring_col", C.POINTER(C.c_int)),
                ("curvature", C.POINTER(C.c_float)), ("half_window", C.POINTER(C.c_int)), ("range", C.POINTER(C.c_float)), ("sorted", C.POINTER(C.c_int)),
                ("sector_host", C.POINTER(C.c_ubyte)), ("picks", C.c_int), ("max_curvature", C.c_float), ("intersect_angle_threshold", C.c_float),
                ("state", C.POINTER(C.c_ubyte)), ("corner", C.POINTER(C.c_int)), ("flat", C.POINTER(C.c_int)), ("voxel_span", C.POINTER(C.c_int)),
                ("voxels", C.POINTER(C.c_float)), ("ring_host", C.POINTER(C.c_ubyte))]


class RingBatch:
    """pvlm_ring_extract_batch: ReOrderVLP + Segmentation + adaptive curvature of a batch of raw scans (n x 4 float32 each) on the GPU."""

    def __init__(self, ctx, raw_scans, n_rings=16, horizon=1800, segment=True, picks=None, keep_arrays=True):
        """picks = (max_curvature, intersect_angle_threshold): also run K24 (feature picks + voxel grid) — see RingBatch.picks().  keep_arrays=False (with picks): the
        per-point arrays curvature / half_window / range / sorted come down only for scans with a ring left to the host, as the C++ host mirror asks for them."""
        self.ctx = ctx
        self._raw = [_f32(r).reshape(-1, 4) for r in raw_scans]
        self.n_rings, self.horizon = n_rings, horizon
        descs = (RawScanDesc * max(len(self._raw), 1))()
        for k, r in enumerate(self._raw):
            descs[k].xyzi = _p(r, C.c_float); descs[k].n = len(r); descs[k].stride_floats = 4
        self._h = C.c_void_p()
        if picks is None:
            ctx._check(ctx.lib.pvlm_ring_extract_batch(ctx._h, C.c_int(len(self._raw)), descs, C.c_int(n_rings), C.c_int(horizon), C.c_int(1 if segment else 0),
                                                       C.byref(self._h)), "pvlm_ring_extract_batch")
        else:
            ctx._check(ctx.lib.pvlm_ring_extract_batch_picks(ctx._h, C.c_int(len(self._raw)), descs, C.c_int(n_rings), C.c_int(horizon), C.c_int((1 if segment else 0) | (2 if keep_arrays else 0)),
                                                             C.c_float(picks[0]), C.c_float(picks[1]), C.byref(self._h)), "pvlm_ring_extract_batch_picks")

    def close(self):
        if self._h and self.ctx._h:
            self.ctx.lib.pvlm_ring_batch_destroy(self.ctx._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def timing(self):
        ms = np.zeros(8)
        self.ctx._check(self.ctx.lib.pvlm_ring_batch_timing(self._h, _p(ms, C.c_double)), "pvlm_ring_batch_timing")
        return dict(zip(("upload", "classify", "columns", "scatter", "edges", "components", "compact_curvature", "download"), ms.tolist()))

    def result(self, scan):
        """The kept cloud of one scan as numpy copies (the picks of the host read these arrays in place)."""
        r = RingResultDesc()
        self.ctx._check(self.ctx.lib.pvlm_ring_batch_scan(self._h, C.c_int(scan), C.byref(r)), "pvlm_ring_batch_scan")
        m = r.n_kept
        arr = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True) if n > 0 and ptr else np.zeros(0, dt)
        out = dict(n_raw=r.n_raw, n_reordered=r.n_reordered, n_kept=m, resolved_points=r.resolved_points, resolved_edges=r.resolved_edges, replayed=r.replayed,
                   ring_count_reordered=arr(r.ring_count_reordered, 64, np.int32), ring_count=arr(r.ring_count, 64, np.int32), source=arr(r.source, m, np.int32),
                   ring_col=arr(r.ring_col, m, np.int32), curvature=arr(r.curvature, m, np.float32), half_window=arr(r.half_window, m, np.int32),
                   range=arr(r.range, m, np.float32), sorted=arr(r.sorted, m, np.int32), sector_host=arr(r.sector_host, self.n_rings * 6, np.uint8))
        return out

    def picks(self, scan):
        """K24's results for one scan: dict(ring_host (n_rings flags), state (per kept point), corner / sharp (edge picks in upstream's order and which of them are
        sharp), flat (plane picks), less_flat (m x 4 centroids, ring by ring)) — or None when the batch was made without picks."""
        r = RingResultDesc()
        self.ctx._check(self.ctx.lib.pvlm_ring_batch_scan(self._h, C.c_int(scan), C.byref(r)), "pvlm_ring_batch_scan")
        if not r.picks:
            return None
        R = self.n_rings
        ring_host = np.ctypeslib.as_array(r.ring_host, shape=(R,)).copy()
        state = np.ctypeslib.as_array(r.state, shape=(max(r.n_kept, 1),))[:r.n_kept].copy()
        corner_t = np.ctypeslib.as_array(r.corner, shape=(R, 181)); flat_t = np.ctypeslib.as_array(r.flat, shape=(R, 25)); span = np.ctypeslib.as_array(r.voxel_span, shape=(R, 2))
        corner = np.concatenate([corner_t[k, 1:1 + corner_t[k, 0]] for k in range(R)]) if R else np.zeros(0, np.int32)
        flat = np.concatenate([flat_t[k, 1:1 + flat_t[k, 0]] for k in range(R)]) if R else np.zeros(0, np.int32)
        less = [np.ctypeslib.as_array(C.cast(C.addressof(r.voxels.contents) + 16 * int(span[k, 0]), C.POINTER(C.c_float)), shape=(int(span[k, 1]), 4)).copy()
                for k in range(R) if span[k, 1] > 0]
        return dict(ring_host=ring_host, state=state, corner=(corner & 0x7FFFFFFF).astype(np.int32), sharp=(corner.view(np.uint32) >> 31).astype(bool),
                    flat=flat.astype(np.int32), less_flat=np.concatenate(less) if less else np.zeros((0, 4), np.float32))

    def fetch(self, scan, state):
        """Device-resident arrays of one scan: state 0 after ReOrderVLP, 1 after Segmentation."""
        res = self.result(scan)
        n = res["n_kept"] if state else res["n_reordered"]
        cloud = np.zeros((max(n, 1), 4), np.float32); rc = np.zeros((max(n, 1), 2), np.int32)
        image = np.zeros((self.n_rings, self.horizon), np.float32); i2p = np.zeros((self.n_rings, self.horizon), np.int32)
        self.ctx._check(self.ctx.lib.pvlm_ring_batch_fetch(self.ctx._h, self._h, C.c_int(scan), C.c_int(state), _p(cloud, C.c_float), _p(rc, C.c_int), _p(image, C.c_float),
                                                           _p(i2p, C.c_int)), "pvlm_ring_batch_fetch")
        return cloud[:n], rc[:n], image, i2p

    def arrays(self, scan):
        """Everything tests/ring_cases.assert_matches_oracle compares, for one scan."""
        res = self.result(scan)
        c0, rc0, image, i2p0 = self.fetch(scan, 0)
        c1, rc1, _, i2p1 = self.fetch(scan, 1)
        return dict(n_reordered=res["n_reordered"], n_kept=res["n_kept"], cloud_reordered=c0, rc_reordered=rc0, range_image=image, image_to_point_reordered=i2p0,
                    ring_count_reordered=res["ring_count_reordered"], cloud_kept=c1, rc_kept=rc1, image_to_point_kept=i2p1, ring_count=res["ring_count"],
                    curvature=res["curvature"], half_window=res["half_window"], range=res["range"], source=res["source"], ring_col=res["ring_col"],
                    resolved_points=res["resolved_points"], resolved_edges=res["resolved_edges"], replayed=res["replayed"], sorted=res["sorted"],
                    sector_host=res["sector_host"])


# ---- K41: SIFT keypoints and (Root)SIFT descriptors ----
FLAG_SIFT_ROOT = 0x1000
SIFT_KEYPOINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32), ("octave", np.int32)])
SIFT_CANDIDATE_DTYPE = np.dtype([("octave", np.int32), ("layer", np.int32), ("r", np.int32), ("c", np.int32), ("x", np.float32), ("y", np.float32), ("size", np.float32),
                                 ("response", np.float32), ("word", np.int32), ("det_layer", np.int32), ("det_r", np.int32), ("det_c", np.int32)])
SIFT_GUARD = 4       # sentinel records sift_extract keeps behind the capacity it passes on
SIFT_TIE_ROOM, SIFT_GUESS_PER_IMAGE = 64, 1 << 15      # how sift_extract sizes a call whose capacity the caller left open


class SiftStats(C.Structure):
    _fields_ = [("images", C.c_longlong), ("octaves", C.c_longlong), ("candidates", C.c_longlong), ("keypoints_detected", C.c_longlong), ("keypoints", C.c_longlong),
                ("part_ms", C.c_double * 6)]


def _sift_images(images):
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    shapes = set(im.shape for im in imgs)
    if len(shapes) > 1 or any(im.ndim != 2 for im in imgs):
        raise PvlmError("pvlm_sift_extract: the images of a batch must be two-dimensional and of one size")
    return imgs


def sift_extract(ctx, images, nfeatures, mask=None, flags=0, capacity=None):
    """pvlm_sift_extract (K41): SIFT keypoints and 128-float descriptors (RootSIFT with FLAG_SIFT_ROOT) of a batch of equal-sized uint8 grey images.  Returns a dict:
    offsets (int64, images + 1), keypoints (SIFT_KEYPOINT_DTYPE), descriptors (n x 128 float32), needed, overflow, guard_intact, stats, calls.  A call that fails
    for capacity has done all the work but the descriptors, so capacity None sizes ONE call by min(nfeatures, SIFT_GUESS_PER_IMAGE) + SIFT_TIE_ROOM keypoints per image
    and repeats it with the reported count only when more come back (calls == 2: more ties at the threshold than the room, or an nfeatures above the guess)."""
    imgs = _sift_images(images)
    rows, cols = imgs[0].shape if imgs else (8, 8)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    if m is not None and m.shape != (rows, cols):
        raise PvlmError("pvlm_sift_extract: the mask must have the images' size")
    ptrs = (C.POINTER(C.c_ubyte) * max(len(imgs), 1))(*[_p(im, C.c_ubyte) for im in imgs])
    off = np.zeros(len(imgs) + 1, np.int64)

    def call(cap):
        kp = np.zeros(cap + SIFT_GUARD, SIFT_KEYPOINT_DTYPE); kp["octave"] = -7; kp["x"] = -7.0
        desc = np.full((cap + SIFT_GUARD, 128), -7.0, np.float32)
        needed = C.c_longlong(0); st = SiftStats()
        rc = ctx.lib.pvlm_sift_extract(ctx._h, C.c_int(len(imgs)), C.c_int(rows), C.c_int(cols), ptrs, _p(m, C.c_ubyte), C.c_int(nfeatures), C.c_uint(flags),
                                       _p(off, C.c_longlong), kp.ctypes.data_as(C.c_void_p), _p(desc, C.c_float), C.c_longlong(cap), C.byref(needed), C.byref(st))
        return rc, kp, desc, needed.value, st

    cap = int(capacity) if capacity is not None else len(imgs) * (min(max(int(nfeatures), 0), SIFT_GUESS_PER_IMAGE) + SIFT_TIE_ROOM)
    rc, kp, desc, needed, st = call(cap)
    calls = 1
    if capacity is None and rc == ERR_CAPACITY:
        cap = needed
        rc, kp, desc, needed, st = call(cap)
        calls = 2
    if rc != ERR_CAPACITY:
        ctx._check(rc, "pvlm_sift_extract")
    n = min(needed, cap)
    return dict(offsets=off.copy(), keypoints=kp[:n], descriptors=desc[:n], needed=needed, overflow=rc == ERR_CAPACITY, calls=calls,
                guard_intact=bool(np.all(kp["octave"][cap:] == -7) and np.all(kp["x"][cap:] == -7.0) and np.all(desc[cap:] == -7.0)),
                stats=dict(images=st.images, octaves=st.octaves, candidates=st.candidates, keypoints_detected=st.keypoints_detected, keypoints=st.keypoints,
                           part_ms=dict(zip("abcdef", (float(v) for v in st.part_ms)))))


def sift_pyramid_debug(ctx, image, octave):
    """pvlm_sift_pyramid_debug (K41): the Gaussian (6 x R x C) and difference (5 x R x C) layers of one octave, that octave's refined candidates
    (SIFT_CANDIDATE_DTYPE) and the image's keypoints before the selection.  Returns a dict with n_octaves, gauss, dog, candidates, keypoints."""
    im = np.ascontiguousarray(image, np.uint8)
    if im.ndim != 2:
        raise PvlmError("pvlm_sift_pyramid_debug: a two-dimensional image")
    rows, cols = im.shape
    n_oct, orows, ocols = C.c_int(0), C.c_int(0), C.c_int(0)
    nc, nk = C.c_longlong(0), C.c_longlong(0)
    # sizing call: no layers, no records
    rc = ctx.lib.pvlm_sift_pyramid_debug(ctx._h, C.c_int(rows), C.c_int(cols), _p(im, C.c_ubyte), C.c_int(octave), C.byref(n_oct), C.byref(orows), C.byref(ocols), None, None,
                                         None, C.c_longlong(0), C.byref(nc), None, C.c_longlong(0), C.byref(nk))
    if rc != ERR_CAPACITY:
        ctx._check(rc, "pvlm_sift_pyramid_debug")
    gauss = np.zeros((6, orows.value, ocols.value), np.float32); dog = np.zeros((5, orows.value, ocols.value), np.float32)
    cands = np.zeros(max(nc.value, 1), SIFT_CANDIDATE_DTYPE); kps = np.zeros(max(nk.value, 1), SIFT_KEYPOINT_DTYPE)
    ctx._check(ctx.lib.pvlm_sift_pyramid_debug(ctx._h, C.c_int(rows), C.c_int(cols), _p(im, C.c_ubyte), C.c_int(octave), C.byref(n_oct), C.byref(orows), C.byref(ocols),
                                               _p(gauss, C.c_float), _p(dog, C.c_float), cands.ctypes.data_as(C.c_void_p), C.c_longlong(len(cands)), C.byref(nc),
                                               kps.ctypes.data_as(C.c_void_p), C.c_longlong(len(kps)), C.byref(nk)), "pvlm_sift_pyramid_debug")
    return dict(n_octaves=n_oct.value, gauss=gauss, dog=dog, candidates=cands[:nc.value], keypoints=kps[:nk.value])
