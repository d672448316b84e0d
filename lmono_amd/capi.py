"""ctypes binding of include/lmono_hip.h (the drop-in C ABI).  Fails loudly when the library is absent."""
import collections
import ctypes as C
import os
import weakref

import numpy as np

from ._abi import PROTOTYPES
from .brief_tools import (_VOC_KEYS, _voc_arrays, check_brief_vocabulary, load_brief_pattern, load_brief_vocabulary,  # noqa: F401
                          save_brief_vocabulary, train_brief_vocabulary)
from .errors import LmonoError

_HERE = os.path.dirname(os.path.abspath(__file__))
MAX_QUERIES = 64 * 6 * 2 + 64 * 6 * 4

# every symbol include/lmono_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = list(PROTOTYPES)


def lib_path():
    # LMONO_HIP_LIB: a diagnostic build of the same sources (scripts/prof_tile.py); the product path is the in-tree library
    return os.environ.get("LMONO_HIP_LIB") or os.path.join(_HERE, "lib", "liblmono_hip.so")


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise LmonoError("HIP library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % p)
    L = C.CDLL(p)
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise LmonoError("HIP library %s does not export %s" % (p, name)) from None
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = L
    return L


class Context:
    """lmono_ctx wrapper.  One per process / GPU."""

    def __init__(self, device=0):
        self.L = load_library()
        self._own_stream = False          # the context starts on the null stream
        # objects created on this context (batches, streams, mappers ...): closed before the context whatever order the
        # interpreter drops them in -- their destroy calls touch the context's stream
        self._children = weakref.WeakSet()
        self.h = self.L.lmono_create(int(device))
        if not self.h:
            raise LmonoError("lmono_create(%d) failed: no usable HIP device" % device)
        self.device = device
        for env, key in (("LMONO_CORR_TILE", self.OPT_CORR_TILE), ("LMONO_LEAD_FULL", self.OPT_LEAD_FULL),       # A/B switches for measurements
                         ("LMONO_ODOM_STREAMS", self.OPT_ODOM_STREAMS), ("LMONO_BOUNDARY_TOL", self.OPT_BOUNDARY_TOL)):
            if os.environ.get(env) is not None:
                self.L.lmono_set_option(self.h, key, int(os.environ[env]))

    def check(self, rc):
        """rc of a library call, or an LmonoError with the library's message and the C return value in .code."""
        if rc < 0:
            e = LmonoError("lmono error %d: %s" % (rc, self.last_error()))
            e.code = int(rc)
            raise e
        return rc

    def last_error(self):
        return self.L.lmono_last_error(self.h).decode()

    def set_stream(self, raw_stream):
        self.check(self.L.lmono_set_stream(self.h, C.c_void_p(raw_stream)))
        self._own_stream = bool(raw_stream)

    def use_own_stream(self):
        """Run on a non-blocking stream of the library's (two contexts on two host threads then overlap)."""
        self.check(self.L.lmono_use_own_stream(self.h))
        self._own_stream = True

    def synchronize(self):
        self.check(self.L.lmono_synchronize(self.h))

    OPT_CORR_TILE = 0
    OPT_DEFER_EVERY = 1
    OPT_ODOM_STREAMS = 2
    OPT_LEAD_FULL = 3
    OPT_BOUNDARY_TOL = 4
    OPT_BA_CLUSTER = 5
    OPT_LEAD_SEED = 6

    def set_option(self, key, value):
        self.check(self.L.lmono_set_option(self.h, int(key), int(value)))

    def get_option(self, key):
        v = C.c_int(0)
        self.check(self.L.lmono_get_option(self.h, int(key), C.byref(v)))
        return int(v.value)

    def odom_chain_groups(self, n_chains):
        """Chain groups (HIP streams) an odometry call with n_chains chains runs on: the rule of odom_run in lidar_abi.hip."""
        g = max(1, min(8, self.get_option(self.OPT_ODOM_STREAMS)))
        if self.get_option(self.OPT_CORR_TILE) != 3:
            return 1
        if self._own_stream:
            g = min(g, 3)
        while g > 1 and n_chains // g < 32:
            g -= 1
        return g

    def host_alloc(self, nbytes):
        """Pinned host memory from the library (lmono_host_alloc) as a numpy uint8 array; free with host_free(array)."""
        p = self.L.lmono_host_alloc(self.h, int(nbytes))
        if not p:
            raise LmonoError("lmono_host_alloc(%d) failed: %s" % (nbytes, self.last_error()))
        arr = np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(p))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            self.L.lmono_host_free(self.h, C.c_void_p(p))

    def timing_reset(self):
        self.check(self.L.lmono_timing_reset(self.h))

    def timing(self):
        """Summed device ms per kernel group since timing_reset(): dict + call counts."""
        ms = np.zeros(52)
        nr, no = C.c_int(0), C.c_int(0)
        self.check(self.L.lmono_timing_read(self.h, ms.ctypes.data, 52, C.byref(nr), C.byref(no)))
        self.diag = ms[13:].copy()
        names = ["frontend_total", "odometry_total", "k_ring_sort", "k_curvature", "k_select", "k_voxel", "k_compact",
                 "k_grid_build", "k_line_index", "k_correspond", "k_lm_solve", "odometry_launch_pairs", "deferred_features"]
        return dict(zip(names, ms.tolist())), nr.value, no.value

    FACTOR_DIMS = {0: (14, 24, 36, 6, 84), 1: (22, 4, 4, 2, 44), 2: (7, 16, 2, 6, 42), 3: (1, 44, 1, 2, 2)}

    def factor_eval(self, kind, params, consts, info, want_jac=True):
        """Batched Evaluate of one BA factor kind on the GPU (host arrays in / out)."""
        npar, ncon, ninf, nres, njac = self.FACTOR_DIMS[kind]
        params = np.ascontiguousarray(params, np.float64).reshape(-1, npar)
        consts = np.ascontiguousarray(consts, np.float64).reshape(-1, ncon)
        info = np.ascontiguousarray(info, np.float64).reshape(ninf)
        n = len(params)
        r = np.zeros((n, nres)); J = np.zeros((n, njac)) if want_jac else None
        self.check(self.L.lmono_factor_eval(self.h, kind, n, params.ctypes.data, consts.ctypes.data, info.ctypes.data,
                                            r.ctypes.data, J.ctypes.data if want_jac else None))
        return r, J

    def factor_eval_blocks(self, kind, params, consts, info, block_mask, J_init=None):
        """Evaluate with ceres' per-block contract: block_mask [n] uint8, bit k = jacobians[k] != NULL.  J starts as J_init (or NaN) so
        that the caller can see which blocks were written."""
        npar, ncon, ninf, nres, njac = self.FACTOR_DIMS[kind]
        params = np.ascontiguousarray(params, np.float64).reshape(-1, npar)
        consts = np.ascontiguousarray(consts, np.float64).reshape(-1, ncon)
        info = np.ascontiguousarray(info, np.float64).reshape(ninf)
        n = len(params)
        mask = np.ascontiguousarray(block_mask, np.uint8).reshape(n)
        r = np.zeros((n, nres))
        J = np.full((n, njac), np.nan) if J_init is None else np.ascontiguousarray(J_init, np.float64).copy()
        self.check(self.L.lmono_factor_eval_blocks(self.h, kind, n, params.ctypes.data, consts.ctypes.data, info.ctypes.data,
                                                   r.ctypes.data, J.ctypes.data, mask.ctypes.data))
        return r, J

    def factor_eval_d(self, kind, count, params_ptr, consts_ptr, info_ptr, r_ptr, J_ptr=None):
        self.check(self.L.lmono_factor_eval_d(self.h, kind, count, C.c_void_p(params_ptr), C.c_void_p(consts_ptr),
                                              C.c_void_p(info_ptr), C.c_void_p(r_ptr), C.c_void_p(J_ptr or 0)))

    @staticmethod
    def _pack_windows(windows):
        """windows: list of dicts(Rs [n,3,3], Ps [n,3], tlc 4x4, trk_start, trk_off, trk_pts)."""
        W = len(windows)
        Rs = np.zeros((W, 11, 9)); Ps = np.zeros((W, 11, 3))
        for k, w in enumerate(windows):
            n = len(w["Rs"]); Rs[k, :n] = np.asarray(w["Rs"]).reshape(n, 9); Ps[k, :n] = w["Ps"]
        tlc = np.ascontiguousarray([np.asarray(w["tlc"]).ravel() for w in windows], np.float64)
        feat_off = np.concatenate([[0], np.cumsum([len(w["trk_start"]) for w in windows])]).astype(np.int32)
        start = np.ascontiguousarray(np.concatenate([w["trk_start"] for w in windows]), np.int32)
        offs, base = [0], 0
        for w in windows:
            offs.extend((np.asarray(w["trk_off"][1:]) + base).tolist()); base += int(w["trk_off"][-1])
        obs_off = np.array(offs, np.int32)
        pts = np.ascontiguousarray(np.concatenate([np.asarray(w["trk_pts"]).reshape(-1, 2) for w in windows]), np.float64)
        return W, feat_off, Rs, Ps, tlc, start, obs_off, pts

    def triangulate(self, windows, depth, track_cnt=3, window_size=10, weight=1500.0, refine_iters=50):
        W, feat_off, Rs, Ps, tlc, start, obs_off, pts = self._pack_windows(windows)
        d = np.ascontiguousarray(depth, np.float64).copy(); flag = np.zeros(len(d), np.int32)
        self.check(self.L.lmono_triangulate(self.h, W, feat_off.ctypes.data, Rs.ctypes.data, Ps.ctypes.data, tlc.ctypes.data, start.ctypes.data,
                                            obs_off.ctypes.data, pts.ctypes.data, d.ctypes.data, flag.ctypes.data, track_cnt, window_size, weight, refine_iters))
        return d, flag

    def outlier_scores(self, windows, depth, track_cnt=3, weight=1500.0):
        W, feat_off, Rs, Ps, tlc, start, obs_off, pts = self._pack_windows(windows)
        d = np.ascontiguousarray(depth, np.float64); sc = np.zeros(len(d))
        self.check(self.L.lmono_outlier_scores(self.h, W, feat_off.ctypes.data, Rs.ctypes.data, Ps.ctypes.data, tlc.ctypes.data, start.ctypes.data,
                                               obs_off.ctypes.data, pts.ctypes.data, d.ctypes.data, track_cnt, weight, sc.ctypes.data))
        return sc

    def shift_depth(self, back_R0, back_P0, R1, P1, tlc, pt_i, depth):
        a = [np.ascontiguousarray(v, np.float64).ravel() for v in (back_R0, back_P0, R1, P1, tlc)]
        pt = np.ascontiguousarray(pt_i, np.float64).reshape(-1, 2); d = np.ascontiguousarray(depth, np.float64); out = np.zeros(len(d))
        self.check(self.L.lmono_shift_depth(self.h, *[v.ctypes.data for v in a], len(d), pt.ctypes.data, d.ctypes.data, out.ctypes.data))
        return out

    def shift_depth_batch(self, frames, pt_i_list, depth_list):
        """frames: [n][40] (back_R0, back_P0, R1, P1, TLC per window); pt_i_list / depth_list: per window arrays.  Returns the list of shifted depths."""
        fr = np.ascontiguousarray(frames, np.float64).reshape(-1, 40)
        off = np.concatenate([[0], np.cumsum([len(d) for d in depth_list])]).astype(np.int32)
        pt = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in pt_i_list]) if off[-1] else np.zeros((0, 2)), np.float64)
        d = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).ravel() for v in depth_list]) if off[-1] else np.zeros(0), np.float64)
        out = np.zeros(len(d))
        self.check(self.L.lmono_shift_depth_batch(self.h, len(fr), fr.ctypes.data, off.ctypes.data, pt.ctypes.data, d.ctypes.data, out.ctypes.data))
        return [out[off[k]:off[k + 1]] for k in range(len(fr))]

    def debug_bounds(self):
        """(hits, line of the first, byte offset of the first, block of the first) of a -DLMONO_BOUNDS build; raises LmonoError on the product build."""
        out = (C.c_ulonglong * 4)()
        self.check(self.L.lmono_debug_bounds(self.h, out))
        return tuple(int(v) for v in out)

    def marginalize(self, windows):
        """windows: list of dicts(poses [11,7], ex [7], invd [F0], obs_feat, obs_j, pts [O,4], laser01 [24], laser_info, mono_info)."""
        W = len(windows)
        feat_off = np.concatenate([[0], np.cumsum([len(w["invd"]) for w in windows])]).astype(np.int32)
        obs_off = np.concatenate([[0], np.cumsum([len(w["obs_j"]) for w in windows])]).astype(np.int32)
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(w[k], dt).ravel() for w in windows]), dt)      # (a window may have no tracks)
        poses = np.ascontiguousarray([w["poses"] for w in windows], np.float64); ex = np.ascontiguousarray([w["ex"] for w in windows], np.float64)
        invd = cat("invd", np.float64); of = cat("obs_feat", np.int32); oj = cat("obs_j", np.int32); pts = cat("pts", np.float64)
        l01 = np.ascontiguousarray([w["laser01"] for w in windows], np.float64)
        li = np.ascontiguousarray(windows[0]["laser_info"], np.float64); mi = np.ascontiguousarray(windows[0]["mono_info"], np.float64)
        J = np.zeros((W, 66, 66)); r = np.zeros((W, 66)); st = np.zeros(W, np.int32)
        self.check(self.L.lmono_marginalize(self.h, W, feat_off.ctypes.data, obs_off.ctypes.data, poses.ctypes.data, ex.ctypes.data, invd.ctypes.data,
                                            of.ctypes.data, oj.ctypes.data, pts.ctypes.data, l01.ctypes.data, li.ctypes.data, mi.ctypes.data,
                                            J.ctypes.data, r.ctypes.data, st.ctypes.data))
        return J, r, st

    def marg_evaluate(self, lin_J, lin_r, x0, x):
        lin_J = np.ascontiguousarray(lin_J, np.float64); lin_r = np.ascontiguousarray(lin_r, np.float64)
        x0 = np.ascontiguousarray(x0, np.float64); x = np.ascontiguousarray(x, np.float64)
        W = len(lin_r); res = np.zeros((W, 66))
        self.check(self.L.lmono_marg_evaluate(self.h, W, lin_J.ctypes.data, lin_r.ctypes.data, x0.ctypes.data, x.ctypes.data, res.ctypes.data))
        return res

    def marg_second_new(self, lin_J, lin_r, x0, x, drop_block):
        """MARGIN_SECOND_NEW: lin_J [W, n0, n0], lin_r [W, n0], x0 / x [W, nb, 7] -> (J [W, n, n], r [W, n], status [W]), n = n0 - 6."""
        lin_J = np.ascontiguousarray(lin_J, np.float64); lin_r = np.ascontiguousarray(lin_r, np.float64)
        x0 = np.ascontiguousarray(x0, np.float64); x = np.ascontiguousarray(x, np.float64)
        W, nb = x.shape[0], x.shape[1]
        n = 6 * nb - 6
        J = np.zeros((W, n, n)); r = np.zeros((W, n)); st = np.zeros(W, np.int32)
        self.check(self.L.lmono_marg_second_new(self.h, W, nb, int(drop_block), lin_J.ctypes.data, lin_r.ctypes.data, x0.ctypes.data, x.ctypes.data,
                                                J.ctypes.data, r.ctypes.data, st.ctypes.data))
        return J, r, st

    def pose_prefix_d(self, incr_ptr, first, n, poses_ptr):
        self.check(self.L.lmono_pose_prefix_d(self.h, C.c_void_p(incr_ptr), first, n, C.c_void_p(poses_ptr)))

    def pose_rebase_d(self, bases_ptr, n_bases, poses_ptr, n):
        self.check(self.L.lmono_pose_rebase_d(self.h, C.c_void_p(bases_ptr or 0), n_bases, C.c_void_p(poses_ptr), n))

    def voxel_filter(self, clouds, leafs):
        """pcl::VoxelGrid on a list of [n,4] float32 clouds (one leaf size each): list of filtered clouds."""
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in clouds]
        off = np.zeros(len(arrs) + 1, np.int64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        cat = np.concatenate(arrs) if off[-1] > 0 else np.zeros((0, 4), np.float32)
        leaf = np.ascontiguousarray(leafs, np.float32)
        out = np.zeros_like(cat) if len(cat) else np.zeros((1, 4), np.float32)
        oo = np.zeros(len(arrs) + 1, np.int64)
        self.check(self.L.lmono_voxel_filter(self.h, len(arrs), cat.ctypes.data, off.ctypes.data, leaf.ctypes.data, out.ctypes.data, oo.ctypes.data))
        return [out[oo[k]:oo[k + 1]].copy() for k in range(len(arrs))]

    def map_refine(self, corner_maps, surf_maps, corner_stacks, surf_stacks, poses_qt, want_nn=False):
        """Scan-to-map optimisation step of laserMapping for a batch of independent streams: lists of [n,4] float32 clouds
        per stream, poses_qt [n_streams,7] (q xyzw, t) initial guesses.  Returns (poses [n_streams,7], stats
        [n_streams,8], nn [total stack points,5] or None)."""
        ns = len(corner_maps)

        def cat(lst):
            arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in lst]
            off = np.zeros(ns + 1, np.int64)
            off[1:] = np.cumsum([len(a) for a in arrs])
            return (np.concatenate(arrs) if off[-1] > 0 else np.zeros((0, 4), np.float32)), off
        cm, cmo = cat(corner_maps); sm, smo = cat(surf_maps); cs, cso = cat(corner_stacks); ss, sso = cat(surf_stacks)
        poses = np.ascontiguousarray(poses_qt, np.float64).reshape(ns, 7).copy()
        stats = np.zeros((ns, 8), np.int32)
        nn = np.zeros((int(cso[-1] + sso[-1]), 5), np.int32) if want_nn else None
        self.check(self.L.lmono_map_refine(self.h, ns, cm.ctypes.data, cmo.ctypes.data, sm.ctypes.data, smo.ctypes.data,
                                           cs.ctypes.data, cso.ctypes.data, ss.ctypes.data, sso.ctypes.data,
                                           poses.ctypes.data, stats.ctypes.data, nn.ctypes.data if want_nn else None))
        return poses, stats, nn

    def close(self):
        if getattr(self, "h", None):
            for child in list(self._children):
                child.close()
            self.L.lmono_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    """Base of the wrappers that own one library object: registered with the context, which closes its children before itself
    (their destroy calls touch the context's stream); close() is idempotent and safe on a half-constructed object."""

    _destroy = None       # name of the C function that frees the handle

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = None
        ctx._children.add(self)

    def _create(self, fn, *args):
        """self.h = fn(ctx, *args); a null handle raises with the library's reason."""
        self.h = getattr(self.ctx.L, fn)(self.ctx.h, *args)
        if not self.h:
            raise LmonoError("%s failed: %s" % (fn, self.ctx.last_error()))

    def close(self):
        if getattr(self, "h", None):
            getattr(self.ctx.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OdomStream(_Handle):
    """Online laserOdometry (lmono_odom_stream): one scan per step(), the previous scan's features stay on the device."""

    _destroy = "lmono_odom_stream_destroy"

    def __init__(self, ctx, max_points, n_lines=64, min_range=5.0, history=8):
        super().__init__(ctx)
        self._create("lmono_odom_stream_create", int(max_points), int(n_lines), float(min_range), int(history))

    def step(self, xyzi=None, dev_ptr=None, n_points=None, warm_start=None):
        """xyzi: [n,4] float32 host array, or dev_ptr + n_points for a scan resident in HBM.  Returns (incr [7] = q_last_curr xyzw +
        t_last_curr, pose [7] = q_w_curr + t_w_curr, info [8])."""
        incr = np.zeros(7); pose = np.zeros(7); info = np.zeros(8, np.int32)
        use = 0
        if warm_start is not None:
            incr[:] = np.asarray(warm_start, np.float64); use = 1
        if dev_ptr is None:
            xyzi = np.ascontiguousarray(xyzi, np.float32)
            ptr, n, on_dev = xyzi.ctypes.data, len(xyzi), 0
        else:
            ptr, n, on_dev = dev_ptr, int(n_points), 1
        self.ctx.check(self.ctx.L.lmono_odom_step(self.ctx.h, self.h, C.c_void_p(ptr), n, on_dev, use, incr.ctypes.data, incr.ctypes.data + 32,
                                                  pose.ctypes.data, pose.ctypes.data + 32, info.ctypes.data))
        return incr, pose, info

    def scan(self):
        """(raw lmono_scan_batch handle, scan index) of the newest scan, for Mapper.process_raw / cloud()."""
        bh = C.c_void_p(0); sc = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_odom_stream_scan(self.h, C.byref(bh), C.byref(sc)))
        return bh.value, sc.value

    def cloud(self, which, cap):
        bh, sc = self.scan()
        out = np.zeros((max(cap, 1), 4), np.float32)
        n = self.ctx.check(self.ctx.L.lmono_batch_get_cloud(self.ctx.h, C.c_void_p(bh), sc, which, out.ctypes.data, cap))
        return out[:n]


class BoundaryReport(C.Structure):
    """lmono_boundary_report (include/lmono_hip.h)"""
    _fields_ = [("n_chains", C.c_int), ("flagged", C.c_int), ("chains_rerun", C.c_int), ("pairs_rerun", C.c_int), ("rounds", C.c_int),
                ("unresolved", C.c_int), ("tol", C.c_double), ("max_resid", C.c_double), ("repair_ms", C.c_double)]


class ScanBatch(_Handle):
    """Device-resident working set of a batch of scans (lmono_scan_batch)."""

    _destroy = "lmono_batch_destroy"

    def __init__(self, ctx, n_scans_cap, total_points_cap):
        super().__init__(ctx)
        self._create("lmono_batch_create", int(n_scans_cap), int(total_points_cap))
        self.n_scans = 0
        self._keep = None

    def scanreg(self, xyzi_dev_ptr, offsets, n_lines=64, min_range=5.0, keepalive=None):
        """xyzi_dev_ptr: raw device pointer of a [total,4] float32 array resident in HBM."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        self.n_scans = len(offsets) - 1
        self._keep = keepalive
        self.ctx.check(self.ctx.L.lmono_scanreg_batch(self.ctx.h, self.h, C.c_void_p(xyzi_dev_ptr), offsets.ctypes.data,
                                                       self.n_scans, int(n_lines), float(min_range)))

    def scanreg_host(self, xyzi, offsets, n_lines=64, min_range=5.0):
        """xyzi: [total,4] float32 numpy array in host memory (KITTI .bin layout): staged to HBM by the library."""
        xyzi = np.ascontiguousarray(xyzi, np.float32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        self.n_scans = len(offsets) - 1
        self._keep = xyzi
        self.ctx.check(self.ctx.L.lmono_scanreg_batch_h(self.ctx.h, self.h, xyzi.ctypes.data, offsets.ctypes.data,
                                                         self.n_scans, int(n_lines), float(min_range)))

    def stage_host(self, host_ptr, total_points, keepalive=None):
        """Asynchronous H2D of a working set (pinned host memory at raw address host_ptr) into this batch's staging buffer."""
        self._keep = keepalive
        self.ctx.check(self.ctx.L.lmono_batch_stage_h(self.ctx.h, self.h, C.c_void_p(host_ptr), int(total_points)))

    def scanreg_staged(self, offsets, n_lines=64, min_range=5.0):
        offsets = np.ascontiguousarray(offsets, np.int64)
        self.n_scans = len(offsets) - 1
        self.ctx.check(self.ctx.L.lmono_scanreg_batch_staged(self.ctx.h, self.h, offsets.ctypes.data, self.n_scans, int(n_lines), float(min_range)))

    def counts(self):
        out = np.zeros((self.n_scans, 6), np.int32)
        self.ctx.check(self.ctx.L.lmono_batch_counts(self.ctx.h, self.h, out.ctypes.data))
        return out

    def cloud(self, scan, which, cap):
        out = np.zeros((max(cap, 1), 4), np.float32)
        n = self.ctx.check(self.ctx.L.lmono_batch_get_cloud(self.ctx.h, self.h, scan, which, out.ctypes.data, cap))
        return out[:n]

    def curvature(self, scan, cap):
        cv = np.zeros(max(cap, 1), np.float32)
        lb = np.zeros(max(cap, 1), np.int32)
        n = self.ctx.check(self.ctx.L.lmono_batch_get_curvature(self.ctx.h, self.h, scan, cv.ctypes.data, lb.ctypes.data, cap))
        return cv[:n], lb[:n]

    def odometry(self, n_chains=1, lead=0):
        incr = np.zeros((self.n_scans, 7))
        poses = np.zeros((self.n_scans, 7))
        self.ctx.check(self.ctx.L.lmono_odom_batch(self.ctx.h, self.h, n_chains, lead, incr.ctypes.data, poses.ctypes.data))
        return incr, poses

    def odometry_d(self, n_chains, lead, incr_ptr=None, poses_ptr=None):
        self.ctx.check(self.ctx.L.lmono_odom_batch_d(self.ctx.h, self.h, n_chains, lead,
                                                      C.c_void_p(incr_ptr or 0), C.c_void_p(poses_ptr or 0)))

    def odometry_shard_d(self, n_chains, lead, first_owned, incr_ptr=None):
        """Rank-local odometry of a scan-range shard: the first `first_owned` scans of the batch are the previous rank's (lead-in)."""
        self.ctx.check(self.ctx.L.lmono_odom_shard_d(self.ctx.h, self.h, n_chains, lead, int(first_owned), C.c_void_p(incr_ptr or 0)))

    def odometry_shard_main_d(self, n_chains, lead, first_owned, incr_ptr=None):
        """odometry_shard_d without the validation of the rank's inner boundaries: shard_validate (after the exchange of the last
        increments) then validates every boundary of the rank, the external one too, in one set of repair rounds."""
        self.ctx.check(self.ctx.L.lmono_odom_shard_main_d(self.ctx.h, self.h, n_chains, lead, int(first_owned), C.c_void_p(incr_ptr or 0)))

    def shard_validate(self, prev_incr, incr_ptr=None):
        """Checks / repairs chain 0's warm start against the previous rank's last increment (None: the rank owns the sequence's first scan;
        only valid as the deferred validation after odometry_shard_main_d); True when this rank's last increment changed."""
        prev = None if prev_incr is None else np.ascontiguousarray(prev_incr, np.float64).reshape(7)
        ch = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_odom_shard_validate(self.ctx.h, self.h, None if prev is None else prev.ctypes.data, C.c_void_p(incr_ptr or 0), C.byref(ch)))
        return bool(ch.value)

    def boundary_report(self):
        """What the boundary validation of the last odometry call did: dict + per-chain residuals and re-run pair counts."""
        rep = BoundaryReport()
        self.ctx.check(self.ctx.L.lmono_odom_boundary_report(self.ctx.h, self.h, C.byref(rep), None, None, 0))
        n = rep.n_chains
        resid = np.zeros(max(n, 1)); rerun = np.zeros(max(n, 1), np.int32)
        self.ctx.check(self.ctx.L.lmono_odom_boundary_report(self.ctx.h, self.h, C.byref(rep), resid.ctypes.data, rerun.ctypes.data, n))
        d = {k: getattr(rep, k) for k, _ in BoundaryReport._fields_}
        d["resid"] = resid[:n]; d["rerun"] = rerun[:n]
        return d

    def correspond(self, scan, q, t):
        q = np.ascontiguousarray(q, np.float64); t = np.ascontiguousarray(t, np.float64)
        out = np.zeros((MAX_QUERIES, 4), np.int32)
        n = self.ctx.check(self.ctx.L.lmono_odom_correspond(self.ctx.h, self.h, scan, q.ctypes.data, t.ctypes.data, out.ctypes.data, MAX_QUERIES))
        return out[:n]


class BaDesc(C.Structure):
    _fields_ = [("n_windows", C.c_int), ("feat_off", C.c_void_p), ("obs_off", C.c_void_p), ("flags", C.c_void_p),
                ("poses", C.c_void_p), ("ex", C.c_void_p), ("inv_depth", C.c_void_p), ("obs_feat", C.c_void_p),
                ("obs_i", C.c_void_p), ("obs_j", C.c_void_p), ("obs_pts", C.c_void_p), ("laser_consts", C.c_void_p),
                ("prior_T", C.c_void_p), ("laser_info", C.c_void_p), ("mono_info", C.c_void_p), ("prior_w", C.c_void_p)]


class BaBatch(_Handle):
    """Batch of independent BA windows resident in HBM (lmono_ba_batch).  `windows`: list of dicts with the keys of
    tests/ba_cases.make_window (poses [n,7], ex, inv_depth, obs_feat/obs_i/obs_j, obs_pts, laser_consts, prior_T, flags)."""

    _destroy = "lmono_ba_batch_destroy"

    def __init__(self, ctx, windows):
        super().__init__(ctx)
        d = self._desc(windows)
        self._create("lmono_ba_batch_create", C.byref(d))

    def update(self, windows):
        """Load another set of windows into the same device arrays (lmono_ba_batch_update)."""
        d = self._desc(windows)
        self.ctx.check(self.ctx.L.lmono_ba_batch_update(self.ctx.h, self.h, C.byref(d)))

    def _desc(self, windows):
        W = len(windows)
        self.W = W
        self.n_poses = [len(w["poses"]) for w in windows]
        feat_off = np.concatenate([[0], np.cumsum([len(w["inv_depth"]) for w in windows])]).astype(np.int32)
        obs_off = np.concatenate([[0], np.cumsum([len(w["obs_feat"]) for w in windows])]).astype(np.int32)
        flags = np.array([[len(w["poses"]), int(w["use_prior"]), int(w["ex_constant"]), int(w["use_mono"])] for w in windows], np.int32)
        poses = np.zeros((W, 11, 7)); poses[:, :, 6] = 1.0
        laser = np.zeros((W, 10, 24))
        for k, w in enumerate(windows):
            poses[k, :len(w["poses"])] = w["poses"]
            laser[k, :len(w["laser_consts"])] = w["laser_consts"]
        cat = lambda key, dt: np.ascontiguousarray(np.concatenate([np.asarray(w[key], dt).reshape(len(w[key]), -1) for w in windows]).ravel(), dt)
        self._keep = dict(feat_off=feat_off, obs_off=obs_off, flags=flags, poses=poses,
                          ex=np.ascontiguousarray([w["ex"] for w in windows], np.float64), inv_depth=cat("inv_depth", np.float64),
                          obs_feat=cat("obs_feat", np.int32), obs_i=cat("obs_i", np.int32), obs_j=cat("obs_j", np.int32),
                          obs_pts=cat("obs_pts", np.float64), laser=laser,
                          prior=np.ascontiguousarray([np.asarray(w["prior_T"]).ravel() for w in windows], np.float64),
                          li=np.ascontiguousarray(windows[0]["laser_info"], np.float64), mi=np.ascontiguousarray(windows[0]["mono_info"], np.float64),
                          pw=np.ascontiguousarray(windows[0]["prior_w"], np.float64))
        k = self._keep
        d = BaDesc(W, *[k[n].ctypes.data for n in ("feat_off", "obs_off", "flags", "poses", "ex", "inv_depth", "obs_feat", "obs_i",
                                                    "obs_j", "obs_pts", "laser", "prior", "li", "mi", "pw")])
        self.feat_off = feat_off
        return d

    def solve(self, max_iter=30):
        self.ctx.check(self.ctx.L.lmono_ba_solve(self.ctx.h, self.h, max_iter))

    def reset(self):
        self.ctx.check(self.ctx.L.lmono_ba_batch_reset(self.ctx.h, self.h))

    def read(self):
        poses = np.zeros((self.W, 11, 7)); ex = np.zeros((self.W, 7)); invd = np.zeros(int(self.feat_off[-1])); sm = np.zeros((self.W, 6))
        self.ctx.check(self.ctx.L.lmono_ba_batch_read(self.ctx.h, self.h, poses.ctypes.data, ex.ctypes.data, invd.ctypes.data, sm.ctypes.data))
        return poses, ex, invd, sm


class Mapper(_Handle):
    """laserMapping with a device-resident cube map (lmono_mapper_*): process(batch, scan, q_wodom, t_wodom) per frame."""

    _destroy = "lmono_mapper_destroy"

    def __init__(self, ctx, line_res=0.4, plane_res=0.8):
        super().__init__(ctx)
        self._create("lmono_mapper_create", line_res, plane_res)

    def process(self, batch, scan, q_wodom, t_wodom):
        q = np.ascontiguousarray(q_wodom, np.float64); t = np.ascontiguousarray(t_wodom, np.float64)
        qo = np.zeros(4); to = np.zeros(3); st = np.zeros(8, np.int32)
        self.ctx.check(self.ctx.L.lmono_mapper_process(self.ctx.h, self.h, batch.h, int(scan), q.ctypes.data, t.ctypes.data,
                                                       qo.ctypes.data, to.ctypes.data, st.ctypes.data))
        return qo, to, st

    def reset(self):
        self.ctx.check(self.ctx.L.lmono_mapper_reset(self.ctx.h, self.h))

    @staticmethod
    def process_batch(ctx, mappers, batches, scans, q_wodom, t_wodom):
        """One frame of several independent streams in one call: lists of Mapper / ScanBatch, scans [n], q_wodom [n,4],
        t_wodom [n,3].  Returns (q [n,4], t [n,3], stats [n,8])."""
        n = len(mappers)
        mh = (C.c_void_p * n)(*[m.h for m in mappers]); bh = (C.c_void_p * n)(*[b.h for b in batches])
        sc = np.ascontiguousarray(scans, np.int32)
        q = np.ascontiguousarray(q_wodom, np.float64).reshape(n, 4); t = np.ascontiguousarray(t_wodom, np.float64).reshape(n, 3)
        qo = np.zeros((n, 4)); to = np.zeros((n, 3)); st = np.zeros((n, 8), np.int32)
        ctx.check(ctx.L.lmono_mapper_process_batch(ctx.h, n, mh, bh, sc.ctypes.data, q.ctypes.data, t.ctypes.data, qo.ctypes.data, to.ctypes.data, st.ctypes.data))
        return qo, to, st

    def cube(self, which, i, j, k):
        n = self.ctx.L.lmono_mapper_cube(self.ctx.h, self.h, which, i, j, k, None, 0)
        self.ctx.check(min(n, 0))
        out = np.zeros((max(n, 1), 4), np.float32)
        if n > 0:
            self.ctx.check(min(self.ctx.L.lmono_mapper_cube(self.ctx.h, self.h, which, i, j, k, out.ctypes.data, n), 0))
        return out[:n]


class Camera(C.Structure):
    """lmono_camera: PINHOLE intrinsics of the cam yaml + kernel_size / kernel_type / blur_type of the map config."""
    _fields_ = [("width", C.c_int), ("height", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double),
                ("kernel_size", C.c_int), ("kernel_type", C.c_int), ("blur_type", C.c_int)]


POINT_RGB = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("bgra", np.uint32)])


def lidar_to_camera(rlc, tlc):
    """The 4 x 4 of map_build_node.cc:216-220: [rlc^T | -rlc^T tlc]."""
    rlc = np.asarray(rlc, np.float64).reshape(3, 3); tlc = np.asarray(tlc, np.float64).reshape(3)
    M = np.eye(4)
    M[:3, :3] = rlc.T
    M[:3, 3] = (-1.0 * rlc.T) @ tlc
    return M


class MapBuilder(_Handle):
    """MapBuilder::associateToMap / depthFill / rgb_map accumulation on the device (lmono_map_builder_*)."""

    _destroy = "lmono_map_builder_destroy"

    def __init__(self, ctx, camera, max_cloud_points=1 << 18, map_capacity_points=None):
        super().__init__(ctx)
        self.cam = camera
        if map_capacity_points is None:
            map_capacity_points = 10 * camera.width * camera.height      # processMapping flushes every 10 frames
        self._create("lmono_map_builder_create", C.byref(camera), int(max_cloud_points), int(map_capacity_points))

    def associate(self, xyzi, transform, bgr, q_wc, t_wc):
        """One associateToMap on host buffers; returns the size of the coloured cloud."""
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4); M = np.ascontiguousarray(transform, np.float64).reshape(16)
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.shape != (self.cam.height, self.cam.width, 3):
            raise LmonoError("image must be [height][width][3] uint8")
        q = np.ascontiguousarray(q_wc, np.float64).reshape(4); t = np.ascontiguousarray(t_wc, np.float64).reshape(3)
        n = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_associate_to_map(self.ctx.h, self.h, xyzi.ctypes.data, len(xyzi), M.ctypes.data, bgr.ctypes.data,
                                                         q.ctypes.data, t.ctypes.data, C.addressof(n)))
        return n.value

    @staticmethod
    def associate_batch(ctx, builders, xyzi_ptrs, n_points, transforms, bgr_ptrs, q_wc, t_wc):
        """One frame of several independent builders; xyzi_ptrs / bgr_ptrs are device pointers (ints).  Returns sizes [n]."""
        n = len(builders)
        mh = (C.c_void_p * n)(*[b.h for b in builders])
        xp = (C.c_void_p * n)(*[int(p) for p in xyzi_ptrs]); bp = (C.c_void_p * n)(*[int(p) for p in bgr_ptrs])
        npt = np.ascontiguousarray(n_points, np.int32)
        M = np.ascontiguousarray(transforms, np.float64).reshape(n, 16)
        q = np.ascontiguousarray(q_wc, np.float64).reshape(n, 4); t = np.ascontiguousarray(t_wc, np.float64).reshape(n, 3)
        out = np.zeros(n, np.int32)
        ctx.check(ctx.L.lmono_associate_to_map_batch(ctx.h, n, mh, xp, npt.ctypes.data, M.ctypes.data, bp, q.ctypes.data, t.ctypes.data, out.ctypes.data))
        return out

    def depth(self):
        d = np.zeros((self.cam.height, self.cam.width), np.uint8)
        self.ctx.check(self.ctx.L.lmono_map_builder_depth(self.ctx.h, self.h, d.ctypes.data))
        return d

    def cloud(self, which=0):
        n = self.ctx.L.lmono_map_builder_cloud(self.ctx.h, self.h, which, None, 0)
        self.ctx.check(min(n, 0))
        out = np.zeros(max(n, 1), POINT_RGB)
        self.ctx.check(min(self.ctx.L.lmono_map_builder_cloud(self.ctx.h, self.h, which, out.ctypes.data, n), 0))
        return out[:n]

    def map(self):
        n = self.ctx.L.lmono_map_builder_map(self.ctx.h, self.h, None, 0)
        self.ctx.check(min(n, 0))
        out = np.zeros(max(n, 1), POINT_RGB)
        self.ctx.check(min(self.ctx.L.lmono_map_builder_map(self.ctx.h, self.h, out.ctypes.data, n), 0))
        return out[:n]

    def clear(self):
        self.ctx.check(self.ctx.L.lmono_map_builder_clear(self.ctx.h, self.h))


VoxelCapacity = collections.namedtuple("VoxelCapacity", "max_voxels slots grow_limit rehashes")


class VoxelMap(_Handle):
    """The voxel-grid global colour map on the device (lmono_voxel_map_*): clouds of POINT_RGB folded in frame by frame,
    bounded by the number of occupied voxels, the same bytes for every insertion order.  insert* return the call's stats
    [points inserted, points rejected, voxels new, voxels afterwards]; an LmonoError carries the C return value in .code.
    The size is fixed at max_voxels unless grow_limit (> 0) lets refused inserts double it up to that limit; reserve / shrink_to_fit
    rebuild the table for another size with the content unchanged, and make a full map usable again."""

    _destroy = "lmono_voxel_map_destroy"

    def __init__(self, ctx, leaf=0.1, max_voxels=1 << 22, grow_limit=0):
        super().__init__(ctx)
        self.leaf = float(np.float32(leaf))
        self.TILE = int(ctx.L.lmono_voxel_map_tile())       # points a workgroup of the insert sums on chip
        self._create("lmono_voxel_map_create", C.c_float(leaf), int(max_voxels))
        if grow_limit:
            self.set_growth(grow_limit)

    @property
    def capacity(self):
        """max_voxels, slots (64 B each), grow_limit (0: fixed size), rehashes (tables replaced so far)."""
        out = np.zeros(4, np.int64)
        self.ctx.check(self.ctx.L.lmono_voxel_map_capacity(self.ctx.h, self.h, out.ctypes.data))
        return VoxelCapacity(*(int(v) for v in out))

    @property
    def max_voxels(self):
        return self.capacity.max_voxels

    def set_growth(self, limit):
        """limit 0: fixed size; else refused inserts and composes rebuild the map for min(limit, 2 * max_voxels) and go in again."""
        self.ctx.check(self.ctx.L.lmono_voxel_map_set_growth(self.ctx.h, self.h, int(limit)))

    def reserve(self, max_voxels):
        """Rebuild the table for max_voxels (>= size) voxels, content unchanged; a full map is usable again."""
        VoxelMap.reserve_batch([self], [max_voxels])

    @staticmethod
    def reserve_batch(maps, max_voxels):
        """reserve for several maps: one clear launch and one rehash launch in all."""
        n = len(maps)
        if n == 0 or len(max_voxels) != n:
            raise LmonoError("one max_voxels per map")
        ctx = maps[0].ctx
        mh = (C.c_void_p * n)(*[m.h for m in maps])
        mv = np.array([int(v) for v in max_voxels], np.int64)
        ctx.check(ctx.L.lmono_voxel_map_reserve(ctx.h, n, mh, mv.ctypes.data))

    def shrink_to_fit(self):
        self.reserve(max(self.size, 1))

    def insert(self, points, bgra=None):
        """points: a POINT_RGB array, or xyz [n][3] float32 with bgra [n] uint32."""
        if bgra is not None:
            xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            p = np.zeros(len(xyz), POINT_RGB)
            p["x"] = xyz[:, 0]; p["y"] = xyz[:, 1]; p["z"] = xyz[:, 2]; p["bgra"] = np.asarray(bgra, np.uint32).reshape(-1)
        else:
            p = np.ascontiguousarray(points)
            if p.dtype != POINT_RGB:
                raise LmonoError("points must be a POINT_RGB array (or xyz float32 with bgra uint32)")
        stats = np.zeros(4, np.int64)
        self.ctx.check(self.ctx.L.lmono_voxel_map_insert(self.ctx.h, self.h, p.ctypes.data if len(p) else None, len(p), stats.ctypes.data))
        return stats

    def insert_d(self, ptr, n):
        """n lmono_point_rgb records in device memory."""
        stats = np.zeros(4, np.int64)
        self.ctx.check(self.ctx.L.lmono_voxel_map_insert_d(self.ctx.h, self.h, C.c_void_p(int(ptr)), int(n), stats.ctypes.data))
        return stats

    def insert_frame(self, builder):
        """The world-frame cloud of a MapBuilder's last frame, straight from its device memory."""
        return VoxelMap.insert_frames(self.ctx, [self], [builder])[0]

    @staticmethod
    def insert_frames(ctx, maps, builders):
        """One frame of several builders into as many maps, two launches in all; returns stats [n][4]."""
        n = len(maps)
        if len(builders) != n:
            raise LmonoError("one builder per map")
        mh = (C.c_void_p * n)(*[m.h for m in maps]); bh = (C.c_void_p * n)(*[b.h for b in builders])
        stats = np.zeros((n, 4), np.int64)
        ctx.check(ctx.L.lmono_voxel_map_insert_frames(ctx.h, n, mh, bh, stats.ctypes.data))
        return stats

    @property
    def size(self):
        return int(self.ctx.check(self.ctx.L.lmono_voxel_map_size(self.ctx.h, self.h)))

    def read(self):
        """One POINT_RGB per voxel, ascending key order (z-major, then y, then x)."""
        n = self.size
        out = np.zeros(max(n, 1), POINT_RGB)
        self.ctx.check(self.ctx.L.lmono_voxel_map_read(self.ctx.h, self.h, out.ctypes.data, n))
        return out[:n]

    def cells(self):
        """Diagnostic view: keys [n] uint64 ascending, counts [n] uint32, sums [n][6] uint64 (offsets x y z, colour r g b)."""
        n = self.size
        keys = np.zeros(max(n, 1), np.uint64); counts = np.zeros(max(n, 1), np.uint32); sums = np.zeros((max(n, 1), 6), np.uint64)
        self.ctx.check(self.ctx.L.lmono_voxel_map_cells(self.ctx.h, self.h, keys.ctypes.data, counts.ctypes.data, sums.ctypes.data, n))
        return keys[:n], counts[:n], sums[:n]

    @staticmethod
    def insert_filtered(maps, filters):
        """The last output of each OutlierFilter into its map, from device memory: the two insert launches and the capacity rules of
        insert_frames; returns stats [n][4]."""
        n = len(maps)
        if n == 0 or len(filters) != n:
            raise LmonoError("one filter per map")
        ctx = maps[0].ctx
        mh = (C.c_void_p * n)(*[m.h for m in maps]); fh = (C.c_void_p * n)(*[f.h for f in filters])
        stats = np.zeros((n, 4), np.int64)
        ctx.check(ctx.L.lmono_voxel_map_insert_filtered(ctx.h, n, mh, fh, stats.ctypes.data))
        return stats

    @staticmethod
    def insert_aligned(maps, aligners):
        """The aligned cloud of each CloudAligner's last align into its map, from device memory: the two insert launches and the capacity
        rules of insert_frames; returns stats [n][4]."""
        n = len(maps)
        if n == 0 or len(aligners) != n:
            raise LmonoError("one aligner per map")
        ctx = maps[0].ctx
        mh = (C.c_void_p * n)(*[m.h for m in maps]); ah = (C.c_void_p * n)(*[a.h for a in aligners])
        stats = np.zeros((n, 4), np.int64)
        ctx.check(ctx.L.lmono_voxel_map_insert_aligned(ctx.h, n, mh, ah, stats.ctypes.data))
        return stats

    def compose(self, sources, transforms, stats=False):
        """Fold the voxel maps `sources`, each moved by its rigid transform ([n][12] or [n][3][4] float64, row-major 3 x 4, applied as given),
        into this map (lmono_voxel_map_compose): every source voxel with its count as weight.  All or nothing; the sources are
        not modified.  With stats=True returns [source voxels moved, source voxels rejected, points moved, points rejected, voxels new,
        voxels afterwards]."""
        n = len(sources)
        t = np.ascontiguousarray(transforms, np.float64).reshape(-1)
        if t.size != 12 * n:
            raise LmonoError("one 3 x 4 transform per source")
        sh = (C.c_void_p * max(n, 1))(*[s.h for s in sources])
        st = np.zeros(6, np.int64)
        self.ctx.check(self.ctx.L.lmono_voxel_map_compose(self.ctx.h, self.h, n, sh, t.ctypes.data if n else None, st.ctypes.data))
        return st if stats else None

    def clear(self):
        self.ctx.check(self.ctx.L.lmono_voxel_map_clear(self.ctx.h, self.h))


def _pose_matrix(tq):
    """[R | t] of a pose (x y z, qx qy qz qw) in fp64; the quaternion is normalised first."""
    tq = np.asarray(tq, np.float64).reshape(7)
    x, y, z, w = tq[3:] / np.sqrt((tq[3:] * tq[3:]).sum())
    R = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                  [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                  [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]], np.float64)
    return R, tq[:3].copy()


def pose_delta(inserted_tq, corrected_tq):
    """The rigid transform that carries what was mapped under the pose `inserted_tq` to where the pose `corrected_tq` puts it:
    D = T_corrected * T_inserted^-1, as [12] float64 (row-major 3 x 4), for VoxelMap.compose.  Poses are (x y z, qx qy qz qw).  With
    q / |q| = (x, y, z, w) and
        R(q) = [[1 - 2(yy + zz), 2(xy - zw), 2(xz + yw)], [2(xy + zw), 1 - 2(xx + zz), 2(yz - xw)], [2(xz - yw), 2(yz + xw), 1 - 2(xx + yy)]]
    the result is D_R = R_c R_i^T (element [a][b] = (R_c[a][0] R_i[b][0] + R_c[a][1] R_i[b][1]) + R_c[a][2] R_i[b][2]) and
    D_t = t_c - D_R t_i (element a = t_c[a] - ((D_R[a][0] t_i[0] + D_R[a][1] t_i[1]) + D_R[a][2] t_i[2])), all in numpy fp64."""
    Ri, ti = _pose_matrix(inserted_tq)
    Rc, tc = _pose_matrix(corrected_tq)
    D = np.zeros((3, 4), np.float64)
    for a in range(3):
        for b in range(3):
            D[a, b] = (Rc[a, 0] * Ri[b, 0] + Rc[a, 1] * Ri[b, 1]) + Rc[a, 2] * Ri[b, 2]
        D[a, 3] = tc[a] - ((D[a, 0] * ti[0] + D[a, 1] * ti[1]) + D[a, 2] * ti[2])
    return D.reshape(12)


class SubmapAtlas:
    """A sequence as submaps, so that the global map can follow a corrected trajectory: every `frames_per_submap` frames go
    into a voxel map of their own (leaf_sub), anchored at the pose of its first frame.  compose(dst, corrected poses) moves every submap
    rigidly by pose_delta(anchor pose, corrected anchor pose) and folds them into dst in one lmono_voxel_map_compose call.
    With grow_limit_sub the submaps start at max_voxels_sub and grow up to that limit; with compact_closed a submap is shrunk to what it holds
    when the next one is opened (the last one at compose), so a closed submap's table is as small as its content allows."""

    def __init__(self, ctx, frames_per_submap, leaf_sub=0.05, max_voxels_sub=1 << 20, grow_limit_sub=0, compact_closed=False):
        if int(frames_per_submap) < 1:
            raise LmonoError("frames_per_submap must be >= 1")
        self.ctx = ctx
        self.frames_per_submap = int(frames_per_submap)
        self.leaf_sub = float(leaf_sub)
        self.max_voxels_sub = int(max_voxels_sub)
        self.grow_limit_sub = int(grow_limit_sub)
        self.compact_closed = bool(compact_closed)
        self._compacted = 0                                  # submaps[:_compacted] have been shrunk to fit
        self.submaps = []
        self.anchor_frames = []
        self.anchor_poses = []
        self.n_frames = 0

    @property
    def anchors(self):
        """Frame indices [m] int64 and poses [m][7] float64 (as inserted) of the submaps' first frames."""
        return np.array(self.anchor_frames, np.int64), np.array(self.anchor_poses, np.float64).reshape(-1, 7)

    def insert_frame(self, source, pose_tq):
        """One frame, already in the world frame of `pose_tq` (x y z, qx qy qz qw): the last frame of a MapBuilder, the last output of an
        OutlierFilter, or a POINT_RGB array.  Returns the insert's stats."""
        pose = np.asarray(pose_tq, np.float64).reshape(7)
        if self.n_frames % self.frames_per_submap == 0:
            self._compact()
            self.submaps.append(VoxelMap(self.ctx, leaf=self.leaf_sub, max_voxels=self.max_voxels_sub, grow_limit=self.grow_limit_sub))
            self.anchor_frames.append(self.n_frames)
            self.anchor_poses.append(pose.copy())
        sub = self.submaps[-1]
        self.n_frames += 1
        if isinstance(source, MapBuilder):
            return sub.insert_frame(source)
        if isinstance(source, OutlierFilter):
            return VoxelMap.insert_filtered([sub], [source])[0]
        return sub.insert(source)

    def _compact(self):
        """Shrink the submaps not yet shrunk (all are closed when this is called) to what they hold: one batched reserve."""
        todo = self.submaps[self._compacted:] if self.compact_closed else []
        if todo:
            VoxelMap.reserve_batch(todo, [max(m.size, 1) for m in todo])
            self._compacted = len(self.submaps)

    def compose(self, dst, corrected_poses_tq, stats=False):
        """corrected_poses_tq: one pose per anchor, or one per frame (the anchors' are taken).  dst: a VoxelMap, usually fresh."""
        P = np.asarray(corrected_poses_tq, np.float64).reshape(-1, 7)
        if len(P) == self.n_frames and self.n_frames != len(self.submaps):
            P = P[np.array(self.anchor_frames, np.int64)]
        if len(P) != len(self.submaps):
            raise LmonoError("corrected poses: one per anchor (%d) or one per frame (%d)" % (len(self.submaps), self.n_frames))
        T = np.array([pose_delta(a, p) for a, p in zip(self.anchor_poses, P)], np.float64).reshape(-1, 12)
        self._compact()
        return dst.compose(self.submaps, T, stats=stats)

    def close(self):
        for s in self.submaps:
            s.close()
        self.submaps = []
        self._compacted = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OutlierFilter(_Handle):
    """Statistical outlier removal on the device, between MapBuilder and VoxelMap (lmono_sor_*).  filter* return the call's
    stats [points in, rejected, isolated, scored, kept, A, Bhi, Blo]; the kept points stay on the device for VoxelMap.insert_filtered and
    come to the host with cloud().  An LmonoError carries the C return value in .code."""

    _destroy = "lmono_sor_destroy"

    def __init__(self, ctx, max_points, mean_k=100, stddev_mul=1.0, cell=0.1, max_rings=8):
        super().__init__(ctx)
        self.max_points = int(max_points)
        self.stats = np.zeros(8, np.int64)
        self._create("lmono_sor_create", int(max_points), int(mean_k), C.c_double(stddev_mul), C.c_float(cell), int(max_rings))

    def filter(self, points):
        """points: a POINT_RGB array on the host."""
        p = np.ascontiguousarray(points)
        if p.dtype != POINT_RGB:
            raise LmonoError("points must be a POINT_RGB array")
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_sor_filter(self.ctx.h, self.h, p.ctypes.data if len(p) else None, len(p), stats.ctypes.data))
        self.stats = stats
        return stats

    def filter_d(self, ptr, n):
        """n lmono_point_rgb records in device memory."""
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_sor_filter_d(self.ctx.h, self.h, C.c_void_p(int(ptr)), int(n), stats.ctypes.data))
        self.stats = stats
        return stats

    @staticmethod
    def filter_frames(filters, builders):
        """The world-frame cloud of each builder's last frame through its filter, one launch per phase for all; returns stats [n][8]."""
        n = len(filters)
        if n == 0 or len(builders) != n:
            raise LmonoError("one builder per filter")
        ctx = filters[0].ctx
        fh = (C.c_void_p * n)(*[f.h for f in filters]); bh = (C.c_void_p * n)(*[b.h for b in builders])
        stats = np.zeros((n, 8), np.int64)
        ctx.check(ctx.L.lmono_sor_filter_frames(ctx.h, n, fh, bh, stats.ctypes.data))
        for f, s in zip(filters, stats):
            f.stats = s.copy()
        return stats

    def cloud(self):
        """The kept points of the last call, in input order."""
        n = int(self.ctx.check(self.ctx.L.lmono_sor_cloud(self.ctx.h, self.h, None, 0)))
        out = np.zeros(max(n, 1), POINT_RGB)
        self.ctx.check(self.ctx.L.lmono_sor_cloud(self.ctx.h, self.h, out.ctypes.data, n))
        return out[:n]

    def scores(self):
        """Diagnostic view of the last call, per input point: keep [n] uint8 and v [n] uint32 (0xffffffff: isolated or rejected)."""
        n = int(self.ctx.check(self.ctx.L.lmono_sor_scores(self.ctx.h, self.h, None, None, 0)))
        keep = np.zeros(max(n, 1), np.uint8); v = np.zeros(max(n, 1), np.uint32)
        self.ctx.check(self.ctx.L.lmono_sor_scores(self.ctx.h, self.h, keep.ctypes.data, v.ctypes.data, n))
        return keep[:n], v[:n]

    def threshold(self):
        """mean, sqrt(var), thr of the last call in v units (2^-16 m, summed over the mean_k distances)."""
        out = np.zeros(3, np.float64)
        self.ctx.check(self.ctx.L.lmono_sor_threshold(self.ctx.h, self.h, out.ctypes.data))
        return out

    def diag(self):
        """Measurement view of the last call: rings scanned summed over the valid points, points scored by the radix select."""
        out = np.zeros(2, np.int64)
        self.ctx.check(self.ctx.L.lmono_sor_diag(self.ctx.h, self.h, out.ctypes.data))
        return out


class CloudAligner(_Handle):
    """Point-to-point ICP of a cloud against a target on the device, between OutlierFilter and VoxelMap (lmono_icp_*).  A target is
    set once (a POINT_RGB array, device memory, a VoxelMap, or the last aligned cloud) and serves every align until the next one.  align* return the
    call's stats [source points, not usable, target points, rejected, iterations, status, pairs, E of the last iteration]; the aligned cloud
    stays on the device for VoxelMap.insert_aligned and comes to the host with cloud().  cell and max_rings tune the search grid and change no
    result (defaults: lmono_icp_default_cell(max_corr), which is max_corr / 1.75 or an ulp or two above it, and 2).  An LmonoError carries the C return value in .code."""

    _destroy = "lmono_icp_destroy"

    def __init__(self, ctx, max_source_points, max_target_points, max_corr=0.5, max_iter=50, eps=1e-8, mse_eps=0.0, cell=None, max_rings=2):
        super().__init__(ctx)
        self.max_source_points = int(max_source_points)
        self.max_target_points = int(max_target_points)
        self.stats = np.zeros(8, np.int64)
        if cell is None:
            cell = ctx.L.lmono_icp_default_cell(C.c_float(max_corr))   # the smallest cell >= max_corr / 1.75 that 2 rings cover max_corr with
        self._create("lmono_icp_create", int(max_source_points), int(max_target_points), C.c_float(max_corr), int(max_iter), C.c_double(eps),
                     C.c_double(mse_eps), C.c_float(cell), int(max_rings))

    @staticmethod
    def _points(points):
        p = np.ascontiguousarray(points)
        if p.dtype != POINT_RGB:
            raise LmonoError("points must be a POINT_RGB array")
        return p

    def set_guess(self, g=None):
        """g: [12] or [3][4] float64, row-major 3 x 4, applied to the source before the first iteration; None: identity."""
        if g is None:
            self.ctx.check(self.ctx.L.lmono_icp_set_guess(self.ctx.h, self.h, None))
            return
        g = np.ascontiguousarray(g, np.float64).reshape(-1)
        if g.size != 12:
            raise LmonoError("the guess is a 3 x 4 transform")
        self.ctx.check(self.ctx.L.lmono_icp_set_guess(self.ctx.h, self.h, g.ctypes.data))

    def set_poll_interval(self, pairs):
        """Launch pairs between two reads of the done words; changes no result."""
        self.ctx.check(self.ctx.L.lmono_icp_set_poll_interval(self.ctx.h, self.h, int(pairs)))

    def set_target(self, points):
        p = self._points(points)
        self.ctx.check(self.ctx.L.lmono_icp_set_target(self.ctx.h, self.h, p.ctypes.data if len(p) else None, len(p)))

    def set_target_d(self, ptr, n):
        """n lmono_point_rgb records in device memory."""
        self.ctx.check(self.ctx.L.lmono_icp_set_target_d(self.ctx.h, self.h, C.c_void_p(int(ptr)), int(n)))

    def set_target_map(self, voxel_map):
        """One point per occupied voxel of a VoxelMap (what read() gives), without a host copy."""
        self.ctx.check(self.ctx.L.lmono_icp_set_target_map(self.ctx.h, self.h, voxel_map.h))

    def set_target_aligned(self):
        """The aligned cloud of the last align becomes the target."""
        self.ctx.check(self.ctx.L.lmono_icp_set_target_aligned(self.ctx.h, self.h))

    def align(self, points):
        """points: a POINT_RGB array on the host."""
        p = self._points(points)
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_icp_align(self.ctx.h, self.h, p.ctypes.data if len(p) else None, len(p), stats.ctypes.data))
        self.stats = stats
        return stats

    def align_d(self, ptr, n):
        """n lmono_point_rgb records in device memory."""
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_icp_align_d(self.ctx.h, self.h, C.c_void_p(int(ptr)), int(n), stats.ctypes.data))
        self.stats = stats
        return stats

    @staticmethod
    def _batch(fn, aligners, others, what):
        n = len(aligners)
        if n == 0 or len(others) != n:
            raise LmonoError("one %s per aligner" % what)
        ctx = aligners[0].ctx
        ah = (C.c_void_p * n)(*[a.h for a in aligners]); oh = (C.c_void_p * n)(*[o.h for o in others])
        stats = np.zeros((n, 8), np.int64)
        ctx.check(getattr(ctx.L, fn)(ctx.h, n, ah, oh, stats.ctypes.data))
        for a, s in zip(aligners, stats):
            a.stats = s.copy()
        return stats

    @staticmethod
    def align_frames(aligners, builders):
        """The world-frame cloud of each builder's last frame against its aligner's target, one launch per phase for all; returns stats [n][8]."""
        return CloudAligner._batch("lmono_icp_align_frames", aligners, builders, "builder")

    @staticmethod
    def align_filtered(aligners, filters):
        """The last output of each OutlierFilter against its aligner's target; returns stats [n][8]."""
        return CloudAligner._batch("lmono_icp_align_filtered", aligners, filters, "filter")

    def transform(self):
        """[3][4] float64 of the last align, the guess included: what VoxelMap.compose takes."""
        out = np.zeros(12, np.float64)
        self.ctx.check(self.ctx.L.lmono_icp_transform(self.ctx.h, self.h, out.ctypes.data))
        return out.reshape(3, 4)

    def cloud(self):
        """Every input point of the last align in input order, moved by its result; the payload is untouched."""
        n = int(self.ctx.check(self.ctx.L.lmono_icp_cloud(self.ctx.h, self.h, None, 0)))
        out = np.zeros(max(n, 1), POINT_RGB)
        self.ctx.check(self.ctx.L.lmono_icp_cloud(self.ctx.h, self.h, out.ctypes.data, n))
        return out[:n]

    def history(self):
        """(pairs, E) [k][2] int64 of every iteration of the last align."""
        n = int(self.ctx.check(self.ctx.L.lmono_icp_history(self.ctx.h, self.h, None, 0)))
        out = np.zeros((max(n, 1), 2), np.int64)
        self.ctx.check(self.ctx.L.lmono_icp_history(self.ctx.h, self.h, out.ctypes.data, n))
        return out[:n]

    def distances(self):
        """The last iteration's squared distance per source point, float32; +inf where the point is unmatched."""
        n = int(self.ctx.check(self.ctx.L.lmono_icp_distances(self.ctx.h, self.h, None, 0)))
        out = np.zeros(max(n, 1), np.float32)
        self.ctx.check(self.ctx.L.lmono_icp_distances(self.ctx.h, self.h, out.ctypes.data, n))
        return out[:n]


NORMAL = np.dtype([("nx", np.float32), ("ny", np.float32), ("nz", np.float32), ("curvature", np.float32)])


class SurfaceNormals(_Handle):
    """Surface normals and curvature of a cloud on the device (lmono_normals_*): per point the unit eigenvector of the smallest
    eigenvalue of its neighbours' scatter matrix within radius, facing the viewpoint (without one: its largest component positive), and that
    eigenvalue over the trace.  compute* return the call's stats [points in, rejected, with a normal, without, sum of the neighbour counts, largest
    count, 0, 0]; read() gives (records, counts) in input order, NaN records where a point is rejected or has fewer than min_neighbours
    neighbours; cloud() the points they belong to.  cell and max_rings tune the search grid and change no result (defaults:
    lmono_normals_default_cell(radius) and 2).  An LmonoError carries the C return value in .code."""

    _destroy = "lmono_normals_destroy"

    def __init__(self, ctx, max_points, radius=0.05, min_neighbours=3, cell=None, max_rings=2):
        super().__init__(ctx)
        self.max_points = int(max_points)
        self.stats = np.zeros(8, np.int64)
        if cell is None:
            cell = ctx.L.lmono_normals_default_cell(C.c_float(radius))
        self._create("lmono_normals_create", int(max_points), C.c_float(radius), int(min_neighbours), C.c_float(cell), int(max_rings))

    @staticmethod
    def _viewpoints(v, n):
        """-> (float32 array or None, its address or None); the array must outlive the call."""
        if v is None:
            return None, None
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        if v.size != 3 * n:
            raise LmonoError("a viewpoint is three floats per stream")
        return v, v.ctypes.data

    def compute(self, points, viewpoint=None):
        """points: a POINT_RGB array on the host."""
        p = CloudAligner._points(points)
        v, vp = self._viewpoints(viewpoint, 1)
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_normals_compute(self.ctx.h, self.h, p.ctypes.data if len(p) else None, len(p), vp, stats.ctypes.data))
        self.stats = stats
        return stats

    def compute_d(self, ptr, n, viewpoint=None):
        """n lmono_point_rgb records in device memory."""
        v, vp = self._viewpoints(viewpoint, 1)
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_normals_compute_d(self.ctx.h, self.h, C.c_void_p(int(ptr)), int(n), vp, stats.ctypes.data))
        self.stats = stats
        return stats

    @staticmethod
    def compute_frames(normals, builders, viewpoints=None):
        """The world-frame cloud of each builder's last frame, one launch per phase for all; viewpoints: [n][3] or None; returns stats [n][8]."""
        n = len(normals)
        if n == 0 or len(builders) != n:
            raise LmonoError("one builder per SurfaceNormals")
        ctx = normals[0].ctx
        v, vp = SurfaceNormals._viewpoints(viewpoints, n)
        nh = (C.c_void_p * n)(*[a.h for a in normals]); bh = (C.c_void_p * n)(*[b.h for b in builders])
        stats = np.zeros((n, 8), np.int64)
        ctx.check(ctx.L.lmono_normals_compute_frames(ctx.h, n, nh, bh, vp, stats.ctypes.data))
        for a, s in zip(normals, stats):
            a.stats = s.copy()
        return stats

    def compute_map(self, voxel_map, viewpoint=None):
        """One point per occupied voxel of a VoxelMap (what read() gives, in the device's order: see cloud()), without a host copy."""
        v, vp = self._viewpoints(viewpoint, 1)
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_normals_compute_map(self.ctx.h, self.h, voxel_map.h, vp, stats.ctypes.data))
        self.stats = stats
        return stats

    def read(self):
        """(records [n] NORMAL, counts [n] uint32) of the last compute, in input order."""
        n = int(self.ctx.check(self.ctx.L.lmono_normals_read(self.ctx.h, self.h, None, None, 0)))
        rec = np.zeros(max(n, 1), NORMAL); cnt = np.zeros(max(n, 1), np.uint32)
        self.ctx.check(self.ctx.L.lmono_normals_read(self.ctx.h, self.h, rec.ctypes.data, cnt.ctypes.data, n))
        return rec[:n], cnt[:n]

    def cloud(self):
        """The points the records of the last compute belong to, in input order."""
        n = int(self.ctx.check(self.ctx.L.lmono_normals_cloud(self.ctx.h, self.h, None, 0)))
        out = np.zeros(max(n, 1), POINT_RGB)
        self.ctx.check(self.ctx.L.lmono_normals_cloud(self.ctx.h, self.h, out.ctypes.data, n))
        return out[:n]


class FpfhDescriptors(_Handle):
    """FPFH descriptors at keypoints on the device (lmono_fpfh_*): the surface is the cloud of a SurfaceNormals after a
    compute, read with its records in device memory; the keypoints are [m][3] float32 positions, not necessarily points of the cloud
    (VoxelMap.read() at a coarse leaf gives serviceable ones).  compute* return the call's stats [keypoints in, with a descriptor,
    without, surface points with an SPFH, sum of their pair counts, largest pair count, sum of the keypoints' contributing points,
    largest]; read() gives (descriptors [m][33] float32, contributing points [m] uint32, flags [m] uint32) in keypoint order, 33 zeros
    and flag 0 where no surface point contributed.  cell and max_rings tune the search grid and change no result (defaults:
    lmono_fpfh_default_cell(radius) and 2).  An LmonoError carries the C return value in .code."""

    _destroy = "lmono_fpfh_destroy"

    def __init__(self, ctx, max_points, max_keypoints, radius=0.05, cell=None, max_rings=2):
        super().__init__(ctx)
        self.max_points, self.max_keypoints = int(max_points), int(max_keypoints)
        self.stats = np.zeros(8, np.int64)
        if cell is None:
            cell = ctx.L.lmono_fpfh_default_cell(C.c_float(radius))
        self._create("lmono_fpfh_create", int(max_points), int(max_keypoints), C.c_float(radius), C.c_float(cell), int(max_rings))

    @staticmethod
    def _keypoints(k):
        k = np.ascontiguousarray(k, np.float32)
        if k.size % 3:
            raise LmonoError("a keypoint is three floats")
        return k.reshape(-1, 3)

    def compute(self, normals, keypoints):
        k = self._keypoints(keypoints)
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_fpfh_compute(self.ctx.h, self.h, normals.h, k.ctypes.data if len(k) else None, len(k), stats.ctypes.data))
        self.stats = stats
        return stats

    @staticmethod
    def compute_batch(fpfhs, normals, keypoints):
        """One launch per phase for all streams; normals may name one SurfaceNormals more than once; returns stats [n][8]."""
        n = len(fpfhs)
        if n == 0 or len(normals) != n or len(keypoints) != n:
            raise LmonoError("one SurfaceNormals and one keypoint array per FpfhDescriptors")
        ctx = fpfhs[0].ctx
        ks = [FpfhDescriptors._keypoints(k) for k in keypoints]
        fh = (C.c_void_p * n)(*[a.h for a in fpfhs]); nh = (C.c_void_p * n)(*[b.h for b in normals])
        kh = (C.c_void_p * n)(*[k.ctypes.data if len(k) else None for k in ks])
        ms = np.array([len(k) for k in ks], np.int64)
        stats = np.zeros((n, 8), np.int64)
        ctx.check(ctx.L.lmono_fpfh_compute_batch(ctx.h, n, fh, nh, kh, ms.ctypes.data, stats.ctypes.data))
        for a, s in zip(fpfhs, stats):
            a.stats = s.copy()
        return stats

    def read(self):
        """(descriptors [m][33] float32, contributing points [m] uint32, flags [m] uint32) of the last compute, in keypoint order."""
        m = int(self.ctx.check(self.ctx.L.lmono_fpfh_read(self.ctx.h, self.h, None, None, None, 0)))
        desc = np.zeros((max(m, 1), 33), np.float32); cnt = np.zeros(max(m, 1), np.uint32); flag = np.zeros(max(m, 1), np.uint32)
        self.ctx.check(self.ctx.L.lmono_fpfh_read(self.ctx.h, self.h, desc.ctypes.data, cnt.ctypes.data, flag.ctypes.data, m))
        return desc[:m], cnt[:m], flag[:m]

    def keypoints(self):
        """The keypoints of the last compute, [m][3] float32."""
        m = int(self.ctx.check(self.ctx.L.lmono_fpfh_keypoints(self.ctx.h, self.h, None, 0)))
        out = np.zeros((max(m, 1), 3), np.float32)
        self.ctx.check(self.ctx.L.lmono_fpfh_keypoints(self.ctx.h, self.h, out.ctypes.data, m))
        return out[:m]


class CoarseAligner(_Handle):
    """Sample-consensus initial alignment on FPFH descriptors on the device (lmono_sacia_*): align(src, tgt) takes two
    FpfhDescriptors after a compute and returns the call's stats [ok, winning hypothesis, its error word, its inliers, void hypotheses,
    usable source keypoints, usable target keypoints, n_hyp]; transform() is the [3][4] float64 that moves the source onto the target, what
    CloudAligner.set_guess takes; errors() gives every hypothesis's (error word uint64, all ones: void; inliers uint32).  launch_hyps
    splits the hypotheses over launches and changes no result.  An LmonoError carries the C return value in .code."""

    _destroy = "lmono_sacia_destroy"

    def __init__(self, ctx, min_sample_dist=0.5, max_corr=1.0, k_corr=10, n_hyp=1024, seed=1, launch_hyps=None):
        super().__init__(ctx)
        self.stats = np.zeros(8, np.int64)
        self._create("lmono_sacia_create", C.c_float(min_sample_dist), C.c_float(max_corr), int(k_corr), int(n_hyp), C.c_uint32(seed), int(launch_hyps or 0))

    def align(self, src, tgt):
        stats = np.zeros(8, np.int64)
        self.ctx.check(self.ctx.L.lmono_sacia_align(self.ctx.h, self.h, src.h, tgt.h, stats.ctypes.data))
        self.stats = stats
        return stats

    def transform(self):
        out = np.zeros(12, np.float64)
        self.ctx.check(self.ctx.L.lmono_sacia_transform(self.ctx.h, self.h, out.ctypes.data))
        return out.reshape(3, 4)

    def errors(self):
        n = int(self.ctx.check(self.ctx.L.lmono_sacia_errors(self.ctx.h, self.h, None, None, 0)))
        err = np.zeros(max(n, 1), np.uint64); inl = np.zeros(max(n, 1), np.uint32)
        self.ctx.check(self.ctx.L.lmono_sacia_errors(self.ctx.h, self.h, err.ctypes.data, inl.ctypes.data, n))
        return err[:n], inl[:n]

    def refine(self, cloud_aligner, source_points):
        """The refineAlignment the reference leaves commented out: the fine alignment started from the coarse transform; returns its stats."""
        cloud_aligner.set_guess(self.transform())
        return cloud_aligner.align(source_points)


TRACK_RECORD = np.dtype([("id", np.int32), ("x_n", np.float32), ("y_n", np.float32), ("u", np.float32), ("v", np.float32),
                         ("vx", np.float32), ("vy", np.float32), ("track_cnt", np.int32)])
TRACK_MAX_POINTS = 512


class RejectF(C.Structure):
    """lmono_reject_f: the parameters of rejectWithF (F_THRESHOLD, F_DIS, FOCAL_LENGTH; hypothesis count and sample seed)."""
    _fields_ = [("f_threshold", C.c_double), ("f_dis", C.c_double), ("focal_length", C.c_double), ("n_hyp", C.c_int32), ("seed", C.c_uint32)]


def feature_frame(records):
    """records -> FeatureManager::Image: {feature_id: [(camera_id 0, [x, y, u, v, vx, vy] float64)]} (FeatureTracker.cc:372-397)."""
    return {int(r["id"]): [(0, np.array([r["x_n"], r["y_n"], r["u"], r["v"], r["vx"], r["vy"]], np.float64))] for r in records}


class FeatureTracker(_Handle):
    """FeatureTracker::trackImage of the mono path on the device (lmono_tracker_*): pyramidal KLT with forward-backward check,
    setMask, goodFeaturesToTrack, liftProjective and velocities.  track() returns the frame's TRACK_RECORD array."""

    _destroy = "lmono_tracker_destroy"

    def __init__(self, ctx, camera, max_cnt=150, min_dist=30, flags=0):
        super().__init__(ctx)
        self.cam = camera
        self.max_cnt = int(max_cnt)
        self._create("lmono_tracker_create", C.byref(camera), int(max_cnt), int(min_dist), int(flags))

    def _format(self, image):
        if image.shape == (self.cam.height, self.cam.width):
            return 0
        if image.shape == (self.cam.height, self.cam.width, 3):
            return 1
        raise LmonoError("image must be [height][width] or [height][width][3] uint8")

    def track(self, time, image):
        image = np.ascontiguousarray(image, np.uint8)
        rec = np.zeros(TRACK_MAX_POINTS, TRACK_RECORD)
        n = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_tracker_track(self.ctx.h, self.h, float(time), image.ctypes.data, self._format(image), rec.ctypes.data, len(rec), C.addressof(n)))
        return rec[:n.value].copy()

    def track_image(self, time, image):
        """trackImage(time, image) -> FeatureManager::Image."""
        return feature_frame(self.track(time, image))

    def reset(self):
        self.ctx.check(self.ctx.L.lmono_tracker_reset(self.ctx.h, self.h))

    def n_levels(self):
        return self.ctx.L.lmono_tracker_pyramid(self.ctx.h, self.h, 0, None, None, None, None, None)

    def pyramid(self, level):
        """-> (image u8, dx i16, dy i16) of one level of the last frame's pyramid."""
        w, h = C.c_int(0), C.c_int(0)
        n = self.ctx.L.lmono_tracker_pyramid(self.ctx.h, self.h, int(level), None, None, None, C.addressof(w), C.addressof(h))
        self.ctx.check(min(n, 0))
        if level >= n:
            raise LmonoError("the pyramid has %d levels" % n)
        img = np.zeros((h.value, w.value), np.uint8); dx = np.zeros((h.value, w.value), np.int16); dy = np.zeros_like(dx)
        self.ctx.check(min(self.ctx.L.lmono_tracker_pyramid(self.ctx.h, self.h, int(level), img.ctypes.data, dx.ctypes.data, dy.ctypes.data, None, None), 0))
        return img, dx, dy

    def response(self):
        r = np.zeros((self.cam.height, self.cam.width), np.float32)
        self.ctx.check(self.ctx.L.lmono_tracker_response(self.ctx.h, self.h, r.ctypes.data))
        return r

    def lk(self, pts):
        """Forward and backward LK between the last two frames on given points -> (fwd [n, 2], rev [n, 2], status [n, 2])."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = len(pts)
        fwd = np.zeros((n, 2), np.float32); rev = np.zeros((n, 2), np.float32); st = np.zeros((n, 2), np.uint8)
        self.ctx.check(self.ctx.L.lmono_tracker_lk(self.ctx.h, self.h, n, pts.ctypes.data, fwd.ctypes.data, rev.ctypes.data, st.ctypes.data))
        return fwd, rev, st

    def set_reject_f(self, f_threshold, f_dis=None, focal_length=460.0, n_hyp=256, seed=0):
        """Switch rejectWithF on from the next frame (use_rejectF: 1, F_THRESHOLD, F_DIS); set_reject_f(None) switches it off."""
        if f_threshold is None:
            self.ctx.check(self.ctx.L.lmono_tracker_set_reject_f(self.ctx.h, self.h, None))
            return
        if f_dis is None:
            raise LmonoError("set_reject_f needs f_threshold and f_dis")
        prm = RejectF(float(f_threshold), float(f_dis), float(focal_length), int(n_hyp), int(seed) & 0xFFFFFFFF)
        self.ctx.check(self.ctx.L.lmono_tracker_set_reject_f(self.ctx.h, self.h, C.byref(prm)))

    def reject_stats(self):
        """-> (stats [4] int32: valid hypotheses, best hypothesis, gate-1 inliers, kept after gate 2; all -1 when the step did
        not run, F [9] fp64 row-major) of the last frame."""
        stats = np.zeros(4, np.int32); F = np.zeros(9, np.float64)
        self.ctx.check(self.ctx.L.lmono_tracker_reject_stats(self.ctx.h, self.h, stats.ctypes.data, F.ctypes.data))
        return stats, F

    def reject_f(self, prev_px, cur_px, frame_key=0):
        """The rejection step alone on 8..512 given pixel pairs -> (status [n] uint8, stats [4], F [9]); leaves the tracks alone."""
        a = np.ascontiguousarray(prev_px, np.float32).reshape(-1, 2); b = np.ascontiguousarray(cur_px, np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise LmonoError("prev_px and cur_px differ in length")
        st = np.zeros(max(len(a), 1), np.uint8); stats = np.zeros(4, np.int32); F = np.zeros(9, np.float64)
        self.ctx.check(self.ctx.L.lmono_tracker_reject_f(self.ctx.h, self.h, len(a), a.ctypes.data, b.ctypes.data, int(frame_key) & 0xFFFFFFFF,
                                                         st.ctypes.data, stats.ctypes.data, F.ctypes.data))
        return st[:len(a)], stats, F


class FeatureTrackerBatch:
    """N independent FeatureTrackers advanced by one frame per call, every phase one launch (lmono_tracker_track_batch).
    Images are device pointers (e.g. torch tensors' data_ptr()) of [height][width] or [height][width][3] uint8.
    max_cnt: one value, or one per stream.  reject_f: None, one dict of set_reject_f arguments for every stream, or a list
    with one dict or None per stream (streams with and without rejection share a batch)."""

    def __init__(self, ctx, cameras, max_cnt=150, min_dist=30, reject_f=None):
        self.ctx = ctx
        cnts = [int(max_cnt)] * len(cameras) if np.isscalar(max_cnt) else [int(v) for v in max_cnt]
        self.trackers = [FeatureTracker(ctx, cam, cnts[s], min_dist) for s, cam in enumerate(cameras)]
        if reject_f is not None:
            self.set_reject_f(reject_f)
        n = len(self.trackers)
        self._handles = (C.c_void_p * n)(*[t.h for t in self.trackers])
        self._rec = np.zeros((n, TRACK_MAX_POINTS), TRACK_RECORD)
        self._recp = (C.c_void_p * n)(*[self._rec[s].ctypes.data for s in range(n)])
        self._caps = np.full(n, TRACK_MAX_POINTS, np.int32)

    def track(self, times, image_ptrs, bgr=False):
        n = len(self.trackers)
        t = np.ascontiguousarray(times, np.float64).reshape(n)
        ip = (C.c_void_p * n)(*[int(p) for p in image_ptrs])
        cnt = np.zeros(n, np.int32)
        self.ctx.check(self.ctx.L.lmono_tracker_track_batch(self.ctx.h, n, self._handles, t.ctypes.data, ip, 1 if bgr else 0, self._recp,
                                                            self._caps.ctypes.data, cnt.ctypes.data))
        return [self._rec[s, :cnt[s]].copy() for s in range(n)]

    def set_reject_f(self, reject_f):
        per = [reject_f] * len(self.trackers) if reject_f is None or isinstance(reject_f, dict) else list(reject_f)
        if len(per) != len(self.trackers):
            raise LmonoError("reject_f needs one entry per stream")
        for t, prm in zip(self.trackers, per):
            if prm is None:
                t.set_reject_f(None)
            else:
                t.set_reject_f(**prm)

    def reject_stats(self):
        return [t.reject_stats() for t in self.trackers]

    def reset(self):
        for t in self.trackers:
            t.reset()

    def close(self):
        for t in self.trackers:
            t.close()


class BriefPattern(C.Structure):
    """lmono_brief_pattern: the 256 pixel-pair tests of DVision's BRIEF (x1, y1, x2, y2 of brief_pattern.yml)."""
    _fields_ = [("x1", C.c_int8 * 256), ("y1", C.c_int8 * 256), ("x2", C.c_int8 * 256), ("y2", C.c_int8 * 256)]


def _brief_pattern_struct(pattern):
    p = np.asarray(pattern)
    if p.shape != (4, 256):
        raise LmonoError("a BRIEF pattern is [4][256] integers (x1, y1, x2, y2)")
    if (np.abs(p.astype(np.int64)) > 127).any():
        raise LmonoError("a BRIEF pattern offset does not fit 8 bits (the library takes -63..63)")
    s = BriefPattern()
    for name, row in zip(("x1", "y1", "x2", "y2"), p):
        getattr(s, name)[:] = [int(v) for v in row]
    return s


class BriefVocabulary(_Handle):
    """A BRIEF vocabulary tree on the device (lmono_brief_vocabulary_*).  voc: the dict of load_brief_vocabulary /
    train_brief_vocabulary (brief_tools.py); a malformed one is refused by the library with its reason."""

    _destroy = "lmono_brief_vocabulary_destroy"

    def __init__(self, ctx, voc):
        super().__init__(ctx)
        nid, par, wt, de, wn, wi = _voc_arrays(voc)
        if not (len(par) == len(wt) == len(de) == len(nid)) or len(wi) != len(wn):
            raise LmonoError("BriefVocabulary: the node arrays (and the word arrays) differ in length")
        self._create("lmono_brief_vocabulary_create", int(voc["k"]), int(voc["L"]), int(voc["scoring"]), int(voc["weighting"]), len(nid), nid.ctypes.data,
                     par.ctypes.data, wt.ctypes.data, de.ctypes.data, len(wn), wn.ctypes.data, wi.ctypes.data)

    def transform(self, descriptors):
        """-> (word int32 [n], weight float64 [n]) of descriptors [n, 8] uint32."""
        de = np.ascontiguousarray(descriptors, np.uint32).reshape(-1, 8)
        word = np.full(len(de), -1, np.int32); weight = np.zeros(len(de))
        self.ctx.check(self.ctx.L.lmono_brief_vocabulary_transform(self.ctx.h, self.h, len(de), de.ctypes.data, word.ctypes.data, weight.ctypes.data))
        return word, weight


class PnPParams(C.Structure):
    """lmono_pnp_params: the PnP threshold on the normalised plane, hypothesis count and sample seed, and the gates of findConnection
    (MIN_BRIEF_LOOP_NUM, MIN_PNP_LOOP_NUM, ANGLE_THRESHOLD in degrees, TRANS_THRESHOLD in m).  A field left 0 takes its default:
    10 / 460, 256, 25, 5, 30, 20."""
    _fields_ = [("threshold", C.c_double), ("n_hyp", C.c_int32), ("seed", C.c_uint32), ("min_brief_loop_num", C.c_int32), ("min_pnp_loop_num", C.c_int32),
                ("angle_threshold", C.c_double), ("trans_threshold", C.c_double)]


def pnp_ransac(ctx, points_3d, points_2d, guess_tq, keys=None, params=None):
    """The PnP step of the loop verification (lmono_pnp_ransac) on a batch of problems in one launch.  points_3d: a list
    of [m, 3] arrays (m <= 512), points_2d: a list of [m, 2] normalised image points, guess_tq: [n, 7] camera-from-world guesses
    t (x y z), q (x y z w), keys: [n] uint32 sample-stream keys (default 0) -> (list of status [m] uint8, pose [n, 7], stats [n, 4])."""
    L = ctx.L
    p3 = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in points_3d]
    p2 = [np.ascontiguousarray(a, np.float32).reshape(-1, 2) for a in points_2d]
    n = len(p3)
    g = np.ascontiguousarray(guess_tq, np.float64).reshape(-1, 7)
    ky = np.zeros(n, np.uint32) if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
    if len(p2) != n or len(g) != n or len(ky) != n or any(len(a) != len(b) for a, b in zip(p3, p2)):
        raise LmonoError("pnp_ransac: points_3d, points_2d, guess_tq and keys differ in length")
    cnt = np.array([len(a) for a in p3], np.int32)
    a3 = np.concatenate(p3 + [np.zeros((1, 3), np.float32)]); a2 = np.concatenate(p2 + [np.zeros((1, 2), np.float32)])
    st = np.zeros(int(cnt.sum()) + 1, np.uint8); pose = np.zeros((n, 7)); stats = np.zeros((n, 4), np.int32)
    ctx.check(L.lmono_pnp_ransac(ctx.h, C.byref(params) if params is not None else None, n, cnt.ctypes.data, a3.ctypes.data, a2.ctypes.data, g.ctypes.data,
                                 ky.ctypes.data, st.ctypes.data, pose.ctypes.data, stats.ctypes.data))
    off = np.concatenate([[0], np.cumsum(cnt)])
    return [st[off[i]:off[i + 1]].copy() for i in range(n)], pose, stats


def _pairs_arrays(pairs_list):
    """A list of [m, 4] arrays -> (m int32 [n], the rows concatenated, with one spare row so that the pointer is never null)."""
    ps = [np.ascontiguousarray(a, np.float64).reshape(-1, 4) for a in pairs_list]
    m = np.array([len(a) for a in ps], np.int32)
    return m, np.concatenate(ps + [np.zeros((1, 4))])


def relative_rotation(ctx, pairs_list):
    """The camera's rotation increment of each problem from its pairs of normalised image points (lmono_relative_rotation, DESIGN.md 6i:
    essential matrix over all pairs, decomposition, cheirality vote), all problems in one launch.  pairs_list: a list of [m, 4] arrays
    (prev x, prev y, cur x, cur y; m <= 512) -> (R [n, 3, 3], stats [n, 6] = pairs used, the four front counts, the winner)."""
    m, flat = _pairs_arrays(pairs_list)
    n = len(m)
    R = np.zeros((n, 3, 3)); stats = np.zeros((n, 6), np.int32)
    ctx.check(ctx.L.lmono_relative_rotation(ctx.h, n, m.ctypes.data, flat.ctypes.data, R.ctypes.data, stats.ctypes.data))
    return R, stats


class ExtrinsicCalibrator(_Handle):
    """The camera-LiDAR rotation calibration of ESTIMATE_LASER == 2 for n_streams independent streams (lmono_excalib_*).
    Quaternions are x y z w.  `streams`: the stream index of each entry of a call (default 0 .. n-1); a stream may be named once per call."""

    _destroy = "lmono_excalib_destroy"

    def __init__(self, ctx, n_streams=1, count=10):
        super().__init__(ctx)
        self.n_streams, self.count = int(n_streams), int(count)
        h = C.c_void_p()
        ctx.check(ctx.L.lmono_excalib_create(ctx.h, self.n_streams, C.byref(h)))
        self.h = h.value

    def _streams(self, streams, n):
        st = np.arange(n, dtype=np.int32) if streams is None else np.ascontiguousarray(streams, np.int32).reshape(-1)
        if len(st) != n:
            raise LmonoError("ExtrinsicCalibrator: streams and the other arguments differ in length")
        return st

    def step(self, pairs_list, q_lidar, streams=None):
        """One frame of each named stream, stages 1-4 in one launch.  q_lidar [n, 4]: the LiDAR's rotation increment over the same frame
        -> dict(R_cam [n, 3, 3], stats [n, 6], rlc [n, 3, 3], sv [n, 4], huber [n], ok [n] bool)."""
        m, flat = _pairs_arrays(pairs_list)
        n = len(m)
        ql = np.ascontiguousarray(q_lidar, np.float64).reshape(-1, 4)
        st = self._streams(streams, n)
        if len(ql) != n:
            raise LmonoError("ExtrinsicCalibrator.step: pairs_list and q_lidar differ in length")
        R = np.zeros((n, 3, 3)); stats = np.zeros((n, 6), np.int32); rlc = np.zeros((n, 3, 3)); sv = np.zeros((n, 4)); hub = np.zeros(n); ok = np.zeros(n, np.int32)
        self.ctx.check(self.ctx.L.lmono_excalib_step(self.h, n, st.ctypes.data, m.ctypes.data, flat.ctypes.data, ql.ctypes.data, self.count, R.ctypes.data,
                                                     stats.ctypes.data, rlc.ctypes.data, sv.ctypes.data, hub.ctypes.data, ok.ctypes.data))
        return dict(R_cam=R, stats=stats, rlc=rlc, sv=sv, huber=hub, ok=ok.astype(bool))

    def push(self, q_cam, q_lidar, streams=None):
        """Stage 4 alone on given rotation pairs q_cam, q_lidar [n, 4] -> dict(rlc, sv, huber, ok)."""
        qc = np.ascontiguousarray(q_cam, np.float64).reshape(-1, 4); ql = np.ascontiguousarray(q_lidar, np.float64).reshape(-1, 4)
        n = len(qc)
        st = self._streams(streams, n)
        if len(ql) != n:
            raise LmonoError("ExtrinsicCalibrator.push: q_cam and q_lidar differ in length")
        rlc = np.zeros((n, 3, 3)); sv = np.zeros((n, 4)); hub = np.zeros(n); ok = np.zeros(n, np.int32)
        self.ctx.check(self.ctx.L.lmono_excalib_push(self.h, n, st.ctypes.data, qc.ctypes.data, ql.ctypes.data, self.count, rlc.ctypes.data, sv.ctypes.data,
                                                     hub.ctypes.data, ok.ctypes.data))
        return dict(rlc=rlc, sv=sv, huber=hub, ok=ok.astype(bool))

    def state(self, s=0):
        """-> (frame_count, M [4, 4]: the running sum, rlc [3, 3]) of stream s."""
        fc = C.c_int(0); M = np.zeros((4, 4)); rlc = np.zeros((3, 3))
        self.ctx.check(self.ctx.L.lmono_excalib_state(self.h, int(s), C.byref(fc), M.ctypes.data, rlc.ctypes.data))
        return fc.value, M, rlc

    def reset(self, s=None):
        self.ctx.check(self.ctx.L.lmono_excalib_reset(self.h, -1 if s is None else int(s)))


class KeyFrames(_Handle):
    """A device-resident store of keyframes (lmono_keyframes_*): FAST corners, BRIEF descriptors of the corners and of
    the window points, and the exhaustive Hamming search of KeyFrame::searchByBRIEFDes.  pattern: [4][256] (load_brief_pattern)."""

    _destroy = "lmono_keyframes_destroy"

    def __init__(self, ctx, camera, pattern, max_keyframes=64, max_keypoints=4096, fast_threshold=0):
        super().__init__(ctx)
        self.cam = camera
        pat = _brief_pattern_struct(pattern)
        self._create("lmono_keyframes_create", C.byref(camera), C.byref(pat), int(max_keyframes), int(max_keypoints), int(fast_threshold))
        self.last_n_keypoints = 0

    def _format(self, image):
        if image.shape == (self.cam.height, self.cam.width):
            return 0
        if image.shape == (self.cam.height, self.cam.width, 3):
            return 1
        raise LmonoError("image must be [height][width] or [height][width][3] uint8")

    def __len__(self):
        n = self.ctx.L.lmono_keyframes_size(self.ctx.h, self.h)
        self.ctx.check(min(n, 0))
        return n

    def add(self, image, window_uv):
        """One keyframe from a host image and its window points [n <= 512][2] -> (index, FAST corners found)."""
        image = np.ascontiguousarray(image, np.uint8)
        uv = np.ascontiguousarray(window_uv, np.float32).reshape(-1, 2)
        idx, nkp = C.c_int(-1), C.c_int(0)
        rc = self.ctx.L.lmono_keyframes_add(self.ctx.h, self.h, image.ctypes.data, self._format(image), len(uv), uv.ctypes.data if len(uv) else None,
                                            C.addressof(idx), C.addressof(nkp))
        self.last_n_keypoints = nkp.value
        self.ctx.check(rc)
        return idx.value, nkp.value

    @classmethod
    def add_batch(cls, stores, image_ptrs, window_uvs, bgr=False):
        """One keyframe for each of several distinct stores, every phase one launch (lmono_keyframes_add_batch).  image_ptrs: device
        pointers (e.g. torch tensors' data_ptr()) -> (indices [n], FAST corners found [n])."""
        n = len(stores)
        ctx = stores[0].ctx
        uvs = [np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in window_uvs]
        if len(uvs) != n or len(image_ptrs) != n:
            raise LmonoError("add_batch needs one image and one window point array per store")
        hs = (C.c_void_p * n)(*[s.h for s in stores])
        ip = (C.c_void_p * n)(*[int(p) for p in image_ptrs])
        up = (C.c_void_p * n)(*[u.ctypes.data if len(u) else None for u in uvs])
        nw = np.array([len(u) for u in uvs], np.int32)
        idx = np.full(n, -1, np.int32); nkp = np.zeros(n, np.int32)
        rc = ctx.L.lmono_keyframes_add_batch(ctx.h, n, hs, ip, 1 if bgr else 0, nw.ctypes.data, up, idx.ctypes.data, nkp.ctypes.data)
        for s, k in zip(stores, nkp):
            s.last_n_keypoints = int(k)
        ctx.check(rc)
        return idx, nkp

    def load(self, keypoints, norm, descriptors, window_uv=None, window_descriptors=None):
        """A keyframe from saved data (the reference's second constructor) -> index."""
        kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 2); nm = np.ascontiguousarray(norm, np.float32).reshape(-1, 2)
        de = np.ascontiguousarray(descriptors, np.uint32).reshape(-1, 8)
        uv = np.zeros((0, 2), np.float32) if window_uv is None else np.ascontiguousarray(window_uv, np.float32).reshape(-1, 2)
        wd = np.zeros((0, 8), np.uint32) if window_descriptors is None else np.ascontiguousarray(window_descriptors, np.uint32).reshape(-1, 8)
        if not (len(kp) == len(nm) == len(de)) or len(uv) != len(wd):
            raise LmonoError("load: keypoints / norm / descriptors (and window points / descriptors) differ in length")
        idx = C.c_int(-1)
        self.ctx.check(self.ctx.L.lmono_keyframes_load(self.ctx.h, self.h, len(kp), kp.ctypes.data, nm.ctypes.data, de.ctypes.data, len(uv), uv.ctypes.data, wd.ctypes.data,
                                                       C.addressof(idx)))
        return idx.value

    def get(self, index):
        """-> dict: keypoints [n, 2], norm [n, 2], descriptors [n, 8], window_uv [m, 2], window_descriptors [m, 8] of a stored keyframe."""
        nk, nw = C.c_int(0), C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_keyframes_get(self.ctx.h, self.h, int(index), C.addressof(nk), None, None, None, C.addressof(nw), None, None))
        kp = np.zeros((nk.value, 2), np.float32); nm = np.zeros_like(kp); de = np.zeros((nk.value, 8), np.uint32)
        uv = np.zeros((nw.value, 2), np.float32); wd = np.zeros((nw.value, 8), np.uint32)
        self.ctx.check(self.ctx.L.lmono_keyframes_get(self.ctx.h, self.h, int(index), None, kp.ctypes.data, nm.ctypes.data, de.ctypes.data, None, uv.ctypes.data, wd.ctypes.data))
        return {"keypoints": kp, "norm": nm, "descriptors": de, "window_uv": uv, "window_descriptors": wd}

    def images(self):
        """-> (blurred image, FAST score image), uint8 [height, width], of the last image added."""
        b = np.zeros((self.cam.height, self.cam.width), np.uint8); s = np.zeros_like(b)
        self.ctx.check(self.ctx.L.lmono_keyframes_images(self.ctx.h, self.h, b.ctypes.data, s.ctypes.data))
        return b, s

    def match(self, cur, old_indices):
        """searchByBRIEFDes of keyframe cur's window descriptors against each of old_indices -> dict of [n_old, n_window] arrays
        status, index, dist, old_uv [.., 2], old_norm [.., 2] and counts [n_old]."""
        old = np.ascontiguousarray(old_indices, np.int32).reshape(-1)
        nw = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_keyframes_get(self.ctx.h, self.h, int(cur), None, None, None, None, C.addressof(nw), None, None))
        n, m = len(old), nw.value
        st = np.zeros((n, m), np.uint8); ix = np.full((n, m), -1, np.int32); di = np.full((n, m), 128, np.int32)
        uv = np.zeros((n, m, 2), np.float32); nm = np.zeros((n, m, 2), np.float32); cnt = np.zeros(n, np.int32)
        self.ctx.check(self.ctx.L.lmono_keyframes_match(self.ctx.h, self.h, int(cur), n, old.ctypes.data, st.ctypes.data, ix.ctypes.data, di.ctypes.data,
                                                        uv.ctypes.data, nm.ctypes.data, cnt.ctypes.data))
        return {"status": st, "index": ix, "dist": di, "old_uv": uv, "old_norm": nm, "counts": cnt}

    def verify(self, cur, old_indices, point_3d, vio_tq, ex_tq, old_tq=None, params=None):
        """findConnection of keyframe cur against each of old_indices (lmono_keyframes_verify): the match, the PnP step
        and the gates.  point_3d: [n_window, 3] world points of cur's window points; vio_tq, ex_tq: [7] t (x y z), q (x y z w) of the
        body and of the camera in the body; old_tq: [n_old, 7] poses of the old keyframes (for the 15-value channel) or None.
        -> dict of per-candidate arrays: counts, inliers, status [n_old, n_window], pnp_tq_old [n_old, 7], loop_info [n_old, 8],
        has_loop [n_old] bool, channel [n_old, 15] or None, relative_euler [n_old, 3], pose [n_old, 7], stats [n_old, 4]; and, ready
        for PoseGraph(poses, loops, loop_info): loops [k, 2] (old, cur) and loops_info [k, 8] of the candidates with has_loop."""
        old = np.ascontiguousarray(old_indices, np.int32).reshape(-1)
        nw = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_keyframes_get(self.ctx.h, self.h, int(cur), None, None, None, None, C.addressof(nw), None, None))
        n, m = len(old), nw.value
        p3 = np.ascontiguousarray(point_3d, np.float32).reshape(-1, 3)
        if len(p3) != m:
            raise LmonoError("verify: point_3d must have one row per window point of the current keyframe (%d)" % m)
        vio = np.ascontiguousarray(vio_tq, np.float64).reshape(7); ex = np.ascontiguousarray(ex_tq, np.float64).reshape(7)
        otq = None if old_tq is None else np.ascontiguousarray(old_tq, np.float64).reshape(-1, 7)
        if otq is not None and len(otq) != n:
            raise LmonoError("verify: old_tq must have one pose per old index")
        cnt = np.zeros(n, np.int32); inl = np.zeros(n, np.int32); st = np.zeros((n, m), np.uint8); tq = np.zeros((n, 7)); li = np.zeros((n, 8))
        hl = np.zeros(n, np.uint8); ch = None if otq is None else np.zeros((n, 15)); eu = np.zeros((n, 3)); pose = np.zeros((n, 7)); stats = np.zeros((n, 4), np.int32)
        self.ctx.check(self.ctx.L.lmono_keyframes_verify(self.ctx.h, self.h, int(cur), n, old.ctypes.data, p3.ctypes.data if m else None, vio.ctypes.data, ex.ctypes.data,
                                                         None if otq is None else otq.ctypes.data, C.byref(params) if params is not None else None,
                                                         cnt.ctypes.data, inl.ctypes.data, st.ctypes.data, tq.ctypes.data, li.ctypes.data, hl.ctypes.data,
                                                         None if ch is None else ch.ctypes.data, eu.ctypes.data, pose.ctypes.data, stats.ctypes.data))
        has = hl.astype(bool)
        loops = np.stack([old[has], np.full(int(has.sum()), int(cur), np.int32)], 1).astype(np.int32)
        return {"counts": cnt, "inliers": inl, "status": st, "pnp_tq_old": tq, "loop_info": li, "has_loop": has, "channel": ch, "relative_euler": eu,
                "pose": pose, "stats": stats, "loops": loops, "loops_info": li[has]}

    def set_vocabulary(self, vocabulary):
        """Attach a BriefVocabulary (None detaches): the store keeps the device tree alive on its own."""
        self.ctx.check(self.ctx.L.lmono_keyframes_set_vocabulary(self.ctx.h, self.h, vocabulary.h if vocabulary is not None else None))

    def bow(self, index):
        """The BoW vector of a stored keyframe -> (word int32 [m] ascending, value float64 [m])."""
        nk = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_keyframes_get(self.ctx.h, self.h, int(index), C.addressof(nk), None, None, None, None, None, None))
        word = np.zeros(nk.value + 1, np.int32); val = np.zeros(nk.value + 1); n = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_keyframes_bow(self.ctx.h, self.h, int(index), C.addressof(n), word.ctypes.data, val.ctypes.data))
        return word[:n.value].copy(), val[:n.value].copy()

    def query(self, cur, max_results=4, max_id=-1):
        """db.query of keyframe cur against the keyframes before it (queryL1) -> (id int32 [n], Score float64 [n]), best first."""
        ids = np.zeros(16, np.int32); sc = np.zeros(16); n = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_keyframes_query(self.ctx.h, self.h, int(cur), int(max_results), int(max_id), C.addressof(n), ids.ctypes.data, sc.ctypes.data))
        return ids[:n.value].copy(), sc[:n.value].copy()

    def detect_loop(self, cur, loop_search_gap=100):
        """LoopDetector::detectLoop of keyframe cur -> (loop index or -1, id int32 [n <= 4], Score float64 [n])."""
        ids = np.zeros(4, np.int32); sc = np.zeros(4); n = C.c_int(0); loop = C.c_int(-1)
        self.ctx.check(self.ctx.L.lmono_keyframes_detect_loop(self.ctx.h, self.h, int(cur), int(loop_search_gap), C.addressof(loop), C.addressof(n), ids.ctypes.data, sc.ctypes.data))
        return loop.value, ids[:n.value].copy(), sc[:n.value].copy()

    @classmethod
    def detect_loop_batch(cls, stores, curs, loop_search_gap=100):
        """detect_loop of one keyframe in each of several distinct stores that share a vocabulary, every phase one launch ->
        list of (loop index, ids, Scores)."""
        n = len(stores)
        ctx = stores[0].ctx
        cur = np.ascontiguousarray(curs, np.int32).reshape(-1)
        if len(cur) != n:
            raise LmonoError("detect_loop_batch needs one keyframe index per store")
        hs = (C.c_void_p * n)(*[s.h for s in stores])
        loop = np.full(n, -1, np.int32); cnt = np.zeros(n, np.int32); ids = np.zeros((n, 4), np.int32); sc = np.zeros((n, 4))
        ctx.check(ctx.L.lmono_keyframes_detect_loop_batch(ctx.h, n, hs, cur.ctypes.data, int(loop_search_gap), loop.ctypes.data, cnt.ctypes.data, ids.ctypes.data, sc.ctypes.data))
        return [(int(loop[s]), ids[s, :cnt[s]].copy(), sc[s, :cnt[s]].copy()) for s in range(n)]

    def clear(self):
        self.ctx.check(self.ctx.L.lmono_keyframes_clear(self.ctx.h, self.h))


class PoseGraph(_Handle):
    """Loop-closure pose graph (lmono_pose_graph_*; a new feature): 4-DoF keyframe graph over odometry poses and
    loop_info records.  optimize() on one GPU; linearise() / reduce_buffer / step() for the multi-GPU round (sharding.py)."""

    _destroy = "lmono_pose_graph_destroy"

    def __init__(self, ctx, poses_tq, loops, loop_info):
        super().__init__(ctx)
        L = ctx.L
        P = np.ascontiguousarray(poses_tq, np.float64).reshape(-1, 7)
        lp = np.ascontiguousarray(loops, np.int32).reshape(-1, 2); li = np.ascontiguousarray(loop_info, np.float64).reshape(-1, 8)
        if len(lp) != len(li):
            raise LmonoError("loops and loop_info differ in length")
        self.n = len(P)
        self._create("lmono_pose_graph_create", self.n, P.ctypes.data, len(lp), lp.ctypes.data, li.ctypes.data)
        rc = C.c_int64(0); bw = C.c_int(0); ne = C.c_int(0)
        L.lmono_pose_graph_info(self.h, C.addressof(rc), C.addressof(bw), C.addressof(ne))
        self.reduce_count, self.bandwidth, self.n_edges = rc.value, bw.value, ne.value
        self.reduce_ptr = L.lmono_pose_graph_reduce_buffer(self.h)

    def reset(self):
        self.ctx.check(self.ctx.L.lmono_pose_graph_reset(self.ctx.h, self.h))

    def order(self):
        """Elimination position of every keyframe: the order H, g and cost are stored in inside the reduce buffer."""
        pos = np.zeros(self.n, np.int32)
        self.ctx.check(self.ctx.L.lmono_pose_graph_order(self.h, pos.ctypes.data))
        return pos

    def use_reduce_tensor(self, tensor):
        """Make a caller-owned contiguous fp64 device tensor of reduce_count elements the buffer linearise() fills and step()
        reads (the tensor handed to torch.distributed.all_reduce)."""
        if tensor.numel() != self.reduce_count or tensor.element_size() != 8 or not tensor.is_contiguous():
            raise LmonoError("reduce tensor must be contiguous fp64 with %d elements" % self.reduce_count)
        self.ctx.check(self.ctx.L.lmono_pose_graph_set_reduce_buffer(self.h, tensor.data_ptr()))
        self.reduce_tensor = tensor
        self.reduce_ptr = tensor.data_ptr()

    def linearise(self, rank=0, world=1):
        self.ctx.check(self.ctx.L.lmono_pose_graph_linearise(self.ctx.h, self.h, rank, world))

    def step(self, max_iter=5):
        done = C.c_int(0)
        self.ctx.check(self.ctx.L.lmono_pose_graph_step(self.ctx.h, self.h, max_iter, C.addressof(done)))
        return bool(done.value)

    def optimize(self, max_iter=5):
        self.ctx.check(self.ctx.L.lmono_pose_graph_optimize(self.ctx.h, self.h, max_iter))
        return self.result()

    def result(self):
        out = np.zeros((self.n, 7)); st = np.zeros(6)
        self.ctx.check(self.ctx.L.lmono_pose_graph_result(self.ctx.h, self.h, out.ctypes.data, st.ctypes.data))
        return out, dict(iterations=int(st[0]), initial_cost=st[1], final_cost=st[2], bandwidth=int(st[3]), accepted=int(st[4]), rejected=int(st[5]))
