"""ctypes bindings for the CPU oracle (oracle/libsdvl_oracle.so) and the synthetic sequence generator.

Test infrastructure only: nothing under slam-sdvl_amd/ imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
CSRC_DIR = os.path.join(ROOT, "slam-sdvl_amd", "csrc")

u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
f64p = C.POINTER(C.c_double)
f32p = C.POINTER(C.c_float)


class Params(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "pyramid_levels", "cell_size", "max_fast_levels", "fast_threshold", "num_features", "use_orb", "orb_size",
        "patch_size", "max_align_its", "search_size", "align_patch_size", "max_align_level", "min_align_level",
        "max_img_align_its", "min_feature_score", "max_matches", "min_matches", "max_failed", "max_optim_pose_its",
        "max_ransac_points", "max_ransac_its", "min_keyframe_its")] + [
        ("inlier_error_threshold", C.c_double), ("lost_ratio", C.c_double)]


class FrameStats(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("state", "quality", "matches", "attempts", "inliers", "outliers", "n_corners",
                                       "align_meas", "keyframe", "relocalized")] + [("pose", C.c_double * 7)]


class SynthView(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("u0", C.c_double), ("v0", C.c_double),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("plane", C.c_double * 4),
                ("seed", C.c_uint32), ("frame_id", C.c_uint32), ("texture", C.c_uint32), ("reserved_", C.c_uint32),
                ("dist", C.c_double * 5)]


def _ensure(path, cmd, cwd):
    if not os.path.exists(path):
        subprocess.check_call(cmd, cwd=cwd)
    return path


def load_oracle(ref_flags=False):
    """the checker (libsdvl_oracle.so: -ffp-contract=off, every parity test compares with it) or, for TIMING ONLY, the same sources
    built here and now with the reference's own flags (CMakeLists.txt:20: -O3 -march=native), libsdvl_oracle_refflags.so"""
    if ref_flags:
        so = os.path.join(ORACLE_DIR, "libsdvl_oracle_refflags.so")
        subprocess.check_call(["make", "-s", "-B", "libsdvl_oracle_refflags.so"], cwd=ORACLE_DIR)   # -march=native: always for THIS host
    else:
        so = _ensure(os.path.join(ORACLE_DIR, "libsdvl_oracle.so"), ["make", "-s"], ORACLE_DIR)
    lib = C.CDLL(so)
    lib.sdvl_ref_shi_tomasi.restype = C.c_double
    return lib


def load_synth():
    so = os.path.join(CSRC_DIR, "libsdvl_synth.so")
    _ensure(so, ["g++", "-O2", "-ffp-contract=off", "-march=x86-64-v3", "-fPIC", "-shared", "-o", so,
                 os.path.join(CSRC_DIR, "synth_host.cc")], CSRC_DIR)
    return C.CDLL(so)


def ptr(a, t):
    return a.ctypes.data_as(t)


TUM_DIST = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633])   # config/config_tum_f1.cfg:15-19
EUROC_DIST = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0])  # config/config_euroc.cfg:15-19
TUM_CAM = np.array([517.3, 516.5, 318.6, 255.3])          # config/config_tum_f1.cfg:11-14
TUM2_CAM = np.array([520.9, 521.0, 325.1, 249.7])         # config/config_tum_f2.cfg:11-14
TUM2_DIST = np.array([0.2312, -0.7849, -0.0033, -0.0001, 0.9172])  # config/config_tum_f2.cfg:15-19
EUROC_CAM = np.array([458.654, 457.296, 367.215, 248.375])  # config/config_euroc.cfg
XI = np.array([0.004, 0.002, 0.001, 0.0008, -0.0012, 0.0005])  # SURVEY §8d trajectory twist per frame


class Oracle:
    def __init__(self, ref_flags=False):
        self.lib = load_oracle(ref_flags)
        self.params = Params()
        self.lib.sdvl_ref_default_params(C.byref(self.params))

    # --- math
    def se3_exp(self, u):
        u = np.ascontiguousarray(u, np.float64); T = np.zeros(7)
        self.lib.sdvl_ref_se3_exp(ptr(u, f64p), ptr(T, f64p)); return T

    def se3_log(self, T):
        T = np.ascontiguousarray(T, np.float64); u = np.zeros(6)
        self.lib.sdvl_ref_se3_log(ptr(T, f64p), ptr(u, f64p)); return u

    def se3_mul(self, A, B):
        A = np.ascontiguousarray(A, np.float64); B = np.ascontiguousarray(B, np.float64); Cc = np.zeros(7)
        self.lib.sdvl_ref_se3_mul(ptr(A, f64p), ptr(B, f64p), ptr(Cc, f64p)); return Cc

    def se3_inv(self, A):
        A = np.ascontiguousarray(A, np.float64); B = np.zeros(7)
        self.lib.sdvl_ref_se3_inv(ptr(A, f64p), ptr(B, f64p)); return B

    def ldlt_solve6(self, A, b):
        A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(6)
        self.lib.sdvl_ref_ldlt_solve6(ptr(A, f64p), ptr(b, f64p), ptr(x, f64p)); return x

    def rand_stream(self, n, seed=1):
        out = np.zeros(n, np.int32)
        self.lib.sdvl_ref_rand_stream(C.c_uint(seed), n, ptr(out, i32p)); return out

    # --- detection
    def pyr_down(self, img):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        out = np.zeros((h // 2, w // 2), np.uint8)
        self.lib.sdvl_ref_pyr_down(ptr(img, u8p), w, h, w, ptr(out, u8p), w // 2); return out

    def pyramid(self, img, levels=5):
        pyr = [np.ascontiguousarray(img, np.uint8)]
        for _ in range(1, levels):
            pyr.append(self.pyr_down(pyr[-1]))
        return pyr

    def fast(self, img, thr=10, nonmax=True, cap=200000):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        out = np.zeros((cap, 3), np.int32)
        n = self.lib.sdvl_ref_fast(ptr(img, u8p), w, h, w, thr, int(nonmax), cap, ptr(out, i32p))
        assert n <= cap
        return out[:n].copy()

    def fast_cells(self, img, cap=200000):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        cs = self.params.cell_size
        ncells = -(-w // cs) * -(-h // cs)
        out = np.zeros((cap, 3), np.int32); offs = np.zeros(ncells + 1, np.int32); ran = np.zeros(ncells, np.uint8)
        n = self.lib.sdvl_ref_fast_cells(ptr(img, u8p), w, h, w, C.byref(self.params), cap, ptr(out, i32p),
                                         ptr(offs, i32p), ptr(ran, u8p))
        assert n <= cap
        return out[:n].copy(), offs, ran

    def detect_pyramid(self, img, nfeatures=None, cap=20000):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        out = np.zeros((cap, 3), np.int32)
        nf = self.params.num_features if nfeatures is None else nfeatures
        n = self.lib.sdvl_ref_detect_pyramid(ptr(img, u8p), w, h, w, C.byref(self.params), nf, cap, ptr(out, i32p))
        assert n <= cap
        return out[:n].copy()

    def retain_best(self, packed, n_points):
        packed = np.ascontiguousarray(packed, np.uint32).copy()
        n = self.lib.sdvl_ref_retain_best(ptr(packed, C.POINTER(C.c_uint32)), len(packed), int(n_points))
        return packed[:n]

    def shi_tomasi(self, img, x, y):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        return self.lib.sdvl_ref_shi_tomasi(ptr(img, u8p), w, h, w, int(x), int(y))

    def filter_corners(self, img, corners, locked=None):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        corners = np.ascontiguousarray(corners, np.int32)
        locked = np.zeros((0, 2)) if locked is None else np.ascontiguousarray(locked, np.float64)
        out = np.zeros(4096, np.int32)
        n = self.lib.sdvl_ref_filter_corners(ptr(img, u8p), w, h, w, C.byref(self.params), len(corners),
                                             ptr(corners, i32p), len(locked), ptr(locked, f64p), 4096, ptr(out, i32p))
        return out[:n].copy()

    def orb_describe(self, img, xy):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        xy = np.ascontiguousarray(xy, np.int32); n = len(xy)
        desc = np.zeros((n, 32), np.uint8); ang = np.zeros(n, np.float32)
        self.lib.sdvl_ref_orb_describe(ptr(img, u8p), w, h, w, n, ptr(xy, i32p), ptr(desc, u8p), ptr(ang, f32p))
        return desc, ang

    def orb_distance(self, a, b):
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        return self.lib.sdvl_ref_orb_distance(ptr(a, u8p), ptr(b, u8p))

    def pose_from_matches(self, cam, obs, pose, w=640, h=480, rand_seed=1, rand_skip=0):
        """SelectInliers + OptimizePose on obs[n][6] = ax, ay, px, py, pz, level"""
        cam = np.ascontiguousarray(cam, np.float64); obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 6)
        n = len(obs); pose = np.array(pose, np.float64)
        nd = C.c_int(); ni = C.c_int(); no = C.c_int(); rf = C.c_int()
        ii = np.zeros(max(n, 1), np.int32); oi = np.zeros(max(n, 1), np.int32)
        self.lib.sdvl_ref_pose_from_matches_ex(C.byref(self.params), w, h, ptr(cam, f64p), n, ptr(obs, f64p), C.c_uint(rand_seed),
                                               int(rand_skip), ptr(pose, f64p), C.byref(nd), C.byref(ni), ptr(ii, i32p),
                                               C.byref(no), ptr(oi, i32p), C.byref(rf))
        return dict(pose=pose, n_draws=nd.value, inliers=ii[:ni.value].copy(), outliers=oi[:no.value].copy(), refined=rf.value)

    def undistort(self, img, cam, dist):
        """Camera::UndistortImage = cv::undistort; cam = fx fy u0 v0, dist = d0..d4"""
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        cam = np.ascontiguousarray(cam, np.float64); dist = np.ascontiguousarray(dist, np.float64)
        out = np.zeros((h, w), np.uint8)
        self.lib.sdvl_ref_undistort(ptr(img, u8p), w, h, w, ptr(cam, f64p), ptr(dist, f64p), ptr(out, u8p))
        return out

    def remap_weights(self):
        out = np.zeros(4096, np.int16)
        self.lib.sdvl_ref_remap_weights(out.ctypes.data_as(C.POINTER(C.c_int16)))
        return out.reshape(32, 32, 4)

    # --- alignment
    def image_align(self, img1, img2, cam, px, bearing, depth, valid, T, fast=False):
        img1 = np.ascontiguousarray(img1, np.uint8); img2 = np.ascontiguousarray(img2, np.uint8); h, w = img1.shape
        cam = np.ascontiguousarray(cam, np.float64); px = np.ascontiguousarray(px, np.float64)
        bearing = np.ascontiguousarray(bearing, np.float64); depth = np.ascontiguousarray(depth, np.float64)
        valid = np.ascontiguousarray(valid, np.uint8); T = np.array(T, np.float64)
        err = C.c_double(); chi2 = C.c_double(); its = np.zeros(8, np.int32); stop = C.c_int(); evals = C.c_int()
        n = self.lib.sdvl_ref_image_align_ex(ptr(img1, u8p), ptr(img2, u8p), w, h, C.byref(self.params), ptr(cam, f64p),
                                             len(px), ptr(px, f64p), ptr(bearing, f64p), ptr(depth, f64p), ptr(valid, u8p),
                                             ptr(T, f64p), int(fast), C.byref(err), C.byref(chi2), ptr(its, i32p), C.byref(stop),
                                             C.byref(evals))
        return dict(T=T, n=n, error=err.value, chi2=chi2.value, its=its, stop=stop.value, evals=evals.value)

    def search_point(self, ref_img, cur_img, cam, ref_pose, cur_pose, feat_px, feat_bearing, feat_level, feat_desc,
                     idepth, idepth_std, fixed, corners, px0, use_orb=None):
        """use_orb: None = as self.params says, else this call alone matches with ORB (True) or ZMSSD (False)"""
        params = self.params
        if use_orb is not None:
            params = Params.from_buffer_copy(self.params)
            params.use_orb = int(use_orb)
        ref_img = np.ascontiguousarray(ref_img, np.uint8); cur_img = np.ascontiguousarray(cur_img, np.uint8)
        h, w = ref_img.shape
        cam = np.ascontiguousarray(cam, np.float64)
        ref_pose = np.ascontiguousarray(ref_pose, np.float64); cur_pose = np.ascontiguousarray(cur_pose, np.float64)
        feat_px = np.ascontiguousarray(feat_px, np.float64); feat_bearing = np.ascontiguousarray(feat_bearing, np.float64)
        feat_desc = np.ascontiguousarray(feat_desc, np.uint8); corners = np.ascontiguousarray(corners, np.int32)
        px = np.array(px0, np.float64); lvl = C.c_int(-1); border = np.zeros(100, np.uint8); slevel = C.c_int(-1)
        stage = C.c_int(-1); best = C.c_int(-1)
        found = self.lib.sdvl_ref_search_point_ex(
            ptr(ref_img, u8p), ptr(cur_img, u8p), w, h, C.byref(params), ptr(cam, f64p), ptr(ref_pose, f64p),
            ptr(cur_pose, f64p), ptr(feat_px, f64p), ptr(feat_bearing, f64p), int(feat_level), ptr(feat_desc, u8p),
            C.c_double(idepth), C.c_double(idepth_std), int(fixed), len(corners), ptr(corners, i32p), ptr(px, f64p),
            C.byref(lvl), ptr(border, u8p), C.byref(slevel), C.byref(stage), C.byref(best))
        return dict(found=found, px=px, level=lvl.value, border=border, slevel=slevel.value, stage=stage.value, best_corner=best.value)

    def align_patch(self, img, border, patch, px0, max_its=10):
        img = np.ascontiguousarray(img, np.uint8); h, w = img.shape
        border = np.ascontiguousarray(border, np.uint8); patch = np.ascontiguousarray(patch, np.uint8)
        px = np.array(px0, np.float64)
        ok = self.lib.sdvl_ref_align_patch(ptr(img, u8p), w, h, w, ptr(border, u8p), ptr(patch, u8p), ptr(px, f64p), max_its)
        return ok, px

    # --- tracker
    def tracker(self, w, h, cam, plane=(0, 0, 1, 2.0), first_pose=(1, 0, 0, 0, 0, 0, 0)):
        return OracleTracker(self, w, h, cam, plane, first_pose)


class OracleTracker:
    def __init__(self, orc, w, h, cam, plane, first_pose):
        self.lib = orc.lib
        self.w, self.h = w, h
        cam = np.ascontiguousarray(cam, np.float64); plane = np.ascontiguousarray(plane, np.float64)
        fp = np.ascontiguousarray(first_pose, np.float64)
        self.lib.sdvl_ref_tracker_create.restype = C.c_void_p
        self.h_ = self.lib.sdvl_ref_tracker_create(C.byref(orc.params), w, h, ptr(cam, f64p), ptr(plane, f64p), ptr(fp, f64p))
        self.set_max_keyframes(1000)   # SDVL.max_keyframes of the reference's cfg files, what tracker.configure() sets on the product side

    def handle_frame(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        st = FrameStats()
        self.lib.sdvl_ref_tracker_handle_frame(C.c_void_p(self.h_), ptr(img, u8p), self.w, C.byref(st))
        return st

    def set_max_keyframes(self, n):
        """SDVL.max_keyframes (the plane-map stub honours it like Map::LimitKeyframes, map.cc:190-205)"""
        self.lib.sdvl_ref_tracker_set_max_keyframes(C.c_void_p(self.h_), int(n))

    def use_mapper(self, on=True, max_search_keyframes=5, max_keyframes=100, map_scale=1.0, scale_min_dist=0.25):
        """the reference's mapper in sequential mode (map.cc) instead of the plane map stub"""
        self.lib.sdvl_ref_tracker_use_mapper(C.c_void_p(self.h_), int(on), int(max_search_keyframes), int(max_keyframes),
                                             C.c_double(map_scale), C.c_double(scale_min_dist))

    def depth_filter(self, cur_pose, ref_pose, bearing, found, px, depth_mean, state12):
        """the body of Map::UpdateCandidates' loop behind SearchPoint (map.cc:454-497) for one candidate -> (outcome, new state)"""
        st = np.array(state12, np.float64)
        cp, rp, bv, pp = (np.ascontiguousarray(a, np.float64) for a in (cur_pose, ref_pose, bearing, px))
        self.lib.sdvl_ref_depth_filter.restype = C.c_int
        self.lib.sdvl_ref_depth_filter.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_double, C.c_void_p]
        rc = self.lib.sdvl_ref_depth_filter(C.c_void_p(self.h_), cp.ctypes.data, rp.ctypes.data, bv.ctypes.data, int(found), pp.ctypes.data,
                                            float(depth_mean), st.ctypes.data)
        return rc, st

    def map_stats(self):
        out = np.zeros(6, np.int32)
        self.lib.sdvl_ref_tracker_map_stats(C.c_void_p(self.h_), ptr(out, i32p))
        return dict(zip(("candidates", "converged", "initialized", "linked", "connected", "keyframes"), out.tolist()))

    def mapper_points(self, cap=20000):
        """x y z converged of the live points created by the mapper (bootstrap points excluded)"""
        out = np.zeros((cap, 4), np.float64)
        n = self.lib.sdvl_ref_tracker_mapper_points(C.c_void_p(self.h_), cap, ptr(out, f64p))
        return out[:n].copy()

    def close(self):
        if self.h_:
            self.lib.sdvl_ref_tracker_destroy(C.c_void_p(self.h_)); self.h_ = None

    def __del__(self):
        self.close()


def quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class Synth:
    """Host renderer of the synthetic plane scene (slam-sdvl_amd/csrc/sdvl_synth.h)."""

    def __init__(self):
        self.lib = load_synth()

    def render(self, T_cw, cam, w, h, seed=20260001, frame_id=0, plane=(0, 0, 1, 2.0), texture=0, dist=None):
        """dist = (k1, k2, p1, p2, k3): the view through that lens (what Camera::UndistortImage undoes); None: pinhole"""
        v = SynthView()
        for i in range(5):
            v.dist[i] = float(dist[i]) if dist is not None else 0.0
        v.fx, v.fy, v.u0, v.v0 = [float(c) for c in cam]
        R = quat_to_R(T_cw[:4])
        for i in range(9):
            v.R[i] = float(R.flat[i])
        for i in range(3):
            v.t[i] = float(T_cw[4 + i])
        for i in range(4):
            v.plane[i] = float(plane[i])
        v.seed = seed; v.frame_id = frame_id; v.texture = texture
        out = np.zeros((h, w), np.uint8)
        self.lib.sdvl_synth_render_host(C.byref(v), w, h, ptr(out, u8p), w)
        return out


def quat_rot(q):
    """rotation matrix of a unit quaternion (w, x, y, z)"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_matches(orc, n, seed, outlier_frac=0.25, noise_px=0.4, fx=525.0):
    """n matches of a camera that moved by a small twist: obs rows = ax, ay, px, py, pz, level"""
    rng = np.random.default_rng(seed)
    true_pose = orc.se3_exp(np.array([0.03, -0.02, 0.01, 0.004, -0.006, 0.003]) * (1 + seed % 3))
    guess = orc.se3_exp(np.zeros(6))
    P = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), rng.uniform(1.5, 3.0, n)], 1)
    R = quat_rot(true_pose[:4])
    pc = P @ R.T + true_pose[4:]
    a = pc[:, :2] / pc[:, 2:3] + rng.normal(0, noise_px / fx, (n, 2))
    bad = rng.random(n) < outlier_frac
    a[bad] += rng.uniform(-40, 40, (int(bad.sum()), 2)) / fx
    lvl = rng.integers(0, 3, n)
    obs = np.concatenate([a, P, lvl[:, None].astype(np.float64)], 1)
    return obs, guess


def trajectory_pose(orc, k, xi=XI):
    """T_k = Exp(k * xi) as a world->camera pose (7 doubles)."""
    return orc.se3_exp(np.asarray(xi) * k)


def search_request_meta(orc, img_ref, img_cur, T_ref, T_cur, cam4, n_req, seed, fixed, noise=0.0):
    """SearchPoint requests seeded on the reference frame's corners: points of the plane z = 2 (world = camera 0) searched in the
    current frame.  Inverse depth on the plane (times 1 + noise N(0,1)), idepth_std 5 % of it for fixed requests and 10 % for
    epipolar ones, px0 = the projection + N(0, 0.7 px).  -> (list of dict(px, bearing, level, desc, idepth, istd, px0), corners of
    the current frame)"""
    rng = np.random.default_rng(seed)
    cref = orc.detect_pyramid(img_ref)
    ccur = orc.detect_pyramid(img_cur)
    pyr_ref = orc.pyramid(img_ref, 5)
    sel = rng.choice(len(cref), size=min(n_req, len(cref)), replace=False)
    Tw = orc.se3_inv(T_ref)
    Rw, tw = quat_to_R(Tw[:4]), Tw[4:]
    Rc, tc = quat_to_R(T_cur[:4]), T_cur[4:]
    meta = []
    for ci in sel:
        x, y, l = cref[ci]
        px = np.array([x * (1 << l), y * (1 << l)], np.float64)
        ray = np.array([(px[0] - cam4[2]) / cam4[0], (px[1] - cam4[3]) / cam4[1], 1.0])
        bearing = ray / np.linalg.norm(ray)
        rw = Rw @ bearing
        s = (2.0 - tw[2]) / rw[2]
        desc, _ = orc.orb_describe(pyr_ref[l], [[x, y]])
        idepth = 1.0 / s * (1.0 + noise * rng.normal())
        istd = 0.05 * idepth if fixed else 0.1 * idepth
        Pw = Rw @ (bearing * s) + tw
        pc = Rc @ Pw + tc
        px0 = np.array([cam4[2] + cam4[0] * pc[0] / pc[2], cam4[3] + cam4[1] * pc[1] / pc[2]]) + rng.normal(size=2) * 0.7
        meta.append(dict(px=px, bearing=bearing, level=int(l), desc=desc[0], idepth=idepth, istd=istd, px0=px0))
    return meta, ccur


def fill_search_reqs(sdvl, meta, f_ref, f_cur, T_ref, T_cur, fixed):
    """the SearchReq array of the product for the requests of search_request_meta, between two uploaded frames"""
    reqs = (sdvl.SearchReq * len(meta))()
    for r, m in zip(reqs, meta):
        r.cur, r.ref = f_cur.h.value, f_ref.h.value
        for k in range(7):
            r.cur_pose[k], r.ref_pose[k] = T_cur[k], T_ref[k]
        r.px[0], r.px[1] = m["px"]
        r.bearing[0], r.bearing[1], r.bearing[2] = m["bearing"]
        r.idepth, r.idepth_std = m["idepth"], m["istd"]
        r.px0[0], r.px0[1] = m["px0"]
        r.level, r.fixed = m["level"], int(fixed)
        for k in range(32):
            r.desc[k] = int(m["desc"][k])
    return reqs


# ---- SearchPoint under warps that are far from the identity (tests/test_oracle_warp_independent.py, tests/test_gpu_search_warp.py)
WARP_CAM = np.array([525.0, 525.0, 319.5, 239.5])
_D = np.pi / 180.0
# view -> (twist of the current view in se3_exp's order, the reference view being the identity pose; SearchPoint calls of 120 that
# the ORACLE finds on its own with ORB matching (fixed, epipolar) and with ZMSSD matching (fixed, epipolar), measured on the CPU)
WARP_VIEWS = {
    "roll30": ((0, 0, 0, 0, 0, 30 * _D), (47, 54), (43, 61)),
    "roll90": ((0, 0, 0, 0, 0, 90 * _D), (28, 40), (29, 40)),                                    # I00 ~ 0
    "tilt25": ((0.9, 0, -0.2, 0, -25 * _D, 0), (21, 24), (29, 30)),                              # anisotropic, sheared
    "zoom1.9-roll20": ((0.05, 0, -(2 - 2 / 1.9), 0, 0, 20 * _D), (8, 9), (8, 9)),
    "zoom0.6": ((0, 0, -(2 - 2 / 0.6), 0, 0, 0), (4, 6), (18, 18)),      # det < 1; no corner's patch leaves the image: warp_border_case
}
_warp_views, _warp_cases, _warp_border_cases = {}, {}, {}


def warp_view(orc, synth, view):
    """-> (reference image, current image, reference pose, current pose) of one view, rendered once per session"""
    if view not in _warp_views:
        if "ref" not in _warp_views:
            T_ref = orc.se3_exp(np.zeros(6))
            _warp_views["ref"] = (synth.render(T_ref, WARP_CAM, 640, 480, texture=0), T_ref)
        T_cur = orc.se3_exp(np.array(WARP_VIEWS[view][0], np.float64))
        _warp_views[view] = _warp_views["ref"] + (synth.render(T_cur, WARP_CAM, 640, 480, texture=0), T_cur)
    img_ref, T_ref, img_cur, T_cur = _warp_views[view]
    return img_ref, img_cur, T_ref, T_cur


def warp_view_case(orc, synth, view, fixed, use_orb=True):
    """the 120 requests of one view and the oracle's answer to each, computed once per session and shared (read-only)"""
    key = (view, bool(fixed), bool(use_orb))
    if key not in _warp_cases:
        img_ref, img_cur, T_ref, T_cur = warp_view(orc, synth, view)
        meta, ccur = search_request_meta(orc, img_ref, img_cur, T_ref, T_cur, WARP_CAM, 120, 11, fixed)
        want = [orc.search_point(img_ref, img_cur, WARP_CAM, T_ref, T_cur, m["px"], m["bearing"], m["level"], m["desc"], m["idepth"],
                                 m["istd"], fixed, ccur, m["px0"], use_orb=use_orb) for m in meta]
        listed = WARP_VIEWS[view][1 if use_orb else 2][0 if fixed else 1]
        _warp_cases[key] = dict(img_ref=img_ref, img_cur=img_cur, T_ref=T_ref, T_cur=T_cur, meta=meta, ccur=ccur, want=want,
                                found_floor=listed // 2)
    return _warp_cases[key]


def warp_border_case(orc, synth, view):
    """Requests that are no corners: points 6, 7 and 9 pixels (of their level, 0 to 2) inside each border of the reference image,
    the nearest the margin test of matcher.cc:83 lets through, on the plane, fixed, px0 = their projection into the current view.
    Rolled or spread by 1 / 0.6 their sample grids cross the border of the reference image.  No detected corner lies where such a
    point lands in the current view, so the current frame's corner list is the detected one plus, per request, three corners at
    and next to its projection on each level the request searches: the search then gets as far as the match and the LK.  The oracle
    answers with ZMSSD matching, where the patch's own pixels, the zeroed ones included, pick the corner.  Same keys as
    warp_view_case, shared (read-only)."""
    if view not in _warp_border_cases:
        img_ref, img_cur, T_ref, T_cur = warp_view(orc, synth, view)
        Rc, tc = quat_to_R(T_cur[:4]), T_cur[4:]
        meta, extra = [], []
        for level in range(3):
            rows, cols = 480 >> level, 640 >> level
            ys, xs = range(20, rows - 20, rows // 5), range(20, cols - 20, cols // 5)
            spots = [(d, y) for d in (6, 7, 9) for y in ys] + [(cols - 1 - d, y) for d in (6, 7, 9) for y in ys]
            spots += [(x, d) for d in (6, 7, 9) for x in xs] + [(x, rows - 1 - d) for d in (6, 7, 9) for x in xs]
            spots += [(6, 6), (cols - 7, 6), (6, rows - 7), (cols - 7, rows - 7)]
            for x, y in spots:
                px = np.array([x, y], np.float64) * (1 << level)
                ray = np.array([(px[0] - WARP_CAM[2]) / WARP_CAM[0], (px[1] - WARP_CAM[3]) / WARP_CAM[1], 1.0])
                bearing = ray / np.linalg.norm(ray)
                idepth = bearing[2] / 2.0                         # on the plane z = 2 (the reference pose is the identity)
                pc = Rc @ (bearing / idepth) + tc
                px0 = np.array([WARP_CAM[2] + WARP_CAM[0] * pc[0] / pc[2], WARP_CAM[3] + WARP_CAM[1] * pc[1] / pc[2]])
                meta.append(dict(px=px, bearing=bearing, level=level, desc=np.zeros(32, np.uint8), idepth=idepth, istd=0.05 * idepth, px0=px0))
                for cl in range(max(0, level - 1), min(2, level + 1) + 1):    # the levels a request of this level searches
                    for dx, dy in ((0, 0), (2, 0), (-1, 2)):
                        cx, cy = int(round(px0[0] / (1 << cl))) + dx, int(round(px0[1] / (1 << cl))) + dy
                        if 8 <= cx < (640 >> cl) - 8 and 8 <= cy < (480 >> cl) - 8:
                            extra.append((cx, cy, cl))
        ccur = np.concatenate([orc.detect_pyramid(img_cur), np.array(sorted(set(extra)), np.int32)])
        want = [orc.search_point(img_ref, img_cur, WARP_CAM, T_ref, T_cur, m["px"], m["bearing"], m["level"], m["desc"], m["idepth"],
                                 m["istd"], True, ccur, m["px0"], use_orb=False) for m in meta]
        _warp_border_cases[view] = dict(img_ref=img_ref, img_cur=img_cur, T_ref=T_ref, T_cur=T_cur, meta=meta, ccur=ccur, want=want)
    return _warp_border_cases[view]
