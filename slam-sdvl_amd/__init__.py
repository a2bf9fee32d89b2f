"""slam-sdvl_amd — MI355X-native SDVL tracking front-end (import with importlib.import_module("slam-sdvl_amd")).

Thin ctypes view of the C-ABI in include/sdvl_hip.h (libsdvl_hip.so, hand-written gfx950 kernels).  There is NO
CPU fallback: importing works anywhere the library loads (so that symbol checks run without a GPU), but every
compute entry point needs an MI355X and raises SdvlError otherwise.  Nothing here touches oracle/.
"""
import ctypes as C
import os

import numpy as np

# PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1.  Two HIP runtimes in one process
# fight over the GPU (whichever initialises second sees no device), so when torch is installed it is imported
# FIRST: libsdvl_hip.so then binds to the already-loaded runtime by soname and shares devices and streams with it.
try:
    import torch  # noqa: F401  (plumbing only: runtime sharing, torch.distributed in bench.py)
except ImportError:  # pure C-ABI use without torch: the system ROCm runtime is loaded instead
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libsdvl_hip.so")
HOST_LIB_PATH = os.path.join(_HERE, "host", "libsdvl_host.so")

# enum sdvl_pixel_format
SDVL_GRAY8, SDVL_RGB8, SDVL_BGR8, SDVL_RGBA8, SDVL_BGRA8 = 0, 1, 2, 3, 4
# enum sdvl_raw_format: Bayer mosaics (1 byte per pixel), YUV 4:2:2 and little-endian 16-bit gray (2 bytes per pixel)
SDVL_BAYER_RGGB8, SDVL_BAYER_GRBG8, SDVL_BAYER_GBRG8, SDVL_BAYER_BGGR8 = 16, 17, 18, 19
SDVL_YUYV8, SDVL_UYVY8 = 20, 21
SDVL_GRAY10_16, SDVL_GRAY12_16, SDVL_GRAY16 = 22, 23, 24


def _raw_bytes(im):
    """a camera image as its bytes [h, w, bytes per pixel]: uint8 [h, w] (gray, Bayer) or [h, w, c] (colour, YUYV / UYVY), or uint16
    [h, w] (16-bit gray, stored little-endian)"""
    im = np.asarray(im)
    if im.dtype == np.uint16:
        im = np.ascontiguousarray(im.astype("<u2", copy=False)).view(np.uint8).reshape(im.shape + (2,))
    im = np.ascontiguousarray(im, np.uint8)
    return im[..., None] if im.ndim == 2 else im

MAX_LEVELS = 8
MAX_CORNERS = 6144

u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
f64p = C.POINTER(C.c_double)
f32p = C.POINTER(C.c_float)


class SdvlError(RuntimeError):
    pass


class Camera(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("width", "height", "fx", "fy", "u0", "v0")]


class DetectParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("cell_size", "max_fast_levels", "fast_threshold", "margin")]


class Keypoint(C.Structure):
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("score", C.c_uint8), ("level", C.c_uint8), ("cell", C.c_uint16)]


class AlignFeature(C.Structure):
    _fields_ = [("px", C.c_double), ("py", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("fz", C.c_double),
                ("depth", C.c_double), ("valid", C.c_int32), ("pad_", C.c_int32)]


class AlignJob(C.Structure):
    _fields_ = [("ref", C.c_void_p), ("cur", C.c_void_p), ("feat_begin", C.c_int32), ("feat_end", C.c_int32),
                ("T", C.c_double * 7)]


class AlignParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("max_level", "min_level", "max_its", "patch_size", "fast")]


class AlignResult(C.Structure):
    _fields_ = [("T", C.c_double * 7), ("error", C.c_double), ("chi2", C.c_double), ("n_meas", C.c_int32),
                ("its", C.c_int32 * MAX_LEVELS), ("stop", C.c_int32), ("iters_run", C.c_int32), ("pad_", C.c_int32)]


class SearchParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("patch_size", "max_align_its", "search_size", "max_fast_levels", "margin", "use_orb", "lk_tree_sums", "pad_")]


class SearchReq(C.Structure):
    _fields_ = [("cur", C.c_void_p), ("ref", C.c_void_p), ("cur_pose", C.c_double * 7), ("ref_pose", C.c_double * 7),
                ("px", C.c_double * 2), ("bearing", C.c_double * 3), ("idepth", C.c_double), ("idepth_std", C.c_double),
                ("px0", C.c_double * 2), ("level", C.c_int32), ("fixed", C.c_int32), ("desc", C.c_uint8 * 32)]


class SearchReqPacked(C.Structure):
    """sdvl_search_req_packed: a request of a sdvl_search_begin batch (frames named by slot)"""
    _fields_ = [("cur", C.c_int32), ("ref", C.c_int32), ("level", C.c_int32), ("fixed", C.c_int32), ("px", C.c_double * 2),
                ("bearing", C.c_double * 3), ("idepth", C.c_double), ("idepth_std", C.c_double), ("px0", C.c_double * 2),
                ("desc", C.c_uint8 * 32)]


class ChainFrame(C.Structure):
    _fields_ = [("cand_begin", C.c_int32), ("cand_end", C.c_int32), ("max_matches", C.c_int32), ("rand_begin", C.c_int32),
                ("pose", C.c_double * 7)]


class SearchRes(C.Structure):
    _fields_ = [("px", C.c_double * 2), ("found", C.c_int32), ("level", C.c_int32), ("best_corner", C.c_int32),
                ("stage", C.c_int32), ("lk_its", C.c_int32), ("slevel", C.c_int32)]


class DepthState(C.Structure):
    """sdvl_depth_state: the depth-filter state of the Point behind a candidate request (point.h:136-150)"""
    _fields_ = [("rho", C.c_double), ("sigma2", C.c_double), ("a", C.c_double), ("b", C.c_double), ("z_range", C.c_double),
                ("cos_alpha", C.c_double), ("last_distance", C.c_double), ("depth_mean", C.c_double), ("position", C.c_double * 3),
                ("fixed", C.c_int32), ("n_failed", C.c_int32), ("track_row", C.c_int32), ("pad_", C.c_int32)]


class DepthParams(C.Structure):
    _fields_ = [("px_error_angle", C.c_double), ("min_depth", C.c_double), ("scale_min_dist", C.c_double),
                ("max_failed", C.c_int32), ("pad_", C.c_int32)]


class DepthOut(C.Structure):
    _fields_ = [("outcome", C.c_int32), ("n_failed", C.c_int32), ("rho", C.c_double), ("sigma2", C.c_double), ("a", C.c_double),
                ("b", C.c_double), ("cos_alpha", C.c_double), ("last_distance", C.c_double), ("position", C.c_double * 3)]


# enum sdvl_depth_format and sdvl_depth_seed's status codes
SDVL_DEPTH_F32, SDVL_DEPTH_U16 = 0, 1
DEPTH_SEED_OK, DEPTH_SEED_HOLE, DEPTH_SEED_FEW, DEPTH_SEED_EDGE, DEPTH_SEED_OUTSIDE = 0, 1, 2, 3, 4


class DepthJob(C.Structure):
    """sdvl_depth_job: one registered depth image and the range of the corner list it answers for"""
    _fields_ = [("depth", C.c_void_p), ("on_device", C.c_int32), ("stride", C.c_int32), ("format", C.c_int32), ("pad_", C.c_int32),
                ("scale", C.c_double), ("c_begin", C.c_int32), ("c_end", C.c_int32)]


class DepthSeedParams(C.Structure):
    """sdvl_depth_seed_params: a field that is 0 takes its default (0.05 m, no upper limit, 0.05, 6)"""
    _fields_ = [("min_depth", C.c_double), ("max_depth", C.c_double), ("edge_ratio", C.c_double), ("min_valid", C.c_int32), ("pad_", C.c_int32)]


class DepthMeasureParams(C.Structure):
    """sdvl_depth_measure_params: the lookup's rule and the depth noise tau = noise_abs + noise_quad z^2 (0: 0.001 m, 0.0015 per metre)"""
    _fields_ = [("rule", DepthSeedParams), ("noise_abs", C.c_double), ("noise_quad", C.c_double)]


# sdvl_stereo_depth's status codes (0 .. 4, as depth seeding's) and the format of a right image in the depth image's slot
STEREO_OK, STEREO_NOMATCH, STEREO_AMBIGUOUS, STEREO_EDGE, STEREO_OUTSIDE = 0, 1, 2, 3, 4
SDVL_DEPTH_RIGHT8 = 2


class StereoJob(C.Structure):
    """sdvl_stereo_job: a left frame, the rectified right image of the pair and the range of the corner list they answer for"""
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("on_device", C.c_int32), ("stride", C.c_int32), ("c_begin", C.c_int32),
                ("c_end", C.c_int32)]


class StereoParams(C.Structure):
    """sdvl_stereo_params: the baseline, and the rule — a field that is 0 takes its default (0.3 m, no upper limit, 192, 20, 80)"""
    _fields_ = [("baseline", C.c_double), ("min_depth", C.c_double), ("max_depth", C.c_double), ("max_disparity", C.c_int32),
                ("max_sad", C.c_int32), ("uniqueness", C.c_int32), ("pad_", C.c_int32), ("dist", C.c_void_p)]


class StereoMeasureParams(C.Structure):
    """sdvl_stereo_measure_params: the matcher's rule and the disparity noise in pixels (0: 0.25 px, not measured against a real pair)"""
    _fields_ = [("rule", StereoParams), ("disparity_sigma", C.c_double)]


class SynthView(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("u0", C.c_double), ("v0", C.c_double),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("plane", C.c_double * 4),
                ("seed", C.c_uint32), ("frame_id", C.c_uint32), ("texture", C.c_uint32), ("reserved_", C.c_uint32),
                ("dist", C.c_double * 5)]


SYNTH_MAX_SURFACES = 8
SYNTH_NO_SURFACE = 255
SYNTH_SCENE_MAX_VIEWS = 4096


class SynthSurface(C.Structure):
    """sdvl_synth_surface: a textured plane n.X = d, unbounded or a rectangle of half extents (half_u, half_v) along (e1, e2) about origin"""
    _fields_ = [("plane", C.c_double * 4), ("origin", C.c_double * 3), ("e1", C.c_double * 3), ("e2", C.c_double * 3),
                ("half_u", C.c_double), ("half_v", C.c_double), ("seed_add", C.c_uint32), ("pad_", C.c_uint32)]


class SynthScene(C.Structure):
    """sdvl_synth_scene: the camera, pose, seeds and lens of SynthView and up to SYNTH_MAX_SURFACES surfaces"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("u0", C.c_double), ("v0", C.c_double),
                ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("seed", C.c_uint32), ("frame_id", C.c_uint32), ("texture", C.c_uint32), ("n_surfaces", C.c_uint32),
                ("dist", C.c_double * 5), ("surfaces", SynthSurface * SYNTH_MAX_SURFACES)]


# every symbol include/sdvl_hip.h declares
ABI_SYMBOLS = [
    "sdvl_ctx_create", "sdvl_ctx_destroy", "sdvl_last_error", "sdvl_ctx_synchronize", "sdvl_ctx_stream",
    "sdvl_ctx_bind_thread", "sdvl_ctx_device", "sdvl_pointer_device", "sdvl_ctx_scratch_device",
    "sdvl_ctx_timing_enable", "sdvl_ctx_timing_only", "sdvl_ctx_timing_get", "sdvl_ctx_timing_reset",
    "sdvl_frame_create", "sdvl_frame_create_many", "sdvl_frame_destroy", "sdvl_frame_upload", "sdvl_frames_upload", "sdvl_ctx_prefetch_images", "sdvl_ctx_prefetch_fence", "sdvl_frame_set_image_device", "sdvl_frame_borrow_image_device",
    "sdvl_pyramid_build", "sdvl_frame_download_level", "sdvl_fast_num_cells", "sdvl_cell_kp_cap", "sdvl_fast_cells",
    "sdvl_detect_corners", "sdvl_frames_corner_counts", "sdvl_frame_download_corners", "sdvl_retain_best",
    "sdvl_frame_set_corners", "sdvl_frames_set_corners", "sdvl_frame_num_corners", "sdvl_shi_tomasi", "sdvl_orb_describe",
    "sdvl_frame_download_descriptors", "sdvl_filter_inputs", "sdvl_filter_inputs_begin", "sdvl_filter_inputs_end", "sdvl_filter_corners_begin", "sdvl_filter_corners_end", "sdvl_orb_describe_points", "sdvl_hamming_argmin", "sdvl_image_align", "sdvl_image_align_begin", "sdvl_image_align_end", "sdvl_align_store_create", "sdvl_align_store_destroy", "sdvl_align_store_write", "sdvl_image_align_begin_stored", "sdvl_search_points", "sdvl_search_begin", "sdvl_search_slot", "sdvl_search_run", "sdvl_align_patches", "sdvl_pose_from_matches", "sdvl_search_points_filter", "sdvl_search_run_filter", "sdvl_depth_filter", "sdvl_search_run_chain", "sdvl_search_chain_end", "sdvl_frame_footprint", "sdvl_undistort", "sdvl_frames_upload_undistorted", "sdvl_convert_gray", "sdvl_frames_upload_color", "sdvl_depth_seed", "sdvl_depth_lookup", "sdvl_depth_stage_begin", "sdvl_depth_stage_end", "sdvl_stereo_depth", "sdvl_stereo_lookup", "sdvl_depth_filter_measured", "sdvl_search_run_filter_measured", "sdvl_depth_filter_stereo", "sdvl_search_run_filter_stereo", "sdvl_ctx_set_wait_hook", "sdvl_ctx_wait_done", "sdvl_ctx_wait_block", "sdvl_ctx_health", "sdvl_ctx_counters",
    "sdvl_track_create", "sdvl_track_destroy", "sdvl_frame_register", "sdvl_frames_register", "sdvl_track_upload", "sdvl_track_append", "sdvl_track_align", "sdvl_track_search",
    "sdvl_track_collect", "sdvl_track_features", "sdvl_track_stats",
    "sdvl_synth_render", "sdvl_synth_render_scene", "sdvl_synth_scene_size", "sdvl_synth_scene_preset", "sdvl_synth_scene_preset_names",
    "sdvl_device_malloc", "sdvl_device_free", "sdvl_device_download",
    "sdvl_frames_own_images", "sdvl_feed_create", "sdvl_feed_destroy", "sdvl_feed_last_error", "sdvl_feed_slot_arrived", "sdvl_feed_images", "sdvl_ctx_feed_acquire", "sdvl_ctx_feed_release", "sdvl_frame_footprint_cap", "sdvl_ctx_set_corner_capacity", "sdvl_frame_corner_capacity", "sdvl_detect_scratch_bytes",
    "sdvl_klt_track", "sdvl_homography_ransac", "sdvl_bundle_adjust", "sdvl_bundle_adjust_depth",
    "sdvl_stereo_rectify_plan", "sdvl_stereo_rectify_plan_message", "sdvl_rectify", "sdvl_frames_upload_rectified",
    "sdvl_frames_upload_color_rectified", "sdvl_rectify_stats", "sdvl_rectify_map_words",
    "sdvl_ctx_set_wait_spin", "sdvl_ctx_fork_mark", "sdvl_ctx_fork_begin", "sdvl_ctx_fork_end", "sdvl_host_alloc_pinned", "sdvl_host_free_pinned", "sdvl_host_register", "sdvl_host_unregister",
]

_lib = None


def load_library():
    """dlopen libsdvl_hip.so; raises SdvlError (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SdvlError("libsdvl_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`"
                            % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.sdvl_last_error.restype = C.c_char_p
        lib.sdvl_last_error.argtypes = [C.c_void_p]
        lib.sdvl_ctx_stream.restype = C.c_void_p
        lib.sdvl_ctx_stream.argtypes = [C.c_void_p]
        lib.sdvl_bundle_adjust.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sdvl_bundle_adjust_depth.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sdvl_synth_scene_preset.argtypes = [C.c_char_p, C.c_void_p]
        lib.sdvl_synth_scene_preset_names.restype = C.c_char_p
        lib.sdvl_synth_render_scene.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib = lib
    return _lib


def synth_scene_presets():
    """the names sdvl_synth_scene_preset knows"""
    return load_library().sdvl_synth_scene_preset_names().decode().split()


def synth_scene(T_cw, cam, preset=None, seed=20260001, frame_id=0, texture=0, dist=None):
    """a SynthScene seen from the world -> camera pose T_cw (qw, qx, qy, qz, tx, ty, tz) by the camera cam = (fx, fy, u0, v0), through the
    lens dist = (k1, k2, p1, p2, k3) if given; its surfaces are those of the named preset (sdvl_synth_scene_preset), none without a name"""
    s = SynthScene()
    s.fx, s.fy, s.u0, s.v0 = [float(c) for c in cam]
    w, x, y, z = [float(q) for q in T_cw[:4]]
    R = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    for i in range(9):
        s.R[i] = R[i]
    for i in range(3):
        s.t[i] = float(T_cw[4 + i])
    for i in range(5):
        s.dist[i] = float(dist[i]) if dist is not None else 0.0
    s.seed, s.frame_id, s.texture = int(seed), int(frame_id), int(texture)
    if preset is not None:
        if load_library().sdvl_synth_scene_preset(preset.encode(), C.byref(s)) != 0:
            raise ValueError("unknown scene preset %r (one of %s)" % (preset, ", ".join(synth_scene_presets())))
    return s


def _ptr(a, t):
    return a.ctypes.data_as(t)


class Frame:
    """Device-resident Frame (pyramid + corners + descriptors) behind an sdvl_frame handle."""

    def __init__(self, ctx, width, height, levels=5):
        self.ctx = ctx
        self.width, self.height, self.levels = width, height, levels
        h = C.c_void_p()
        ctx._check(ctx.lib.sdvl_frame_create(ctx.h, width, height, levels, C.byref(h)))
        self.h = h

    def upload(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.shape == (self.height, self.width)
        self._keep = img
        self.ctx._check(self.ctx.lib.sdvl_frame_upload(self.ctx.h, self.h, _ptr(img, u8p), self.width))
        return self

    def set_image_device(self, dev_ptr, stride=None):
        self.ctx._check(self.ctx.lib.sdvl_frame_set_image_device(self.ctx.h, self.h, C.c_void_p(dev_ptr), stride or self.width))
        return self

    def borrow_image_device(self, dev_ptr):
        """level 0 aliases the caller's HBM image (dense rows) until the next upload / own_images"""
        self.ctx._check(self.ctx.lib.sdvl_frame_borrow_image_device(self.ctx.h, self.h, C.c_void_p(dev_ptr)))
        return self

    def corner_capacity(self):
        return self.ctx.lib.sdvl_frame_corner_capacity(self.h)

    def level(self, l):
        w, h = self.width >> l, self.height >> l
        out = np.zeros((h, w), np.uint8)
        self.ctx._check(self.ctx.lib.sdvl_frame_download_level(self.ctx.h, self.h, l, _ptr(out, u8p), w))
        return out

    def set_corners(self, xyl):
        xyl = np.ascontiguousarray(xyl, np.int32).reshape(-1, 3)
        self.ctx._check(self.ctx.lib.sdvl_frame_set_corners(self.ctx.h, self.h, len(xyl), _ptr(xyl, i32p)))
        return self

    def descriptors(self, cap=MAX_CORNERS):
        """host mirror of the frame's ORB descriptors, [n_corners][32] (computed now if they have not been)"""
        out = np.zeros((cap, 32), np.uint8)
        n = (C.c_int32 * 1)()
        hs = (C.c_void_p * 1)(self.h)
        self.ctx._check(self.ctx.lib.sdvl_frames_corner_counts(self.ctx.h, 1, hs, n))
        self.ctx._check(self.ctx.lib.sdvl_frame_download_descriptors(self.ctx.h, self.h, cap, _ptr(out, u8p)))
        return out[:n[0]]

    def close(self):
        if self.h:
            self.ctx.lib.sdvl_frame_destroy(self.ctx.h, self.h)
            self.h = None



class AlignStore:
    """sdvl_align_store: alignment feature records kept in HBM (Relocalize aligns every frame against the same keyframes)"""

    def __init__(self, ctx, capacity):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.sdvl_align_store_create(ctx.h, int(capacity), C.byref(h)))
        self.h = h

    def write(self, offset, feats, begin=0, end=None):
        """records [offset, offset + end - begin) of the store <- feats[begin:end] (an AlignFeature array)"""
        end = len(feats) if end is None else end
        src = C.byref(feats, begin * C.sizeof(AlignFeature))
        self.ctx._check(self.ctx.lib.sdvl_align_store_write(self.ctx.h, self.h, int(offset), int(end - begin), src))

    def close(self):
        if self.h:
            self.ctx._check(self.ctx.lib.sdvl_align_store_destroy(self.ctx.h, self.h))
            self.h = None


class Distortion(C.Structure):
    _fields_ = [("d", C.c_double * 5)]


class StereoRig(C.Structure):
    """sdvl_stereo_rig: K1, D1 (left), K2, D2 (right), R, T with X_right = R X_left + T"""
    _fields_ = [("left", Camera), ("left_dist", Distortion), ("right", Camera), ("right_dist", Distortion), ("R", C.c_double * 9),
                ("T", C.c_double * 3)]


class Rectification(C.Structure):
    """sdvl_rectification: one camera of a rectified pair (raw K and D, its rotation R_i, the rectified camera)"""
    _fields_ = [("raw", Camera), ("dist", Distortion), ("R", C.c_double * 9), ("rect", Camera)]


class StereoRectified(C.Structure):
    """sdvl_stereo_rectified: the plan's output"""
    _fields_ = [("left", Rectification), ("right", Rectification), ("baseline", C.c_double)]

    def camera(self):
        """the rectified camera (fx, fy, u0, v0), the same for both images"""
        c = self.left.rect
        return np.array([c.fx, c.fy, c.u0, c.v0])


class RectifyPlanError(SdvlError):
    """sdvl_stereo_rectify_plan refused the rig; `code` is its sdvl_rectify_plan_error"""

    def __init__(self, code, message):
        SdvlError.__init__(self, message)
        self.code = code


def rectification(raw, dist, R, rect, width=0, height=0):
    """a Rectification from raw = (fx, fy, u0, v0), dist = (k1, k2, p1, p2, k3), R [3][3] and rect = (fx, fy, u0, v0)"""
    r = Rectification()
    r.raw = Camera(float(width), float(height), *[float(v) for v in raw])
    r.dist = Distortion((C.c_double * 5)(*[float(v) for v in dist]))
    r.R = (C.c_double * 9)(*[float(v) for v in np.asarray(R, np.float64).reshape(9)])
    r.rect = Camera(float(width), float(height), *[float(v) for v in rect])
    return r


def stereo_rectify_plan(K1, D1, K2, D2, R, T, width, height, override=None):
    """sdvl_stereo_rectify_plan (host code, no device): the calibrated rig K_i = (fx, fy, u0, v0), D_i = (k1, k2, p1, p2, k3), R [3][3],
    T [3] with X_right = R X_left + T -> StereoRectified; `override` = (fx, fy, u0, v0) sets the rectified intrinsics.  Raises
    RectifyPlanError for a rig the plan refuses."""
    lib = load_library()
    lib.sdvl_stereo_rectify_plan_message.restype = C.c_char_p
    rig = StereoRig()
    rig.left = Camera(float(width), float(height), *[float(v) for v in K1])
    rig.right = Camera(float(width), float(height), *[float(v) for v in K2])
    rig.left_dist = Distortion((C.c_double * 5)(*[float(v) for v in D1]))
    rig.right_dist = Distortion((C.c_double * 5)(*[float(v) for v in D2]))
    rig.R = (C.c_double * 9)(*[float(v) for v in np.asarray(R, np.float64).reshape(9)])
    rig.T = (C.c_double * 3)(*[float(v) for v in np.asarray(T, np.float64).reshape(3)])
    ov = Camera(float(width), float(height), *[float(v) for v in override]) if override is not None else None
    out = StereoRectified()
    rc = lib.sdvl_stereo_rectify_plan(C.byref(rig), int(width), int(height), C.byref(ov) if ov is not None else None, C.byref(out))
    if rc != 0:
        raise RectifyPlanError(rc, lib.sdvl_stereo_rectify_plan_message(rc).decode())
    return out


class PoseObs(C.Structure):
    _fields_ = [("ax", C.c_double), ("ay", C.c_double), ("px", C.c_double), ("py", C.c_double), ("pz", C.c_double), ("inv_cov", C.c_double)]


class PoseJob(C.Structure):
    _fields_ = [("obs_begin", C.c_int32), ("obs_end", C.c_int32), ("rand_begin", C.c_int32), ("nits_begin", C.c_int32), ("pose", C.c_double * 7)]


class PoseParams(C.Structure):
    _fields_ = [("max_ransac_points", C.c_int32), ("max_ransac_its", C.c_int32), ("max_optim_pose_its", C.c_int32), ("pad_", C.c_int32),
                ("inlier_threshold", C.c_double), ("fx", C.c_double)]


class PoseResult(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("n_draws", C.c_int32), ("n_inliers", C.c_int32), ("n_outliers", C.c_int32), ("refined", C.c_int32)]


class KltJob(C.Structure):
    """sdvl_klt_job: a pair of frames (same size, pyramids built) and a range of the call's points"""
    _fields_ = [("prev", C.c_void_p), ("next", C.c_void_p), ("pt_begin", C.c_int32), ("pt_end", C.c_int32)]


class KltParams(C.Structure):
    _fields_ = [("win_size", C.c_int32), ("max_level", C.c_int32), ("max_its", C.c_int32), ("pad_", C.c_int32),
                ("eps", C.c_double), ("min_eig_threshold", C.c_double)]


class HomographyJob(C.Structure):
    _fields_ = [("m_begin", C.c_int32), ("m_end", C.c_int32), ("draw_begin", C.c_int32), ("draw_end", C.c_int32)]


class HomographyResult(C.Structure):
    _fields_ = [("H", C.c_double * 9), ("best_draw", C.c_int32), ("n_its", C.c_int32), ("n_inliers", C.c_int32), ("pad_", C.c_int32)]


class BundleProblem(C.Structure):
    """sdvl_bundle_problem: ranges of one local window in the call's poses (free ones first), points and edges"""
    _fields_ = [("kf_begin", C.c_int32), ("kf_end", C.c_int32), ("pt_begin", C.c_int32), ("pt_end", C.c_int32),
                ("edge_begin", C.c_int32), ("edge_end", C.c_int32)]


class BundleEdge(C.Structure):
    _fields_ = [("point", C.c_int32), ("keyframe", C.c_int32), ("u", C.c_double), ("v", C.c_double)]


class BundleEdgeDepth(C.Structure):
    """sdvl_bundle_edge_depth: depth = the measured camera-frame z of the observation in metres, <= 0: none"""
    _fields_ = [("point", C.c_int32), ("keyframe", C.c_int32), ("u", C.c_double), ("v", C.c_double), ("depth", C.c_double)]


class BundleStage(C.Structure):
    _fields_ = [("lam", C.c_double), ("chi2_before", C.c_double), ("chi2_after", C.c_double), ("iterations", C.c_int32),
                ("trials", C.c_int32), ("accepted_mask", C.c_int32), ("pad_", C.c_int32), ("trials_per_it", C.c_int32 * 10)]


class BundleResult(C.Structure):
    _fields_ = [("stage", BundleStage * 2), ("status", C.c_int32), ("n_level1", C.c_int32), ("n_free", C.c_int32), ("pad_", C.c_int32)]


class TrackPoint(C.Structure):
    """sdvl_track_point: what the tracked step reads of one Point; ref is the handle of a registered Frame"""
    _fields_ = [("position", C.c_double * 3), ("px", C.c_double * 2), ("bearing", C.c_double * 3), ("idepth", C.c_double),
                ("idepth_std", C.c_double), ("ref", C.c_void_p), ("level", C.c_int32), ("fixed", C.c_int32), ("score", C.c_int32),
                ("n_failed", C.c_int32), ("last_frame", C.c_int32), ("status", C.c_int32), ("desc", C.c_uint8 * 32)]


class TrackFeature(C.Structure):
    """sdvl_track_feature: one feature of last_frame; point = row of its point, -1 = none, | TRACK_DUPLICATE = seen earlier in the list"""
    _fields_ = [("px", C.c_double * 2), ("bearing", C.c_double * 3), ("level", C.c_int32), ("point", C.c_int32)]


TRACK_DUPLICATE = 0x40000000


class TrackParams(C.Structure):
    _fields_ = [("align", AlignParams), ("search", SearchParams), ("pose", PoseParams), ("cell_size", C.c_int32), ("patch_size", C.c_int32),
                ("max_failed", C.c_int32), ("pad_", C.c_int32)]


class TrackJob(C.Structure):
    _fields_ = [("tracker", C.c_int32), ("feat_buf", C.c_int32), ("last", C.c_void_p), ("cur", C.c_void_p), ("T", C.c_double * 7),
                ("last_pose", C.c_double * 7), ("frame_id", C.c_int32), ("max_matches", C.c_int32)]


class TrackResult(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("align_error", C.c_double), ("scene_depth", C.c_double)] + [(n, C.c_int32) for n in (
        "align_meas", "align_iters", "n_features", "n_requests", "matches", "attempts", "n_draws", "n_inliers", "n_outliers", "refined",
        "n_points", "n_deleted", "lk_iters", "n_corners", "status")]


class TrackFeatureOut(C.Structure):
    _fields_ = [("px", C.c_double * 2), ("level", C.c_int32), ("point", C.c_int32)]


class TrackPointStat(C.Structure):
    _fields_ = [("score", C.c_int32), ("n_failed", C.c_int32), ("last_frame", C.c_int32), ("status", C.c_int32)]


class TrackSet:
    """sdvl_track_set: the device-resident tracking tables of n trackers and the tracked step on them (include/sdvl_hip.h)"""

    def __init__(self, ctx, n_trackers, max_points, max_features, grid_cells, max_matches, max_ransac_its):
        self.ctx = ctx
        self.n, self.cells, self.max_ransac_its = int(n_trackers), int(grid_cells), int(max_ransac_its)
        h = C.c_void_p()
        ctx._check(ctx.lib.sdvl_track_create(ctx.h, self.n, int(max_points), int(max_features), self.cells, int(max_matches),
                                             self.max_ransac_its, C.byref(h)))
        self.h = h
        self.n_points = {}      # tracker -> point rows its table holds (sdvl_track_stats returns that many)
        ctx.lib.sdvl_track_features.restype = C.POINTER(TrackFeatureOut)
        ctx.lib.sdvl_track_features.argtypes = [C.c_void_p, C.c_int]
        ctx.lib.sdvl_track_stats.restype = C.POINTER(TrackPointStat)
        ctx.lib.sdvl_track_stats.argtypes = [C.c_void_p, C.c_int]

    def _rows(self, fn, trackers, feat_buf, points, features):
        """points / features: per named tracker a list (or ctypes array) of TrackPoint / TrackFeature rows"""
        n = len(trackers)
        assert len(feat_buf) == len(points) == len(features) == n
        tr, fb = np.asarray(trackers, np.int32), np.asarray(feat_buf, np.int32)
        npt, nft = np.asarray([len(p) for p in points], np.int32), np.asarray([len(f) for f in features], np.int32)
        pa = (TrackPoint * max(int(npt.sum()), 1))(*[r for p in points for r in p])
        fa = (TrackFeature * max(int(nft.sum()), 1))(*[r for f in features for r in f])
        # (the rows are staged before the call returns: nothing has to outlive it)
        self.ctx._check(fn(self.ctx.h, self.h, n, _ptr(tr, i32p), _ptr(fb, i32p), _ptr(npt, i32p), pa, _ptr(nft, i32p), fa))
        return tr.tolist(), npt.tolist()

    def upload(self, trackers, feat_buf, points, features):
        """sdvl_track_upload: the tables of the named trackers are replaced"""
        for t, k in zip(*self._rows(self.ctx.lib.sdvl_track_upload, trackers, feat_buf, points, features)):
            self.n_points[t] = k

    def append(self, trackers, feat_buf, points, features):
        """sdvl_track_append: the rows go behind the rows the tables hold"""
        for t, k in zip(*self._rows(self.ctx.lib.sdvl_track_append, trackers, feat_buf, points, features)):
            self.n_points[t] = self.n_points.get(t, 0) + k

    def step(self, jobs, cell_rank, rand_raw, cam, params, between=None):
        """sdvl_track_align, the `between` callable (corners of the new frames: detect or set them there), sdvl_track_search and
        sdvl_track_collect.  jobs: TrackJob array; cell_rank [n_jobs][grid_cells]; rand_raw [n_jobs][max_ransac_its].
        -> (TrackResult array, per job the new frame's features [matches] and the point statistics [n_points], as numpy copies)"""
        n = len(jobs)
        lib = self.ctx.lib
        rank = np.ascontiguousarray(cell_rank, np.uint16).reshape(n, self.cells)
        raw = np.ascontiguousarray(rand_raw, np.int32).reshape(n, self.max_ransac_its)
        n_points = [self.n_points.get(jobs[j].tracker, 0) for j in range(n)]
        self.ctx._check(lib.sdvl_track_align(self.ctx.h, self.h, n, jobs, _ptr(rank, C.POINTER(C.c_uint16)), _ptr(raw, i32p), C.byref(cam),
                                             C.byref(params)))
        if between is not None:
            between()
        self.ctx._check(lib.sdvl_track_search(self.ctx.h, self.h))
        res = (TrackResult * n)()
        self.ctx._check(lib.sdvl_track_collect(self.ctx.h, self.h, n, res))
        feat_t = np.dtype([("px", "<f8", 2), ("level", "<i4"), ("point", "<i4")])
        stat_t = np.dtype([("score", "<i4"), ("n_failed", "<i4"), ("last_frame", "<i4"), ("status", "<i4")])
        feats, stats = [], []
        for j in range(n):
            fp, sp = lib.sdvl_track_features(self.h, j), lib.sdvl_track_stats(self.h, j)
            feats.append(np.ctypeslib.as_array(C.cast(fp, u8p), (res[j].matches * C.sizeof(TrackFeatureOut),)).view(feat_t).copy()
                         if res[j].matches else np.zeros(0, feat_t))
            stats.append(np.ctypeslib.as_array(C.cast(sp, u8p), (n_points[j] * C.sizeof(TrackPointStat),)).view(stat_t).copy()
                         if n_points[j] else np.zeros(0, stat_t))
        return res, feats, stats

    def close(self):
        if self.h:
            self.ctx._check(self.ctx.lib.sdvl_track_destroy(self.ctx.h, self.h))
            self.h = None


BUNDLE_MAX_FREE = 16
BUNDLE_OK, BUNDLE_EMPTY, BUNDLE_NO_EDGES, BUNDLE_NONFINITE = 0, 1, 2, 3


def ransac_budget_table(size, max_points, max_its):
    """iteration budget after an improvement to s supporters, s = 0..size (feature_align.cc:199-207)"""
    import math
    npoints = min(max_points, size)
    out = []
    for s in range(size + 1):
        nits = max_its
        if size > 0:
            tmp = 1.0 - (1.0 - (float(s) / float(size)))
            for _ in range(1, npoints):
                tmp *= tmp
            if not tmp < 1e-5:
                den = math.log(1.0 - tmp) if tmp < 1.0 else -math.inf
                nits = min(max_its, int(math.log(1.0 - 0.99) / den))
        out.append(nits)
    return out

class Context:
    """One sdvl_ctx = one HIP stream on one MI355X."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.sdvl_ctx_create(device, C.byref(h))
        if rc != 0:
            raise SdvlError("sdvl_ctx_create(device=%d) failed with %d: no MI355X visible; there is no CPU fallback" % (device, rc))
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise SdvlError("sdvl error %d: %s" % (rc, self.lib.sdvl_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.lib.sdvl_ctx_destroy(self.h)
            self.h = None

    def stream(self):
        return self.lib.sdvl_ctx_stream(self.h)

    def synchronize(self):
        self._check(self.lib.sdvl_ctx_synchronize(self.h))

    # ---- timing
    def timing_enable(self, on=True):
        self._check(self.lib.sdvl_ctx_timing_enable(self.h, int(on)))

    def timing_only(self, name=None):
        """time only the launches of kernel `name`; None = every launch"""
        self.lib.sdvl_ctx_timing_only.argtypes = [C.c_void_p, C.c_char_p]
        self._check(self.lib.sdvl_ctx_timing_only(self.h, name.encode() if name else None))

    def timing_reset(self):
        self._check(self.lib.sdvl_ctx_timing_reset(self.h))

    def timing_get(self):
        names = ((C.c_char * 32) * 32)()
        ms = (C.c_double * 32)()
        launches = (C.c_int64 * 32)()
        n = C.c_int()
        self._check(self.lib.sdvl_ctx_timing_get(self.h, 32, names, ms, launches, C.byref(n)))
        return {names[i].value.decode(): (ms[i], launches[i]) for i in range(n.value)}

    # ---- frames
    def frame(self, img=None, width=None, height=None, levels=5, pyramid=True):
        if img is not None:
            height, width = img.shape
        f = Frame(self, width, height, levels)
        if img is not None:
            f.upload(img)
            if pyramid:
                self.pyramid_build([f])
        return f

    def pyramid_build(self, frames):
        arr = (C.c_void_p * len(frames))(*[f.h for f in frames])
        self._check(self.lib.sdvl_pyramid_build(self.h, len(frames), arr))

    def set_corner_capacity(self, max_corners):
        """corners_ capacity of the frames created from now on (<= MAX_CORNERS)"""
        self._check(self.lib.sdvl_ctx_set_corner_capacity(self.h, int(max_corners)))

    def own_images(self, frames):
        """frames whose level 0 aliases a caller image copy it into their own storage (one launch)"""
        arr = (C.c_void_p * len(frames))(*[f.h for f in frames])
        self._check(self.lib.sdvl_frames_own_images(self.h, len(frames), arr))

    def fast_cells(self, frames, dp, cap=None):
        """-> list of (keypoints[(x,y,score,level,cell)], cell_offsets) per frame.  cap = keypoints per frame; None: as many as
        the cells can hold (cells x sdvl_cell_kp_cap) — a fixed default refused the denser grids of small cells"""
        n = len(frames)
        cpl = (C.c_int * 4)()
        tot = C.c_int()
        self._check(self.lib.sdvl_fast_num_cells(frames[0].width, frames[0].height, C.byref(dp), cpl, C.byref(tot)))
        if cap is None:
            cap = max(1, tot.value * self.lib.sdvl_cell_kp_cap(dp.cell_size))
        kps = (Keypoint * (n * cap))()
        offs = np.zeros((n, tot.value + 1), np.int32)
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        self._check(self.lib.sdvl_fast_cells(self.h, n, arr, C.byref(dp), cap, kps, _ptr(offs, i32p)))
        raw = np.frombuffer(kps, dtype=np.dtype([("x", "<u2"), ("y", "<u2"), ("score", "u1"), ("level", "u1"), ("cell", "<u2")]))
        out = []
        for i in range(n):
            k = raw[i * cap: i * cap + offs[i, -1]]
            out.append((np.stack([k["x"], k["y"], k["score"], k["level"], k["cell"]], 1).astype(np.int32), offs[i].copy()))
        return out, [cpl[i] for i in range(dp.max_fast_levels)]

    def detect_corners(self, frames, dp, nfeatures=1000):
        """DetectPyramid fully on device -> list of corners [(x, y, level)] per frame"""
        n = len(frames)
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        self._check(self.lib.sdvl_detect_corners(self.h, n, arr, C.byref(dp), nfeatures))
        counts = np.zeros(n, np.int32)
        self._check(self.lib.sdvl_frames_corner_counts(self.h, n, arr, _ptr(counts, i32p)))
        out = []
        for f, c in zip(frames, counts):
            xyl = np.zeros((max(int(c), 1), 3), np.int32)
            k = C.c_int()
            self._check(self.lib.sdvl_frame_download_corners(self.h, f.h, len(xyl), _ptr(xyl, i32p), C.byref(k)))
            out.append(xyl[:k.value].copy())
        return out

    def retain_best(self, packed, n_points, cooperative=0):
        """cooperative: 0 = one lane, 2 = the 8-lane group of select_cells, 3 = one wave as in select_pack; 1 (the retired workgroup
        form) and every other value raise SdvlError"""
        packed = np.ascontiguousarray(packed, np.uint32).copy()
        k = C.c_int()
        self._check(self.lib.sdvl_retain_best(self.h, _ptr(packed, C.POINTER(C.c_uint32)), len(packed), int(n_points), int(cooperative),
                                              C.byref(k)))
        return packed[:k.value]

    def shi_tomasi(self, frames, cap=MAX_CORNERS):
        n = len(frames)
        out = np.zeros((n, cap), np.float64)
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        self._check(self.lib.sdvl_shi_tomasi(self.h, n, arr, cap, _ptr(out, f64p)))
        return [out[i, :self.lib.sdvl_frame_num_corners(frames[i].h)].copy() for i in range(n)]

    def orb_describe(self, frames, want=True, cap=MAX_CORNERS):
        n = len(frames)
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        if not want:
            self._check(self.lib.sdvl_orb_describe(self.h, n, arr, cap, None))
            return None
        out = np.zeros((n, cap, 32), np.uint8)
        self._check(self.lib.sdvl_orb_describe(self.h, n, arr, cap, _ptr(out, u8p)))
        return [out[i, :self.lib.sdvl_frame_num_corners(frames[i].h)].copy() for i in range(n)]

    def filter_corners(self, frames, locked_px, cell_size=32, margin=19, min_feature_score=50):
        """sdvl_filter_corners_begin / _end: Frame::FilterCorners for the frames, selection on the device.  locked_px[i] = (k, 2)
        positions whose cells are locked (FastDetector::LockCell).  Returns per frame (indices, xyl, scores, descriptors)."""
        n = len(frames)
        w, h = frames[0].width, frames[0].height
        gw, gh = (w + cell_size - 1) // cell_size, (h + cell_size - 1) // cell_size
        words = (gw * gh + 31) // 32
        mask = np.zeros((n, words), np.uint32)
        for i, pts in enumerate(locked_px):
            for x, y in np.asarray(pts, np.float64).reshape(-1, 2):
                c = int(y / cell_size) * gw + int(x / cell_size)
                mask[i, c >> 5] |= np.uint32(1 << (c & 31))
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        self._check(self.lib.sdvl_filter_corners_begin(self.h, n, arr, mask.ctypes.data_as(C.POINTER(C.c_uint32)), words, cell_size, margin,
                                                       min_feature_score, 1))
        cap = gw * gh
        counts = np.zeros(n, np.int32)
        rec = np.zeros((n, cap, 14), np.int32)      # 56-byte records: index, x, y, level, score, pad, desc[32]
        self._check(self.lib.sdvl_filter_corners_end(self.h, n, cap, _ptr(counts, i32p), rec.ctypes.data_as(C.c_void_p)))
        out = []
        for i in range(n):
            r = rec[i, :counts[i]]
            out.append((r[:, 0].copy(), r[:, 1:4].copy(), r[:, 4].copy(), r[:, 6:].copy().view(np.uint8).reshape(-1, 32)))
        return out

    def filter_inputs(self, frames, cap=MAX_CORNERS, with_desc=True):
        """sdvl_filter_inputs: what Frame::FilterCorners needs from the frames in one round trip.  Returns per frame (xyl, scores,
        descriptors or None)."""
        n = len(frames)
        xyl = np.zeros((n, cap, 3), np.int32)
        scores = np.zeros((n, cap), np.float64)
        desc = np.zeros((n, cap, 32), np.uint8) if with_desc else None
        counts = np.zeros(n, np.int32)
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        self._check(self.lib.sdvl_filter_inputs(self.h, n, arr, cap, _ptr(xyl, i32p), _ptr(scores, f64p),
                                                _ptr(desc, u8p) if with_desc else None, _ptr(counts, i32p)))
        return [(xyl[i, :c].copy(), scores[i, :c].copy(), desc[i, :c].copy() if with_desc else None) for i, c in enumerate(counts)]

    def orb_describe_points(self, frame, xyl):
        xyl = np.ascontiguousarray(xyl, np.int32).reshape(-1, 3)
        desc = np.zeros((len(xyl), 32), np.uint8)
        ang = np.zeros(len(xyl), np.float32)
        self._check(self.lib.sdvl_orb_describe_points(self.h, frame.h, len(xyl), _ptr(xyl, i32p), _ptr(desc, u8p), _ptr(ang, f32p)))
        return desc, ang

    def hamming_argmin(self, queries, cand_lists, threshold=100):
        """ORBDetector::Distance over per-query candidate lists + SearchFeatures' arg-min (orb_detector.cc:398-410,
        matcher.cc:254-289).  queries [n][32] u8; cand_lists: n arrays [k_i][32] u8.  -> (best_index[n], best_dist[n])"""
        q = np.ascontiguousarray(queries, np.uint8).reshape(-1, 32)
        n = len(q)
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in cand_lists])
        cands = (np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint8).reshape(-1, 32) for c in cand_lists]))
                 if n else np.zeros((0, 32), np.uint8))
        if len(cands) == 0:
            cands = np.zeros((1, 32), np.uint8)
        bi = np.zeros(n, np.int32)
        bd = np.zeros(n, np.int32)
        self.lib.sdvl_hamming_argmin.argtypes = [C.c_void_p, C.c_int, u8p, i32p, u8p, C.c_int, i32p, i32p]
        self._check(self.lib.sdvl_hamming_argmin(self.h, n, _ptr(q, u8p), _ptr(offs, i32p), _ptr(cands, u8p), int(threshold),
                                                 _ptr(bi, i32p), _ptr(bd, i32p)))
        return bi, bd

    @staticmethod
    def _align_jobs(jobs):
        ja = (AlignJob * len(jobs))()
        for i, (ref, cur, b, e, T) in enumerate(jobs):
            ja[i].ref = ref.h.value
            ja[i].cur = cur.h.value
            ja[i].feat_begin, ja[i].feat_end = b, e
            for k in range(7):
                ja[i].T[k] = float(T[k])
        return ja

    def image_align(self, jobs, feats, cam, ap):
        """jobs: list of (ref Frame, cur Frame, feat_begin, feat_end, T7); feats: AlignFeature array"""
        n = len(jobs)
        res = (AlignResult * n)()
        self._check(self.lib.sdvl_image_align(self.h, n, self._align_jobs(jobs), len(feats), feats, C.byref(cam), C.byref(ap), res))
        return res

    def image_align_stored(self, jobs, store, cam, ap):
        """sdvl_image_align_begin_stored + _end: as image_align, with feat_begin / feat_end naming records of `store` (AlignStore)"""
        n = len(jobs)
        res = (AlignResult * n)()
        self._check(self.lib.sdvl_image_align_begin_stored(self.h, n, self._align_jobs(jobs), store.h, C.byref(cam), C.byref(ap)))
        self._check(self.lib.sdvl_image_align_end(self.h, n, res))
        return res

    def search_points(self, reqs, cam, sp):
        n = len(reqs)
        res = (SearchRes * n)()
        self._check(self.lib.sdvl_search_points(self.h, n, reqs, C.byref(cam), C.byref(sp), res))
        return res

    def frames_upload(self, frames, addresses, stride):
        """sdvl_frames_upload: images at host `addresses` (ints; pinned memory is read by one gather kernel, pageable memory is
        copied image by image) become level 0 of `frames`; the memory must stay alive until the stream has passed"""
        n = len(frames)
        fr = (C.c_void_p * n)(*[f.h for f in frames])
        im = (C.c_void_p * n)(*[int(a) for a in addresses])
        self._check(self.lib.sdvl_frames_upload(self.h, n, fr, im, int(stride)))

    @staticmethod
    def _stated_results(n, cur_poses, ref_poses, bearings, found, px, levels=None):
        """what the stated depth_filter entries take in a search's place, as contiguous arrays [n][7], [n][7], [n][3], [n], [n][2] and,
        for the entries that look a depth up, the found levels [n]"""
        arrs = [np.ascontiguousarray(cur_poses, np.float64).reshape(n, 7), np.ascontiguousarray(ref_poses, np.float64).reshape(n, 7),
                np.ascontiguousarray(bearings, np.float64).reshape(n, 3), np.ascontiguousarray(found, np.int32).reshape(n),
                np.ascontiguousarray(px, np.float64).reshape(n, 2)]
        return arrs + ([np.ascontiguousarray(levels, np.int32).reshape(n)] if levels is not None else [])

    def _filter_entry(self, name, n, head, track_set, tail=(), searched=False, status=False):
        """One of the depth filter's entries through _check: (context, n, head..., the track set's handle or null, tail..., results...).
        An int goes as it is, None as null, an array or a ctypes object by its address.  -> the results: the SearchRes array of a
        searched entry, the DepthOut array, the status bytes (uint8 [n], 255 where no depth was looked up) of an entry that writes them"""
        out = ([(SearchRes * n)()] if searched else []) + [(DepthOut * n)()] + ([np.full(max(n, 1), 255, np.uint8)] if status else [])
        args = [*head, track_set.h if track_set is not None else None, *tail, *out]
        fn = getattr(self.lib, name)
        if fn.argtypes is None:  # (an entry's ints stand at the same places in every call)
            fn.argtypes = [C.c_void_p, C.c_int] + [C.c_int if type(a) is int else C.c_void_p for a in args]
        self._check(fn(self.h, n, *[a.ctypes.data if type(a) is np.ndarray else a if a is None or type(a) in (int, C.c_void_p) else C.addressof(a)
                                    for a in args]))
        if status:
            out[-1] = out[-1][:n]
        return out[0] if len(out) == 1 else tuple(out)

    def search_points_filter(self, reqs, cam, sp, states, fparams, track_set=None):
        """sdvl_search_points_filter: (search results, depth-filter outcomes); with track_set (a TrackSet) the rows the states name
        are patched in its tables"""
        return self._filter_entry("sdvl_search_points_filter", len(reqs), [reqs, cam, sp, states, fparams], track_set, searched=True)

    def depth_filter(self, cur_poses, ref_poses, bearings, found, px, cam, states, fparams, track_set=None):
        """sdvl_depth_filter: the mapper's depth filter alone.  cur_poses / ref_poses [n][7], bearings [n][3], found [n], px [n][2];
        states: DepthState array -> DepthOut array"""
        n = len(states)
        return self._filter_entry("sdvl_depth_filter", n, self._stated_results(n, cur_poses, ref_poses, bearings, found, px) + [cam, states, fparams],
                                  track_set)

    def depth_seed(self, jobs, width, height, xyl, cam, dist=None, **rule):
        """sdvl_depth_seed: the depth of corners from registered depth images.  jobs: (depth, c_begin, c_end) or (depth, c_begin, c_end,
        scale) each, depth a numpy [height, width] float32 (metres) or uint16 (units of `scale` metres) image — read where it lies in host
        memory, padded rows allowed — or a DepthJob made by the caller (device pointers, pinned memory).  xyl [n][3] level coordinates and
        level; cam a Camera; dist (k1, k2, p1, p2, k3) or None; rule: min_depth, max_depth, edge_ratio, min_valid (0: the default)
        -> (z float64 [n], status uint8 [n], ok per job int32)"""
        keep, arr, d5, mp = self._depth_measure_args(jobs, width, height, dist, 0.0, 0.0, rule)
        xyl = np.ascontiguousarray(xyl, np.int32).reshape(-1, 3)
        n = len(xyl)
        z, status, ok = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint8), np.zeros(max(len(jobs), 1), np.int32)
        self.lib.sdvl_depth_seed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_depth_seed(self.h, len(jobs), arr, width, height, n, xyl.ctypes.data, C.addressof(cam),
                                             C.addressof(d5) if d5 is not None else None, C.addressof(mp.rule), z.ctypes.data, status.ctypes.data,
                                             ok.ctypes.data))
        return z[:n], status[:n], ok[:len(jobs)]

    def stereo_depth(self, jobs, xyl, cam, baseline, dist=None, **rule):
        """sdvl_stereo_depth: the depth of corners from rectified stereo pairs.  jobs: (left Frame, right, c_begin, c_end) each, right a
        numpy [height, width] uint8 image — host memory, padded rows allowed, copied to HBM by the call — or a StereoJob made by the caller
        (device pointers, pinned memory).  xyl [n][3] level coordinates and level; cam a Camera; baseline in metres; dist (k1, k2, p1, p2,
        k3) or None: a lens is refused; rule: min_depth, max_depth, max_disparity, max_sad, uniqueness (0: the default)
        -> (z float64 [n], disparity float64 [n], status uint8 [n], ok per job int32)"""
        keep, arr, d5, p = self._stereo_args(jobs, baseline, dist, rule)
        xyl = np.ascontiguousarray(xyl, np.int32).reshape(-1, 3)
        n = len(xyl)
        z, disparity, status = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint8)
        ok = np.zeros(max(len(jobs), 1), np.int32)
        self.lib.sdvl_stereo_depth.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        self._check(self.lib.sdvl_stereo_depth(self.h, len(jobs), C.addressof(arr), n, xyl.ctypes.data, C.addressof(cam), C.addressof(p),
                                               z.ctypes.data, disparity.ctypes.data, status.ctypes.data, ok.ctypes.data))
        del keep
        return z[:n], disparity[:n], status[:n], ok[:len(jobs)]

    def _stereo_args(self, jobs, baseline, dist, rule):
        """the stereo side of an entry -> (objects to keep alive, StereoJob array, distortion or None, StereoParams)"""
        keep, arr = [], (StereoJob * max(len(jobs), 1))()
        for j, job in enumerate(jobs):
            if isinstance(job, StereoJob):
                arr[j] = job
                continue
            left, r = job[0], job[1]
            assert r.dtype == np.uint8 and r.ndim == 2 and r.strides[1] == 1 and r.shape == (left.height, left.width)
            keep.append(r)
            arr[j] = StereoJob(left.h, r.ctypes.data, 0, r.strides[0], int(job[2]), int(job[3]))
        d5 = Distortion((C.c_double * 5)(*[float(x) for x in dist])) if dist is not None else None
        p = StereoParams(float(baseline), float(rule.pop("min_depth", 0.0)), float(rule.pop("max_depth", 0.0)), int(rule.pop("max_disparity", 0)),
                         int(rule.pop("max_sad", 0)), int(rule.pop("uniqueness", 0)), 0, C.addressof(d5) if d5 is not None else None)
        assert not rule, "unknown rule field %s" % list(rule)
        return keep, arr, d5, p

    def stereo_lookup(self, jobs, px, levels, cam, baseline, dist=None, **rule):
        """sdvl_stereo_lookup: stereo_depth's rule at level-0 positions px [n][2] of the left image (sub-pixel) with the window stride of
        levels [n]; jobs, cam, baseline, dist and rule as for stereo_depth, the jobs' ranges indexing the positions
        -> (z float64 [n], disparity float64 [n], status uint8 [n], ok per job int32)"""
        keep, arr, d5, p = self._stereo_args(jobs, baseline, dist, rule)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        levels = np.ascontiguousarray(levels, np.int32).reshape(-1)
        n = len(px)
        assert len(levels) == n
        z, disparity, status = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint8)
        ok = np.zeros(max(len(jobs), 1), np.int32)
        self.lib.sdvl_stereo_lookup.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8
        self._check(self.lib.sdvl_stereo_lookup(self.h, len(jobs), C.addressof(arr), n, px.ctypes.data, levels.ctypes.data, C.addressof(cam),
                                                C.addressof(p), z.ctypes.data, disparity.ctypes.data, status.ctypes.data, ok.ctypes.data))
        del keep
        return z[:n], disparity[:n], status[:n], ok[:len(jobs)]

    def depth_lookup(self, jobs, width, height, px, levels, cam, dist=None, **rule):
        """sdvl_depth_lookup: depth_seed's rule at level-0 positions px [n][2] (sub-pixel) with the window stride of levels [n]; jobs, cam,
        dist and rule as for depth_seed, the jobs' ranges indexing the positions -> (z float64 [n], status uint8 [n], ok per job int32)"""
        keep, arr, d5, mp = self._depth_measure_args(jobs, width, height, dist, 0.0, 0.0, rule)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        levels = np.ascontiguousarray(levels, np.int32).reshape(-1)
        n = len(px)
        assert len(levels) == n
        z, status, ok = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint8), np.zeros(max(len(jobs), 1), np.int32)
        self.lib.sdvl_depth_lookup.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_depth_lookup(self.h, len(jobs), arr, width, height, n, px.ctypes.data, levels.ctypes.data, C.addressof(cam),
                                               C.addressof(d5) if d5 is not None else None, C.addressof(mp.rule), z.ctypes.data, status.ctypes.data,
                                               ok.ctypes.data))
        return z[:n], status[:n], ok[:len(jobs)]

    def _depth_measure_args(self, jobs, width, height, dist, noise_abs, noise_quad, rule):
        """the depth side of the two measured entries -> (objects to keep alive, job array, distortion or None, DepthMeasureParams)"""
        keep, arr = [], (DepthJob * max(len(jobs), 1))()
        for j, job in enumerate(jobs):
            if isinstance(job, DepthJob):
                arr[j] = job
                continue
            d = job[0]
            assert d.dtype in (np.float32, np.uint16) and d.ndim == 2 and d.strides[1] == d.itemsize and d.shape == (height, width)
            keep.append(d)
            arr[j] = DepthJob(d.ctypes.data, 0, d.strides[0], SDVL_DEPTH_U16 if d.dtype == np.uint16 else SDVL_DEPTH_F32, 0,
                              float(job[3]) if len(job) > 3 else 1.0, int(job[1]), int(job[2]))
        mp = DepthMeasureParams(DepthSeedParams(float(rule.pop("min_depth", 0.0)), float(rule.pop("max_depth", 0.0)),
                                                float(rule.pop("edge_ratio", 0.0)), int(rule.pop("min_valid", 0)), 0), float(noise_abs), float(noise_quad))
        assert not rule, "unknown rule field %s" % list(rule)
        d5 = Distortion((C.c_double * 5)(*[float(x) for x in dist])) if dist is not None else None
        return keep, arr, d5, mp

    def depth_filter_measured(self, cur_poses, ref_poses, bearings, found, px, levels, cam, states, fparams, jobs, width, height, dist=None,
                              noise_abs=0.0, noise_quad=0.0, track_set=None, **rule):
        """sdvl_depth_filter_measured: depth_filter's arguments and the found level of every item [n]; jobs as for depth_seed, each the depth
        image of the current frame of the items c_begin .. c_end (an item in no job has no image); noise_abs / noise_quad and rule: 0 takes
        the default -> (DepthOut array, status uint8 [n]: depth_seed's codes, 255 where no depth was looked up)"""
        n = len(states)
        stated = self._stated_results(n, cur_poses, ref_poses, bearings, found, px, levels)
        keep, arr, d5, mp = self._depth_measure_args(jobs, width, height, dist, noise_abs, noise_quad, rule)
        return self._filter_entry("sdvl_depth_filter_measured", n, stated + [cam, states, fparams], track_set,
                                  [len(jobs), arr, int(width), int(height), d5, mp], status=True)

    def search_points_filter_measured(self, reqs, cam, sp, states, fparams, jobs, width, height, dist=None, noise_abs=0.0, noise_quad=0.0,
                                      track_set=None, **rule):
        """sdvl_search_begin / _slot / sdvl_search_run_filter_measured: search_points_filter's requests (frames by handle) with the depth
        side of depth_filter_measured -> (SearchRes array, DepthOut array, status uint8 [n])"""
        self._pack_search_requests(reqs)
        keep, arr, d5, mp = self._depth_measure_args(jobs, width, height, dist, noise_abs, noise_quad, rule)
        return self._filter_entry("sdvl_search_run_filter_measured", len(reqs), [cam, sp, states, fparams], track_set,
                                  [len(jobs), arr, int(width), int(height), d5, mp], searched=True, status=True)

    def depth_filter_stereo(self, cur_poses, ref_poses, bearings, found, px, levels, cam, states, fparams, jobs, baseline, disparity_sigma=0.0,
                            dist=None, track_set=None, **rule):
        """sdvl_depth_filter_stereo: depth_filter's arguments and the found level of every item [n]; jobs as for stereo_depth, each the left
        frame and right image of the current frame of the items c_begin .. c_end (an item in no job has no pair); disparity_sigma in pixels
        (0: 0.25, not measured against a real pair) and rule: 0 takes the default
        -> (DepthOut array, status uint8 [n]: stereo_depth's codes, 255 where nothing was matched)"""
        n = len(states)
        stated = self._stated_results(n, cur_poses, ref_poses, bearings, found, px, levels)
        keep, arr, d5, p = self._stereo_args(jobs, baseline, dist, rule)
        mp = StereoMeasureParams(p, float(disparity_sigma))
        return self._filter_entry("sdvl_depth_filter_stereo", n, stated + [cam, states, fparams], track_set, [len(jobs), arr, mp], status=True)

    def _pack_search_requests(self, reqs):
        """sdvl_search_begin / _slot: the requests (frames by handle) into the context's packed records"""
        n = len(reqs)
        lib = self.lib
        lib.sdvl_search_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(SearchReqPacked))]
        lib.sdvl_search_slot.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        packed = C.POINTER(SearchReqPacked)()
        self._check(lib.sdvl_search_begin(self.h, n, C.byref(packed)))
        for i, r in enumerate(reqs):
            d = packed[i]
            d.cur = lib.sdvl_search_slot(self.h, r.cur, r.cur_pose)
            d.ref = lib.sdvl_search_slot(self.h, r.ref, r.ref_pose)
            assert d.cur >= 0 and d.ref >= 0
            d.level, d.fixed = r.level, r.fixed
            d.px[0], d.px[1] = r.px[0], r.px[1]
            for k in range(3):
                d.bearing[k] = r.bearing[k]
            d.idepth, d.idepth_std = r.idepth, r.idepth_std
            d.px0[0], d.px0[1] = r.px0[0], r.px0[1]
            for k in range(32):
                d.desc[k] = r.desc[k]

    def search_points_filter_stereo(self, reqs, cam, sp, states, fparams, jobs, baseline, disparity_sigma=0.0, dist=None, track_set=None, **rule):
        """sdvl_search_begin / _slot / sdvl_search_run_filter_stereo: search_points_filter's requests (frames by handle) with the stereo
        side of depth_filter_stereo -> (SearchRes array, DepthOut array, status uint8 [n])"""
        self._pack_search_requests(reqs)
        keep, arr, d5, p = self._stereo_args(jobs, baseline, dist, rule)
        mp = StereoMeasureParams(p, float(disparity_sigma))
        return self._filter_entry("sdvl_search_run_filter_stereo", len(reqs), [cam, sp, states, fparams], track_set, [len(jobs), arr, mp],
                                  searched=True, status=True)

    def track_points_download(self, track_set):
        """the point rows of every tracker of a TrackSet as the device holds them: uint8 [n_trackers * max_points][144]"""
        self.lib.sdvl_track_points_device.restype = C.c_void_p
        self.lib.sdvl_track_points_device.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        np_, nt = C.c_int(0), C.c_int(0)
        p = self.lib.sdvl_track_points_device(track_set.h, C.byref(np_), C.byref(nt))
        rows = np_.value * nt.value
        return self.device_download(p, rows * C.sizeof(TrackPoint)).reshape(rows, C.sizeof(TrackPoint))

    def search_chain(self, reqs, cam, sp, trackers, req_points, fx, max_ransac_points=5, max_ransac_its=100, max_optim_pose_its=10,
                     inlier_error_threshold=2.0):
        """sdvl_search_begin / _slot / _run_chain / _chain_end.  reqs: SearchReq array (frames by handle); trackers: list of
        dict(cells=[[request index or -1, ...], ...] in SelectPoints order, max_matches, pose7, draws=raw rand() values);
        req_points[n][3].  Returns (search results, per tracker dict(pose, n_draws, refined, n_obs, inliers, outliers))."""
        n = len(reqs)
        lib = self.lib
        self._pack_search_requests(reqs)
        nf = len(trackers)
        cf = (ChainFrame * nf)()
        cand_req, cand_first, rand_raw = [], [], []
        for f, t in enumerate(trackers):
            cf[f].cand_begin = len(cand_req)
            for cell in t["cells"]:
                first = len(cand_req)
                for r in cell:
                    cand_req.append(int(r))
                    cand_first.append(first)
            cf[f].cand_end = len(cand_req)
            cf[f].max_matches = int(t["max_matches"])
            cf[f].rand_begin = len(rand_raw)
            rand_raw += [int(d) for d in t["draws"][:max_ransac_its]]
            for c in range(7):
                cf[f].pose[c] = float(t["pose"][c])
        cr = np.asarray(cand_req, np.int32); cfi = np.asarray(cand_first, np.int32); rr = np.asarray(rand_raw, np.int32)
        pts = np.ascontiguousarray(req_points, np.float64).reshape(n, 3)
        prm = PoseParams(max_ransac_points, max_ransac_its, max_optim_pose_its, 0, inlier_error_threshold / fx, fx)
        res = (SearchRes * n)()
        lib.sdvl_search_run_chain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._check(lib.sdvl_search_run_chain(self.h, n, C.byref(cam), C.byref(sp), res, nf, cf, len(cr), _ptr(cr, i32p), _ptr(cfi, i32p),
                                              _ptr(pts, f64p), len(rr), _ptr(rr, i32p), C.byref(prm)))
        pres = (PoseResult * nf)()
        n_obs = np.zeros(nf, np.int32)
        total = sum(int(t["max_matches"]) for t in trackers)
        lists = np.zeros(max(total, 1), np.int32)
        lib.sdvl_search_chain_end.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(lib.sdvl_search_chain_end(self.h, nf, pres, _ptr(n_obs, i32p), _ptr(lists, i32p)))
        out, b = [], 0
        for f, t in enumerate(trackers):
            out.append(dict(pose=np.array(list(pres[f].pose)), n_draws=pres[f].n_draws, refined=pres[f].refined, n_obs=int(n_obs[f]),
                            inliers=lists[b:b + pres[f].n_inliers].copy(),
                            outliers=lists[b + pres[f].n_inliers:b + pres[f].n_inliers + pres[f].n_outliers].copy()))
            b += int(t["max_matches"])
        return res, out

    def align_patches(self, frames, levels, border, patch, uv, max_its=10):
        n = len(frames)
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        levels = np.ascontiguousarray(levels, np.int32)
        border = np.ascontiguousarray(border, np.uint8).reshape(n, 100)
        patch = np.ascontiguousarray(patch, np.uint8).reshape(n, 64)
        uv = np.array(uv, np.float64).reshape(n, 2)
        conv = np.zeros(n, np.uint8)
        its = np.zeros(n, np.int32)
        self._check(self.lib.sdvl_align_patches(self.h, n, arr, _ptr(levels, i32p), _ptr(border, u8p), _ptr(patch, u8p), max_its,
                                                _ptr(uv, f64p), _ptr(conv, u8p), _ptr(its, i32p)))
        return uv, conv, its

    def pose_from_matches(self, jobs, fx, max_ransac_points=5, max_ransac_its=100, max_optim_pose_its=10, inlier_error_threshold=2.0):
        """jobs: list of (obs[n][6] = ax, ay, px, py, pz, level; pose7; rand_draws[max_ransac_its] raw rand() values).
        Returns per job dict(pose, n_draws, inliers, outliers, refined)."""
        n = len(jobs)
        pj = (PoseJob * n)()
        obs_all, rand_all, nits_all = [], [], []
        for k, (obs, pose, draws) in enumerate(jobs):
            obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 6)
            size = len(obs)
            pj[k].obs_begin = len(obs_all); pj[k].obs_end = len(obs_all) + size
            pj[k].rand_begin = len(rand_all); pj[k].nits_begin = len(nits_all)
            for c in range(7):
                pj[k].pose[c] = float(pose[c])
            for o in obs:
                obs_all.append(PoseObs(o[0], o[1], o[2], o[3], o[4], 1.0 / (1 << int(o[5]))))
            assert len(draws) >= max_ransac_its
            rand_all += [int(d) % size if size else 0 for d in draws[:max_ransac_its]]
            nits_all += ransac_budget_table(size, max_ransac_points, max_ransac_its)
        po = (PoseObs * max(len(obs_all), 1))(*obs_all)
        ra = np.asarray(rand_all, np.int32); ni = np.asarray(nits_all, np.int32)
        prm = PoseParams(max_ransac_points, max_ransac_its, max_optim_pose_its, 0, inlier_error_threshold / fx, fx)
        res = (PoseResult * n)()
        lists = np.zeros(max(len(obs_all), 1), np.int32)
        self.lib.sdvl_pose_from_matches.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_pose_from_matches(self.h, n, pj, len(obs_all), po, len(ra), _ptr(ra, i32p), len(ni), _ptr(ni, i32p),
                                                    C.byref(prm), res, _ptr(lists, i32p)))
        out = []
        for k in range(n):
            b = pj[k].obs_begin
            out.append(dict(pose=np.array(list(res[k].pose)), n_draws=res[k].n_draws, refined=res[k].refined,
                            inliers=lists[b:b + res[k].n_inliers].copy(),
                            outliers=lists[b + res[k].n_inliers:b + res[k].n_inliers + res[k].n_outliers].copy()))
        return out

    def track_set(self, n_trackers, max_points, max_features, grid_cells, max_matches, max_ransac_its):
        """sdvl_track_create: device-resident tracking tables for n_trackers (TrackSet)"""
        return TrackSet(self, n_trackers, max_points, max_features, grid_cells, max_matches, max_ransac_its)

    def register(self, frames, poses):
        """sdvl_frames_register: (frame, pose [7]) pairs become addressable by the points of tracking tables"""
        n = len(frames)
        arr = (C.c_void_p * max(n, 1))(*[f.h for f in frames])
        p7 = np.ascontiguousarray(poses, np.float64).reshape(n, 7)
        self._check(self.lib.sdvl_frames_register(self.h, n, arr, _ptr(p7, f64p)))

    def klt_track(self, jobs, win_size=30, max_level=4, max_its=30, eps=0.001, min_eig_threshold=1e-4):
        """cv::calcOpticalFlowPyrLK as HomographyInit::TrackSecondFrame calls it (homography_init.cc:195-198), all jobs in one launch.
        jobs: list of (prev Frame, next Frame, prev_xy [n][2], initial next_xy [n][2]).
        Returns per job dict(xy float32 [n][2], status bool [n], err float32 [n])."""
        kj = (KltJob * max(len(jobs), 1))()
        prev_all, next_all = [], []
        at = 0
        for k, (fp, fn, pxy, nxy) in enumerate(jobs):
            pxy = np.asarray(pxy, np.float32).reshape(-1, 2)
            nxy = np.asarray(nxy, np.float32).reshape(-1, 2)
            assert len(pxy) == len(nxy)
            kj[k].prev, kj[k].next = fp.h.value, fn.h.value
            kj[k].pt_begin, kj[k].pt_end = at, at + len(pxy)
            at += len(pxy)
            prev_all.append(pxy)
            next_all.append(nxy)
        prev = np.ascontiguousarray(np.concatenate(prev_all) if jobs else np.zeros((0, 2)), np.float32)
        nxt = np.ascontiguousarray(np.concatenate(next_all) if jobs else np.zeros((0, 2)), np.float32).copy()
        status = np.zeros(max(at, 1), np.uint8)
        err = np.zeros(max(at, 1), np.float32)
        prm = KltParams(win_size, max_level, max_its, 0, eps, min_eig_threshold)
        self.lib.sdvl_klt_track.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_klt_track(self.h, len(jobs), kj, at, prev.ctypes.data, nxt.ctypes.data, status.ctypes.data, err.ctypes.data,
                                            C.byref(prm)))
        return [dict(xy=nxt[kj[k].pt_begin:kj[k].pt_end].copy(), status=status[kj[k].pt_begin:kj[k].pt_end].astype(bool),
                     err=err[kj[k].pt_begin:kj[k].pt_end].copy()) for k in range(len(jobs))]

    def homography_ransac(self, jobs, threshold, max_its=2000, confidence=0.995):
        """The RANSAC of cv::findHomography(src, dst, CV_RANSAC, threshold) (homography_init.cc:253), all jobs in one call.
        jobs: list of (src [n][2], dst [n][2], draws4 [k][4]: the 4-subsets the caller's random stream would draw, indices into the
        job's matches).  Returns per job dict(H [3][3], best_draw, n_its, inliers)."""
        n = len(jobs)
        hj = (HomographyJob * max(n, 1))()
        src_all, dst_all, draw_all = [np.zeros((0, 2))], [np.zeros((0, 2))], [np.zeros((0, 4), np.int32)]
        m_at = d_at = 0
        for k, (src, dst, draws) in enumerate(jobs):
            src = np.asarray(src, np.float64).reshape(-1, 2)
            dst = np.asarray(dst, np.float64).reshape(-1, 2)
            draws = np.asarray(draws, np.int32).reshape(-1, 4)
            assert len(src) == len(dst)
            hj[k].m_begin, hj[k].m_end = m_at, m_at + len(src)
            hj[k].draw_begin, hj[k].draw_end = d_at, d_at + len(draws)
            m_at += len(src)
            d_at += len(draws)
            src_all.append(src); dst_all.append(dst); draw_all.append(draws)
        src = np.ascontiguousarray(np.concatenate(src_all), np.float64)
        dst = np.ascontiguousarray(np.concatenate(dst_all), np.float64)
        draws = np.ascontiguousarray(np.concatenate(draw_all), np.int32)
        res = (HomographyResult * max(n, 1))()
        lists = np.zeros(max(m_at, 1), np.int32)
        self.lib.sdvl_homography_ransac.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_double, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_homography_ransac(self.h, n, hj, m_at, src.ctypes.data, dst.ctypes.data, d_at, draws.ctypes.data,
                                                    float(threshold), int(max_its), float(confidence), res, lists.ctypes.data))
        return [dict(H=np.array(list(res[k].H)).reshape(3, 3), best_draw=res[k].best_draw, n_its=res[k].n_its,
                     inliers=lists[hj[k].m_begin:hj[k].m_begin + res[k].n_inliers].copy()) for k in range(n)]

    def bundle_adjust(self, problems, cam, bf=None):
        """Bundle::Local (extra/bundle.cc:110-223) for every problem of the list in one launch.
        With bf (pixel x metres) the problems' edge_d [n_e] (measured camera-frame z in metres, 0: none) makes depth edges of the
        observations that carry one (sdvl_bundle_adjust_depth; a problem without edge_d has none); without bf edge_d is not looked at.
        problems: dicts with poses [n_kf][7] (free ones first), fixed [n_kf], points [n_pt][3], edge_pt [n_e], edge_kf [n_e] (indices
        inside the problem), edge_uv [n_e][2]; cam = (fx, fy, cx, cy).  The inputs are not modified.
        Returns per problem dict(status, poses, points, levels [n_e], pose_stages [n_kf], point_stages [n_pt], n_level1,
        stages: two dicts(iterations, trials, lam, chi2_before, chi2_after, trials_per_it, accepted_its))."""
        n = len(problems)
        bp = (BundleProblem * max(n, 1))()
        poses_all, fixed_all, pts_all = [np.zeros((0, 7))], [np.zeros(0, np.int32)], [np.zeros((0, 3))]
        edge_n = sum(len(p["edge_pt"]) for p in problems)
        fields = [("point", np.int32), ("keyframe", np.int32), ("u", np.float64), ("v", np.float64)]
        be = np.zeros(max(edge_n, 1), np.dtype(fields + ([("depth", np.float64)] if bf is not None else [])))
        assert be.dtype.itemsize == C.sizeof(BundleEdge if bf is None else BundleEdgeDepth)
        k_at = p_at = e_at = 0
        for j, p in enumerate(problems):
            poses = np.asarray(p["poses"], np.float64).reshape(-1, 7)
            pts = np.asarray(p["points"], np.float64).reshape(-1, 3)
            uv = np.asarray(p["edge_uv"], np.float64).reshape(-1, 2)
            assert len(p["fixed"]) == len(poses) and len(p["edge_pt"]) == len(p["edge_kf"]) == len(uv)
            bp[j] = BundleProblem(k_at, k_at + len(poses), p_at, p_at + len(pts), e_at, e_at + len(uv))
            sl = be[e_at:e_at + len(uv)]
            sl["point"], sl["keyframe"], sl["u"], sl["v"] = p["edge_pt"], p["edge_kf"], uv[:, 0], uv[:, 1]
            if bf is not None and "edge_d" in p:
                assert len(p["edge_d"]) == len(uv)
                sl["depth"] = p["edge_d"]
            k_at += len(poses); p_at += len(pts); e_at += len(uv)
            poses_all.append(poses); fixed_all.append(np.asarray(p["fixed"], np.int32)); pts_all.append(pts)
        poses = np.ascontiguousarray(np.concatenate(poses_all), np.float64).copy()
        fixed = np.ascontiguousarray(np.concatenate(fixed_all), np.int32)
        pts = np.ascontiguousarray(np.concatenate(pts_all), np.float64).copy()
        levels = np.zeros(max(e_at, 1), np.int32)
        kstage, pstage = np.zeros(max(k_at, 1), np.int32), np.zeros(max(p_at, 1), np.int32)
        res = (BundleResult * max(n, 1))()
        c = Camera(0.0, 0.0, float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]))
        if bf is None:
            self._check(self.lib.sdvl_bundle_adjust(self.h, n, bp, k_at, poses.ctypes.data, fixed.ctypes.data, p_at, pts.ctypes.data, e_at, be.ctypes.data,
                                                    C.byref(c), levels.ctypes.data, kstage.ctypes.data, pstage.ctypes.data, res))
        else:
            self._check(self.lib.sdvl_bundle_adjust_depth(self.h, n, bp, k_at, poses.ctypes.data, fixed.ctypes.data, p_at, pts.ctypes.data, e_at,
                                                          be.ctypes.data, C.byref(c), float(bf), levels.ctypes.data, kstage.ctypes.data, pstage.ctypes.data, res))
        out = []
        for j in range(n):
            b, r = bp[j], res[j]
            stages = [dict(iterations=s.iterations, trials=s.trials, lam=s.lam, chi2_before=s.chi2_before, chi2_after=s.chi2_after,
                           trials_per_it=list(s.trials_per_it)[:s.iterations],
                           accepted_its=[bool(s.accepted_mask >> i & 1) for i in range(s.iterations)]) for s in r.stage]
            out.append(dict(status=r.status, n_level1=r.n_level1, n_free=r.n_free, stages=stages, poses=poses[b.kf_begin:b.kf_end].copy(),
                            points=pts[b.pt_begin:b.pt_end].copy(), levels=levels[b.edge_begin:b.edge_end].copy(),
                            pose_stages=kstage[b.kf_begin:b.kf_end].copy(), point_stages=pstage[b.pt_begin:b.pt_end].copy()))
        return out

    def undistort(self, imgs, cam, dist, frames=None):
        """Camera::UndistortImage for a batch of host images (numpy u8 [h, w]).  With `frames` the result becomes their
        level 0 (fused upload); otherwise it is returned as numpy arrays."""
        n = len(imgs)
        imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
        h, w = imgs[0].shape
        src = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        d = Distortion((C.c_double * 5)(*[float(x) for x in dist]))
        if frames is not None:
            arr = (C.c_void_p * n)(*[f.h for f in frames])
            self._check(self.lib.sdvl_frames_upload_undistorted(self.h, n, arr, src, w, 0, C.byref(cam), C.byref(d)))
            return None
        buf = self.device_malloc(n * w * h)
        try:
            dst = (C.c_void_p * n)(*[buf + i * w * h for i in range(n)])
            self.lib.sdvl_undistort.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_int]
            self._check(self.lib.sdvl_undistort(self.h, n, src, w, 0, w, h, C.byref(cam), C.byref(d), dst, w))
            out = self.device_download(buf, n * w * h).reshape(n, h, w)
        finally:
            self.device_free(buf)
        return [out[i].copy() for i in range(n)]

    def convert_gray(self, imgs, fmt):
        """cv::cvtColor(img, CV_*2GRAY) on the device for a batch of host colour images (numpy u8 [h, w, 3 or 4]; fmt = SDVL_* value)
        -> numpy gray images.  Raw formats: u8 [h, w] (Bayer), u8 [h, w, 2] (YUYV / UYVY) or u16 [h, w] (16-bit gray)"""
        n = len(imgs)
        imgs = [_raw_bytes(im) for im in imgs]
        h, w, ch = imgs[0].shape
        src = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        buf = self.device_malloc(n * w * h)
        try:
            dst = (C.c_void_p * n)(*[buf + i * w * h for i in range(n)])
            self.lib.sdvl_convert_gray.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
            self._check(self.lib.sdvl_convert_gray(self.h, n, src, w * ch, 0, w, h, int(fmt), dst, w))
            out = self.device_download(buf, n * w * h).reshape(n, h, w)
        finally:
            self.device_free(buf)
        return [out[i].copy() for i in range(n)]

    def upload_color(self, frames, imgs, fmt, cam=None, dist=None):
        """host colour images (numpy u8 [h, w, 3 or 4]; raw formats as for convert_gray) -> level 0 of `frames` = undistort(gray(img))
        (no lens without cam / dist); follow with pyramid_build"""
        n = len(imgs)
        imgs = [_raw_bytes(im) for im in imgs]
        h, w, ch = imgs[0].shape
        src = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        d = Distortion((C.c_double * 5)(*[float(x) for x in dist])) if dist is not None else None
        self.lib.sdvl_frames_upload_color.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_frames_upload_color(self.h, n, arr, src, w * ch, 0, int(fmt), C.byref(cam) if cam is not None else None,
                                                      C.byref(d) if d is not None else None))

    frames_upload_color = upload_color   # (the C entry's name)

    # ---- stereo rigs as calibrated
    stereo_rectify_plan = staticmethod(stereo_rectify_plan)

    @staticmethod
    def _image_sources(imgs, width=None):
        """host images (numpy u8 [h, stride]) or device images (objects with data_ptr / stride / shape, e.g. torch tensors on the
        context's GPU) -> (kept arrays, pointer array, h, w, stride, on_device); `width`: the columns that count, when rows are wider"""
        on_device = hasattr(imgs[0], "data_ptr")
        if on_device:
            keep = list(imgs)
            ptrs = [int(im.data_ptr()) for im in keep]
            stride = int(keep[0].stride(0))
        else:
            keep = [np.ascontiguousarray(im, np.uint8) for im in imgs]
            ptrs = [im.ctypes.data for im in keep]
            stride = keep[0].shape[1]
        h = int(keep[0].shape[0])
        w = int(width) if width is not None else int(keep[0].shape[1])
        return keep, (C.c_void_p * len(ptrs))(*ptrs), h, w, stride, int(on_device)

    def rectify(self, imgs, r, frames=None, width=None):
        """sdvl_rectify for a batch of raw images of one camera (see _image_sources) behind the Rectification r.  With `frames` the
        result becomes their level 0 (sdvl_frames_upload_rectified); otherwise it is returned as numpy arrays."""
        keep, src, h, w, stride, on_device = self._image_sources(imgs, width)
        n = len(keep)
        if frames is not None:
            arr = (C.c_void_p * n)(*[f.h for f in frames])
            self.lib.sdvl_frames_upload_rectified.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            self._check(self.lib.sdvl_frames_upload_rectified(self.h, n, arr, src, stride, on_device, C.byref(r)))
            return None
        buf = self.device_malloc(n * w * h)
        try:
            dst = (C.c_void_p * n)(*[buf + i * w * h for i in range(n)])
            self.lib.sdvl_rectify.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
            self._check(self.lib.sdvl_rectify(self.h, n, src, stride, on_device, w, h, C.byref(r), dst, w))
            out = self.device_download(buf, n * w * h).reshape(n, h, w)
        finally:
            self.device_free(buf)
        return [out[i].copy() for i in range(n)]

    def upload_color_rectified(self, frames, imgs, fmt, r):
        """host colour or raw images (as for upload_color) -> level 0 of `frames` = rectify(gray(img))"""
        n = len(imgs)
        imgs = [_raw_bytes(im) for im in imgs]
        h, w, ch = imgs[0].shape
        src = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        arr = (C.c_void_p * n)(*[f.h for f in frames])
        self.lib.sdvl_frames_upload_color_rectified.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        self._check(self.lib.sdvl_frames_upload_color_rectified(self.h, n, arr, src, w * ch, 0, int(fmt), C.byref(r)))

    def rectify_stats(self):
        """(rectification maps built on this context, pixels of the last map built with a tap outside the raw image)"""
        out = (C.c_int64 * 2)()
        self.lib.sdvl_rectify_stats.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_rectify_stats(self.h, out))
        return int(out[0]), int(out[1])

    def rectify_map_words(self, r, width, height, src_stride=None):
        """the per-pixel words of the camera's map: uint32 [h][w], or [h][w][2] for the wide map (a side above 2044)"""
        wide = width > 2044 or height > 2044
        out = np.zeros((height, width, 2) if wide else (height, width), np.uint32)
        self.lib.sdvl_rectify_map_words.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._check(self.lib.sdvl_rectify_map_words(self.h, int(width), int(height), int(src_stride or width), C.byref(r), out.ctypes.data))
        return out

    # ---- synthetic frames in HBM
    def device_malloc(self, nbytes):
        p = C.c_void_p()
        self._check(self.lib.sdvl_device_malloc(self.h, C.c_int64(nbytes), C.byref(p)))
        return p.value

    def device_free(self, p):
        self._check(self.lib.sdvl_device_free(self.h, C.c_void_p(p)))

    def device_download(self, p, nbytes):
        out = np.zeros(nbytes, np.uint8)
        self._check(self.lib.sdvl_device_download(self.h, C.c_void_p(p), C.c_int64(nbytes), _ptr(out, u8p)))
        return out

    def synth_render(self, views, width, height, dev_out, frame_bytes=None):
        n = len(views)
        arr = (SynthView * n)(*views)
        self._check(self.lib.sdvl_synth_render(self.h, n, arr, width, height, C.c_void_p(dev_out), C.c_int64(frame_bytes or width * height)))

    def synth_render_scene(self, scenes, width, height, dev_out, frame_bytes=None, dev_depth=None, dev_surface=None):
        """renders the SynthScenes into HBM: image i at dev_out + i * frame_bytes; dev_depth (float32) and dev_surface (uint8), where
        given, get the ground truth of every pixel, width * height entries per scene"""
        n = len(scenes)
        arr = (SynthScene * n)(*scenes)
        self._check(self.lib.sdvl_synth_render_scene(self.h, n, arr, width, height, dev_out, frame_bytes or width * height, dev_depth, dev_surface))


def default_detect_params(use_orb=True, orb_size=31, patch_size=8):
    """Config defaults (config.cc:55-85) with the TUM cfg overrides (config/config_tum_f1.cfg:34-42)."""
    return DetectParams(cell_size=32, max_fast_levels=3, fast_threshold=10,
                        margin=(4 + orb_size // 2) if use_orb else (1 + patch_size // 2))


def default_align_params(fast=False):
    return AlignParams(max_level=4, min_level=2, max_its=30, patch_size=4, fast=int(fast))


def default_search_params(use_orb=True, orb_size=31, patch_size=8):
    return SearchParams(patch_size=8, max_align_its=10, search_size=6, max_fast_levels=3,
                        margin=(4 + orb_size // 2) if use_orb else (1 + patch_size // 2), use_orb=int(use_orb))


class Feed:
    """sdvl_feed: one copy stream filled by one thread; consumers (contexts) acquire / release its slots"""

    def __init__(self, device=0, n_slots=2):
        self.lib = load_library()
        self.lib.sdvl_feed_last_error.restype = C.c_char_p
        self.lib.sdvl_feed_last_error.argtypes = [C.c_void_p]
        self.lib.sdvl_feed_slot_arrived.argtypes = [C.c_void_p, C.c_int]
        h = C.c_void_p()
        if self.lib.sdvl_feed_create(device, n_slots, C.byref(h)) != 0:
            raise SdvlError("sdvl_feed_create failed")
        self.h = h

    def images(self, slot, host_ptrs, stride, width, height, dev_dst):
        n = len(host_ptrs)
        src = (C.c_void_p * n)(*[int(p) for p in host_ptrs])
        dst = (C.c_void_p * n)(*[int(p) for p in dev_dst])
        if self.lib.sdvl_feed_images(self.h, slot, n, src, stride, width, height, dst) != 0:
            raise SdvlError("sdvl_feed_images: %s" % self.lib.sdvl_feed_last_error(self.h).decode())

    def arrived(self, slot):
        """True once the slot's last transfer is in HBM (never blocks)"""
        r = self.lib.sdvl_feed_slot_arrived(self.h, slot)
        if r < 0:
            raise SdvlError("sdvl_feed_slot_arrived: %s" % self.lib.sdvl_feed_last_error(self.h).decode())
        return r == 1

    def acquire(self, ctx, slot):
        ctx._check(self.lib.sdvl_ctx_feed_acquire(ctx.h, self.h, slot))

    def release(self, ctx, slot):
        ctx._check(self.lib.sdvl_ctx_feed_release(ctx.h, self.h, slot))

    def close(self):
        if self.h:
            self.lib.sdvl_feed_destroy(self.h)
            self.h = None
