"""ctypes view of the host layer (host/libsdvl_host.so): B independent SDVL trackers on one MI355X stepping
together (sdvl::SDVLBatch).  No CPU fallback: construction fails without a GPU."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "host", "libsdvl_host.so")


class FrameStats(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("state", "quality", "matches", "attempts", "inliers", "outliers", "n_corners",
                                       "align_meas", "keyframe", "relocalized")] + [("pose", C.c_double * 7)] + [
        (n, C.c_int) for n in ("align_features", "align_iters", "search_requests", "lk_iters", "host_path")]


_lib = None


def load_host_library():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError("libsdvl_host.so is not built (%s): run __graft_entry__.build()" % HOST_LIB_PATH)
        lib = C.CDLL(HOST_LIB_PATH)
        lib.sdvlh_last_error.restype = C.c_char_p
        lib.sdvlh_device_create.restype = C.c_void_p
        lib.sdvlh_device_ctx.restype = C.c_void_p
        lib.sdvlh_device_ctx.argtypes = [C.c_void_p]
        lib.sdvlh_device_destroy.argtypes = [C.c_void_p]
        lib.sdvlh_batch_create.restype = C.c_void_p
        lib.sdvlh_batch_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.sdvlh_batch_destroy.argtypes = [C.c_void_p]
        lib.sdvlh_batch_step_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.sdvlh_batch_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.sdvlh_batch_step_device_transient.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.sdvlh_batch_set_next_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.sdvlh_config_set.argtypes = [C.c_char_p, C.c_double]
        _lib = lib
    return _lib


# config/config_tum_f1.cfg:34-42 over the defaults of config.cc:55-85
TUM_OVERRIDES = {"SDVL.cell_size": 32, "SDVL.min_avg_shift": 5, "SDVL.max_matches": 200, "SDVL.max_keyframes": 1000,
                 "SDVL.use_orb": 1, "SDVL.fast_threshold": 10, "SDVL.lost_ratio": 0.7, "SDVL.num_features": 1000}


def configure(overrides=None):
    lib = load_host_library()
    lib.sdvlh_config_reset()
    for k, v in (TUM_OVERRIDES if overrides is None else overrides).items():
        if lib.sdvlh_config_set(k.encode(), float(v)) != 0:
            raise KeyError(k)


def set_device_pose(on):
    """pose stage (RANSAC + refinement, feature_align.cc:73-82,152-243) on the device (default) or the host implementation"""
    load_host_library().sdvlh_set_device_pose(int(bool(on)))


def set_track_tables(on):
    """device-resident tracking tables (default) on / off: off = the host assembles every request"""
    load_host_library().sdvlh_set_track_tables(int(bool(on)))


def set_device_filter(on):
    """the mapper's depth filter (Point::Update / HasConverged behind the candidate search) on the device (default) / on the host"""
    load_host_library().sdvlh_set_device_filter(int(bool(on)))


def bind_to_gpu_numa_node(gpu=0):
    """Restrict this process (and the threads it creates later) to the CPUs of the NUMA node the GPU hangs off: the host
    objects of the trackers, the pinned staging buffers and the doorbell writes then stay on that socket.  Returns the
    node, or None when the topology cannot be read (nothing is changed then).  Call it before creating devices."""
    import os
    try:
        import torch
        p = torch.cuda.get_device_properties(gpu)
        bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read())
        if node < 0:
            return None
        cpus = set()
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return node
    except (OSError, ValueError, AttributeError, RuntimeError):
        return None


def set_mapper(on):
    """map mode of the batches / farms created afterwards: the reference's mapper in sequential mode (map.cc) instead of
    the plane map stub; the first keyframe is bootstrapped from the scene plane in both modes unless the batch is told
    TrackerBatch.set_two_frame_init(True)"""
    load_host_library().sdvlh_set_mapper(int(bool(on)))


def device_pose():
    return bool(load_host_library().sdvlh_device_pose())


class HostDevice:
    def __init__(self, gpu=0):
        self.lib = load_host_library()
        self.h = self.lib.sdvlh_device_create(gpu)
        if not self.h:
            raise RuntimeError("no MI355X: %s" % self.lib.sdvlh_last_error().decode())

    def ctx_handle(self):
        return self.lib.sdvlh_device_ctx(self.h)

    def close(self):
        if self.h:
            self.lib.sdvlh_device_destroy(self.h)
            self.h = None


# enum sdvl_pixel_format (include/sdvl_hip.h) and the bytes per pixel of each
# and enum sdvl_raw_format (16 ..): Bayer mosaics named by their top-left 2x2 tile, YUV 4:2:2, little-endian 16-bit gray
PIXEL_FORMATS = {"gray": 0, "rgb": 1, "bgr": 2, "rgba": 3, "bgra": 4,
                 "bayer_rggb": 16, "bayer_grbg": 17, "bayer_gbrg": 18, "bayer_bggr": 19,
                 "yuyv": 20, "uyvy": 21, "gray10": 22, "gray12": 23, "gray16": 24}
PIXEL_CHANNELS = {0: 1, 1: 3, 2: 3, 3: 4, 4: 4, 16: 1, 17: 1, 18: 1, 19: 1, 20: 2, 21: 2, 22: 2, 23: 2, 24: 2}   # bytes per pixel


def pixel_format(fmt):
    """a pixel format name or SDVL_* value -> the SDVL_* value"""
    code = PIXEL_FORMATS.get(fmt.lower()) if isinstance(fmt, str) else int(fmt)
    if code not in PIXEL_CHANNELS:
        raise ValueError("unknown pixel format %r (one of %s)" % (fmt, ", ".join(PIXEL_FORMATS)))
    return code


class TrackerBatch:
    def __init__(self, dev, B, w, h, cam4, plane4=(0, 0, 1, 2.0), first_poses=None, host_threads=1):
        self.lib = dev.lib
        self.dev = dev
        self.B, self.w, self.h_img = B, w, h
        self.channels = 1   # set_color
        self.depth_dtype = np.float32   # set_depth
        cam4 = np.ascontiguousarray(cam4, np.float64)
        plane4 = np.ascontiguousarray(plane4, np.float64)
        if first_poses is None:
            first_poses = np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float64), (B, 1))
        first_poses = np.ascontiguousarray(first_poses, np.float64).reshape(B, 7)
        self.h = self.lib.sdvlh_batch_create(dev.h, B, w, h, cam4.ctypes.data, plane4.ctypes.data, first_poses.ctypes.data, host_threads)
        if not self.h:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        self._stats = (FrameStats * B)()

    def _step_depth(self, name, ptrs, depth_ptrs):
        """a step call with the B depth pointers beside the images (None entries: no depth image for that tracker)"""
        fn = getattr(self.lib, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert len(depth_ptrs) == self.B, "one depth image per tracker (None: none)"
        dptrs = (C.c_void_p * self.B)(*[None if p is None else int(p) for p in depth_ptrs])
        if fn(self.h, ptrs, self.w * self.channels, dptrs, self._stats) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        return self._stats

    @staticmethod
    def _second(depths, rights, names):
        """the step calls' second images under either name: depths= / depth_ptrs= or rights= / right_ptrs= (set_stereo), never both"""
        if depths is not None and rights is not None:
            raise ValueError("%s and %s name the same argument: give one" % names)
        return depths if rights is None else rights

    def step_host(self, imgs, depths=None, rights=None):
        """depths (set_depth): per tracker the frame's registered depth image, numpy [h, w] float32 or uint16 as set_depth named it, or None;
        rights (set_stereo): another name for the same argument — per tracker the pair's rectified right image, numpy [h, w] uint8, or None"""
        depths = self._second(depths, rights, ("depths", "rights"))
        # (16-bit gray frames go as their little-endian bytes)
        imgs = [np.ascontiguousarray(im, "<u2").view(np.uint8) if np.asarray(im).dtype == np.uint16 else np.ascontiguousarray(im, np.uint8) for im in imgs]
        ptrs = (C.c_void_p * self.B)(*[im.ctypes.data for im in imgs])
        if depths is not None:
            depths = [None if d is None else np.ascontiguousarray(d, self.depth_dtype).reshape(self.h_img, self.w) for d in depths]
            return self._step_depth("sdvlh_batch_step_host_depth", ptrs, [None if d is None else d.ctypes.data for d in depths])
        if self.lib.sdvlh_batch_step_host(self.h, ptrs, self.w * self.channels, self._stats) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        return self._stats

    def step_device(self, dev_ptrs, depth_ptrs=None, right_ptrs=None):
        """depth_ptrs (set_depth): per tracker the device pointer of the frame's registered depth image (dense rows), or None; right_ptrs
        (set_stereo): another name for the same argument — the device pointers of the pairs' right images"""
        depth_ptrs = self._second(depth_ptrs, right_ptrs, ("depth_ptrs", "right_ptrs"))
        ptrs = (C.c_void_p * self.B)(*[int(p) for p in dev_ptrs])
        if depth_ptrs is not None:
            return self._step_depth("sdvlh_batch_step_device_depth", ptrs, depth_ptrs)
        if self.lib.sdvlh_batch_step_device(self.h, ptrs, self.w * self.channels, self._stats) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        return self._stats

    def set_depth(self, on=True, format="f32", scale=1.0, edge_ratio=0.0, min_valid=0, min_depth=0.0, max_depth=0.0):
        """depth cameras: the trackers seed their keyframes' points from the registered depth image handed over with each frame (depths= /
        depth_ptrs= of the step calls) instead of the scene plane — every keyframe on the plane map, the bootstrap keyframe with the
        reference's mapper.  format "f32" (metres) or "u16" (units of `scale` metres: TUM 1 / 5000, millimetres 0.001); the rule's fields
        as sdvl_depth_seed_params (0: the default — edge_ratio 0.05, min_valid 6, min_depth 0.05, no max_depth).  A first frame without a
        depth image, or with fewer usable corners than SDVL.min_init_corners, is not kept (state 0) and the next frame starts over.
        Raises together with set_two_frame_init(True)"""
        code = {"f32": 0, "u16": 1}.get(format.lower() if isinstance(format, str) else None)
        if code is None:
            raise ValueError("unknown depth format %r (f32 or u16)" % (format,))
        self.lib.sdvlh_batch_set_depth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double]
        if self.lib.sdvlh_batch_set_depth(self.h, int(bool(on)), code, float(scale), float(edge_ratio), int(min_valid), float(min_depth),
                                          float(max_depth)) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        self.depth_dtype = np.uint16 if code == 1 else np.float32

    def set_stereo(self, baseline, on=True, min_depth=0.0, max_depth=0.0, max_disparity=0, max_sad=0, uniqueness=0):
        """stereo cameras: depth seeding's keyframe path with a sparse stereo matcher as the producer (SDVL::SetStereoSeeding).  The second
        image handed over with each frame (rights= / right_ptrs= of the step calls, or depths= / depth_ptrs=) is the pair's rectified right
        image: 8-bit gray of the camera image's size and intrinsics, dense rows, the right camera `baseline` metres along the left camera's
        x axis.  The filtered corners of the step's keyframes are matched in it by one sdvl_stereo_depth call — every keyframe on the plane
        map, the bootstrap keyframe with the reference's mapper.  The rule's fields as sdvl_stereo_params (0: the default — min_depth 0.3 m,
        no max_depth, max_disparity 192, max_sad 20 per sample, uniqueness 80); the trackers share baseline and rule.  A first frame
        without a right image, or with fewer OK corners than SDVL.min_init_corners, is not kept (state 0) and the next frame starts over.
        Raises together with set_two_frame_init(True), set_depth(True), set_depth_mapping, set_depth_bundle and on a camera with a lens"""
        self.lib.sdvlh_batch_set_stereo.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]
        if self.lib.sdvlh_batch_set_stereo(self.h, int(bool(on)), float(baseline), float(min_depth), float(max_depth), int(max_disparity),
                                           int(max_sad), int(uniqueness)) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        self.depth_dtype = np.uint8 if on else np.float32

    def set_stereo_rectification(self, rig=None, on=True, plan_only=False):
        """stereo rigs as calibrated (SDVL::SetStereoRectification; needs set_stereo): rig = (K1, D1, K2, D2, R, T) with K_i = fx fy u0 v0,
        D_i = k1 k2 p1 p2 k3, R [3][3] and T [3] such that X_right = R X_left + T.  The rig is planned for the batch's image size and the
        step calls then take the RAW images of both cameras (imgs and rights=): the left one is rectified inside its frame's upload, the
        right ones into HBM in one launch per step, and only in a step that reads them.  Returns (rectified camera fx fy u0 v0, baseline):
        the batch must have been made with that camera and set_stereo called with that baseline — plan_only=True returns them without
        setting anything, on any batch of the image size.  Poses are the rectified left camera's.  Raises RuntimeError for a rig the plan
        refuses, without set_stereo, on a camera with a lens of its own, when camera or baseline differ from the plan's and with the
        mapper thread started."""
        self.lib.sdvlh_batch_set_stereo_rectification.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        if not on:
            if self.lib.sdvlh_batch_set_stereo_rectification(self.h, 0, None, 0, None) != 0:
                raise RuntimeError(self.lib.sdvlh_last_error().decode())
            return None
        K1, D1, K2, D2, R, T = rig
        rig30 = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).ravel() for v in (K1, D1, K2, D2, R, T)]))
        assert rig30.shape == (30,), "rig = (K1[4], D1[5], K2[4], D2[5], R[3][3], T[3])"
        out = np.zeros(5)
        if self.lib.sdvlh_batch_set_stereo_rectification(self.h, 1, rig30.ctypes.data, int(bool(plan_only)), out.ctypes.data) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        return out[:4].copy(), float(out[4])

    def stereo_stats(self, i):
        """tracker i's stereo seeding so far: dict(keyframes, seeds, ok, nomatch, ambiguous, edge, outside, no_image) — keyframes seeded,
        points seeded, the keyframes' filtered corners by status, keyframes or first frames that came without a right image"""
        out = (C.c_longlong * 8)()
        self.lib.sdvlh_batch_stereo_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self.lib.sdvlh_batch_stereo_stats(self.h, int(i), out) != 0:
            raise RuntimeError("no tracker %d" % i)
        return dict(zip(("keyframes", "seeds", "ok", "nomatch", "ambiguous", "edge", "outside", "no_image"), [int(v) for v in out]))

    def seeded_points(self, i):
        """the live points tracker i seeded from depth, oldest first: rows of x y z keyframe_id u v level (float64; u, v in level coordinates)"""
        self.lib.sdvlh_batch_seeded_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        n = self.lib.sdvlh_batch_seeded_points(self.h, int(i), 0, None)
        if n < 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode() if n == -2 else "no tracker %d" % i)
        out = np.zeros((max(n, 1), 7), np.float64)
        n = self.lib.sdvlh_batch_seeded_points(self.h, int(i), n, out.ctypes.data)
        return out[:n].copy()

    def depth_stats(self, i):
        """tracker i's depth seeding so far: dict(keyframes, seeds, ok, hole, few, edge, outside, no_depth) — keyframes seeded, points
        seeded, the keyframes' filtered corners by status, keyframes or first frames that came without a depth image"""
        out = (C.c_longlong * 8)()
        self.lib.sdvlh_batch_depth_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self.lib.sdvlh_batch_depth_stats(self.h, int(i), out) != 0:
            raise RuntimeError("no tracker %d" % i)
        return dict(zip(("keyframes", "seeds", "ok", "hole", "few", "edge", "outside", "no_depth"), [int(v) for v in out]))

    def set_depth_mapping(self, on=True, noise_abs=0.0, noise_quad=0.0):
        """depth cameras inside the reference's mapper (SDVL::SetDepthMapping; needs set_depth and a mapper batch): the depth image of
        every tracked frame feeds the candidates' depth filter as a measurement (sdvl_search_run_filter_measured), and the corners of a
        new keyframe become fixed points at their measured depth — matched in a connected keyframe or on the new keyframe alone.  The
        sensor's depth noise is tau = noise_abs + noise_quad z^2 (0: 0.001 m and 0.0015 per metre, an order of magnitude and not a
        measurement); the trackers share it.  The points fixed from depth join seeded_points.  Raises RuntimeError without depth seeding,
        without the mapper, with the mapper thread started and with the host depth filter."""
        self.lib.sdvlh_batch_set_depth_mapping.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
        if self.lib.sdvlh_batch_set_depth_mapping(self.h, int(bool(on)), float(noise_abs), float(noise_quad)) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())

    def depth_map_stats(self, i):
        """tracker i's depth mapping so far: dict(measured, hole, few, edge, outside, keyframes, fixed_matched, fixed_unmatched, linked) —
        candidate updates that took the measured depth and those that fell back by the lookup's status, keyframes whose corners were looked
        up, corners fixed and matched in a connected keyframe, fixed on the new keyframe alone, and measured corners linked to a point"""
        out = (C.c_longlong * 9)()
        self.lib.sdvlh_batch_depth_map_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self.lib.sdvlh_batch_depth_map_stats(self.h, int(i), out) != 0:
            raise RuntimeError("no tracker %d, or not a mapper batch" % i)
        return dict(zip(("measured", "hole", "few", "edge", "outside", "keyframes", "fixed_matched", "fixed_unmatched", "linked"), [int(v) for v in out]))

    def set_stereo_mapping(self, on=True, disparity_sigma=0.0):
        """stereo cameras inside the reference's mapper (SDVL::SetStereoMapping; needs set_stereo and a mapper batch): the right image of
        every tracked frame feeds the candidates' depth filter through the stereo matcher at the found pixel
        (sdvl_search_run_filter_stereo), and the corners of a new keyframe become fixed points at the depth sdvl_stereo_depth gives them —
        matched in a connected keyframe or on the new keyframe alone.  The depth noise is tau = disparity_sigma z^2 / (fx baseline);
        disparity_sigma in pixels, 0: 0.25, an order of magnitude that nobody has measured against a real pair (on the synthetic `shelf`
        scene the matcher's median error is 0.04 - 0.07 px); the trackers share it.  A frame without a right image is mapped as before.
        The points fixed from the pair join seeded_points; stereo_stats keeps counting what the driver seeds.  Raises RuntimeError without
        stereo seeding, without the mapper, with the mapper thread started, with the host depth filter and for a negative or non-finite
        disparity_sigma; while it is on, set_stereo(on=False) raises."""
        self.lib.sdvlh_batch_set_stereo_mapping.argtypes = [C.c_void_p, C.c_int, C.c_double]
        if self.lib.sdvlh_batch_set_stereo_mapping(self.h, int(bool(on)), float(disparity_sigma)) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())

    def stereo_map_stats(self, i):
        """tracker i's stereo mapping so far: dict(measured, nomatch, ambiguous, edge, outside, keyframes, fixed_matched, fixed_unmatched,
        linked) — candidate updates that took the matcher's depth and those that fell back by its status, keyframes whose corners were
        matched, corners fixed and matched in a connected keyframe, fixed on the new keyframe alone, and measured corners linked to a point"""
        out = (C.c_longlong * 9)()
        self.lib.sdvlh_batch_stereo_map_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self.lib.sdvlh_batch_stereo_map_stats(self.h, int(i), out) != 0:
            raise RuntimeError("no tracker %d, or not a mapper batch" % i)
        return dict(zip(("measured", "nomatch", "ambiguous", "edge", "outside", "keyframes", "fixed_matched", "fixed_unmatched", "linked"),
                        [int(v) for v in out]))

    def set_next_device(self, dev_ptrs):
        """look-ahead: the device images the NEXT step_device call will be given (None: none); their pyramids and corner detection
        are queued behind the coming step's search / pose chain (SDVLBatch::SetNextImages).  The buffers must keep their CONTENT until that
        call: the look-ahead is recognised by device address alone.  It belongs to the one coming step and is dropped if that step cannot use it"""
        ptrs = (C.c_void_p * self.B)(*[int(p) for p in dev_ptrs]) if dev_ptrs is not None else None
        if self.lib.sdvlh_batch_set_next_device(self.h, ptrs, self.w * self.channels) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())

    def set_distortion(self, dist5):
        """the batch's camera gets a lens (Camera.d1..d5 of the reference's cfg files) and the images of every later step are RAW camera
        frames: Camera::UndistortImage (main.cc:133) runs inside the step, fused into the frames' upload"""
        d = np.ascontiguousarray(dist5, np.float64)
        self.lib.sdvlh_batch_set_distortion.argtypes = [C.c_void_p, C.c_void_p]
        if self.lib.sdvlh_batch_set_distortion(self.h, d.ctypes.data) != 0:
            raise RuntimeError("sdvlh_batch_set_distortion")

    def set_color(self, fmt):
        """the images of every later step are COLOUR camera frames (h x w x channels, interleaved) of pixel format `fmt` ("gray", "rgb",
        "bgr", "rgba", "bgra" or the SDVL_* value): cv::cvtColor (video_source.cc:63) runs on the device inside the step, before the
        undistortion of set_distortion.  "rgb" puts the R weight on byte 0 — what main.cc computes on cv::VideoCapture's BGR bytes.
        RAW camera formats (enum sdvl_raw_format) go the same way: "bayer_rggb" / "bayer_grbg" / "bayer_gbrg" / "bayer_bggr" (h x w bytes,
        named by the 2x2 tile at the top-left corner), "yuyv" / "uyvy" (h x w x 2 bytes, even w), "gray10" / "gray12" / "gray16" (h x w
        little-endian uint16).  Row strides are w x bytes per pixel"""
        code = pixel_format(fmt)
        self.lib.sdvlh_batch_set_color.argtypes = [C.c_void_p, C.c_int]
        if self.lib.sdvlh_batch_set_color(self.h, code) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        self.channels = PIXEL_CHANNELS[code]

    def set_two_frame_init(self, on=True):
        """the trackers start from the camera alone: the reference's two-frame initialisation (first frame's corners tracked by device
        KLT until the median shift reaches SDVL.min_avg_shift, homography by device RANSAC, decomposition, triangulation, points as
        depth-filter candidates) instead of the plane bootstrap.  FrameStats.state is 0 on the first frame, 1 while the second frame is
        awaited, 2 from the frame that initialises.  Requires the reference's mapper: call set_mapper(True) BEFORE creating the batch,
        otherwise this raises"""
        self.lib.sdvlh_batch_set_two_frame_init.argtypes = [C.c_void_p, C.c_int]
        if self.lib.sdvlh_batch_set_two_frame_init(self.h, int(bool(on))) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())

    def set_bundle_adjustment(self, on=True):
        """the trackers' mappers run the reference's local bundle adjustment (Map::BundleAdjustment, map.cc:130-137,844-869) after every
        keyframe update of a map with more than two keyframes: the windows of all trackers of a step are solved in one sdvl_bundle_adjust
        call.  Off by default.  Requires the reference's mapper: call set_mapper(True) BEFORE creating the batch, otherwise this raises"""
        self.lib.sdvlh_batch_set_bundle_adjustment.argtypes = [C.c_void_p, C.c_int]
        if self.lib.sdvlh_batch_set_bundle_adjustment(self.h, int(bool(on))) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())

    def set_depth_bundle(self, on=True, bf=0.0):
        """depth edges in the local bundle adjustment (SDVL::SetDepthBundle; needs set_depth and set_bundle_adjustment): an observation
        that carries a measured depth — the corners a keyframe was seeded from, and the tracked features a frame held when it became a
        keyframe in a step that was handed its depth image — becomes a three-row edge (sdvl_bundle_adjust_depth), which fixes the
        scale a window with one fixed keyframe leaves free.  Features added to a keyframe in a later step stay monocular edges.  bf
        (pixel x metres) turns depth noise into pixels; 0: 1 / noise_quad of set_depth_mapping (666.7 at its default), an order of
        magnitude that nobody has measured against a sensor.  Off by default.  Raises RuntimeError without depth seeding, without bundle
        adjustment on, with the mapper thread started and for a negative or non-finite bf."""
        self.lib.sdvlh_batch_set_depth_bundle.argtypes = [C.c_void_p, C.c_int, C.c_double]
        if self.lib.sdvlh_batch_set_depth_bundle(self.h, int(bool(on)), float(bf)) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())

    def depth_bundle_stats(self, i):
        """tracker i's depth edges so far: dict(ok, hole, few, edge, outside: the lookups of new keyframes' features by status; stored:
        observations that got a depth; features: the features handed to the lookup; last / total: dict(edges, depth_edges, depth_level1) of
        the last window and of all windows)"""
        out = (C.c_longlong * 13)()
        self.lib.sdvlh_batch_depth_bundle_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self.lib.sdvlh_batch_depth_bundle_stats(self.h, int(i), out) != 0:
            raise RuntimeError("no tracker %d, or not a mapper batch" % i)
        v = [int(x) for x in out]
        d = dict(zip(("ok", "hole", "few", "edge", "outside", "stored"), v[:6]))
        d["last"] = dict(zip(("edges", "depth_edges", "depth_level1"), v[6:9]))
        d["total"] = dict(zip(("edges", "depth_edges", "depth_level1"), v[9:12]))
        d["features"] = v[12]
        return d

    def bundle_stats(self, i):
        """mapper mode only: dict(runs, skipped, n_free, n_fixed, n_points, n_edges, last) of tracker i; `last` is the BundleResult
        (sdvl_bundle_result) of its last window, zeros before the first run"""
        from . import BundleResult
        counts = (C.c_longlong * 6)()
        last = BundleResult()
        self.lib.sdvlh_batch_bundle_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        if self.lib.sdvlh_batch_bundle_stats(self.h, int(i), counts, C.byref(last)) != 0:
            raise RuntimeError("tracker %d has no mapper" % i)
        out = dict(zip(("runs", "skipped", "n_free", "n_fixed", "n_points", "n_edges"), [int(c) for c in counts]))
        out["last"] = last
        return out

    def keyframe_poses(self, i):
        """(frame ids, poses[n][7]) of tracker i's keyframes, oldest first"""
        self.lib.sdvlh_batch_keyframe_poses.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        n = self.lib.sdvlh_batch_keyframe_poses(self.h, int(i), 0, None, None)
        poses = np.zeros((max(n, 1), 7), np.float64)
        ids = np.zeros(max(n, 1), np.int32)
        n = self.lib.sdvlh_batch_keyframe_poses(self.h, int(i), n, poses.ctypes.data, ids.ctypes.data)
        return ids[:n].copy(), poses[:n].copy()

    def step_device_transient(self, dev_ptrs, depth_ptrs=None, right_ptrs=None):
        """frames in HBM that stay valid for THIS step only (a slot of an input ring): aliased while tracked, frames that become
        keyframes take a copy at the end of the step.  depth_ptrs / right_ptrs as for step_device: a second image is read inside the step only"""
        depth_ptrs = self._second(depth_ptrs, right_ptrs, ("depth_ptrs", "right_ptrs"))
        ptrs = (C.c_void_p * self.B)(*[int(p) for p in dev_ptrs])
        if depth_ptrs is not None:
            return self._step_depth("sdvlh_batch_step_device_transient_depth", ptrs, depth_ptrs)
        if self.lib.sdvlh_batch_step_device_transient(self.h, ptrs, self.w * self.channels, self._stats) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        return self._stats

    STAGES = ["upload_pyr", "fast", "select", "corners_orb", "prelude", "image_align", "prepare", "search", "finish", "pose", "mapping",
              "epilogue", "mapper", "total", "map_candidates", "map_connections", "map_init", "map_finish",
              "map_begin", "map_emit", "map_search", "map_apply", "relocalize", "map_bundle"]

    def map_stats(self, i):
        """mapper mode only: candidates, converged, initialized, linked, connected, keyframes of tracker i"""
        out = (C.c_int * 6)()
        self.lib.sdvlh_batch_map_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self.lib.sdvlh_batch_map_stats(self.h, int(i), out) != 0:
            raise RuntimeError("tracker %d has no mapper" % i)
        return dict(zip(("candidates", "converged", "initialized", "linked", "connected", "keyframes"), list(out)))

    def map_points(self, i):
        """mapper mode only: the live points tracker i's mapper created, rows of x y z fixed (float64) — keyframes oldest first, each
        keyframe's features in order, each point once; deleted points and the bootstrap keyframe's own points are left out"""
        self.lib.sdvlh_batch_map_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        n = self.lib.sdvlh_batch_map_points(self.h, int(i), 0, None)
        if n == -1:
            raise RuntimeError("tracker %d has no mapper" % i)
        if n < 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        out = np.zeros((max(n, 1), 4), np.float64)
        n = self.lib.sdvlh_batch_map_points(self.h, int(i), n, out.ctypes.data)
        return out[:n].copy()

    def stage_times(self, reset=False):
        """accumulated wall seconds per host stage of SDVLBatch::HandleFrames -> (dict, steps)"""
        out = (C.c_double * len(self.STAGES))()
        self.lib.sdvlh_batch_stage_times.restype = C.c_long
        self.lib.sdvlh_batch_stage_times.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        n = self.lib.sdvlh_batch_stage_times(self.h, out, len(self.STAGES), int(reset))
        return {k: out[i] for i, k in enumerate(self.STAGES)}, n

    def close(self):
        if self.h:
            self.lib.sdvlh_batch_destroy(self.h)
            self.h = None


class TrackerFarm:
    """G groups x Bg sequences on one GPU; each group = host thread + sdvl_ctx (stream) + SDVLBatch, free-running."""

    def __init__(self, gpu, G, Bg, w, h, cam4, plane4=(0, 0, 1, 2.0), first_poses=None, host_threads_per_group=1):
        self.lib = load_host_library()
        self.G, self.Bg, self.w, self.h_img = G, Bg, w, h
        self.channels = 1   # set_color
        n = G * Bg
        cam4 = np.ascontiguousarray(cam4, np.float64)
        plane4 = np.ascontiguousarray(plane4, np.float64)
        if first_poses is None:
            first_poses = np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float64), (n, 1))
        first_poses = np.ascontiguousarray(first_poses, np.float64).reshape(n, 7)
        self.lib.sdvlh_farm_create.restype = C.c_void_p
        self.lib.sdvlh_farm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        self.lib.sdvlh_farm_destroy.argtypes = [C.c_void_p]
        self.lib.sdvlh_farm_ctx.restype = C.c_void_p
        self.lib.sdvlh_farm_ctx.argtypes = [C.c_void_p, C.c_int]
        self.lib.sdvlh_farm_batch.restype = C.c_void_p
        self.lib.sdvlh_farm_batch.argtypes = [C.c_void_p, C.c_int]
        self.lib.sdvlh_farm_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        self.lib.sdvlh_farm_reserve.argtypes = [C.c_void_p, C.c_int]
        self.h = self.lib.sdvlh_farm_create(gpu, G, Bg, w, h, cam4.ctypes.data, plane4.ctypes.data, first_poses.ctypes.data,
                                            host_threads_per_group)
        if not self.h:
            raise RuntimeError("no MI355X: %s" % self.lib.sdvlh_last_error().decode())

    def ctx_handle(self, g=0):
        return self.lib.sdvlh_farm_ctx(self.h, g)

    def reserve(self, frames_per_group):
        """pool HBM frames up front (keyframes keep theirs): no hipMalloc on the tracking path for that many frames"""
        if self.lib.sdvlh_farm_reserve(self.h, int(frames_per_group)) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())

    def set_distortion(self, dist5):
        """every group's camera gets the lens; the frames of run() are RAW camera frames from then on (TrackerBatch.set_distortion)"""
        d = np.ascontiguousarray(dist5, np.float64)
        self.lib.sdvlh_batch_set_distortion.argtypes = [C.c_void_p, C.c_void_p]
        for g in range(self.G):
            if self.lib.sdvlh_batch_set_distortion(self.lib.sdvlh_farm_batch(self.h, g), d.ctypes.data) != 0:
                raise RuntimeError("sdvlh_batch_set_distortion")

    def set_color(self, fmt):
        """every group's frames are COLOUR or RAW camera frames of `fmt` (TrackerBatch.set_color).  Formats of more than one byte per pixel
        must be resident in HBM: run() refuses them together with set_host_input (the host input and its input ring carry one byte per
        pixel).  The four Bayer formats are one byte per pixel: they ride the host input, with or without the ring, as gray does, and are
        converted inside the step"""
        code = pixel_format(fmt)
        self.lib.sdvlh_farm_set_color.argtypes = [C.c_void_p, C.c_int]
        if self.lib.sdvlh_farm_set_color(self.h, code) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        self.channels = PIXEL_CHANNELS[code]

    def set_fibers(self, n):
        """n > 1: every worker thread interleaves n group-steps, switching at GPU waits (use G = n * workers groups)"""
        self.lib.sdvlh_farm_set_fibers.argtypes = [C.c_void_p, C.c_int]
        self.lib.sdvlh_farm_set_fibers(self.h, int(n))

    def set_host_input(self, on):
        """the pointers of run() are HOST pointers (pinned memory): every step uploads its frames inside the step"""
        self.lib.sdvlh_farm_set_host_input.argtypes = [C.c_void_p, C.c_int]
        self.lib.sdvlh_farm_set_host_input(self.h, int(bool(on)))

    def alloc_stats(self, n_steps):
        """output records for run(); touched here so that the workers do not take the first-touch page faults"""
        out = (FrameStats * (n_steps * self.G * self.Bg))()
        C.memset(out, 0, C.sizeof(out))
        return out

    def run(self, dev_frames, workers=0, out=None):
        """dev_frames: int array [n_steps, G*Bg] of device pointers -> FrameStats array [n_steps*G*Bg];
        workers = host threads (0 = one per group); workers < G schedules group-steps dynamically"""
        dev_frames = np.ascontiguousarray(dev_frames, np.uint64)
        n_steps = dev_frames.shape[0]
        assert dev_frames.shape[1] == self.G * self.Bg
        if out is None:
            out = self.alloc_stats(n_steps)
        assert len(out) >= n_steps * self.G * self.Bg
        if self.lib.sdvlh_farm_run(self.h, n_steps, dev_frames.ctypes.data, self.w * self.channels, out, int(workers)) != 0:
            raise RuntimeError(self.lib.sdvlh_last_error().decode())
        return out

    def feed_stats(self):
        """last host-fed run -> (seconds the feeder spent inside the transfer calls, seconds it waited for a free ring slot, transfers,
        seconds the workers waited for their transfer to be issued and to arrive (summed over groups), group-steps that began before their
        images had arrived, seconds the feeder waited for its own earlier transfers)"""
        out = (C.c_double * 6)()
        self.lib.sdvlh_farm_feed_stats.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.sdvlh_farm_feed_stats(self.h, out)
        return out[0], out[1], int(out[2]), out[3], int(out[4]), out[5]

    def set_input_ring(self, on):
        """host-fed runs: the images of step s + 1 travel on the group's copy stream while step s computes (default on)"""
        self.lib.sdvlh_farm_set_input_ring.argtypes = [C.c_void_p, C.c_int]
        self.lib.sdvlh_farm_set_input_ring(self.h, int(bool(on)))

    def stage_times(self, reset=False):
        tot, steps = None, 0
        self.lib.sdvlh_batch_stage_times.restype = C.c_long
        self.lib.sdvlh_batch_stage_times.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        for g in range(self.G):
            out = (C.c_double * len(TrackerBatch.STAGES))()
            n = self.lib.sdvlh_batch_stage_times(self.lib.sdvlh_farm_batch(self.h, g), out, len(TrackerBatch.STAGES), int(reset))
            steps += n
            tot = [a + b for a, b in zip(tot, out)] if tot else list(out)
        return {k: tot[i] for i, k in enumerate(TrackerBatch.STAGES)}, steps

    def close(self):
        if self.h:
            self.lib.sdvlh_farm_destroy(self.h)
            self.h = None
