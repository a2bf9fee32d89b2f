"""Colour camera frames on the MI355X: cv::cvtColor(frame, img, CV_*2GRAY) (video_source.cc:63) as to_gray_kernel, standalone
(sdvl_convert_gray) and fused into the frames' upload ahead of the undistortion (sdvl_frames_upload_color, main.cc:128-137), checked bit
for bit against the numpy restatement of OpenCV's luma and the oracle's cv::undistort; closed-loop tracking of colour frames against the
oracle fed the numpy gray."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from oraclelib import TUM_CAM, TUM_DIST, XI, trajectory_pose
from test_color_cpu import to_gray

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {"rgb": 1, "bgr": 2, "rgba": 3, "bgra": 4}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def trk():
    importlib.import_module("slam-sdvl_amd")
    return importlib.import_module("slam-sdvl_amd.tracker")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def colourise(gray, seed, channels=3):
    """a colour frame whose luma is not its gray source: seeded per-channel offsets, so that the weights and their order matter"""
    rng = np.random.default_rng(seed)
    off = rng.integers(-40, 41, (channels,))
    noise = rng.integers(-6, 7, gray.shape + (channels,))
    return np.clip(gray[..., None].astype(np.int32) + off + noise, 0, 255).astype(np.uint8)


def convert(ctx, srcs, src_stride, on_device, w, h, fmt, dst_stride=None):
    """sdvl_convert_gray over raw addresses -> numpy gray images [n, h, w]"""
    n = len(srcs)
    ds = dst_stride or w
    buf = ctx.device_malloc(n * ds * h)
    try:
        dst = (C.c_void_p * n)(*[buf + i * ds * h for i in range(n)])
        src = (C.c_void_p * n)(*[int(p) for p in srcs])
        lib = ctx.lib
        lib.sdvl_convert_gray.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        ctx._check(lib.sdvl_convert_gray(ctx.h, n, src, src_stride, int(on_device), w, h, CODES[fmt], dst, ds))
        out = ctx.device_download(buf, n * ds * h).reshape(n, h, ds)[:, :, :w]
    finally:
        ctx.device_free(buf)
    return out


def test_convert_gray_is_exhaustive(ctx):
    """one 4096 x 4096 image holds every (c0, c1, c2) triple once: all four formats equal numpy everywhere"""
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    alpha = np.random.default_rng(5).integers(0, 256, (4096, 4096, 1), dtype=np.uint8)
    for fmt in ("rgb", "bgr", "rgba", "bgra"):
        img = rgb if len(fmt) == 3 else np.concatenate([rgb, alpha], -1)
        got = ctx.convert_gray([img], CODES[fmt])[0]
        assert np.array_equal(got, to_gray(img, fmt)), fmt
    got = ctx.convert_gray([np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [90, 90, 90]]], np.uint8)], CODES["rgb"])[0]
    assert got.tolist() == [[76, 150, 29, 90]]


def _host_images(n, w, h, ch, pitch, offset, seed):
    """n colour images with row pitch `pitch` bytes, starting `offset` bytes into one buffer each -> (buffers, arrays)"""
    rng = np.random.default_rng(seed)
    bufs, views = [], []
    for i in range(n):
        raw = rng.integers(0, 256, offset + pitch * h, dtype=np.uint8)
        bufs.append(raw)
        views.append(np.lib.stride_tricks.as_strided(raw[offset:], (h, w, ch), (pitch, ch, 1)))
    return bufs, views


@pytest.mark.parametrize("w,h", [(640, 480), (752, 480), (1280, 960), (641, 480)])
def test_convert_gray_layouts(ctx, pkg, w, h):
    """dense and padded pitches (not multiples of 16), sources 1-15 bytes off alignment, from pageable, pinned and device memory"""
    import torch
    lib = ctx.lib
    for fmt in ("rgb", "bgra"):
        ch = len(fmt)
        for pitch, offset in ((w * ch, 0), (w * ch + 7, 0), (w * ch, 5), (w * ch + 33, 13), (w * ch + 16, 0)):
            n = 3
            bufs, views = _host_images(n, w, h, ch, pitch, offset, seed=w + pitch + offset)
            want = [to_gray(v, fmt) for v in views]
            # pageable
            got = convert(ctx, [b.ctypes.data + offset for b in bufs], pitch, False, w, h, fmt)
            for i in range(n):
                assert np.array_equal(got[i], want[i]), ("pageable", fmt, pitch, offset, i)
            # pinned
            pinned = C.c_void_p()
            total = len(bufs[0])
            ctx._check(lib.sdvl_host_alloc_pinned(ctx.h, C.c_int64(total * n), C.byref(pinned)))
            try:
                for i in range(n):
                    C.memmove(pinned.value + i * total, bufs[i].ctypes.data, total)
                got = convert(ctx, [pinned.value + i * total + offset for i in range(n)], pitch, False, w, h, fmt)
                ctx.synchronize()
            finally:
                ctx._check(lib.sdvl_host_free_pinned(ctx.h, pinned))
            for i in range(n):
                assert np.array_equal(got[i], want[i]), ("pinned", fmt, pitch, offset, i)
            # device, with a padded destination
            dev = torch.from_numpy(np.concatenate(bufs)).cuda()
            torch.cuda.synchronize()
            got = convert(ctx, [dev.data_ptr() + i * total + offset for i in range(n)], pitch, True, w, h, fmt, dst_stride=w + 3)
            for i in range(n):
                assert np.array_equal(got[i], want[i]), ("device", fmt, pitch, offset, i)
            del dev


def test_convert_gray_256_frames(ctx):
    """the bench's group size, n = 1 and n = 256, from pageable host memory and from HBM"""
    import torch
    w, h = 640, 480
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, (256, h, w, 3), dtype=np.uint8)
    for n in (1, 256):
        got = convert(ctx, [imgs[i].ctypes.data for i in range(n)], 3 * w, False, w, h, "bgr")
        assert np.array_equal(got, to_gray(imgs[:n], "bgr")), n
    dev = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    fb = h * w * 3
    got = convert(ctx, [dev.data_ptr() + i * fb for i in range(256)], 3 * w, True, w, h, "rgb")
    assert np.array_equal(got, to_gray(imgs, "rgb"))


def test_refuses_bad_arguments(ctx):
    lib = ctx.lib
    img = np.zeros((4, 8, 3), np.uint8)
    buf = ctx.device_malloc(64)
    try:
        src = (C.c_void_p * 1)(img.ctypes.data)
        dst = (C.c_void_p * 1)(buf)
        lib.sdvl_convert_gray.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        assert lib.sdvl_convert_gray(ctx.h, 1, src, 24, 0, 8, 4, 9, dst, 8) == -1
        assert b"format" in lib.sdvl_last_error(ctx.h)
        assert lib.sdvl_convert_gray(ctx.h, 1, src, 23, 0, 8, 4, 1, dst, 8) == -1
        assert b"stride" in lib.sdvl_last_error(ctx.h)
        same = (C.c_void_p * 1)(buf)
        assert lib.sdvl_convert_gray(ctx.h, 1, same, 24, 1, 8, 4, 1, same, 8) == -1
        assert b"in-place" in lib.sdvl_last_error(ctx.h)
        assert lib.sdvl_convert_gray(ctx.h, 1, None, 24, 0, 8, 4, 1, dst, 8) == -1
    finally:
        ctx.device_free(buf)


def test_frames_upload_color_through_the_lens(pkg, orc, synth):
    """level 0 = undistort(gray(raw)) bit for bit (not gray(undistort(raw))); the pyramid equals the gray upload's; one map per camera"""
    ctx = pkg.Context(0)
    try:
        w, h = 640, 480
        cam = pkg.Camera(w, h, *TUM_CAM)
        raws = [colourise(synth.render(trajectory_pose(orc, k), TUM_CAM, w, h, frame_id=k, dist=TUM_DIST), 300 + k) for k in range(3)]
        for fmt in ("rgb", "bgr"):
            grays = [to_gray(r, fmt) for r in raws]
            fc = [ctx.frame(width=w, height=h) for _ in raws]
            fg = [ctx.frame(width=w, height=h) for _ in raws]
            ctx.upload_color(fc, raws, CODES[fmt], cam, TUM_DIST)
            ctx.pyramid_build(fc)
            ctx.undistort(grays, cam, TUM_DIST, frames=fg)
            ctx.pyramid_build(fg)
            for i in range(3):
                want0 = orc.undistort(grays[i], TUM_CAM, TUM_DIST)
                assert np.array_equal(fc[i].level(0), want0), (fmt, i)
                for l in range(5):
                    assert np.array_equal(fc[i].level(l), fg[i].level(l)), (fmt, i, l)
            # without a lens (null cam / dist): level 0 is the gray image itself
            ctx.upload_color(fc, raws, CODES[fmt])
            for i in range(3):
                assert np.array_equal(fc[i].level(0), grays[i]), (fmt, i)
            for f in fc + fg:
                f.close()
        counters = (C.c_int64 * 4)()
        ctx.lib.sdvl_ctx_counters.argtypes = [C.c_void_p, C.c_void_p]
        assert ctx.lib.sdvl_ctx_counters(ctx.h, counters) == 0
        assert counters[2] == 1, counters[2]
    finally:
        ctx.close()


def _closed_loop(trk, orc, synth, fmt, lens, n_frames=8, B=2, check=True):
    trk.configure()
    dev = trk.HostDevice(0)
    xis = [XI * (1.0 + 0.15 * i) * (1 if i % 2 == 0 else -1) for i in range(B)]
    seeds = [20260001 + i for i in range(B)]
    batch = trk.TrackerBatch(dev, B, 640, 480, TUM_CAM)
    batch.set_color(fmt)
    if lens:
        batch.set_distortion(TUM_DIST)
    oracles = [orc.tracker(640, 480, TUM_CAM) for _ in range(B)]
    ch = 4 if fmt.endswith("a") else 3
    rows = []
    for k in range(n_frames):
        raw = [colourise(synth.render(trajectory_pose(orc, k, xis[i]), TUM_CAM, 640, 480, seed=seeds[i], frame_id=k,
                                      dist=TUM_DIST if lens else None), 1000 * k + i, ch) for i in range(B)]
        got = batch.step_host(raw)
        for i in range(B):
            g = got[i]
            rows.append((g.state, g.quality, g.keyframe, g.n_corners, g.matches, g.attempts, g.inliers, g.outliers, g.align_meas))
            if not check:
                continue
            gray = to_gray(raw[i], fmt)
            want = oracles[i].handle_frame(orc.undistort(gray, TUM_CAM, TUM_DIST) if lens else gray)
            assert rows[-1] == (want.state, want.quality, want.keyframe, want.n_corners, want.matches, want.attempts, want.inliers,
                                want.outliers, want.align_meas), (fmt, lens, k, i)
            assert np.abs(np.array(g.pose[:]) - np.array(want.pose[:])).max() <= POSE_TOL, (fmt, lens, k, i)
            if k > 0:
                assert g.quality == 0 and g.matches >= 100
    batch.close()
    for o in oracles:
        o.close()
    dev.close()
    return rows


@pytest.mark.parametrize("fmt,lens", [("rgb", False), ("rgb", True), ("bgr", True), ("bgra", False)])
def test_colour_frames_closed_loop(trk, orc, synth, fmt, lens):
    _closed_loop(trk, orc, synth, fmt, lens)


def test_swapping_the_byte_order_changes_the_result(trk, orc, synth):
    a = _closed_loop(trk, orc, synth, "rgb", False, n_frames=4, check=False)
    b = _closed_loop(trk, orc, synth, "bgr", False, n_frames=4, check=False)
    assert a != b


def test_lookahead_on_colour_device_frames(trk, orc, synth):
    """SDVLBatch::SetNextImages on colour frames in HBM: the look-ahead converts too, and gives the results of plain steps"""
    import torch
    trk.configure()
    B, n = 2, 6
    xis = [XI * (1.0 + 0.15 * i) * (1 if i % 2 == 0 else -1) for i in range(B)]
    frames = np.stack([np.stack([colourise(synth.render(trajectory_pose(orc, k, xis[i]), TUM_CAM, 640, 480, seed=20260001 + i, frame_id=k),
                                           77 * k + i) for i in range(B)]) for k in range(n)])
    dev_frames = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    fb = 640 * 480 * 3
    ptr = lambda k, i: dev_frames.data_ptr() + (k * B + i) * fb
    runs = []
    for ahead in (False, True):
        dev = trk.HostDevice(0)
        batch = trk.TrackerBatch(dev, B, 640, 480, TUM_CAM)
        batch.set_color("rgb")
        rows = []
        for k in range(n):
            if ahead and k >= 1 and k + 1 < n:
                batch.set_next_device([ptr(k + 1, i) for i in range(B)])
            got = batch.step_device([ptr(k, i) for i in range(B)])
            rows += [(g.state, g.quality, g.keyframe, g.n_corners, g.matches, g.attempts, g.inliers, g.outliers, tuple(g.pose[:])) for g in got]
        batch.close()
        dev.close()
        runs.append(rows)
    assert runs[0] == runs[1]
    oracles = [orc.tracker(640, 480, TUM_CAM) for _ in range(B)]
    for k in range(n):
        for i in range(B):
            want = oracles[i].handle_frame(to_gray(frames[k, i], "rgb"))
            assert runs[1][k * B + i][:8] == (want.state, want.quality, want.keyframe, want.n_corners, want.matches, want.attempts,
                                              want.inliers, want.outliers), (k, i)
    for o in oracles:
        o.close()


def test_farm_on_colour_device_frames(trk, orc, synth):
    """a farm fed colour frames resident in HBM equals the same farm fed their gray; colour with the host input is refused"""
    import torch
    trk.configure()
    G, Bg, n = 2, 2, 5
    N = G * Bg
    xis = [XI * (1.0 + 0.1 * i) * (1 if i % 2 == 0 else -1) for i in range(N)]
    col = np.stack([np.stack([colourise(synth.render(trajectory_pose(orc, k, xis[i]), TUM_CAM, 640, 480, seed=20260001 + i, frame_id=k),
                                        55 * k + i, 4) for i in range(N)]) for k in range(n)])
    gray = to_gray(col, "bgra")
    results = []
    for fmt, data in (("bgra", col), ("gray", gray)):
        d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        torch.cuda.synchronize()
        fb = data[0, 0].nbytes
        ptrs = np.array([[d.data_ptr() + (k * N + i) * fb for i in range(N)] for k in range(n)], np.uint64)
        farm = trk.TrackerFarm(0, G, Bg, 640, 480, TUM_CAM)
        farm.set_color(fmt)
        out = farm.run(ptrs)
        results.append([(o.state, o.quality, o.keyframe, o.n_corners, o.matches, o.attempts, o.inliers, o.outliers, tuple(o.pose[:])) for o in out])
        farm.close()
        del d
    assert results[0] == results[1]
    assert all(r[1] == 0 and r[4] >= 100 for r in results[0][N:])   # tracked
    farm = trk.TrackerFarm(0, 1, 1, 640, 480, TUM_CAM)
    try:
        farm.set_color("rgb")
        farm.set_host_input(True)
        host = np.zeros((1, 1), np.uint64)
        with pytest.raises(RuntimeError, match="colour"):
            farm.run(host)
    finally:
        farm.close()


def test_track_sequence_reads_p6_frames(orc, synth, tmp_path):
    """track_sequence --list with P6 files prints the records it prints for P5 files of the numpy-converted frames"""
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    n = 5
    outs = []
    for kind in ("P6", "P5"):
        lst = tmp_path / ("%s.txt" % kind)
        with open(lst, "w") as fh:
            for k in range(n):
                rgb = colourise(synth.render(trajectory_pose(orc, k), TUM_CAM, 640, 480, frame_id=k), 900 + k)
                p = tmp_path / ("f%03d.%s" % (k, "ppm" if kind == "P6" else "pgm"))
                with open(p, "wb") as out:
                    out.write(b"%s\n640 480\n255\n" % kind.encode())
                    out.write(rgb.tobytes() if kind == "P6" else to_gray(rgb, "rgb").tobytes())
                fh.write(str(p) + "\n")
        r = subprocess.run([exe, "--list", str(lst)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        rows = r.stdout.strip().splitlines()
        assert len(rows) == n
        outs.append(rows)
    assert outs[0] == outs[1]
    assert int(outs[0][-1].split()[3]) >= 100    # matches: tracked


def test_gray_steps_never_launch_the_conversion(trk, orc, synth):
    """the gray path is untouched: the kernel-timing names of gray steps never include to_gray, colour steps do"""
    trk.configure()
    dev = trk.HostDevice(0)
    lib = importlib.import_module("slam-sdvl_amd").load_library()
    ctx = dev.ctx_handle()
    assert lib.sdvl_ctx_timing_enable(C.c_void_p(ctx), 1) == 0
    batch = trk.TrackerBatch(dev, 1, 640, 480, TUM_CAM)

    def names():
        nm = ((C.c_char * 32) * 64)()
        ms = (C.c_double * 64)()
        la = (C.c_int64 * 64)()
        cnt = C.c_int()
        assert lib.sdvl_ctx_timing_get(C.c_void_p(ctx), 64, nm, ms, la, C.byref(cnt)) == 0
        return {nm[i].value.decode(): la[i] for i in range(cnt.value)}

    for k in range(3):
        batch.step_host([synth.render(trajectory_pose(orc, k), TUM_CAM, 640, 480, frame_id=k)])
    gray_names = names()
    assert "frames_upload" in gray_names or len(gray_names) > 3
    assert not any(n.startswith("to_gray") for n in gray_names), gray_names
    batch.set_color("rgb")
    batch.step_host([colourise(synth.render(trajectory_pose(orc, 3), TUM_CAM, 640, 480, frame_id=3), 3)])
    assert names().get("to_gray", 0) >= 1
    batch.close()
    dev.close()
