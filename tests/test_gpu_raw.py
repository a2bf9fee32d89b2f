"""Raw camera formats on the MI355X (enum sdvl_raw_format: Bayer mosaics, YUYV / UYVY, 16-bit gray): bayer_gray_kernel and
wide_gray_kernel bit for bit against the numpy restatement (tests/raw_restatement.py, the specification), standalone
(sdvl_convert_gray) and fused into the frames' upload ahead of the undistortion (sdvl_frames_upload_color); closed-loop tracking of raw
frames, in a TrackerBatch and in a TrackerFarm (resident, host-fed with and without the input ring), against the same run fed the
restated gray: both see the same gray bytes, so every record is equal without a tolerance."""
import ctypes as C
import importlib

import numpy as np
import pytest

import raw_restatement as raw
from oraclelib import TUM_CAM, TUM_DIST, XI, trajectory_pose
from test_color_cpu import to_gray

pytestmark = pytest.mark.gpu
FORMATS = list(raw.RAW_FORMATS)
CONVERT_ARGS = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
# (width, height): below one 16-pixel unit, both borders in one lane (16), a unit and a remainder (18, 34), two units, the bench's size,
# and an odd size that takes the byte path
SIZES = [(2, 2), (3, 3), (16, 4), (18, 5), (32, 6), (34, 5), (640, 480), (641, 479)]


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


def code(fmt):
    return raw.RAW_FORMATS[fmt][0]


def bpp(fmt):
    return raw.RAW_FORMATS[fmt][1]


def sizes_of(fmt):
    if fmt in raw.BAYER:
        return SIZES
    if fmt in raw.GRAY_BITS:
        return SIZES + [(8, 4)]                                      # (a row of exactly 16 bytes)
    return sorted(set((w + (w & 1), h) for w, h in SIZES + [(8, 4)]))  # YUV 4:2:2: even widths


def natural(view, fmt):
    """the bytes [h, w, bpp] of an image as the array the restatement takes"""
    if fmt in raw.BAYER:
        return view[..., 0]
    if fmt in raw.GRAY_BITS:
        return view[..., 0].astype(np.uint16) | (view[..., 1].astype(np.uint16) << 8)
    return view


def colourise(gray, seed):
    rng = np.random.default_rng(seed)
    off = rng.integers(-40, 41, (3,))
    noise = rng.integers(-6, 7, gray.shape + (3,))
    return np.clip(gray[..., None].astype(np.int32) + off + noise, 0, 255).astype(np.uint8)


def raw_frame(gray, fmt, seed):
    """a raw camera frame of `fmt` that shows the gray image: (the frame in its natural array, its restated gray)"""
    rng = np.random.default_rng(seed)
    if fmt in raw.BAYER:
        f = raw.bayer_sample(colourise(gray, seed), fmt)
    elif fmt in raw.GRAY_BITS:
        s = raw.GRAY_BITS[fmt] - 8
        f = (gray.astype(np.uint16) << s) | rng.integers(0, 1 << s, gray.shape).astype(np.uint16)
    else:
        chroma = rng.integers(0, 256, gray.shape, dtype=np.uint8)
        f = np.stack([gray, chroma] if fmt == "yuyv" else [chroma, gray], -1)
    return f, raw.raw_to_gray(f, fmt)


def convert(ctx, srcs, src_stride, on_device, w, h, fmt_code, dst_stride=None, expect=0):
    """sdvl_convert_gray over raw addresses -> numpy gray images [n, h, w] (or the return code if it is not `expect`)"""
    n = len(srcs)
    ds = dst_stride or w
    buf = ctx.device_malloc(max(1, n * ds * h))
    try:
        dst = (C.c_void_p * n)(*[buf + i * ds * h for i in range(n)])
        src = (C.c_void_p * n)(*[int(p) for p in srcs])
        ctx.lib.sdvl_convert_gray.argtypes = CONVERT_ARGS
        rc = ctx.lib.sdvl_convert_gray(ctx.h, n, src, src_stride, int(on_device), w, h, fmt_code, dst, ds)
        if expect != 0:
            return rc
        ctx._check(rc)
        out = ctx.device_download(buf, n * ds * h).reshape(n, h, ds)[:, :, :w]
    finally:
        ctx.device_free(buf)
    return out


def _host_images(n, w, h, ch, pitch, offset, seed):
    """n images of ch bytes per pixel with row pitch `pitch` bytes, starting `offset` bytes into one buffer each -> (buffers, views)"""
    rng = np.random.default_rng(seed)
    bufs, views = [], []
    for i in range(n):
        b = rng.integers(0, 256, offset + pitch * h, dtype=np.uint8)
        bufs.append(b)
        views.append(np.lib.stride_tricks.as_strided(b[offset:], (h, w, ch), (pitch, ch, 1)))
    return bufs, views


@pytest.mark.parametrize("fmt", FORMATS)
def test_convert_gray_layouts(ctx, fmt):
    """every size x dense and padded pitches (not multiples of 16) x sources 1-15 bytes off alignment, from pageable, pinned and device
    memory (the last with a padded destination), n = 3 and n = 1: equal to the restatement everywhere"""
    import torch
    lib = ctx.lib
    ch = bpp(fmt)
    for w, h in sizes_of(fmt):
        for pitch, offset in ((w * ch, 0), (w * ch + 7, 0), (w * ch, 5), (w * ch + 33, 13), (w * ch + 16, 0)):
            n = 3
            bufs, views = _host_images(n, w, h, ch, pitch, offset, seed=w + pitch + offset + code(fmt))
            want = [raw.raw_to_gray(natural(v, fmt), fmt) for v in views]
            tag = (fmt, w, h, pitch, offset)
            got = convert(ctx, [b.ctypes.data + offset for b in bufs], pitch, False, w, h, code(fmt))
            for i in range(n):
                assert np.array_equal(got[i], want[i]), ("pageable",) + tag + (i,)
            got = convert(ctx, [bufs[1].ctypes.data + offset], pitch, False, w, h, code(fmt))
            assert np.array_equal(got[0], want[1]), ("pageable, n = 1",) + tag
            pinned = C.c_void_p()
            total = len(bufs[0])
            ctx._check(lib.sdvl_host_alloc_pinned(ctx.h, C.c_int64(total * n), C.byref(pinned)))
            try:
                for i in range(n):
                    C.memmove(pinned.value + i * total, bufs[i].ctypes.data, total)
                got = convert(ctx, [pinned.value + i * total + offset for i in range(n)], pitch, False, w, h, code(fmt))
                ctx.synchronize()
            finally:
                ctx._check(lib.sdvl_host_free_pinned(ctx.h, pinned))
            for i in range(n):
                assert np.array_equal(got[i], want[i]), ("pinned",) + tag + (i,)
            dev = torch.from_numpy(np.concatenate(bufs)).cuda()
            torch.cuda.synchronize()
            got = convert(ctx, [dev.data_ptr() + i * total + offset for i in range(n)], pitch, True, w, h, code(fmt), dst_stride=w + 3)
            for i in range(n):
                assert np.array_equal(got[i], want[i]), ("device, padded destination",) + tag + (i,)
            if (w & 15) == 0:   # a destination pitch that keeps the rows 16-byte aligned: the row-by-row vector form
                got = convert(ctx, [dev.data_ptr() + i * total + offset for i in range(n)], pitch, True, w, h, code(fmt), dst_stride=w + 16)
                for i in range(n):
                    assert np.array_equal(got[i], want[i]), ("device, aligned padded destination",) + tag + (i,)
            del dev


@pytest.mark.parametrize("fmt", raw.BAYER)
def test_bayer_contents(ctx, fmt):
    """a flat colour (its luma everywhere, borders included), all 255 (no overflow), 0 / 255 checkerboards at the period of the mosaic"""
    for w, h in ((2, 2), (16, 4), (34, 5), (640, 480), (641, 479)):
        rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        flat = np.broadcast_to(np.array((200, 17, 91), np.uint8), (h, w, 3))
        r0, c0 = raw.RED_SITE[fmt]
        cases = {"flat": raw.bayer_sample(flat, fmt), "255": np.full((h, w), 255, np.uint8),
                 "checker": (255 * ((rr + cc) & 1)).astype(np.uint8), "checker'": (255 * ((rr + cc + 1) & 1)).astype(np.uint8),
                 "red sites": (255 * (((rr & 1) == r0) & ((cc & 1) == c0))).astype(np.uint8),
                 "rows": (255 * (rr & 1)).astype(np.uint8), "columns": (255 * (cc & 1)).astype(np.uint8)}
        names = list(cases)
        got = ctx.convert_gray([np.ascontiguousarray(cases[k]) for k in names], code(fmt))
        for k, g in zip(names, got):
            assert np.array_equal(g, raw.bayer_to_gray(cases[k], fmt)), (fmt, w, h, k)
        assert np.array_equal(got[0], to_gray(flat, "rgb")), (fmt, w, h)
        assert np.all(got[1] == 255)


def test_gray16_is_exhaustive(ctx):
    """one 256 x 256 image holds every uint16 once"""
    v = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    for fmt in raw.GRAY_BITS:
        got = ctx.convert_gray([v], code(fmt))[0]
        assert np.array_equal(got, raw.gray16_to_gray(v, fmt)), fmt
    b = np.arange(256, dtype=np.uint16).reshape(16, 16)
    assert np.array_equal(ctx.convert_gray([b << 8], code("gray16"))[0], b.astype(np.uint8))


@pytest.mark.parametrize("fmt", ["bayer_gbrg", "uyvy", "gray10"])
def test_convert_gray_256_frames(ctx, fmt):
    """the bench's group size from HBM: 256 jobs in one launch over four distinct 640 x 480 images"""
    import torch
    w, h, ch = 640, 480, bpp(fmt)
    bufs, views = _host_images(4, w, h, ch, w * ch, 0, seed=31 + code(fmt))
    want = [raw.raw_to_gray(natural(v, fmt), fmt) for v in views]
    dev = torch.from_numpy(np.concatenate(bufs)).cuda()
    torch.cuda.synchronize()
    got = convert(ctx, [dev.data_ptr() + (i % 4) * w * h * ch for i in range(256)], w * ch, True, w, h, code(fmt))
    for i in range(256):
        assert np.array_equal(got[i], want[i % 4]), (fmt, i)


def test_refusals_name_their_reason(ctx):
    lib = ctx.lib
    img = np.zeros((8, 32), np.uint8)
    src = [img.ctypes.data]

    def refused(w, h, stride, fmt_code, word):
        assert convert(ctx, src, stride, False, w, h, fmt_code, expect=-1) == -1, (w, h, stride, fmt_code)
        msg = lib.sdvl_last_error(ctx.h)
        assert word in msg, (msg, word)
        return msg

    assert b"stride" not in refused(7, 4, 16, code("yuyv"), b"width")       # an odd width
    refused(5, 4, 10, code("uyvy"), b"width")
    refused(1, 4, 8, code("bayer_rggb"), b"size")                            # Bayer 1 x N and N x 1
    refused(8, 1, 8, code("bayer_bggr"), b"size")
    refused(8, 4, 7, code("bayer_grbg"), b"stride")                          # below width x bytes per pixel
    refused(8, 4, 15, code("yuyv"), b"stride")
    refused(8, 4, 15, code("gray12"), b"stride")
    for bad in (9, 5, 15, 25):
        refused(8, 4, 32, bad, b"format")
    # the smallest images that are accepted
    assert convert(ctx, src, 2, False, 2, 2, code("bayer_rggb")).shape == (1, 2, 2)
    assert convert(ctx, src, 4, False, 2, 1, code("yuyv")).shape == (1, 1, 2)
    assert convert(ctx, src, 2, False, 1, 1, code("gray16")).shape == (1, 1, 1)


def test_frames_upload_raw_through_the_lens(pkg, orc, synth):
    """level 0 = undistort(gray(raw)) bit for bit with a lens, the restated gray itself without one"""
    ctx = pkg.Context(0)
    try:
        w, h = 640, 480
        cam = pkg.Camera(w, h, *TUM_CAM)
        base = [synth.render(trajectory_pose(orc, k), TUM_CAM, w, h, frame_id=k, dist=TUM_DIST) for k in range(2)]
        for fmt in ("bayer_grbg", "uyvy", "gray12"):
            frames = [raw_frame(b, fmt, 400 + k) for k, b in enumerate(base)]
            raws, grays = [f[0] for f in frames], [f[1] for f in frames]
            fc = [ctx.frame(width=w, height=h) for _ in raws]
            ctx.frames_upload_color(fc, raws, code(fmt))
            for i in range(len(raws)):
                assert np.array_equal(fc[i].level(0), grays[i]), (fmt, i)
            ctx.frames_upload_color(fc, raws, code(fmt), cam, TUM_DIST)
            ctx.pyramid_build(fc)
            for i in range(len(raws)):
                assert np.array_equal(fc[i].level(0), orc.undistort(grays[i], TUM_CAM, TUM_DIST)), (fmt, i)
            for f in fc:
                f.close()
    finally:
        ctx.close()


def _records(stats):
    return [tuple(tuple(getattr(s, n)[:]) if n == "pose" else getattr(s, n) for n, _ in type(s)._fields_) for s in stats]


def _sequences(orc, synth, fmt, n_seq, n_frames, scale=0.15):
    """[frame][sequence] -> (raw frame, restated gray) of n_seq cameras moving differently over the synthetic plane"""
    xis = [XI * (1.0 + scale * i) * (1 if i % 2 == 0 else -1) for i in range(n_seq)]
    return [[raw_frame(synth.render(trajectory_pose(orc, k, xis[i]), TUM_CAM, 640, 480, seed=20260001 + i, frame_id=k), fmt, 1000 * k + i)
             for i in range(n_seq)] for k in range(n_frames)]


@pytest.mark.parametrize("fmt,how", [("bayer_rggb", "host"), ("yuyv", "host"), ("gray10", "device")])
def test_raw_frames_closed_loop(trk, orc, synth, fmt, how):
    """two trackers, eight frames: a batch fed raw frames gives, field for field and bit for bit, the records of a batch fed their
    restated gray; "device": step_device with the look-ahead (set_next_device) on raw frames in HBM"""
    import torch
    trk.configure()
    B, n = 2, 8
    seq = _sequences(orc, synth, fmt, B, n)
    runs = []
    for feed in (fmt, "gray"):
        data = np.stack([np.stack([seq[k][i][0 if feed == fmt else 1] for i in range(B)]) for k in range(n)])
        dev = trk.HostDevice(0)
        batch = trk.TrackerBatch(dev, B, 640, 480, TUM_CAM)
        batch.set_color(feed)
        rows = []
        if how == "host":
            for k in range(n):
                rows += _records(batch.step_host([data[k, i] for i in range(B)]))
        else:
            d = torch.from_numpy(data.view(np.uint8)).cuda()
            torch.cuda.synchronize()
            fb = data[0, 0].nbytes
            ptr = lambda k, i: d.data_ptr() + (k * B + i) * fb
            for k in range(n):
                if 1 <= k < n - 1:
                    batch.set_next_device([ptr(k + 1, i) for i in range(B)])
                rows += _records(batch.step_device([ptr(k, i) for i in range(B)]))
            del d
        batch.close()
        dev.close()
        runs.append(rows)
    assert runs[0] == runs[1]
    names = [n_ for n_, _ in trk.FrameStats._fields_]
    q, m = names.index("quality"), names.index("matches")
    assert all(r[q] == 0 and r[m] >= 100 for r in runs[0][B:]), fmt    # tracked


def test_farm_on_bayer_frames(trk, orc, synth):
    """2 groups x 2 sequences x 6 steps on BGGR mosaics, resident in HBM, host-fed through the input ring and host-fed without it: each
    equals the same farm on the restated gray; formats of more than one byte per pixel stay refused on the host input"""
    import torch
    trk.configure()
    G, Bg, n = 2, 2, 6
    N = G * Bg
    fb = 640 * 480
    seq = _sequences(orc, synth, "bayer_bggr", N, n, scale=0.1)
    pinned = torch.empty(n * N * fb, dtype=torch.uint8, pin_memory=True)
    idx = np.arange(n, dtype=np.uint64)[:, None] * N + np.arange(N, dtype=np.uint64)[None, :]
    results = {}
    for feed in ("bayer_bggr", "gray"):
        data = np.stack([np.stack([seq[k][i][0 if feed != "gray" else 1] for i in range(N)]) for k in range(n)])
        for mode in ("resident", "ring", "no-ring"):
            farm = trk.TrackerFarm(0, G, Bg, 640, 480, TUM_CAM)
            farm.set_color(feed)
            if mode == "resident":
                d = torch.from_numpy(data).cuda()
                torch.cuda.synchronize()
                ptrs = (d.data_ptr() + idx * fb).astype(np.uint64)
            else:
                pinned.numpy()[:] = data.reshape(-1)
                ptrs = (pinned.data_ptr() + idx * fb).astype(np.uint64)
                farm.set_host_input(True)
                farm.set_input_ring(mode == "ring")
            results[feed, mode] = _records(farm.run(ptrs, G))
            farm.close()
            d = None
    want = results["gray", "resident"]
    for key, got in results.items():
        assert got == want, key
    names = [n_ for n_, _ in trk.FrameStats._fields_]
    q, m = names.index("quality"), names.index("matches")
    assert all(r[q] == 0 and r[m] >= 100 for r in want[N:])
    for fmt in ("rgb", "yuyv"):
        farm = trk.TrackerFarm(0, 1, 1, 640, 480, TUM_CAM)
        try:
            farm.set_color(fmt)
            farm.set_host_input(True)
            with pytest.raises(RuntimeError, match="colour"):
                farm.run(np.zeros((1, 1), np.uint64))
        finally:
            farm.close()


def test_track_sequence_reads_raw_p5_frames(orc, synth, tmp_path):
    """track_sequence --list --raw-format: P5 files holding mosaics (width W) or YUYV rows (width 2 W) give the records of P5 files of
    their restated gray"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slam-sdvl_amd", "host", "track_sequence")
    n = 5
    base = [synth.render(trajectory_pose(orc, k), TUM_CAM, 640, 480, frame_id=k) for k in range(n)]
    for fmt in ("bayer_gbrg", "yuyv"):
        outs = []
        for kind in (fmt, "gray"):
            lst = tmp_path / ("%s_%s.txt" % (fmt, kind))
            with open(lst, "w") as fh:
                for k in range(n):
                    frame, gray = raw_frame(base[k], fmt, 700 + k)
                    data = frame if kind == fmt else gray
                    p = tmp_path / ("%s_%s_%03d.pgm" % (fmt, kind, k))
                    with open(p, "wb") as out:
                        out.write(b"P5\n%d 480\n255\n" % (data.size // 480))
                        out.write(data.tobytes())
                    fh.write(str(p) + "\n")
            cmd = [exe, "--list", str(lst)] + (["--raw-format", fmt] if kind == fmt else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            rows = r.stdout.strip().splitlines()
            assert len(rows) == n
            outs.append(rows)
        assert outs[0] == outs[1], fmt
        assert int(outs[0][-1].split()[3]) >= 100    # matches: tracked
    # a P5 of the wrong width for the format is refused
    r = subprocess.run([exe, "--list", str(tmp_path / "yuyv_gray.txt"), "--raw-format", "yuyv"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
