"""The scene with depth on the device (sdvl_synth_render_scene) against its host twin, and the trackers on `shelf`: closed loop with the
reference's mapper against the CPU oracle, the map points both sides triangulate (TrackerBatch.map_points against mapper_points())
against each other and against the scene's true surfaces, device-rendered frames, bundle adjustment on a scene that has depth (record
only) and track_sequence --scene."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import scene_cases as sc
from oraclelib import TUM_CAM, TUM_DIST, XI, quat_to_R, trajectory_pose

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4          # tests/test_gpu_tracker.py
# Position gap between a map point of the product and the same row of the oracle: 10 x the worst gap measured in the 40-frame run
# below, the factor for other machines' rounding of FP64 sums; never looser than 1e-3 m, far below the 2 cm of the geometry
POINT_GAP_MEASURED = 9.46e-12   # metres, tracker 1 (tracker 0: 5.72e-12)
POINT_TOL = min(10 * POINT_GAP_MEASURED, 1e-3)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def trk():
    importlib.import_module("slam-sdvl_amd")
    return importlib.import_module("slam-sdvl_amd.tracker")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ss():
    return sc.scene_synth()


def borrowed(sdvl, handle):
    """the package's Context over a sdvl_ctx the host layer owns (never closed here)"""
    c = sdvl.Context.__new__(sdvl.Context)
    c.lib, c.h = sdvl.load_library(), C.c_void_p(handle)
    return c


def device_render(ctx, scenes, w, h, truth=True, frame_bytes=None):
    """-> (raw image buffer of n * frame_bytes bytes, depth bits uint32 [n, h, w] or None, ids [n, h, w] or None)"""
    n, fb = len(scenes), frame_bytes or w * h
    out = ctx.device_malloc(n * fb)
    dd = ctx.device_malloc(4 * n * w * h) if truth else None
    ds = ctx.device_malloc(n * w * h) if truth else None
    try:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        assert hip.hipMemset(out, 0xA5, n * fb) == 0 and hip.hipDeviceSynchronize() == 0
        ctx.synth_render_scene(scenes, w, h, out, frame_bytes=fb, dev_depth=dd, dev_surface=ds)
        img = ctx.device_download(out, n * fb).reshape(n, fb)
        depth = ctx.device_download(dd, 4 * n * w * h).view(np.uint32).reshape(n, h, w) if truth else None
        surf = ctx.device_download(ds, n * w * h).reshape(n, h, w) if truth else None
    finally:
        for p in (out, dd, ds):
            if p:
                ctx.device_free(p)
    return img, depth, surf


def assert_equals_host(ctx, ss, scenes, w, h, truth=True, pad=0):
    fb = w * h + pad
    img, depth, surf = device_render(ctx, scenes, w, h, truth, fb)
    for i, s in enumerate(scenes):
        want, wd, ws = ss.render(s, w, h)
        assert np.array_equal(img[i, :w * h].reshape(h, w), want), i
        assert (img[i, w * h:] == 0xA5).all(), "padding bytes written"
        if truth:
            assert np.array_equal(depth[i], wd.view(np.uint32)), i
            assert np.array_equal(surf[i], ws), i


def varied_scene(ss, orc, k, n_surfaces, **kw):
    """a scene of n_surfaces (0..8) that all show: the shelf's four and four more small boards nearer still"""
    s = ss.scene(trajectory_pose(orc, k), preset="shelf", frame_id=k, **kw)
    extra = [((0, 0, 1, 1.0), (-0.3, 0.3, 1.0), (0.1, 0.08)), ((0, 0, 1, 0.9), (0.2, -0.25, 0.9), (0.07, 0.1)),
             ((0.6, 0, 0.8, 0.88), (0.0, 0.1, 1.1), (0.12, 0.05)), ((0, 0, 1, 0.8), (0.3, 0.2, 0.8), (0.03, 0.03))]
    for j, (plane, origin, half) in enumerate(extra):
        e1 = (0.8, 0, -0.6) if plane[0] else (1, 0, 0)
        sc.set_surface(s, 4 + j, plane, origin, e1=e1, half=half, seed_add=1000 + j)
    s.n_surfaces = n_surfaces
    return s


@pytest.mark.parametrize("w,h", [(70, 9), (64, 4), (1, 1)])
@pytest.mark.parametrize("n_surfaces", [0, 1, 8])
def test_device_equals_host_small(ctx, ss, orc, w, h, n_surfaces):
    s = varied_scene(ss, orc, 3, n_surfaces)
    s.u0, s.v0 = w / 2.0, h / 2.0
    s.fx = s.fy = 0.8 * w                               # a wide view: the small frame still crosses several surfaces
    assert_equals_host(ctx, ss, [s], w, h)


def test_device_equals_host_three_views_in_one_call(ctx, ss, orc):
    scenes = [varied_scene(ss, orc, k, 8, texture=k % 2) for k in (0, 9, 31)]
    _, _, surf = ss.render(scenes[1])
    assert len(np.unique(surf)) == 8                    # every surface of the record shows
    assert_equals_host(ctx, ss, scenes, 640, 480)


@pytest.mark.parametrize("texture", [0, 1])
def test_device_equals_host_through_the_lens(ctx, ss, orc, texture):
    assert_equals_host(ctx, ss, [varied_scene(ss, orc, 5, 4, texture=texture, dist=TUM_DIST)], 160, 120)


def test_device_without_truth_buffers_and_with_padded_frames(ctx, ss, orc):
    scenes = [varied_scene(ss, orc, k, 4) for k in (1, 2)]
    assert_equals_host(ctx, ss, scenes, 70, 9, truth=False)
    assert_equals_host(ctx, ss, scenes, 70, 9, truth=True, pad=37)
    assert_equals_host(ctx, ss, scenes, 70, 9, truth=False, pad=37)


def test_one_surface_scene_on_the_device_equals_the_plane_renderer(ctx, sdvl, ss, orc):
    w, h, n = 640, 480, 3
    views, scenes = [], []
    for k in range(n):
        T, dist = trajectory_pose(orc, 4 * k), (TUM_DIST if k == 2 else None)
        s = ss.scene(T, frame_id=k, texture=k % 2, dist=dist)
        s.n_surfaces = 1
        sc.set_surface(s, 0, (0, 0, 1, 2.0))
        scenes.append(s)
        v = sdvl.SynthView()
        v.fx, v.fy, v.u0, v.v0 = s.fx, s.fy, s.u0, s.v0
        for i in range(9):
            v.R[i] = s.R[i]
        for i in range(3):
            v.t[i] = s.t[i]
        for i in range(5):
            v.dist[i] = s.dist[i]
        v.plane[0], v.plane[1], v.plane[2], v.plane[3] = 0.0, 0.0, 1.0, 2.0
        v.seed, v.frame_id, v.texture = s.seed, s.frame_id, s.texture
        views.append(v)
    buf = ctx.device_malloc(n * w * h)
    try:
        ctx.synth_render(views, w, h, buf)
        plane = ctx.device_download(buf, n * w * h)
    finally:
        ctx.device_free(buf)
    img, _, surf = device_render(ctx, scenes, w, h)
    assert np.array_equal(img.reshape(-1), plane) and (surf == 0).all()
    assert len(np.unique(plane)) > 100


def test_refusals(ctx, sdvl, ss, orc):
    lib = ctx.lib
    s = varied_scene(ss, orc, 0, 4)
    arr = (sdvl.SynthScene * 1)(s)
    buf = ctx.device_malloc(64 * 4)

    def refused(*args):
        rc = lib.sdvl_synth_render_scene(ctx.h, *args)
        msg = lib.sdvl_last_error(ctx.h).decode()
        assert rc == -1 and msg, (args, rc, msg)
        return msg

    try:
        msgs = [refused(1, None, 64, 4, buf, 256, None, None), refused(1, arr, 64, 4, None, 256, None, None),
                refused(1, arr, 0, 4, buf, 256, None, None), refused(1, arr, 64, -1, buf, 256, None, None),
                refused(1, arr, 64, 4, buf, 255, None, None), refused(-1, arr, 64, 4, buf, 256, None, None),
                refused(sdvl.SYNTH_SCENE_MAX_VIEWS + 1, arr, 64, 4, buf, 256, None, None)]
        arr[0].n_surfaces = 9
        msgs.append(refused(1, arr, 64, 4, buf, 256, None, None))
        assert "frame_bytes" in msgs[4] and "surfaces" in msgs[-1]
        assert lib.sdvl_synth_render_scene(None, 1, arr, 64, 4, buf, 256, None, None) == -1
        assert lib.sdvl_ctx_health(ctx.h) == 0
        arr[0].n_surfaces = 4
        assert lib.sdvl_synth_render_scene(ctx.h, 0, None, 64, 4, None, 0, None, None) == 0     # nothing to do
        assert lib.sdvl_synth_render_scene(ctx.h, 1, arr, 64, 4, buf, 256, None, None) == 0     # and the context still works
        assert lib.sdvl_ctx_health(ctx.h) == 0
    finally:
        ctx.device_free(buf)


# ---- the trackers on `shelf`
def counters(g):
    return (g.state, g.quality, g.keyframe, g.n_corners, g.matches, g.attempts, g.inliers, g.outliers, g.align_meas)


def mapper_batch(trk, B):
    trk.configure()
    trk.set_mapper(True)
    try:
        dev = trk.HostDevice(0)
        return dev, trk.TrackerBatch(dev, B, sc.W, sc.H, TUM_CAM, host_threads=1)
    finally:
        trk.set_mapper(False)


def centre(T):
    return -quat_to_R(np.asarray(T[:4])).T @ np.asarray(T[4:7])


def test_closed_loop_with_the_reference_mapper_on_the_shelf(trk, orc):
    """B = 2 on host-rendered `shelf` frames against two oracle trackers: every FrameStats counter, the poses and the map bookkeeping on
    every frame; at the end the map points, row by row; and the product's own points against the scene's true surfaces.
    The oracle alone meets the geometry conditions on both trajectories (tracker 1: 179 converged points, 97.8 % within 5 cm, per
    surface 91 / 39 / 35 / 10), so both trackers are held to the same ones."""
    B = 2
    runs = [sc.oracle_shelf_run(orc, i) for i in range(B)]
    frames = [sc.shelf_frames(orc, i)[0] for i in range(B)]
    dev, batch = mapper_batch(trk, B)
    try:
        worst = 0.0
        for k in range(sc.N_FRAMES):
            got = batch.step_host([frames[i][k] for i in range(B)])
            for i in range(B):
                assert counters(got[i]) == runs[i]["stats"][k], (k, i, counters(got[i]), runs[i]["stats"][k])
                d = float(np.abs(np.array(got[i].pose[:]) - runs[i]["poses"][k]).max())
                worst = max(worst, d)
                assert d <= POSE_TOL, (k, i, d)
                assert batch.map_stats(i) == runs[i]["map_stats"][k], (k, i)
                if k > 0:
                    assert got[i].quality == 0 and got[i].matches >= sc.MIN_MATCHES, (k, i)
        scene = sc.shelf_scene(orc)
        for i in range(B):
            got, want = batch.map_points(i), runs[i]["points"]
            assert got.shape == want.shape and len(got) > 0, (i, got.shape, want.shape)
            assert np.array_equal(got[:, 3], want[:, 3]), i
            gap = float(np.abs(got[:, :3] - want[:, :3]).max())
            rep = sc.geometry_report(scene, got)
            print("tracker %d: %d map points, worst position gap to the oracle %.3g m, worst pose gap %.3g; %s" % (i, len(got), gap, worst, rep))
            assert gap <= POINT_TOL, (i, gap)
            sc.assert_geometry(rep)
    finally:
        batch.close()
        dev.close()


_host_fed = {}


def host_fed_run(trk, orc, bundle=False):
    """tracker 0 alone (B = 1, mapper) on the host-rendered frames -> per-frame (counters, pose), keyframes, bundle stats; once per process"""
    if bundle not in _host_fed:
        frames = sc.shelf_frames(orc, 0)[0]
        dev, batch = mapper_batch(trk, 1)
        try:
            if bundle:
                batch.set_bundle_adjustment(True)
            per = []
            for im in frames:
                g = batch.step_host([im])[0]
                per.append((counters(g), tuple(g.pose[:])))
            _host_fed[bundle] = dict(per=per, keyframes=batch.keyframe_poses(0), bundle=batch.bundle_stats(0), points=batch.map_points(0))
        finally:
            batch.close()
            dev.close()
    return _host_fed[bundle]


def test_device_rendered_frames_give_the_host_fed_results(trk, sdvl, orc):
    want = host_fed_run(trk, orc)
    _, poses = sc.shelf_frames(orc, 0)
    ss = sc.scene_synth()
    scenes = [ss.scene(T, preset="shelf", seed=sc.SEED, frame_id=k) for k, T in enumerate(poses)]
    fb = sc.W * sc.H
    dev, batch = mapper_batch(trk, 1)
    try:
        ctx, buf = borrowed(sdvl, dev.ctx_handle()), None
        buf = ctx.device_malloc(len(scenes) * fb)
        ctx.synth_render_scene(scenes, sc.W, sc.H, buf)
        per = []
        for k in range(len(scenes)):
            g = batch.step_device([buf + k * fb])[0]
            per.append((counters(g), tuple(g.pose[:])))
        points = batch.map_points(0)
    finally:
        batch.close()
        if buf:
            ctx.device_free(buf)
        dev.close()
    assert per == want["per"]
    assert np.array_equal(points, want["points"])


def test_map_points_on_a_plane_map_batch_raises(trk, orc):
    trk.configure()
    dev = trk.HostDevice(0)
    batch = trk.TrackerBatch(dev, 1, sc.W, sc.H, TUM_CAM)
    try:
        batch.step_host([sc.shelf_frames(orc, 0)[0][0]])
        with pytest.raises(RuntimeError):
            batch.map_points(0)
    finally:
        batch.close()
        dev.close()


def test_bundle_adjustment_on_a_scene_with_depth_is_recorded(trk, orc):
    """record only: keyframe position error against the true trajectory with and without the local bundle adjustment"""
    runs = {"with adjustment": host_fed_run(trk, orc, bundle=True), "without": host_fed_run(trk, orc)}
    for name, r in runs.items():
        ids, kf = r["keyframes"]
        err = [float(np.linalg.norm(centre(kf[q]) - centre(trajectory_pose(orc, int(ids[q]))))) for q in range(len(ids))]
        print("%s: %d keyframes, position error mean %.3g max %.3g m, adjustments %d, skipped %d" %
              (name, len(ids), np.mean(err), np.max(err), r["bundle"]["runs"], r["bundle"]["skipped"]))
    adj = runs["with adjustment"]
    assert adj["bundle"]["runs"] >= 1 and adj["bundle"]["skipped"] == 0
    assert all(c[1] != 2 for c, _ in adj["per"])        # never TRACKING_BAD
    assert runs["without"]["bundle"]["runs"] == 0


def test_track_sequence_renders_the_scene(orc):
    """host/track_sequence --scene shelf, host-rendered and --prerender (device-rendered): the oracle's answers on the host twin's frames,
    by the criteria of test_cpp_example_track_sequence_matches_the_oracle"""
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    n = 12
    ref = orc.tracker(sc.W, sc.H, TUM_CAM)
    wants = [ref.handle_frame(im) for im in sc.shelf_frames(orc, 0)[0][:n]]
    ref.close()
    for extra in ([], ["--prerender"]):
        r = subprocess.run([exe, "--synthetic", str(n), "--scene", "shelf"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        rows = [l.split() for l in r.stdout.strip().splitlines()]
        assert len(rows) == n
        for k, (row, w) in enumerate(zip(rows, wants)):
            assert [int(v) for v in row[:6]] == [k, w.state, w.quality, w.matches, w.attempts, w.inliers], (extra, k)
            assert np.abs(np.array([float(v) for v in row[6:13]]) - np.array(w.pose[:])).max() <= POSE_TOL
        assert "tracked frames/s" in r.stderr
    r = subprocess.run([exe, "--synthetic", "2", "--scene", "nosuch"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "shelf" in r.stderr
