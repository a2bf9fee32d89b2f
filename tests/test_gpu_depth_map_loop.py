"""Depth cameras inside the reference's mapper in the closed loop (TrackerBatch.set_depth_mapping): `shelf`, two trackers, a deliberately
wrong plane, 40 device-rendered frames of 640 x 480 with the renderer's registered depth, beside the same batch with the switch off (the
monocular mapper behind a depth bootstrap: the yardstick).

1. switch on: every frame tracked, every keyframe after the bootstrap fixes points from depth, candidate updates are measured
2. map quality: scene_cases.assert_geometry holds, and the share of points within 5 cm of a true surface is no lower than with the switch off
3. the points fixed from depth carry the renderer's depth: see test_fixed_points_carry_the_renderers_depth for the frame they are held in
4. the worst camera-centre error is at most twice that with the switch off (a guard)
5. inert: a batch with the switch on whose frames after the bootstrap come without depth images equals the batch with the switch off exactly
6. 16-bit depth against a float image of the same rounded values; the refusals of the switch; host/track_sequence --depth-mapping

Measured on an MI355X: see DESIGN.md section 7 (the figures the tests print with -s)."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import scene_cases as sc
from oraclelib import TUM_CAM, quat_to_R, trajectory_pose

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, W, H = 2, sc.N_FRAMES, sc.W, sc.H
FB = W * H
WRONG_PLANE = (0, 0, 1, 5.0)
NOISE = dict(noise_abs=0.002, noise_quad=0.001)          # explicit: no test rests on the defaults
INT_FIELDS = ("state", "quality", "matches", "attempts", "inliers", "outliers", "n_corners", "align_meas", "keyframe", "relocalized",
              "align_features", "align_iters", "search_requests", "lk_iters", "host_path")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def trk():
    importlib.import_module("slam-sdvl_amd")
    return importlib.import_module("slam-sdvl_amd.tracker")


def poses_of(orc, i):
    return [trajectory_pose(orc, k, sc.tracker_twist(i)) for k in range(N)]


class Rendered:
    """N frames of B trackers on `shelf` and their depth images in HBM, with host copies on demand"""

    def __init__(self, ctx, orc):
        ss = sc.scene_synth()
        scenes = [ss.scene(T, preset="shelf", seed=sc.SEED + i, frame_id=k) for i in range(B) for k, T in enumerate(poses_of(orc, i))]
        self.ctx = ctx
        self.buf = ctx.device_malloc(B * N * FB)
        self.dd = ctx.device_malloc(4 * B * N * FB)
        ctx.synth_render_scene(scenes, W, H, self.buf, dev_depth=self.dd)
        ctx.synchronize()

    def imgs(self, k):
        return [self.buf + (i * N + k) * FB for i in range(B)]

    def depths(self, k):
        return [self.dd + 4 * (i * N + k) * FB for i in range(B)]

    def host_depth(self, i, k):
        return self.ctx.device_download(self.dd + 4 * (i * N + k) * FB, 4 * FB).view(np.float32).reshape(H, W)

    def host_img(self, i, k):
        return self.ctx.device_download(self.buf + (i * N + k) * FB, FB).reshape(H, W)

    def close(self):
        self.ctx.device_free(self.buf)
        self.ctx.device_free(self.dd)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shelf(ctx, orc):
    r = Rendered(ctx, orc)
    yield r
    r.close()


def make_batch(trk, n=B, mapper=True):
    trk.configure()
    trk.set_mapper(mapper)
    try:
        dev = trk.HostDevice(0)
        return dev, trk.TrackerBatch(dev, n, W, H, TUM_CAM, plane4=WRONG_PLANE, host_threads=1)
    finally:
        trk.set_mapper(False)


def raw(stats, i):
    return bytes(memoryview(stats[i]))


def centre(T):
    return -quat_to_R(np.asarray(T[:4])).T @ np.asarray(T[4:7])


_runs = {}


def mapped_run(trk, shelf, on, depth_after_bootstrap=True):
    """the mapper batch over the N frames, once per process -> dict(raw, states, poses, map_stats per step, points, seeded, stats)"""
    key = (on, depth_after_bootstrap)
    if key not in _runs:
        dev, batch = make_batch(trk)
        try:
            batch.set_depth()
            if on:
                batch.set_depth_mapping(**NOISE)
            out = dict(raw=[], states=[], poses=[], map_stats=[])
            for k in range(N):
                with_depth = k == 0 or depth_after_bootstrap
                st = batch.step_device(shelf.imgs(k), shelf.depths(k)) if with_depth else batch.step_device(shelf.imgs(k))
                out["raw"].append([raw(st, i) for i in range(B)])
                out["states"].append([(st[i].state, st[i].quality, st[i].keyframe) for i in range(B)])
                out["poses"].append([np.array(st[i].pose[:]) for i in range(B)])
                out["map_stats"].append([batch.depth_map_stats(i) for i in range(B)])
            out["points"] = [batch.map_points(i) for i in range(B)]
            out["seeded"] = [batch.seeded_points(i) for i in range(B)]
            out["stats"] = [batch.depth_stats(i) for i in range(B)]
            _runs[key] = out
        finally:
            batch.close()
            dev.close()
    return _runs[key]


def test_switch_on_tracks_and_fixes_points_on_every_keyframe(trk, shelf):
    r = mapped_run(trk, shelf, True)
    for i in range(B):
        assert r["states"][0][i] == (0, 0, 1), r["states"][0][i]
        kfs = []
        for k in range(1, N):
            assert r["states"][k][i][:2] == (2, 0), (i, k, r["states"][k][i])
            if r["states"][k][i][2]:
                kfs.append(k)
        assert kfs, "the run makes keyframes after the bootstrap"
        for k in kfs:      # the mapper works on a keyframe in the step that made it
            a, b = r["map_stats"][k - 1][i], r["map_stats"][k][i]
            fixed = (b["fixed_matched"] + b["fixed_unmatched"]) - (a["fixed_matched"] + a["fixed_unmatched"])
            assert b["keyframes"] == a["keyframes"] + 1 and fixed > 0, (i, k, a, b)
        last = r["map_stats"][-1][i]
        assert last["measured"] > 0 and last["keyframes"] == len(kfs), (i, last, kfs)
        assert r["stats"][i]["keyframes"] == 1                # the driver seeds the bootstrap keyframe alone, as before
        print("tracker %d: keyframes at %s; %s" % (i, kfs, last))


def test_map_quality_beside_the_monocular_mapper(trk, orc, shelf):
    on, off = mapped_run(trk, shelf, True), mapped_run(trk, shelf, False)
    scene = sc.shelf_scene(orc)
    for i in range(B):
        rep_on, rep_off = sc.geometry_report(scene, on["points"][i]), sc.geometry_report(scene, off["points"][i])
        print("tracker %d: switch on %d points %s" % (i, len(on["points"][i]), rep_on))
        print("tracker %d: switch off %d points %s" % (i, len(off["points"][i]), rep_off))
        sc.assert_geometry(rep_on)
        assert rep_on["share"] >= rep_off["share"], (i, rep_on["share"], rep_off["share"])
        assert all(v == 0 for v in off["map_stats"][-1][i].values()), off["map_stats"][-1][i]


def test_fixed_points_carry_the_renderers_depth(trk, orc, shelf):
    """A point fixed from depth on keyframe k stands at its corner's bearing times the measured range, in the keyframe's camera frame,
    and is placed in the world with the keyframe's ESTIMATED pose.  What the renderer's depth determines is the point in the camera
    frame; its world position carries the keyframe's pose error besides, which is the trajectory error of the guard below and no
    property of the depth.  So the point is taken back into the keyframe's camera frame with the pose the tracker reported for that
    frame and out into the world with the renderer's TRUE pose of the frame: there it lies on a true surface to 1e-6 m, the bound
    test_gpu_depth_loop.py holds its bootstrap seeds to.  The distance of the points as the map holds them is printed beside it."""
    r = mapped_run(trk, shelf, True)
    scene = sc.shelf_scene(orc)
    for i in range(B):
        truth = poses_of(orc, i)
        pts = r["seeded"][i]
        later = pts[pts[:, 3] > 0]
        assert len(later) >= 20 and len(set(later[:, 3])) >= 1, len(later)
        worst, worst_world = 0.0, 0.0
        for p in later:
            k = int(p[3])
            assert r["states"][k][i][2] == 1, (i, k)              # its keyframe is a keyframe of the run
            T_est, T_true = r["poses"][k][i], truth[k]
            p_cam = quat_to_R(T_est[:4]) @ p[:3] + T_est[4:7]
            p_true = quat_to_R(np.asarray(T_true[:4])).T @ (p_cam - np.asarray(T_true[4:7]))
            worst = max(worst, sc.distance_to_surfaces(scene, p_true)[0])
            worst_world = max(worst_world, sc.distance_to_surfaces(scene, p[:3])[0])
        print("tracker %d: %d points fixed from depth on %d keyframes: worst distance to a true surface %.3g m in their keyframe's frame, %.3g m as the map "
              "holds them (with the keyframes' pose error)" % (i, len(later), len(set(later[:, 3])), worst, worst_world))
        assert worst <= 1e-6, (i, worst)


def test_trajectory_beside_the_monocular_mapper(trk, orc, shelf):
    on, off = mapped_run(trk, shelf, True), mapped_run(trk, shelf, False)
    worst = {"on": 0.0, "off": 0.0}
    for i in range(B):
        truth = poses_of(orc, i)
        e_on = max(float(np.linalg.norm(centre(on["poses"][k][i]) - centre(truth[k]))) for k in range(N))
        e_off = max(float(np.linalg.norm(centre(off["poses"][k][i]) - centre(truth[k]))) for k in range(N))
        print("tracker %d: worst camera-centre error over %d frames: depth mapping %.4g m, monocular mapper %.4g m" % (i, N, e_on, e_off))
        worst["on"], worst["off"] = max(worst["on"], e_on), max(worst["off"], e_off)
    assert worst["on"] <= 2.0 * worst["off"], worst


def test_inert_without_depth_images(trk, shelf):
    """the switch on, but no depth image behind the bootstrap: FrameStats and the map's points equal the switch-off batch's, exactly"""
    on, off = mapped_run(trk, shelf, True, depth_after_bootstrap=False), mapped_run(trk, shelf, False, depth_after_bootstrap=False)
    assert on["raw"] == off["raw"]
    for i in range(B):
        assert on["points"][i].tobytes() == off["points"][i].tobytes() and len(on["points"][i]) > 0
        assert on["seeded"][i].tobytes() == off["seeded"][i].tobytes()
        assert all(v == 0 for v in on["map_stats"][-1][i].values()), on["map_stats"][-1][i]
    assert any(s[2] for row in on["states"][1:] for s in row), "the run makes keyframes after the bootstrap"


def test_u16_depth(trk, shelf):
    """16-bit depth made as round(z * 5000) against a float image of the same rounded values (see test_gpu_depth_loop.test_u16_depth for
    why the two are not the same numbers to the last bit): equal counters of FrameStats, equal decisions and equal depth-mapping counters
    over 16 frames, from pageable host images"""
    n, scale = 16, 1.0 / 5000
    u16 = [[np.round(shelf.host_depth(i, k).astype(np.float64) * 5000).astype(np.uint16) for i in range(B)] for k in range(n)]
    imgs = [[shelf.host_img(i, k) for i in range(B)] for k in range(n)]
    runs = {}
    for fmt in ("u16", "f32"):
        dev, batch = make_batch(trk)
        try:
            batch.set_depth(format=fmt, scale=scale)
            batch.set_depth_mapping(**NOISE)
            per = []
            for k in range(n):
                d = u16[k] if fmt == "u16" else [(v.astype(np.float64) * scale).astype(np.float32) for v in u16[k]]
                st = batch.step_host(imgs[k], depths=d)
                per.append([[getattr(st[i], f) for f in INT_FIELDS] for i in range(B)])
            runs[fmt] = (per, [batch.depth_map_stats(i) for i in range(B)], [batch.depth_stats(i) for i in range(B)])
        finally:
            batch.close()
            dev.close()
    assert runs["u16"] == runs["f32"]
    for i in range(B):
        assert runs["u16"][1][i]["measured"] > 0 and all(row[i][:2] == [2, 0] for row in runs["u16"][0][1:])
    print("u16 == f32 over %d frames: %s" % (n, runs["u16"][1]))


def test_refusals(trk):
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "depth_map_check")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)     # the mapper thread can only be started from C++
    assert r.returncode == 0 and "0 failed" in r.stdout, r.stdout + r.stderr
    dev, batch = make_batch(trk, n=1)
    try:
        with pytest.raises(RuntimeError, match="depth seeding"):
            batch.set_depth_mapping()
        batch.set_depth()
        with pytest.raises(RuntimeError, match="negative"):
            batch.set_depth_mapping(noise_abs=-1.0)
        trk.set_device_filter(False)
        try:
            with pytest.raises(RuntimeError, match="host depth filter"):
                batch.set_depth_mapping()
        finally:
            trk.set_device_filter(True)
        batch.set_depth_mapping(**NOISE)
        batch.set_depth_mapping(on=False)
    finally:
        batch.close()
        dev.close()
    dev, batch = make_batch(trk, n=1, mapper=False)
    try:
        batch.set_depth()
        with pytest.raises(RuntimeError, match="mapper"):
            batch.set_depth_mapping()
        with pytest.raises(RuntimeError):
            batch.depth_map_stats(0)
    finally:
        batch.close()
        dev.close()


def test_track_sequence_depth_mapping():
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    n = 16
    r = subprocess.run([exe, "--synthetic", str(n), "--scene", "shelf", "--depth", "--depth-mapping", "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [l.split() for l in lines[:-1]]
    assert len(rows) == n and all([int(v) for v in row[1:3]] == [2, 0] for row in rows[1:]), rows
    out = json.loads(lines[-1])
    assert out["tracked"] == n - 1 and out["mapper"] is True
    dm = out["depth_mapping"]
    assert set(dm) == {"measured", "hole", "few", "edge", "outside", "keyframes", "fixed_matched", "fixed_unmatched", "linked"}, dm
    assert "depth mapping: %d measured updates" % dm["measured"] in r.stderr, r.stderr
    print(dm)
    # valid beside --depth only
    assert subprocess.run([exe, "--synthetic", "2", "--scene", "shelf", "--depth-mapping"], capture_output=True, text=True, timeout=120).returncode == 2
