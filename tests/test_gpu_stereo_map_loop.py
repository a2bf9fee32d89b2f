"""Stereo cameras inside the reference's mapper in the closed loop (TrackerBatch.set_stereo_mapping): `shelf`, two trackers, a deliberately
wrong plane, 40 device-rendered pairs of 640 x 480, baseline 0.11 m, beside the same batch with the switch off (the monocular mapper behind
a stereo bootstrap: what the project did before the switch, and the yardstick).  It mirrors tests/test_gpu_depth_map_loop.py.

1. switch on: every frame tracked, every keyframe after the bootstrap is matched and fixes points in its own step, candidate updates are
   measured, and the driver still seeds the bootstrap keyframe alone
2. map quality: scene_cases.assert_geometry holds, and the share of points near a true surface is no lower than with the switch off
3. the points fixed from the pair, taken into their keyframe's camera frame with the reported pose and out with the true one: at least
   95 % within scene_cases.NEAR of a true surface (the cap test_gpu_stereo_loop.py puts on seeds)
4. the worst camera-centre error is at most twice that with the switch off
5. inert: the switch on without right images behind the bootstrap equals the switch-off batch exactly; a batch that is told
   set_stereo_mapping(on=False) equals one that is never told
6. every combination that throws; host/stereo_map_check --device; host/track_sequence --stereo --stereo-mapping

Measured on an MI355X: see DESIGN.md section 7 (the figures the tests print with -s)."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import scene_cases as sc
import stereo_cases as stc
from oraclelib import TUM_CAM, quat_to_R, trajectory_pose

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, W, H = 2, sc.N_FRAMES, sc.W, sc.H
FB = W * H
WRONG_PLANE = (0, 0, 1, 5.0)
BASELINE = stc.BASELINE
SIGMA = 0.3                                              # explicit: no test rests on the default
NOISE = dict(noise_abs=0.002, noise_quad=0.001)          # of the depth-mapping run printed beside it
STAT_NAMES = {"measured", "nomatch", "ambiguous", "edge", "outside", "keyframes", "fixed_matched", "fixed_unmatched", "linked"}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def trk():
    importlib.import_module("slam-sdvl_amd")
    return importlib.import_module("slam-sdvl_amd.tracker")


def poses_of(orc, i):
    return [trajectory_pose(orc, k, sc.tracker_twist(i)) for k in range(N)]


class RenderedPairs:
    """N pairs of B trackers in HBM: frame k of tracker i, its right image and the left view's true depth"""

    def __init__(self, ctx, orc):
        ss = sc.scene_synth()
        lefts, rights = [], []
        for i in range(B):
            for k, T in enumerate(poses_of(orc, i)):
                lefts.append(ss.scene(T, preset="shelf", seed=sc.SEED + i, frame_id=k))
                rights.append(ss.scene(stc.right_pose(T, BASELINE), preset="shelf", seed=sc.SEED + i, frame_id=k))
        self.ctx = ctx
        self.buf = ctx.device_malloc(B * N * FB)
        self.rr = ctx.device_malloc(B * N * FB)
        self.dd = ctx.device_malloc(4 * B * N * FB)
        ctx.synth_render_scene(lefts, W, H, self.buf, dev_depth=self.dd)
        ctx.synth_render_scene(rights, W, H, self.rr)
        ctx.synchronize()

    def imgs(self, k):
        return [self.buf + (i * N + k) * FB for i in range(B)]

    def rights(self, k):
        return [self.rr + (i * N + k) * FB for i in range(B)]

    def depths(self, k):
        return [self.dd + 4 * (i * N + k) * FB for i in range(B)]

    def close(self):
        for p in (self.buf, self.rr, self.dd):
            self.ctx.device_free(p)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shelf(ctx, orc):
    r = RenderedPairs(ctx, orc)
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


def mapped_run(trk, shelf, mode, rights_after_bootstrap=True, n=N):
    """the mapper batch over n frames, once per process.  mode: "on" (stereo mapping), "off" (never told), "told-off"
    (set_stereo_mapping(on=False)), "depth" (depth mapping from the renderer's depth, the figures printed beside)"""
    key = (mode, rights_after_bootstrap, n)
    if key not in _runs:
        dev, batch = make_batch(trk)
        try:
            if mode == "depth":
                batch.set_depth()
                batch.set_depth_mapping(**NOISE)
            else:
                batch.set_stereo(BASELINE)
                if mode == "on":
                    batch.set_stereo_mapping(disparity_sigma=SIGMA)
                elif mode == "told-off":
                    batch.set_stereo_mapping(on=False)
            out = dict(raw=[], states=[], poses=[], map_stats=[])
            for k in range(n):
                if mode == "depth":
                    st = batch.step_device(shelf.imgs(k), shelf.depths(k))
                elif k == 0 or rights_after_bootstrap:
                    st = batch.step_device(shelf.imgs(k), right_ptrs=shelf.rights(k))
                else:
                    st = batch.step_device(shelf.imgs(k))
                out["raw"].append([raw(st, i) for i in range(B)])
                out["states"].append([(st[i].state, st[i].quality, st[i].keyframe) for i in range(B)])
                out["poses"].append([np.array(st[i].pose[:]) for i in range(B)])
                out["map_stats"].append([batch.depth_map_stats(i) if mode == "depth" else batch.stereo_map_stats(i) for i in range(B)])
            out["points"] = [batch.map_points(i) for i in range(B)]
            out["seeded"] = [batch.seeded_points(i) for i in range(B)]
            out["stats"] = [batch.depth_stats(i) if mode == "depth" else batch.stereo_stats(i) for i in range(B)]
            _runs[key] = out
        finally:
            batch.close()
            dev.close()
    return _runs[key]


def test_switch_on_tracks_and_fixes_points_on_every_keyframe(trk, shelf):
    r = mapped_run(trk, shelf, "on")
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
        assert set(last) == STAT_NAMES
        assert last["measured"] > 0 and last["keyframes"] == len(kfs), (i, last, kfs)
        assert r["stats"][i]["keyframes"] == 1                # the driver seeds the bootstrap keyframe alone, as before
        print("tracker %d: keyframes at %s; %s" % (i, kfs, last))


def test_map_quality_beside_the_monocular_mapper(trk, orc, shelf):
    on, off = mapped_run(trk, shelf, "on"), mapped_run(trk, shelf, "off")
    scene = sc.shelf_scene(orc)
    for i in range(B):
        rep_on, rep_off = sc.geometry_report(scene, on["points"][i]), sc.geometry_report(scene, off["points"][i])
        print("tracker %d: switch on %d points %s" % (i, len(on["points"][i]), rep_on))
        print("tracker %d: switch off %d points %s" % (i, len(off["points"][i]), rep_off))
        sc.assert_geometry(rep_on)
        assert rep_on["share"] >= rep_off["share"], (i, rep_on["share"], rep_off["share"])
        assert all(v == 0 for v in off["map_stats"][-1][i].values()), off["map_stats"][-1][i]
        assert off["stats"][i]["keyframes"] == 1 and all(s[i][:2] == (2, 0) for s in off["states"][1:])


def test_fixed_points_lie_on_the_true_surfaces(trk, orc, shelf):
    """A point fixed from the pair on keyframe k stands at its corner's bearing times the matched range in the keyframe's camera frame and
    is placed in the world with the keyframe's ESTIMATED pose.  It is taken back into the camera frame with the pose the tracker reported
    and out into the world with the renderer's TRUE pose, as tests/test_gpu_depth_map_loop.py does: what is left is the matcher's error.
    At least 95 % within scene_cases.NEAR of a true surface, the cap test_shelf_from_a_stereo_pair applies to seeds"""
    r = mapped_run(trk, shelf, "on")
    scene = sc.shelf_scene(orc)
    for i in range(B):
        truth = poses_of(orc, i)
        pts = r["seeded"][i]
        later = pts[pts[:, 3] > 0]
        assert len(later) >= 20 and len(set(later[:, 3])) >= 1, len(later)
        dist, dist_world = [], []
        for p in later:
            k = int(p[3])
            assert r["states"][k][i][2] == 1, (i, k)              # its keyframe is a keyframe of the run
            T_est, T_true = r["poses"][k][i], truth[k]
            p_cam = quat_to_R(T_est[:4]) @ p[:3] + T_est[4:7]
            p_true = quat_to_R(np.asarray(T_true[:4])).T @ (p_cam - np.asarray(T_true[4:7]))
            dist.append(sc.distance_to_surfaces(scene, p_true)[0])
            dist_world.append(sc.distance_to_surfaces(scene, p[:3])[0])
        dist, dist_world = np.array(dist), np.array(dist_world)
        share = float((dist <= sc.NEAR).mean())
        print("tracker %d: %d points fixed from the pair on %d keyframes: %.1f %% within %g m of a true surface in their keyframe's frame (median %.4g m, "
              "worst %.4g m); as the map holds them (with the keyframes' pose error) %.1f %%, worst %.4g m"
              % (i, len(later), len(set(later[:, 3])), 100 * share, sc.NEAR, float(np.median(dist)), float(dist.max()),
                 100 * float((dist_world <= sc.NEAR).mean()), float(dist_world.max())))
        assert share >= 0.95, (i, share)


def test_trajectory_beside_the_monocular_mapper(trk, orc, shelf):
    on, off, depth = mapped_run(trk, shelf, "on"), mapped_run(trk, shelf, "off"), mapped_run(trk, shelf, "depth")
    worst = {"on": 0.0, "off": 0.0}
    for i in range(B):
        truth = poses_of(orc, i)
        e = {m: max(float(np.linalg.norm(centre(r["poses"][k][i]) - centre(truth[k]))) for k in range(N)) for m, r in (("on", on), ("off", off), ("depth", depth))}
        print("tracker %d: worst camera-centre error over %d frames: stereo mapping %.4g m, monocular mapper behind the stereo bootstrap %.4g m, depth mapping "
              "from the renderer's depth %.4g m" % (i, N, e["on"], e["off"], e["depth"]))
        worst["on"], worst["off"] = max(worst["on"], e["on"]), max(worst["off"], e["off"])
    assert worst["on"] <= 2.0 * worst["off"], worst


def test_inert_without_right_images(trk, shelf):
    """the switch on, but no right image behind the bootstrap: FrameStats, the map's points and the seeded points equal the switch-off
    batch's exactly, and nothing is counted"""
    on, off = mapped_run(trk, shelf, "on", rights_after_bootstrap=False), mapped_run(trk, shelf, "off", rights_after_bootstrap=False)
    assert on["raw"] == off["raw"]
    for i in range(B):
        assert on["points"][i].tobytes() == off["points"][i].tobytes() and len(on["points"][i]) > 0
        assert on["seeded"][i].tobytes() == off["seeded"][i].tobytes()
        assert all(v == 0 for v in on["map_stats"][-1][i].values()), on["map_stats"][-1][i]
    assert any(s[2] for row in on["states"][1:] for s in row), "the run makes keyframes after the bootstrap"


def test_inert_when_never_set(trk, shelf):
    """a stereo batch that is told set_stereo_mapping(on=False) and one that is never told: the same bytes, and what
    tests/test_gpu_stereo_loop.py's mapper test sees — every frame (2, 0), the driver seeds the bootstrap keyframe alone"""
    told, never = mapped_run(trk, shelf, "told-off"), mapped_run(trk, shelf, "off")
    assert told["raw"] == never["raw"]
    for i in range(B):
        assert told["points"][i].tobytes() == never["points"][i].tobytes() and told["seeded"][i].tobytes() == never["seeded"][i].tobytes()
        assert never["stats"][i]["keyframes"] == 1 and all(v == 0 for v in never["map_stats"][-1][i].values())
    assert mapped_run(trk, shelf, "on")["raw"] != never["raw"]


def test_every_combination_that_throws(trk):
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "stereo_map_check")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    r = subprocess.run([exe, "--device"], capture_output=True, text=True, timeout=120)     # the mapper thread can only be started from C++
    assert r.returncode == 0 and "(mapper and tracker): 0 failed" in r.stdout, r.stdout + r.stderr
    cases = [
        # (mapper, what comes first, what must then raise, a word of the message)
        (True, lambda b: None, lambda b: b.set_stereo_mapping(), "stereo seeding"),
        (True, lambda b: b.set_depth(), lambda b: b.set_stereo_mapping(), "stereo seeding"),
        (False, lambda b: b.set_stereo(BASELINE), lambda b: b.set_stereo_mapping(), "mapper"),
        (True, lambda b: b.set_stereo(BASELINE), lambda b: b.set_stereo_mapping(disparity_sigma=-0.1), "disparity_sigma"),
        (True, lambda b: b.set_stereo(BASELINE), lambda b: b.set_stereo_mapping(disparity_sigma=float("nan")), "disparity_sigma"),
        (True, lambda b: b.set_stereo(BASELINE), lambda b: b.set_stereo_mapping(disparity_sigma=float("inf")), "disparity_sigma"),
        (True, lambda b: (b.set_stereo(BASELINE), b.set_stereo_mapping(disparity_sigma=SIGMA)), lambda b: b.set_stereo(BASELINE, on=False), "stereo mapping is on"),
        (True, lambda b: (b.set_stereo(BASELINE), b.set_stereo_mapping(disparity_sigma=SIGMA)), lambda b: b.set_depth(on=False), "stereo mapping is on"),
        (True, lambda b: (b.set_stereo(BASELINE), b.set_stereo_mapping(disparity_sigma=SIGMA)), lambda b: b.set_depth_mapping(), "stereo pair"),
    ]
    for n, (mapper, first, then, word) in enumerate(cases):
        dev, batch = make_batch(trk, n=1, mapper=mapper)
        try:
            first(batch)
            with pytest.raises(RuntimeError, match=word):
                then(batch)
        except BaseException:
            print("case %d" % n)
            raise
        finally:
            batch.close()
            dev.close()
    dev, batch = make_batch(trk, n=1)
    try:
        batch.set_stereo(BASELINE)
        trk.set_device_filter(False)
        try:
            with pytest.raises(RuntimeError, match="host depth filter"):
                batch.set_stereo_mapping(disparity_sigma=SIGMA)
        finally:
            trk.set_device_filter(True)
        # and what the switch leaves alone: on, another sigma, off, stereo seeding off behind it
        batch.set_stereo_mapping(disparity_sigma=SIGMA)
        batch.set_stereo_mapping(disparity_sigma=0.1)
        batch.set_stereo_mapping(on=False)
        batch.set_stereo(BASELINE, on=False)
    finally:
        batch.close()
        dev.close()
    dev, batch = make_batch(trk, n=1, mapper=False)
    try:
        with pytest.raises(RuntimeError):
            batch.stereo_map_stats(0)
    finally:
        batch.close()
        dev.close()


def test_track_sequence_stereo_mapping():
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    n = 16
    r = subprocess.run([exe, "--synthetic", str(n), "--scene", "shelf", "--stereo", "--baseline", "0.11", "--stereo-mapping", "--disparity-sigma", str(SIGMA),
                        "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [l.split() for l in lines[:-1]]
    assert len(rows) == n and all([int(v) for v in row[1:3]] == [2, 0] for row in rows[1:]), rows
    out = json.loads(lines[-1])
    assert out["tracked"] == n - 1 and out["mapper"] is True
    sm = out["stereo_mapping"]
    assert set(sm) == STAT_NAMES, sm
    assert "stereo mapping: %d measured updates" % sm["measured"] in r.stderr and "stereo seeding: 1 keyframes" in r.stderr, r.stderr
    print(sm)
