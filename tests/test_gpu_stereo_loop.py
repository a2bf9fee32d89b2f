"""Stereo cameras in the closed loop (TrackerBatch.set_stereo): trackers that seed their keyframes from the rectified right image of a
pair, matched at the keyframes' filtered corners by sdvl_stereo_depth.  40 device-rendered pairs of 640 x 480 of `shelf`, B = 2, baseline
0.11 m; the right camera's centre is the left one's plus the baseline along the left camera's x axis, the same orientation.

1. the plane map with a deliberately WRONG plane: tracked on every frame after the first with enough matches, the seeds on the true
   surfaces, the pose error beside the same batch seeded from the renderer's true depth image
2. the reference's mapper behind a stereo bootstrap
3. the switch: inert when off, a first frame without a right image, every combination that throws"""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import scene_cases as sc
import stereo_cases as stc
from oraclelib import TUM_CAM, TUM2_DIST, quat_to_R, trajectory_pose

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, W, H = 2, sc.N_FRAMES, sc.W, sc.H
FB = W * H
WALL = (0, 0, 1, 2.0)
WRONG_PLANE = (0, 0, 1, 5.0)
BASELINE = stc.BASELINE


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
    """N pairs of B trackers in HBM: frame k of tracker i at img(i, k), its right image at right(i, k), the left view's true depth at depth(i, k)"""

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

    def host(self, ptr):
        return self.ctx.device_download(ptr, FB).reshape(H, W)

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


def make_batch(trk, n=B, plane4=WALL, mapper=False):
    trk.configure()
    trk.set_mapper(mapper)
    try:
        dev = trk.HostDevice(0)
        return dev, trk.TrackerBatch(dev, n, W, H, TUM_CAM, plane4=plane4, host_threads=1)
    finally:
        trk.set_mapper(False)


def raw(stats, i):
    return bytes(memoryview(stats[i]))


def centre(T):
    return -quat_to_R(np.asarray(T[:4])).T @ np.asarray(T[4:7])


def plane_map_run(trk, shelf, stereo):
    """the plane map with a WRONG plane on `shelf`, seeded from the right images (stereo) or from the renderer's true depth"""
    dev, batch = make_batch(trk, plane4=WRONG_PLANE)
    try:
        if stereo:
            batch.set_stereo(BASELINE)
        else:
            batch.set_depth()
        states, poses = [], []
        for k in range(N):
            st = batch.step_device(shelf.imgs(k), right_ptrs=shelf.rights(k)) if stereo else batch.step_device(shelf.imgs(k), shelf.depths(k))
            states.append([(st[i].state, st[i].quality, st[i].keyframe, st[i].matches) for i in range(B)])
            poses.append([np.array(st[i].pose[:]) for i in range(B)])
        return dict(states=states, poses=poses, seeded=[batch.seeded_points(i) for i in range(B)],
                    stats=[batch.stereo_stats(i) if stereo else batch.depth_stats(i) for i in range(B)])
    finally:
        batch.close()
        dev.close()


def test_shelf_from_a_stereo_pair(trk, orc, shelf):
    """every frame after the first (which is the bootstrap keyframe, state 0) is tracked, state 2, with at least scene_cases.MIN_MATCHES
    matches; at least 95 % of the seeded points lie within scene_cases.NEAR of a surface; the worst camera-centre error over the run is at
    most TWICE that of the same batch seeded from the renderer's true depth image"""
    r = plane_map_run(trk, shelf, True)
    d = plane_map_run(trk, shelf, False)
    scene = sc.shelf_scene(orc)
    worst = {"stereo": 0.0, "depth": 0.0}
    for i in range(B):
        assert r["states"][0][i][:3] == (0, 0, 1), r["states"][0][i]
        for k in range(1, N):
            assert r["states"][k][i][0] == 2 and r["states"][k][i][3] >= sc.MIN_MATCHES, (i, k, r["states"][k][i])
        pts = r["seeded"][i]
        dist = np.array([sc.distance_to_surfaces(scene, p[:3])[0] for p in pts])
        share = float((dist <= sc.NEAR).mean())
        st = r["stats"][i]
        truth = poses_of(orc, i)
        e_s = max(float(np.linalg.norm(centre(r["poses"][k][i]) - centre(truth[k]))) for k in range(N))
        e_d = max(float(np.linalg.norm(centre(d["poses"][k][i]) - centre(truth[k]))) for k in range(N))
        print("tracker %d: %d live seeds of %d keyframes, %.1f %% within %g m of a surface (median %.4f m); fewest matches %d; worst camera-centre "
              "error over %d frames: stereo %.4g m, true depth %.4g m; %s"
              % (i, len(pts), st["keyframes"], 100 * share, sc.NEAR, float(np.median(dist)), min(s[i][3] for s in r["states"][1:]), N, e_s, e_d, st))
        assert len(pts) >= 150 and len(set(pts[:, 3])) >= 2, (i, len(pts))
        assert share >= 0.95, (i, share)
        assert st["seeds"] == st["ok"] and st["keyframes"] >= 2 and st["no_image"] == 0 and st["ok"] > 0 and st["nomatch"] > 0, st
        worst["stereo"], worst["depth"] = max(worst["stereo"], e_s), max(worst["depth"], e_d)
    assert worst["stereo"] <= 2.0 * worst["depth"], worst


def test_mapper_behind_a_stereo_bootstrap(trk, orc, shelf):
    dev, batch = make_batch(trk, plane4=WRONG_PLANE, mapper=True)
    try:
        batch.set_stereo(BASELINE)
        for k in range(N):
            st = batch.step_device(shelf.imgs(k), right_ptrs=shelf.rights(k))
            for i in range(B):
                if k > 0:
                    assert (st[i].state, st[i].quality) == (2, 0), (i, k, st[i].state, st[i].quality)
        scene = sc.shelf_scene(orc)
        for i in range(B):
            rep = sc.geometry_report(scene, batch.map_points(i))
            print("tracker %d: mapper behind the stereo bootstrap: %s; %s" % (i, rep, batch.stereo_stats(i)))
            sc.assert_geometry(rep)
            assert batch.stereo_stats(i)["keyframes"] == 1      # the bootstrap keyframe alone; the mapper seeds the others
    finally:
        batch.close()
        dev.close()


def test_inert_when_off(trk, shelf):
    """set_stereo(on=False), and right images handed to a batch that was never told about stereo, change nothing: FrameStats byte for byte"""
    n = 12

    def run(batch, rights):
        out = []
        for k in range(n):
            st = batch.step_device(shelf.imgs(k), right_ptrs=shelf.rights(k)) if rights else batch.step_device(shelf.imgs(k))
            out.append([raw(st, i) for i in range(B)])
        return out

    dev, batch = make_batch(trk)
    try:
        want = run(batch, False)
    finally:
        batch.close()
        dev.close()
    for told in (True, False):
        dev, batch = make_batch(trk)
        try:
            if told:
                batch.set_stereo(BASELINE, on=False)
            assert run(batch, True) == want, told
            assert batch.stereo_stats(0)["keyframes"] == 0 and len(batch.seeded_points(0)) == 0
        finally:
            batch.close()
            dev.close()


def test_first_frame_without_a_right_image_starts_over(trk, shelf):
    dev, batch = make_batch(trk, plane4=WRONG_PLANE)
    try:
        batch.set_stereo(BASELINE)
        st = batch.step_device(shelf.imgs(0), right_ptrs=[None, shelf.rights(0)[1]])
        assert (st[0].state, st[0].keyframe) == (0, 0) and (st[1].state, st[1].keyframe) == (0, 1)
        assert len(batch.seeded_points(0)) == 0 and len(batch.seeded_points(1)) >= 150
        st = batch.step_device(shelf.imgs(1))                       # no right images at all: tracker 0 still waits, tracker 1 tracks
        assert (st[0].state, st[0].keyframe) == (0, 0) and (st[1].state, st[1].quality) == (2, 0)
        st = batch.step_device(shelf.imgs(2), right_ptrs=shelf.rights(2))
        assert (st[0].state, st[0].keyframe) == (0, 1) and (st[1].state, st[1].quality) == (2, 0)
        for k in range(3, 8):
            st = batch.step_device(shelf.imgs(k), right_ptrs=shelf.rights(k))
            assert all((st[i].state, st[i].quality) == (2, 0) for i in range(B)), k
        assert batch.stereo_stats(0)["no_image"] == 2 and batch.stereo_stats(1)["no_image"] == 0
        # too few OK corners: a right image that shows something else is not kept either (host images, under the name rights=)
        dev2, b2 = make_batch(trk, n=1, plane4=WRONG_PLANE)
        try:
            b2.set_stereo(BASELINE)
            left0, left1 = shelf.host(shelf.imgs(0)[0]), shelf.host(shelf.imgs(1)[0])
            st = b2.step_host([left0], rights=[np.ascontiguousarray(left0[::-1])])
            assert (st[0].state, st[0].keyframe) == (0, 0) and len(b2.seeded_points(0)) == 0
            st = b2.step_host([left1], rights=[shelf.host(shelf.rights(1)[0])])
            assert (st[0].state, st[0].keyframe) == (0, 1) and len(b2.seeded_points(0)) >= 150
            with pytest.raises(ValueError):
                b2.step_host([left1], depths=[left1], rights=[left1])
            with pytest.raises(ValueError):
                b2.step_device(shelf.imgs(2)[:1], depth_ptrs=shelf.rights(2)[:1], right_ptrs=shelf.rights(2)[:1])
        finally:
            b2.close()
            dev2.close()
    finally:
        batch.close()
        dev.close()


def write_pgm(path, a):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a, np.uint8).tobytes())


def test_track_sequence_stereo(trk, shelf, tmp_path):
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    r = subprocess.run([exe, "--synthetic", str(N), "--scene", "shelf", "--stereo", "--baseline", "0.11", "--plane", "0", "0", "1", "5", "--json"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [l.split() for l in lines[:-1]]
    assert len(rows) == N and all([int(v) for v in row[1:3]] == [2, 0] for row in rows[1:]), rows
    assert json.loads(lines[-1])["tracked"] == N - 1
    assert "--plane is ignored" in r.stderr and "stereo seeding:" in r.stderr
    # two pairs as 8-bit P5 files through --right-list: the frames of the same images passed from Python
    imgs = [shelf.host(shelf.imgs(k)[0]) for k in range(2)]
    rights = [shelf.host(shelf.rights(k)[0]) for k in range(2)]
    for k in range(2):
        write_pgm(str(tmp_path / ("f%d.pgm" % k)), imgs[k])
        write_pgm(str(tmp_path / ("r%d.pgm" % k)), rights[k])
    (tmp_path / "frames.txt").write_text("".join("%s\n" % (tmp_path / ("f%d.pgm" % k)) for k in range(2)))
    (tmp_path / "right.txt").write_text("".join("%s\n" % (tmp_path / ("r%d.pgm" % k)) for k in range(2)))
    r = subprocess.run([exe, "--list", str(tmp_path / "frames.txt"), "--right-list", str(tmp_path / "right.txt"), "--baseline", "0.11"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in r.stdout.strip().splitlines()]
    dev, batch = make_batch(trk, n=1, plane4=WRONG_PLANE)
    try:
        batch.set_stereo(BASELINE)
        for k in range(2):
            st = batch.step_host([imgs[k]], rights=[rights[k]])[0]
            assert [int(v) for v in rows[k][:6]] == [k, st.state, st.quality, st.matches, st.attempts, st.inliers], (k, rows[k])
            assert [float(v) for v in rows[k][6:13]] == list(st.pose[:]), k
        ds = batch.stereo_stats(0)
    finally:
        batch.close()
        dev.close()
    want = "stereo seeding: %d keyframes, %d seeds; corners OK %d NOMATCH %d AMBIGUOUS %d EDGE %d OUTSIDE %d; %d frames without a right image" % (
        ds["keyframes"], ds["seeds"], ds["ok"], ds["nomatch"], ds["ambiguous"], ds["edge"], ds["outside"], ds["no_image"])
    assert want in r.stderr and ds["seeds"] >= 150, (want, r.stderr)


def test_every_combination_that_throws(trk):
    def fresh(mapper):
        return make_batch(trk, n=1, mapper=mapper)

    cases = [
        # (mapper, what comes first, what must then raise)
        (True, lambda b: b.set_two_frame_init(True), lambda b: b.set_stereo(BASELINE)),
        (True, lambda b: b.set_stereo(BASELINE), lambda b: b.set_two_frame_init(True)),
        (False, lambda b: b.set_depth(), lambda b: b.set_stereo(BASELINE)),
        (False, lambda b: b.set_stereo(BASELINE), lambda b: b.set_depth()),
        (True, lambda b: b.set_stereo(BASELINE), lambda b: b.set_depth_mapping()),
        (True, lambda b: (b.set_depth(), b.set_depth_mapping()), lambda b: b.set_stereo(BASELINE)),
        (True, lambda b: (b.set_stereo(BASELINE), b.set_bundle_adjustment(True)), lambda b: b.set_depth_bundle()),
        (True, lambda b: (b.set_depth(), b.set_bundle_adjustment(True), b.set_depth_bundle()), lambda b: b.set_stereo(BASELINE)),
        (False, lambda b: b.set_distortion(TUM2_DIST), lambda b: b.set_stereo(BASELINE)),
        (False, lambda b: None, lambda b: b.set_stereo(0.0)),
        (False, lambda b: None, lambda b: b.set_stereo(float("nan"))),
        (False, lambda b: None, lambda b: b.set_stereo(BASELINE, max_disparity=512)),
        (False, lambda b: None, lambda b: b.set_stereo(BASELINE, uniqueness=101)),
    ]
    for n, (mapper, first, then) in enumerate(cases):
        dev, batch = fresh(mapper)
        try:
            first(batch)
            with pytest.raises(RuntimeError):
                then(batch)
        except BaseException:
            print("case %d" % n)
            raise
        finally:
            batch.close()
            dev.close()
    # and what the switch leaves alone: off and on again, another baseline
    dev, batch = fresh(False)
    try:
        batch.set_stereo(BASELINE)
        batch.set_stereo(BASELINE, on=False)
        batch.set_depth()
        batch.set_depth(on=False)
        batch.set_stereo(0.05, max_disparity=128)
    finally:
        batch.close()
        dev.close()
