"""The two-frame initialisation on the device, through the C-ABI: sdvl_klt_track and sdvl_homography_ransac against their numpy
restatements (tests/klt_restatement.py, tests/homography_restatement.py) and against the truth of the scenes of tests/init_cases.py.

KLT.  Status must equal the float64 restatement's and every kept point must lie within init_cases.KLT_TOL = max(4 g, 0.01 px) of
it, g = 8.4e-4 px being the float32-against-float64 gap of the restatement itself (tests/test_init_restatement_cpu.py) and 0.01 px
the half step of the oscillation rule.  Points whose restatement result lies within 0.01 px of the image bound, or whose level-0
min-eigenvalue lies within 1e-3 relative of the threshold, may differ: at most 2 % of a call's points (the CPU tests show that the
scenes hold none).  Sizes: 1, 63, 64, 65 and 284 points in one job; three jobs of 0, 1 and 284 points over two frame pairs in one
call; a 160x120 pair whose level 4 (10x7) is smaller than the window, points 3 px from each border; initial flow equal to the
previous position and to the truth + 3 px.

RANSAC.  best_draw and n_its equal the restatement's; the inlier lists are equal apart from matches whose squared error is within
1e-9 relative of the squared threshold (none is expected, at most 1 %); H scaled to unit norm within 1e-4.  n = 4, 5, 64, 65, 300,
outlier shares 0 and 0.3, draw tables with a repeated index and a collinear triple, two jobs of different n in one call.

The chain.  Two frames to a scaled relative pose without any CPU stand-in: sdvl_klt_track for three trackers in one call,
sdvlh_homography_matches, sdvl_homography_ransac for the three in one call, sdvlh_homography_from_inliers (host/homography_init.cc).
On scenes A and B: the median shift passes min_avg_shift = 20, at least min_init_corners = 50 points survive
CheckDecompositionInliers, the visibility test alone decides, and pose and baseline lie within the bounds of
tests/test_init_restatement_cpu.py (rotation 0.1 deg, translation direction 0.5 deg, baseline 5.5 % / 9.7 %).  A second frame from
the first pose (another noise draw) keeps every point and shifts by less than a pixel: the tracker would stay in its second-frame state.

Run with -s: every test prints its figures before it asserts."""
import importlib

import numpy as np
import pytest

import init_cases as ic
from homography_restatement import ransac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx, orc, synth):
    """frame 0, the scenes and the small pair on the device, each uploaded once"""
    f0, sm = ic.frame0(orc, synth), ic.small(orc, synth)
    d = dict(f0=ctx.frame(f0["img"], levels=5), A=ctx.frame(ic.scene(orc, synth, "A")["img"], levels=5),
             B=ctx.frame(ic.scene(orc, synth, "B")["img"], levels=5), s0=ctx.frame(sm["img0"], levels=5), s1=ctx.frame(sm["img1"], levels=5))
    yield d
    for f in d.values():
        f.close()


def check_klt(got, ref, sel, w, h, label):
    """got: one job's answer for the points ref[sel]"""
    st_ref, xy_ref = ref["status"][sel], ref["xy"][sel].astype(np.float64)
    ex = ic.klt_excepted(ref, w, h)[sel]
    both = got["status"] & st_ref & ~ex
    gap = float(np.abs(got["xy"][both].astype(np.float64) - xy_ref[both]).max()) if both.any() else 0.0
    flips = int(((got["status"] != st_ref) & ~ex).sum())
    print(label, "points", len(st_ref), "kept", int(st_ref.sum()), "excepted", int(ex.sum()), "status flips", flips, "largest gap", gap)
    assert ex.sum() <= 0.02 * len(ex)    # the cap; the scenes hold none
    assert flips == 0
    assert gap <= ic.KLT_TOL
    assert np.all(got["err"][got["status"]] >= 0) and np.all(got["err"][~got["status"]] == 0)


def test_device_pyramid_is_the_restatements_input(dev, orc, synth):
    """the restatement reads the oracle's pyrDown levels, the kernel the frames' own: the same bytes, the 10x7 level included"""
    sm = ic.small(orc, synth)
    for l in range(5):
        assert np.array_equal(dev["s0"].level(l), sm["pyr0"][l]) and np.array_equal(dev["s1"].level(l), sm["pyr1"][l])
    assert sm["pyr0"][4].shape == (7, 10)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 284])
def test_klt_against_restatement(ctx, dev, orc, synth, n):
    f0, ref = ic.frame0(orc, synth), ic.klt_reference(orc, synth, "A")
    assert len(f0["px"]) == 284
    got = ctx.klt_track([(dev["f0"], dev["A"], f0["px"][:n], f0["px"][:n])])[0]
    check_klt(got, ref, slice(0, n), ic.W, ic.H, "A n=%d" % n)


def test_klt_three_jobs_in_one_call(ctx, dev, orc, synth):
    f0 = ic.frame0(orc, synth)
    refA, refB = ic.klt_reference(orc, synth, "A"), ic.klt_reference(orc, synth, "B")
    px = f0["px"]
    got = ctx.klt_track([(dev["f0"], dev["A"], px[:0], px[:0]), (dev["f0"], dev["B"], px[100:101], px[100:101]), (dev["f0"], dev["A"], px, px)])
    assert len(got[0]["status"]) == 0
    check_klt(got[1], refB, slice(100, 101), ic.W, ic.H, "job of 1 (B)")
    check_klt(got[2], refA, slice(0, 284), ic.W, ic.H, "job of 284 (A)")


def test_klt_initial_flow_near_truth(ctx, dev, orc, synth):
    f0, ref = ic.frame0(orc, synth), ic.klt_reference(orc, synth, "A", "truth+3")
    got = ctx.klt_track([(dev["f0"], dev["A"], f0["px"], ref["start"])])[0]
    check_klt(got, ref, slice(0, 284), ic.W, ic.H, "A from truth + 3 px")


@pytest.mark.parametrize("init", ["prev", "truth+3"])
def test_klt_small_frame(ctx, dev, orc, synth, init):
    sm, ref = ic.small(orc, synth), ic.klt_reference(orc, synth, "SMALL", init)
    got = ctx.klt_track([(dev["s0"], dev["s1"], sm["px"], ref["start"])])[0]
    check_klt(got, ref, slice(0, len(sm["px"])), ic.SMALL_W, ic.SMALL_H, "160x120 " + init)


@pytest.mark.parametrize("name", ["A", "B"])
def test_klt_against_truth(ctx, dev, orc, synth, name):
    f0, s = ic.frame0(orc, synth), ic.scene(orc, synth, name)
    got = ctx.klt_track([(dev["f0"], dev[name], f0["px"], f0["px"])])[0]
    e = np.linalg.norm(got["xy"].astype(np.float64) - s["truth"], axis=1)
    m = s["interior"]
    good = (got["status"] & (e <= 0.5))[m]
    print(name, "kept", int(got["status"].sum()), "interior", int(m.sum()), "within 0.5 px", int(good.sum()), "median", float(np.median(e[m])))
    assert good.sum() >= 0.95 * m.sum()


def test_klt_refusals(sdvl, ctx, dev, orc, synth):
    px = ic.frame0(orc, synth)["px"][:4]
    with pytest.raises(sdvl.SdvlError):                       # frames of different sizes
        ctx.klt_track([(dev["f0"], dev["s1"], px, px)])
    with pytest.raises(sdvl.SdvlError):                       # only the 30x30 window
        ctx.klt_track([(dev["f0"], dev["A"], px, px)], win_size=21)
    with pytest.raises(sdvl.SdvlError):                       # a level the pyramids do not have
        ctx.klt_track([(dev["f0"], dev["A"], px, px)], max_level=5)
    other = sdvl.Context(0)
    try:
        f = other.frame(ic.frame0(orc, synth)["img"], levels=5)
        other.synchronize()
        with pytest.raises(sdvl.SdvlError):                   # a frame of another context
            ctx.klt_track([(dev["f0"], f, px, px)])
        f.close()
    finally:
        other.close()


def test_klt_second_frame_without_motion(ctx, dev, orc, synth):
    """the first pose rendered again with another noise draw: every point kept, median shift far below SDVL.min_avg_shift"""
    from pose_restatement import se3_exp
    f0 = ic.frame0(orc, synth)
    again = synth.render(se3_exp(np.zeros(6)), ic.TUM_CAM, ic.W, ic.H, plane=ic.PLANE, texture=1, frame_id=1)
    fr = ctx.frame(again, levels=5)
    try:
        got = ctx.klt_track([(dev["f0"], fr, f0["px"], f0["px"])])[0]
    finally:
        fr.close()
    shift = np.median(np.linalg.norm(got["xy"].astype(np.float64) - f0["px"], axis=1)[got["status"]])
    print("kept", int(got["status"].sum()), "median shift", float(shift))
    assert got["status"].all() and shift < 1.0 < ic.MIN_AVG_SHIFT


# --------------------------------------------------------------------------------------------------------------- RANSAC
def check_ransac(got, c, label):
    want = ransac(c["src"], c["dst"], c["draws"], c["threshold"])
    t2 = c["threshold"] ** 2
    near = np.abs(want["d2"] - t2) <= 1e-9 * t2
    diff = set(got["inliers"].tolist()) ^ set(want["inliers"].tolist())
    hgap = float(np.abs(ic.unit_h(got["H"]) - ic.unit_h(want["H"])).max()) if want["best_draw"] >= 0 else 0.0
    print(label, "best_draw", got["best_draw"], want["best_draw"], "n_its", got["n_its"], want["n_its"], "inliers", len(got["inliers"]),
          len(want["inliers"]), "borderline", int(near.sum()), "H gap", hgap)
    assert got["best_draw"] == want["best_draw"] and got["n_its"] == want["n_its"]
    assert near.sum() <= 0.01 * len(near)
    assert diff <= set(np.nonzero(near)[0].tolist())
    assert np.all(np.diff(got["inliers"]) > 0)
    assert hgap <= 1e-4


@pytest.mark.parametrize("share", [0.0, 0.3])
@pytest.mark.parametrize("n", [4, 5, 64, 65, 300])
def test_ransac_against_restatement(ctx, n, share):
    c = ic.ransac_case(n, share, 11 + n)
    got = ctx.homography_ransac([(c["src"], c["dst"], c["draws"])], c["threshold"])[0]
    check_ransac(got, c, "n=%d share=%.1f" % (n, share))


def test_ransac_walk_past_the_first_wave_of_draws(ctx):
    """six matches in ten are gross outliers: the budget stays above 64 draws, the walk crosses the hypotheses kernel's blocks and the
    best draw improves several times (an addition to the issue's cases, same rule)"""
    c = ic.ransac_case(300, 0.6, 611)
    got = ctx.homography_ransac([(c["src"], c["dst"], c["draws"])], c["threshold"])[0]
    check_ransac(got, c, "n=300 share=0.6")
    assert got["n_its"] > 64


def test_ransac_two_jobs_in_one_call(ctx):
    a, b, e = ic.ransac_case(65, 0.3, 5), ic.ransac_case(300, 0.0, 311), ic.ransac_case(64, 0.3, 75)
    cut = dict(e, draws=e["draws"][:2])                       # only the two degenerate draws: no model
    got = ctx.homography_ransac([(a["src"], a["dst"], a["draws"]), (b["src"], b["dst"], b["draws"]), (cut["src"], cut["dst"], cut["draws"])],
                                a["threshold"])
    check_ransac(got[0], a, "job 0 (65)")
    check_ransac(got[1], b, "job 1 (300)")
    check_ransac(got[2], cut, "job 2 (degenerate draws only)")
    assert got[2]["best_draw"] == -1 and got[2]["n_its"] == 2 and len(got[2]["inliers"]) == 0


def test_ransac_refusals(sdvl, ctx):
    c = ic.ransac_case(64, 0.0, 75)
    bad = c["draws"].copy()
    bad[3, 2] = 64                                            # an index outside the match list
    with pytest.raises(sdvl.SdvlError):
        ctx.homography_ransac([(c["src"], c["dst"], bad)], c["threshold"])
    big = np.zeros((8193, 2))
    with pytest.raises(sdvl.SdvlError):                       # beyond the cap of 8192 matches
        ctx.homography_ransac([(big, big, c["draws"])], c["threshold"])


# ------------------------------------------------------------------------------------------------------------ the chain
def test_two_frames_to_a_scaled_pose(ctx, dev, orc, synth):
    from pose_restatement import quat_to_rot
    from test_init_restatement_cpu import SCALE_GAP
    host = ic.host_library()
    f0 = ic.frame0(orc, synth)
    px = f0["px"]
    names = ["A", "B", "A"]
    tracks = ctx.klt_track([(dev["f0"], dev[nm], px, px) for nm in names])           # all trackers' KLT in one call
    jobs, kept = [], []
    for k, (nm, tr) in enumerate(zip(names, tracks)):
        ok = tr["status"]
        px1, px2 = px[ok], tr["xy"][ok]
        shift = np.median(np.linalg.norm(px1.astype(np.float64) - px2.astype(np.float64), axis=1))
        assert shift >= ic.MIN_AVG_SHIFT and ok.sum() >= 50
        src, dst = ic.host_matches(host, px1, px2, ic.TUM_CAM)
        jobs.append((src, dst, ic.draws_table(int(ok.sum()), 2000, 40 + k)))
        kept.append((ok, px1, px2))
    found = ctx.homography_ransac(jobs, 2.0 / ic.TUM_CAM[0])                          # all trackers' RANSAC in one call
    for nm, (ok, px1, px2), r in zip(names, kept, found):
        assert r["best_draw"] >= 0 and r["n_its"] <= 2000
        g = ic.host_init(host, px1, px2, ic.TUM_CAM, r["inliers"], min_init_corners=50)
        s = ic.scene(orc, synth, nm)
        rot, tdir = ic.pose_errors(g["R"], g["t"], s["T"])
        baseline = np.linalg.norm(-g["R"].T @ g["t"])
        want = np.linalg.norm(-quat_to_rot(s["T"][:4]).T @ s["T"][4:]) / np.median(f0["depth"][ok])
        print(nm, "tracked", int(ok.sum()), "ransac inliers", len(r["inliers"]), "n_its", r["n_its"], "candidates", len(g["inliers"]), "scores", g["scores"],
              "rotation", rot, "translation direction", tdir, "baseline", baseline, "expected", want)
        assert g["rc"] == 1 and len(g["inliers"]) >= 50
        assert g["scores"][1] / g["scores"][0] < 0.9
        assert rot <= 0.1 and tdir <= 0.5
        assert abs(baseline / want - 1.0) <= SCALE_GAP[nm]


# ------------------------------------------------------------------------------------------- the tracker starts from a camera
TRACKING_BAD = 2


@pytest.fixture(scope="module")
def trk():
    return importlib.import_module("slam-sdvl_amd.tracker")


def _mapper_batch(trk, B, two_frame):
    trk.configure(dict(trk.TUM_OVERRIDES, **{"SDVL.min_avg_shift": ic.MIN_AVG_SHIFT}))
    trk.set_mapper(True)
    try:
        dev = trk.HostDevice(0)
        batch = trk.TrackerBatch(dev, B, ic.W, ic.H, ic.TUM_CAM)
    finally:
        trk.set_mapper(False)
    if two_frame is not None:
        batch.set_two_frame_init(two_frame)
    return dev, batch


@pytest.mark.parametrize("B", [1, 3])
def test_tracker_batch_initialises_from_two_frames(trk, orc, synth, B):
    """TrackerBatch with set_mapper(True) and set_two_frame_init(True): frame 0 -> state 0 and one keyframe; the same pose again
    (frame_id 1) -> state 1, no map; scene A's frame -> state 2, two keyframes, candidates >= min_init_corners, the pose within the
    bounds of tests/test_init_restatement_cpu.py; then frames further along the sideways motion: never TRACKING_BAD, matches >=
    min_matches.  Their pose error against the scaled truth is printed, not asserted.  With B = 3 the middle
    tracker sees the unmoved frame once more, so one step holds two initialising trackers and a waiting one, and the next steps two
    running trackers beside an initialising one."""
    from pose_restatement import quat_to_rot, se3_exp
    from test_init_restatement_cpu import SCALE_GAP
    dev, batch = _mapper_batch(trk, B, True)
    try:
        f0, sA = ic.frame0(orc, synth), ic.scene(orc, synth, "A")
        ident = se3_exp(np.zeros(6))
        still = [synth.render(ident, ic.TUM_CAM, ic.W, ic.H, plane=ic.PLANE, texture=1, frame_id=k) for k in (1, 9)]
        follow = []
        for k in range(1, 6):
            T = se3_exp(ic.POSES["A"] * (1.0 + 0.2 * k))
            follow.append(("follow", synth.render(T, ic.TUM_CAM, ic.W, ic.H, plane=ic.PLANE, texture=1, frame_id=2 + k), T))
        plain = [("first", f0["img"], None), ("still", still[0], None), ("init", sA["img"], sA["T"])] + follow
        lagged = plain[:2] + [("still", still[1], None)] + plain[2:-1]
        seqs = [lagged if i == 1 else plain for i in range(B)]
        scale = [None] * B
        n_follow = [0] * B
        for step in range(len(plain)):
            st = batch.step_host([seqs[i][step][1] for i in range(B)])
            for i in range(B):
                kind, _, T = seqs[i][step]
                ms = batch.map_stats(i)
                g = st[i]
                pose = np.array(g.pose[:])
                R, t = quat_to_rot(pose[:4]), pose[4:]
                if kind == "first":
                    assert (g.state, g.keyframe) == (0, 1) and ms["keyframes"] == 1
                elif kind == "still":
                    assert (g.state, g.keyframe) == (1, 0) and ms["keyframes"] == 1 and ms["candidates"] == 0
                elif kind == "init":
                    rot, tdir = ic.pose_errors(R, t, T)
                    t_true = np.linalg.norm(-quat_to_rot(T[:4]).T @ T[4:])
                    baseline = np.linalg.norm(-R.T @ t)
                    scale[i] = baseline / t_true
                    print("step", step, "tracker", i, "state", g.state, "keyframes", ms["keyframes"], "candidates", ms["candidates"], "rotation", rot,
                          "translation direction", tdir, "baseline", baseline, "scale", scale[i])
                    assert (g.state, g.keyframe) == (2, 1) and ms["keyframes"] == 2
                    assert ms["candidates"] >= 50
                    assert rot <= 0.1 and tdir <= 0.5
                    assert abs(baseline * np.median(f0["depth"]) / t_true - 1.0) <= SCALE_GAP["A"]
                else:
                    rot, _ = ic.pose_errors(R, t, T)
                    gap = np.linalg.norm(-R.T @ t - scale[i] * (-quat_to_rot(T[:4]).T @ T[4:]))
                    print("step", step, "tracker", i, "follow-on: quality", g.quality, "matches", g.matches, "keyframe", g.keyframe,
                          "rotation error", rot, "camera centre gap (map units)", gap)
                    assert g.state == 2 and g.quality != TRACKING_BAD and g.matches >= 20
                    n_follow[i] += 1
        assert min(n_follow) >= 4 and n_follow[0] == 5
    finally:
        batch.close()
        dev.close()
        trk.configure()


def test_two_frame_init_needs_the_mapper(trk):
    trk.configure()
    dev = trk.HostDevice(0)
    batch = trk.TrackerBatch(dev, 1, ic.W, ic.H, ic.TUM_CAM)          # plane map stub
    try:
        with pytest.raises(RuntimeError):
            batch.set_two_frame_init(True)
    finally:
        batch.close()
        dev.close()


def test_switch_off_changes_nothing(trk, orc, synth):
    """a batch told set_two_frame_init(False) gives the FrameStats of a batch that never heard of the switch, byte for byte"""
    from oraclelib import trajectory_pose
    imgs = [synth.render(trajectory_pose(orc, k), ic.TUM_CAM, ic.W, ic.H, frame_id=k) for k in range(5)]
    runs = []
    for two_frame in (None, False):
        dev, batch = _mapper_batch(trk, 1, two_frame)
        try:
            runs.append([bytes(batch.step_host([im])[0]) for im in imgs])
        finally:
            batch.close()
            dev.close()
    trk.configure()
    assert runs[0] == runs[1]
