"""The tracked step's table kernels (csrc/sdvl_track.hip: track_upload, track_project, track_clear_bins, track_commit, the registry
writes, and the table source of the alignment) against tests/track_restatement.py, on tables the test makes itself: the cases of
tests/track_cases.py, each asserted there (without a GPU) to be what it claims.  Per case the restatement is fed
    T       from ctx.image_align on the equivalent AlignFeature records (px, bearing, depth = |P - C_last|, valid = has a live point),
    search  the oracle's SearchPoint answers,
    pose    the oracle's SelectInliers + OptimizePose on the same rand() stream,
and every integer of sdvl_track_result, every row of the point statistics and every row of the new feature list must equal it; the
alignment's figures and the pose are bit-equal to the plain entry points' (ctx.image_align, ctx.pose_from_matches), the feature
positions bit-equal to the oracle's, the pose within POSE_TOL of the oracle's, the scene depth the restated median of the device's
own pose within 32 ulp of |P| + |t| (a dozen FP64 operations from a unit quaternion)."""
import importlib
import math
from collections import Counter

import numpy as np
import pytest

import track_cases as tc
import track_restatement as tr
from test_gpu_parity import POSE_TOL

pytestmark = pytest.mark.gpu

MAX_POINTS, MAX_FEATURES = 768, 704
_w = {"compared": Counter(), "trace": Counter(), "alone": {}}


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    for s in _w.get("sets", {}).values():
        s.close()
    for f in _w.get("frames", {}).values():
        f.close()
    c.close()


@pytest.fixture(scope="module")
def world(ctx, sdvl, orc, synth):
    """the scene, its cases, the reference frame (registered at the identity) and the parameters of a step, made once"""
    if "sc" not in _w:
        sc = tc.scene(orc, synth)
        _w.update(sc=sc, cases=tc.by_name(tc.cases(sc)), frames={}, sets={})
        _w["frames"]["ref"] = ctx.frame(sc["img"]["same"])
        _w["frames"]["ref"].set_corners(sc["corners"]["same"])
        ctx.register([_w["frames"]["ref"]], [tc.ID])
        _w["cam"] = sdvl.Camera(tc.W, tc.H, *tc.CAM4)
        _w["draws"] = {}
    return _w


def params(sdvl, orc, max_its):
    p = sdvl.TrackParams()
    p.align = sdvl.default_align_params()
    p.align.max_its = max_its
    p.search = sdvl.default_search_params()
    p.pose = sdvl.PoseParams(orc.params.max_ransac_points, orc.params.max_ransac_its, orc.params.max_optim_pose_its, 0,
                             orc.params.inlier_error_threshold / tc.CAM4[0], tc.CAM4[0])
    p.cell_size, p.patch_size, p.max_failed = tc.CELL, tc.PATCH, tc.MAX_FAILED
    assert orc.params.max_failed == tc.MAX_FAILED and orc.params.patch_size == tc.PATCH and orc.params.cell_size == tc.CELL
    assert orc.params.max_ransac_its == tc.MAX_RANSAC_ITS
    return p


def track_set(w, ctx, n, max_features=MAX_FEATURES):
    key = (n, max_features)
    if key not in w["sets"]:
        w["sets"][key] = ctx.track_set(n, MAX_POINTS, max_features, tc.N_CELLS, tc.MAX_MATCHES, tc.MAX_RANSAC_ITS)
    return w["sets"][key]


def cur_frame(w, ctx, view, slot, corners):
    """a frame of its own per job slot holding the view's image; corners = "set": the oracle's list set by hand once (no bins)"""
    key = (view, slot, corners)
    if key not in w["frames"]:
        f = ctx.frame(w["sc"]["img"][view])
        if corners == "set":
            f.set_corners(w["sc"]["corners"][view])
        w["frames"][key] = f
    return w["frames"][key]


def point_rows(sdvl, ref, rows):
    out = []
    for p in rows:
        r = p["rec"]
        t = sdvl.TrackPoint()
        t.position[:] = r["P"]
        t.px[:] = r["px"]
        t.bearing[:] = r["bearing"]
        t.idepth, t.idepth_std = r["idepth"], r["istd"]
        t.ref = ref.h.value
        t.level, t.fixed = r["level"], r["fixed"]
        t.score, t.n_failed, t.last_frame, t.status = p["score"], p["n_failed"], p["last_frame"], p["status"]
        t.desc[:] = [int(b) for b in r["desc"]]
        out.append(t)
    return out


def feature_rows(sdvl, rows):
    out = []
    for f in rows:
        t = sdvl.TrackFeature()
        t.px[:] = f["px"]
        t.bearing[:] = f["bearing"]
        t.level, t.point = f["level"], f["point"]
        out.append(t)
    return out


def draws(w, orc, seed):
    if seed not in w["draws"]:
        w["draws"][seed] = orc.rand_stream(tc.MAX_RANSAC_ITS, seed)
    return w["draws"][seed]


def plain_align(w, ctx, sdvl, case, cur, ap, points=None, features=None, last=None, T0=None, last_centre=(0.0, 0.0, 0.0)):
    """ctx.image_align on the AlignFeature records the table source stands for"""
    points = case.points if points is None else points
    features = case.features if features is None else features
    feats = (sdvl.AlignFeature * max(len(features), 1))()
    for a, f in zip(feats, features):
        a.px, a.py = f["px"]
        a.fx, a.fy, a.fz = f["bearing"]
        pt = -1 if f["point"] < 0 else f["point"] & (tr.DUPLICATE - 1)
        a.valid = int(pt >= 0 and not points[pt]["status"] & tr.DELETED)
        if a.valid:
            P = points[pt]["rec"]["P"]
            dx, dy, dz = P[0] - last_centre[0], P[1] - last_centre[1], P[2] - last_centre[2]
            a.depth = math.sqrt(dx * dx + dy * dy + dz * dz)
    T0 = w["sc"]["T0"][case.view] if T0 is None else T0
    return ctx.image_align([(w["frames"]["ref"] if last is None else last, cur, 0, len(features), T0)], feats, w["cam"], ap)[0]


def prepare(w, ctx, sdvl, orc, n_trackers, names, trackers, corners, max_features=MAX_FEATURES, upload=True):
    """the inputs of one step of a set of n_trackers: job j runs case names[j] on tracker trackers[j]; the tables are uploaded"""
    s = track_set(w, ctx, n_trackers, max_features)
    cases = [w["cases"][n] for n in names]
    ref = w["frames"]["ref"]
    if upload:
        s.upload(trackers, [0] * len(names), [point_rows(sdvl, ref, c.points) for c in cases], [feature_rows(sdvl, c.features) for c in cases])
    jobs = (sdvl.TrackJob * len(names))()
    curs = []
    for j, c in enumerate(cases):
        cur = cur_frame(w, ctx, c.view, j, corners)
        curs.append(cur)
        jobs[j].tracker, jobs[j].feat_buf = trackers[j], 0
        jobs[j].last, jobs[j].cur = ref.h.value, cur.h.value
        jobs[j].T[:] = w["sc"]["T0"][c.view] if c.T0 is None else c.T0
        jobs[j].last_pose[:] = tc.ID
        jobs[j].frame_id, jobs[j].max_matches = tc.FRAME_ID, c.max_matches
    rank = np.stack([c.rank() for c in cases])
    raw = np.stack([draws(w, orc, c.seed) for c in cases])
    return s, jobs, rank, raw, curs


def run(w, ctx, sdvl, orc, n_trackers, names, trackers, corners, max_features=MAX_FEATURES, between=None, max_its=0):
    """one step -> per job (result, features, stats, cur frame)"""
    s, jobs, rank, raw, curs = prepare(w, ctx, sdvl, orc, n_trackers, names, trackers, corners, max_features)

    def detect():
        if between is not None:
            between()
        if corners == "detect":
            ctx.detect_corners(curs, sdvl.default_detect_params(), orc.params.num_features)
    res, feats, stats = s.step(jobs, rank, raw, w["cam"], params(sdvl, orc, max_its), detect)
    return [(res[j], feats[j], stats[j], curs[j]) for j in range(len(names))]


def result_ints(r):
    return {n: getattr(r, n) for n in ("align_meas", "align_iters", "n_features", "n_requests", "matches", "attempts", "n_draws", "n_inliers",
                                       "n_outliers", "refined", "n_points", "n_deleted", "lk_iters", "n_corners", "status")}


def compare(w, ctx, sdvl, orc, case, got, label):
    """the device step of a controlled-pose case (alignment of max_its = 0 from the reference frame) against the restatement"""
    al = plain_align(w, ctx, sdvl, case, got[3], params(sdvl, orc, 0).align)
    assert tuple(al.T[:]) == w["sc"]["T0"][case.view], label           # max_its = 0: the alignment hands its start back
    out = compare_step(w, ctx, sdvl, orc, case, got, label, al)
    assert got[0].lk_iters == plain_lk_iterations(w, ctx, sdvl, orc, case, got[3], tuple(al.T[:])), label
    return out


def plain_lk_iterations(w, ctx, sdvl, orc, case, cur, T):
    """sdvl_track_result.lk_iters is no bookkeeping of the reference's but a count over ALL the step's requests (every candidate is
    searched, tried or not): the same requests through ctx.search_points"""
    sc = w["sc"]
    start = tr.se3_mul(T, tc.ID)
    points = [tr.Point(p["rec"]["P"], p["score"], p["n_failed"], p["last_frame"], p["status"]) for p in case.points]
    grid = tr.project_points(start, [tr.Feature(f["px"], f["level"], f["point"]) for f in case.features], points, tc.FRAME_ID, tc.CAM, tc.CELL,
                             tc.PATCH)
    cand = [e for cell in grid for e in cell]
    if not cand:
        return 0
    reqs = (sdvl.SearchReq * len(cand))()
    for r, (pt, px0) in zip(reqs, cand):
        rec = case.points[pt]["rec"]
        r.cur, r.ref = cur.h.value, w["frames"]["ref"].h.value
        r.cur_pose[:], r.ref_pose[:] = start, tc.ID
        r.px[:], r.bearing[:], r.px0[:] = rec["px"], rec["bearing"], px0
        r.idepth, r.idepth_std, r.level, r.fixed = rec["idepth"], rec["istd"], rec["level"], rec["fixed"]
        r.desc[:] = [int(b) for b in rec["desc"]]
    res = ctx.search_points(reqs, w["cam"], sdvl.default_search_params())
    for r, (pt, px0) in zip(res, cand):          # and what it finds is what the oracle finds
        assert bool(r.found) == tc.answer(sc, case.view, case.points[pt]["rec"])[0], (case.name, pt)
    return sum(r.lk_its for r in res)


def compare_step(w, ctx, sdvl, orc, case, got, label, al, view=None, search=None, points=None, features=None, last_pose=tc.ID,
                 frame_id=tc.FRAME_ID, same_form=True):
    """One job of a device step against track_restatement.step.  al: ctx.image_align's result on the records the tables stand for;
    view: the image the step tracked into; points / features: the restatement's rows before the step where they are not the case's"""
    res, feats, stats, cur = got
    sc = w["sc"]
    view = case.view if view is None else view
    print("%s: align error %r / %r, meas %d / %d, iters %d / %d" % (label, res.align_error, al.error, res.align_meas, al.n_meas, res.align_iters,
                                                                     al.iters_run))
    if same_form:
        assert (res.align_error, res.align_meas, res.align_iters) == (al.error, al.n_meas, al.iters_run), label
    else:       # the sums run in another order (see test_live_step_with_the_alignment_running): tests/test_gpu_parity.py's acceptance
        assert res.align_meas == al.n_meas and abs(res.align_iters - al.iters_run) <= 1, label
        assert abs(res.align_error - al.error) <= 1e-4 * max(1.0, abs(al.error)), label
    trace = Counter()
    n_rows = len(case.points) if points is None else len(points)
    want, new, rows, points = tc.restate(sc, case, T=tuple(al.T[:]), trace=trace, search=search, points=points, features=features,
                                         last_pose=last_pose, frame_id=frame_id)
    ints = result_ints(res)
    print("%s: %s" % (label, ints))
    for n in ("n_features", "n_requests", "matches", "attempts", "n_draws", "n_inliers", "n_outliers", "refined", "n_points", "n_deleted"):
        assert ints[n] == want[n], (label, n, ints[n], want[n])
    assert ints["status"] == 0 and ints["n_corners"] == len(sc["corners"][view]), label
    # the point statistics, row by row
    assert len(stats) == n_rows, label
    got_rows = [tuple(int(v) for v in s) for s in stats.tolist()]
    bad = [(i, g, r) for i, (g, r) in enumerate(zip(got_rows, rows)) if g != r]
    assert not bad, (label, bad[:5])
    # the new feature list, row by row: level and point equal, the position the oracle's bit for bit
    assert len(feats) == want["matches"] == len(new), label
    for i, (g, f) in enumerate(zip(feats, new)):
        assert (int(g["level"]), int(g["point"])) == (f.level, f.point), (label, i)
        assert tuple(g["px"].tolist()) == f.px, (label, i)
    # the pose: the oracle's within POSE_TOL; ctx.pose_from_matches' on the restated observations and the same draws bit for bit
    pose = np.array(res.pose[:])
    assert np.abs(pose - np.array(want["pose"])).max() <= POSE_TOL, label
    plain = ctx.pose_from_matches([(np.array(want["observations"]).reshape(-1, 6), want["start_pose"], draws(w, orc, case.seed))], fx=tc.CAM4[0],
                                  max_ransac_points=orc.params.max_ransac_points, max_ransac_its=orc.params.max_ransac_its,
                                  max_optim_pose_its=orc.params.max_optim_pose_its, inlier_error_threshold=orc.params.inlier_error_threshold)[0]
    if same_form:
        assert np.array_equal(pose, plain["pose"]), (label, pose, plain["pose"])
    else:       # the pose stage started from a pose that differs from the restated one in its last bits
        assert np.abs(pose - plain["pose"]).max() <= POSE_TOL, label
    assert (plain["n_draws"], plain["refined"], len(plain["inliers"]), len(plain["outliers"])) == (res.n_draws, res.refined, res.n_inliers, res.n_outliers)
    assert list(plain["outliers"]) == want["outliers"] and list(plain["inliers"]) == want["inliers"], label
    # the scene depth, restated from the pose the device returned
    depth, at = tr.scene_depth(tuple(pose.tolist()), new, points)
    if at < 0:
        assert res.scene_depth == 0.0, label
    else:
        P = points[new[at].point].P
        bound = 32 * 2.0 ** -52 * (math.sqrt(P[0] ** 2 + P[1] ** 2 + P[2] ** 2) + math.sqrt(sum(v * v for v in pose[4:])))
        print("%s: scene depth %r / %r (bound %.3g)" % (label, res.scene_depth, depth, bound))
        assert abs(res.scene_depth - depth) <= bound, (label, res.scene_depth, depth)
    w["compared"][case.name] += 1
    w["trace"].update(trace)
    return want, new, points


def as_bytes(got):
    res, feats, stats, _ = got
    return bytes(res), feats.tobytes(), stats.tobytes()


# ---- every case alone in a set of 3 (the pose stage in separate launches, the 256- or 512-thread projection); the current frame's
#      corners set by hand: no bins, the track_clear_bins path
@pytest.mark.parametrize("name", tc.SMALL + ("over-256",))
def test_case_alone_in_a_set_of_three(world, ctx, sdvl, orc, name):
    w = world
    got = run(w, ctx, sdvl, orc, 3, [name], [1], "set")[0]
    compare(w, ctx, sdvl, orc, w["cases"][name], got, name)
    w["alone"][name] = as_bytes(got)


def test_the_largest_feature_list_the_alignment_takes(world, ctx, sdvl, orc):
    """2048 feature rows, 100 of them with points: stride 2048, the 512-thread projection with 53 KB of dynamic LDS"""
    w = world
    got = run(w, ctx, sdvl, orc, 3, ["rows-2048"], [2], "set", max_features=2048)[0]
    compare(w, ctx, sdvl, orc, w["cases"]["rows-2048"], got, "rows-2048")


# ---- batching: the sets of 5 (fused pose stage, three waves) and 33 (one wave; the 128-thread projection), corners detected between
#      alignment and search (bins valid); jobs in another order than the trackers, fewer jobs than trackers
@pytest.mark.parametrize("n_trackers", [5, 33])
def test_every_tracker_of_a_larger_set_equals_the_case_alone(world, ctx, sdvl, orc, n_trackers):
    w = world
    missing = [n for n in tc.SMALL if n not in w["alone"]]
    for n in missing:          # (this test run on its own)
        w["alone"][n] = as_bytes(run(w, ctx, sdvl, orc, 3, [n], [1], "set")[0])
    rng = np.random.default_rng(n_trackers)
    n_jobs = n_trackers - 1                                     # fewer jobs than trackers
    for lo in range(0, len(tc.SMALL), n_jobs):
        names = [tc.SMALL[(lo + i) % len(tc.SMALL)] for i in range(n_jobs)]
        trackers = [int(t) for t in rng.permutation(n_trackers)[:n_jobs]]          # and not in tracker order
        assert trackers != sorted(trackers)
        got = run(w, ctx, sdvl, orc, n_trackers, names, trackers, "detect")
        for j, (n, g) in enumerate(zip(names, got)):
            label = "%s as job %d of %d on tracker %d" % (n, j, n_jobs, trackers[j])
            if lo + j < len(tc.SMALL):
                compare(w, ctx, sdvl, orc, w["cases"][n], g, label)
            a, b = as_bytes(g), w["alone"][n]
            assert a[1] == b[1] and a[2] == b[2], label       # feature list and point statistics
            assert a[0] == b[0], (label, result_ints(g[0]), g[0].align_error, g[0].scene_depth)


# ---- live: the alignment runs (default parameters, real motion from k = 0 to k = 4) on the table rows.
#      image_align_track_* and the plain entry point are one template over two feature sources, but not always in one form.  The plain
#      entry point precomputes with four waves and iterates with one wave for a job of up to 384 features, four beyond; the table
#      source uses four waves for both in a set of at most 32 trackers or beyond 384 features, one wave for both otherwise
#      (sdvl_image_align_track_enqueue).  The forms add the features up in different orders.  So: beyond 384 features ("live-wide")
#      the two run the same form in every set, and everything is bit-equal.  At 200 features ("live") they never do, and the
#      alignment's error differs in its last bits (measured: 0.00010410315885880751 in a set of 3, 0.0001041031588588104 in a set of
#      33, against 0.00010410315885880781); there the alignment is accepted as tests/test_gpu_parity.py accepts it and the pose, which
#      starts from it, within POSE_TOL.
@pytest.mark.parametrize("name,n_trackers,corners", [("live-wide", 3, "detect"), ("live-wide", 33, "set"), ("live", 3, "set"), ("live", 33, "detect")])
def test_live_step_with_the_alignment_running(world, ctx, sdvl, orc, name, n_trackers, corners):
    w = world
    sc, case = w["sc"], w["cases"][name]
    ap = sdvl.default_align_params()
    got = run(w, ctx, sdvl, orc, n_trackers, [name], [n_trackers - 2], corners, max_its=ap.max_its)[0]
    al = plain_align(w, ctx, sdvl, case, got[3], ap, T0=tc.ID)
    T = tuple(al.T[:])
    assert al.iters_run > 0 and al.n_meas > 100 and np.abs(np.array(T) - np.array(sc["T0"]["moved"])).max() < 5e-3      # it aligned the frames
    start = tr.se3_mul(T, tc.ID)

    def search(pt, px0):
        rec = case.points[pt]["rec"]
        return tc.answer(sc, "moved", rec, start=start, key=("live", T, rec["key"]))
    want, new, points = compare_step(w, ctx, sdvl, orc, case, got, "%s in a set of %d, corners %s" % (name, n_trackers, corners), al, search=search,
                                     same_form=len(case.features) > 384)
    assert want["matches"] >= 100 and want["attempts"] > want["matches"]


# ---- two steps in a row: the second reads the feature list the first wrote (the other buffer) and, appended between them, points
#      whose reference frame is the first step's current frame — registered by the kernels with its final pose, not by the test
def test_two_steps_in_a_row_with_points_appended_between(world, ctx, sdvl, orc):
    w = world
    sc, case = w["sc"], w["cases"]["step-one"]
    s = track_set(w, ctx, 3)
    got1 = run(w, ctx, sdvl, orc, 3, ["step-one"], [2], "detect")[0]
    want1, new1, points1 = compare(w, ctx, sdvl, orc, case, got1, "step one")
    pose1 = tuple(got1[0].pose[:])
    B, n0 = got1[3], len(points1)
    extra = tc.seed_on_view(sc, "moved", pose1, 6)
    state = dict(score=9, n_failed=0, status=tr.P_FOUND, last_frame=tc.FRAME_ID)      # the first tried in their cells
    s.append([2], [1], [point_rows(sdvl, B, [dict(state, rec=r) for r in extra])],
             [feature_rows(sdvl, [dict(px=r["px"], bearing=r["bearing"], level=r["level"], point=n0 + k) for k, r in enumerate(extra)])])
    # the second step: from B into a frame that holds the reference image again, alignment of max_its = 0 from the inverse motion
    two = tc.Case("step-two", "same", seed=62, order_seed=62)
    cur = cur_frame(w, ctx, "same", "second", "set")
    T0 = tuple(float(v) for v in orc.se3_inv(np.array(pose1)))
    jobs = (sdvl.TrackJob * 1)()
    jobs[0].tracker, jobs[0].feat_buf = 2, 1
    jobs[0].last, jobs[0].cur = B.h.value, cur.h.value
    jobs[0].T[:] = T0
    jobs[0].last_pose[:] = pose1
    jobs[0].frame_id, jobs[0].max_matches = tc.FRAME_ID + 1, two.max_matches
    res, feats, stats = s.step(jobs, two.rank()[None], draws(w, orc, two.seed)[None], w["cam"], params(sdvl, orc, 0))
    got2 = (res[0], feats[0], stats[0], cur)
    # its restatement starts from what the restatement of step one left
    recs = [p["rec"] for p in case.points] + extra
    points2 = points1 + [tr.Point(r["P"], 9, 0, tc.FRAME_ID, tr.P_FOUND) for r in extra]
    features2 = [tr.Feature(f.px, f.level, f.point) for f in new1] + [tr.Feature(r["px"], r["level"], n0 + k) for k, r in enumerate(extra)]
    start2 = tr.se3_mul(T0, pose1)

    def search(pt, px0):
        if pt < n0:
            return tc.answer(sc, "same", recs[pt], start=start2, key=("step-two", recs[pt]["key"]))
        return tc.answer(sc, "same", recs[pt], start=start2, ref_pose=pose1, ref_view="moved", key=("step-two", recs[pt]["key"]))
    centre = tuple(float(v) for v in orc.se3_inv(np.array(pose1))[4:])
    rows = [dict(rec=dict(P=p.P), status=p.status) for p in points2]
    frows = [dict(px=f.px, bearing=tr.unproject(tc.CAM, f.px), level=f.level, point=f.point) for f in features2]
    al = plain_align(w, ctx, sdvl, two, cur, params(sdvl, orc, 0).align, points=rows, features=frows, last=B, T0=T0, last_centre=centre)
    assert tuple(al.T[:]) == T0
    want2, new2, _ = compare_step(w, ctx, sdvl, orc, two, got2, "step two", al, search=search, points=points2, features=features2,
                                  last_pose=pose1, frame_id=tc.FRAME_ID + 1)
    assert want2["n_features"] == want1["matches"] + len(extra) and want2["n_requests"] >= want1["n_points"]
    hits = [f.point for f in new2 if f.point >= n0]
    assert len(hits) >= 3, hits            # appended points were found: their reference frame's pose in the registry is the final one


# ---- refusals: each returns its message and leaves the set usable (a good step afterwards gives what the case gives alone).  Only
#      inputs the API validates: nothing here reaches a kernel
def test_refusals_leave_the_set_usable(world, ctx, sdvl, orc):
    w = world
    good = "features-7"
    if good not in w["alone"]:
        w["alone"][good] = as_bytes(run(w, ctx, sdvl, orc, 3, [good], [1], "set")[0])
    case = w["cases"][good]
    ref = w["frames"]["ref"]
    P, F = point_rows(sdvl, ref, case.points), feature_rows(sdvl, case.features)
    prm = params(sdvl, orc, 0)

    def still_good(between=None):
        assert as_bytes(run(w, ctx, sdvl, orc, 3, [good], [1], "set", between=between)[0]) == w["alone"][good]

    s = track_set(w, ctx, 3)

    def upload_in_flight():
        with pytest.raises(sdvl.SdvlError, match="sdvl_track_upload while a step is in flight"):
            s.upload([0], [0], [P], [F])
        with pytest.raises(sdvl.SdvlError, match="sdvl_track_upload while a step is in flight"):
            s.append([0], [0], [P], [F])
    still_good(upload_in_flight)                  # the step the upload was refused in completes, untouched

    with pytest.raises(sdvl.SdvlError, match="a tracker is named twice in one upload"):
        s.upload([2, 2], [0, 0], [P, P], [F, F])
    still_good()
    with pytest.raises(sdvl.SdvlError, match="table larger than the set's capacity"):
        s.upload([2], [0], [P * (MAX_POINTS // len(P) + 1)], [F])
    with pytest.raises(sdvl.SdvlError, match="table larger than the set's capacity"):
        s.upload([2], [0], [P], [F * (MAX_FEATURES // len(F) + 1)])
    with pytest.raises(sdvl.SdvlError, match="bad tracker / buffer index"):
        s.upload([3], [0], [P], [F])
    still_good()
    outside = feature_rows(sdvl, case.features)
    outside[3].point = len(P)
    with pytest.raises(sdvl.SdvlError, match="feature names a point outside its tracker's table"):
        s.upload([2], [0], [P], [outside])
    outside[3].point = len(P) | sdvl.TRACK_DUPLICATE
    with pytest.raises(sdvl.SdvlError, match="feature names a point outside its tracker's table"):
        s.upload([2], [0], [P], [outside])
    still_good()

    # refusals of sdvl_track_align
    def refused(message, change):
        s_, jobs, rank, raw, curs = prepare(w, ctx, sdvl, orc, 3, [good, good], [1, 2], "set")
        cam = sdvl.Camera(tc.W, tc.H, *tc.CAM4)
        rank, raw = rank.copy(), raw.copy()
        change(jobs, rank, raw, cam)
        with pytest.raises(sdvl.SdvlError, match=message):
            s_.step(jobs, rank, raw, cam, prm)
        still_good()

    def twice(jobs, rank, raw, cam):
        jobs[1].tracker = 1
    refused("a tracker appears twice in one step", twice)

    def bad_rank(jobs, rank, raw, cam):
        rank[1, 17] = tc.N_CELLS
    refused("cell rank out of range", bad_rank)

    def other_grid(jobs, rank, raw, cam):
        cam.width = 672.0             # 21 x 15 cells
    refused("the set's grid does not match camera / cell size", other_grid)

    def too_many_matches(jobs, rank, raw, cam):
        jobs[0].max_matches = tc.MAX_MATCHES + 1
    refused("max_matches above the set's", too_many_matches)

    def negative_draw(jobs, rank, raw, cam):
        raw[0, 5] = -1
    refused(r"rand\(\) values are non-negative", negative_draw)

    def no_tracker(jobs, rank, raw, cam):
        jobs[0].tracker = 3
    refused("bad tracker / buffer index", no_tracker)


def test_more_features_than_the_alignment_takes(world, ctx, sdvl, orc):
    """A set may be created for up to 4096 features, and track_project has a form with more than 60 KB of dynamic LDS for strides beyond
    2360; the alignment that opens every step takes at most SDVL_MAX_ALIGN_FEATURES = 2048 features per job, so a table of 2400 rows is
    refused there and that form is never launched.  The refusal leaves the set usable."""
    w = world
    s = track_set(w, ctx, 3, 2400)
    case = w["cases"]["rows-2048"]
    ref = w["frames"]["ref"]
    feats = feature_rows(sdvl, case.features)
    feats = feats + feats[:352]
    assert len(feats) == 2400 and sum(1 for f in feats if f.point >= 0) <= 120
    s.upload([0], [0], [point_rows(sdvl, ref, case.points)], [feats])
    _, jobs, rank, raw, curs = prepare(w, ctx, sdvl, orc, 3, ["rows-2048"], [0], "set", max_features=2400, upload=False)
    with pytest.raises(sdvl.SdvlError, match="too many features in one alignment job"):
        s.step(jobs, rank, raw, w["cam"], params(sdvl, orc, 0))
    got = run(w, ctx, sdvl, orc, 3, ["features-9"], [0], "set", max_features=2400)[0]
    compare(w, ctx, sdvl, orc, w["cases"]["features-9"], got, "features-9 in the set of 2400")


def test_every_case_was_compared_and_every_branch_met(world):
    """last in the module: nothing above was skipped on the way, and the restatement's trace over what was compared on the device has
    been through every branch of tests/track_cases.py's list"""
    w = world
    names = set(w["cases"]) | {"step-two"}
    assert set(w["compared"]) == names, sorted(names - set(w["compared"]))
    missing = [b for b in tc.BRANCHES if not w["trace"][b]]
    assert not missing, missing
