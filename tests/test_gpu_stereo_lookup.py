"""sdvl_stereo_lookup (kernel stereo_lookup, csrc/sdvl_stereo.hip) and the depth filter fed by it (sdvl_depth_filter_stereo,
sdvl_search_run_filter_stereo: stereo_lookup over the search results, then the filter's third form, csrc/sdvl_depth_filter.hip) on the
MI355X against their specification tests/stereo_lookup_restatement.py, on the cases of tests/stereo_lookup_cases.py.

The lookup: statuses equal, disparities and depths bit-equal — the designed pairs at jittered positions, searched ranges of 3, 63, 64, 65,
128, 129 and 512 disparities (the lane rounds), levels 0 to 4 with centres off their level's grid, the centre rule (the half, negative and
non-finite positions, a window at each border), 0 positions and 1, two pairs with an empty job and unnamed positions in one call, the right
image in HBM, pinned and pageable.  sdvl_stereo_depth over the same corners still equals its own restatement.

The filter: outcomes, n_failed and status bytes exact; a float is held to the case's own bound (stereo_lookup_restatement.tolerance, the
scheme of depth_measure_restatement: exp moved by +-4 ulp, times 4, plus 8 ulp of the value); a request that does not measure equals
Context.depth_filter bit for bit.  Launches of 1, 127, 128 and 129 requests; rows patched in a tracking table; the fused entry against
search followed by the stated one; every refusal; the structures against the compiled header."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_restatement as dr
import stereo_cases as stc
import stereo_lookup_cases as slc
import stereo_lookup_restatement as sl
import stereo_restatement as sr
from depth_restatement import CONVERGED, DELETED, FIXED_STALE, NOT_FOUND, SKIPPED, UPDATED
from oraclelib import TUM_CAM
from track_restatement import TRASH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_T = np.dtype([("P", "<f8", 3), ("ipx", "<f8", 2), ("ibearing", "<f8", 3), ("idepth", "<f8"), ("idepth_std", "<f8"), ("ref", "<i4"), ("pad_", "<i4"),
                  ("ilevel", "<i4"), ("fixed", "<i4"), ("score", "<i4"), ("n_failed", "<i4"), ("last_frame", "<i4"), ("status", "<i4"), ("desc", "u1", 32)])
assert ROW_T.itemsize == 144
MAX_POINTS, N_TRACKERS = 6, 2
N_ROWS = MAX_POINTS * N_TRACKERS

CASES = slc.all_cases()
NAMES = [c["name"] for c in CASES]
_w = {"alone": {}, "ratio": {}, "pairs": {}}


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    if "set" in _w:
        _w.pop("set").close()
    if "frame" in _w:
        _w.pop("frame").close()
    for f, _ in _w["pairs"].values():
        f.close()
    _w["pairs"].clear()
    c.close()


def camera(sdvl, cam4, w, h):
    return sdvl.Camera(w, h, *[float(c) for c in cam4])


def check(got, want):
    """got: the entry's (z, disparity, status, ok); want: the restatement's (z, disparity, status, ok)"""
    z, disp, status, ok = got
    wz, wd, ws, wok = want
    bad = np.flatnonzero(status != ws)
    assert len(bad) == 0, (bad[:10], status[bad[:10]], ws[bad[:10]])
    assert np.array_equal(disp.view(np.uint64), wd.view(np.uint64)), np.abs(disp - wd).max()
    assert np.array_equal(z.view(np.uint64), wz.view(np.uint64)), np.abs(z - wz).max()
    assert list(ok) == list(wok)


def lookup_case(sdvl, ctx, c, px, lv):
    h, w = c["left"].shape
    left = ctx.frame(np.array(c["left"]), pyramid=False)
    right = np.array(c["right"])    # (a writable, pageable copy)
    try:
        return ctx.stereo_lookup([(left, right, 0, len(px))], px, lv, camera(sdvl, c["cam"], w, h), c["baseline"], **c["rule"])
    finally:
        left.close()


def restated(c, px, lv):
    return sl.stereo_lookup([(c["left"], c["right"], 0, len(px))], px, lv, c["cam"], c["baseline"], **c["rule"])


# ---------------------------------------------------------------------------------------------------- the lookup
@pytest.mark.parametrize("name", ["integer", "noise", "half", "constant", "constant1", "periodic", "outside", "edge", "dlo", "dlo_miss", "end0",
                                  "end1", "end2"])
def test_designed_cases_at_jittered_positions(sdvl, ctx, name):
    """within half a pixel of a corner: the lookup's restatement, and through it sdvl_stereo_depth's, bit for bit"""
    c = stc.designed_cases()[name]
    px, lv = slc.positions_of(c)
    got = lookup_case(sdvl, ctx, c, px, lv)
    if c["want"] is not None:
        assert np.array_equal(got[2], c["want"]), (got[2], c["want"])
    check(got, restated(c, px, lv))
    want = stc.restate(c)
    assert np.array_equal(got[2], want["status"]) and got[0].tobytes() == want["z"].tobytes() and got[1].tobytes() == want["disparity"].tobytes()
    assert ctx.lib.sdvl_ctx_health(ctx.h) == 0


@pytest.mark.parametrize("n_range", stc.RANGES)
def test_lane_rounds(sdvl, ctx, n_range):
    c = stc.range_case(n_range)
    px, lv = slc.positions_of(c)
    want = restated(c, px, lv)
    check(lookup_case(sdvl, ctx, c, px, lv), want)
    if n_range > 3:
        assert (want[2] == sr.OK).sum() >= 6


def test_centre_rule(sdvl, ctx):
    c, px, lv, want = slc.centre_cases()
    got = lookup_case(sdvl, ctx, c, px, lv)
    check(got, restated(c, px, lv))
    for i, w in enumerate(want):
        if isinstance(w, int):
            assert got[2][i] == w, (i, px[i], lv[i])


def test_levels_0_to_4_off_the_grid(sdvl, ctx, orc):
    """a `shelf` pair at 640 x 480: positions of levels 0 to 4 (a level-4 window is 129 pixels a side) whose centres are no multiples of
    their stride"""
    c, _ = stc.shelf_pair(orc, 13)
    rng = np.random.default_rng(slc.JITTER_SEED + 7)
    px, lv = [], []
    for l in range(5):
        s = 1 << l
        for _ in range(6):
            px.append((rng.uniform(4 * s + 200, 639 - 4 * s), rng.uniform(4 * s, 479 - 4 * s)))
            lv.append(l)
    px, lv = np.array(px), np.array(lv, np.int32)
    centres = np.floor(px + 0.5).astype(np.int64)
    assert ((centres[:, 0] % (1 << lv) != 0) & (lv > 0)).sum() >= 12
    want = restated(c, px, lv)
    assert (want[2] != sr.OUTSIDE).all() and (want[2][lv == 4] == sr.OK).any() and len(set(want[2])) >= 2
    check(lookup_case(sdvl, ctx, c, px, lv), want)


def test_no_position_and_one(sdvl, ctx):
    c = stc.designed_cases()["noise"]
    h, w = c["left"].shape
    left, right, cam = ctx.frame(np.array(c["left"]), pyramid=False), np.array(c["right"]), camera(sdvl, c["cam"], w, h)
    z, disp, status, ok = ctx.stereo_lookup([(left, right, 0, 0)], np.zeros((0, 2)), np.zeros(0, np.int32), cam, c["baseline"])
    assert len(z) == 0 and len(disp) == 0 and len(status) == 0 and list(ok) == [0]
    px, lv = slc.positions_of(c)
    check(ctx.stereo_lookup([(left, right, 0, 1)], px[17:18], lv[17:18], cam, c["baseline"]), restated(c, px[17:18], lv[17:18]))
    left.close()


def test_jobs_of_two_pairs_an_empty_one_and_unnamed_positions(sdvl, ctx):
    a, b = stc.designed_cases()["noise"], stc.designed_cases()["integer"]
    h, w = a["left"].shape
    pa, la = slc.positions_of(a)
    pb, lb = slc.positions_of(b)
    na, nb = 40, 30
    px = np.concatenate([pa[:na], pb[:2], pb[:nb], pa[:1]])
    lv = np.concatenate([la[:na], lb[:2], lb[:nb], la[:1]])
    fa, fb_ = ctx.frame(np.array(a["left"]), pyramid=False), ctx.frame(np.array(b["left"]), pyramid=False)
    ra, rb = np.array(a["right"]), np.array(b["right"])
    got = ctx.stereo_lookup([(fa, ra, 0, na), (fb_, rb, na + 2, na + 2), (fb_, rb, na + 2, na + 2 + nb)], px, lv, camera(sdvl, TUM_CAM, w, h), stc.BASELINE)
    want = sl.stereo_lookup([(a["left"], a["right"], 0, na), (b["left"], b["right"], na + 2, na + 2), (b["left"], b["right"], na + 2, na + 2 + nb)], px, lv,
                            TUM_CAM, stc.BASELINE)
    check(got, want)
    assert list(got[2][na:na + 2]) == [sr.NOMATCH] * 2 and got[2][-1] == sr.NOMATCH and list(got[3]) == [na, 0, nb]
    fa.close(); fb_.close()


def test_sources_and_the_existing_entry(sdvl, ctx, orc):
    """one `shelf` pair at 640 x 480 at positions displaced below the stride, its right image in HBM, pinned and pageable: three calls,
    one answer, the restatement's.  sdvl_stereo_depth over the pair's corners still equals ITS restatement, and the lookup at the corners
    themselves gives its bytes"""
    import torch
    c, _, px, lv, _ = slc.shelf_jittered(orc, 13)
    want = restated(c, px, lv)
    assert (want[2] == sr.OK).sum() >= 150
    h, w = c["left"].shape
    left, cam, n = ctx.frame(np.array(c["left"]), pyramid=False), camera(sdvl, c["cam"], w, h), len(px)
    right = np.array(c["right"])
    first = None
    for where in ("hbm", "pinned", "pageable"):
        keep = None
        if where == "hbm":
            keep = torch.from_numpy(right).cuda()
            ptr = keep.data_ptr()
        elif where == "pinned":
            keep = torch.from_numpy(right).pin_memory()
            ptr = keep.data_ptr()
        else:
            ptr = right.ctypes.data
        got = ctx.stereo_lookup([sdvl.StereoJob(left.h, ptr, 1 if where == "hbm" else 0, w, 0, n)], px, lv, cam, c["baseline"])
        check(got, want)
        first = first or got
        for x, y in zip(got, first):
            assert x.tobytes() == y.tobytes(), where
        assert ctx.lib.sdvl_ctx_health(ctx.h) == 0
        del keep
    corners = ctx.stereo_depth([(left, right, 0, n)], c["xyl"], cam, c["baseline"])
    ref = stc.restate(c)
    assert np.array_equal(corners[2], ref["status"]) and corners[0].tobytes() == ref["z"].tobytes() and corners[1].tobytes() == ref["disparity"].tobytes()
    s = (1 << c["xyl"][:, 2]).astype(np.float64)
    at = ctx.stereo_lookup([(left, right, 0, n)], np.stack([c["xyl"][:, 0] * s, c["xyl"][:, 1] * s], 1), c["xyl"][:, 2], cam, c["baseline"])
    for x, y in zip(at, corners):
        assert x.tobytes() == y.tobytes()
    left.close()


# ---------------------------------------------------------------------------------------------------- the filter
def cam_of(sdvl, cam):
    return sdvl.Camera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["u0"], cam["v0"])


def filter_params(sdvl, p):
    fp = sdvl.DepthParams()
    fp.px_error_angle, fp.min_depth, fp.scale_min_dist, fp.max_failed = p["px_error_angle"], p["min_depth"], p["scale_min_dist"], p["max_failed"]
    return fp


def states_of(sdvl, cases, track_rows=None):
    states = (sdvl.DepthState * len(cases))()
    for i, c in enumerate(cases):
        s, st = states[i], c["state"]
        s.rho, s.sigma2, s.a, s.b, s.z_range = st["rho"], st["sigma2"], st["a"], st["b"], st["z_range"]
        s.cos_alpha, s.last_distance, s.depth_mean = st["cos_alpha"], st["last_distance"], st["depth_mean"]
        s.position[:] = st["position"]
        s.fixed, s.n_failed = st["fixed"], st["n_failed"]
        s.track_row = -1 if track_rows is None else track_rows[i]
    return states


def pair_on_device(ctx, name):
    """-> (left Frame, right image: a pageable array the call stages)"""
    if name not in _w["pairs"]:
        left, right = slc.pair(name)
        _w["pairs"][name] = (ctx.frame(np.array(left), pyramid=False), np.array(right))
    return _w["pairs"][name]


def call_key(c):
    return (c["group"], c["disparity_sigma"], tuple(sorted(c["rule"].items())), tuple(sorted(c["params"].items())))


def launch(ctx, sdvl, cases, track_rows=None, track_set=None):
    """the cases (of one group) as one call of sdvl_depth_filter_stereo, one job per request that has a pair"""
    assert len({call_key(c) for c in cases}) == 1
    c0 = cases[0]
    jobs = []
    for i, c in enumerate(cases):
        if c["pair"] is not None:
            f, r = pair_on_device(ctx, c["pair"])
            jobs.append(sdvl.StereoJob(f.h, r.ctypes.data, 0, r.strides[0], i, i + 1))
    return ctx.depth_filter_stereo([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases],
                                   [1 if c["found"] else 0 for c in cases], [c["px"] for c in cases], [c["level"] for c in cases], cam_of(sdvl, c0["cam"]),
                                   states_of(sdvl, cases, track_rows), filter_params(sdvl, c0["params"]), jobs, c0["baseline"], c0["disparity_sigma"], None,
                                   track_set, **c0["rule"])


def triangulated(ctx, sdvl, cases, track_rows=None, track_set=None):
    c0 = cases[0]
    return ctx.depth_filter([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases],
                            [1 if c["found"] else 0 for c in cases], [c["px"] for c in cases], cam_of(sdvl, c0["cam"]), states_of(sdvl, cases, track_rows),
                            filter_params(sdvl, c0["params"]), track_set)


def as_result(o, status):
    told = o.outcome in (UPDATED, CONVERGED, FIXED_STALE)
    return dict(outcome=o.outcome, n_failed=o.n_failed, rho=o.rho, sigma2=o.sigma2, a=o.a, b=o.b, cos_alpha=o.cos_alpha if told else None,
                last_distance=o.last_distance if told else None, position=tuple(o.position) if told else None, row={}, status=int(status))


def alone(ctx, sdvl, name):
    if name not in _w["alone"]:
        fout, status = launch(ctx, sdvl, [slc.by_name(name)])
        _w["alone"][name] = (bytes(fout[0]), int(status[0]))
    return _w["alone"][name]


@pytest.mark.parametrize("name", NAMES)
def test_case_alone(ctx, sdvl, name):
    """a launch of one request"""
    c = slc.by_name(name)
    raw, status = alone(ctx, sdvl, name)
    o = sdvl.DepthOut.from_buffer_copy(raw)
    got = as_result(o, status)
    want, bound = slc.expected(c)
    bad, ratio = slc.differences(c, got, with_row=False)
    for k, r in sorted(ratio.items()):
        print("%s %s: device %r restatement %r ratio %.3g" % (name, k, dr._numbers(got)[k], dr._numbers(want)[k], r))
        key = "position" if k.startswith("position") else k
        if r >= _w["ratio"].get(key, (-1.0, None))[0]:
            _w["ratio"][key] = (r, name)
    assert not bad, (name, c["purpose"], bad)
    if status != sr.OK:
        assert raw == bytes(triangulated(ctx, sdvl, [c])[0]), name      # not measured: the triangulated filter's answer, bit for bit
    if want["outcome"] in (NOT_FOUND, NOT_FOUND | DELETED, SKIPPED):
        st = c["state"]
        assert (o.rho, o.sigma2, o.a, o.b) == (st["rho"], st["sigma2"], st["a"], st["b"] + (0.0 if c["found"] else 1.0))
    if c["state"]["fixed"] and want["position"] is not None:
        assert tuple(o.position) == c["state"]["position"]
    if c["want"].get("exact_range") and want["outcome"] in (UPDATED, CONVERGED):
        r0, r1, truth = c["state"]["rho"], o.rho, 1.0 / c["range"]
        assert min(r0, truth) - 1e-12 <= r1 <= max(r0, truth) + 1e-12, (r0, r1, truth)


@pytest.mark.parametrize("n", [127, 128, 129])
def test_plain_cases_in_one_launch(ctx, sdvl, n):
    """the filter's workgroup is 128 lanes behind an `i >= n` guard, the lookup one wave per request: misses, hits in no job, OK and every
    status that is not, in one launch of n requests in an order that changes with n, give the bits and the status they give alone"""
    usual = slc.groups()["plain"]
    assert len(usual) >= 20 and len(usual) % 7
    order = [usual[(7 * i + n) % len(usual)] for i in range(n)]
    assert {c["name"] for c in order} == {c["name"] for c in usual}
    fout, status = launch(ctx, sdvl, order)
    for i, c in enumerate(order):
        assert (bytes(fout[i]), int(status[i])) == alone(ctx, sdvl, c["name"]), (n, i, c["name"])
    assert set(int(s) for s in status) == {sr.OK, sr.NOMATCH, sr.AMBIGUOUS, sr.EDGE, sr.OUTSIDE, sl.NO_LOOKUP}
    tri = triangulated(ctx, sdvl, order)
    not_ok = [i for i in range(n) if status[i] != sr.OK]
    assert len(not_ok) >= n // 3 and len(not_ok) < n
    for i in not_ok:
        assert bytes(fout[i]) == bytes(tri[i]), (n, i, order[i]["name"])
    assert any(bytes(fout[i]) != bytes(tri[i]) for i in range(n) if status[i] == sr.OK)


@pytest.mark.parametrize("group", sorted(g for g in slc.groups() if g != "plain"))
def test_other_groups_in_one_launch(ctx, sdvl, group):
    cases = slc.groups()[group]
    fout, status = launch(ctx, sdvl, cases)
    for i, c in enumerate(cases):
        assert (bytes(fout[i]), int(status[i])) == alone(ctx, sdvl, c["name"]), (group, c["name"])


def test_one_job_for_a_range_of_requests(ctx, sdvl):
    """a job names a RANGE of requests: three on one pair, one before and one behind them on none; and no job at all"""
    names = ("no-job", "ok-00-integer-level0", "ok-03-integer-level1", "skip-depth_mean", "no-job-level3")
    cases = [slc.by_name(n) for n in names]
    f, r = pair_on_device(ctx, "integer")
    args = ([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases], [1] * 5, [c["px"] for c in cases],
            [c["level"] for c in cases], cam_of(sdvl, slc.CAM), states_of(sdvl, cases), filter_params(sdvl, slc.PARAMS))
    fout, status = ctx.depth_filter_stereo(*args, [(f, r, 1, 4)], stc.BASELINE, slc.SIGMA)
    for i, n in enumerate(names):
        assert (bytes(fout[i]), int(status[i])) == alone(ctx, sdvl, n), n
    fout, status = ctx.depth_filter_stereo(*args, [], stc.BASELINE, slc.SIGMA)
    assert list(status) == [255] * 5 and bytes(fout) == bytes(triangulated(ctx, sdvl, cases))


# ---------------------------------------------------------------------------------------------------- the row patch
def table(ctx, sdvl):
    if "set" not in _w:
        _w["frame"] = ctx.frame(np.zeros((480, 640), np.uint8))
        ctx.register([_w["frame"]], [(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)])
        _w["set"] = ctx.track_set(N_TRACKERS, MAX_POINTS, 8, 300, 8, 100)
    rows = []
    for t in range(N_TRACKERS):
        rows.append([])
        for k in range(MAX_POINTS):
            p = sdvl.TrackPoint()
            r = t * MAX_POINTS + k
            p.position[:] = (0.5 + r, -1.5 - r, 2.0 + 0.25 * r)
            p.px[:] = (100.0 + r, 200.0 - r)
            p.bearing[:] = dr.unproject(slc.CAM, (10.0 + r, 12.0 - r))
            p.idepth, p.idepth_std = 0.4 + 0.01 * r, 0.05 + 0.001 * r
            p.ref = _w["frame"].h.value
            p.level, p.fixed, p.score, p.n_failed, p.last_frame, p.status = r % 3, 0, 10 + r, 5 + r % 4, 7, r % 4
            p.desc[:] = [(r * 17 + j) % 256 for j in range(32)]
            rows[-1].append(p)
    _w["set"].upload(list(range(N_TRACKERS)), [0] * N_TRACKERS, rows, [[] for _ in range(N_TRACKERS)])
    return _w["set"]


def rows_of(ctx, s):
    return ctx.track_points_download(s).copy().view(ROW_T).reshape(-1)


ROW_LAUNCHES = [
    ("ok-00-integer-level0", "ok-converges", "skip-depth_mean", "ok-01-integer-level0"),      # measured: updated, converged, skipped
    ("miss-n_failed-3", "miss-n_failed-15", "ok-fixed", "ok-converges"),                      # kept miss, deleted miss, a fixed point
    ("nomatch-constant", "edge", "no-job", "ok-05-noise-level3"),                             # the triangulated update behind a status, and without a pair
]


@pytest.mark.parametrize("k", range(len(ROW_LAUNCHES)))
def test_row_patch(ctx, sdvl, k):
    """rows 0, MAX_POINTS (tracker 1, index 0) and the last row are named by three requests, a fourth has none: the named rows change as
    the restatement says and hold what the same lane returned; every other row keeps its bytes"""
    s = table(ctx, sdvl)
    named = (0, MAX_POINTS, N_ROWS - 1)
    cases = [slc.by_name(n) for n in ROW_LAUNCHES[k]]
    before = rows_of(ctx, s)
    fout, status = launch(ctx, sdvl, cases, track_rows=list(named) + [-1], track_set=s)
    after = rows_of(ctx, s)
    for i, c in enumerate(cases):
        assert (bytes(fout[i]), int(status[i])) == alone(ctx, sdvl, c["name"])
    for r in range(N_ROWS):
        if r not in named:
            assert after[r].tobytes() == before[r].tobytes(), (k, r)
            continue
        c, o = cases[named.index(r)], fout[named.index(r)]
        want, bound = slc.expected(c)
        patch = want["row"]
        expect = np.array([before[r]], ROW_T)
        for key in ("n_failed", "fixed"):
            if key in patch:
                expect[key][0] = patch[key]
        if patch.get("trash"):
            expect["status"][0] = before[r]["status"] | TRASH
        for key in ("P", "idepth", "idepth_std"):
            if key in patch:
                expect[key][0] = after[r][key]
        assert after[r].tobytes() == expect.tobytes(), (k, r, c["name"], after[r], expect)
        if "P" in patch:
            assert tuple(after[r]["P"]) == tuple(o.position)
            for i in range(3):
                assert abs(after[r]["P"][i] - patch["P"][i]) <= bound["row.P%d" % i]
        if "idepth" in patch:
            assert after[r]["idepth"] == o.rho and abs(after[r]["idepth"] - patch["idepth"]) <= bound["row.idepth"]
            assert abs(after[r]["idepth_std"] - patch["idepth_std"]) <= bound["row.idepth_std"]
    if k == 2:
        table(ctx, sdvl)
        triangulated(ctx, sdvl, cases[:3], track_rows=list(named), track_set=s)
        tri = rows_of(ctx, s)
        for r in named:
            assert tri[r].tobytes() == after[r].tobytes(), r


# ---------------------------------------------------------------------------------------------------- behind the search
def test_search_run_filter_stereo_equals_search_then_filter(ctx, sdvl, orc, synth):
    """candidate requests through sdvl_search_run_filter_stereo, and through sdvl_search_points followed by sdvl_depth_filter_stereo on its
    results (pixel and level): the same kernels on the same records, so outcomes and status bytes are equal bit for bit.  The right image
    is the plane seen from 0.11 m to the right, so most hits measure; the second half of the requests is in no job"""
    from oraclelib import fill_search_reqs, search_request_meta, trajectory_pose
    k_cur = 30
    T_ref, T_cur = trajectory_pose(orc, 0), trajectory_pose(orc, k_cur)
    img_ref, img_cur = (synth.render(T, TUM_CAM, 640, 480, frame_id=k) for T, k in ((T_ref, 0), (T_cur, k_cur)))
    img_right = synth.render(stc.right_pose(T_cur, stc.BASELINE), TUM_CAM, 640, 480, frame_id=k_cur)
    meta, ccur = search_request_meta(orc, img_ref, img_cur, T_ref, T_cur, TUM_CAM, 200, 47, False, 0.05)
    f_ref, f_cur = ctx.frame(img_ref), ctx.frame(img_cur)
    f_cur.set_corners(ccur)
    reqs = fill_search_reqs(sdvl, meta, f_ref, f_cur, T_ref, T_cur, False)
    n = len(reqs)
    states = (sdvl.DepthState * n)()
    for i, m in enumerate(meta):
        st = states[i]
        st.rho, st.sigma2, st.a, st.b, st.z_range = m["idepth"], m["istd"] ** 2, 10.0 + i % 5, 10.0 + i % 7, 6.0
        st.cos_alpha, st.last_distance, st.depth_mean = 1.0, 1.0 / m["idepth"], 2.0
        st.position[:] = (0.1, 0.2, 2.0)
        st.fixed, st.n_failed, st.track_row = int(i % 11 == 3), i % 17, -1
    cam = sdvl.Camera(640.0, 480.0, *[float(v) for v in TUM_CAM])
    fp, sp = filter_params(sdvl, dict(px_error_angle=dr.pixel_error_angle(TUM_CAM[0]), min_depth=0.25, scale_min_dist=0.25, max_failed=15)), sdvl.default_search_params()
    half = n // 2
    right = np.array(img_right)
    jobs = [(f_cur, right, 0, half)]
    res, fout, status = ctx.search_points_filter_stereo(reqs, cam, sp, states, fp, jobs, stc.BASELINE, slc.SIGMA)
    plain = ctx.search_points(reqs, cam, sp)
    assert [(r.found, tuple(r.px), r.level) for r in plain] == [(r.found, tuple(r.px), r.level) for r in res]
    got, gstatus = ctx.depth_filter_stereo([T_cur] * n, [T_ref] * n, [m["bearing"] for m in meta], [r.found for r in plain], [tuple(r.px) for r in plain],
                                           [r.level if r.found else 0 for r in plain], cam, states, fp, jobs, stc.BASELINE, slc.SIGMA)
    assert bytes(got) == bytes(fout) and np.array_equal(gstatus, status)
    counts = np.bincount(status, minlength=256)
    print("status counts OK %d NOMATCH %d AMBIGUOUS %d EDGE %d OUTSIDE %d none %d" % tuple(counts[[0, 1, 2, 3, 4, 255]]))
    assert counts[sr.OK] >= 10 and counts[255] >= half, counts[[0, 1, 2, 3, 4, 255]]
    assert all(status[i] == 255 for i in range(n) if i >= half or not res[i].found)
    # the lookup entry at the found pixels says the same of the first half's hits
    hits = [i for i in range(half) if res[i].found]
    z, disp, st_l, _ = ctx.stereo_lookup([(f_cur, right, 0, len(hits))], [tuple(res[i].px) for i in hits], [res[i].level for i in hits], cam, stc.BASELINE)
    assert [int(s) for s in st_l] == [int(status[i]) for i in hits]
    # not measured: the triangulated search + filter, bit for bit; measured: not
    _, tri = ctx.search_points_filter(reqs, cam, sp, states, fp)
    for i in range(n):
        if status[i] != sr.OK:
            assert bytes(fout[i]) == bytes(tri[i]), i
    assert any(bytes(fout[i]) != bytes(tri[i]) for i in range(n) if status[i] == sr.OK)
    f_ref.close(); f_cur.close()


# ---------------------------------------------------------------------------------------------------- plumbing
def test_lookup_refusals(sdvl, ctx):
    """every refusal returns SDVL_ERR_INVALID with a message and leaves the context healthy"""
    lib = ctx.lib
    w, h = stc.W, stc.H
    limg = stc.ramp()
    rimg = np.array(stc.shifted(limg, 7))
    left = ctx.frame(np.array(limg), pyramid=False)
    other = sdvl.Context(0)
    foreign = other.frame(np.array(limg), pyramid=False)
    px, lv = np.array([[80.2, 60.3], [80.4, 59.8]]), np.array([0, 1], np.int32)
    cam = camera(sdvl, TUM_CAM, w, h)
    z, disp, status, ok = np.zeros(2), np.zeros(2), np.zeros(2, np.uint8), np.zeros(2, np.int32)
    lib.sdvl_stereo_lookup.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    lens = sdvl.Distortion((C.c_double * 5)(0.1, 0, 0, 0, 0))

    def call(job=None, rule=None, null=None, lv_=lv, n_jobs=1, second=None, n=2):
        j = dict(left=left.h, right=rimg.ctypes.data, on_device=0, stride=w, c_begin=0, c_end=2)
        j.update(job or {})
        jobs = (sdvl.StereoJob * 2)(sdvl.StereoJob(**j), sdvl.StereoJob(**dict(j, **(second or {}))))
        r = dict(baseline=0.11)
        r.update(rule or {})
        p = sdvl.StereoParams(**r)
        lvc = np.ascontiguousarray(lv_, np.int32)
        args = dict(jobs=C.addressof(jobs), px=px.ctypes.data, lv=lvc.ctypes.data, cam=C.addressof(cam), p=C.addressof(p), z=z.ctypes.data,
                    disp=disp.ctypes.data, status=status.ctypes.data, ok=ok.ctypes.data)
        if null:
            args[null] = None
        rc = lib.sdvl_stereo_lookup(ctx.h, n_jobs, args["jobs"], n, args["px"], args["lv"], args["cam"], args["p"], args["z"], args["disp"],
                                    args["status"], args["ok"])
        return rc, lib.sdvl_last_error(ctx.h).decode()

    assert call()[0] == 0 and list(status) == [0, 0] and list(disp) == [7.0, 7.0]
    refused = [(dict(null="jobs"), "null pointer"), (dict(null="px"), "null pointer"), (dict(null="lv"), "null pointer"), (dict(null="cam"), "null pointer"),
               (dict(null="p"), "null parameters"), (dict(null="z"), "null pointer"), (dict(null="disp"), "null pointer"), (dict(null="status"), "null pointer"),
               (dict(null="ok"), "null pointer"), (dict(job=dict(left=None)), "null image"), (dict(job=dict(right=None)), "null image"),
               (dict(rule=dict(baseline=0.0)), "baseline"), (dict(rule=dict(baseline=float("nan"))), "baseline"), (dict(rule=dict(baseline=float("inf"))), "baseline"),
               (dict(rule=dict(max_disparity=512)), "max_disparity"), (dict(rule=dict(uniqueness=101)), "uniqueness"), (dict(rule=dict(max_sad=256)), "max_sad"),
               (dict(rule=dict(min_depth=-0.1)), "min_depth"), (dict(rule=dict(max_depth=float("nan"))), "max_depth"),
               (dict(job=dict(stride=w - 1)), "stride smaller"),
               (dict(lv_=[0, 5]), "level lies outside the left frame's pyramid"), (dict(lv_=[-1, 0]), "level lies outside the left frame's pyramid"),
               (dict(job=dict(c_begin=2, c_end=1)), "range outside"), (dict(job=dict(c_end=3)), "range outside"), (dict(job=dict(c_begin=-1)), "range outside"),
               (dict(n_jobs=2, second=dict(c_begin=1, c_end=2)), "ranges overlap"),
               (dict(job=dict(left=foreign.h)), "another context"),
               (dict(rule=dict(dist=C.addressof(lens))), "a lens"),
               (dict(n=-1), "negative count")]
    for kw, word in refused:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("sdvl_stereo_lookup:") and word in msg, (kw, rc, msg)
        assert lib.sdvl_ctx_health(ctx.h) == 0
    assert call(n_jobs=0)[0] == 0 and call(n=0, job=dict(c_end=0))[0] == 0      # nothing to do
    assert call(lv_=[0, 5], job=dict(c_end=1))[0] == 0                           # the level of a position no job names is not looked at
    assert status[1] == sr.NOMATCH
    assert call()[0] == 0 and list(status) == [0, 0] and list(z) == [TUM_CAM[0] * 0.11 / 7.0] * 2
    foreign.close()
    other.close()
    left.close()


def test_filter_refusals(ctx, sdvl):
    """a sigma that is negative or not finite, a bad rule or job, a level outside the pyramid: refused with a message, nothing patched"""
    c = slc.by_name("ok-00-integer-level0")
    f, r = pair_on_device(ctx, "integer")
    s = table(ctx, sdvl)
    before = rows_of(ctx, s)

    def call(job=None, level=0, baseline=stc.BASELINE, sigma=slc.SIGMA, found=1, **rule):
        j = dict(left=f.h, right=r.ctypes.data, on_device=0, stride=slc.W, c_begin=0, c_end=1)
        j.update(job or {})
        return ctx.depth_filter_stereo([c["cur_pose"]], [c["ref_pose"]], [c["bearing"]], [found], [c["px"]], [level], cam_of(sdvl, slc.CAM),
                                       states_of(sdvl, [c], [0]), filter_params(sdvl, slc.PARAMS), [sdvl.StereoJob(**j)], baseline, sigma, rule.pop("dist", None), s,
                                       **rule)

    for kw, msg in ((dict(sigma=-0.1), "disparity_sigma"), (dict(sigma=float("nan")), "disparity_sigma"), (dict(sigma=float("inf")), "disparity_sigma"),
                    (dict(baseline=0.0), "baseline"), (dict(baseline=float("nan")), "baseline"),
                    (dict(max_disparity=512), "max_disparity"), (dict(uniqueness=101), "uniqueness"), (dict(max_sad=256), "max_sad"),
                    (dict(min_depth=-1.0), "min_depth"), (dict(dist=(0.1, 0, 0, 0, 0)), "a lens"),
                    (dict(job=dict(stride=slc.W - 1)), "stride smaller"), (dict(job=dict(left=None)), "null image"), (dict(job=dict(right=None)), "null image"),
                    (dict(job=dict(c_end=2)), "range outside"), (dict(job=dict(c_begin=-1)), "range outside"), (dict(job=dict(c_begin=1, c_end=0)), "range outside"),
                    (dict(level=8), "level outside"), (dict(level=-1), "level outside"), (dict(level=5), "outside the left frame's pyramid")):
        with pytest.raises(sdvl.SdvlError, match=msg) as e:
            call(**kw)
        assert "sdvl_depth_filter_stereo" in str(e.value), str(e.value)
        assert ctx.lib.sdvl_ctx_health(ctx.h) == 0
    assert rows_of(ctx, s).tobytes() == before.tobytes()
    call(level=5, found=0)                                   # a miss's level is not looked at
    table(ctx, sdvl)
    fout, status = call()
    assert int(status[0]) == sr.OK and rows_of(ctx, s)[0]["idepth"] == fout[0].rho
    fout, status = ctx.depth_filter_stereo(np.zeros((0, 7)), np.zeros((0, 7)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0, np.int32),
                                           cam_of(sdvl, slc.CAM), (sdvl.DepthState * 0)(), filter_params(sdvl, slc.PARAMS), [], stc.BASELINE)
    assert len(status) == 0


def test_struct_sizes_match_the_compiled_header(sdvl, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "sdvl_hip.h"', 'int main() {',
           '  printf("%zu %zu %zu %zu %zu\\n", sizeof(sdvl_stereo_measure_params), offsetof(sdvl_stereo_measure_params, rule), '
           'offsetof(sdvl_stereo_measure_params, disparity_sigma), sizeof(sdvl_stereo_params), sizeof(sdvl_stereo_job));',
           '  printf("%g\\n", (double)SDVL_STEREO_DISPARITY_SIGMA);', '  return 0;', '}']
    path = tmp_path / "stereo_measure_abi.cc"
    path.write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "stereo_measure_abi")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(path), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    P = sdvl.StereoMeasureParams
    assert [int(v) for v in out[:5]] == [C.sizeof(P), P.rule.offset, P.disparity_sigma.offset, C.sizeof(sdvl.StereoParams), C.sizeof(sdvl.StereoJob)] == [56, 0, 48, 48, 32]
    assert float(out[5]) == sl.DISPARITY_SIGMA == 0.25


def test_largest_ratios():
    """not a check of its own: prints, per output, the largest |device - restatement| / bound test_case_alone met"""
    print()
    for k, (r, name) in sorted(_w["ratio"].items()):
        print("device vs restatement, %-13s largest deviation / bound %.3g (%s)" % (k, r, name))
    assert all(r <= 1.0 for r, _ in _w["ratio"].values())
