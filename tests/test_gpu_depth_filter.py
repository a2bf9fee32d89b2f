"""depth_filter_kernel (csrc/sdvl_depth_filter.hip) alone, through sdvl_depth_filter, against the pure-Python restatement of
Map::UpdateCandidates' loop body (tests/depth_restatement.py) on the named cases of tests/depth_cases.py: misses around max_failed,
det, cos_alpha, the two depth tests and l on both sides of their thresholds, negative tau, the clamp, regular updates over the range of
states a candidate passes through (sigma2 down to 1e-9, a + b up to 600), the early return of Point::Update, a sequence of twelve
updates; and the kernel's writes into the tracking tables, which no test had read back.

Decisions, n_failed and the row's integer fields are exact.  A float is held to the case's own bound for that output
(depth_restatement.tolerance): 4 times the restatement's largest movement when each acos / sin / exp result is moved by +-4 ulp, plus
8 ulp of the value; an output with no transcendental behind it keeps the 8 ulp alone.  The 4 ulp are an assumption (see tolerance()).

Measured on an MI355X, 2026-10-20 (test_largest_ratios prints the figures, run with -s): 51 of the 53 cases come back bit-equal to
the restatement; sequence-01 and sequence-04 do not, and give the largest |device - restatement| / bound per output: a 0.12, b 0.11,
rho 0.07, sigma2 0.05 (3.8e-13 relative), cos_alpha 0.06, last_distance 0.10, position 0.13.  Against libraries built with one scratch
change to the kernel each, these tests fail: `>=` in the deletion test: test_case_alone[miss-n_failed-14], test_row_patch[2];
`depth <= min_depth`: test_case_alone[too-close-min_depth-equal]; the row's idepth_std without the root: test_row_patch[1-3]; the row's
fixed set by every update: test_row_patch[1], [3]; cur * ref^-1 given to ComputeTau: 40 cases of test_case_alone, the sequence,
test_row_patch[1-3]; an exact pi: 36 cases of test_case_alone, test_row_patch[1-3]."""
import importlib
import math

import numpy as np
import pytest

import depth_cases as dc
import depth_restatement as dr
from depth_restatement import CONVERGED, DELETED, FIXED_STALE, NOT_FOUND, SKIPPED, UPDATED
from track_restatement import TRASH

pytestmark = pytest.mark.gpu

CASES = dc.all_cases()
NAMES = [c["name"] for c in CASES]
ROW_T = np.dtype([("P", "<f8", 3), ("ipx", "<f8", 2), ("ibearing", "<f8", 3), ("idepth", "<f8"), ("idepth_std", "<f8"), ("ref", "<i4"), ("pad_", "<i4"),
                  ("ilevel", "<i4"), ("fixed", "<i4"), ("score", "<i4"), ("n_failed", "<i4"), ("last_frame", "<i4"), ("status", "<i4"), ("desc", "u1", 32)])
assert ROW_T.itemsize == 144
MAX_POINTS, N_TRACKERS = 6, 2
N_ROWS = MAX_POINTS * N_TRACKERS
_w = {"alone": {}, "ratio": {}}


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
    c.close()


def camera(sdvl):
    return sdvl.Camera(dc.CAM["width"], dc.CAM["height"], dc.CAM["fx"], dc.CAM["fy"], dc.CAM["u0"], dc.CAM["v0"])


def filter_params(sdvl, p=dc.PARAMS):
    fp = sdvl.DepthParams()
    fp.px_error_angle, fp.min_depth, fp.scale_min_dist, fp.max_failed = p["px_error_angle"], p["min_depth"], p["scale_min_dist"], p["max_failed"]
    return fp


def launch(ctx, sdvl, cases, track_rows=None, track_set=None):
    """the cases as one call of sdvl_depth_filter -> DepthOut array"""
    n = len(cases)
    states = (sdvl.DepthState * n)()
    for i, c in enumerate(cases):
        s, st = states[i], c["state"]
        s.rho, s.sigma2, s.a, s.b, s.z_range = st["rho"], st["sigma2"], st["a"], st["b"], st["z_range"]
        s.cos_alpha, s.last_distance, s.depth_mean = st["cos_alpha"], st["last_distance"], st["depth_mean"]
        s.position[:] = st["position"]
        s.fixed, s.n_failed = st["fixed"], st["n_failed"]
        s.track_row = -1 if track_rows is None else track_rows[i]
    assert all(c["params"] == cases[0]["params"] for c in cases)          # one parameter record per call
    return ctx.depth_filter([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases],
                            [1 if c["found"] else 0 for c in cases], [c["px"] for c in cases], camera(sdvl), states,
                            filter_params(sdvl, cases[0]["params"]), track_set)


def as_result(o):
    """a DepthOut in the restatement's form"""
    told = o.outcome in (UPDATED, CONVERGED, FIXED_STALE)
    return dict(outcome=o.outcome, n_failed=o.n_failed, rho=o.rho, sigma2=o.sigma2, a=o.a, b=o.b, cos_alpha=o.cos_alpha if told else None,
                last_distance=o.last_distance if told else None, position=tuple(o.position) if told else None, row={})


def alone(ctx, sdvl, name):
    """the case as a launch of its own (n = 1) -> the raw bytes of its DepthOut, kept for the batched tests"""
    if name not in _w["alone"]:
        _w["alone"][name] = bytes(launch(ctx, sdvl, [dc.by_name(name)])[0])
    return _w["alone"][name]


def held(c, got, where):
    bad, ratio = dc.differences(c, got, with_row=False)
    for k, r in ratio.items():
        key = "position" if k.startswith("position") else k
        if r >= _w["ratio"].get(key, (-1.0, None))[0]:
            _w["ratio"][key] = (r, c["name"])
    assert not bad, (where, c["name"], c["purpose"], bad)


# ---------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", NAMES)
def test_case_alone(ctx, sdvl, name):
    c = dc.by_name(name)
    o = sdvl.DepthOut.from_buffer_copy(alone(ctx, sdvl, name))
    got = as_result(o)
    want, bound = dc.expected(c)
    for k, r in sorted(dc.differences(c, got, with_row=False)[1].items()):
        print("%s %s: device %r restatement %r ratio %.3g" % (name, k, dr._numbers(got)[k], dr._numbers(want)[k], r))
    held(c, got, "alone")
    if want["outcome"] in (NOT_FOUND, NOT_FOUND | DELETED, SKIPPED):
        # nothing computed reaches these outputs: the state comes back as it went in (b + 1 for a miss), bit for bit
        st = c["state"]
        assert (o.rho, o.sigma2, o.a, o.b) == (st["rho"], st["sigma2"], st["a"], st["b"] + (0.0 if c["found"] else 1.0))
    if c["state"]["fixed"] and want["position"] is not None:
        assert tuple(o.position) == c["state"]["position"]                  # Point::GetPosition of a fixed point: p3d_, untouched


@pytest.mark.parametrize("n", [127, 128, 129, 300])
def test_all_cases_in_one_launch(ctx, sdvl, n):
    """the workgroup is 128 lanes behind an `i >= n` guard: every case in one launch of n items, in an order that changes with n, gives
    the bits it gives alone, wherever it stands and whoever its neighbours are"""
    usual = [c for c in CASES if c["params"] == dc.PARAMS]                 # all but the case with a min_depth of its own
    assert len(usual) == len(CASES) - 1 and len(usual) % 7
    order = [usual[(7 * i + n) % len(usual)] for i in range(n)]
    assert {c["name"] for c in order} == {c["name"] for c in usual}
    fout = launch(ctx, sdvl, order)
    for i, c in enumerate(order):
        assert bytes(fout[i]) == alone(ctx, sdvl, c["name"]), (n, i, c["name"])


def test_sequence_follows_the_device_too(ctx, sdvl):
    """the twelve updates again, each step's state now the DEVICE's previous output: the same decision at every step, converged by
    the last one alone, at the depth the point lies at"""
    seq = dc.sequence()
    st = dict(seq[0]["state"])
    for k, c in enumerate(seq):
        o = launch(ctx, sdvl, [dict(c, state=st)])[0]
        assert o.outcome == (CONVERGED if k == len(seq) - 1 else UPDATED), (k, o.outcome)
        st = dict(st, rho=o.rho, sigma2=o.sigma2, a=o.a, b=o.b, cos_alpha=o.cos_alpha, last_distance=o.last_distance, n_failed=o.n_failed)
    want, bound = dc.expected(seq[-1])
    print("sequence end: device chain rho %r, restatement chain rho %r, last step's bound %.3g" % (o.rho, want["rho"], bound["rho"]))
    assert abs(1.0 / o.rho - 2.5) < 1e-3


# ---------------------------------------------------------------------------------------------------- the row patch
def table(ctx, sdvl):
    """a set of 2 trackers with MAX_POINTS rows each, all uploaded, every row different -> the set"""
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
            p.bearing[:] = dr.unproject(dc.CAM, (100.0 + r, 200.0 - r))
            p.idepth, p.idepth_std = 0.4 + 0.01 * r, 0.05 + 0.001 * r
            p.ref = _w["frame"].h.value
            p.level, p.fixed, p.score, p.n_failed, p.last_frame, p.status = r % 3, 0, 10 + r, 5 + r % 4, 7, r % 4
            p.desc[:] = [(r * 17 + j) % 256 for j in range(32)]
            rows[-1].append(p)
    _w["set"].upload(list(range(N_TRACKERS)), [0] * N_TRACKERS, rows, [[] for _ in range(N_TRACKERS)])
    return _w["set"]


def rows_of(ctx, s):
    return ctx.track_points_download(s).copy().view(ROW_T).reshape(-1)


def patched(c, before, after, o, where):
    """one named row before and after the call that ran case c on it with the device outcome o: it changed exactly as the restatement
    says.  Integers exact, floats within the case's bound and equal to what the same lane returned to the host"""
    want, bound = dc.expected(c)
    patch = want["row"]
    expect = np.array([before], ROW_T)
    for k in ("n_failed", "fixed"):
        if k in patch:
            expect[k][0] = patch[k]
    if patch.get("trash"):
        expect["status"][0] = before["status"] | TRASH
    for k in ("P", "idepth", "idepth_std"):
        if k in patch:
            expect[k][0] = after[k]                               # compared below, not byte for byte
    assert after.tobytes() == expect.tobytes(), (where, c["name"], after, expect)
    if "P" in patch:
        assert tuple(after["P"]) == tuple(o.position)
        for i in range(3):
            assert abs(after["P"][i] - patch["P"][i]) <= bound["row.P%d" % i], (where, c["name"], "P", i)
    else:
        assert after["P"].tobytes() == before["P"].tobytes()
    if "idepth" in patch:
        assert after["idepth"] == o.rho and abs(after["idepth"] - patch["idepth"]) <= bound["row.idepth"]
        assert abs(after["idepth_std"] - math.sqrt(o.sigma2)) <= math.ulp(after["idepth_std"])        # Point::GetStd
        assert abs(after["idepth_std"] - patch["idepth_std"]) <= bound["row.idepth_std"], (where, c["name"], after["idepth_std"], patch["idepth_std"])
    else:
        assert (after["idepth"], after["idepth_std"]) == (before["idepth"], before["idepth_std"])


# per outcome one launch of four items: rows 0, MAX_POINTS (tracker 1, index 0) and the last row, and a fourth item without a row
ROW_LAUNCHES = [
    ("miss-n_failed-0", "miss-n_failed-15", "too-close-min_depth-below", "regular-01"),          # kept miss, deleted miss, skipped
    ("regular-01", "regular-05", "early-return-fixed-stale", "miss-n_failed-16"),                  # updated, converged, fixed stale
    ("early-return-skipped", "convergence-fixed-wide", "miss-n_failed-14", "regular-05"),         # early return untouched, fixed point, miss at the limit
    ("convergence-l-above", "convergence-l-below", "no-triangulation-det-below", "tau-clamp-2.40mrad"),
]


def test_row_launches_name_every_outcome():
    seen = {dc.expected(dc.by_name(n))[0]["outcome"] for names in ROW_LAUNCHES for n in names[:3]}
    assert seen == {NOT_FOUND, NOT_FOUND | DELETED, SKIPPED, UPDATED, CONVERGED, FIXED_STALE}
    assert any(dc.expected(dc.by_name(names[3]))[0]["row"] for names in ROW_LAUNCHES)          # the item without a row would have patched one


@pytest.mark.parametrize("k", range(len(ROW_LAUNCHES)))
def test_row_patch(ctx, sdvl, k):
    s = table(ctx, sdvl)
    named = (0, MAX_POINTS, N_ROWS - 1)
    cases = [dc.by_name(n) for n in ROW_LAUNCHES[k]]
    before = rows_of(ctx, s)
    fout = launch(ctx, sdvl, cases, track_rows=list(named) + [-1], track_set=s)
    after = rows_of(ctx, s)
    for i, c in enumerate(cases):
        assert bytes(fout[i]) == alone(ctx, sdvl, c["name"])        # a table to patch changes nothing of what comes back
    for r in range(N_ROWS):
        if r in named:
            c = cases[named.index(r)]
            patched(c, before[r], after[r], fout[named.index(r)], "launch %d row %d" % (k, r))
            if dc.expected(c)[0]["outcome"] == SKIPPED:
                assert after[r].tobytes() == before[r].tobytes()
        else:
            assert after[r].tobytes() == before[r].tobytes(), (k, r)


def test_rows_patched_twice_accumulate(ctx, sdvl):
    """a deleted miss and then an update on the same row: the trash bit stays, n_failed goes back to 0, fixed follows the update"""
    s = table(ctx, sdvl)
    r = MAX_POINTS + 2
    before = rows_of(ctx, s)
    launch(ctx, sdvl, [dc.by_name("miss-n_failed-16")], track_rows=[r], track_set=s)
    mid = rows_of(ctx, s)
    assert (mid[r]["n_failed"], mid[r]["status"]) == (17, before[r]["status"] | TRASH)
    o = launch(ctx, sdvl, [dc.by_name("regular-05")], track_rows=[r], track_set=s)[0]
    after = rows_of(ctx, s)
    assert o.outcome == CONVERGED and (after[r]["n_failed"], after[r]["fixed"], after[r]["status"]) == (0, 1, before[r]["status"] | TRASH)
    others = [i for i in range(N_ROWS) if i != r]
    assert after[others].tobytes() == before[others].tobytes()


def test_track_row_without_a_set_and_refusals(ctx, sdvl):
    s = table(ctx, sdvl)
    before = rows_of(ctx, s)
    c = dc.by_name("regular-05")
    # a row named with no set given: accepted, nothing patched (there is nothing to patch), the same answer
    o = launch(ctx, sdvl, [c, c], track_rows=[3, 10 ** 6], track_set=None)
    assert bytes(o[0]) == bytes(o[1]) == alone(ctx, sdvl, c["name"])
    assert rows_of(ctx, s).tobytes() == before.tobytes()
    for bad_row in (N_ROWS, -2, 2 ** 31 - 1):
        with pytest.raises(sdvl.SdvlError, match="track_row outside the tables"):
            launch(ctx, sdvl, [c, c], track_rows=[0, bad_row], track_set=s)
    for key in ("sigma2", "z_range"):
        for v in (0.0, -1.0, math.nan):
            with pytest.raises(sdvl.SdvlError, match="sigma2 and z_range must be positive"):
                launch(ctx, sdvl, [dict(c, state=dict(c["state"], **{key: v}))])
    assert rows_of(ctx, s).tobytes() == before.tobytes()                      # a refused call has patched nothing, not even row 0
    # the context is as usable as before
    assert bytes(launch(ctx, sdvl, [c])[0]) == alone(ctx, sdvl, c["name"])
    o = launch(ctx, sdvl, [c], track_rows=[N_ROWS - 1], track_set=s)[0]
    assert rows_of(ctx, s)[N_ROWS - 1]["idepth"] == o.rho
    assert ctx.depth_filter(np.zeros((0, 7)), np.zeros((0, 7)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 2)), camera(sdvl),
                            (sdvl.DepthState * 0)(), filter_params(sdvl)) is not None


# ---------------------------------------------------------------------------------------------------- behind the search
def test_search_plus_filter_alone_equals_search_points_filter(ctx, sdvl, orc, synth):
    """a batch of candidate requests through sdvl_search_points_filter, and through sdvl_search_points followed by sdvl_depth_filter on
    its results: the same kernel on the same records, so the outcomes are equal bit for bit, and so are the rows both patch"""
    from oraclelib import TUM_CAM, fill_search_reqs, search_request_meta, trajectory_pose
    k_cur = 30
    T_ref, T_cur = trajectory_pose(orc, 0), trajectory_pose(orc, k_cur)
    img_ref, img_cur = (synth.render(T, TUM_CAM, 640, 480, frame_id=k) for T, k in ((T_ref, 0), (T_cur, k_cur)))
    meta, ccur = search_request_meta(orc, img_ref, img_cur, T_ref, T_cur, TUM_CAM, 200, 47, False, 0.05)
    f_ref, f_cur = ctx.frame(img_ref), ctx.frame(img_cur)
    f_cur.set_corners(ccur)
    reqs = fill_search_reqs(sdvl, meta, f_ref, f_cur, T_ref, T_cur, False)
    n = len(reqs)
    s = table(ctx, sdvl)
    states = (sdvl.DepthState * n)()
    for i, m in enumerate(meta):
        st = states[i]
        st.rho, st.sigma2, st.a, st.b, st.z_range = m["idepth"], m["istd"] ** 2, 10.0 + i % 5, 10.0 + i % 7, 6.0
        st.cos_alpha, st.last_distance, st.depth_mean = 1.0, 1.0 / m["idepth"], 2.0
        st.position[:] = (0.1, 0.2, 2.0)
        st.fixed, st.n_failed, st.track_row = int(i % 11 == 3), i % 17, (i % N_ROWS if i < N_ROWS else -1)
    cam, fp, sp = camera(sdvl), filter_params(sdvl), sdvl.default_search_params()
    res, fout = ctx.search_points_filter(reqs, cam, sp, states, fp, track_set=s)
    rows_a = rows_of(ctx, s)
    table(ctx, sdvl)                                                       # the same rows again
    plain = ctx.search_points(reqs, cam, sp)
    assert [(r.found, tuple(r.px), r.level) for r in plain] == [(r.found, tuple(r.px), r.level) for r in res]
    got = ctx.depth_filter([T_cur] * n, [T_ref] * n, [m["bearing"] for m in meta], [r.found for r in plain], [tuple(r.px) for r in plain], cam, states, fp, s)
    assert bytes(got) == bytes(fout)
    assert rows_of(ctx, s).tobytes() == rows_a.tobytes()
    outcomes = [o.outcome & 0xFF for o in fout]
    assert outcomes.count(UPDATED) + outcomes.count(CONVERGED) >= 20 and outcomes.count(NOT_FOUND) >= 5, outcomes
    _, no_set = ctx.search_points_filter(reqs, cam, sp, states, fp)
    assert bytes(no_set) == bytes(fout)                                    # and a table to patch changes nothing of what comes back
    f_ref.close(); f_cur.close()


@pytest.mark.parametrize("n", [1, 129])
def test_entries_launch_what_they_did_before(ctx, sdvl, orc, synth, n):
    """the kernels each of the six entries launches, by the context's own launch counts: the stated entries one filter kernel (the stereo
    one behind one stereo_lookup), the searched entries what sdvl_search_points launches for the same requests and then the same.
    n = 129: the first size with a second 128-lane workgroup, one request repeated; only launches are counted here, the values are
    the business of the tests above and of test_gpu_depth_measure.py / test_gpu_stereo_lookup.py"""
    from oraclelib import TUM_CAM, fill_search_reqs, search_request_meta, trajectory_pose
    if "launch_pair" not in _w:
        T_ref, T_cur = trajectory_pose(orc, 0), trajectory_pose(orc, 30)
        img_ref, img_cur = (synth.render(T, TUM_CAM, 640, 480, frame_id=k) for T, k in ((T_ref, 0), (T_cur, 30)))
        meta, ccur = search_request_meta(orc, img_ref, img_cur, T_ref, T_cur, TUM_CAM, 1, 47, False, 0.05)
        _w["launch_pair"] = (T_ref, T_cur, img_ref, np.array(img_cur), ccur, meta[0])
    T_ref, T_cur, img_ref, img_cur, ccur, m = _w["launch_pair"]
    f_ref, f_cur = ctx.frame(img_ref), ctx.frame(img_cur)
    f_cur.set_corners(ccur)
    reqs = fill_search_reqs(sdvl, [m] * n, f_ref, f_cur, T_ref, T_cur, False)
    states = (sdvl.DepthState * n)()
    for st in states:
        st.rho, st.sigma2, st.a, st.b, st.z_range = m["idepth"], m["istd"] ** 2, 10.0, 10.0, 6.0
        st.cos_alpha, st.last_distance, st.depth_mean = 1.0, 1.0 / m["idepth"], 2.0
        st.position[:] = (0.1, 0.2, 2.0)
        st.fixed, st.n_failed, st.track_row = 0, 0, -1
    cam, fp, sp = camera(sdvl), filter_params(sdvl), sdvl.default_search_params()
    depth_jobs = [(np.full((480, 640), 2.0, np.float32), 0, n)]
    stereo_jobs = [(f_cur, img_cur, 0, n)]                                 # (the left image as its own right one: a pair all the same)

    def counted(call):
        ctx.timing_reset()
        out = call()
        return out, {k: launches for k, (_, launches) in ctx.timing_get().items() if launches > 0}

    ctx.timing_enable(True)
    try:
        plain, search = counted(lambda: ctx.search_points(reqs, cam, sp))
        assert search and not {"depth_filter", "depth_filter_measured", "depth_filter_stereo", "stereo_lookup"} & set(search), search
        stated = ([T_cur] * n, [T_ref] * n, [m["bearing"]] * n, [r.found for r in plain], [tuple(r.px) for r in plain])
        levels = [r.level if r.found else 0 for r in plain]
        got = {
            "stated, triangulated": counted(lambda: ctx.depth_filter(*stated, cam, states, fp))[1],
            "stated, measured": counted(lambda: ctx.depth_filter_measured(*stated, levels, cam, states, fp, depth_jobs, 640, 480))[1],
            "stated, stereo": counted(lambda: ctx.depth_filter_stereo(*stated, levels, cam, states, fp, stereo_jobs, 0.11))[1],
            "searched, triangulated": counted(lambda: ctx.search_points_filter(reqs, cam, sp, states, fp))[1],
            "searched, measured": counted(lambda: ctx.search_points_filter_measured(reqs, cam, sp, states, fp, depth_jobs, 640, 480))[1],
            "searched, stereo": counted(lambda: ctx.search_points_filter_stereo(reqs, cam, sp, states, fp, stereo_jobs, 0.11))[1],
        }
    finally:
        ctx.timing_enable(False)
        f_ref.close(); f_cur.close()
    own = {"triangulated": {"depth_filter": 1}, "measured": {"depth_filter_measured": 1}, "stereo": {"stereo_lookup": 1, "depth_filter_stereo": 1}}
    print("n = %d, sdvl_search_points: %s" % (n, search))
    for entry, launches in got.items():
        print("n = %d, %s: %s" % (n, entry, launches))
    for entry, launches in got.items():
        form, source = entry.split(", ")
        assert launches == dict(search if form == "searched" else {}, **own[source]), (n, entry, launches)


def test_largest_ratios():
    """not a check of its own: prints, per output, the largest |device - restatement| / bound the tests above met (all are <= 1, or a
    test above has failed)"""
    print()
    for k, (r, name) in sorted(_w["ratio"].items()):
        print("device vs restatement, %-13s largest deviation / bound %.3g (%s)" % (k, r, name))
    assert all(r <= 1.0 for r, _ in _w["ratio"].values())
