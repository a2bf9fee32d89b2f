"""depth_filter_measured_kernel (csrc/sdvl_depth_filter.hip) through sdvl_depth_filter_measured, against its specification
tests/depth_measure_restatement.py on the cases of tests/depth_measure_cases.py: float and 16-bit images (16-bit at an odd address and with
rows wider than their samples, both in HBM; tight images in pageable memory), with and without a lens, found levels 0 to 4 on 24 x 16,
every status, a request in no job, misses, a fixed point, the early return of Point::Update, a converging update, rows patched in a
tracking table, and launches of 1, 127, 128 and 129 requests.

Outcomes, n_failed and status bytes are exact.  A float is held to the case's own bound (depth_measure_restatement.tolerance): behind a
measured update exp is the only transcendental call, so the bound is 4 times what +-4 ulp on its result move the output, plus 8 ulp of the
value; outputs without a transcendental behind them keep the 8 ulp.  A request that does not measure (status not OK, no image, a miss)
equals Context.depth_filter on the same inputs bit for bit: device against device, no tolerance.

test_largest_ratios prints the largest |device - restatement| / bound per output (run with -s).  Measured on an MI355X, 2026-10-20: 41 of
the 43 cases come back bit-equal to the restatement, every measured update among them; `edge` and `edge-stride4`, triangulated fall-backs, give
position 0.039, rho and last_distance 0.028 of their bound."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_measure_cases as mc
import depth_restatement as dr
import depth_seed_restatement as dsr
from depth_restatement import CONVERGED, DELETED, FIXED_STALE, NOT_FOUND, SKIPPED, UPDATED
from track_restatement import TRASH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_T = np.dtype([("P", "<f8", 3), ("ipx", "<f8", 2), ("ibearing", "<f8", 3), ("idepth", "<f8"), ("idepth_std", "<f8"), ("ref", "<i4"), ("pad_", "<i4"),
                  ("ilevel", "<i4"), ("fixed", "<i4"), ("score", "<i4"), ("n_failed", "<i4"), ("last_frame", "<i4"), ("status", "<i4"), ("desc", "u1", 32)])
assert ROW_T.itemsize == 144
MAX_POINTS, N_TRACKERS = 6, 2
N_ROWS = MAX_POINTS * N_TRACKERS

CASES = mc.all_cases()
NAMES = [c["name"] for c in CASES]
_w = {"alone": {}, "ratio": {}, "dev": {}}


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
    _w["dev"].clear()
    c.close()


def camera(sdvl, cam):
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


def job_of(sdvl, c, i):
    """the case's image as request i's job: `tight` a pageable numpy array (staged by the call); `odd` in HBM one byte past an aligned
    address; `padded` in HBM with rows 10 bytes wider than their samples"""
    import torch
    d = c["depth"]
    h, w = d.shape
    fmt = sdvl.SDVL_DEPTH_U16 if d.dtype == np.uint16 else sdvl.SDVL_DEPTH_F32
    if c["layout"] == "tight":
        key = ("tight", c["kind"])
        if key not in _w["dev"]:
            _w["dev"][key] = np.array(d)
        a = _w["dev"][key]
        return sdvl.DepthJob(a.ctypes.data, 0, a.strides[0], fmt, 0, c["scale"], i, i + 1)
    row = w * d.itemsize
    pitch, lead = (row, 1) if c["layout"] == "odd" else (row + 10, 0)
    key = (c["layout"], c["kind"])
    if key not in _w["dev"]:
        buf = np.full(lead + h * pitch, 0xA5, np.uint8)
        buf[lead:].reshape(h, pitch)[:, :row] = d.view(np.uint8).reshape(h, row)
        _w["dev"][key] = torch.from_numpy(buf).cuda()
    t = _w["dev"][key]
    assert t.data_ptr() % 2 == 0
    return sdvl.DepthJob(t.data_ptr() + lead, 1, pitch, fmt, 0, c["scale"], i, i + 1)


def call_key(c):
    return (c["group"], tuple(sorted(c["cam"].items())), c["dist"], tuple(sorted(c["rule"].items())), tuple(sorted(c["params"].items())))


def launch(ctx, sdvl, cases, track_rows=None, track_set=None):
    """the cases (of one group) as one call of sdvl_depth_filter_measured -> (DepthOut array, status bytes)"""
    assert len({call_key(c) for c in cases}) == 1
    c0 = cases[0]
    jobs = [job_of(sdvl, c, i) for i, c in enumerate(cases) if c["depth"] is not None]
    return ctx.depth_filter_measured([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases],
                                     [1 if c["found"] else 0 for c in cases], [c["px"] for c in cases], [c["level"] for c in cases],
                                     camera(sdvl, c0["cam"]), states_of(sdvl, cases, track_rows), filter_params(sdvl, c0["params"]), jobs,
                                     int(c0["cam"]["width"]), int(c0["cam"]["height"]), c0["dist"], c0["noise_abs"], c0["noise_quad"], track_set,
                                     **c0["rule"])


def triangulated(ctx, sdvl, cases, track_rows=None, track_set=None):
    """the same cases through sdvl_depth_filter"""
    c0 = cases[0]
    return ctx.depth_filter([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases],
                            [1 if c["found"] else 0 for c in cases], [c["px"] for c in cases], camera(sdvl, c0["cam"]), states_of(sdvl, cases, track_rows),
                            filter_params(sdvl, c0["params"]), track_set)


def as_result(o, status):
    told = o.outcome in (UPDATED, CONVERGED, FIXED_STALE)
    return dict(outcome=o.outcome, n_failed=o.n_failed, rho=o.rho, sigma2=o.sigma2, a=o.a, b=o.b, cos_alpha=o.cos_alpha if told else None,
                last_distance=o.last_distance if told else None, position=tuple(o.position) if told else None, row={}, status=int(status))


def alone(ctx, sdvl, name):
    """the case as a launch of its own (n = 1) -> (the raw bytes of its DepthOut, its status byte)"""
    if name not in _w["alone"]:
        fout, status = launch(ctx, sdvl, [mc.by_name(name)])
        _w["alone"][name] = (bytes(fout[0]), int(status[0]))
    return _w["alone"][name]


# ---------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", NAMES)
def test_case_alone(ctx, sdvl, name):
    c = mc.by_name(name)
    raw, status = alone(ctx, sdvl, name)
    o = sdvl.DepthOut.from_buffer_copy(raw)
    got = as_result(o, status)
    want, bound = mc.expected(c)
    bad, ratio = mc.differences(c, got, with_row=False)
    for k, r in sorted(ratio.items()):
        print("%s %s: device %r restatement %r ratio %.3g" % (name, k, dr._numbers(got)[k], dr._numbers(want)[k], r))
        key = "position" if k.startswith("position") else k
        if r >= _w["ratio"].get(key, (-1.0, None))[0]:
            _w["ratio"][key] = (r, name)
    assert not bad, (name, c["purpose"], bad)
    if status != dsr.OK:
        # not measured: the triangulated filter's answer, bit for bit
        assert raw == bytes(triangulated(ctx, sdvl, [c])[0]), name
    if want["outcome"] in (NOT_FOUND, NOT_FOUND | DELETED, SKIPPED):
        st = c["state"]
        assert (o.rho, o.sigma2, o.a, o.b) == (st["rho"], st["sigma2"], st["a"], st["b"] + (0.0 if c["found"] else 1.0))
    if c["state"]["fixed"] and want["position"] is not None:
        assert tuple(o.position) == c["state"]["position"]
    if c["want"].get("exact_range") and want["outcome"] in (UPDATED, CONVERGED):
        # the measurement is the point's range: the estimate moves towards it and not past it
        r0, r1, truth = c["state"]["rho"], o.rho, 1.0 / c["range"]
        assert min(r0, truth) - 1e-12 <= r1 <= max(r0, truth) + 1e-12, (r0, r1, truth)


@pytest.mark.parametrize("n", [127, 128, 129])
def test_plain_cases_in_one_launch(ctx, sdvl, n):
    """the workgroup is 128 lanes behind an `i >= n` guard: the cases of the largest group in one launch of n requests, one job each, in an
    order that changes with n, give the bits and the status they give alone"""
    usual = mc.groups()["plain"]
    assert len(usual) >= 25 and len(usual) % 7
    order = [usual[(7 * i + n) % len(usual)] for i in range(n)]
    assert {c["name"] for c in order} == {c["name"] for c in usual}
    fout, status = launch(ctx, sdvl, order)
    for i, c in enumerate(order):
        assert (bytes(fout[i]), int(status[i])) == alone(ctx, sdvl, c["name"]), (n, i, c["name"])
    # every request that did not measure, against the triangulated filter in one launch of the same n
    tri = triangulated(ctx, sdvl, order)
    not_ok = [i for i in range(n) if status[i] != dsr.OK]
    assert len(not_ok) >= n // 3 and len(not_ok) < n
    for i in not_ok:
        assert bytes(fout[i]) == bytes(tri[i]), (n, i, order[i]["name"])
    assert any(bytes(fout[i]) != bytes(tri[i]) for i in range(n) if status[i] == dsr.OK)


@pytest.mark.parametrize("group", sorted(g for g in mc.groups() if g != "plain"))
def test_other_groups_in_one_launch(ctx, sdvl, group):
    cases = mc.groups()[group]
    fout, status = launch(ctx, sdvl, cases)
    for i, c in enumerate(cases):
        assert (bytes(fout[i]), int(status[i])) == alone(ctx, sdvl, c["name"]), (group, c["name"])


def test_one_job_for_a_range_of_requests(ctx, sdvl):
    """a job names a RANGE of requests: three requests on one image, one before and one behind them on none"""
    names = ("no-job", "ok-00-level0", "ok-03-level1", "skip-depth_mean", "no-job-level3")
    cases = [mc.by_name(n) for n in names]
    img = np.array(mc.image("f32"))
    fout, status = ctx.depth_filter_measured([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases], [1] * 5,
                                             [c["px"] for c in cases], [c["level"] for c in cases], camera(sdvl, mc.CAM), states_of(sdvl, cases),
                                             filter_params(sdvl, mc.PARAMS), [(img, 1, 4)], mc.W, mc.H, None, mc.NOISE["noise_abs"], mc.NOISE["noise_quad"])
    for i, n in enumerate(names):
        assert (bytes(fout[i]), int(status[i])) == alone(ctx, sdvl, n), n
    # and with no job at all every request is the triangulated filter's
    fout, status = ctx.depth_filter_measured([c["cur_pose"] for c in cases], [c["ref_pose"] for c in cases], [c["bearing"] for c in cases], [1] * 5,
                                             [c["px"] for c in cases], [c["level"] for c in cases], camera(sdvl, mc.CAM), states_of(sdvl, cases),
                                             filter_params(sdvl, mc.PARAMS), [], mc.W, mc.H)
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
            p.bearing[:] = dr.unproject(mc.CAM, (10.0 + r, 12.0 - r))
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
    ("ok-00-level0", "ok-converges", "skip-depth_mean", "ok-01-level0"),        # measured: updated, converged, skipped
    ("miss-n_failed-3", "miss-n_failed-15", "ok-fixed", "ok-converges"),        # kept miss, deleted miss, a fixed point
    ("hole-zero", "edge", "no-job", "ok-u16-0"),                               # the triangulated update behind a status, and without an image
]


@pytest.mark.parametrize("k", range(len(ROW_LAUNCHES)))
def test_row_patch(ctx, sdvl, k):
    """rows 0, MAX_POINTS (tracker 1, index 0) and the last row are named by three requests, a fourth has none: the named rows change as
    the restatement says and hold what the same lane returned; every other row keeps its bytes"""
    s = table(ctx, sdvl)
    named = (0, MAX_POINTS, N_ROWS - 1)
    cases = [mc.by_name(n) for n in ROW_LAUNCHES[k]]
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
        want, bound = mc.expected(c)
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
        # the rows the triangulated filter patches from the same requests are the same bytes
        table(ctx, sdvl)
        triangulated(ctx, sdvl, cases[:3], track_rows=list(named), track_set=s)
        tri = rows_of(ctx, s)
        for r in named:
            assert tri[r].tobytes() == after[r].tobytes(), r


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx, sdvl):
    """an unknown format, U16 without a scale, a short stride, a range outside n, a level outside the pyramid, negative noise: refused
    with a message, nothing patched, the context as usable as before"""
    c = mc.by_name("ok-00-level0")
    img = np.array(mc.image("f32"))
    s = table(ctx, sdvl)
    before = rows_of(ctx, s)

    def call(job=None, level=0, n_req=1, **kw):
        j = dict(depth=img.ctypes.data, on_device=0, stride=mc.W * 4, format=0, pad_=0, scale=1.0, c_begin=0, c_end=1)
        j.update(job or {})
        cases = [c] * n_req
        return ctx.depth_filter_measured([c["cur_pose"]] * n_req, [c["ref_pose"]] * n_req, [c["bearing"]] * n_req, [1] * n_req, [c["px"]] * n_req,
                                         [level] * n_req, camera(sdvl, mc.CAM), states_of(sdvl, cases, [0] * n_req), filter_params(sdvl, mc.PARAMS),
                                         [sdvl.DepthJob(**j)], mc.W, mc.H, None, kw.pop("noise_abs", 0.004), kw.pop("noise_quad", 0.002), s, **kw)

    for kw, msg in ((dict(job=dict(format=2)), "unknown depth format"), (dict(job=dict(format=-1)), "unknown depth format"),
                    (dict(job=dict(format=1, stride=mc.W * 2, scale=0.0)), "needs scale > 0"),
                    (dict(job=dict(stride=mc.W * 4 - 1)), "stride smaller than width"), (dict(job=dict(format=1, stride=mc.W * 2 - 1)), "stride smaller than width"),
                    (dict(job=dict(c_end=2)), "range outside"), (dict(job=dict(c_begin=-1)), "range outside"), (dict(job=dict(c_begin=1, c_end=0)), "range outside"),
                    (dict(job=dict(depth=None)), "null depth image"),
                    (dict(level=8), "level outside"), (dict(level=-1), "level outside"),
                    (dict(noise_abs=-0.001), "must not be negative"), (dict(noise_quad=float("nan")), "must not be negative"),
                    (dict(min_valid=10), "min_valid"), (dict(edge_ratio=-0.1), "edge_ratio")):
        with pytest.raises(sdvl.SdvlError, match=msg) as e:
            call(**kw)
        assert "sdvl_depth_filter_measured" in str(e.value), str(e.value)
        assert ctx.lib.sdvl_ctx_health(ctx.h) == 0
    assert rows_of(ctx, s).tobytes() == before.tobytes()
    fout, status = call()
    assert int(status[0]) == dsr.OK and rows_of(ctx, s)[0]["idepth"] == fout[0].rho
    # nothing to do
    fout, status = ctx.depth_filter_measured(np.zeros((0, 7)), np.zeros((0, 7)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0, np.int32),
                                             camera(sdvl, mc.CAM), (sdvl.DepthState * 0)(), filter_params(sdvl, mc.PARAMS), [], mc.W, mc.H)
    assert len(status) == 0


def test_staged_images_are_shared_between_begin_and_end(ctx, sdvl):
    """between sdvl_depth_stage_begin and _end a pageable image is staged once: a change of its contents is not seen until _end"""
    c = mc.by_name("ok-00-level0")
    img = np.array(mc.image("f32"))
    job = [(img, 0, 1)]

    def run():
        return ctx.depth_filter_measured([c["cur_pose"]], [c["ref_pose"]], [c["bearing"]], [1], [c["px"]], [0], camera(sdvl, mc.CAM), states_of(sdvl, [c]),
                                         filter_params(sdvl, mc.PARAMS), job, mc.W, mc.H, None, mc.NOISE["noise_abs"], mc.NOISE["noise_quad"])

    first = run()
    assert (bytes(first[0][0]), int(first[1][0])) == alone(ctx, sdvl, c["name"])
    assert ctx.lib.sdvl_depth_stage_begin(ctx.h) == 0
    assert bytes(run()[0]) == bytes(first[0])
    img[:] = 0.0                                             # holes everywhere
    kept = run()
    assert bytes(kept[0]) == bytes(first[0]) and int(kept[1][0]) == dsr.OK
    # the seed call of the same step reads the same copy
    z, st, _ = ctx.depth_seed(job, mc.W, mc.H, np.array([[12, 8, 0]], np.int32), camera(sdvl, mc.CAM))
    assert int(st[0]) == dsr.OK and z[0] == float(mc.image("f32")[8, 12])
    assert ctx.lib.sdvl_depth_stage_end(ctx.h) == 0
    fresh = run()
    assert int(fresh[1][0]) == dsr.HOLE and bytes(fresh[0]) == bytes(triangulated(ctx, sdvl, [c]))


# ---------------------------------------------------------------------------------------------------- behind the search
def test_search_run_filter_measured_equals_search_then_filter(ctx, sdvl, orc, synth):
    """candidate requests through sdvl_search_run_filter_measured, and through sdvl_search_points followed by sdvl_depth_filter_measured on
    its results (pixel and level): the same kernel on the same records, so outcomes and status bytes are equal bit for bit; the depth
    image is the renderer's plane depth, so most hits measure"""
    from oraclelib import TUM_CAM, fill_search_reqs, search_request_meta, trajectory_pose
    k_cur = 30
    T_ref, T_cur = trajectory_pose(orc, 0), trajectory_pose(orc, k_cur)
    img_ref, img_cur = (synth.render(T, TUM_CAM, 640, 480, frame_id=k) for T, k in ((T_ref, 0), (T_cur, k_cur)))
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
    depth = np.full((480, 640), 2.0, np.float32)
    depth[:, 320:] = 0.0                                     # the right half has no depth: HOLE and FEW beside the border
    half = n // 2
    jobs = [(depth, 0, half)]                                # and the second half of the requests has no image
    res, fout, status = ctx.search_points_filter_measured(reqs, cam, sp, states, fp, jobs, 640, 480, None, 0.004, 0.002)
    plain = ctx.search_points(reqs, cam, sp)
    assert [(r.found, tuple(r.px), r.level) for r in plain] == [(r.found, tuple(r.px), r.level) for r in res]
    got, gstatus = ctx.depth_filter_measured([T_cur] * n, [T_ref] * n, [m["bearing"] for m in meta], [r.found for r in plain], [tuple(r.px) for r in plain],
                                             [r.level if r.found else 0 for r in plain], cam, states, fp, jobs, 640, 480, None, 0.004, 0.002)
    assert bytes(got) == bytes(fout) and np.array_equal(gstatus, status)
    counts = np.bincount(status, minlength=256)
    assert counts[dsr.OK] >= 10 and counts[dsr.HOLE] >= 5 and counts[255] >= half, counts[[0, 1, 2, 3, 4, 255]]
    assert all(status[i] == 255 for i in range(n) if i >= half or not res[i].found)
    # not measured: the triangulated search + filter, bit for bit
    _, tri = ctx.search_points_filter(reqs, cam, sp, states, fp)
    for i in range(n):
        if status[i] != dsr.OK:
            assert bytes(fout[i]) == bytes(tri[i]), i
    f_ref.close(); f_cur.close()


def test_struct_size_matches_the_compiled_header(sdvl, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "sdvl_hip.h"', 'int main() {',
           '  printf("%zu %zu %zu %zu\\n", sizeof(sdvl_depth_measure_params), offsetof(sdvl_depth_measure_params, rule), '
           'offsetof(sdvl_depth_measure_params, noise_abs), offsetof(sdvl_depth_measure_params, noise_quad));', '  return 0;', '}']
    path = tmp_path / "depth_measure_abi.cc"
    path.write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "depth_measure_abi")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(path), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    P = sdvl.DepthMeasureParams
    assert [int(v) for v in out] == [C.sizeof(P), P.rule.offset, P.noise_abs.offset, P.noise_quad.offset] == [48, 0, 32, 40]


def test_largest_ratios():
    """not a check of its own: prints, per output, the largest |device - restatement| / bound test_case_alone met"""
    print()
    for k, (r, name) in sorted(_w["ratio"].items()):
        print("device vs restatement, %-13s largest deviation / bound %.3g (%s)" % (k, r, name))
    assert all(r <= 1.0 for r, _ in _w["ratio"].values())
