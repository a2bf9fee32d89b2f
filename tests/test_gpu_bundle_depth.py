"""sdvl_bundle_adjust_depth on the device, through the C-ABI, against tests/bundle_depth_restatement.py on the problems of
tests/bundle_depth_cases.py.

Per case, as tests/test_gpu_bundle.py does for the monocular call: the status, the level every edge ended on, the vertices that
dropped out of a stage, the iterations, the trials of every iteration and whether it ended on an accepted trial are EQUAL to the
restatement's up to the first trial the restatement marks settled (|chi - chi'| < 1e-9 chi; with a depth on every edge most cases
have some, tests/test_bundle_depth_restatement_cpu.py prints them and asserts the margins before them), chi2 agrees to 1e-9 relative,
and the final poses and points lie within BOUND of the restatement's.

BOUND.  Both sides are FP64 and differ in the order of their sums (and in the last bits of sin / cos).  Measured on the MI355X, the
largest deviation of any pose entry or point coordinate over the 17 cases is MEASURED = 1.78e-9 (a point coordinate of `dropped/all`;
`triple/all` 8.7e-10, `pair/all` 7.1e-10); BOUND is 10 x that, the factor the project uses to cover inputs conditioned differently
from these.  The other 14 cases stay below 1e-13.  Why three cases stand 1e4 above the rest, and above the monocular call's 1.24e-11: a
depth on every edge of a small window makes the problem so well conditioned that the fifth Huber iteration already ends settled, so
every trial of stage 2 is decided by the last bits of chi2.  The restatement rejects all of them there (`triple/all`: trials [4, 8],
`dropped/all`: [2, 9]), the device accepts some ([7, 3, 1], [1, 1, 1]), and an accepted settled step still moves the estimates by
1e-10 .. 1e-9 (in the restatement itself, `pair/all` after one and after three stage-2 iterations differs by 5.5e-10).  Both ends are
the same minimum to the precision chi2 can tell: chi2 agrees to 1e-9 relative in every case.

`scale` against the truth: the bounds of the CPU test (<= 1e-9 with a depth on every edge, <= 1e-5 with one on half).

Same bits: all cases in two orders, `full/all` alone and a repeated call; problems without a depth mixed into a call with depth
problems give the bytes the monocular call gives for them.
Refusals: a NaN depth, bf <= 0 with depth edges present and 17 free poses are refused with nothing written; NaN in one observation
ends that problem with SDVL_BUNDLE_NONFINITE and leaves the others of the call bit-identical.

Run with -s: every test prints its figures before it asserts."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bundle_cases as bc
import bundle_depth_cases as dc
import bundle_depth_restatement as bd
import bundle_restatement as br
from test_gpu_bundle import same_bits, wide_problem

pytestmark = pytest.mark.gpu

MEASURED = 1.78e-9       # case `dropped/all`, a point coordinate, behind settled trials; the cases without them stay below 1e-13
BOUND = 10 * MEASURED


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def together(ctx):
    """all cases in one call, in the order of dc.NAMES"""
    return dict(zip(dc.NAMES, ctx.bundle_adjust([dc.case(n) for n in dc.NAMES], dc.CAM, bf=dc.BF)))


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_against_the_restatement(together, name):
    got, ref = together[name], dc.restated(name)
    d_pose = float(np.abs(got["poses"] - ref["poses"]).max())
    d_pt = float(np.abs(got["points"] - ref["points"]).max())
    settled = next(((t["stage"], t["it"]) for t in ref["log"] if t["settled"]), None)
    print("%s: status %d level-1 %d | stage trials %s / %s | chi2 %.6g -> %.6g, %.6g -> %.6g | first settled %s | deviation pose %.3g point %.3g"
          % (name, got["status"], got["n_level1"], got["stages"][0]["trials_per_it"], got["stages"][1]["trials_per_it"],
             got["stages"][0]["chi2_before"], got["stages"][0]["chi2_after"], got["stages"][1]["chi2_before"], got["stages"][1]["chi2_after"],
             settled, d_pose, d_pt))
    assert got["status"] == ref["status"] == br.OK
    assert np.array_equal(got["levels"], ref["levels"]) and got["n_level1"] == ref["n_level1"]
    assert np.array_equal(got["pose_stages"], ref["pose_stages"])
    assert np.array_equal(got["point_stages"], ref["point_stages"])
    for s in range(2):
        g, r = got["stages"][s], ref["stages"][s]
        if r is None:
            assert g["iterations"] == 0
            continue
        upto = len(r["trials_per_it"])
        if settled is not None and settled[0] <= s:
            upto = settled[1] if settled[0] == s else 0
        else:
            assert g["iterations"] == r["iterations"] and g["trials"] == r["trials"]
        assert g["trials_per_it"][:upto] == r["trials_per_it"][:upto]
        assert g["accepted_its"][:upto] == r["accepted_its"][:upto]
        assert g["chi2_after"] <= g["chi2_before"]
        assert abs(g["chi2_before"] - r["chi2_before"]) <= 1e-9 * r["chi2_before"]
        assert abs(g["chi2_after"] - r["chi2_after"]) <= 1e-9 * r["chi2_after"]
    assert d_pose <= BOUND and d_pt <= BOUND


def test_wrong_depths_end_on_level_one(together):
    p, lv = dc.case("wrong_depth"), together["wrong_depth"]["levels"] == 1
    clean = ~p["wrong"] & ~p["shifted"]
    print("wrong depths %d, on level 1 %d; clean edges on level 1 %d" % (p["wrong"].sum(), (lv & p["wrong"]).sum(), (lv & clean).sum()))
    assert lv[p["wrong"]].all() and (lv & clean).sum() <= 2


def test_scale_against_the_truth(ctx):
    probs = [dc.scale(src, share) for src in ("pair", "triple") for share in dc.SHARES]
    mono = ctx.bundle_adjust(probs, dc.CAM)
    depth = ctx.bundle_adjust(probs, dc.CAM, bf=dc.BF)
    for p, m, g in zip(probs, mono, depth):
        d_mono = float(np.abs(m["points"] - p["truth_points"]).max())
        d = max(float(np.abs(g["points"] - p["truth_points"]).max()), float(np.abs(g["poses"] - p["truth_poses"]).max()))
        print("%s: monocular call ends %.3g from the truth, depth call %.3g (chi2 %.3g -> %.3g)"
              % (p["name"], d_mono, d, g["stages"][0]["chi2_before"], g["stages"][1]["chi2_after"]))
        assert m["status"] == g["status"] == br.OK and g["n_level1"] == 0
        assert d_mono >= 0.29
        assert d <= (1e-9 if p["name"].endswith("/all") else 1e-5)


def test_same_bits_in_every_batch_position(ctx, together):
    rev = dict(zip(dc.NAMES[::-1], ctx.bundle_adjust([dc.case(n) for n in dc.NAMES[::-1]], dc.CAM, bf=dc.BF)))
    alone = ctx.bundle_adjust([dc.case("full/all")], dc.CAM, bf=dc.BF)[0]
    again = dict(zip(dc.NAMES, ctx.bundle_adjust([dc.case(n) for n in dc.NAMES], dc.CAM, bf=dc.BF)))
    for n in dc.NAMES:
        assert same_bits(together[n], rev[n]), n
        assert same_bits(together[n], again[n]), n
    assert same_bits(together["full/all"], alone)


def test_problems_without_a_depth_give_the_monocular_bytes(ctx, together):
    mono = dict(zip(bc.NAMES, ctx.bundle_adjust([bc.case(n) for n in bc.NAMES], bc.CAM)))
    zeros = {n: dict(bc.case(n), edge_d=np.zeros(len(bc.case(n)["edge_pt"]))) for n in bc.NAMES}
    # interleaved with depth problems; `single` and `rejects` come without edge_d at all
    mix, keys = [], []
    for n in bc.NAMES:
        mix += [dc.case(n + "/all"), bc.case(n) if n in ("single", "rejects") else zeros[n], dc.case(n + "/half")]
        keys += [n + "/all", n, n + "/half"]
    got = ctx.bundle_adjust(mix, dc.CAM, bf=dc.BF)
    for k, g in zip(keys, got):
        assert same_bits(g, mono[k] if k in mono else together[k]), k
    only = ctx.bundle_adjust([zeros[n] for n in bc.NAMES], dc.CAM, bf=dc.BF)       # no depth in the whole call: bf is not looked at
    for n, g in zip(bc.NAMES, only):
        assert same_bits(g, mono[n]), n
    assert same_bits(ctx.bundle_adjust([zeros["full"]], dc.CAM, bf=0.0)[0], mono["full"])


def raw_call(sdvl, ctx, p, bf):
    """through the raw entry point with marked outputs -> rc and whether anything was written"""
    poses, pts = np.array(p["poses"]), np.array(p["points"])
    keep = (poses.copy(), pts.copy())
    n_e = len(p["edge_pt"])
    prob = (sdvl.BundleProblem * 1)(sdvl.BundleProblem(0, len(poses), 0, len(pts), 0, n_e))
    edges = (sdvl.BundleEdgeDepth * n_e)(*[sdvl.BundleEdgeDepth(int(a), int(b), u, v, d)
                                           for a, b, (u, v), d in zip(p["edge_pt"], p["edge_kf"], p["edge_uv"], p["edge_d"])])
    lv, ks, ps = np.full(n_e, 7, np.int32), np.full(len(poses), 7, np.int32), np.full(len(pts), 7, np.int32)
    res = (sdvl.BundleResult * 1)()
    res[0].status = 77
    cam = sdvl.Camera(0, 0, *dc.CAM)
    fixed = np.asarray(p["fixed"], np.int32)
    rc = ctx.lib.sdvl_bundle_adjust_depth(ctx.h, 1, prob, len(poses), poses.ctypes.data, fixed.ctypes.data, len(pts), pts.ctypes.data, n_e, edges,
                                          C.byref(cam), bf, lv.ctypes.data, ks.ctypes.data, ps.ctypes.data, res)
    untouched = (np.array_equal(poses, keep[0]) and np.array_equal(pts, keep[1]) and (lv == 7).all() and (ks == 7).all() and (ps == 7).all()
                 and res[0].status == 77)
    return rc, untouched


def test_refusals_write_nothing(sdvl, ctx):
    pair = dc.case("pair/all")
    d = np.array(pair["edge_d"])
    d[2] = np.nan
    assert raw_call(sdvl, ctx, dict(pair, edge_d=d), dc.BF) == (-1, True)
    assert "depth" in ctx.lib.sdvl_last_error(ctx.h).decode()
    d[2] = np.inf
    assert raw_call(sdvl, ctx, dict(pair, edge_d=d), dc.BF) == (-1, True)
    for bf in (0.0, -1.0, float("nan"), float("inf")):
        assert raw_call(sdvl, ctx, pair, bf) == (-1, True), bf
        assert "bf" in ctx.lib.sdvl_last_error(ctx.h).decode()
    wide = wide_problem(sdvl.BUNDLE_MAX_FREE + 1)
    assert raw_call(sdvl, ctx, dict(wide, edge_d=np.full(len(wide["edge_pt"]), 5.0)), dc.BF) == (-3, True)
    with pytest.raises(sdvl.SdvlError):
        ctx.bundle_adjust([dc.case("triple/all"), dict(pair, edge_d=d)], dc.CAM, bf=dc.BF)
    rc, untouched = raw_call(sdvl, ctx, pair, dc.BF)           # the same call with nothing wrong runs
    assert rc == 0 and not untouched


def test_a_nan_observation_ends_its_own_problem(ctx, together):
    pair = dc.case("pair/all")
    nan = dict(pair, edge_uv=np.array(pair["edge_uv"]))
    nan["edge_uv"][3, 0] = np.nan
    got = ctx.bundle_adjust([dc.case("triple/all"), nan, dc.case("single/half"), dc.case("pair/all")], dc.CAM, bf=dc.BF)
    print("statuses", [g["status"] for g in got])
    assert [g["status"] for g in got] == [br.OK, br.NONFINITE, br.OK, br.OK]
    assert got[1]["poses"].tobytes() == np.asarray(nan["poses"], np.float64).tobytes()
    assert got[1]["points"].tobytes() == np.asarray(nan["points"], np.float64).tobytes()
    assert not got[1]["levels"].any() and not got[1]["pose_stages"].any() and not got[1]["point_stages"].any()
    assert bd.bundle_adjust(nan)["status"] == br.NONFINITE
    for g, n in ((got[0], "triple/all"), (got[2], "single/half"), (got[3], "pair/all")):
        assert same_bits(g, together[n]), n
