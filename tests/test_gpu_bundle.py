"""sdvl_bundle_adjust on the device, through the C-ABI, against tests/bundle_restatement.py on the problems of tests/bundle_cases.py.

Per case: the status, the level every edge ended on, the vertices that dropped out of a stage, the number of iterations, the trials of
every iteration and whether it ended on an accepted trial are EQUAL to the restatement's up to the first trial the restatement marks
settled (|chi - chi'| < 1e-9 chi; no case has one, tests/test_bundle_restatement_cpu.py asserts the margins), and the final poses and
points lie within BOUND of it.

BOUND.  Both sides are FP64 and differ in the order of their sums (and in the last bits of sin / cos).  Measured on the MI355X, the
largest deviation of any pose entry or point coordinate over the eight cases is MEASURED = 1.24e-11 (case `behind`, whose two points
that start behind a camera end 8 units away on level-1 edges only); BOUND is 10 x that, the factor covering inputs conditioned
differently from these, and stays below the project's pose tolerance 1e-4.

Batching: all cases in one call, in two orders, and `full` alone give every problem the same bits; so does a repeated call.
Limits: 17 free poses is SDVL_ERR_CAPACITY and writes nothing; an empty problem and one without an edge to a free pose return their
status with their inputs untouched; NaN in one observation ends that problem with SDVL_BUNDLE_NONFINITE and leaves the others of the
call bit-identical.

Run with -s: every test prints its figures before it asserts."""
import importlib

import numpy as np
import pytest

import bundle_cases as bc
import bundle_restatement as br

pytestmark = pytest.mark.gpu

MEASURED = 1.24e-11      # case `behind`, a point coordinate; the other cases stay below 1.1e-12
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
    """all cases in one call, in the order of bc.NAMES"""
    return dict(zip(bc.NAMES, ctx.bundle_adjust([bc.case(n) for n in bc.NAMES], bc.CAM)))


def same_bits(a, b):
    return (a["status"] == b["status"] and a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
            and np.array_equal(a["levels"], b["levels"]) and np.array_equal(a["pose_stages"], b["pose_stages"])
            and np.array_equal(a["point_stages"], b["point_stages"]) and a["n_level1"] == b["n_level1"]
            and all(np.array([x[k] for k in ("lam", "chi2_before", "chi2_after")]).tobytes() == np.array([y[k] for k in ("lam", "chi2_before", "chi2_after")]).tobytes()
                    and x["trials_per_it"] == y["trials_per_it"] and x["accepted_its"] == y["accepted_its"] for x, y in zip(a["stages"], b["stages"])))


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_against_the_restatement(together, name):
    got, ref = together[name], bc.restated(name)
    d_pose = float(np.abs(got["poses"] - ref["poses"]).max())
    d_pt = float(np.abs(got["points"] - ref["points"]).max())
    print("%s: status %d level-1 %d | stage trials %s / %s | chi2 %.6g -> %.6g, %.6g -> %.6g | deviation pose %.3g point %.3g"
          % (name, got["status"], got["n_level1"], got["stages"][0]["trials_per_it"], got["stages"][1]["trials_per_it"],
             got["stages"][0]["chi2_before"], got["stages"][0]["chi2_after"], got["stages"][1]["chi2_before"], got["stages"][1]["chi2_after"],
             d_pose, d_pt))
    assert got["status"] == ref["status"] == br.OK
    assert np.array_equal(got["levels"], ref["levels"]) and got["n_level1"] == ref["n_level1"]
    assert np.array_equal(got["pose_stages"], ref["pose_stages"])
    assert np.array_equal(got["point_stages"], ref["point_stages"])
    settled = next(((t["stage"], t["it"]) for t in ref["log"] if t["settled"]), None)
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


def test_same_bits_in_every_batch_position(ctx, together):
    rev = dict(zip(bc.NAMES[::-1], ctx.bundle_adjust([bc.case(n) for n in bc.NAMES[::-1]], bc.CAM)))
    alone = ctx.bundle_adjust([bc.case("full")], bc.CAM)[0]
    again = dict(zip(bc.NAMES, ctx.bundle_adjust([bc.case(n) for n in bc.NAMES], bc.CAM)))
    for n in bc.NAMES:
        assert same_bits(together[n], rev[n]), n
        assert same_bits(together[n], again[n]), n
    assert same_bits(together["full"], alone)


def wide_problem(n_free):
    """n_free free poses + one fixed, 40 points seen by all"""
    rng = np.random.default_rng(5)
    n_kf = n_free + 1
    poses = np.stack([bc.arc_pose(k, n_kf) for k in range(n_kf)])
    pts = np.stack([rng.uniform(-1, 1, 40), rng.uniform(-0.7, 0.7, 40), rng.uniform(4, 6, 40)], 1)
    ept, ekf = np.repeat(np.arange(40), n_kf).astype(np.int32), np.tile(np.arange(n_kf), 40).astype(np.int32)
    uv = np.concatenate([bc.project(poses[k], pts[p:p + 1]) for p, k in zip(ept, ekf)]) + 0.3 * rng.standard_normal((len(ept), 2))
    return dict(poses=poses, fixed=np.array([0] * n_free + [1], np.int32), points=pts + 0.01 * rng.standard_normal(pts.shape), edge_pt=ept, edge_kf=ekf,
                edge_uv=uv)


def test_capacity_and_the_cap_itself(sdvl, ctx):
    with pytest.raises(sdvl.SdvlError, match="-3"):
        ctx.bundle_adjust([bc.case("pair"), wide_problem(sdvl.BUNDLE_MAX_FREE + 1)], bc.CAM)
    # nothing was written: the call's own arrays through the raw entry point
    import ctypes as C
    p = wide_problem(17)
    poses, pts = np.array(p["poses"]), np.array(p["points"])
    keep = (poses.copy(), pts.copy())
    prob = (sdvl.BundleProblem * 1)(sdvl.BundleProblem(0, len(poses), 0, len(pts), 0, len(p["edge_pt"])))
    edges = (sdvl.BundleEdge * len(p["edge_pt"]))(*[sdvl.BundleEdge(int(a), int(b), u, v) for a, b, (u, v) in zip(p["edge_pt"], p["edge_kf"], p["edge_uv"])])
    lv, ks, ps = np.full(len(p["edge_pt"]), 7, np.int32), np.full(len(poses), 7, np.int32), np.full(len(pts), 7, np.int32)
    res = (sdvl.BundleResult * 1)()
    res[0].status = 77
    cam = sdvl.Camera(0, 0, *bc.CAM)
    rc = ctx.lib.sdvl_bundle_adjust(ctx.h, 1, prob, len(poses), poses.ctypes.data, p["fixed"].ctypes.data, len(pts), pts.ctypes.data, len(edges), edges,
                                    C.byref(cam), lv.ctypes.data, ks.ctypes.data, ps.ctypes.data, res)
    assert rc == -3
    assert np.array_equal(poses, keep[0]) and np.array_equal(pts, keep[1]) and (lv == 7).all() and (ks == 7).all() and (ps == 7).all() and res[0].status == 77
    # 16 free poses is inside the cap and agrees with the restatement
    p = wide_problem(sdvl.BUNDLE_MAX_FREE)
    p["cam"] = bc.CAM
    got, ref = ctx.bundle_adjust([p], bc.CAM)[0], br.bundle_adjust(p)
    d = max(np.abs(got["poses"] - ref["poses"]).max(), np.abs(got["points"] - ref["points"]).max())
    print("16 free poses: trials %s / %s, deviation %.3g" % (got["stages"][0]["trials_per_it"], got["stages"][1]["trials_per_it"], d))
    assert got["status"] == br.OK and got["stages"][0]["trials_per_it"] == ref["stages"][0]["trials_per_it"]
    assert d <= BOUND


def test_degenerate_problems_return_a_status(ctx, together):
    pair = bc.case("pair")
    none = np.zeros(0, np.int32)
    empty = dict(poses=np.zeros((0, 7)), fixed=none, points=np.zeros((0, 3)), edge_pt=none, edge_kf=none, edge_uv=np.zeros((0, 2)))
    no_edges = dict(pair, edge_pt=none, edge_kf=none, edge_uv=np.zeros((0, 2)))
    only_fixed = dict(pair, edge_pt=pair["edge_pt"][pair["edge_kf"] == 1], edge_kf=pair["edge_kf"][pair["edge_kf"] == 1],
                      edge_uv=pair["edge_uv"][pair["edge_kf"] == 1])
    nan = dict(pair, edge_uv=np.array(pair["edge_uv"]))
    nan["edge_uv"][3, 0] = np.nan
    inf = dict(pair, points=np.array(pair["points"]))
    inf["points"][2, 1] = np.inf
    got = ctx.bundle_adjust([bc.case("triple"), empty, no_edges, nan, bc.case("single"), only_fixed, inf, bc.case("pair")], bc.CAM)
    print("statuses", [g["status"] for g in got])
    assert [g["status"] for g in got] == [br.OK, br.EMPTY, br.NO_EDGES, br.NONFINITE, br.OK, br.NO_EDGES, br.NONFINITE, br.OK]
    for g, p in ((got[1], empty), (got[2], no_edges), (got[3], nan), (got[5], only_fixed), (got[6], inf)):
        assert g["poses"].tobytes() == np.asarray(p["poses"], np.float64).tobytes()
        assert g["points"].tobytes() == np.asarray(p["points"], np.float64).tobytes()
        assert not g["levels"].any() and not g["pose_stages"].any() and not g["point_stages"].any()
    assert br.bundle_adjust(dict(nan, cam=bc.CAM))["status"] == br.NONFINITE
    for g, n in ((got[0], "triple"), (got[4], "single"), (got[7], "pair")):
        assert same_bits(g, together[n]), n
