"""The ORACLE's depth filter (sdvl_ref_depth_filter: the loop body of Tracker::UpdateCandidates with PointUpdate, PointHasConverged and
PointUnpromote, oracle/ref_tracker.h) against the pure-Python restatement written from the reference's text
(tests/depth_restatement.py), on every case of tests/depth_cases.py.  The oracle is what the existing filter tests hold the device
against (test_depth_filter_behind_the_search_matches_oracle, test_gpu_forms.check_search_points_filter); until now nothing held the
oracle itself, and its outcome in the early-return branch of Point::Update was 2 or 3 where include/sdvl_hip.h says 1 or 4.

Both sides call the host's libm, so the two differ only where the oracle's vector algebra (oracle/ref_math.h) orders an operation
otherwise than the restatement; the comparison nevertheless allows what a device result is allowed (depth_cases.differences: the
per-case, per-output bound of depth_restatement.tolerance) and prints the largest ratio met (run with -s).  Outcomes, n_failed and
the fixed flag are exact."""
import pytest

import depth_cases as dc
from depth_restatement import CONVERGED, FIXED_STALE, UPDATED
from oraclelib import TUM_CAM

NAMES = [c["name"] for c in dc.all_cases()]
_w = {"ratio": {}}


@pytest.fixture(scope="module")
def ref(orc):
    assert tuple(TUM_CAM) == (dc.CAM["fx"], dc.CAM["fy"], dc.CAM["u0"], dc.CAM["v0"]) and orc.params.max_failed == dc.PARAMS["max_failed"]
    t = orc.tracker(int(dc.CAM["width"]), int(dc.CAM["height"]), TUM_CAM)
    yield t                       # map_scale 1 and scale_min_dist 0.25 are the tracker's own: min_depth = 0.25
    t.close()


def oracle_result(ref, c):
    s = c["state"]
    st0 = [s["rho"], s["sigma2"], s["a"], s["b"], s["z_range"], s["cos_alpha"], s["last_distance"], *s["position"], float(s["fixed"]), float(s["n_failed"])]
    # min_depth is the tracker's map_scale * scale_min_dist: a case with a min_depth of its own sets the map scale that gives it
    scale = c["params"]["min_depth"] / 0.25
    assert scale * 0.25 == c["params"]["min_depth"] and c["params"]["scale_min_dist"] == 0.25 and c["params"]["max_failed"] == dc.PARAMS["max_failed"]
    ref.use_mapper(True, map_scale=scale, scale_min_dist=0.25)
    rc, st = ref.depth_filter(c["cur_pose"], c["ref_pose"], c["bearing"], c["found"], c["px"], s["depth_mean"], st0)
    told = rc in (UPDATED, CONVERGED, FIXED_STALE)
    got = dict(outcome=rc, n_failed=int(st[11]), rho=float(st[0]), sigma2=float(st[1]), a=float(st[2]), b=float(st[3]),
               cos_alpha=float(st[5]) if told else None, last_distance=float(st[6]) if told else None,
               position=tuple(float(v) for v in st[7:10]) if rc in (CONVERGED, FIXED_STALE) else None, row={})
    return got, st, st0


@pytest.mark.parametrize("name", NAMES)
def test_oracle_depth_filter_equals_restatement(ref, name):
    c = dc.by_name(name)
    want, _ = dc.expected(c)
    got, st, st0 = oracle_result(ref, c)
    # the oracle keeps the position of a point that has not converged in its estimate, not in p3d: nothing to compare for UPDATED
    bad, ratio = dc.differences(c, got, with_row=False, skip=("position0", "position1", "position2") if got["outcome"] == UPDATED else ())
    for k, r in ratio.items():
        if r > _w["ratio"].get(k, (0.0, None))[0]:
            _w["ratio"][k] = (r, name)
    assert not bad, (name, bad)
    assert bool(st[10]) == (bool(c["state"]["fixed"]) or want["outcome"] in (CONVERGED, FIXED_STALE))
    assert st[4] == c["state"]["z_range"]
    if want["outcome"] not in (UPDATED, CONVERGED):
        # a miss changes b and n_failed, a skip and an early return nothing; p3d appears only where the point becomes fixed
        keep = [i for i in range(12) if not (want["outcome"] == FIXED_STALE and i in (7, 8, 9, 10))]
        same = [i for i in keep if not (not c["found"] and i in (3, 11))]
        assert all(st[i] == st0[i] for i in same), (name, list(st), st0)
    if want["outcome"] == CONVERGED and c["state"]["fixed"]:
        assert tuple(st[7:10]) == c["state"]["position"]


def test_oracle_early_return_outcomes_are_the_headers(ref):
    """the early return of Point::Update: SKIPPED (1) when HasConverged says no, FIXED_STALE (4) when it says yes: before this change the
    wrapper answered 2 and 3 there"""
    early = [c for c in dc.all_cases() if c["want"].get("regime") == "early-return"]
    assert len(early) == 3
    got = sorted(oracle_result(ref, c)[0]["outcome"] for c in early)
    assert got == [1, 4, 4]


def test_worst_ratios_are_reported():
    print()
    for k, (r, name) in sorted(_w["ratio"].items()):
        print("oracle vs restatement, %-13s largest deviation / bound %.3g (%s)" % (k, r, name))
    assert not _w["ratio"] or max(r for r, _ in _w["ratio"].values()) <= 1.0
