"""tests/depth_restatement.py and tests/depth_cases.py without a GPU: micro-cases whose answers are written out here, every case
checked to be what its name says (branch, side of the threshold, regime of tau, with the margins depth_cases states), the planted
faults, and, where mpmath imports, the restatement's float64 arithmetic against the same formulas at 60 digits.

Measured 2026-10-20 over the 53 cases (the figures are printed by the tests, run with -s):
* The early return of Point::Update IS reached on valid inputs: the 31st geometry of the search in depth_cases._early_return_cases is
  the second whose v.t / |t| rounds to 1 + 2^-52; three cases stand on the two (SKIPPED, FIXED_STALE through l < 0.1, FIXED_STALE of a
  point fixed already).
* float64 against 60 digits, largest relative error: sigma2 2.2e-7 (regular-04: a prior of 1e-9, the three terms of point.cc:90
  cancel), rho, last_distance and position 6.9e-11 (negative-tau-1.50mrad: gamma_plus is 4e-4 and comes from PI), a and b 3.8e-12
  (regular-03, a + b = 301), cos_alpha 3.8e-16.  Largest error / error_bound: 0.60 (rho, negative-tau-1.50mrad), 0.07 for sigma2,
  below 0.01 for a and b.
* Planted faults, cases that separate each: miss_b_kept 4, delete_ge 1, tau_inverse_pose 40, no_clamp 4, no_depth_mean_test 1,
  exact_pi 36, position_old_rho 34, fixed_recomputed 3, n_failed_kept 16, converge_prev_cos 2, row_std_sigma2 39,
  row_fixed_on_updated 27, row_trash_every_miss 2.  WITNESS names the one
  that is asserted."""
import math

import pytest

import depth_cases as dc
import depth_restatement as dr
from depth_restatement import CONVERGED, DELETED, FIXED_STALE, NOT_FOUND, SKIPPED, UPDATED

NAMES = [c["name"] for c in dc.all_cases()]
# the case that is asserted to separate each planted fault (any one would do)
WITNESS = {
    "miss_b_kept": "miss-n_failed-0", "delete_ge": "miss-n_failed-14", "tau_inverse_pose": "regular-05", "no_clamp": "tau-clamp-2.40mrad",
    "no_depth_mean_test": "too-close-depth_mean-below", "exact_pi": "regular-03", "position_old_rho": "regular-09",
    "fixed_recomputed": "convergence-fixed-wide", "n_failed_kept": "regular-04", "converge_prev_cos": "convergence-l-above",
    "row_std_sigma2": "regular-07", "row_fixed_on_updated": "convergence-l-above", "row_trash_every_miss": "miss-n_failed-0",
}
ID = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------- written-out answers
def right_triangle(**st):
    """reference camera at the origin looking along z, the point on its axis at depth 1, the current camera one unit to the right and
    not rotated: the rays meet under 45 degrees.  alpha = 90, beta = 45 degrees, so with eps the pixel-error angle and PI the
    reference's constant, tau = sin(pi/4 + eps) / sin(PI - 3 pi/4 - eps) - 1"""
    cur = (1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0)
    px = (dc.CAM["u0"] - dc.CAM["fx"], dc.CAM["v0"])                     # (-1, 0, 1) in the current camera
    return dict(cur_pose=cur, ref_pose=ID, bearing=(0.0, 0.0, 1.0), found=True, px=px, cam=dc.CAM, params=dc.PARAMS, state=dc.state(**st))


def test_micro_right_triangle_update():
    o = dr.restate(**right_triangle(rho=1.0, sigma2=1.0, a=10.0, b=10.0, z_range=6.0, n_failed=4))
    t = o["trace"]
    eps = dc.PARAMS["px_error_angle"]
    assert eps == pytest.approx(2.0 * math.atan(1.0 / (2.0 * 517.3)), rel=1e-15) and 1.93e-3 < eps < 1.94e-3
    assert t["det"] == pytest.approx(0.5, abs=1e-15) and t["depth"] == pytest.approx(1.0, abs=1e-15)
    assert t["cos_alpha_tri"] == pytest.approx(math.sqrt(0.5), abs=1e-15)
    assert t["alpha"] == pytest.approx(math.pi / 2, abs=1e-15) and t["beta"] == pytest.approx(math.pi / 4, abs=1e-15)
    tau = math.sin(math.pi / 4 + eps) / math.sin(3.14159265 - 0.75 * math.pi - eps) - 1.0
    assert t["tau"] == pytest.approx(tau, rel=1e-12) and not t["clamped"]
    # the reference's PI is 3.6e-9 short: tau is 2 tan(eps) / (1 - tan(eps)) plus that much, not closer
    ideal = 2.0 * math.tan(eps) / (1.0 - math.tan(eps))
    assert 3e-9 < t["tau"] - ideal < 4e-9
    # the measurement equals rho: m = rho = 1, both weights leave rho where it is; sigma2 = C1 s2 + C2 sigma2
    tau_inv = 0.5 * (1.0 / (1.0 - tau) - 1.0 / (1.0 + tau))
    tau2 = tau_inv * tau_inv
    s2 = tau2 / (1.0 + tau2)
    c1 = 0.5 / (math.sqrt(1.0 + tau2) * math.sqrt(2.0 * 3.14159265))
    c2 = 0.5 / 6.0
    c1, c2 = c1 / (c1 + c2), c2 / (c1 + c2)
    assert o["rho"] == pytest.approx(1.0, abs=1e-15)
    assert o["sigma2"] == pytest.approx(c1 * s2 + c2 * 1.0, rel=1e-12)
    f = c1 * 11.0 / 21.0 + c2 * 10.0 / 21.0
    e = c1 * 11.0 * 12.0 / (21.0 * 22.0) + c2 * 10.0 * 11.0 / (21.0 * 22.0)
    a = (e - f) / (f - e / f)
    assert o["a"] == pytest.approx(a, rel=1e-10) and o["b"] == pytest.approx(a * (1.0 - f) / f, rel=1e-10)
    assert o["position"] == pytest.approx((0.0, 0.0, 1.0), abs=1e-15)
    assert o["cos_alpha"] == pytest.approx(math.sqrt(0.5), abs=1e-15) and o["last_distance"] == pytest.approx(math.sqrt(2.0), abs=1e-15)
    # l = 4 sqrt(sigma2) cos_alpha / last_distance = 2 sqrt(sigma2), far above 0.1
    assert t["l"] == pytest.approx(2.0 * math.sqrt(o["sigma2"]), rel=1e-12) and o["outcome"] == UPDATED and o["n_failed"] == 0
    assert o["row"] == dict(P=o["position"], idepth=o["rho"], idepth_std=math.sqrt(o["sigma2"]), n_failed=0)


def test_micro_right_triangle_converges_with_a_narrow_prior():
    o = dr.restate(**right_triangle(rho=1.0, sigma2=1e-4))
    assert o["outcome"] == CONVERGED and o["trace"]["l"] < 2.0 * math.sqrt(1e-4) and o["row"]["fixed"] == 1
    assert o["sigma2"] < 1e-4                                           # a measurement at the mean narrows the posterior


def test_micro_miss():
    for nf, gone in ((0, False), (14, False), (15, True), (16, True)):
        st = dc.state(0.5, sigma2=0.04, a=12.5, b=7.25, n_failed=nf)
        o = dr.restate(cur_pose=ID, ref_pose=ID, bearing=(0.0, 0.0, 1.0), found=False, px=(0.0, 0.0), cam=dc.CAM, params=dc.PARAMS, state=st)
        assert (o["outcome"], o["n_failed"], o["b"]) == (NOT_FOUND | (DELETED if gone else 0), nf + 1, 8.25)
        assert (o["rho"], o["sigma2"], o["a"]) == (0.5, 0.04, 12.5) and o["position"] is None and o["cos_alpha"] is None
        assert o["row"] == (dict(n_failed=nf + 1, trash=True) if gone else dict(n_failed=nf + 1))


def test_micro_guards():
    base = right_triangle(rho=1.0)
    # the found pixel on the reference ray's own direction: no triangulation
    o = dr.restate(**dict(base, px=(dc.CAM["u0"], dc.CAM["v0"])))
    assert o["outcome"] == SKIPPED and o["trace"]["det"] == 0.0 and o["row"] == {}
    # a baseline of 1e-3 at depth 1: parallax 1e-3 rad, cos_alpha 1 - 5e-7 >= 0.999999
    near = dict(base, cur_pose=(1.0, 0.0, 0.0, 0.0, -1e-3, 0.0, 0.0), px=(dc.CAM["u0"] - dc.CAM["fx"] * 1e-3, dc.CAM["v0"]))
    o = dr.restate(**near)
    assert o["outcome"] == SKIPPED and (o["trace"]["det"] < 0.000001 or o["trace"]["cos_alpha_tri"] >= 0.999999)
    # depth 1 against depth_mean 4.1 * 0.25
    o = dr.restate(**dict(base, state=dc.state(1.0, depth_mean=4.1)))
    assert o["outcome"] == SKIPPED and o["trace"]["depth"] == pytest.approx(1.0, abs=1e-15) and "tau" not in o["trace"]
    o = dr.restate(**dict(base, state=dc.state(1.0, depth_mean=3.9)))
    assert o["outcome"] == UPDATED


def test_ulps_move_each_transcendental_result_and_nothing_else():
    kw = right_triangle(rho=0.7, sigma2=0.01)          # 3 sigma from the measurement: C1 and C2 both count
    base = dr.restate(**kw)
    for j, name in enumerate(dr.TRANSCENDENTALS):
        ul = tuple(3 if i == j else 0 for i in range(5))
        o = dr.restate(ulps=ul, **kw)
        assert (o["trace"]["det"], o["trace"]["depth"], o["trace"]["cos_alpha_tri"]) == (base["trace"]["det"], base["trace"]["depth"], base["trace"]["cos_alpha_tri"])
        moved = ("C1", o["trace"]["C1"], base["trace"]["C1"]) if name == "exp" else ("tau", o["trace"]["tau"], base["trace"]["tau"])
        assert moved[1] != moved[2], (name, moved)
        assert (o["trace"]["tau"] == base["trace"]["tau"]) == (name == "exp")
        if name == "acos_alpha":
            assert o["trace"]["alpha"] == base["trace"]["alpha"] + 3 * math.ulp(base["trace"]["alpha"])
    assert dr._moved(1.0, -2) == 1.0 - 2.0 ** -52 and dr._moved(1.0, 2) == 1.0 + 2.0 ** -51 and dr._moved(math.inf, 3) == math.inf


# ---------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_says(name):
    dc.check(dc.by_name(name))


def test_the_cases_cover_what_they_are_there_for():
    cases = dc.all_cases()
    res = {c["name"]: dr.restate(**dc.inputs(c)) for c in cases}
    names = set(res)
    assert {"miss-n_failed-%d" % n for n in (0, 14, 15, 16)} <= names
    for stem in ("no-triangulation-det", "too-close-min_depth", "too-close-depth_mean", "convergence-l"):
        assert {stem + "-below", stem + "-above"} <= names
    assert {"no-parallax-skipped", "no-parallax-passes", "convergence-fixed-wide", "convergence-fixed-narrow"} <= names
    regimes = [c["want"].get("regime") for c in cases]
    assert regimes.count("negative-tau") >= 2 and regimes.count("clamp") >= 2 and regimes.count("regular") >= 12
    reg = [c for c in cases if c["want"].get("regime") == "regular"]
    phis = [math.acos(res[c["name"]]["trace"]["cos_alpha_tri"]) for c in reg]
    assert min(phis) < 1.01e-2 and max(phis) > 0.299
    assert {c["state"]["sigma2"] for c in reg} == {1.0, 1e-3, 1e-6, 1e-9}
    assert min(c["state"]["a"] for c in reg) == 1.0 and max(c["state"]["a"] for c in reg) == 300.0
    assert min(c["state"]["b"] for c in reg) == 1.0 and max(c["state"]["b"] for c in reg) == 300.0
    assert max(c["state"]["a"] + c["state"]["b"] for c in reg) == 600.0
    assert len({c["state"]["z_range"] for c in reg}) == 2
    ks = {round((c["state"]["rho"] - res[c["name"]]["trace"]["x"]) / math.sqrt(c["state"]["sigma2"]), 6) for c in reg}
    assert ks == {0.3, 1.0, 3.0, 10.0}
    assert min(res[c["name"]]["trace"]["C1"] for c in reg) < 1e-20          # 10 sigma from rho with a wide prior: C1 vanishes
    assert any(c["ref_pose"][:4] != ID[:4] and c["cur_pose"][:4] != ID[:4] for c in reg)
    # the early return is reached, with both results
    early = [c for c in cases if c["want"].get("regime") == "early-return"]
    assert {res[c["name"]]["outcome"] for c in early} == {SKIPPED, FIXED_STALE}, "the early return of Point::Update was not reached"
    assert any(res[c["name"]]["outcome"] == FIXED_STALE and not c["state"]["fixed"] for c in early)
    # the sequence: twelve updates, each from the restatement's previous output, converged by the last one alone
    seq = dc.sequence()
    assert len(seq) == dc.SEQUENCE_STEPS == 12
    assert [res[c["name"]]["outcome"] for c in seq] == [UPDATED] * 11 + [CONVERGED]
    for prev, nxt in zip(seq, seq[1:]):
        o = res[prev["name"]]
        assert tuple(nxt["state"][k] for k in ("rho", "sigma2", "a", "b", "cos_alpha", "last_distance")) == tuple(o[k] for k in ("rho", "sigma2", "a", "b", "cos_alpha", "last_distance"))
    assert abs(1.0 / res[seq[-1]["name"]]["rho"] - 2.5) < 1e-3                # seeded at 2.9, the point lies at 2.5
    outcomes = {o["outcome"] for o in res.values()}
    assert outcomes == {NOT_FOUND, NOT_FOUND | DELETED, SKIPPED, UPDATED, CONVERGED, FIXED_STALE}


def test_fixed_points_keep_their_position_bit_for_bit():
    for name in ("convergence-fixed-wide", "convergence-fixed-narrow", "early-return-already-fixed"):
        c = dc.by_name(name)
        want, bound = dc.expected(c)
        assert want["position"] == c["state"]["position"] and want["row"]["P"] == c["state"]["position"]
        # no transcendental behind the position, cos_alpha and last_distance of a fixed point: the floor of 8 ulp alone
        for k in ("position0", "position1", "position2") + (("cos_alpha", "last_distance") if want["outcome"] == CONVERGED else ()):
            v = dr._numbers(want)[k]
            assert bound[k] == dr.FLOOR_ULP * math.ulp(v), (name, k)


# ---------------------------------------------------------------------------------------------------- planted faults
@pytest.mark.parametrize("fault", sorted(dr.FAULTS))
def test_every_planted_fault_is_separated(fault):
    hits = [c["name"] for c in dc.all_cases() if dc.differences(c, dr.restate(fault=fault, **dc.inputs(c)))[0]]
    print("\n%s: separated by %d cases: %s" % (fault, len(hits), ", ".join(hits[:6]) + (" ..." if len(hits) > 6 else "")))
    assert WITNESS[fault] in hits, (fault, hits)


def test_no_fault_means_no_difference():
    for c in dc.all_cases():
        bad, ratio = dc.differences(c, dr.restate(**dc.inputs(c)))
        assert not bad and all(r == 0.0 for r in ratio.values()), c["name"]
    assert set(WITNESS) == set(dr.FAULTS)


# ---------------------------------------------------------------------------------------------------- 60 digits
def exact(c, mp):
    """the formulas of an update (found, every guard passed) in mpmath at the working precision, from the case's float inputs taken
    exactly -> dict of rho, sigma2, a, b, cos_alpha, last_distance, position0..2 and the quantities the error bound is made from"""
    m = mp.mpf

    def rot(q):
        w, x, y, z = q
        return ((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)), (2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)),
                (2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)))

    def mv(R, v):
        return tuple(sum(R[i][j] * v[j] for j in range(3)) for i in range(3))

    def inv(T):
        q = T[:4]
        n2 = sum(c * c for c in q)
        r = (q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2)
        return r + tuple(-c for c in mv(rot(r), T[4:]))

    def mul(A, B):
        a0, a1, a2, a3 = A[:4]
        b0, b1, b2, b3 = B[:4]
        q = (a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2, a0 * b2 + a2 * b0 + a3 * b1 - a1 * b3,
             a0 * b3 + a3 * b0 + a1 * b2 - a2 * b1)
        n = mp.sqrt(sum(c * c for c in q))
        return tuple(c / n for c in q) + tuple(A[4 + i] + mv(rot(A[:4]), B[4:])[i] for i in range(3))

    def app(T, p):
        return tuple(mv(rot(T[:4]), p)[i] + T[4 + i] for i in range(3))

    def norm(v):
        return mp.sqrt(sum(c * c for c in v))

    def par(s1, s2, p):
        v1, v2 = tuple(a - b for a, b in zip(s1, p)), tuple(a - b for a, b in zip(s2, p))
        return sum(a * b for a, b in zip(v1, v2)) / (norm(v1) * norm(v2))

    cur, ref, fv = tuple(m(v) for v in c["cur_pose"]), tuple(m(v) for v in c["ref_pose"]), tuple(m(v) for v in c["bearing"])
    st = {k: (m(v) if isinstance(v, float) else v) for k, v in c["state"].items()}
    PI = m(3.14159265)
    pose = mul(cur, inv(ref))
    v = ((m(c["px"][0]) - m(dc.CAM["u0"])) / m(dc.CAM["fx"]), (m(c["px"][1]) - m(dc.CAM["v0"])) / m(dc.CAM["fy"]), m(1))
    a1 = tuple(x / norm(v) for x in v)
    a0 = mv(rot(pose[:4]), fv)
    m00, m01, m11 = sum(x * x for x in a0), sum(x * y for x, y in zip(a0, a1)), sum(x * x for x in a1)
    det = m00 * m11 - m01 * m01
    t = pose[4:]
    depth = abs(-(m11 * sum(x * y for x, y in zip(a0, t)) - m01 * sum(x * y for x, y in zip(a1, t))) / det)
    ref_world, cur_world = inv(ref), inv(cur)
    pose2 = mul(ref, inv(cur))
    t2 = pose2[4:]
    av = tuple(fv[i] * depth - t2[i] for i in range(3))
    alpha = mp.acos(sum(x * y for x, y in zip(fv, t2)) / norm(t2))
    beta = mp.acos(-sum(x * y for x, y in zip(av, t2)) / (norm(t2) * norm(av)))
    beta_plus = beta + m(c["params"]["px_error_angle"])
    gamma_plus = PI - alpha - beta_plus
    depth_plus = norm(t2) * mp.sin(beta_plus) / mp.sin(gamma_plus)
    tau = depth_plus - depth
    gap = depth - tau
    tau_inverse = (1 / (gap if gap > m("0.0000001") else m(0.0000001)) - 1 / (depth + tau)) / 2
    tau2 = tau_inverse * tau_inverse
    x = 1 / depth
    ns = mp.sqrt(st["sigma2"] + tau2)
    s2 = 1 / (1 / st["sigma2"] + 1 / tau2)
    mm = s2 * (st["rho"] / st["sigma2"] + x / tau2)
    expo = -(x - st["rho"]) ** 2 / (2 * ns * ns)
    C1 = st["a"] / (st["a"] + st["b"]) * mp.exp(expo) / (ns * mp.sqrt(2 * PI))
    C2 = st["b"] / (st["a"] + st["b"]) / st["z_range"]
    C1, C2 = C1 / (C1 + C2), C2 / (C1 + C2)
    a, b = st["a"], st["b"]
    f = C1 * (a + 1) / (a + b + 1) + C2 * a / (a + b + 1)
    e = C1 * (a + 1) * (a + 2) / ((a + b + 1) * (a + b + 2)) + C2 * a * (a + 1) / ((a + b + 1) * (a + b + 2))
    rho = C1 * mm + C2 * st["rho"]
    sigma2 = C1 * (s2 + mm * mm) + C2 * (st["sigma2"] + st["rho"] ** 2) - rho * rho
    a_new = (e - f) / (f - e / f)
    b_new = a_new * (1 - f) / f
    pos = tuple(m(p) for p in c["state"]["position"]) if c["state"]["fixed"] else app(ref_world, tuple(fv[i] / rho for i in range(3)))
    out = dict(rho=rho, sigma2=sigma2, a=a_new, b=b_new, cos_alpha=par(ref_world[4:], cur_world[4:], pos),
               last_distance=norm(tuple(cur_world[4 + i] - pos[i] for i in range(3))), position0=pos[0], position1=pos[1], position2=pos[2])
    # where rounding is amplified: the two subtractions that make tau (gamma_plus from PI, tau from depth_plus), the exponent, and
    # the three differences of the posterior
    k_tau = (abs(depth_plus) + depth) / abs(tau) * (1 + PI / abs(mp.tan(gamma_plus)) + PI / abs(mp.tan(beta_plus)) + 1 / mp.sqrt(1 - mp.cos(alpha) ** 2)
                                                    + 1 / mp.sqrt(1 - mp.cos(beta) ** 2))
    clamped = not gap > m("0.0000001")
    k_tau2 = k_tau * abs(tau) * ((0 if clamped else 1 / gap ** 2) + 1 / (depth + tau) ** 2) / abs(tau_inverse)      # d log tau2 / d log tau
    cond = dict(tau=k_tau, tau2=k_tau2 * (1 + abs(expo)),
                sigma2=(abs(C1 * (s2 + mm * mm)) + abs(C2 * (st["sigma2"] + st["rho"] ** 2)) + rho * rho) / abs(sigma2),
                a=(abs(e) + abs(f)) / abs(e - f) + (abs(f) + abs(e / f)) / abs(f - e / f))
    return out, cond


U = 2.0 ** -53
K_OPS = 64          # roundings that add up along the longest path of the update (the pose products in front of it included)


def error_bound(value, cond, key):
    """relative float64 error allowed on an output: K_OPS roundings, amplified first by the cancellations that make tau2 (gamma_plus
    from PI, tau from depth_plus; every later quantity depends on tau2 with a sensitivity of at most 1 + |exponent|), then by the
    output's own cancellation, which the error brought in by tau2 passes through as well (sigma2: the three terms of point.cc:90
    against their sum; a and b: e - f and f - e / f)"""
    own = cond["sigma2"] if key == "sigma2" else cond["a"] if key in ("a", "b") else 1
    return K_OPS * U * float((1 + cond["tau2"]) * own)


def test_float64_error_against_60_digits():
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    worst, worst_ratio = {}, {}
    with mp.workdps(60):
        for c in dc.all_cases():
            want = dr.restate(**dc.inputs(c))
            if want["outcome"] not in (UPDATED, CONVERGED):
                continue
            ex, cond = exact(c, mp)
            got = dr._numbers(want)
            for k, v in ex.items():
                if c["state"]["fixed"] and k.startswith("position"):
                    assert got[k] == float(v)
                    continue
                scale = abs(v) if not k.startswith("position") else max(abs(ex["position%d" % i]) for i in range(3))
                rel = float(abs(mp.mpf(got[k]) - v) / scale)
                key = "position" if k.startswith("position") else k
                bound = error_bound(v, cond, key)
                if rel > worst.get(key, (0.0,))[0]:
                    worst[key] = (rel, c["name"])
                if rel / bound > worst_ratio.get(key, (0.0,))[0]:
                    worst_ratio[key] = (rel / bound, c["name"], rel, bound)
                assert rel <= bound, (c["name"], k, rel, bound, {q: float(x) for q, x in cond.items()})
    print()
    for k in worst:
        print("float64 vs 60 digits, %-13s worst relative error %.2e (%s); worst error / bound %.3f (%s: %.2e of %.2e)"
              % (k, worst[k][0], worst[k][1], worst_ratio[k][0], worst_ratio[k][1], worst_ratio[k][2], worst_ratio[k][3]))
    assert set(worst) == {"rho", "sigma2", "a", "b", "cos_alpha", "last_distance", "position"}
