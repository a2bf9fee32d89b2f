"""The cases of tests/test_gpu_depth_measure.py, shared with tests/test_depth_measure_restatement_cpu.py: one candidate each through the
depth filter with a measured depth (tests/depth_measure_restatement.py).

Geometry.  A small camera, 24 x 16 pixels (fx = fy = 20, u0 12, v0 8), so that window strides of 8 and 16 (found levels 3 and 4) push
neighbours off the image.  A measured case is built FROM the measurement: the found pixel px and the depth sample z the image holds at its
centre give P_c = unproject(px) z / unproject(px).z, the current pose takes it to the world point P, and the candidate's bearing is the
direction of P from the reference camera.  The range of P along that bearing is known without the restatement: |ref P|.  The cases that
need the early return of Point::Update (norm_scale NaN) are depth_cases' own, on its camera, behind a depth image that is all holes: a
measured update cannot get there with inputs the entry accepts (tau is finite and sigma2 positive).

Every case names the call it can share a launch with (`group`): camera, lens, rule, noise and filter parameters belong to a call.

Test infrastructure only."""
import math

import numpy as np

import depth_cases as dcs
import depth_measure_restatement as dm
import depth_restatement as dr
import depth_seed_restatement as dsr
from depth_restatement import CONVERGED, DELETED, FIXED_STALE, NOT_FOUND, SKIPPED, UPDATED

W, H = 24, 16
CAM = dict(width=float(W), height=float(H), fx=20.0, fy=20.0, u0=12.0, v0=8.0)
PARAMS = dict(px_error_angle=dr.pixel_error_angle(CAM["fx"]), min_depth=0.25, scale_min_dist=0.25, max_failed=15)
NOISE = dict(noise_abs=0.004, noise_quad=0.002)             # explicit: no test rests on the defaults
LENS = (-0.25, 0.08, 0.002, -0.003, 0.01)
LENS_OUT = (0.6, 0.0, 0.0, 0.0, 0.0)                         # throws the image's corners off the raw grid
U16_SCALE = 1.0 / 5000


def ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def slanted(w=W, h=H):
    """a gently slanted surface: 1.5 m + 0.4 mm a column + 0.2 mm a row (a window of stride 16 spans 19 mm: no edge)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (1.5 + 0.0004 * xx + 0.0002 * yy).astype(np.float32)


_IMG = {}


def image(kind):
    if kind not in _IMG:
        f = slanted()
        if kind == "f32":
            d = f
        elif kind == "u16":
            d = np.round(f.astype(np.float64) * 5000).astype(np.uint16)
        elif kind == "hole":
            d = f.copy(); d[8, 12] = 0.0
        elif kind == "nan":
            d = f.copy(); d[8, 12] = np.nan
        elif kind == "few":
            d = f.copy()
            for dx, dy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
                d[8 + dy, 12 + dx] = 0.0
        elif kind == "edge":
            d = f.copy(); d[:, 13:] *= np.float32(1.2)
        elif kind == "edge4":                                 # a step that only a stride of 4 reaches
            d = f.copy(); d[:, 15:] *= np.float32(1.2)
        elif kind == "u16-hole":
            d = np.round(f.astype(np.float64) * 5000).astype(np.uint16); d[8, 12] = 0
        elif kind == "tum-holes":
            d = np.zeros((480, 640), np.float32)
        else:
            raise KeyError(kind)
        _IMG[kind] = ro(d)
    return _IMG[kind]


REF_Q, REF_C = dcs.quat((0.3, -0.5, 0.8), 0.2), (0.4, -0.2, 0.1)


def cur_pose_of(k=0, baseline=0.35):
    """current cameras beside the reference one, turned and rolled a little differently each"""
    q = dcs.quat_mul(dcs.quat((0.1 + 0.05 * k, 0.9, -0.2), 0.12 + 0.02 * k), REF_Q)
    c = (REF_C[0] + baseline * math.cos(0.7 * k), REF_C[1] + baseline * math.sin(0.7 * k), REF_C[2] - 0.05 * k * baseline / 0.35)
    return dcs.pose_of(q, c)


def measured_geometry(px, z, cur_pose, ref_pose=None):
    """-> dict(cur_pose, ref_pose, bearing, range, P): the candidate whose point is the one the sample z at px measures"""
    ref_pose = dcs.pose_of(REF_Q, REF_C) if ref_pose is None else ref_pose
    v = dr.unproject(CAM, px)
    k = z / v[2]
    P = dr.se3_apply(dr.se3_inverse(cur_pose), (v[0] * k, v[1] * k, v[2] * k))
    p_r = dr.se3_apply(ref_pose, P)
    rng = dr.norm3(p_r)
    return dict(cur_pose=cur_pose, ref_pose=ref_pose, bearing=(p_r[0] / rng, p_r[1] / rng, p_r[2] / rng), range=rng, P=P)


def centre_sample(kind, px, dist=None, scale=1.0):
    """the sample the restatement's centre names, whatever its status would be"""
    fu, fv = dm.centre(px, CAM, dist)
    return float(dsr.metres(image(kind), scale)[int(fv), int(fu)])


def case(name, purpose, kind, px, level, st, k=0, found=True, dist=None, rule=None, params=PARAMS, cam=CAM, group="plain", z_for_geometry=None,
         baseline=0.35, flip=False, layout="tight", **want):
    scale = U16_SCALE if kind is not None and kind.startswith("u16") else 1.0
    z = z_for_geometry
    if z is None:
        z = centre_sample(kind, px, dist, scale) if kind is not None else 1.5
        z = z if z == z and z > 0 else 1.5
    geo = measured_geometry(px, z, cur_pose_of(k, baseline))
    bearing = tuple(-c for c in geo["bearing"]) if flip else geo["bearing"]
    return dict(name=name, purpose=purpose, cur_pose=geo["cur_pose"], ref_pose=geo["ref_pose"], bearing=bearing, found=found, px=tuple(px), level=level,
                state=st, params=params, cam=cam, depth=None if kind is None else image(kind), kind=kind, dist=dist, scale=scale, rule=rule or {},
                noise_abs=NOISE["noise_abs"], noise_quad=NOISE["noise_quad"], group=group, range=geo["range"], layout=layout, want=want)


def inputs(c):
    return dict(cur_pose=c["cur_pose"], ref_pose=c["ref_pose"], bearing=c["bearing"], found=c["found"], px=c["px"], level=c["level"], cam=c["cam"],
                state=c["state"], params=c["params"], depth=c["depth"], dist=c["dist"], scale=c["scale"], rule=c["rule"], noise_abs=c["noise_abs"],
                noise_quad=c["noise_quad"])


def triangulated_inputs(c):
    """what depth_restatement.restate and Context.depth_filter take of the case"""
    return dict(cur_pose=c["cur_pose"], ref_pose=c["ref_pose"], bearing=c["bearing"], found=c["found"], px=c["px"], cam=c["cam"], state=c["state"],
                params=c["params"])


S = dcs.state


def _ok_cases():
    out = []
    # the states a candidate passes through, at sub-pixel positions whose rounding goes either way, levels 0 .. 3
    grid = [  # px, level, k, rho factor, sigma2, a, b, z_range, n_failed
        ((12.3, 7.6), 0, 0, 1.10, 1.0, 10.0, 10.0, 6.0, 0),
        ((12.6, 7.7), 0, 1, 0.90, 0.05, 12.0, 9.0, 6.0, 3),
        ((5.5, 3.5), 0, 2, 1.02, 1e-3, 40.0, 3.0, 2.5, 1),         # both coordinates on the half: rounded up
        ((20.49, 12.51), 1, 3, 0.97, 1e-2, 25.0, 30.0, 6.0, 0),
        ((11.2, 8.4), 2, 4, 1.30, 1.0, 1.0, 1.0, 6.0, 7),
        ((12.4, 8.2), 3, 5, 0.75, 0.3, 10.0, 14.0, 6.0, 0),          # stride 8: the row below the image is off it, six samples stay
        ((2.2, 13.9), 1, 6, 1.00, 1e-6, 300.0, 1.0, 2.5, 2),
        ((17.8, 2.1), 0, 7, 1.05, 1e-4, 150.0, 150.0, 6.0, 0),
    ]
    for i, (px, level, k, fac, sigma2, a, b, z_range, nf) in enumerate(grid):
        z = centre_sample("f32", px)
        geo = measured_geometry(px, z, cur_pose_of(k))
        st = S(fac / geo["range"], sigma2=sigma2, a=a, b=b, z_range=z_range, depth_mean=1.5, n_failed=nf)
        out.append(case("ok-%02d-level%d" % (i, level), "a measured update on level %d, rho %.2f of the truth, sigma2 %.1g" % (level, fac, sigma2), "f32", px,
                        level, st, k=k, updated=True, exact_range=True))
    # level 4: stride 16 leaves the centre alone -> FEW under the default rule, OK when one sample is enough
    z = centre_sample("f32", (12.3, 7.6))
    geo = measured_geometry((12.3, 7.6), z, cur_pose_of(1))
    st = S(1.1 / geo["range"], sigma2=0.2, depth_mean=1.5)
    out.append(case("few-level4", "stride 16 on 24 x 16: one sample of nine is on the image -> FEW, the triangulated update", "f32", (12.3, 7.6), 4, st, k=1,
                    status=dsr.FEW))
    out.append(case("ok-level4-min_valid1", "the same with min_valid 1: measured", "f32", (12.3, 7.6), 4, st, k=1, rule=dict(min_valid=1), group="min_valid1",
                    updated=True, exact_range=True))
    # an update that converges: a narrow prior at the truth
    px = (9.7, 6.2)
    geo = measured_geometry(px, centre_sample("f32", px), cur_pose_of(2))
    out.append(case("ok-converges", "a narrow prior at the measured range: l < 0.1 after the update", "f32", px, 0,
                    S(1.0 / geo["range"], sigma2=1e-5, a=30.0, b=8.0, depth_mean=1.5, n_failed=2), k=2, outcome=CONVERGED, exact_range=True))
    out.append(case("ok-wide-stays", "the seed state at the measured range: one update does not converge", "f32", px, 0,
                    S(1.0 / geo["range"], depth_mean=1.5), k=2, outcome=UPDATED, exact_range=True))
    # a point that is fixed already: Update and HasConverged still run, the position is the state's
    fixed_at = (0.123, -4.5, 7.25)
    out.append(case("ok-fixed", "fixed = 1: CONVERGED whatever l is, the position is state.position", "f32", px, 1,
                    S(1.2 / geo["range"], sigma2=0.5, position=fixed_at, fixed=1, depth_mean=1.5), k=2, outcome=CONVERGED, position=fixed_at))
    # no parallax at all: the triangulated rule would skip, the measured one updates
    out.append(case("ok-no-parallax", "the current camera 0.1 mm beside the reference one: no triangulation to guard, the update runs", "f32", (12.3, 7.6), 0,
                    S(1.1 / 1.5, sigma2=0.2, depth_mean=1.5), k=1, baseline=1e-4, updated=True, exact_range=True))
    # 16-bit
    for i, (px, level, k) in enumerate((((12.3, 7.6), 0, 0), ((6.6, 10.4), 1, 3), ((13.1, 7.9), 2, 5))):
        geo = measured_geometry(px, centre_sample("u16", px, scale=U16_SCALE), cur_pose_of(k))
        out.append(case("ok-u16-%d" % i, "a 16-bit image (1 / 5000 m a unit), level %d" % level, "u16", px, level,
                        S(0.95 / geo["range"], sigma2=0.02, a=14.0, b=10.5, depth_mean=1.5), k=k, updated=True, exact_range=True,
                        layout=("odd", "padded", "tight")[i]))
    return out


def _skipped_cases():
    out = []
    px = (12.3, 7.6)
    geo = measured_geometry(px, centre_sample("f32", px), cur_pose_of(1))
    out.append(case("skip-depth_mean", "range %.3g < depth_mean 8 x 0.25: SKIPPED" % geo["range"], "f32", px, 0,
                    S(1.0 / geo["range"], sigma2=0.1, depth_mean=8.0), k=1, outcome=SKIPPED))
    out.append(case("skip-min_depth", "range %.3g < min_depth 2: SKIPPED" % geo["range"], "f32", px, 0, S(1.0 / geo["range"], sigma2=0.1, depth_mean=1.5),
                    k=1, params=dict(PARAMS, min_depth=2.0), group="min_depth2", outcome=SKIPPED))
    # a candidate whose ray points away from what the sample measures: a negative range is skipped by the positive test itself, the
    # minimum-depth tests being set so low that they would let it pass
    out.append(case("skip-negative-range", "the bearing reversed: range %.3g, not positive, SKIPPED before the minimum-depth tests" % -geo["range"], "f32", px, 0,
                    S(1.0 / geo["range"], sigma2=0.1, depth_mean=-40.0), k=1, flip=True, params=dict(PARAMS, min_depth=-10.0), group="min_depth-10",
                    outcome=SKIPPED))
    return out


def _fallback_cases():
    """status not OK, or no image: the triangulated update of depth_restatement on a geometry that triangulates"""
    out = []
    st = S(1.0 / 1.45, sigma2=0.05, a=11.0, b=12.0, depth_mean=1.5, n_failed=4)
    c = (12.3, 7.6)
    out.append(case("hole-zero", "the centre sample is 0: HOLE", "hole", c, 0, st, k=1, status=dsr.HOLE))
    out.append(case("hole-nan", "the centre sample is NaN: HOLE", "nan", c, 1, st, k=2, status=dsr.HOLE))
    out.append(case("hole-u16", "a 16-bit zero: HOLE", "u16-hole", c, 0, st, k=3, status=dsr.HOLE, layout="odd"))
    out.append(case("few", "four of the eight neighbours are holes: FEW", "few", c, 0, st, k=1, status=dsr.FEW))
    out.append(case("edge", "a 20 % step beside the centre: EDGE", "edge", c, 0, st, k=4, status=dsr.EDGE))
    out.append(case("edge-stride4", "a 20 % step three columns away, found on level 2: EDGE by the stride", "edge4", c, 2, st, k=4, status=dsr.EDGE))
    out.append(case("edge-stride4-level0", "the same image found on level 0: the window stays on this side of the step", "edge4", c, 0, st, k=4, updated=True,
                    status=dsr.OK))
    out.append(case("outside-right", "px 23.7 rounds to column 24: OUTSIDE", "f32", (23.7, 8.2), 0, st, k=2, z_for_geometry=1.5, status=dsr.OUTSIDE))
    out.append(case("outside-bottom", "px 15.5 rounds to row 16: OUTSIDE", "f32", (11.0, 15.5), 0, st, k=2, z_for_geometry=1.5, status=dsr.OUTSIDE))
    out.append(case("no-job", "a hit whose request is in no job: no lookup", None, c, 0, st, k=1, status=dm.NO_LOOKUP))
    out.append(case("no-job-level3", "the same on level 3", None, (7.1, 9.3), 3, st, k=5, status=dm.NO_LOOKUP))
    # misses, with an image at hand that is never looked at
    for nf in (3, 15):
        gone = nf + 1 > 15
        out.append(case("miss-n_failed-%d" % nf, "Unpromote from n_failed = %d: %s" % (nf, "deleted" if gone else "kept"), "f32", c, 0,
                        S(0.5, sigma2=0.04, a=12.5, b=7.25, cos_alpha=0.99, last_distance=2.1, n_failed=nf), k=1, found=False,
                        outcome=NOT_FOUND | (DELETED if gone else 0), status=dm.NO_LOOKUP))
    return out


def _lens_cases():
    out = []
    for i, (px, level, k) in enumerate((((4.3, 3.6), 0, 0), ((19.6, 12.2), 0, 1), ((12.4, 8.3), 2, 2), ((3.2, 12.7), 1, 3))):
        z = centre_sample("f32", px, LENS)
        geo = measured_geometry(px, z, cur_pose_of(k))
        out.append(case("lens-ok-%d" % i, "through a lens: the centre is the raw pixel of px's ray", "f32", px, level,
                        S(1.05 / geo["range"], sigma2=0.05, depth_mean=1.5), k=k, dist=LENS, group="lens", updated=True, exact_range=True, status=dsr.OK))
    z = centre_sample("u16", (4.3, 3.6), LENS, U16_SCALE)
    geo = measured_geometry((4.3, 3.6), z, cur_pose_of(4))
    out.append(case("lens-ok-u16", "a 16-bit image through the lens", "u16", (4.3, 3.6), 0, S(1.05 / geo["range"], sigma2=0.05, depth_mean=1.5), k=4, dist=LENS,
                    group="lens", updated=True, exact_range=True, status=dsr.OK, layout="padded"))
    st = S(1.0 / 1.45, sigma2=0.05, depth_mean=1.5)
    out.append(case("lens-outside", "a lens that throws the corner's ray off the raw grid: OUTSIDE", "f32", (22.6, 14.8), 0, st, k=1, dist=LENS_OUT,
                    z_for_geometry=1.5, group="lens-out", status=dsr.OUTSIDE))
    out.append(case("lens-d0-zero", "d[0] == 0: no lens, whatever the other coefficients say", "f32", (4.3, 3.6), 0, st, k=1,
                    dist=(0.0, 0.5, 0.01, -0.02, 4.0), z_for_geometry=centre_sample("f32", (4.3, 3.6)), group="lens-d0", updated=True, exact_range=True,
                    status=dsr.OK))
    return out


def _early_return_cases():
    """depth_cases' three early returns of Point::Update (norm_scale NaN), on its camera, behind an image of holes: the triangulated rule"""
    out = []
    for name in ("early-return-skipped", "early-return-fixed-stale", "early-return-already-fixed"):
        found = [c for c in dcs.all_cases() if c["name"] == name]
        for c in found:
            out.append(dict(name="hole-" + name, purpose=c["purpose"] + "; behind a HOLE", cur_pose=c["cur_pose"], ref_pose=c["ref_pose"], bearing=c["bearing"],
                            found=True, px=tuple(c["px"]), level=0, state=c["state"], params=c["params"], cam=dcs.CAM, depth=image("tum-holes"), kind="tum-holes",
                            dist=None, scale=1.0, rule={}, noise_abs=NOISE["noise_abs"], noise_quad=NOISE["noise_quad"], group="tum", range=None,
                            layout="tight", want=dict(status=dsr.HOLE, outcome=c["want"]["outcome"], nan_norm_scale=True)))
    return out


_ALL = {}


def all_cases():
    if "cases" not in _ALL:
        _ALL["cases"] = _ok_cases() + _skipped_cases() + _fallback_cases() + _lens_cases() + _early_return_cases()
        names = [c["name"] for c in _ALL["cases"]]
        assert len(set(names)) == len(names)
    return _ALL["cases"]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def groups():
    """group -> its cases: what one call can take"""
    out = {}
    for c in all_cases():
        out.setdefault(c["group"], []).append(c)
    return out


_TOL = {}


def expected(c):
    """-> (the restatement's result, the bound per float output), computed once per case"""
    if c["name"] not in _TOL:
        _TOL[c["name"]] = dm.tolerance(**inputs(c))
    return _TOL[c["name"]]


def differences(c, got, with_row=True):
    """depth_cases.differences against this file's expectation"""
    want, bound = expected(c)
    bad, ratio = {}, {}
    for k in ("outcome", "n_failed", "status"):
        if got[k] != want[k]:
            bad[k] = (got[k], want[k], 0)
    gn, wn = dr._numbers(got), dr._numbers(want)
    if not with_row:
        gn, wn = ({k: v for k, v in d.items() if not k.startswith("row.")} for d in (gn, wn))
    for k in sorted(set(gn) | set(wn)):
        if k not in gn or k not in wn:
            bad[k] = (gn.get(k), wn.get(k), None)
        elif wn[k] != wn[k] or gn[k] != gn[k]:
            if not (wn[k] != wn[k] and gn[k] != gn[k]):
                bad[k] = (gn[k], wn[k], None)
        else:
            d = abs(gn[k] - wn[k])
            ratio[k] = d / bound[k] if bound[k] > 0 else (0.0 if d == 0 else math.inf)
            if d > bound[k]:
                bad[k] = (gn[k], wn[k], bound[k])
    for k in ("n_failed", "fixed", "trash") if with_row else ():
        if got["row"].get(k) != want["row"].get(k):
            bad["row." + k] = (got["row"].get(k), want["row"].get(k), 0)
    return bad, ratio


def check(c):
    """asserts, on the CPU, that the restatement takes the case where its name says"""
    base = dm.restate(**inputs(c))
    want = c["want"]
    if "status" in want:
        assert base["status"] == want["status"], (c["name"], base["status"], want["status"])
    if "outcome" in want:
        assert base["outcome"] == want["outcome"], (c["name"], base["outcome"], want["outcome"])
    if want.get("updated"):
        assert base["outcome"] in (UPDATED, CONVERGED) and base["status"] == dsr.OK, (c["name"], base["outcome"], base["status"])
    if "position" in want:
        assert base["position"] == tuple(want["position"]), (c["name"], base["position"])
    if base["status"] == dsr.OK:
        assert len(dm.spread_outcomes(**inputs(c))) == 1, (c["name"], "the outcome depends on the last bits of exp")
    if want.get("nan_norm_scale"):
        t = base["trace"]
        assert t["norm_scale"] != t["norm_scale"], (c["name"], t)
    return base
