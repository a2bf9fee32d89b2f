"""The named inputs of the sparse image alignment (ImageAlign::ComputePose, image_align.cc:46-267) that
tests/test_oracle_align_independent.py and tests/test_gpu_align.py share: reference keyframes away from the world frame (rolled 30
and 90 degrees, tilted 25, zoomed 0.6 and 1.9), a tilted scene plane, features that leave the current image during the iterations,
at a level's first evaluation or only later, a start 0.2 m and 0.1 rad off, every level range, iteration limits of 1 and 2, both
branches of a fast call, a start that measures nothing, a band of features that no coarse level sees (the sticky stop), flat
images, depths scaled by 0.02, 50, -1 and 0, points behind and exactly on the current camera plane, and frames whose level widths
are no multiples of 4.

A case is a function of its seed: CASES[name]() -> a spec; case(name) adds what follows from it without rendering (poses, features);
frames(synth, c) renders its two frames, once per view and session.  Nothing here calls the oracle.

Poses are world -> camera (q, t).  T_rel = T_cur * T_ref^-1 is what the job receives (image_align.cc:66), and the start is
Exp(pert) * T_rel unless the spec gives `start` itself.  Features are pixels of the REFERENCE frame intersected with the scene
plane in the reference camera's frame: bearing = the pixel's unit ray, depth = the distance of the point from the reference
camera's centre (image_align.cc:159-160), every 17th feature without a live point.

Admission.  A seed is committed only if the oracle's n_meas, its and stop do not change when the start pose and the depths move one
ulp up and one ulp down (test_oracle_align_independent.py::test_every_case_is_stable_on_the_oracle runs that screen on every case).
Every case below carries the first seed tried, 1: none was discarded.

`one_eval` cases (max_its = 1 on one level) are those whose surface has no minimum (points behind the camera, a flat current
image, scaled depths): the oracle wanders for a dozen steps and more there and reduction order decides where it ends, so they are
held to one evaluation."""
import numpy as np

from oraclelib import EUROC_CAM, TUM_CAM, WARP_VIEWS, XI
from pose_restatement import SE3_IDENTITY, quat_to_rot, se3_exp, se3_mul

SMALL_CAM = np.array([268.0, 267.5, 163.7, 127.2])     # a 330x250 frame: level widths 165, 82, 41
PLANE = (0.0, 0.0, 1.0, 2.0)
TILTED = (0.5, 0.1, 0.86, 2.0)
PERT = np.array([0.01, -0.01, 0.005, 0.002, 0.002, -0.004])
DEFAULTS = dict(max_level=4, min_level=2, max_its=30)   # Config::MaxAlignLevel, MinAlignLevel, MaxImgAlignIts (config.cc)
ZERO6 = np.zeros(6)


def se3_inv(T):
    q = np.array([T[0], -T[1], -T[2], -T[3]])
    return np.concatenate([q, -(quat_to_rot(q) @ T[4:])])


def interior(w, h, n, rng, margin=48):
    return np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1)


def near_border(w, h, n, rng, lo=14.0, hi=40.0):
    """half of the features lo to hi pixels from one of the four borders, half inside"""
    side = np.arange(n) % 8
    near = rng.uniform(lo, hi, n)
    xs = np.select([side == 0, side == 1, side >= 4], [near, w - near, rng.uniform(60, w - 60, n)], rng.uniform(lo + 6, w - lo - 6, n))
    ys = np.select([side == 2, side == 3, side >= 4], [near, h - near, rng.uniform(60, h - 60, n)], rng.uniform(lo + 6, h - lo - 6, n))
    return np.stack([xs, ys], 1)


def band(w, h, n, rng, lo=26.0, hi=46.0):
    """every feature lo to hi pixels from a border: visible at levels 2 and 3 (borders of 12 and 24 pixels), at level 4 (48) none"""
    side = np.arange(n) % 4
    near = rng.uniform(lo, hi, n)
    xs = np.select([side == 0, side == 1], [near, w - near], rng.uniform(lo, w - lo, n))
    ys = np.select([side == 2, side == 3], [near, h - near], rng.uniform(lo, h - lo, n))
    return np.stack([xs, ys], 1)


def edge_pixels(w, h, levels, n_inside, rng):
    """per level, 16 features a thousandth of a level pixel on either side of the border tests (ui - 3 < 0, ui + 3 >= W of
    PrecomputePatches and the same two of ComputeResiduals) on all four sides, as test_gpu_forms.edge_features places them, and
    n_inside features inside"""
    pts, eps = [], 1e-3
    for level in levels:
        s = float(1 << level)
        lw, lh = w >> level, h >> level
        for x in (3 - eps, 3 + eps, lw - 3 - eps, lw - 3 + eps):
            pts += [(x * s, rng.uniform(8, lh - 8) * s) for _ in range(2)]
        for y in (3 - eps, 3 + eps, lh - 3 - eps, lh - 3 + eps):
            pts += [(rng.uniform(8, lw - 8) * s, y * s) for _ in range(2)]
    m = 3 * (1 << max(levels)) + 8
    return np.concatenate([np.array(pts), interior(w, h, n_inside, rng, margin=m)])


def _spec(seed=1, n=200, ref=ZERO6, step=3 * XI, pert=PERT, start=None, plane=PLANE, size=(640, 480), cam=TUM_CAM, pixels="interior",
          params=None, fast=False, one_eval=False, flat=None, depth_scale=None, extra=None, big=None):
    def make(seed=seed):
        return dict(seed=seed, n=n, ref=np.asarray(ref, np.float64), step=np.asarray(step, np.float64), pert=np.asarray(pert, np.float64),
                    start=start, plane=plane, size=size, cam=np.asarray(cam, np.float64), pixels=pixels, params=dict(params or {}), fast=fast,
                    one_eval=one_eval, flat=flat, depth_scale=depth_scale, extra=extra, big=big)
    return make


_WT = {k: np.array(v[0], np.float64) for k, v in WARP_VIEWS.items()}
LEAVE = np.array([0.12, 0.06, 0, 0, 0, 0.05])
ONE = dict(max_its=1)

CASES = {
    # ---- reference keyframes away from the world frame; `big`: also run with that many features (the four-wave form)
    "ref-roll30": _spec(ref=_WT["roll30"], big=385),
    "ref-roll90": _spec(ref=_WT["roll90"]),
    "ref-tilt25": _spec(ref=_WT["tilt25"], big=450),
    "ref-zoom0.6": _spec(ref=_WT["zoom0.6"]),
    "ref-zoom1.9-roll20": _spec(ref=_WT["zoom1.9-roll20"], step=XI, pert=PERT / 5),
    "tilted-plane": _spec(plane=TILTED, n=120),
    "step-roll8": _spec(ref=_WT["roll30"], step=np.array([0.02, 0.01, 0, 0, 0, 8 * np.pi / 180]), n=150),
    # ---- features leave the current image
    "leaving": _spec(step=LEAVE, start=SE3_IDENTITY, pixels="near_border", big=420),
    "leaving-at-it0": _spec(step=LEAVE, pert=PERT / 2, pixels="near_border", n=160),
    "leaving-later": _spec(step=LEAVE / 4, start=SE3_IDENTITY, pixels="near_border", n=160, params=dict(max_level=2, min_level=2)),
    "far-start": _spec(ref=_WT["roll30"], pert=np.array([0.2, 0.1, 0, 0, 0, 0.1]), n=180),
    # ---- levels and iteration limits
    "levels-0-4": _spec(ref=_WT["roll30"], n=100, params=dict(max_level=4, min_level=0)),
    "levels-4-4": _spec(ref=_WT["tilt25"], n=80, params=dict(max_level=4, min_level=4)),
    "levels-0-0": _spec(ref=_WT["roll90"], n=150, step=XI, pert=PERT / 10, size=(330, 250), cam=SMALL_CAM, params=dict(max_level=0, min_level=0)),
    "its1": _spec(start="early", params=ONE, n=120),
    "its2": _spec(ref=_WT["roll30"], params=dict(max_its=2), n=90),
    # ---- fast calls (Relocalize): early-out after the coarsest level, and all levels
    "fast-early": _spec(start="early", params=ONE, fast=True, n=120, big=400),
    "fast-exact": _spec(ref=_WT["roll30"], pert=ZERO6, fast=True, n=140),
    # ---- nothing measured, the sticky stop, flat images
    "nothing-measured": _spec(ref=_WT["roll30"], pert=np.array([5.0, 0, 0, 0, 0, 0]), n=64, big=390),
    "band-no-level4": _spec(pixels="band", n=90),
    "nan-depth0": _spec(depth_scale="zero", start=np.array([1.0, 0, 0, 0, 0, 0, 1.0]), n=50),
    "flat-reference": _spec(flat="ref", n=40),
    "flat-current": _spec(flat="cur", n=70, params=dict(max_level=3, min_level=3, max_its=1), one_eval=True),
    # ---- depth edges, one evaluation
    "depth-mix-l2": _spec(depth_scale="mix", params=dict(max_level=2, min_level=2, max_its=1), one_eval=True),
    "depth-mix-l4": _spec(depth_scale="mix", ref=_WT["roll30"], params=dict(max_level=4, min_level=4, max_its=1), one_eval=True, big=400),
    "behind-tz-4": _spec(start=np.array([1.0, 0, 0, 0, 0, 0, -4.0]), params=dict(max_level=3, min_level=3, max_its=1), one_eval=True),
    "zero-z": _spec(start="zero-z", extra="zero-z", n=100, params=dict(max_level=2, min_level=2, max_its=1), one_eval=True),
    # ---- level widths that are no multiples of 4: the byte shift of the window's rows changes from row to row
    "w752": _spec(size=(752, 480), cam=EUROC_CAM, pixels="edges", n=48 + 72),
    "w752-roll30": _spec(size=(752, 480), cam=EUROC_CAM, ref=_WT["roll30"], pixels="edges", n=48 + 112),
    "w330": _spec(size=(330, 250), cam=SMALL_CAM, pixels="edges", n=64 + 56, step=XI, pert=PERT / 4, params=dict(max_level=3, min_level=0)),
    "w330-one": _spec(size=(330, 250), cam=SMALL_CAM, pixels="edges", n=64 + 36, start=SE3_IDENTITY, step=ZERO6,
                      params=dict(max_level=3, min_level=3, max_its=1), one_eval=True),
}
EARLY = np.array([0.05, 0.02, 0, 0, 0, 0.02])
_made, _views = {}, {}


def features_of(c, px):
    """bearing, depth and validity of reference pixels px[n][2]: the scene plane seen from the reference camera"""
    n = len(px)
    cam, T_ref = c["cam"], c["T_ref"]
    ray = np.stack([(px[:, 0] - cam[2]) / cam[0], (px[:, 1] - cam[3]) / cam[1], np.ones(n)], 1)
    bearing = ray / np.linalg.norm(ray, axis=1, keepdims=True)
    R, t = quat_to_rot(T_ref[:4]), T_ref[4:]
    nc = R @ np.array(c["plane"][:3], np.float64)            # the plane n.X = d of the world, in the reference camera's frame
    dc = c["plane"][3] + nc @ t
    depth = dc / (bearing @ nc)
    valid = np.ones(n, np.uint8)
    valid[::17] = 0
    return bearing, depth, valid


def _build(c, n):
    rng = np.random.default_rng(c["seed"] + 1000 * n)
    w, h = c["size"]
    if c["pixels"] == "interior":
        px = interior(w, h, n, rng)
    elif c["pixels"] == "near_border":
        px = near_border(w, h, n, rng)
    elif c["pixels"] == "band":
        px = band(w, h, n, rng)
    else:
        levels = range(c["limits"]["min_level"], c["limits"]["max_level"] + 1)
        px = edge_pixels(w, h, levels, n - 16 * len(levels), rng)
    assert len(px) == n, (len(px), n)
    bearing, depth, valid = features_of(c, px)
    if c["depth_scale"] == "mix":                            # interleaved subsets: near, far, behind the reference camera, on its centre
        k = np.arange(n) % 8
        depth = depth * np.select([k == 1, k == 3, k == 5, k == 7], [0.02, 50.0, -1.0, 0.0], 1.0)
    if c["depth_scale"] == "zero":                           # every fifth point on the reference camera's centre: a start that moves the
        depth = depth * (np.arange(n) % 5 != 2)              # camera back along its axis lands them on the principal point, with 1 / z = inf
    start = c["start"]
    if c["extra"] == "zero-z":
        # feature 1 sits on the optical axis and feature 2 off it, both at z = d0 in the reference frame EXACTLY (d0 is the rounded
        # product the alignment itself forms, bearing_z * depth); the start moves the camera forward by d0 without turning, so 1
        # lands on 0 / 0 and 2 on x / 0, and every other feature, pushed three times as far out, stays in front
        px[1] = (c["cam"][2], c["cam"][3])
        px[2] = (450.0, 300.0)
        bearing, depth, valid = features_of(c, px)
        depth = depth * 3.0
        depth[2] = 2.5
        d0 = bearing[2, 2] * depth[2]
        depth[1] = d0
        assert bearing[1, 2] == 1.0 and bearing[1, 0] == 0.0 and bearing[1, 1] == 0.0 and valid[1] and valid[2]
        start = np.array([1.0, 0, 0, 0, 0, 0, -d0])
    for a in (px, bearing, depth, valid):
        a.setflags(write=False)
    return dict(px=px, bearing=bearing, depth=depth, valid=valid), start


def case(name):
    """the case's poses and features, made once and shared (read-only)"""
    if name not in _made:
        c = CASES[name]()
        c["name"] = name
        c["limits"] = dict(DEFAULTS, **c["params"])
        c["T_ref"] = se3_exp(c["ref"])
        c["T_cur"] = se3_mul(se3_exp(c["step"]), c["T_ref"])
        c["T_rel"] = se3_mul(c["T_cur"], se3_inv(c["T_ref"]))
        c["feats"], start = _build(c, c["n"])
        if isinstance(start, str) and start == "early":
            start = se3_mul(se3_exp(EARLY), c["T_rel"])
        elif start is None:
            start = se3_mul(se3_exp(c["pert"]), c["T_rel"])
        c["start"] = np.array(start, np.float64)
        c["start"].setflags(write=False)
        c["feats_big"] = _build(c, c["big"])[0] if c["big"] else None
        _made[name] = c
    return _made[name]


def frames(synth, c):
    """-> (reference image, current image), each view rendered once per session and shared (read-only)"""
    w, h = c["size"]
    out = []
    for which, T in (("ref", c["T_ref"]), ("cur", c["T_cur"])):
        if c["flat"] == which:
            key = ("flat", w, h)
            if key not in _views:
                _views[key] = np.full((h, w), 128, np.uint8)
        else:
            key = (tuple(T), tuple(c["cam"]), w, h, tuple(c["plane"]))
            if key not in _views:
                _views[key] = synth.render(T, c["cam"], w, h, plane=c["plane"], texture=0)
        _views[key].setflags(write=False)
        out.append(_views[key])
    return out


ONE_EVAL_CASES = [k for k in CASES if CASES[k]()["one_eval"]]
MULTI_CASES = [k for k in CASES if k not in ONE_EVAL_CASES]
BIG_CASES = [k for k in CASES if CASES[k]()["big"]]


class oracle_limits:
    """the oracle's copy of the alignment limits set to a case's for the duration of a with block"""
    NAMES = dict(max_level="max_align_level", min_level="min_align_level", max_its="max_img_align_its")

    def __init__(self, orc, limits):
        self.p, self.limits = orc.params, dict(DEFAULTS, **limits)

    def __enter__(self):
        self.old = {k: getattr(self.p, self.NAMES[k]) for k in self.limits}
        for k, v in self.limits.items():
            setattr(self.p, self.NAMES[k], v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.p, self.NAMES[k], v)


def oracle_answer(orc, synth, c, big=False, start=None, depth=None):
    """orc.image_align on a case's inputs under its limits, the oracle's limits restored after"""
    img_ref, img_cur = frames(synth, c)
    f = c["feats_big"] if big else c["feats"]
    with oracle_limits(orc, c["limits"]):
        return orc.image_align(img_ref, img_cur, c["cam"], f["px"], f["bearing"], f["depth"] if depth is None else depth, f["valid"],
                               c["start"] if start is None else start, fast=c["fast"])
