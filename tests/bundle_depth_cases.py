"""The bundle-adjustment problems with depth edges that tests/test_bundle_depth_restatement_cpu.py and tests/test_gpu_bundle_depth.py share.

They are the problems of tests/bundle_cases.py with a measured depth on their edges: the true camera-frame z of the observation,
perturbed by 0.5 px (Gaussian, seeded) of disparity at BF = 1 / 0.0015 px m, in two shares:

  <name>/all    every edge carries a depth
  <name>/half   a seeded half of the edges do; the others are monocular edges (edge_d = 0)

and two cases of their own:

  wrong_depth   `outliers` with a depth on every edge, 10 % of the depths off by x 0.8 or x 1.25: what a read across an occlusion edge
                gives (at most one per point).  A wrong depth shows in the third row alone; the edge goes to level 1 as a whole.
                Five Huber iterations do not always free a point from a depth that is 33 px of disparity off: some clean edges
                of such a point go to level 1 with it (seeds 41 .. 45: 2, 8, 0, 4, 2 clean edges; every wrong one at all five)
  scale(...)    `pair` / `triple` with exact observations and exact depths, started at the truth scaled by 1.05 about the fixed
                keyframe's centre: a minimum of the monocular problem (its scale is a gauge freedom), 0.3 from the depth problem's

Every case is made once and handed out read-only.  A case whose trials or edges come too close to a threshold gets another seed here,
never another threshold."""
import numpy as np

import bundle_cases as bc
from bundle_cases import CAM, ro  # noqa: F401
from bundle_restatement import quat_to_rot

BF = 1.0 / 0.0015
DISPARITY_NOISE = 0.5
SHARES = ("all", "half")
WRONG_SEED = 43
NAMES = tuple("%s/%s" % (n, s) for n in bc.NAMES for s in SHARES) + ("wrong_depth",)
_made = {}


def true_z(prob):
    """camera-frame z of every edge's point at the truth"""
    R = quat_to_rot(prob["truth_poses"][:, :4])[prob["edge_kf"]]
    return np.einsum("nj,nj->n", R[:, 2, :], prob["truth_points"][prob["edge_pt"]]) + prob["truth_poses"][prob["edge_kf"], 6]


def with_depth(prob, share, seed, noise=DISPARITY_NOISE):
    rng = np.random.default_rng([seed, 7])
    z = true_z(prob)
    n_e = len(z)
    d = BF / (BF / z + noise * rng.standard_normal(n_e))
    if share == "half":
        keep = np.zeros(n_e, bool)
        keep[rng.permutation(n_e)[:n_e // 2]] = True
        d = np.where(keep, d, 0.0)
    return dict(prob, edge_d=ro(d), bf=BF)


def case(name):
    if name in _made:
        return _made[name]
    if name == "wrong_depth":
        base = with_depth(bc.case("outliers"), "all", bc.SHAPES["outliers"][4])
        rng = np.random.default_rng(WRONG_SEED)
        n_e = len(base["edge_d"])
        wrong = np.zeros(n_e, bool)
        for e in rng.permutation(n_e):                    # as with the shifted observations: at most one wrong depth per point
            if wrong.sum() < n_e // 10 and not wrong[base["edge_pt"] == base["edge_pt"][e]].any():
                wrong[e] = True
        factor = np.where(rng.random(n_e) < 0.5, 0.8, 1.25)
        prob = dict(base, name=name, edge_d=ro(np.where(wrong, base["edge_d"] * factor, base["edge_d"])), wrong=ro(wrong))
    else:
        src, share = name.split("/")
        prob = dict(with_depth(bc.case(src), share, bc.SHAPES[src][4]), name=name)
    _made[name] = prob
    return prob


def scale(src, share, s=1.05):
    """exact observations and depths; the start is the truth scaled by s about the fixed keyframe's centre"""
    key = ("scale", src, share, s)
    if key in _made:
        return _made[key]
    p = with_depth(bc.case(src, noise=0.0), share, bc.SHAPES[src][4], noise=0.0)
    fixed_pose = p["truth_poses"][p["n_free"]]
    c0 = -quat_to_rot(fixed_pose[:4])[0].T @ fixed_pose[4:]
    poses = np.array(p["truth_poses"])
    for k in range(p["n_free"]):
        R = quat_to_rot(poses[k, :4])[0]
        poses[k, 4:] = -R @ (c0 + s * (-R.T @ poses[k, 4:] - c0))
    points = c0 + s * (p["truth_points"] - c0)
    prob = dict(p, name="scale/%s/%s" % (src, share), poses=ro(poses), points=ro(points))
    _made[key] = prob
    return prob


def restated(name):
    """the depth restatement's result of case(name), computed once"""
    from bundle_depth_restatement import bundle_adjust
    key = ("restated", name)
    if key not in _made:
        _made[key] = bundle_adjust(case(name))
    return _made[key]
