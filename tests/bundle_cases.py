"""The local bundle-adjustment problems that tests/test_bundle_restatement_cpu.py and tests/test_gpu_bundle.py share.

A pinhole 640x480 camera (fx = fy = 520, centre 320, 240); keyframes on a short arc (0.3 apart, each looking at the middle
of the scene); points on two depth layers (4 and 6); observations = projections of the truth + seeded Gaussian noise (0.5 px); the
starts are the truth perturbed (poses by a twist of sigma 0.004, points by sigma 0.02).  Poses are listed free ones first.

  pair      1 free + the keyframe with id 0 (fixed), 8 points seen by both          the smallest solvable system, 6 x 6
  triple    2 free + 1 fixed, 12 points seen by all three                           Schur coupling between two poses
  full      11 free + 5 fixed, 300 points seen by 2 - 8 keyframes                   the 66 x 66 system
  outliers  4 free + 2 fixed, 60 points, 10 % of the observations shifted 8 - 30 px Huber weights, level-1 edges, stage 2 without them
            (seen by 5 - 6 keyframes, at most one shifted observation per point: a point is not dragged off its other views)
  behind    3 free + 1 fixed, 30 points, two start behind camera 0                  isDepthPositive, the non-finite guard
  single    3 free + 1 fixed, 30 points, five of them seen once                     rank-deficient point blocks held up by lambda
  rejects   3 free + 1 fixed, 40 points, the free poses start 0.2 rad off           rejected trials: lambda ni, restore
            (0.2 rad alone converges without a rejection at every seed tried: the points start 1.2 off as well, which gives
            two iterations of three trials in stage 1 and two of two trials in stage 2)
  dropped   3 free (the last sees no point) + 1 fixed, 20 points                    a vertex without edges

Every case is made once and handed out read-only; case(name, noise=0.0, start=s) is the same scene with exact observations and
the start perturbations scaled by s (the ground-truth test).  A case whose trials or edges come too close to a threshold gets another seed here, never another threshold."""
import numpy as np

from bundle_restatement import exp_update, quat_to_rot

CAM = (520.0, 520.0, 320.0, 240.0)
SPACING = 0.3
NAMES = ("pair", "triple", "full", "outliers", "behind", "single", "rejects", "dropped")
#            free fixed points views  seed
SHAPES = {
    "pair": (1, 1, 8, (2, 2), 11),
    "triple": (2, 1, 12, (3, 3), 12),
    "full": (11, 5, 300, (2, 8), 13),
    "outliers": (4, 2, 60, (5, 6), 300),
    "behind": (3, 1, 30, (2, 4), 121),
    "single": (3, 1, 30, (2, 4), 16),
    "rejects": (3, 1, 40, (2, 4), 171),
    "dropped": (3, 1, 20, (2, 3), 18),
}
_made = {}


def ro(a):
    a.setflags(write=False)
    return a


def arc_pose(k, n):
    """world -> camera pose of keyframe k of n"""
    c = np.array([SPACING * (k - 0.5 * (n - 1)), 0.015 * k, 0.0])
    th = -np.arctan2(c[0], 5.0)                           # looking at the middle of the scene
    q = np.array([np.cos(0.5 * th), 0.0, np.sin(0.5 * th), 0.0])
    return np.concatenate([q, -quat_to_rot(q)[0] @ c])


def project(pose, X):
    Xc = X @ quat_to_rot(pose[:4])[0].T + pose[4:]
    return np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]], 1)


def case(name, noise=0.5, start=1.0):
    key = (name, noise, start)
    if key in _made:
        return _made[key]
    n_free, n_fixed, n_pt, (lo, hi), seed = SHAPES[name]
    rng = np.random.default_rng(seed)
    n_kf = n_free + n_fixed
    truth_poses = np.stack([arc_pose(k, n_kf) for k in range(n_kf)])
    z = np.where(rng.random(n_pt) < 0.5, 4.0, 6.0)
    truth_points = np.stack([rng.uniform(-1.2, 1.2, n_pt) * z / 4, rng.uniform(-0.8, 0.8, n_pt) * z / 4, z], 1)
    seeing = n_kf - 1 if name == "dropped" else n_kf      # `dropped`: free keyframe n_free - 1 sees nothing
    kf_ids = [k for k in range(n_kf) if not (name == "dropped" and k == n_free - 1)]
    ept, ekf = [], []
    for p in range(n_pt):
        c = int(rng.integers(lo, hi + 1))
        if name == "single" and p < 5:
            c = 1
        if name == "behind" and p in (3, 7):
            c = seeing
        for k in sorted(rng.choice(seeing, size=min(c, seeing), replace=False)):
            ept.append(p)
            ekf.append(kf_ids[k])
    order = rng.permutation(len(ept))                     # callers need not sort their edges
    ept, ekf = np.array(ept, np.int32)[order], np.array(ekf, np.int32)[order]
    uv = np.concatenate([project(truth_poses[k], truth_points[p:p + 1]) for p, k in zip(ept, ekf)])
    uv = uv + noise * rng.standard_normal(uv.shape)
    shifted = np.zeros(len(ept), bool)
    if name == "outliers":
        for e in rng.permutation(len(ept)):               # at most one shifted observation per point
            if shifted.sum() < len(ept) // 10 and not shifted[ept == ept[e]].any():
                shifted[e] = True
        ang, r = rng.uniform(0, 2 * np.pi, len(ept)), rng.uniform(8.0, 30.0, len(ept))
        uv = uv + shifted[:, None] * np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    poses = truth_poses.copy()
    for k in range(n_free):
        tw = 0.004 * start * rng.standard_normal(6)
        if name == "rejects":
            d = rng.standard_normal(3)
            tw[:3] = 0.2 * d / np.linalg.norm(d)
        poses[k] = exp_update(truth_poses[k], tw)
    points = truth_points + (1.2 if name == "rejects" else 0.02) * start * rng.standard_normal(truth_points.shape)
    if name == "behind":
        for p in (3, 7):                                  # mirrored through camera 0's centre: negative depth there
            c0 = -quat_to_rot(truth_poses[0, :4])[0].T @ truth_poses[0, 4:]
            points[p] = c0 - 0.3 * (truth_points[p] - c0)
    fixed = np.array([0] * n_free + [1] * n_fixed, np.int32)
    prob = dict(name=name, poses=ro(poses), fixed=ro(fixed), points=ro(points), edge_pt=ro(ept), edge_kf=ro(ekf), edge_uv=ro(uv), cam=CAM,
                truth_poses=ro(truth_poses), truth_points=ro(truth_points), shifted=ro(shifted), n_free=n_free)
    _made[key] = prob
    return prob


def restated(name):
    """the restatement's result of case(name), computed once"""
    from bundle_restatement import bundle_adjust
    key = ("restated", name)
    if key not in _made:
        _made[key] = bundle_adjust(case(name))
    return _made[key]
