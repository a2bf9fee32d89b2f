"""The named inputs of the pose stage (FeatureAlign::SelectInliers + OptimizePose, feature_align.cc:73-82, 152-283, 341-431) that
tests/test_oracle_pose_independent.py and tests/test_gpu_pose.py share: start poses far from the identity, pyramid levels 0 to 4,
near, behind-the-camera and repeated observations, match counts at the edges the kernels have, outlier shares 0 to 0.65 and every
limit away from its default.

A case is a function of its seed: CASES[name]() -> dict(obs[n][6] = ax, ay, px, py, pz, level; pose = start pose (q, t);
params = the limits that differ from DEFAULTS; rand_seed, rand_skip; rank_deficient).  Nothing here calls the oracle.

Admission.  The stage is chaotic on outlier-heavy jobs (a match at the threshold, a chi2 that rises by rounding, two draws with
the same support), so a seed is committed only if the oracle is stable on it: n_draws and both lists identical and the pose within
1e-12 when every start-pose component, and again every ax, is moved by one ulp
(test_oracle_pose_independent.py::test_every_case_is_stable_on_the_oracle runs that screen on every case; nothing is screened or
skipped at run time).  The seeds below are the first that passed, tried upwards from 1: seed 1 everywhere except points2 (seeds 1
to 3 discarded by the screen) and the four cases whose seed was chosen for what they show (see WITNESS in
test_oracle_pose_independent.py): optim0, optim1, nine, seven-tight.  The one-match case is `pose_free`: one match leaves the pose a
four-dimensional null space that the LDLT fills from rounding, so the screen, and every comparison, holds where the match LANDS
instead of the pose.  `rank_deficient` marks the cases whose hypotheses (not their final pose) are solved from fewer than 3 matches."""
import numpy as np

from pose_restatement import quat_to_rot, se3_exp, se3_mul

FX = 517.3                                        # config/config_tum_f1.cfg:11
DEFAULTS = dict(max_ransac_points=5, max_ransac_its=100, max_optim_pose_its=10, inlier_error_threshold=2.0)   # config.cc
_D = np.pi / 180.0
_H = np.sqrt(0.5)

# start poses (q, t).  The rolls are written as quaternions so that 180 degrees has a scalar part of exactly 0.
STARTS = {
    "identity": np.array([1.0, 0, 0, 0, 0, 0, 0]),
    "roll30": np.array([np.cos(15 * _D), 0, 0, np.sin(15 * _D), 0.2, -0.1, 0.3]),
    "roll90": np.array([_H, 0, 0, _H, -0.3, 0.2, 0.1]),
    "roll180": np.array([0.0, 0, 0, 1.0, 0.1, 0.4, -0.2]),
    "oblique100": se3_exp(np.array([3.0, -4.0, 5.0, 100 * _D * 1 / np.sqrt(14.0), 100 * _D * 2 / np.sqrt(14.0), 100 * _D * 3 / np.sqrt(14.0)])),
}
SMALL = np.array([0.012, -0.008, 0.01, 0.004, -0.006, 0.003])         # start offset from the truth: a small twist
LARGE = np.array([0.06, -0.05, 0.04, 0.12, -0.15, 0.18])              # 0.1-0.2 rad: the first updates are large


def scene(seed, n, start="identity", offset=SMALL, outliers=0.2, noise_px=0.4, depth=(1.5, 3.0), levels=5, behind=0, repeat=0,
          identity_group=0):
    """n matches seen from a true pose T with start = Exp(offset) * T, so that the start pose is exactly the named one.
    Points are drawn in the true camera frame (|x/z| <= 0.6, |y/z| <= 0.45, depth in `depth`); `outliers` of them get an observation
    moved by up to 40 px; `behind` matches get a point 0.5 to 2 m BEHIND the start camera; the last `repeat` rows copy row 0;
    `identity_group` matches (every third row from 0) are instead exact observations from the pose SE3() of points in front of it."""
    rng = np.random.default_rng(seed)
    T_start = STARTS[start]
    T_true = se3_mul(se3_exp(-np.asarray(offset, np.float64)), T_start)
    R, t = quat_to_rot(T_true[:4]), T_true[4:]
    z = rng.uniform(depth[0], depth[1], n)
    pc = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1)
    P = (pc - t) @ R                                                   # R^T (pc - t)
    a = pc[:, :2] / pc[:, 2:3] + rng.normal(0, noise_px / FX, (n, 2))
    bad = rng.random(n) < outliers
    a[bad] += rng.uniform(-40, 40, (int(bad.sum()), 2)) / FX
    lvl = rng.integers(0, levels, n).astype(np.float64)
    if behind:
        Rs, ts = quat_to_rot(T_start[:4]), T_start[4:]
        rows = rng.choice(n, behind, replace=False)
        pb = np.stack([rng.uniform(-0.5, 0.5, behind), rng.uniform(-0.5, 0.5, behind), -rng.uniform(0.5, 2.0, behind)], 1)
        P[rows] = (pb - ts) @ Rs
    if identity_group:
        rows = np.arange(identity_group) * 3
        zi = rng.uniform(1.5, 3.0, identity_group)
        P[rows] = np.stack([rng.uniform(-0.5, 0.5, identity_group) * zi, rng.uniform(-0.4, 0.4, identity_group) * zi, zi], 1)
        a[rows] = P[rows, :2] / P[rows, 2:3]
    obs = np.concatenate([a, P, lvl[:, None]], 1)
    if repeat:
        obs[n - repeat:] = obs[0]
    return obs, T_start.copy()


def _case(seed, n, rand_seed=3, rand_skip=0, params=None, rank_deficient=False, pose_free=False, **kw):
    def make(seed=seed):
        obs, pose = scene(seed, n, **kw)
        return dict(obs=obs, pose=pose, params=dict(params or {}), rand_seed=rand_seed, rand_skip=rand_skip,
                    rank_deficient=rank_deficient, pose_free=pose_free)
    return make


CASES = {
    # ---- default limits: start poses, levels, geometry, counts, outlier shares
    "identity-150": _case(1, 150, start="identity", outliers=0.2),
    "one-match": _case(1, 1, start="roll30", outliers=0.0, rank_deficient=True, pose_free=True),
    "seven-tight": _case(5, 7, start="roll90", outliers=0.3, params=dict(inlier_error_threshold=0.5)),   # seed: see WITNESS
    "nine": _case(2, 9, start="roll90", outliers=0.3),                                                    # seed: see WITNESS
    "five": _case(1, 5, start="roll90", outliers=0.0),
    "six": _case(1, 6, start="oblique100", outliers=0.0),
    "roll30-63": _case(1, 63, start="roll30", outliers=0.1, rand_skip=5),
    "roll90-64": _case(1, 64, start="roll90", outliers=0.3, rand_skip=11),
    "roll180-65-clean": _case(1, 65, start="roll180", outliers=0.0, noise_px=0.2),                 # every match a supporter: budget 0
    "oblique-192": _case(1, 192, start="oblique100", outliers=0.4),
    "oblique-193-far": _case(1, 193, start="oblique100", offset=LARGE, outliers=0.2, rand_skip=7),
    "roll90-256": _case(1, 256, start="roll90", outliers=0.5),
    "roll30-257": _case(1, 257, start="roll30", outliers=0.3, offset=LARGE),
    "oblique-384-heavy": _case(1, 384, start="oblique100", outliers=0.65),
    "identity-385-heavy": _case(1, 385, start="identity", outliers=0.55, rand_skip=3),
    "roll180-1024-near": _case(1, 1024, start="roll180", outliers=0.3, depth=(0.15, 2.0)),
    "near-120": _case(1, 120, start="roll30", outliers=0.25, depth=(0.15, 0.6)),
    "behind-100": _case(1, 100, start="roll90", outliers=0.2, behind=4),
    "repeated-40": _case(1, 40, start="roll180", outliers=0.1, repeat=20),
    "roll180-90-far": _case(1, 90, start="roll180", offset=LARGE, outliers=0.35),
    # ---- limits away from their defaults
    "points1": _case(1, 80, start="roll30", outliers=0.3, params=dict(max_ransac_points=1, inlier_error_threshold=8.0), rank_deficient=True),
    "points2": _case(4, 80, start="roll90", outliers=0.3, params=dict(max_ransac_points=2, inlier_error_threshold=8.0), rank_deficient=True),
    "points8": _case(1, 120, start="oblique100", outliers=0.3, params=dict(max_ransac_points=8)),
    "its1": _case(1, 70, start="roll30", outliers=0.3, params=dict(max_ransac_its=1)),
    "its63": _case(1, 100, start="roll90", outliers=0.62, params=dict(max_ransac_its=63)),
    "its64": _case(1, 100, start="roll180", outliers=0.62, params=dict(max_ransac_its=64)),
    "its65": _case(1, 100, start="oblique100", outliers=0.62, params=dict(max_ransac_its=65)),
    "its129": _case(1, 100, start="roll30", outliers=0.62, params=dict(max_ransac_its=129)),
    "optim0": _case(2, 60, start="roll30", offset=LARGE, outliers=0.2, identity_group=12, params=dict(max_optim_pose_its=0)),
    "optim1": _case(3, 60, start="roll90", offset=LARGE, outliers=0.2, identity_group=12, params=dict(max_optim_pose_its=1)),
    "optim5": _case(1, 110, start="oblique100", offset=LARGE, outliers=0.25, params=dict(max_optim_pose_its=5)),
    "optim6": _case(1, 110, start="roll180", offset=LARGE, outliers=0.25, params=dict(max_optim_pose_its=6)),
    "thr0": _case(1, 75, start="roll90", outliers=0.2, params=dict(inlier_error_threshold=0.0)),
    "thr0.5": _case(1, 130, start="oblique100", outliers=0.3, params=dict(inlier_error_threshold=0.5)),
    "thr8": _case(1, 130, start="roll180", outliers=0.4, offset=LARGE, params=dict(inlier_error_threshold=8.0)),
}
_made = {}


def case(name):
    """the case's inputs, made once and shared (read-only)"""
    if name not in _made:
        c = CASES[name]()
        c["name"] = name
        c["limits"] = dict(DEFAULTS, **c["params"])
        c["obs"].setflags(write=False)
        c["pose"].setflags(write=False)
        _made[name] = c
    return _made[name]


DEFAULT_CASES = [k for k in CASES if not case(k)["params"]]
PARAM_CASES = [k for k in CASES if k not in DEFAULT_CASES]


class oracle_limits:
    """the oracle's copy of the limits set to a case's for the duration of a with block"""

    def __init__(self, orc, limits):
        self.p, self.limits = orc.params, dict(DEFAULTS, **limits)

    def __enter__(self):
        self.old = {k: getattr(self.p, k) for k in self.limits}
        for k, v in self.limits.items():
            setattr(self.p, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.p, k, v)


def oracle_answer(orc, c, cam, limits=None, obs=None, pose=None):
    """orc.pose_from_matches on a case's inputs under `limits` (default: the case's own), the oracle's limits restored after"""
    with oracle_limits(orc, c["limits"] if limits is None else limits):
        return orc.pose_from_matches(cam, c["obs"] if obs is None else obs, c["pose"] if pose is None else pose,
                                     rand_seed=c["rand_seed"], rand_skip=c["rand_skip"])
