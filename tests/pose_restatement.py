"""FeatureAlign::SelectInliers, ConvergePose, OptimizePose and RescueOutliers (feature_align.cc:152-283, 341-431) restated in
float64 numpy from the reference's text, not from oracle/ref_tracker.h or csrc/sdvl_pose.hip: what
tests/test_oracle_pose_independent.py holds the oracle's pose stage against.

Nothing here calls the oracle.  The SE3 exponential, the quaternion product and the quaternion-to-rotation conversion are written
out below (extra/se3.cc:72-94, 114-130, 166-177); the normal equations are summed by numpy over all features at once and solved by
numpy.linalg.lstsq, where the reference accumulates feature by feature and solves with Eigen's pivoted LDLT (feature_align.cc:402):
on a system of full rank the two agree to rounding, on a rank-deficient one (fewer than three matches) the LDLT fills the null
space from rounding and lstsq takes the minimum-norm solution, so only what the null space does not decide can be compared there.
rand() is libc's, through ctypes.

restate(...) returns dict(pose, n_draws, inliers, outliers, refined, trace).  trace counts how often each branch was taken and
keeps the smallest relative distance of any tested reprojection error to the threshold it was tested against (`margin`; a zero
threshold has no relative distance and is left out).  fault=<name> plants exactly one error, see FAULTS."""
import ctypes as C

import numpy as np

K_MAD_NORM = 1.4826                 # feature_align.h:114
K_TUKEY_C = 4.6851 * 4.6851         # feature_align.h:115
SMALL_EPS = 1e-10                   # extra/se3.h:30

FAULTS = {
    "update_side": "T * Exp(dT) in place of Exp(dT) * T (feature_align.cc:411)",
    "rotation_transposed": "R^T p + t where the pose is applied to a point (:269, :362, :389)",
    "inv_cov_error_only": "sqrt_inv_cov scales the error but not the Jacobian (:394)",
    "median_low": "median taken at (n - 1) // 2 in place of n // 2 (extra/utils.cc:217)",
    "switch_at_4": "scale forced at i == 4 in place of i == 5 (:380)",
    "rollback_keeps_current": "the roll-back on rising chi2 keeps the current pose (:406)",
    "rescue_1x": "RescueOutliers tests against 1x the threshold in place of 2x (:239)",
    "supporters_ge": "a draw replaces the best one with >= supporters in place of > (:196)",
    "window_no_wrap": "the draw's window stops at the end of the match list in place of wrapping (:182)",
    "best_is_start": "with no supporter anywhere the matches are classified with the start pose, not SE3() (:159, :215)",
}
BRANCHES = ("rollback", "scale_switch", "step_stop", "out_of_its", "budget_small", "budget_zero", "rescue_adds", "rescue_none",
            "empty_inliers")


# ---------------------------------------------------------------------------------------------------- SE3 (extra/se3.cc)
def quat_to_rot(q):
    """Eigen::Quaterniond::toRotationMatrix of (w, x, y, z) (se3.h:41)"""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def hat(v):                                           # se3.cc:132-138
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def rotation_exp(omega):                              # se3.cc:114-130
    theta = np.sqrt(omega @ omega)
    half = 0.5 * theta
    if theta < SMALL_EPS:
        t2 = theta * theta
        imag = 0.5 - 0.0208333 * t2 + 0.000260417 * t2 * t2
    else:
        imag = np.sin(half) / theta
    return np.array([np.cos(half), imag * omega[0], imag * omega[1], imag * omega[2]]), theta


def se3_exp(u):                                       # se3.cc:72-94: (upsilon, omega) -> (q, t) as 7 numbers
    u = np.asarray(u, np.float64)
    upsilon, omega = u[:3], u[3:]
    q, theta = rotation_exp(omega)
    Om = hat(omega)
    if theta < SMALL_EPS:
        V = quat_to_rot(q)
    else:
        t2 = theta * theta
        V = np.eye(3) + (1 - np.cos(theta)) / t2 * Om + (theta - np.sin(theta)) / (t2 * theta) * (Om @ Om)
    return np.concatenate([q, V @ upsilon])


def quat_mul(a, b):                                   # Eigen's quaternion product
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def se3_mul(A, B):                                    # se3.cc:166-177 (the product is normalised)
    q = quat_mul(A[:4], B[:4])
    q = q / np.sqrt(q @ q)
    return np.concatenate([q, A[4:] + quat_to_rot(A[:4]) @ B[4:]])


def se3_matrix(T):
    """the 4x4 matrix of a pose (q, t): what two poses are compared by"""
    M = np.eye(4)
    M[:3, :3] = quat_to_rot(T[:4])
    M[:3, 3] = T[4:]
    return M


SE3_IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0])      # se3.cc:26-32


# ---------------------------------------------------------------------------------------------------- the stage
class _Stage:
    def __init__(self, obs, fx, max_ransac_points, max_ransac_its, max_optim_pose_its, inlier_error_threshold, fault):
        assert fault is None or fault in FAULTS, fault
        obs = np.asarray(obs, np.float64).reshape(-1, 6)
        self.a, self.P = obs[:, :2], obs[:, 2:5]
        self.s = 1.0 / (1 << obs[:, 5].astype(np.int64))          # sqrt_inv_cov, :271, :364, :392
        self.fx, self.points, self.its, self.optim_its = fx, max_ransac_points, max_ransac_its, max_optim_pose_its
        self.thr = inlier_error_threshold / fx                    # :193
        self.fault = fault
        self.trace = dict.fromkeys(BRANCHES, 0)
        self.trace["margin"] = np.inf

    def apply(self, T, idx):                                      # se3.h:68
        R = quat_to_rot(T[:4])
        if self.fault == "rotation_transposed":
            R = R.T
        return self.P[idx] @ R.T + T[4:]

    def errors(self, T, idx):
        """-> (scaled 2-vector errors, camera-frame positions): :269-272 = :362-364 = :389-393"""
        pos = self.apply(T, idx)
        e = (self.a[idx] - pos[:, :2] / pos[:, 2:3]) * self.s[idx, None]     # SimpleProject of (ax, ay, 1) is (ax, ay)
        return e, pos

    def check(self, T, idx, thr, inl=None, outl=None):            # CheckReprojectionError, :258-283
        idx = np.asarray(idx, np.int64)
        if len(idx) == 0:
            return 0
        e, _ = self.errors(T, idx)
        norm = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
        if thr > 0:
            self.trace["margin"] = min(self.trace["margin"], float(np.min(np.abs(norm - thr)) / thr))
        ok = norm <= thr
        if inl is not None:
            inl.extend(int(i) for i in idx[ok])
        if outl is not None:
            outl.extend(int(i) for i in idx[~ok])
        return int(ok.sum())

    def converge(self, start, idx):                               # ConvergePose, :341-421 -> pose or None
        idx = np.asarray(idx, np.int64)
        last = start.copy()
        se3 = start.copy()
        chi2 = 0.0
        if len(idx) == 0:
            return None                                           # :367-368
        e, _ = self.errors(se3, idx)
        norms = np.sort(np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]))
        mid = (len(norms) - 1) // 2 if self.fault == "median_low" else len(norms) // 2      # extra/utils.cc:215-220
        scale = K_MAD_NORM * norms[mid]
        ran_out = True
        for i in range(self.optim_its):
            if i == (4 if self.fault == "switch_at_4" else 5):
                scale = 0.85 / self.fx                            # :380-381
                self.trace["scale_switch"] += 1
            e, pos = self.errors(se3, idx)
            J = jacobian_3d_to_plane(pos)                         # [n, 2, 6]
            if self.fault != "inv_cov_error_only":
                J = J * self.s[idx, None, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                w = tukey(np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) / scale)
            A = np.einsum("n,nkr,nkc->rc", w, J, J)               # :396
            b = -np.einsum("n,nkr,nk->r", w, J, e)                # :397
            new_chi2 = float(np.sum((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) * w))         # :398
            if np.all(np.isfinite(A)) and np.all(np.isfinite(b)):
                dT = np.linalg.lstsq(A, b, rcond=None)[0]         # :402, a general solver in place of the LDLT
            else:
                dT = np.full(6, np.nan)
            if (i > 0 and new_chi2 > chi2) or np.isnan(dT[0]):    # :405-408
                if self.fault != "rollback_keeps_current":
                    se3 = last
                self.trace["rollback"] += 1
                ran_out = False
                break
            if self.fault == "update_side":
                T_new = se3_mul(se3, se3_exp(dT))
            else:
                T_new = se3_mul(se3_exp(dT), se3)                 # :411
            last = se3
            se3 = T_new
            chi2 = new_chi2
            if np.max(np.abs(dT)) <= 1e-10:                       # :417, AbsMax extra/utils.cc:28-42
                self.trace["step_stop"] += 1
                ran_out = False
                break
        if ran_out:
            self.trace["out_of_its"] += 1
        return se3

    def select_inliers(self, start, rand):                        # :152-216
        size = len(self.a)
        inl, outl = [], []
        if size == 0:
            return inl, outl, 0
        npoints = min(self.points, size)
        nits, best_supporters, it, n_draws = self.its, 0, 0, 0
        best = start.copy() if self.fault == "best_is_start" else SE3_IDENTITY.copy()      # SE3 best_se3, :159
        everyone = np.arange(size)
        while it < nits:
            index = rand() % size                                 # :180
            n_draws += 1
            if self.fault == "window_no_wrap":
                sel = [index + i for i in range(npoints) if index + i < size]
            else:
                sel = [(index + i) % size for i in range(npoints)]                         # :181-184
            se3 = self.converge(start, sel)                       # every draw starts from the frame's pose, :351
            if se3 is None:
                it += 1
                continue
            supporters = self.check(se3, everyone, self.thr)      # :193
            better = supporters >= best_supporters if self.fault == "supporters_ge" else supporters > best_supporters
            if better:                                            # :196-210
                best_supporters, best = supporters, se3
                epsilon = 1.0 - float(supporters) / float(size)
                tmp = 1.0 - epsilon
                for _ in range(1, npoints):
                    tmp *= tmp
                if tmp < 1e-5:
                    nits = self.its
                    self.trace["budget_small"] += 1
                else:
                    with np.errstate(divide="ignore"):
                        nits = min(self.its, int(np.log(1.0 - 0.99) / np.log(1.0 - tmp)))
                    if nits == 0:
                        self.trace["budget_zero"] += 1
            it += 1
        self.check(best, everyone, self.thr, inl, outl)           # :215
        return inl, outl, n_draws


def jacobian_3d_to_plane(pos):                                    # extra/utils.cc:99-118, for [n, 3] points -> [n, 2, 6]
    x, y = pos[:, 0], pos[:, 1]
    z_inv = 1.0 / pos[:, 2]
    z_inv_2 = z_inv * z_inv
    J = np.zeros((len(pos), 2, 6))
    J[:, 0, 0] = -z_inv
    J[:, 0, 2] = x * z_inv_2
    J[:, 0, 3] = y * J[:, 0, 2]
    J[:, 0, 4] = -(1.0 + x * J[:, 0, 2])
    J[:, 0, 5] = y * z_inv
    J[:, 1, 1] = -z_inv
    J[:, 1, 2] = y * z_inv_2
    J[:, 1, 3] = 1.0 + y * J[:, 1, 2]
    J[:, 1, 4] = -J[:, 0, 3]
    J[:, 1, 5] = -x * z_inv
    return J


def tukey(x):                                                     # GetTukeyValue, :423-431
    x2 = x * x
    with np.errstate(invalid="ignore"):
        return np.where(x2 <= K_TUKEY_C, (1.0 - x2 / K_TUKEY_C) ** 2, 0.0)


def libc_rand(seed, skip=0):
    """rand() of libc after srand(seed) and `skip` draws, the way FeatureAlign consumes it (:180)"""
    libc = C.CDLL("libc.so.6")
    libc.srand(C.c_uint(seed))
    for _ in range(skip):
        libc.rand()
    return libc.rand


def restate(obs, pose, fx, rand_seed=1, rand_skip=0, max_ransac_points=5, max_ransac_its=100, max_optim_pose_its=10,
            inlier_error_threshold=2.0, fault=None):
    """FeatureAlign::SelectInliers (:152-216) and FeatureAlign::OptimizePose(frame) (:73-79) on obs[n][6] = ax, ay, px, py, pz,
    level from the start pose (q, t): -> dict(pose, n_draws, inliers, outliers, refined, trace)"""
    st = _Stage(obs, fx, max_ransac_points, max_ransac_its, max_optim_pose_its, inlier_error_threshold, fault)
    pose = np.array(pose, np.float64)
    inl, outl, n_draws = st.select_inliers(pose, libc_rand(rand_seed, rand_skip))
    refined = 0
    for second in (False, True):
        if not inl:
            st.trace["empty_inliers"] += 1
        se3 = st.converge(pose, inl)                              # OptimizePose, :218-230
        if se3 is not None:
            pose, refined = se3, 1                                # frame->SetPose, :224
            cfeatures, inl = inl, []
            st.check(pose, cfeatures, st.thr, inl, outl)
        if second:
            break
        init_inliers = len(inl)                                   # RescueOutliers, :232-243
        cfeatures, outl = outl, []
        st.check(pose, cfeatures, (1 if fault == "rescue_1x" else 2) * st.thr, inl, outl)
        if not len(inl) > init_inliers:
            st.trace["rescue_none"] += 1
            break
        st.trace["rescue_adds"] += 1
    return dict(pose=pose, n_draws=n_draws, inliers=np.array(inl, np.int32), outliers=np.array(outl, np.int32), refined=refined,
                trace=st.trace)
