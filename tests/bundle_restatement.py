"""numpy float64 restatement of what Bundle::Local (extra/bundle.cc:110-223) makes g2o do: the specification of sdvl_bundle_adjust.
Written from the g2o sources the reference ships (optimization_algorithm_levenberg.cpp:61-189, block_solver.hpp, base_binary_edge.hpp,
robust_kernel_impl.cpp:78-91, types_six_dof_expmap.cpp:103-147, sparse_optimizer.cpp:340-410), not from csrc/sdvl_bundle.hip.

A problem is dict(poses [n_kf][7] (qw qx qy qz tx ty tz, world -> camera, free ones first), fixed [n_kf], points [n_pt][3],
edge_pt [n_e], edge_kf [n_e], edge_uv [n_e][2], cam (fx, fy, cx, cy)).

  edge     err = obs - (fx x/z + cx, fy y/z + cy) of R(q) X + t, information I; Jacobians of linearizeOplus (rotation in the first three
           pose columns); pose update exp(d) T, point update X + d
  Huber    delta = sqrt(5.991) on e = err.err: e <= delta^2: rho = (e, 1), else (2 delta sqrt(e) - delta^2, delta / sqrt(e)); H and b are
           scaled by rho' only; chi2 = rho[0]
  LM       lambda0 = 1e-5 max |H_jj| at iteration 0 of a stage, ni = 2; lambda on the diagonals of pose AND point blocks; the Schur
           complement on the poses, a dense Cholesky, back-substitution for the points;
           rho = (chi - chi') / (sum x_j (lambda x_j + b_j) + 1e-3); accepted when rho > 0 and chi' finite:
           lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), ni = 2; rejected: lambda *= ni, ni *= 2, estimates restored; trials repeat
           while rho < 0, at most 10; the stage ends when the trial count reached 10 or rho == 0, or when nBad (consecutive iterations
           with (chi0 - chi) 1e3 < chi0) reaches 3
  stages   5 iterations with Huber; every edge with chi2 > 5.991 or depth <= 0 goes to level 1, all kernels off; 10 iterations on
           the level-0 edges
  vertices a fixed pose contributes no unknowns; a vertex without an active edge drops out of the stage

What g2o leaves implicit and this file states:
  * the outlier test after stage 1 sees the ACCEPTED estimates (g2o's edges keep the errors of the last trial, also a rejected one);
  * LinearSolverEigen's sparse LL^T is a dense column Cholesky; a pivot that is not > 0 (NaN included) is a failed solve;
  * a failed solve is a rejected trial outright (g2o applies the stale x and lets rho decide);
  * a stage whose initial chi2 is not finite ends the problem with status NONFINITE and the inputs restored;
  * delta is sqrt(5.991) in double (bundle.cc:150 rounds it to float);
  * exp() takes the quaternion (cos(theta/2), sin(theta/2)/theta omega) directly instead of Quaterniond(R), and the series of
    sin(x)/x, (1 - cos x)/x^2, (x - sin x)/x^3 below theta = 1e-5 (se3quat.h:237-243 takes R = V = I + W + W^2 there);
  * (2 rho - 1)^3 is two multiplications;
  * 3x3 point blocks are inverted by the adjugate.
A trial is "settled" when |chi - chi'| < 1e-9 chi: from there on the decisions depend on the last bits of a sum."""
import math

import numpy as np

CHI2_TH = 5.991
DELTA = math.sqrt(CHI2_TH)
DBL_MAX = 1.7976931348623157e308
OK, EMPTY, NO_EDGES, NONFINITE = 0, 1, 2, 3
STAGE_ITS = (5, 10)
MAX_TRIALS = 10


def quat_to_rot(q):
    """[n][4] unit quaternions (w x y z) -> [n][3][3]"""
    q = np.asarray(q, np.float64).reshape(-1, 4)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def exp_update(pose, d):
    """exp(d) * pose, d = (omega, upsilon) (types_six_dof_expmap.h oplusImpl, se3quat.h:223-257, :104-110)"""
    om, up = d[:3], d[3:]
    th2 = float(om @ om)
    th = math.sqrt(th2)
    if th < 1e-5:
        a, b, c = 1 - th2 / 6, 0.5 - th2 / 24, 1.0 / 6 - th2 / 120
        qw, s = 1 - th2 / 8, 0.5 - th2 / 48
    else:
        a, b, c = math.sin(th) / th, (1 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
        qw, s = math.cos(0.5 * th), math.sin(0.5 * th) / th
    W = skew(om)
    W2 = W @ W
    dR = np.eye(3) + a * W + b * W2
    V = np.eye(3) + b * W + c * W2
    dq = np.array([qw, s * om[0], s * om[1], s * om[2]])
    q = pose[:4]
    nq = np.array([dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2] - dq[3] * q[3],
                   dq[0] * q[1] + dq[1] * q[0] + dq[2] * q[3] - dq[3] * q[2],
                   dq[0] * q[2] - dq[1] * q[3] + dq[2] * q[0] + dq[3] * q[1],
                   dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1] + dq[3] * q[0]])
    if nq[0] < 0:
        nq = -nq
    nq = nq / math.sqrt(float(nq @ nq))
    return np.concatenate([nq, dR @ pose[4:] + V @ up])


def edge_terms(poses, points, edge_pt, edge_kf, edge_uv, cam, jac=True):
    """-> err [n][2], z [n], Ji [n][2][3] (point), Jj [n][2][6] (pose)"""
    fx, fy, cx, cy = cam
    R = quat_to_rot(poses[:, :4])[edge_kf]
    Xc = np.einsum("nij,nj->ni", R, points[edge_pt]) + poses[edge_kf, 4:]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    with np.errstate(all="ignore"):
        err = edge_uv - np.stack([fx * x / z + cx, fy * y / z + cy], 1)
        if not jac:
            return err, z, None, None
        z2 = z * z
        tmp = np.zeros((len(z), 2, 3))
        tmp[:, 0, 0] = fx; tmp[:, 0, 2] = -x / z * fx
        tmp[:, 1, 1] = fy; tmp[:, 1, 2] = -y / z * fy
        Ji = (-1.0 / z)[:, None, None] * np.einsum("nij,njk->nik", tmp, R)
        Jj = np.zeros((len(z), 2, 6))
        Jj[:, 0, 0] = x * y / z2 * fx; Jj[:, 0, 1] = -(1 + x * x / z2) * fx; Jj[:, 0, 2] = y / z * fx
        Jj[:, 0, 3] = -1.0 / z * fx; Jj[:, 0, 5] = x / z2 * fx
        Jj[:, 1, 0] = (1 + y * y / z2) * fy; Jj[:, 1, 1] = -x * y / z2 * fy; Jj[:, 1, 2] = -x / z * fy
        Jj[:, 1, 4] = -1.0 / z * fy; Jj[:, 1, 5] = y / z2 * fy
    return err, z, Ji, Jj


def huber(e):
    """rho[0], rho[1] of robust_kernel_impl.cpp:78-91 for e = err.err"""
    with np.errstate(all="ignore"):
        s = np.sqrt(e)
        inl = e <= DELTA * DELTA
        return np.where(inl, e, 2 * s * DELTA - DELTA * DELTA), np.where(inl, 1.0, DELTA / s)


def inv3_sym(H):
    """[n][3][3] symmetric -> inverse by the adjugate"""
    a, b, c, d, e, f = H[:, 0, 0], H[:, 0, 1], H[:, 0, 2], H[:, 1, 1], H[:, 1, 2], H[:, 2, 2]
    A, B, Cc = d * f - e * e, c * e - b * f, b * e - c * d
    D, E, F = a * f - c * c, b * c - a * e, a * d - b * b
    with np.errstate(all="ignore"):
        inv = 1.0 / (a * A + b * B + c * Cc)
        out = np.empty_like(H)
        out[:, 0, 0] = A * inv; out[:, 0, 1] = out[:, 1, 0] = B * inv; out[:, 0, 2] = out[:, 2, 0] = Cc * inv
        out[:, 1, 1] = D * inv; out[:, 1, 2] = out[:, 2, 1] = E * inv; out[:, 2, 2] = F * inv
    return out


def cholesky_solve(S, rhs):
    """dense column Cholesky S = L L^T and the two substitutions; None when a pivot is not > 0"""
    n = len(S)
    L = np.tril(S).copy()
    for k in range(n):
        d = L[k, k]
        if not d > 0.0 or not np.isfinite(d):
            return None
        d = math.sqrt(d)
        L[k, k] = d
        L[k + 1:, k] /= d
        for j in range(k + 1, n):
            L[j:, j] -= L[j:, k] * L[j, k]
    y = rhs.copy()
    for k in range(n):
        y[k] /= L[k, k]
        y[k + 1:] -= L[k + 1:, k] * y[k]
    for k in range(n - 1, -1, -1):
        y[k] /= L[k, k]
        y[:k] -= L[k, :k] * y[k]
    return y


class System:
    """H and b of the active edges at (poses, points): buildSystem (block_solver.hpp, base_binary_edge.hpp:60-115)"""

    def __init__(self, prob, poses, points, active, robust):
        self.n_free = nf = int(np.sum(np.asarray(prob["fixed"]) == 0))
        self.n_pt = npt = len(points)
        ept, ekf, euv = prob["edge_pt"][active], prob["edge_kf"][active], prob["edge_uv"][active]
        err, _, Ji, Jj = edge_terms(poses, points, ept, ekf, euv, prob["cam"])
        e = np.sum(err * err, 1)
        w = huber(e)[1] if robust else np.ones(len(e))
        self.Hpp, self.bp = np.zeros((nf, 6, 6)), np.zeros((nf, 6))
        self.Hll, self.bl = np.zeros((npt, 3, 3)), np.zeros((npt, 3))
        np.add.at(self.Hll, ept, w[:, None, None] * np.einsum("nki,nkj->nij", Ji, Ji))
        np.add.at(self.bl, ept, -w[:, None] * np.einsum("nki,nk->ni", Ji, err))
        free = ekf < nf
        self.f_pt, self.f_kf = ept[free], ekf[free]
        np.add.at(self.Hpp, self.f_kf, w[free, None, None] * np.einsum("nki,nkj->nij", Jj[free], Jj[free]))
        np.add.at(self.bp, self.f_kf, -w[free, None] * np.einsum("nki,nk->ni", Jj[free], err[free]))
        self.W = w[free, None, None] * np.einsum("nki,nkj->nij", Jj[free], Ji[free])        # [n_free_edges][6][3]
        # vertices without an active edge are not part of the system (sparse_optimizer.cpp initializeOptimization)
        self.pose_on = np.zeros(nf, bool)
        self.pose_on[self.f_kf] = True
        self.pt_on = np.zeros(npt, bool)
        self.pt_on[ept] = True

    def max_diagonal(self):
        d = [0.0]
        if self.pose_on.any():
            d.append(np.abs(np.diagonal(self.Hpp[self.pose_on], axis1=1, axis2=2)).max())
        if self.pt_on.any():
            d.append(np.abs(np.diagonal(self.Hll[self.pt_on], axis1=1, axis2=2)).max())
        return float(max(d))

    def solve(self, lam):
        """-> (dp [n_free][6], dl [n_pt][3], scale) or None"""
        nf = self.n_free
        Hinv = inv3_sym(self.Hll + lam * np.eye(3))
        Hinv[~self.pt_on] = 0.0
        Wd = np.zeros((nf, 6, self.n_pt, 3))
        Wd[self.f_kf, :, self.f_pt, :] = self.W
        Wd = Wd.reshape(6 * nf, self.n_pt, 3)
        Y = np.einsum("apk,pkl->apl", Wd, Hinv)
        S = -np.einsum("apl,bpl->ab", Y, Wd)
        for a in range(nf):
            S[6 * a:6 * a + 6, 6 * a:6 * a + 6] += self.Hpp[a] + lam * np.eye(6)
        rhs = self.bp.reshape(-1) - np.einsum("apl,pl->a", Y, self.bl)
        on = np.repeat(self.pose_on, 6)
        x = np.zeros(6 * nf)
        if on.any():
            xs = cholesky_solve(S[np.ix_(on, on)], rhs[on])
            if xs is None:
                return None
            x[on] = xs
        dl = np.einsum("pkl,pl->pk", Hinv, self.bl - np.einsum("apl,a->pl", Wd, x))
        scale = float(np.sum(x * (lam * x + self.bp.reshape(-1)))) + float(np.sum(dl * (lam * dl + self.bl)))
        return x.reshape(nf, 6), dl, scale


def chi2_of(prob, poses, points, active, robust):
    err, _, _, _ = edge_terms(poses, points, prob["edge_pt"][active], prob["edge_kf"][active], prob["edge_uv"][active], prob["cam"], jac=False)
    e = np.sum(err * err, 1)
    return float(np.sum(huber(e)[0] if robust else e))


def decide(chi, chi_new, scale, ok):
    """-> (rho, accepted)"""
    if not ok:
        return -math.inf, False
    with np.errstate(all="ignore"):
        rho = float((np.float64(chi) - np.float64(chi_new)) / np.float64(scale + 1e-3))
    return rho, bool(rho > 0 and math.isfinite(chi_new))


def run_stage(prob, poses, points, active, robust, n_its, log, stage):
    """-> poses, points, stats (None: the initial chi2 is not finite)"""
    st = dict(iterations=0, trials=0, lam=0.0, chi2_before=0.0, chi2_after=0.0, trials_per_it=[], accepted_its=[])
    lam, ni, n_bad = 0.0, 2.0, 0
    for it in range(n_its):
        chi = chi2_of(prob, poses, points, active, robust)
        if it == 0:
            st["chi2_before"] = st["chi2_after"] = chi
            if not math.isfinite(chi):
                return None
        chi0 = chi
        sysm = System(prob, poses, points, active, robust)
        if it == 0:
            lam, ni, n_bad = 1e-5 * sysm.max_diagonal(), 2.0, 0
        q, rho, accepted = 0, 0.0, False
        while True:
            sol = sysm.solve(lam)
            if sol is not None:
                dp, dl, scale = sol
                new_poses = poses.copy()
                for a in range(sysm.n_free):
                    new_poses[a] = exp_update(poses[a], dp[a])
                new_points = points + dl
                chi_new = chi2_of(prob, new_poses, new_points, active, robust)
            else:
                scale, chi_new = 0.0, DBL_MAX
            rho, accepted = decide(chi, chi_new, scale, sol is not None)
            log.append(dict(stage=stage, it=it, trial=q, chi=chi, chi_new=chi_new, scale=scale, ok=sol is not None, accepted=accepted,
                            settled=bool(sol is not None and abs(chi - chi_new) < 1e-9 * chi)))
            if accepted:
                t = 2 * rho - 1
                lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - t * t * t))
                ni = 2.0
                chi, poses, points = chi_new, new_poses, new_points
            else:
                lam *= ni
                ni *= 2.0
            q += 1
            if not (rho < 0 and q < MAX_TRIALS):
                break
        st["iterations"] += 1
        st["trials"] += q
        st["trials_per_it"].append(q)
        st["accepted_its"].append(accepted)
        st["chi2_after"] = chi
        if q == MAX_TRIALS or rho == 0:
            break
        n_bad = n_bad + 1 if (chi0 - chi) * 1e3 < chi0 else 0
        if n_bad >= 3:
            break
    st["lam"] = lam
    return poses, points, st


def bundle_adjust(prob, stage_its=STAGE_ITS):
    """stage_its: iterations of the two optimize() calls (Bundle::Local: 5 and 10).
    -> dict(status, poses, points, levels [n_e], stages [2], pose_stages [n_kf], point_stages [n_pt] (bit s: the vertex had an active
    edge in stage s), n_level1, log)"""
    poses0, points0 = np.array(prob["poses"], np.float64).reshape(-1, 7), np.array(prob["points"], np.float64).reshape(-1, 3)
    n_e = len(prob["edge_pt"])
    nf = int(np.sum(np.asarray(prob["fixed"]) == 0))
    out = dict(status=OK, poses=poses0.copy(), points=points0.copy(), levels=np.zeros(n_e, np.int32), stages=[None, None],
               pose_stages=np.zeros(len(poses0), np.int32), point_stages=np.zeros(len(points0), np.int32), n_level1=0, log=[])
    if len(poses0) == 0 or len(points0) == 0:
        out["status"] = EMPTY
        return out
    if n_e == 0 or not np.any(prob["edge_kf"] < nf):
        out["status"] = NO_EDGES
        return out
    poses, points = poses0.copy(), points0.copy()
    active = np.ones(n_e, bool)
    for stage in range(2):
        if stage == 1:
            err, z, _, _ = edge_terms(poses, points, prob["edge_pt"], prob["edge_kf"], prob["edge_uv"], prob["cam"], jac=False)
            with np.errstate(all="ignore"):
                bad = (np.sum(err * err, 1) > CHI2_TH) | ~(z > 0.0)
            out["levels"] = bad.astype(np.int32)
            out["n_level1"] = int(bad.sum())
            active = ~bad
            if not np.any(active & (prob["edge_kf"] < nf)):
                break                       # nothing left to solve: the stage is not run
        np.bitwise_or.at(out["pose_stages"], prob["edge_kf"][active], 1 << stage)
        np.bitwise_or.at(out["point_stages"], prob["edge_pt"][active], 1 << stage)
        res = run_stage(prob, poses, points, active, stage == 0, stage_its[stage], out["log"], stage)
        if res is None:
            out.update(status=NONFINITE, levels=np.zeros(n_e, np.int32), n_level1=0)
            return out
        poses, points, out["stages"][stage] = res
    out["poses"], out["points"] = poses, points
    return out
