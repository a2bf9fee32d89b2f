"""numpy float64 restatement of local bundle adjustment with depth edges: the specification of sdvl_bundle_adjust_depth.
Layered on tests/bundle_restatement.py (the monocular specification, imported and left as it is) and written from the g2o sources the
reference ships (types_six_dof_expmap.cpp:150-234, EdgeStereoSE3ProjectXYZ), not from csrc/sdvl_bundle.hip.

A problem is the dict of bundle_restatement.py with two additions: edge_d [n_e], the measured camera-frame z of the observation in
metres (0: none), and bf in pixel * metres.

  edge_d <= 0   EdgeSE3ProjectXYZ in every respect: two rows, Huber delta^2 = 5.991, level 1 when chi2 > 5.991 or z <= 0
  edge_d  > 0   EdgeStereoSE3ProjectXYZ, information I: err = (u - u', v - v', (u - bf/d) - (u' - bf/z)) with (u', v') the
                projection and z the camera-frame depth of the point; rows 0 and 1 of both Jacobians are the monocular edge's, row 2 is
                row 0 plus the bf terms of linearizeOplus (:210-212, :228-233); Huber delta^2 = 7.815; level 1, as a whole, when
                chi2 > 7.815 or z <= 0 (7.815: the 95 % point of chi2 with three degrees of freedom, as 5.991 is with two)
  the rest      LM schedule, Schur complement, Cholesky, stages, statuses, "settled" trials: bundle_restatement.py

One unit of the third residual is dz * bf / z^2: bf converts depth noise to pixels.

What g2o leaves implicit and this file states, beyond the list in bundle_restatement.py:
  * cam_project's 1/z is a double (a float in g2o, :151), and u' is fx x / z + cx exactly as in the monocular edge;
  * sums over the three rows run ((r0 + r1) + r2): chi2 = (e0 e0 + e1 e1) + e2 e2, and every product J^T J, J^T e alike, so that
    a third row of zeros leaves the monocular bits;
  * rows 0 and 1 of the point Jacobian are the monocular -1/z tmp R (:202-208 writes the same thing as -fx R/z + fx x R/z^2);
  * the information matrix is I;
  * the two thresholds above, and each edge's Huber delta is sqrt() of its own threshold."""
import math

import numpy as np

import bundle_restatement as br
from bundle_restatement import EMPTY, NO_EDGES, NONFINITE, OK, STAGE_ITS  # noqa: F401  (the statuses are shared)

CHI2_TH_MONO = br.CHI2_TH
CHI2_TH_DEPTH = 7.815


def thresholds(edge_d):
    """the outlier threshold (= Huber delta^2) of every edge"""
    return np.where(np.asarray(edge_d, np.float64) > 0.0, CHI2_TH_DEPTH, CHI2_TH_MONO)


def edge_terms(poses, points, edge_pt, edge_kf, edge_uv, edge_d, cam, bf, jac=True):
    """-> err [n][3], z [n], Ji [n][3][3] (point), Jj [n][3][6] (pose); the third row of an edge without a depth is zero"""
    err2, z, Ji2, Jj2 = br.edge_terms(poses, points, edge_pt, edge_kf, edge_uv, cam, jac=jac)
    fx, _, cx, _ = cam
    n = len(z)
    has = np.asarray(edge_d, np.float64) > 0.0
    R = br.quat_to_rot(poses[:, :4])[edge_kf]
    Xc = np.einsum("nij,nj->ni", R, points[edge_pt]) + poses[edge_kf, 4:]
    x, y = Xc[:, 0], Xc[:, 1]
    err = np.zeros((n, 3))
    err[:, :2] = err2
    with np.errstate(all="ignore"):
        d = np.where(has, edge_d, 1.0)
        e3 = (edge_uv[:, 0] - bf / d) - ((fx * x / z + cx) - bf / z)
        err[:, 2] = np.where(has, e3, 0.0)
        if not jac:
            return err, z, None, None
        z2 = z * z
        Ji, Jj = np.zeros((n, 3, 3)), np.zeros((n, 3, 6))
        Ji[:, :2], Jj[:, :2] = Ji2, Jj2
        Ji3 = Ji2[:, 0, :] - bf * R[:, 2, :] / z2[:, None]
        Jj3 = Jj2[:, 0, :].copy()
        Jj3[:, 0] = Jj2[:, 0, 0] - bf * y / z2
        Jj3[:, 1] = Jj2[:, 0, 1] + bf * x / z2
        Jj3[:, 5] = Jj2[:, 0, 5] - bf / z2
        Ji[:, 2] = np.where(has[:, None], Ji3, 0.0)
        Jj[:, 2] = np.where(has[:, None], Jj3, 0.0)
    return err, z, Ji, Jj


def chi2_rows(err):
    return (err[:, 0] * err[:, 0] + err[:, 1] * err[:, 1]) + err[:, 2] * err[:, 2]


def huber(e, th):
    """rho[0], rho[1] of robust_kernel_impl.cpp:78-91 for e = err.err with delta = sqrt(th) per edge"""
    with np.errstate(all="ignore"):
        delta = np.sqrt(th)
        s = np.sqrt(e)
        inl = e <= delta * delta
        return np.where(inl, e, 2 * s * delta - delta * delta), np.where(inl, 1.0, delta / s)


def jtj(A, B):
    """sum over the three rows of A[:, k, :, None] * B[:, k, None, :], in the order ((r0 + r1) + r2)"""
    t = [A[:, k, :, None] * B[:, k, None, :] for k in range(3)]
    return (t[0] + t[1]) + t[2]


def jte(A, err):
    t = [A[:, k, :] * err[:, k, None] for k in range(3)]
    return (t[0] + t[1]) + t[2]


class System(br.System):
    """H and b of the active edges with three-row edges; max_diagonal() and solve() are the monocular system's"""

    def __init__(self, prob, poses, points, active, robust):
        self.n_free = nf = int(np.sum(np.asarray(prob["fixed"]) == 0))
        self.n_pt = npt = len(points)
        ept, ekf, euv, ed = prob["edge_pt"][active], prob["edge_kf"][active], prob["edge_uv"][active], prob["edge_d"][active]
        err, _, Ji, Jj = edge_terms(poses, points, ept, ekf, euv, ed, prob["cam"], prob["bf"])
        e = chi2_rows(err)
        w = huber(e, thresholds(ed))[1] if robust else np.ones(len(e))
        self.Hpp, self.bp = np.zeros((nf, 6, 6)), np.zeros((nf, 6))
        self.Hll, self.bl = np.zeros((npt, 3, 3)), np.zeros((npt, 3))
        np.add.at(self.Hll, ept, w[:, None, None] * jtj(Ji, Ji))
        np.add.at(self.bl, ept, -w[:, None] * jte(Ji, err))
        free = ekf < nf
        self.f_pt, self.f_kf = ept[free], ekf[free]
        np.add.at(self.Hpp, self.f_kf, w[free, None, None] * jtj(Jj[free], Jj[free]))
        np.add.at(self.bp, self.f_kf, -w[free, None] * jte(Jj[free], err[free]))
        self.W = w[free, None, None] * jtj(Jj[free], Ji[free])        # [n_free_edges][6][3]
        self.pose_on = np.zeros(nf, bool)
        self.pose_on[self.f_kf] = True
        self.pt_on = np.zeros(npt, bool)
        self.pt_on[ept] = True


def chi2_of(prob, poses, points, active, robust):
    ed = prob["edge_d"][active]
    err, _, _, _ = edge_terms(poses, points, prob["edge_pt"][active], prob["edge_kf"][active], prob["edge_uv"][active], ed, prob["cam"], prob["bf"],
                              jac=False)
    e = chi2_rows(err)
    return float(np.sum(huber(e, thresholds(ed))[0] if robust else e))


def run_stage(prob, poses, points, active, robust, n_its, log, stage):
    """bundle_restatement.run_stage over this file's System and chi2_of -> poses, points, stats (None: the initial chi2 is not finite)"""
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
                    new_poses[a] = br.exp_update(poses[a], dp[a])
                new_points = points + dl
                chi_new = chi2_of(prob, new_poses, new_points, active, robust)
            else:
                scale, chi_new = 0.0, br.DBL_MAX
            rho, accepted = br.decide(chi, chi_new, scale, sol is not None)
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
            if not (rho < 0 and q < br.MAX_TRIALS):
                break
        st["iterations"] += 1
        st["trials"] += q
        st["trials_per_it"].append(q)
        st["accepted_its"].append(accepted)
        st["chi2_after"] = chi
        if q == br.MAX_TRIALS or rho == 0:
            break
        n_bad = n_bad + 1 if (chi0 - chi) * 1e3 < chi0 else 0
        if n_bad >= 3:
            break
    st["lam"] = lam
    return poses, points, st


def classify(prob, poses, points):
    """the outlier test after stage 1 -> bad [n_e]"""
    err, z, _, _ = edge_terms(poses, points, prob["edge_pt"], prob["edge_kf"], prob["edge_uv"], prob["edge_d"], prob["cam"], prob["bf"], jac=False)
    with np.errstate(all="ignore"):
        return (chi2_rows(err) > thresholds(prob["edge_d"])) | ~(z > 0.0)


def bundle_adjust(prob, stage_its=STAGE_ITS):
    """-> the dict of bundle_restatement.bundle_adjust"""
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
            bad = classify(prob, poses, points)
            out["levels"] = bad.astype(np.int32)
            out["n_level1"] = int(bad.sum())
            active = ~bad
            if not np.any(active & (prob["edge_kf"] < nf)):
                break
        np.bitwise_or.at(out["pose_stages"], prob["edge_kf"][active], 1 << stage)
        np.bitwise_or.at(out["point_stages"], prob["edge_pt"][active], 1 << stage)
        res = run_stage(prob, poses, points, active, stage == 0, stage_its[stage], out["log"], stage)
        if res is None:
            out.update(status=NONFINITE, levels=np.zeros(n_e, np.int32), n_level1=0)
            return out
        poses, points, out["stages"][stage] = res
    out["poses"], out["points"] = poses, points
    return out
