"""ImageAlign::ComputePose, Optimize, ComputeResiduals and PrecomputePatches (image_align.cc:46-267) restated in float64 numpy from
the reference's text, not from oracle/ref_align.h or csrc/sdvl_image_align.hip: what tests/test_oracle_align_independent.py holds
the oracle's sparse image alignment against.

Nothing here calls the oracle and nothing here is float32.  The reference rounds the level position, the four bilinear weights,
every interpolated intensity, gradient and residual and the running chi2 to float (image_align.cc:141-192, 214-260); here they are
float64 throughout, so the distance measured to the oracle is the size of "the same mathematics, rounded otherwise".  The normal
equations are summed by numpy over all measured pixels at once and solved by numpy.linalg.solve (lstsq where that reports a singular
matrix), where the reference accumulates pixel by pixel and solves with Eigen's pivoted LDLT (:102): on a system of full rank the
two agree to rounding, H = 0 gives x = 0 in both, and a non-finite system gives a non-finite x in both.  The two pyramids are inputs
(Frame::GetPyramid).  The SE3 exponential and product are those of tests/pose_restatement.py (extra/se3.cc).

floorf of a NaN or of a value beyond int is undefined where the reference converts it to int (:167-168); the x86 conversion
yields INT_MIN, which the border test of :171 rejects, and that is what is restated: a projection that is not finite is outside.

restate(...) returns dict(T, n, its, error, chi2, stop, evals, trace).  trace counts how often each branch was taken (BRANCHES).
fault=<name> plants exactly one error, see FAULTS."""
import numpy as np

from pose_restatement import quat_to_rot, se3_exp, se3_mul

FAULTS = {
    "update_side": "Exp(-x) * T in place of T * Exp(-x) (image_align.cc:116)",
    "jacobian_at_current_point": "Jacobian3DToPlane taken at the point in the current frame, at every evaluation (:238)",
    "focal_not_scaled": "the Jacobian is scaled by fx in place of fx / 2^level (:263)",
    "depth_is_z": "the feature's depth read as the z of its point, not as its distance from the camera centre (:159-160, :234-235)",
    "h_keeps_departed": "H summed over the level's visible set although some of it projects outside the current image (:171-172, :198)",
    "border_gt": "> in place of >= in the current image's border test (:171)",
    "rollback_keeps_current": "the roll-back on rising chi2 keeps the current pose (:110)",
    "chi2_compared_at_it0": "a level's first evaluation is compared with the chi2 of the level before, too (:109)",
    "stop_not_sticky": "stop_ is cleared at the start of every level (:36, :99, :109)",
    "fast_ignored": "the early-out of a fast call is not taken (:73-76)",
    "invalid_counted": "features without a live point are precomputed and measured (:155, :229)",
}
BRANCHES = ("rollback", "step_stop", "out_of_its", "set_changed_it0", "set_changed_later", "fast_early_out", "stop_n_meas", "stop_nan")


def jacobian_3d_to_plane(p):
    """extra/utils.cc:99-118 for points p[n][3] -> [n][2][6]"""
    with np.errstate(all="ignore"):
        x, y = p[:, 0], p[:, 1]
        z_inv = 1.0 / p[:, 2]
        z_inv_2 = z_inv * z_inv
        J = np.zeros((len(p), 2, 6))
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


def _bilinear(img, ui, vi, su, sv, psize, dc=0, dr=0):
    """the patch of psize x psize bilinear sums whose pixel (x, y) has its top-left neighbour at column ui - psize/2 + x + dc, row
    vi - psize/2 + y + dr (:184-188, :250-260) -> [n][psize*psize], row-major like pixel_counter"""
    half = psize // 2
    ys, xs = np.mgrid[0:psize, 0:psize]
    r = vi[:, None] + (ys.ravel() - half + dr)[None, :]
    c = ui[:, None] + (xs.ravel() - half + dc)[None, :]
    w_tl = ((1.0 - su) * (1.0 - sv))[:, None]
    w_tr = (su * (1.0 - sv))[:, None]
    w_bl = ((1.0 - su) * sv)[:, None]
    w_br = (su * sv)[:, None]
    return w_tl * img[r, c] + w_tr * img[r, c + 1] + w_bl * img[r + 1, c] + w_br * img[r + 1, c + 1]


class _Align:
    def __init__(self, pyr1, pyr2, cam, px, bearing, depth, valid, max_level, min_level, max_its, patch_size, fault):
        assert fault is None or fault in FAULTS, fault
        self.pyr1 = [np.asarray(p, np.float64) for p in pyr1]
        self.pyr2 = [np.asarray(p, np.float64) for p in pyr2]
        self.fx, self.fy, self.u0, self.v0 = (float(c) for c in cam)
        self.px = np.asarray(px, np.float64).reshape(-1, 2)
        f = np.asarray(bearing, np.float64).reshape(-1, 3)
        depth = np.asarray(depth, np.float64)
        self.valid = np.asarray(valid).astype(bool)
        if fault == "invalid_counted":
            self.valid = np.ones_like(self.valid)
        with np.errstate(all="ignore"):
            if fault == "depth_is_z":
                self.xyz_ref = f * (depth / f[:, 2])[:, None]
            else:
                self.xyz_ref = f * depth[:, None]                      # :160 = :235
        self.max_level, self.min_level, self.max_its, self.psize, self.fault = max_level, min_level, max_its, patch_size, fault
        n, area = len(self.px), patch_size * patch_size
        # :35-41, :61-63
        self.stop, self.chi2, self.error, self.n_meas = False, 1e10, 1e10, 0
        self.patch_cache = np.zeros((n, area))
        self.jac = np.zeros((n, area, 6))
        self.visible = np.zeros(n, bool)
        self.its = np.zeros(8, np.int32)
        self.evals = 0
        self.trace = dict.fromkeys(BRANCHES, 0)

    # :208-267
    def precompute(self, level):
        psize, border = self.psize, self.psize // 2 + 1
        img = self.pyr1[level]
        rows, cols = img.shape
        scale = 1.0 / (1 << level)
        u_ref, v_ref = self.px[:, 0] * scale, self.px[:, 1] * scale
        ui, vi = np.floor(u_ref).astype(np.int64), np.floor(v_ref).astype(np.int64)
        ok = self.valid & ~((ui - border < 0) | (vi - border < 0) | (ui + border >= cols) | (vi + border >= rows))     # :229
        idx = np.nonzero(ok)[0]
        self.visible[idx] = True                                                                                       # :231
        self.level_set = ok
        ui, vi = ui[idx], vi[idx]
        su, sv = u_ref[idx] - ui, v_ref[idx] - vi
        self.patch_cache[idx] = _bilinear(img, ui, vi, su, sv, psize)                                                   # :253
        dx = 0.5 * (_bilinear(img, ui, vi, su, sv, psize, dc=1) - _bilinear(img, ui, vi, su, sv, psize, dc=-1))        # :257-258
        dy = 0.5 * (_bilinear(img, ui, vi, su, sv, psize, dr=1) - _bilinear(img, ui, vi, su, sv, psize, dr=-1))        # :259-260
        self.grad = np.zeros((len(self.px), psize * psize, 2))
        self.grad[idx, :, 0], self.grad[idx, :, 1] = dx, dy
        self.fl = self.fx if self.fault == "focal_not_scaled" else self.fx / (1 << level)
        fj = jacobian_3d_to_plane(self.xyz_ref[idx])                                                                    # :238
        with np.errstate(all="ignore"):
            self.jac[idx] = (dx[:, :, None] * fj[:, None, 0, :] + dy[:, :, None] * fj[:, None, 1, :]) * self.fl         # :263

    # :127-206
    def residuals(self, T, level, patches):
        self.evals += 1
        psize, border = self.psize, self.psize // 2 + 1
        img = self.pyr2[level]
        rows, cols = img.shape
        if patches:
            self.precompute(level)
            self.last_set = self.level_set.copy()
        scale = 1.0 / (1 << level)
        R, t = quat_to_rot(T[:4]), T[4:]
        cand = np.nonzero(self.visible & self.valid)[0]                                                                # :151-156
        with np.errstate(all="ignore"):
            xyz_cur = self.xyz_ref[cand] @ R.T + t                                                                      # :161
            u = (self.u0 + self.fx * xyz_cur[:, 0] / xyz_cur[:, 2]) * scale                                             # :163-164, camera.cc
            v = (self.v0 + self.fy * xyz_cur[:, 1] / xyz_cur[:, 2]) * scale
            finite = np.isfinite(u) & np.isfinite(v)
            fu, fv = np.floor(np.where(finite, u, -1.0)), np.floor(np.where(finite, v, -1.0))
            if self.fault == "border_gt":
                inside = finite & ~((fu < 0) | (fv < 0) | (fu - border < 0) | (fv - border < 0) | (fu + border > cols) | (fv + border > rows))
            else:
                inside = finite & ~((fu < 0) | (fv < 0) | (fu - border < 0) | (fv - border < 0) | (fu + border >= cols) | (fv + border >= rows))
        m = cand[inside]
        now = np.zeros(len(self.px), bool)
        now[m] = True
        if not np.array_equal(now, self.last_set):
            self.trace["set_changed_it0" if patches else "set_changed_later"] += 1
        self.last_set = now
        ui, vi = fu[inside].astype(np.int64), fv[inside].astype(np.int64)
        su, sv = u[inside] - ui, v[inside] - vi
        res = _bilinear(img, ui, vi, su, sv, psize) - self.patch_cache[m]                                               # :188-189
        self.n_meas = res.size                                                                                         # :193
        J = self.jac[m]
        if self.fault == "jacobian_at_current_point":
            fj = jacobian_3d_to_plane(xyz_cur[inside])
            g = self.grad[m]
            J = (g[:, :, 0, None] * fj[:, None, 0, :] + g[:, :, 1, None] * fj[:, None, 1, :]) * self.fl
        with np.errstate(all="ignore"):
            Jh = self.jac[np.nonzero(self.level_set)[0]] if self.fault == "h_keeps_departed" else J
            H = np.einsum("npr,npc->rc", Jh, Jh)                                                                        # :198
            Jres = -np.einsum("npr,np->r", J, res)                                                                      # :199
            chi2 = float((res * res).sum()) / self.n_meas if self.n_meas else np.nan                                    # :192, :205
        return chi2, H, Jres

    @staticmethod
    def solve(H, Jres):                                                                                                # :102
        if not (np.isfinite(H).all() and np.isfinite(Jres).all()):
            return np.full(6, np.nan)
        try:
            return np.linalg.solve(H, Jres)
        except np.linalg.LinAlgError:
            return np.linalg.lstsq(H, Jres, rcond=None)[0]

    # :86-125
    def optimize(self, T, level):
        T_bk = T.copy()
        if self.fault == "stop_not_sticky":
            self.stop = False
        for i in range(self.max_its):
            new_chi2, H, Jres = self.residuals(T, level, i == 0)
            if self.n_meas == 0:                                                                                       # :98-99
                self.stop = True
                self.trace["stop_n_meas"] += 1
            x = self.solve(H, Jres)
            if np.isnan(x[0]):                                                                                         # :103-106
                self.stop = True
                self.trace["stop_nan"] += 1
            first = i == 0 and self.fault != "chi2_compared_at_it0"
            if (not first and new_chi2 > self.chi2) or self.stop:                                                      # :109-112
                self.trace["rollback"] += 1
                return T if self.fault == "rollback_keeps_current" else T_bk
            T_bk = T.copy()
            T = se3_mul(se3_exp(-x), T) if self.fault == "update_side" else se3_mul(T, se3_exp(-x))                     # :115-116
            self.chi2 = new_chi2
            self.its[level] += 1
            self.error = float(np.abs(x).max())                                                                        # :121
            if self.error <= 1e-10:
                self.trace["step_stop"] += 1
                return T
        if self.max_its > 0:
            self.trace["out_of_its"] += 1
        return T

    # :46-84
    def compute_pose(self, T0, fast):
        T = np.array(T0, np.float64)
        if len(self.px) == 0:                                                                                          # :54-58
            return T
        for level in range(self.max_level, self.min_level - 1, -1):
            self.jac[:] = 0.0                                                                                          # :69
            T = self.optimize(T, level)
            if fast and self.fault != "fast_ignored" and self.error > 0.01:                                            # :73-76
                self.error = 1e10
                self.trace["fast_early_out"] += 1
                break
        return T


def restate(pyr1, pyr2, cam, px, bearing, depth, valid, T0, max_level=4, min_level=2, max_its=30, patch_size=4, fast=False, fault=None):
    a = _Align(pyr1, pyr2, cam, px, bearing, depth, valid, max_level, min_level, max_its, patch_size, fault)
    T = a.compute_pose(T0, fast)
    return dict(T=T, n=a.n_meas // (patch_size * patch_size), its=a.its, error=a.error, chi2=a.chi2, stop=int(a.stop), evals=a.evals,
                trace=a.trace)
