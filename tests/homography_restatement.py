"""numpy float64 restatement of the two-frame initialisation behind the tracked points: the RANSAC of
cv::findHomography(src, dst, CV_RANSAC, 2 / fx) (homography_init.cc:253) and HomographyInit's own arithmetic
(homography_init.cc:83-183, 237-327, 329-533), written from OpenCV's algorithm (modules/calib3d/src/ptsetreg.cpp, fundam.cpp)
and the reference's lines, not from csrc/sdvl_init.hip or host/homography_init.cc.

ransac() is the specification of sdvl_homography_ransac.  The caller supplies the 4-index subsets (it owns the random stream);
the loop is the sequential one of RANSACPointSetRegistrator::run:
  * draws are walked in order, at most min(max_its, number of draws given), and while it < budget;
  * a draw with a repeated index, or with three of its four points collinear in src or in dst (OpenCV's haveCollinearPoints test:
    |dx2 dy1 - dy2 dx1| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|)), is skipped and still counts as an iteration;
  * H of the four points with H22 = 1 (here: the 8 x 8 system of the DLT solved by LAPACK);
  * a match supports H when |dst - H src|^2 <= threshold^2;
  * a count above max(best count, 3) becomes the best, and the budget becomes RANSACUpdateNumIters(confidence,
    (n - count) / n, 4, budget): log(1 - confidence) / log(1 - w^4) rounded to nearest-even, never above the old budget;
  * n_its = draws walked, inliers = ascending indices of the best draw's supporters.
OpenCV redraws a degenerate subset from its own generator and special-cases n == 4; neither is restated: a degenerate draw is an
iteration without a model, and n == 4 takes the same loop.

init_from_tracks() is ComputeHomography and the scaling of InitSecondFrame: correspondences rounded to float32 (cv::Point2f,
:248-249), RANSAC, the DLT refit of H on the inliers (Hartley normalisation, the smallest eigenvector of the 9x9; OpenCV's
Levenberg-Marquardt polish is left out), DecomposeHomography, CheckInliers (whose threshold is InlierErrorThreshold() unscaled,
:294: in normalised coordinates every match passes), ChooseBestDecomposition, CheckDecompositionInliers, the median-depth scale."""
import math

import numpy as np

FLT_EPSILON = 1.1920928955078125e-07
DBL_MIN = 2.2250738585072014e-308
DBL_EPSILON = 2.220446049250313e-16
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


# ------------------------------------------------------------------------------------------------ RANSAC (the device stage)
def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters, ptsetreg.cpp"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def collinear3(p, i, j, k):
    dx1, dy1 = p[j][0] - p[i][0], p[j][1] - p[i][1]
    dx2, dy2 = p[k][0] - p[i][0], p[k][1] - p[i][1]
    return abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2))


def degenerate(idx, src, dst):
    if len(set(int(i) for i in idx)) < 4:
        return True
    s, d = [src[i] for i in idx], [dst[i] for i in idx]
    return any(collinear3(s, *t) or collinear3(d, *t) for t in TRIPLES)


def homography4(s, d):
    """H with d_i ~ H s_i for four correspondences, H22 = 1: the 8 x 8 linear system of the direct linear transform, solved by LAPACK
    (the device forms the same H in closed form through projective bases; the two agree to rounding)"""
    A, b = [], []
    for (x, y), (u, v) in zip(s, d):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y]); b.append(u)
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y]); b.append(v)
    h = np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64))
    return np.append(h, 1.0).reshape(3, 3)


def reprojection_d2(H, src, dst):
    x, y = src[:, 0], src[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (H[2, 0] * x + H[2, 1] * y) + H[2, 2]
        dx = ((H[0, 0] * x + H[0, 1] * y) + H[0, 2]) / w - dst[:, 0]
        dy = ((H[1, 0] * x + H[1, 1] * y) + H[1, 2]) / w - dst[:, 1]
        return dx * dx + dy * dy


def ransac(src, dst, draws4, threshold, max_its=2000, confidence=0.995):
    """-> dict(best_draw, n_its, inliers, H, d2 (of the best draw, for the tests' borderline screen))"""
    src = np.asarray(src, np.float64).reshape(-1, 2)
    dst = np.asarray(dst, np.float64).reshape(-1, 2)
    draws4 = np.asarray(draws4, np.int64).reshape(-1, 4)
    n = len(src)
    budget = min(max_its, len(draws4))
    best, best_count, best_H, best_d2 = -1, 3, np.zeros((3, 3)), np.zeros(n)
    t2 = threshold * threshold
    it = 0
    while it < budget:
        idx = draws4[it]
        it += 1
        if degenerate(idx, src, dst):
            continue
        H = homography4([src[i] for i in idx], [dst[i] for i in idx])
        d2 = reprojection_d2(H, src, dst)
        count = int(np.count_nonzero(d2 <= t2))
        if count > best_count:
            best, best_count, best_H, best_d2 = it - 1, count, H, d2
            budget = min(budget, update_num_iters(confidence, (n - count) / n, 4, budget))
    inl = np.nonzero(best_d2 <= t2)[0] if best >= 0 else np.zeros(0, np.int64)
    return dict(best_draw=best, n_its=it, inliers=inl.astype(np.int32), H=best_H, d2=best_d2)


# ------------------------------------------------------------------------------------------------ the host stage
def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def refit_dlt(src, dst):
    """H of all the given matches: Hartley normalisation, the eigenvector of the smallest eigenvalue of A^T A (fundam.cpp runKernel)"""
    def norm(p):
        c = p.mean(0)
        s = np.abs(p - c).mean(0)
        s = 1.0 / np.where(s > DBL_EPSILON, s, 1.0)
        return np.array([[s[0], 0, -c[0] * s[0]], [0, s[1], -c[1] * s[1]], [0, 0, 1.0]])
    T1, T2 = norm(src), norm(dst)
    a = np.c_[src, np.ones(len(src))] @ T1.T
    b = np.c_[dst, np.ones(len(dst))] @ T2.T
    rows = []
    for (x, y, _), (u, v, _) in zip(a, b):
        rows.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
        rows.append([0, 0, 0, x, y, 1, -v * x, -v * y, -v])
    A = np.array(rows)
    _, vec = np.linalg.eigh(A.T @ A)
    H = np.linalg.inv(T2) @ vec[:, 0].reshape(3, 3) @ T1
    return H / H[2, 2]


def decompose(H):
    """DecomposeHomography, homography_init.cc:329-443 -> list of 8 dict(R, t, n, d), or None (a degenerate motion case)"""
    U, sv, Vt = np.linalg.svd(H)
    V = Vt.T
    d1, d2, d3 = np.abs(sv)
    s = np.linalg.det(U) * np.linalg.det(V)
    if not (d1 != d2 and d2 != d3):
        return None
    x1 = math.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    x3 = math.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    e1, e3 = (1.0, -1.0, 1.0, -1.0), (1.0, 1.0, -1.0, -1.0)
    out = []
    for k in range(4):                                   # d' > 0, eq. 13-14
        sin_t = (d1 - d3) * x1 * x3 * e1[k] * e3[k] / d2
        cos_t = (d1 * x3 * x3 + d3 * x1 * x1) / d2
        Rp = np.array([[cos_t, 0, -sin_t], [0, 1, 0], [sin_t, 0, cos_t]])
        tp = np.array([(d1 - d3) * x1 * e1[k], 0.0, (d1 - d3) * -x3 * e3[k]])
        out.append(dict(Rp=Rp, tp=tp, n=V @ np.array([x1 * e1[k], 0.0, x3 * e3[k]]), d=s * d2))
    for k in range(4):                                   # d' < 0, eq. 15-16
        sin_p = (d1 + d3) * x1 * x3 * e1[k] * e3[k] / d2
        cos_p = (d3 * x1 * x1 - d1 * x3 * x3) / d2
        Rp = np.array([[cos_p, 0, sin_p], [0, -1, 0], [sin_p, 0, -cos_p]])
        tp = np.array([(d1 + d3) * x1 * e1[k], 0.0, (d1 + d3) * x3 * e3[k]])
        out.append(dict(Rp=Rp, tp=tp, n=V @ np.array([x1 * e1[k], 0.0, x3 * e3[k]]), d=s * -d2))
    for dec in out:
        dec["R"] = s * U @ dec["Rp"] @ V.T
        dec["t"] = U @ dec["tp"]
    return out


def sampson(E, s, d):
    v3 = np.array([s[0], s[1], 1.0])
    v3d = np.array([d[0], d[1], 1.0])
    fv, ftv = E @ v3, E.T @ v3d
    e = fv @ v3d
    return e * e / (fv[:2] @ fv[:2] + ftv[:2] @ ftv[:2])


def choose(decs, H, src, dst, inliers, inlier_error_threshold):
    """ChooseBestDecomposition, :449-533 -> (the decomposition, the two visibility scores of the second round)"""
    for dec in decs:
        dec["score"] = -sum(1 for i in inliers if (H[2, 0] * src[i, 0] + H[2, 1] * src[i, 1] + H[2, 2]) / dec["d"] > 0.0)
    decs = sorted(decs, key=lambda q: q["score"])[:4]    # std::sort on the score alone; ties are decided by the second round
    for dec in decs:
        dec["score"] = -sum(1 for i in inliers if (np.array([src[i, 0], src[i, 1], 1.0]) @ dec["n"]) / dec["d"] > 0.0)
    decs = sorted(decs, key=lambda q: q["score"])[:2]
    scores = (-decs[0]["score"], -decs[1]["score"])
    if decs[1]["score"] / decs[0]["score"] < 0.9:
        return decs[0], scores
    limit = inlier_error_threshold * inlier_error_threshold * 4
    tot = []
    for dec in decs:
        E = np.stack([np.cross(dec["t"], dec["R"][:, j]) for j in range(3)], 1)
        tot.append(sum(min(sampson(E, src[m], dst[m]), limit) for m in range(len(src))))
    return (decs[0] if tot[0] <= tot[1] else decs[1]), scores


def triangulate(R, T, v1, v2):
    """extra/utils.cc:133-159"""
    v2 = R @ v2
    b = np.array([T @ v1, T @ v2])
    A = np.array([[v1 @ v1, -(v1 @ v2)], [v1 @ v2, -(v2 @ v2)]])
    lam = np.linalg.inv(A) @ b
    return (lam[0] * v1 + T + lam[1] * v2) / 2


def init_from_tracks(px1, px2, cam, draws4, inlier_error_threshold=2.0, map_scale=1.0, max_its=2000, confidence=0.995):
    """px1, px2: the tracked pixels of frame 1 and frame 2 (float32, as pixels1_ / pixels2_); cam = fx fy u0 v0.
    -> dict(R, t (frame 1 -> frame 2, scaled), scores, n_h_inliers, inliers, depth_median, n_its) or dict(failed=...)"""
    fx, fy, u0, v0 = [float(c) for c in cam]

    def unproject(px):                                   # Camera::Unproject (camera.h): the unit ray of a pixel
        v = np.stack([(px[:, 0] - u0) / fx, (px[:, 1] - v0) / fy, np.ones(len(px))], 1)
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    px1 = np.asarray(px1, np.float32).astype(np.float64)
    px2 = np.asarray(px2, np.float32).astype(np.float64)
    v1, v2 = unproject(px1), unproject(px2)
    src = (v1[:, :2] / v1[:, 2:3]).astype(np.float32).astype(np.float64)   # cv::Point2f, :248-249
    dst = (v2[:, :2] / v2[:, 2:3]).astype(np.float32).astype(np.float64)
    r = ransac(src, dst, draws4, 2.0 / fx, max_its, confidence)
    if r["best_draw"] < 0:
        return dict(failed="ransac")
    inl = r["inliers"]
    H = refit_dlt(src[inl], dst[inl])
    decs = decompose(H)
    if decs is None:
        return dict(failed="decompose")
    err = np.sqrt(reprojection_d2(H, src, dst))
    h_inl = [i for i in range(len(src)) if err[i] <= inlier_error_threshold]        # CheckInliers, :284-297
    best, scores = choose(decs, H, src, dst, h_inl, inlier_error_threshold)
    R, T = best["R"], best["t"]
    tri, inliers = [], []
    for i in range(len(src)):                            # CheckDecompositionInliers, :299-327
        xyz = triangulate(R, T, v2[i], v1[i])
        tri.append(xyz)
        e1 = np.linalg.norm(v2[i, :2] / v2[i, 2] - xyz[:2] / xyz[2]) * fx
        pc = R.T @ (xyz - T)
        e2 = np.linalg.norm(v1[i, :2] / v1[i, 2] - pc[:2] / pc[2]) * fx
        if e1 <= inlier_error_threshold and e2 <= inlier_error_threshold:
            inliers.append(i)
    tri = np.array(tri)
    z = np.sort(tri[:, 2])
    depth = z[len(z) // 2]                               # GetMedianVector, extra/utils.cc:215-220
    scale = map_scale / depth
    # frame 1 at the identity: frame 2's centre is -R^T T, scaled; its translation is -R * centre (:119-121)
    centre = scale * (-R.T @ T)
    return dict(R=R, t=-R @ centre, scores=scores, n_ransac_inliers=len(inl), n_h_inliers=len(h_inl), inliers=np.array(inliers),
                depth_median=depth, n_its=r["n_its"], H=H, tri=tri)
