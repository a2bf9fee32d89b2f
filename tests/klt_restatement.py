"""numpy restatement of cv::calcOpticalFlowPyrLK as HomographyInit::TrackSecondFrame calls it (homography_init.cc:195-198:
window 30x30, maxLevel 4, 30 iterations or |delta| <= 0.001, OPTFLOW_USE_INITIAL_FLOW, min-eigen threshold 1e-4), written from
OpenCV's algorithm (modules/video/src/lkpyramid.cpp, LKTrackerInvoker), not from the device code.  It is the specification of
sdvl_klt_track.

What is OpenCV's: the coarse-to-fine loop, the window placed at p / 2^l - 14.5, the bilinear weights (1-a)(1-b), a(1-b), (1-a)b and
1 minus their sum, the 2x2 matrix of the template's Scharr gradients in OpenCV's units (gradient and intensity products times
2^-10: its 32-fold values times FLT_SCALE = 2^-20), the min-eigenvalue of that matrix over 2 * 900 against the threshold and the
determinant against FLT_EPSILON (level 0: the point is lost; other levels: the level is skipped), the window tests
(floor < -30 or >= size: level 0 loses the point), delta = -G^-1 b, the stop at delta.delta <= eps^2 (in double), and the
oscillation rule (j > 0, |delta + delta_prev| < 0.01 in both components: half the step is taken back).

What is stated here instead of pinned to OpenCV: arithmetic is plain floating point of `dtype` (OpenCV rounds the
template and the samples to 1/32 grey level in fixed point); reads outside a level clamp to its edge, and the gradients
are those of the level so extended (OpenCV pads its own pyramid by reflection and sets the derivative to zero outside); the levels
are the caller's (the frames' pyrDown pyramids; OpenCV would drop levels no larger than the window); and a point whose level-0 result lies outside the image [0, w) x [0, h) is lost (OpenCV keeps it while the window's corner is
inside).  err is the mean absolute difference of the window at the result, level 0."""
import numpy as np

FLT_EPSILON = 1.1920928955078125e-07


def scharr(img, dtype, pad):
    """(3, 10, 3) / 32 gradients of the level EXTENDED by clamping, at every pixel of the level and `pad` pixels around it (left of
    the image the x gradient is zero, above it the x gradient of the first row lives on, ...); exact in float32 (multiples of 1/32)"""
    p = np.pad(img.astype(np.int32), pad + 1, mode="edge")
    dx = p[:, 2:] - p[:, :-2]                       # rows y-1 .. y+1 at x
    gx = 3 * dx[:-2] + 10 * dx[1:-1] + 3 * dx[2:]
    dy = p[2:, :] - p[:-2, :]
    gy = 3 * dy[:, :-2] + 10 * dy[:, 1:-1] + 3 * dy[:, 2:]
    return gx.astype(dtype) * dtype(1.0 / 32.0), gy.astype(dtype) * dtype(1.0 / 32.0)


def _bilinear(img, x0, y0, w00, w01, w10, w11, pad=0):
    """img (already of dtype; its pixel (0, 0) at index (pad, pad)) at the integer corners (x0, y0) .. (x0 + 1, y0 + 1), clamped,
    with the four weights [n, 1]"""
    h, w = img.shape
    x0, y0 = x0 + pad, y0 + pad
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    return ((img[ya, xa] * w00 + img[ya, xb] * w01) + img[yb, xa] * w10) + img[yb, xb] * w11


def _floor_int(v):
    """floor to an integer the way the device converts: NaN -> 0, saturating"""
    f = np.floor(v.astype(np.float64))
    f = np.where(np.isnan(f), 0.0, f)
    return np.clip(f, -2147483648.0, 2147483647.0).astype(np.int64)


def _weights(frac, dtype):
    a, b = frac[:, 0:1], frac[:, 1:2]
    one = dtype(1.0)
    w00 = (one - a) * (one - b)
    w01 = a * (one - b)
    w10 = (one - a) * b
    w11 = one - w00 - w01 - w10
    return w00, w01, w10, w11


def klt_track(prev_pyr, next_pyr, prev_xy, next_xy, win=30, max_level=4, max_its=30, eps=0.001, min_eig_threshold=1e-4,
              dtype=np.float64):
    """prev_pyr / next_pyr: lists of u8 levels; prev_xy [n][2]; next_xy [n][2] the initial flow.
    -> dict(xy [n][2] of dtype, status [n] bool, err [n], min_eig [n] (level 0), its [n] (level 0))"""
    F = dtype
    n = len(prev_xy)
    prev = np.asarray(prev_xy, F).reshape(n, 2)
    out = np.array(next_xy, F).reshape(n, 2)
    half = F((win - 1) * 0.5)
    wy, wx = np.divmod(np.arange(win * win), win)
    status = np.ones(n, bool)
    min_eig0 = np.zeros(n, F)
    its0 = np.zeros(n, np.int32)
    k10 = F(1.0 / 1024.0)
    tmpl0 = None
    for level in range(max_level, -1, -1):
        I, J = prev_pyr[level].astype(F), next_pyr[level].astype(F)
        h, w = I.shape
        gpad = win + 3                  # the window tests keep every sample within win + 1 pixels of the level
        gx, gy = scharr(prev_pyr[level], F, gpad)
        p = prev * F(1.0 / (1 << level))
        nxt = out * F(1.0 / (1 << level)) if level == max_level else out * F(2.0)
        out = nxt.copy()
        pp = p - half
        ip = _floor_int(pp)
        ok = (ip[:, 0] >= -win) & (ip[:, 0] < w) & (ip[:, 1] >= -win) & (ip[:, 1] < h)
        if level == 0:
            status &= ok
        wts = _weights(pp - ip.astype(F), F)
        x0, y0 = ip[:, 0:1] + wx[None, :], ip[:, 1:2] + wy[None, :]
        Iw = _bilinear(I, x0, y0, *wts)
        Ix = _bilinear(gx, x0, y0, *wts, pad=gpad)
        Iy = _bilinear(gy, x0, y0, *wts, pad=gpad)
        A11 = (Ix * Ix).sum(1, dtype=F) * k10
        A12 = (Ix * Iy).sum(1, dtype=F) * k10
        A22 = (Iy * Iy).sum(1, dtype=F) * k10
        D = A11 * A22 - A12 * A12
        with np.errstate(invalid="ignore"):
            min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4.0) * A12 * A12)) / F(2 * win * win)
        bad = (min_eig.astype(np.float64) < min_eig_threshold) | (D < F(FLT_EPSILON))
        if level == 0:
            status &= ~(ok & bad)
            min_eig0 = min_eig
            tmpl0 = Iw
        act = ok & ~bad
        with np.errstate(divide="ignore", invalid="ignore"):
            Dinv = F(1.0) / D
        nw = nxt - half
        prevd = np.zeros((n, 2), F)
        for j in range(max_its):
            idx = np.nonzero(act)[0]
            if len(idx) == 0:
                break
            inx = _floor_int(nw[idx])
            okj = (inx[:, 0] >= -win) & (inx[:, 0] < w) & (inx[:, 1] >= -win) & (inx[:, 1] < h)
            if level == 0:
                status[idx[~okj]] = False
            act[idx[~okj]] = False
            idx, inx = idx[okj], inx[okj]
            if len(idx) == 0:
                break
            if level == 0:
                its0[idx] += 1
            wj = _weights(nw[idx] - inx.astype(F), F)
            Jw = _bilinear(J, inx[:, 0:1] + wx[None, :], inx[:, 1:2] + wy[None, :], *wj)
            diff = Jw - Iw[idx]
            b1 = (diff * Ix[idx]).sum(1, dtype=F) * k10
            b2 = (diff * Iy[idx]).sum(1, dtype=F) * k10
            a11, a12, a22, di = A11[idx], A12[idx], A22[idx], Dinv[idx]
            delta = np.stack([(a12 * b2 - a22 * b1) * di, (a12 * b1 - a11 * b2) * di], 1)
            nw[idx] = nw[idx] + delta
            out[idx] = nw[idx] + half
            d64 = delta.astype(np.float64)
            small = d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1] <= eps * eps
            s = (delta + prevd[idx]).astype(np.float64)
            osc = ~small & (j > 0) & (np.abs(s[:, 0]) < 0.01) & (np.abs(s[:, 1]) < 0.01)
            out[idx[osc]] = out[idx[osc]] - delta[osc] * F(0.5)
            act[idx[small | osc]] = False
            prevd[idx] = delta
    w0, h0 = prev_pyr[0].shape[1], prev_pyr[0].shape[0]
    inside = (out[:, 0] >= 0) & (out[:, 0] < w0) & (out[:, 1] >= 0) & (out[:, 1] < h0)
    status &= inside
    # err: mean absolute window difference at the result, level 0
    nw = out - half
    inx = _floor_int(nw)
    wj = _weights(nw - inx.astype(F), F)
    Jw = _bilinear(next_pyr[0].astype(F), inx[:, 0:1] + wx[None, :], inx[:, 1:2] + wy[None, :], *wj)
    err = np.abs(Jw - tmpl0).sum(1, dtype=F) / F(win * win)
    err = np.where(status, err, F(0.0))
    return dict(xy=out, status=status, err=err, min_eig=min_eig0, its=its0)
