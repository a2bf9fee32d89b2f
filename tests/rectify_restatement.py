"""Stereo rectification as this project states it, in plain numpy: the specification of sdvl_stereo_rectify_plan (csrc/rectify_plan.cc),
of the map kernel rectify_map (csrc/sdvl_undistort.hip) and of the remap behind both maps.  include/sdvl_hip.h carries the rule in words.

  plan(...)            the rotations R1, R2 (Bouguet's construction), the one rectified pinhole camera, the baseline
  map_fixed(...)       the fixed-point source position (iu, iv) = cvRound(32 u), cvRound(32 v) of every rectified pixel
  undistort_fixed(...) the same for Camera::UndistortImage's map in cv::undistort's evaluation order (what sdvl_undistort builds)
  words(...)           the packed words of a map, narrow or wide
  no_source(...)       how many pixels have one of their four taps outside the raw image
  remap(...)           cv::remap's bilinear fixed-point arithmetic, a tap outside the image reads 0

Every FP64 expression is written in the order the C++ and the kernel evaluate it (numpy does not contract a * b + c), so the plan agrees
to the last bits up to libm's sin / cos / atan2 / acos, and the map word for word.

Test infrastructure only."""
import math

import numpy as np

PLAN_NULL, PLAN_SIZE, PLAN_T, PLAN_R, PLAN_VERTICAL, PLAN_ORDER, PLAN_EMPTY, PLAN_INTRINSICS = 1, 2, 3, 4, 5, 6, 7, 8
MAP_MAX = 2044        # a side above it: the wide map


class Refused(Exception):
    def __init__(self, code):
        Exception.__init__(self, "plan refused with code %d" % code)
        self.code = code


# ---- 3 x 3 matrices as nested lists of python floats: every product written out, left to right
def mul3(a, b):
    return [[a[r][0] * b[0][k] + a[r][1] * b[1][k] + a[r][2] * b[2][k] for k in range(3)] for r in range(3)]


def transpose3(a):
    return [[a[k][r] for k in range(3)] for r in range(3)]


def apply3(a, v):
    return [a[r][0] * v[0] + a[r][1] * v[1] + a[r][2] * v[2] for r in range(3)]


def norm3(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def identity3():
    return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def rotation_of(w):
    """exp of a rotation vector: I + sin(th) K + (1 - cos(th)) K K"""
    th = norm3(w)
    if th < 1e-15:
        return identity3()
    k = [w[0] / th, w[1] / th, w[2] / th]
    K = [[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]]
    KK = mul3(K, K)
    s, c = math.sin(th), 1 - math.cos(th)
    eye = identity3()
    return [[eye[r][q] + s * K[r][q] + c * KK[r][q] for q in range(3)] for r in range(3)]


def rotation_vector_of(R):
    """for turns below 90 degrees: the axis from the skew part, the angle from atan2(|skew part|, (trace - 1) / 2)"""
    v = [0.5 * (R[2][1] - R[1][2]), 0.5 * (R[0][2] - R[2][0]), 0.5 * (R[1][0] - R[0][1])]
    s, c = norm3(v), 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)
    if s < 1e-15:
        return [0.0, 0.0, 0.0]
    th = math.atan2(s, c)
    return [v[i] / s * th for i in range(3)]


def as_lists(R):
    return [[float(R[r][k]) for k in range(3)] for r in range(3)]


# ---- the lens
def distort(x, y, D):
    """the forward radial-tangential model on normalised coordinates, in sdvl_undistort's expression order"""
    k1, k2, p1, p2, k3 = [float(d) for d in D]
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    return x * kr + p1 * _2xy + p2 * (r2 + 2 * x2), y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy


def undistort_points(K, D, u, v, iterations=50):
    """the rays of raw pixels without the lens: fixed-point iteration of the model"""
    fx, fy, u0, v0 = [float(c) for c in K]
    k1, k2, p1, p2, k3 = [float(d) for d in D]
    xd, yd = (u - u0) / fx, (v - v0) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2 * x * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        dx, dy = p1 * _2xy + p2 * (r2 + 2 * x2), p1 * (r2 + 2 * y2) + p2 * _2xy
        x, y = (xd - dx) / kr, (yd - dy) / kr
    return x, y


def inner_rectangle(K, D, R, w, h):
    """[max x of the left border, min x of the right] x [max y of the top, min y of the bottom] in the rectified frame -> x0, x1, y0, y1"""
    cols, rows = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)

    def rays(u, v):
        x, y = undistort_points(K, D, u, v)
        qx = R[0][0] * x + R[0][1] * y + R[0][2] * 1.0
        qy = R[1][0] * x + R[1][1] * y + R[1][2] * 1.0
        qz = R[2][0] * x + R[2][1] * y + R[2][2] * 1.0
        if not (np.all(np.isfinite(qx / qz)) and np.all(np.isfinite(qy / qz)) and np.all(qz > 0)):
            raise Refused(PLAN_EMPTY)
        return qx / qz, qy / qz

    y0 = rays(cols, 0 * cols)[1].max()
    y1 = rays(cols, 0 * cols + (h - 1))[1].min()
    x0 = rays(0 * rows, rows)[0].max()
    x1 = rays(0 * rows + (w - 1), rows)[0].min()
    return x0, x1, y0, y1


def plan(K1, D1, K2, D2, R, T, w, h, override=None):
    """-> dict(R1, R2 [3][3] arrays, rect = (fx, fy, u0, v0), baseline); raises Refused(code)"""
    def positive(v):
        return math.isfinite(v) and v > 0
    if w < 2 or h < 2 or w > 4095 or h > 4095:
        raise Refused(PLAN_SIZE)
    if not all(positive(float(K[i])) for K in (K1, K2) for i in (0, 1)):
        raise Refused(PLAN_INTRINSICS)
    if override is not None and not (positive(float(override[0])) and positive(float(override[1])) and math.isfinite(override[2])
                                     and math.isfinite(override[3])):
        raise Refused(PLAN_INTRINSICS)
    T = [float(t) for t in T]
    if not all(math.isfinite(t) for t in T) or norm3(T) == 0:
        raise Refused(PLAN_T)
    R = as_lists(R)
    RtR = mul3(transpose3(R), R)
    for r in range(3):
        for k in range(3):
            if not abs(RtR[r][k] - (1.0 if r == k else 0.0)) <= 1e-9:
                raise Refused(PLAN_R)
    if not R[0][0] + R[1][1] + R[2][2] - 1 > 0:
        raise Refused(PLAN_R)
    om = rotation_vector_of(R)
    rr = rotation_of([-0.5 * om[0], -0.5 * om[1], -0.5 * om[2]])
    t = apply3(rr, T)
    if abs(t[1]) > abs(t[0]):
        raise Refused(PLAN_VERTICAL)
    if t[0] > 0:
        raise Refused(PLAN_ORDER)
    u = [-1.0, 0.0, 0.0]
    ww = [t[1] * u[2] - t[2] * u[1], t[2] * u[0] - t[0] * u[2], t[0] * u[1] - t[1] * u[0]]
    nw = norm3(ww)
    if nw > 0:
        tu = t[0] * u[0] + t[1] * u[1] + t[2] * u[2]
        angle = math.acos(min(abs(tu) / norm3(t), 1.0))
        ww = [c * (angle / nw) for c in ww]
    wR = rotation_of(ww)
    R1, R2 = mul3(wR, transpose3(rr)), mul3(wR, rr)
    if override is not None:
        rect = tuple(float(c) for c in override)
    else:
        a, b = inner_rectangle(K1, D1, R1, w, h), inner_rectangle(K2, D2, R2, w, h)
        x0, x1, y0, y1 = max(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), min(a[3], b[3])
        if not x1 > x0 or not y1 > y0:
            raise Refused(PLAN_EMPTY)
        f = max((w - 1 + 4) / (x1 - x0), (h - 1 + 4) / (y1 - y0))
        rect = (f, f, (w - 1) / 2.0 - f * ((x0 + x1) / 2), (h - 1) / 2.0 - f * ((y0 + y1) / 2))
    return dict(R1=np.array(R1), R2=np.array(R2), rect=tuple(float(c) for c in rect), baseline=norm3(T))


# ---- the maps
def rays_matrix(Ri, rect):
    """M = R_i^T K_rect^-1, every entry as the host code writes it"""
    fx, fy, u0, v0 = [float(c) for c in rect]
    Ri = as_lists(Ri)
    ifx, ify = 1.0 / fx, 1.0 / fy
    cx, cy = -u0 * ifx, -v0 * ify
    M = []
    for k in range(3):
        a, b, c = Ri[0][k], Ri[1][k], Ri[2][k]
        M.append([a * ifx, b * ify, a * cx + b * cy + c])
    return M


def fixed_of(K, D, x, y):
    """normalised rays -> (iu, iv) = cvRound(32 u), cvRound(32 v), saturated to int32 like the device's conversion"""
    fx, fy, u0, v0 = [float(c) for c in K]
    xd, yd = distort(x, y, D)
    u, v = fx * xd + u0, fy * yd + v0
    lim = float(2 ** 31 - 1)
    with np.errstate(invalid="ignore"):
        iu = np.clip(np.rint(u * 32), -lim - 1, lim)
        iv = np.clip(np.rint(v * 32), -lim - 1, lim)
    return np.nan_to_num(iu).astype(np.int64).astype(np.int32), np.nan_to_num(iv).astype(np.int64).astype(np.int32)


def map_fixed(K, D, Ri, rect, w, h):
    """the rectified camera's map: pixel (j, i) -> the ray M (j, i, 1), evaluated directly, x / w, y / w, the lens, K"""
    M = rays_matrix(Ri, rect)
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x = M[0][0] * j + M[0][1] * i + M[0][2]
    y = M[1][0] * j + M[1][1] * i + M[1][2]
    ww = M[2][0] * j + M[2][1] * i + M[2][2]
    with np.errstate(divide="ignore", invalid="ignore"):
        iu, iv = fixed_of(K, D, x / ww, y / ww)
    behind = ~(ww > 0)                 # a ray that does not point forward in the raw camera's frame has no source: sx = sy = -2, a = b = 0
    iu[behind] = iv[behind] = -64
    return iu, iv


def undistort_fixed(K, D, w, h):
    """Camera::UndistortImage's map as cv::undistort builds it (stripes of 4096 / cols rows, the row's x accumulated column by column):
    what sdvl_undistort builds, restated from csrc/sdvl_undistort.hip's tables"""
    fx, fy, u0, v0 = [float(c) for c in K]
    xw, yw = np.zeros(w), np.zeros(h)
    stripe0 = min(max(1, (1 << 12) // max(w, 1)), h)
    for y0 in range(0, h, stripe0):
        # the inverse of [[fx, 0, u0], [0, fy, v0 - y0], [0, 0, 1]] in cv::invert's closed form
        c12 = v0 - y0
        d = 1.0 / (fx * (fy * 1.0 - c12 * 0.0) - 0.0 * (0.0 * 1.0 - c12 * 0.0) + u0 * (0.0 * 0.0 - fy * 0.0))
        ir = [(fy * 1.0 - c12 * 0.0) * d, (u0 * 0.0 - 0.0 * 1.0) * d, (0.0 * c12 - u0 * fy) * d,
              (c12 * 0.0 - 0.0 * 1.0) * d, (fx * 1.0 - u0 * 0.0) * d, (u0 * 0.0 - fx * c12) * d,
              (0.0 * 0.0 - fy * 0.0) * d, (0.0 * 0.0 - fx * 0.0) * d, (fx * fy - 0.0 * 0.0) * d]
        for i in range(min(stripe0, h - y0)):
            _x, _y, _w = i * ir[1] + ir[2], i * ir[4] + ir[5], i * ir[7] + ir[8]
            yw[y0 + i] = _y * (1. / _w)
            if y0 == 0 and i == 0:
                for j in range(w):
                    xw[j] = _x * (1. / _w)
                    _x += ir[0]
                    _w += ir[6]
    x, y = np.meshgrid(xw, yw)
    return fixed_of(K, D, x, y)


def positions(iu, iv):
    """integer source positions (the library's cast to short) and 5-bit fractions"""
    sx = (iu >> 5).astype(np.int16).astype(np.int32)
    sy = (iv >> 5).astype(np.int16).astype(np.int32)
    return sx, sy, (iu & 31).astype(np.uint32), (iv & 31).astype(np.uint32)


def words(iu, iv, w, h):
    """the packed words: uint32 [h][w], or [h][w][2] where a side exceeds MAP_MAX"""
    sx, sy, a, b = positions(iu, iv)
    sxc = (np.clip(sx, -2, w) + 2).astype(np.uint32)
    syc = (np.clip(sy, -2, h) + 2).astype(np.uint32)
    if w > MAP_MAX or h > MAP_MAX:
        return np.stack([a | b << np.uint32(5), sxc | syc << np.uint32(16)], axis=-1)
    return a | b << np.uint32(5) | sxc << np.uint32(10) | syc << np.uint32(21)


def no_source(iu, iv, w, h):
    """pixels with one of their four taps outside the raw image"""
    sx, sy, _, _ = positions(iu, iv)
    return int(np.count_nonzero((sx < 0) | (sy < 0) | (sx + 1 >= w) | (sy + 1 >= h)))


def remap(img, iu, iv):
    """(S0 (32-b)(32-a) + S1 (32-b) a + S2 b (32-a) + S3 b a + 512) >> 10, a tap outside the image reads 0: cv::remap's bilinear
    fixed-point result (csrc/sdvl_undistort.hip shows the equality with the library's 15-bit table)"""
    h, w = img.shape
    sx, sy, a, b = positions(iu, iv)
    a, b = a.astype(np.int64), b.astype(np.int64)
    src = img.astype(np.int64)
    acc = np.full(sx.shape, 512, np.int64)
    for dy, dx, wt in ((0, 0, (32 - b) * (32 - a)), (0, 1, (32 - b) * a), (1, 0, b * (32 - a)), (1, 1, b * a)):
        x, y = sx + dx, sy + dy
        inside = (x >= 0) & (y >= 0) & (x < w) & (y < h)
        acc += np.where(inside, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0) * wt
    return (acc >> 10).astype(np.uint8)


def rectify(img, K, D, Ri, rect, w=None, h=None):
    """one raw image through the rectified camera's map"""
    hh, ww = img.shape
    iu, iv = map_fixed(K, D, Ri, rect, w or ww, h or hh)
    return remap(img, iu, iv)
