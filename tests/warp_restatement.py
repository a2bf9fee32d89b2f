"""Matcher::WarpMatrixAffine, GetSearchLevel and CreatePatch (matcher.cc:293-357) restated in float64 numpy from the reference's
text, not from oracle/ref_*.h: what tests/test_oracle_warp_independent.py holds the oracle against, and what
tests/test_gpu_search_warp.py asks which samples of a patch lie outside the reference image."""
import numpy as np

from oraclelib import WARP_CAM, quat_to_R


def unproject(px):                                   # camera.cc:74-79
    v = np.array([(px[0] - WARP_CAM[2]) / WARP_CAM[0], (px[1] - WARP_CAM[3]) / WARP_CAM[1], 1.0])
    return v / np.linalg.norm(v)


def project(p):                                      # camera.cc:69-72
    return np.array([WARP_CAM[2] + WARP_CAM[0] * p[0] / p[2], WARP_CAM[3] + WARP_CAM[1] * p[1] / p[2]])


def relative_pose(T_ref, T_cur):                     # matcher.cc:55: frame pose * reference pose^-1
    Rr, tr = quat_to_R(T_ref[:4]), T_ref[4:]
    Rc, tc = quat_to_R(T_cur[:4]), T_cur[4:]
    R = Rc @ Rr.T
    return R, tc - R @ tr


def warp_matrix(R, t, px, bearing, depth, level):    # matcher.cc:293-312
    half = 5
    p3d = bearing * depth
    du = unproject(px + np.array([half, 0.0]) * (1 << level))
    dv = unproject(px + np.array([0.0, half]) * (1 << level))
    du = du * (p3d[2] / du[2])
    dv = dv * (p3d[2] / dv[2])
    c, cu, cv = project(R @ p3d + t), project(R @ du + t), project(R @ dv + t)
    return np.stack([(cu - c) / half, (cv - c) / half], axis=1)      # columns


def search_level(A, max_fast_levels=3):              # matcher.cc:314-323
    det, lvl = np.linalg.det(A), 0
    while det > 3.0 and lvl < max_fast_levels - 1:
        lvl += 1
        det *= 0.25
    return lvl


def create_patch(Ainv, img, px, level, slevel):      # matcher.cc:325-357 with Interpolate8U, extra/utils.cc:44-59
    """-> (10x10 border patch, True where the sample lies outside the image)"""
    rows, cols = img.shape
    out, outside = np.zeros((10, 10), np.uint8), np.zeros((10, 10), bool)
    im = img.astype(np.float64)
    for y in range(10):
        for x in range(10):
            p = Ainv @ (np.array([x - 5.0, y - 5.0]) * (1 << slevel)) + px / (1 << level)
            if p[0] < 0 or p[1] < 0 or p[0] >= cols - 1 or p[1] >= rows - 1:
                outside[y, x] = True
                continue
            x0, y0 = int(np.floor(p[0])), int(np.floor(p[1]))
            ax, ay = p[0] - x0, p[1] - y0
            val = (1 - ax) * (1 - ay) * im[y0, x0] + (1 - ax) * ay * im[y0 + 1, x0] + ax * (1 - ay) * im[y0, x0 + 1] + ax * ay * im[y0 + 1, x0 + 1]
            out[y, x] = int(val)                      # (uint8_t) float: truncation
    return out, outside


def restate_border_case(orc, c):
    """the restatement's search level, patch and outside mask for each request of an oraclelib.warp_border_case"""
    pyr = orc.pyramid(c["img_ref"], 5)
    R, t = relative_pose(c["T_ref"], c["T_cur"])
    out = []
    for m in c["meta"]:
        A = warp_matrix(R, t, m["px"], m["bearing"], 1.0 / m["idepth"], m["level"])
        sl = search_level(A)
        patch, outside = create_patch(np.linalg.inv(A), pyr[m["level"]], m["px"], m["level"], sl)
        out.append(dict(slevel=sl, patch=patch, outside=outside))
    return out
