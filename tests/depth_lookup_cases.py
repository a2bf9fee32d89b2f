"""The images and positions tests/test_depth_lookup_restatement_cpu.py and tests/test_gpu_depth_lookup.py share.

Two 64 x 48 depth images of one scene, float metres and 16-bit at 1 / 5000 m: a gently slanted surface at 2 m with a hole (zeros; the
float image has a NaN in it as well), and a step to 3 m right of column 40.  The positions cover whole-numbered and .5 coordinates
(the centre rounds half up), levels 0 .. 2 (the window's stride), the border (a window partly off the image, a centre off it), the
hole and its rim (HOLE, FEW), the step (EDGE at the stride that reaches it, OK at the one that does not), a position that is not
finite, and positions in no job."""
import numpy as np

W, H = 64, 48
CAM = dict(width=float(W), height=float(H), fx=60.0, fy=60.0, u0=32.0, v0=24.0)
LENS = (-0.25, 0.08, 0.002, -0.003, 0.01)
U16_SCALE = 1.0 / 5000.0


def images():
    yy, xx = np.mgrid[0:H, 0:W]
    f = (2.0 + 0.0005 * xx + 0.0003 * yy).astype(np.float32)
    f[:, 41:] += 1.0
    f[20:26, 10:16] = 0.0
    f[22, 12] = np.nan
    u = np.nan_to_num(np.round(f.astype(np.float64) / U16_SCALE), nan=0.0).astype(np.uint16)
    f.setflags(write=False)
    u.setflags(write=False)
    return f, u


def positions():
    """-> px [n][2], levels [n]"""
    px, lv = [], []
    rng = np.random.default_rng(9)
    for level in (0, 1, 2):
        for x, y in ((30.0, 20.0), (30.5, 20.5), (30.49, 19.51), (7.5, 40.0),                     # plain surface, ties
                     (0.0, 0.0), (63.0, 47.0), (-0.5, 10.0), (-0.51, 10.0), (63.49, 47.49), (63.5, 20.0), (1.0, 1.0), (2.0, 45.5),   # border
                     (12.0, 22.0), (13.0, 23.0), (9.0, 22.0), (8.0, 19.0), (16.5, 26.0), (17.9, 27.9),   # hole, its rim
                     (40.0, 10.0), (39.0, 10.0), (38.0, 10.0), (36.0, 10.0), (41.0, 30.0), (42.5, 30.0), (45.0, 30.0)):   # the step
            px.append((x, y))
            lv.append(level)
        for _ in range(20):
            px.append((rng.uniform(-2, W + 2), rng.uniform(-2, H + 2)))
            lv.append(level)
    px += [(float("nan"), 5.0), (5.0, float("inf")), (1e300, -1e300)]
    lv += [0, 1, 2]
    return np.array(px, np.float64), np.array(lv, np.int32)
