"""Designed inputs for the kernels that decide which corners a keyframe keeps and what descriptor it carries (csrc/sdvl_orb.hip: Shi-Tomasi
score, ORB, the per-cell selection in its four forms, sdvl_filter_inputs) and for the ORB threshold of the patch search, shared by
tests/test_corner_cases_cpu.py (which asserts on the oracle alone that every case hits what it claims) and tests/test_gpu_corners.py
(device against oracle, bit for bit).  numpy and the oracle only; made once per process, read-only.

A corner is (x, y, level) in level coordinates.  The two limits the cases turn on:
  Shi-Tomasi (extra/utils.cc:61-97): the 8x8 box and its gradient ring must lie inside the image, 5 <= x <= W - 6 (same in y); score 0 outside
  ORB (orb_detector.cc:439-445, IsInsideLimits): 19 <= x < W - 19 (same in y); the device answers 32 zero bytes and angle -1 outside.  The
  oracle's orb_describe does not test it: `orb_want` calls it for inside points only.

Test infrastructure only."""
import numpy as np

LEVELS = 5
ORB_MARGIN = 19
# name -> rows, columns, seed of uniform noise.  P: level widths 131, 65, 32, 16, 8 (no multiple of 4 at levels 0 and 1, ORB's inside set is
# empty from level 2 on, Shi-Tomasi's at level 4); Q: level 3 is 40 x 41, where every ORB-inside point touches a limit; R: levels 3 and 4
NOISE = {"P": (99, 131, 101), "Q": (320, 328, 102), "R": (480, 640, 103)}

_made = {}


def made(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def noise(seed, h, w):
    return ro(np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8))


def noise_image(name):
    h, w, seed = NOISE[name]
    return made(("noise", name), lambda: noise(seed, h, w))


def level_shapes(h, w, levels=LEVELS):
    return [(h >> l, w >> l) for l in range(levels)]


def shi_inside(x, y, W, H):
    return not (x - 4 < 1 or x + 4 >= W - 1 or y - 4 < 1 or y + 4 >= H - 1)


def orb_inside(x, y, W, H):
    return ORB_MARGIN <= x < W - ORB_MARGIN and ORB_MARGIN <= y < H - ORB_MARGIN


def existing(vals, size):
    return sorted({int(v) for v in vals if 0 <= v < size})


def pyramid_of(orc, img, levels=LEVELS):
    return made(("pyr", id(img), levels), lambda: (img, [ro(p) for p in orc.pyramid(img, levels)]))[1]


# ------------------------------------------------------------------------------------------------ want
def shi_want(orc, pyr, xyl):
    return np.array([orc.shi_tomasi(pyr[l], x, y) for x, y, l in xyl], np.float64)


def orb_want(orc, pyr, xyl):
    """descriptors [n][32] and angles [n] as the device must return them: the oracle's inside the limits, zeros and -1 outside"""
    xyl = np.asarray(xyl, np.int32).reshape(-1, 3)
    desc, ang = np.zeros((len(xyl), 32), np.uint8), np.full(len(xyl), -1.0, np.float32)
    for l in range(len(pyr)):
        H, W = pyr[l].shape
        idx = [i for i, (x, y, ll) in enumerate(xyl) if ll == l and orb_inside(x, y, W, H)]
        if idx:
            desc[idx], ang[idx] = orc.orb_describe(pyr[l], xyl[idx, :2])
    return desc, ang


# ------------------------------------------------------------------------------------------------ 1. chosen points
def shi_points(name):
    """one list for all levels of a noise image: the points next to and on both sides of Shi-Tomasi's limit, and a few interior ones"""
    def make():
        h, w, seed = NOISE[name]
        rng = np.random.default_rng(seed + 1000)
        pts = []
        for l, (H, W) in enumerate(level_shapes(h, w)):
            xs, ys = existing((0, 4, 5, W - 6, W - 5, W - 1), W), existing((0, 4, 5, H - 6, H - 5, H - 1), H)
            pts += [(x, y, l) for y in ys for x in xs]
            if W >= 11 and H >= 11:
                pts += [(int(rng.integers(5, W - 5)), int(rng.integers(5, H - 5)), l) for _ in range(6)]
        return ro(np.array(pts, np.int32))
    return made(("shi_points", name), make)


def shi_wave_list():
    """65 level-0 points of P: the kernel scores four corners per wave, 16 lanes each.  Group g of four (g = 0 .. 15) holds an inside point
    at place k where bit k of g is set and an outside one elsewhere: all 16 patterns; one inside point more.  Prefixes of it are the lists
    of 1, 2, 3, 4, 5, 63, 64 and 65 corners."""
    def make():
        h, w, seed = NOISE["P"]
        rng = np.random.default_rng(seed + 2000)
        outside = [(x, y) for x in (0, 4, w - 5, w - 1) for y in (0, 4, 40, h - 5, h - 1)] + [(60, 4), (60, h - 5), (4, 50), (w - 5, 50)]
        pts = []
        for g in range(16):
            for k in range(4):
                if (g >> k) & 1:
                    pts.append((int(rng.integers(5, w - 5)), int(rng.integers(5, h - 5)), 0))
                else:
                    pts.append(outside[int(rng.integers(0, len(outside)))] + (0,))
        pts.append((int(rng.integers(5, w - 5)), int(rng.integers(5, h - 5)), 0))
        return ro(np.array(pts, np.int32))
    return made("shi_wave_list", make)


SHI_WAVE_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65)


def orb_points(name):
    """one list for all levels of a noise image: where a level has ORB-inside points, the points on both sides of every limit and a few
    interior ones; where it has none (its width or height is below 39), points that get zeros"""
    def make():
        h, w, seed = NOISE[name]
        rng = np.random.default_rng(seed + 3000)
        pts = []
        for l, (H, W) in enumerate(level_shapes(h, w)):
            if W >= 39 and H >= 39:
                xs, ys = existing((18, 19, W - 20, W - 19), W), existing((18, 19, H - 20, H - 19), H)
                pts += [(x, y, l) for y in ys for x in xs]
                pts += [(int(rng.integers(19, W - 19)), int(rng.integers(19, H - 19)), l) for _ in range(5)]
            else:
                pts += [(x, y, l) for x, y in {(0, 0), (W - 1, H - 1), (W // 2, H // 2), (min(19, W - 1), min(19, H - 1))}]
        return ro(np.array(sorted(pts, key=lambda p: p[2]), np.int32))
    return made(("orb_points", name), make)


# ramp -> the angle (degrees) ORB's intensity centroid has at a point whose disc lies inside the image; None: no gradient at all
RAMP_ANGLES = {"3x": 0.0, "240-3x": 180.0, "3y": 90.0, "240-3y": 270.0, "x+y": 45.0, "100+x-y": 315.0, "100-x+y": 135.0, "250-x-y": 225.0,
               "77": 0.0, "rings": None}
RAMP_AXIS = ("3x", "240-3x", "3y", "240-3y")
RAMP_DIAGONAL = ("x+y", "100+x-y", "100-x+y", "250-x-y")
RAMP_LEVELS = 3
RAMP_POINTS = ro(np.array([(30, 30, 0), (19, 19, 0), (60, 44, 0)], np.int32))      # the last two are the first and the last inside point


def ramp_images():
    """64 rows x 80 columns.  The centroid of a linear ramp points along its gradient: the quadrant boundaries (m01 == 0 or m10 == 0), the
    |m10| == |m01| tie of cv::fastAtan2's `ax >= ay` branch, a flat patch (m10 == m01 == 0: angle 0, every test 'p < p' false)"""
    def make():
        yy, xx = np.mgrid[0:64, 0:80]
        f = {"3x": 3 * xx, "240-3x": 240 - 3 * xx, "3y": 3 * yy, "240-3y": 240 - 3 * yy, "x+y": xx + yy, "100+x-y": 100 + xx - yy,
             "100-x+y": 100 - xx + yy, "250-x-y": 250 - xx - yy, "77": 77 + 0 * xx, "rings": ((xx - 30) ** 2 + (yy - 30) ** 2) % 256}
        for v in f.values():
            assert v.min() >= 0 and v.max() <= 255
        return {k: ro(v.astype(np.uint8)) for k, v in f.items()}
    return made("ramps", make)


# ------------------------------------------------------------------------------------------------ 2. batches
BATCH_SIZES = (1, 7, 8, 9, 17)
BATCH_LENGTHS = (0, 1, 4, 5, 37, 64, 0, 200)


def batch_frame(k):
    """frame k of a batch: (image, corners).  P's size for even k, 120 x 160 for odd k; BATCH_LENGTHS[k % 8] points anywhere on levels 0 to 2,
    the borders included"""
    def make():
        h, w = (NOISE["P"][0], NOISE["P"][1]) if k % 2 == 0 else (120, 160)
        rng = np.random.default_rng(7000 + k)
        img = noise(7100 + k, h, w)
        pts = []
        for _ in range(BATCH_LENGTHS[k % 8]):
            l = int(rng.integers(0, 3))
            pts.append((int(rng.integers(0, w >> l)), int(rng.integers(0, h >> l)), l))
        return img, ro(np.array(pts, np.int32).reshape(-1, 3))
    return made(("batch_frame", k), make)


# ------------------------------------------------------------------------------------------------ 3. selection
BIN_CELLS_SMALL, BIN_CORNERS_SMALL, BIN_CELLS, UNBINNED_CELLS = 512, 2048, 2048, 4096       # csrc/sdvl_orb.hip: the dispatch of filter_select


def select_form(n_cells, ccap):
    """the dispatch's condition (sdvl_filter_corners_begin), restated; ccap = the longest corner list of the call, at least 1"""
    if n_cells <= BIN_CELLS_SMALL and ccap <= BIN_CORNERS_SMALL:
        return "small"
    if n_cells <= BIN_CELLS:
        return "large"
    return "unbinned" if n_cells <= UNBINNED_CELLS else "four-slot"


def eligible_points(h, w, cell, margin=ORB_MARGIN, levels=3):
    """every (x, y, level, cell) FilterCorners would take into a cell (fast_detector.cc:185-192), sorted by cell"""
    gw = -(-w // cell)
    out = []
    for l in range(levels):
        H, W = h >> l, w >> l
        if W - margin <= margin or H - margin <= margin:
            continue
        yy, xx = np.mgrid[margin:H - margin, margin:W - margin]
        c = ((yy << l) // cell) * gw + (xx << l) // cell
        out.append(np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, l), c.ravel()], 1))
    a = np.concatenate(out).astype(np.int32)
    return a[np.argsort(a[:, 3], kind="stable")]


def cell_of(xyl, cell, gw):
    xyl = np.asarray(xyl).reshape(-1, 3)
    return ((xyl[:, 1] << xyl[:, 2]) // cell) * gw + (xyl[:, 0] << xyl[:, 2]) // cell


def is_eligible(xyl, h, w, margin=ORB_MARGIN):
    x, y, l = np.asarray(xyl).reshape(-1, 3).T
    return (x >= margin) & (y >= margin) & (x < (w >> l) - margin) & (y < (h >> l) - margin)


# form -> width, height, cell size, corners strewn over the other cells, eligible corners of the counted cells, length the list is padded to
# with corners inside the margin.  The counted cells sit on both sides of the bins' capacity (10 slots, 4 in the four-slot form) and far
# beyond it: a fuller cell is scanned from the whole list.
FORMS = {
    "small": (128, 96, 32, 100, (9, 10, 11, 25), 0),
    "large": (160, 120, 32, 120, (9, 10, 11, 25), 2100),
    "unbinned": (416, 320, 8, 1500, (9, 10, 11, 25), 0),
    "four-slot": (640, 480, 8, 3000, (3, 4, 5, 12), 0),
}


def selection_case(orc, form):
    """dict(img, corners, cell, form, counted {cell: k}, ties {cell: (indices of the one point's occurrences)}).  In a counted cell the
    corners stand in ascending score, so the winner is the last of them; a tie cell lists its best point twice (a b a) or three times
    (a b a c a), b and c scoring lower: the reference's `score > truncated best` takes the last occurrence."""
    def make():
        w, h, cell, n_strewn, counts, pad_to = FORMS[form]
        seed = 9000 + sorted(FORMS).index(form)
        rng = np.random.default_rng(seed)
        img = noise(seed + 50, h, w)
        pyr = pyramid_of(orc, img)
        gw = -(-w // cell)
        el = eligible_points(h, w, cell)
        cells, first, sizes = np.unique(el[:, 3], return_index=True, return_counts=True)
        need = list(counts) + [3, 3]
        roomy = cells[sizes >= max(need)]
        chosen = [int(c) for c in rng.choice(roomy, len(need), replace=False)]
        corners, groups = [], []
        for c, k in zip(chosen, need):
            lo = first[np.searchsorted(cells, c)]
            pts = el[lo:lo + sizes[np.searchsorted(cells, c)], :3]
            pts = pts[rng.choice(len(pts), k, replace=False)]
            sc = shi_want(orc, pyr, pts)
            pts = pts[np.argsort(sc)]                        # ascending: the last one wins
            if c == chosen[-2]:
                pts = pts[[2, 1, 2]]                         # a b a
            elif c == chosen[-1]:
                pts = pts[[2, 1, 2, 0, 2]]                   # a b a c a
            groups.append(list(range(len(corners), len(corners) + len(pts))))
            corners += [tuple(p) for p in pts]
        free = el[~np.isin(el[:, 3], chosen)]
        coarse = free[free[:, 2] > 0]
        strewn = [free[rng.choice(len(free), n_strewn // 2)]]
        if len(coarse):
            strewn.append(coarse[rng.choice(len(coarse), n_strewn - n_strewn // 2)])     # half of them from levels 1 and 2
        corners += [tuple(p[:3]) for p in np.concatenate(strewn)]
        while len(corners) < pad_to:                         # inside the margin: listed, never taken into a cell
            corners.append((int(rng.integers(0, ORB_MARGIN)), int(rng.integers(0, h)), 0))
        keys = rng.random(len(corners))
        for g in groups:
            keys[g] = np.sort(keys[g])                       # a group keeps its order, wherever its corners land in the list
        order = np.argsort(keys)
        place = np.argsort(order)                            # corner i of the build stands at place[i]
        corners = np.array(corners, np.int32)[order]
        ties = {chosen[-2]: tuple(int(place[i]) for i in np.array(groups[-2])[[0, 2]]),
                chosen[-1]: tuple(int(place[i]) for i in np.array(groups[-1])[[0, 2, 4]])}
        return dict(img=img, corners=ro(corners), cell=cell, form=form, gw=gw, n_cells=gw * -(-h // cell),
                    counted=dict(zip(chosen[:len(counts)], counts)), ties=ties)
    return made(("selection", form), make)


def oracle_filter(orc, img, corners, locked=None, cell=32, min_score=50, use_orb=1):
    """orc.filter_corners with the grid, threshold and margin (19 with ORB, 5 without) of this call alone"""
    old = orc.params.cell_size, orc.params.min_feature_score, orc.params.use_orb
    orc.params.cell_size, orc.params.min_feature_score, orc.params.use_orb = cell, min_score, use_orb
    try:
        return orc.filter_corners(img, corners, locked if locked is not None and len(locked) else None)
    finally:
        orc.params.cell_size, orc.params.min_feature_score, orc.params.use_orb = old


THRESHOLD_CELL = 4


def threshold_case(orc):
    """128 + integer noise in [-A, A] on 96 x 128, every third eligible level-0 point listed, cells of 4 px: Shi-Tomasi scores around
    min_feature_score = 50.  A is the first of 12, 13, 14 at which the oracle keeps at least a quarter of the eligible cells, drops at
    least a quarter, and at least 5 listed corners score in (50, 51): such a score passes `score > best` and is dropped by `best > 50`."""
    def make():
        h, w = 96, 128
        ys, xs = np.mgrid[ORB_MARGIN:h - ORB_MARGIN:3, ORB_MARGIN:w - ORB_MARGIN:3]
        corners = ro(np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size, np.int64)], 1).astype(np.int32))
        gw = -(-w // THRESHOLD_CELL)
        n_cells = len(set(cell_of(corners, THRESHOLD_CELL, gw).tolist()))
        for A in (12, 13, 14):
            img = ro((128 + np.random.default_rng(4000 + A).integers(-A, A + 1, (h, w))).astype(np.uint8))
            scores = shi_want(orc, pyramid_of(orc, img), corners)
            kept = oracle_filter(orc, img, corners, cell=THRESHOLD_CELL)
            near = int(((scores > 50) & (scores < 51)).sum())
            if 4 * len(kept) >= n_cells and 4 * (n_cells - len(kept)) >= n_cells and near >= 5:
                return dict(img=img, corners=corners, cell=THRESHOLD_CELL, A=A, scores=ro(scores), n_cells=n_cells, near=near,
                            above=int(scores.max()) + 1)
        raise AssertionError("no amplitude puts the scores around the threshold")
    return made("threshold", make)


MARGIN_W, MARGIN_H, MARGIN_CELL = 216, 188, 32      # 7 x 6 cells; at margin 5 corners of levels 1 and 2 reach the last row and column


def margin_case(orc):
    """corners on both sides of the margin (19) on levels 0 to 2 and corners anywhere, the margin zone included.  `locked`: positions of
    corners the oracle keeps without locks, in cells that corners of levels 0, 1 and 2 fall into: locking them changes the result.  The same list is also filtered
    at margin 5 (the reference's margin without ORB): corners of levels 1 and 2 then fall into the last row and column of cells, and
    kept corners lie outside ORB's limits (zero descriptors)."""
    def make():
        w, h, cell = MARGIN_W, MARGIN_H, MARGIN_CELL
        rng = np.random.default_rng(9100)
        img = noise(9101, h, w)
        pts = []
        for l in range(3):
            W, H = w >> l, h >> l
            pts += [(x, y, l) for y in (18, 19, H - 20, H - 19) for x in (18, 19, W - 20, W - 19)]
            pts += [(int(rng.integers(0, W)), int(rng.integers(0, H)), l) for _ in range((150, 100, 80)[l])]
            pts += [(W - 6 - k % 2, int(rng.integers(5, H - 5)), l) for k in range(6)]      # last column at margin 5
            pts += [(int(rng.integers(5, W - 5)), H - 6 - k % 2, l) for k in range(6)]      # last row at margin 5
        corners = np.array(pts, np.int32)[rng.permutation(len(pts))]
        out = dict(img=img, corners=ro(corners), cell=cell, gw=-(-w // cell), gh=-(-h // cell))
        for use_orb, margin in ((1, 19), (0, 5)):
            first = oracle_filter(orc, img, corners, cell=cell, use_orb=use_orb)
            elig = is_eligible(corners, h, w, margin)
            cells = cell_of(corners, cell, out["gw"])
            locked = []
            for l in range(3):      # kept corners (on noise the level-0 corner of a cell wins) whose cell also holds eligible corners of level l
                shared = [i for i in first if (elig & (corners[:, 2] == l) & (cells == cells[i])).any()]
                for i in shared[::max(1, len(shared) // 3)][:3]:
                    s = 1 << corners[i, 2]
                    locked.append([float(corners[i, 0] * s) + 0.5, float(corners[i, 1] * s) + 0.25])
            out[margin] = dict(first=ro(first), locked=ro(np.array(locked, np.float64)))
        return out
    return made("margin", make)


def selection_batch():
    """9 frames of 128 x 96, each with a list and locked positions of its own; frame 4 has no corners, frame 6 no locks"""
    def make():
        w, h = 128, 96
        frames = []
        for k in range(9):
            rng = np.random.default_rng(9200 + k)
            n = 0 if k == 4 else 40 + 30 * k
            pts = []
            for _ in range(n):
                l = int(rng.integers(0, 2))
                pts.append((int(rng.integers(10, (w >> l) - 10)), int(rng.integers(10, (h >> l) - 10)), l))
            locked = np.stack([rng.uniform(0, w, k % 3 + 1), rng.uniform(0, h, k % 3 + 1)], 1) if k != 6 else np.zeros((0, 2))
            frames.append((noise(9300 + k, h, w), ro(np.array(pts, np.int32).reshape(-1, 3)), ro(locked)))
        return frames
    return made("selection_batch", make)


# sdvl_detect_corners' num_features on white noise: more corners than the 1280 the launches are cut for, on level 0 alone, whose corners
# win their cells: some of the kept corners stand beyond the bound
DEVICE_COUNT_FEATURES = 4000


def device_count_image():
    return made("device_count", lambda: noise(9400, 480, 640))


# ------------------------------------------------------------------------------------------------ 4. sdvl_filter_inputs
def inputs_frames(n):
    """n frames of 128 x 96 with ragged corner lists (frame 2 of a batch has none) on levels 0 to 2, ORB's and Shi-Tomasi's borders included"""
    def make():
        w, h = 128, 96
        frames = []
        for k in range(n):
            rng = np.random.default_rng(9500 + k)
            cnt = (23, 64, 0, 1, 150, 65, 7, 128, 90)[k % 9]
            pts = []
            for _ in range(cnt):
                l = int(rng.integers(0, 3))
                pts.append((int(rng.integers(0, w >> l)), int(rng.integers(0, h >> l)), l))
            frames.append((noise(9600 + k, h, w), ro(np.array(pts, np.int32).reshape(-1, 3))))
        return frames
    return made(("inputs", n), make)


# ------------------------------------------------------------------------------------------------ 5. the search's threshold
def flip_bits(desc, bits):
    d = np.array(desc, np.uint8)
    for b in bits:
        d[(b % 256) >> 3] ^= np.uint8(1 << (b & 7))
    return d


def search_bit_case(orc, synth, n_base=4):
    """The first n_base requests of search_request_meta(frames 0 and 4, 160 requests, seed 11, fixed) that the oracle matches.  j = the
    corner it matched, D = the oracle's descriptor of corner j.  Per request and bit i of 256 two requests that differ from it in the
    descriptor alone: A_i = D with bits i+1 .. i+99 (mod 256) flipped (distance 99 to corner j: a match), B_i with bit i flipped too
    (distance 100: the threshold's `>=`, no match).  meta = [base][bit][A, B] flattened; `base` the unchanged requests and answers."""
    def make():
        from oraclelib import TUM_CAM, search_request_meta, trajectory_pose
        T_ref, T_cur = trajectory_pose(orc, 0), trajectory_pose(orc, 4)
        img_ref, img_cur = (ro(synth.render(T, TUM_CAM, 640, 480, seed=20260001, frame_id=k)) for T, k in ((T_ref, 0), (T_cur, 4)))
        meta, ccur = search_request_meta(orc, img_ref, img_cur, T_ref, T_cur, TUM_CAM, 160, 11, True)
        case = dict(img_ref=img_ref, img_cur=img_cur, T_ref=T_ref, T_cur=T_cur, ccur=ro(ccur), cam=TUM_CAM)
        pyr = pyramid_of(orc, img_cur)
        base, out = [], []
        for m in meta:
            want = search_want(orc, case, m)
            if want["stage"] < 2:
                continue
            x, y, l = ccur[want["best_corner"]]
            D = orc.orb_describe(pyr[l], [[x, y]])[0][0]
            base.append(dict(meta=m, want=want, D=ro(D)))
            for i in range(256):
                a = flip_bits(D, range(i + 1, i + 100))
                out.append(dict(m, desc=ro(a)))
                out.append(dict(m, desc=ro(flip_bits(a, [i]))))
            if len(base) == n_base:
                break
        assert len(base) == n_base
        case.update(base=base, meta=out)
        return case
    return made(("search_bits", n_base), make)


def search_want(orc, case, m):
    return orc.search_point(case["img_ref"], case["img_cur"], case["cam"], case["T_ref"], case["T_cur"], m["px"], m["bearing"], m["level"],
                            m["desc"], m["idepth"], m["istd"], True, case["ccur"], m["px0"])


def search_bit_wants(orc, case):
    """the oracle's answer to every request of the case, computed once"""
    return made(("search_bit_wants", id(case)), lambda: (case, [search_want(orc, case, m) for m in case["meta"]]))[1]
