"""The cases of tests/test_gpu_track_tables.py, shared with tests/test_track_restatement_cpu.py, which asserts without a GPU that each is
what it claims to be.

One scene for everything, made once per process: two views (k = 0 and k = 4 of the usual trajectory) of the plane z = 2 through a camera
with fx = fy = 512, u0 = 320, v0 = 240 at 640x480, 5 levels, cell 32 (300 cells).  The reference frame (k = 0, identity pose) gives the
points: one per corner, on the plane, with its descriptor, as oraclelib.search_request_meta seeds them; the last frame's features are
those corners.  Every case tracks from the reference frame
    "same"   into the reference image again (T0 = last_pose = identity: hand-placed points project exactly, in binary), or
    "moved"  into the k = 4 image with T0 = the k = 4 pose,
with an alignment of max_its = 0, so that T comes back as T0 and the pose every projection is made with is known beforehand.  A case is
rows for the two tables, a cell order, max_matches and a seed of the rand() stream; point rows reuse the scene's records and only
change score, n_failed, status and last_frame (several rows may share a record: two points at one place land in one cell).  A record
with its descriptor's bits turned over is one the search cannot find.  The oracle's SearchPoint answer per (view, record) is cached."""
from collections import Counter

import numpy as np

import track_restatement as tr
from oraclelib import trajectory_pose
from track_restatement import DELETED, DUPLICATE, P_FOUND, TRASH

W, H, LEVELS, CELL, PATCH, MAX_FAILED = 640, 480, 5, 32, 8, 15
CAM4 = np.array([512.0, 512.0, 320.0, 240.0])
CAM = dict(width=float(W), height=float(H), fx=512.0, fy=512.0, u0=320.0, v0=240.0)
ID = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
N_CELLS = 300
MAX_MATCHES = 320          # of the sets; a case asks for this many unless it is about the cap
MAX_RANSAC_ITS = 100
FRAME_ID = 41

# what the restatement's trace must have met at least once over all cases
BRANCHES = ("behind-camera", "outside-margin", "seen", "deleted-point", "trash-seen", "trash-unseen", "last-frame-is-this-frame",
            "feature-without-point", "duplicate-feature", "equal-scores-in-a-cell", "hit", "miss", "hit-behind-a-miss", "cell-of-misses",
            "miss-at-max-failed", "deleted-beyond-max-failed", "cap-reached", "cap-reached-before-the-last-cell", "outlier",
            "every-match-an-outlier", "no-depth", "median-of-even", "median-of-odd", "trash-becomes-deleted")

_made = {}


def scene(orc, synth):
    if "scene" in _made:
        return _made["scene"]
    T4 = tuple(float(v) for v in trajectory_pose(orc, 4))
    assert tuple(float(v) for v in trajectory_pose(orc, 0)) == ID
    img = {"same": synth.render(np.array(ID), CAM4, W, H, frame_id=0), "moved": synth.render(np.array(T4), CAM4, W, H, frame_id=4)}
    corners = {v: orc.detect_pyramid(img[v]) for v in img}
    pyr = orc.pyramid(img["same"], LEVELS)
    start = {"same": tr.se3_mul(ID, ID), "moved": tr.se3_mul(T4, ID)}
    assert start["same"] == ID
    records = []
    c0 = corners["same"]
    desc = np.zeros((len(c0), 32), np.uint8)
    for l in range(3):
        idx = np.flatnonzero(c0[:, 2] == l)
        if len(idx):
            desc[idx], _ = orc.orb_describe(pyr[l], c0[idx, :2])
    for i, (x, y, l) in enumerate(c0.tolist()):
        px = (float(x << l), float(y << l))
        b = tr.unproject(CAM, px)
        s = 2.0 / b[2]                          # on the plane z = 2; the reference pose is the identity
        records.append(dict(key=("corner", i), P=(b[0] * s, b[1] * s, b[2] * s), px=px, bearing=b, level=l, desc=desc[i].copy(), idepth=1.0 / s,
                            istd=0.05 / s, fixed=1))
    sc = dict(orc=orc, img=img, corners=corners, T0={"same": ID, "moved": T4}, start=start, records=records, answers={})
    # the records a case may give a point to: in both views well inside the margin and away from every cell edge, so that no rounding
    # of the projection decides where they go (the hand-placed points are the ones ON the thresholds, exactly)
    sc["usable"] = [i for i, r in enumerate(records) if all(_clear(sc, v, r) for v in ("same", "moved"))]
    _made["scene"] = sc
    return sc


def _px0(sc, view, rec):
    return tr.project(CAM, tr.relative_pos(sc["start"][view], rec["P"]))


def _clear(sc, view, rec):
    x, y = _px0(sc, view, rec)
    away = all(abs(v - CELL * round(v / CELL)) > 1e-3 for v in (x, y))      # a thousandth of a pixel from the nearest cell edge
    return away and PATCH + 1 <= x < W - PATCH - 1 and PATCH + 1 <= y < H - PATCH - 1


def flipped(rec):
    """the same record with every bit of its descriptor turned over: nothing in any frame matches it"""
    return dict(rec, key=("flipped",) + rec["key"], desc=rec["desc"] ^ 0xFF)


def hand(name, u, v, z=2.0):
    """a hand-placed record that projects exactly onto pixel (u, v) from the identity pose; first seen there in the reference frame"""
    P = ((u - 320.0) / 512.0 * z, (v - 240.0) / 512.0 * z, z)
    b = tr.unproject(CAM, (float(u), float(v)))
    n = float(np.sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]))
    return dict(key=("hand", name), P=P, px=(float(u), float(v)), bearing=b, level=0, desc=np.zeros(32, np.uint8), idepth=1.0 / n, istd=0.05 / n, fixed=1)


def answer(sc, view, rec, start=None, ref_pose=ID, ref_view="same", key=None):
    """the oracle's SearchPoint for one record seen from the view's start pose -> (found, px, level), cached"""
    key = (view, rec["key"]) if key is None else key
    if key not in sc["answers"]:
        start = sc["start"][view] if start is None else start
        px0 = tr.project(CAM, tr.relative_pos(start, rec["P"]))
        a = sc["orc"].search_point(sc["img"][ref_view], sc["img"][view], CAM4, np.array(ref_pose), np.array(start), rec["px"], rec["bearing"], rec["level"],
                                   rec["desc"], rec["idepth"], rec["istd"], rec["fixed"], sc["corners"][view], px0)
        sc["answers"][key] = (bool(a["found"]), (float(a["px"][0]), float(a["px"][1])), int(a["level"]))
    return sc["answers"][key]


def found(sc, view, rec):
    return answer(sc, view, rec)[0]


# ---- building cases
class Case:
    def __init__(self, name, view, max_matches=MAX_MATCHES, seed=1, order_seed=None):
        self.name, self.view, self.max_matches, self.seed = name, view, max_matches, seed
        self.points, self.features = [], []      # rows: dict(rec, score, n_failed, status, last_frame); dict(px, bearing, level, point)
        self.order = list(range(N_CELLS))
        if order_seed is not None:
            self.order = [int(c) for c in np.random.default_rng(order_seed).permutation(N_CELLS)]
        self.claims = {}
        self.T0 = None             # start of the alignment where it is not the view's pose

    def point(self, rec, score=0, n_failed=0, status=P_FOUND, last_frame=FRAME_ID - 1, feature=True):
        self.points.append(dict(rec=rec, score=score, n_failed=n_failed, status=status, last_frame=last_frame))
        if feature:
            self.feature(rec, len(self.points) - 1)
        return len(self.points) - 1

    def feature(self, rec, point):
        self.features.append(dict(px=rec["px"], bearing=rec["bearing"], level=rec["level"], point=point))

    def cell_of(self, sc, rec):
        x, y = _px0(sc, self.view, rec)
        return int(y / CELL) * 20 + int(x / CELL)

    def rank(self):
        r = np.zeros(N_CELLS, np.uint16)
        r[np.array(self.order)] = np.arange(N_CELLS, dtype=np.uint16)
        return r


def restate(sc, case, T=None, search=None, pose=None, final_pose=None, trace=None, points=None, features=None, last_pose=ID, frame_id=FRAME_ID):
    """track_restatement.step on a case: by default the search is the oracle's cached answers and the pose the oracle's
    SelectInliers + OptimizePose on the case's rand() stream"""
    orc = sc["orc"]
    if points is None:
        points = [tr.Point(p["rec"]["P"], p["score"], p["n_failed"], p["last_frame"], p["status"]) for p in case.points]
    if features is None:
        features = [tr.Feature(f["px"], f["level"], f["point"]) for f in case.features]
    if search is None:
        def search(pt, px0):
            return answer(sc, case.view, case.points[pt]["rec"])
    if pose is None:
        def pose(start, obs):
            if not obs:
                return dict(pose=start, n_draws=0, inliers=[], outliers=[], refined=0)
            return orc.pose_from_matches(CAM4, np.array(obs), np.array(start), W, H, rand_seed=case.seed)
    T = sc["T0"][case.view] if T is None else T
    return tr.step(points, features, T, last_pose, frame_id, case.max_matches, case.order, CAM, CELL, PATCH, MAX_FAILED, search, pose, trace,
                   final_pose) + (points,)


def _singles(sc, view):
    """usable records the oracle finds in the view, one per cell, and the usable ones it does not find"""
    hit, seen = [], set()
    for i in sc["usable"]:
        rec = sc["records"][i]
        x, y = _px0(sc, view, rec)
        c = int(y / CELL) * 20 + int(x / CELL)
        if c not in seen and found(sc, view, rec):
            seen.add(c)
            hit.append(rec)
    return hit


def cases(sc):
    if "cases" in _made:
        return _made["cases"]
    R = sc["records"]
    live = {v: _singles(sc, v) for v in ("same", "moved")}
    assert len(live["moved"]) >= 60 and len(live["same"]) >= 60, (len(live["moved"]), len(live["same"]))
    out = []

    # -- hand-placed points on every threshold of ProjectPoint, and everything ProjectPoints skips
    c = Case("thresholds", "same", order_seed=3)
    for name, u, v, z in (("behind", 100, 100, -1e-3), ("in-front", 100, 100, 1e-3),
                          ("x7", 7, 100, 2.0), ("x8", 8, 100, 2.0), ("x631", 631, 100, 2.0), ("x632", 632, 100, 2.0),
                          ("y7", 100, 7, 2.0), ("y8", 100, 8, 2.0), ("y471", 100, 471, 2.0), ("y472", 100, 472, 2.0),
                          ("cell-corner", 352, 96, 2.0), ("before-cell-corner", 351, 95, 2.0)):
        c.point(hand(name, u, v, z))
    c.point(dict(hand("on-the-camera-plane", 100, 100, 1.0), P=(0.25, -0.125, 0.0)))      # z = 0 exactly: projects to infinities
    c.point(dict(hand("camera-centre", 100, 100, 1.0), P=(0.0, 0.0, 0.0)))                  # 0 / 0
    L = live["same"]
    c.point(L[0], status=DELETED | P_FOUND, last_frame=FRAME_ID - 7)
    c.point(L[1], status=TRASH | P_FOUND)
    c.point(hand("trash-outside", 2, 2), status=TRASH | P_FOUND)
    c.point(L[2], last_frame=FRAME_ID)
    c.feature(L[3], -1)
    dup = c.point(L[4], score=2)
    c.feature(L[4], dup | DUPLICATE)
    for rec in L[5:45]:
        c.point(rec, score=len(c.points) % 4)
    c.claims = dict(unseen=["behind", "x7", "x632", "y7", "y472", "trash-outside", "on-the-camera-plane", "camera-centre"], seen=["in-front", "x8", "x631", "y8", "y471", "cell-corner",
                                                                                           "before-cell-corner"])
    out.append(c)

    # -- three points in one cell, two of them with equal scores, in both list orders: the miss has the highest score, the hit is the
    #    equal-score point the feature list names first, the other one is never tried
    for name, first in (("tie-ab", 0), ("tie-ba", 1)):
        c = Case(name, "moved", order_seed=4)
        L = live["moved"]
        a = dict(L[10], key=L[10]["key"] + ("a",))
        b = dict(L[10], key=L[10]["key"] + ("b",))
        c.point(flipped(L[10]), score=7, feature=False)
        c.point(a, score=5, feature=False)
        c.point(b, score=5, feature=False)
        for p in ((1, 0, 2) if first == 0 else (2, 0, 1)):
            c.feature(c.points[p]["rec"], p)
        for rec in L[11:30]:
            c.point(rec, score=1)
        c.claims = dict(tried=[0, 1 if first == 0 else 2], untried=2 if first == 0 else 1)
        out.append(c)

    # -- the cap reached in the middle of the cell order: 40 cells hold a findable point, 10 matches are asked for
    c = Case("cap-10-of-40", "moved", max_matches=10, order_seed=5)
    for k, rec in enumerate(live["moved"][:40]):
        c.point(rec, score=k % 3)
    out.append(c)

    # -- failures: a cell whose first candidate misses and second hits, a cell of only misses, n_failed around MaxFailed before a miss,
    #    and max_matches equal to the number found
    c = Case("failures", "moved", order_seed=6)
    L = live["moved"]
    c.point(flipped(L[0]), score=9)
    c.point(L[0], score=1, n_failed=4)
    c.point(flipped(L[1]), score=3)
    c.point(dict(flipped(L[1]), key=("flipped-again",) + L[1]["key"]), score=3, n_failed=2)
    for k, nf in enumerate((MAX_FAILED - 1, MAX_FAILED, MAX_FAILED + 1)):
        c.point(flipped(L[2 + k]), n_failed=nf)
    c.point(flipped(L[5]), n_failed=MAX_FAILED, status=TRASH | P_FOUND)
    for rec in L[6:17]:
        c.point(rec, score=2)
    c.max_matches = 12          # = the number found: L[0] and L[6:17]
    # the cells of the misses come first: the last hit is the last thing the loop does
    first = []
    for p in c.points[2:8] + c.points[:2] + c.points[8:]:
        if c.cell_of(sc, p["rec"]) not in first:
            first.append(c.cell_of(sc, p["rec"]))
    c.order = first + [k for k in c.order if k not in first]
    out.append(c)

    # -- nothing found at all
    c = Case("nothing-found", "moved", order_seed=7)
    for rec in live["moved"][:9]:
        c.point(flipped(rec), n_failed=1)
    out.append(c)

    # -- an odd and an even number of surviving points (what survives RemoveOutliers is asserted in check_cases)
    for name, n, seed in (("survivors-21", 21, 11), ("survivors-22", 22, 12)):
        c = Case(name, "moved", seed=seed, order_seed=8)
        for rec in live["moved"][20:20 + n]:
            c.point(rec)
        out.append(c)

    # -- every match an outlier: three points whose positions are wrong by a few pixels in opposite directions — the search still finds
    #    their corners, no pose explains them
    c = Case("all-outliers", "moved", seed=5, order_seed=9)
    for k, rec in enumerate(live["moved"][30:30 + ALL_OUTLIERS_N]):
        sx, sy = ALL_OUTLIERS_SHIFT[k % len(ALL_OUTLIERS_SHIFT)]
        c.point(dict(rec, key=rec["key"] + ("shifted", k), P=(rec["P"][0] + sx, rec["P"][1] + sy, rec["P"][2])))
    out.append(c)

    # -- and some of them outliers: 20 good points and 3 whose positions are wrong by five pixels
    c = Case("some-outliers", "moved", seed=6, order_seed=10)
    for rec in live["moved"][45:65]:
        c.point(rec, score=1)
    for k, rec in enumerate(live["moved"][65:68]):
        sx, sy = ((0.02, 0.0), (0.0, -0.02), (-0.02, 0.02))[k]
        c.point(dict(rec, key=rec["key"] + ("shifted", k), P=(rec["P"][0] + sx, rec["P"][1] + sy, rec["P"][2])), score=2)
    out.append(c)

    # -- launch forms: feature counts around the request block of 4 and the stride granule
    for n in (1, 7, 8, 9):
        c = Case("features-%d" % n, "moved", seed=20 + n, order_seed=20 + n)
        for rec in live["moved"][40:40 + n]:
            c.point(rec, score=n)
        out.append(c)

    # -- more than 256 candidates (stride above 256: the 512-thread projection, the commit scan's second round); the cell order puts a
    #    two-candidate cell (a miss, then a hit) across candidate position 256
    c = Case("over-256", "moved", seed=31)
    U = [R[i] for i in sc["usable"]]
    doubles = live["moved"][:150]
    for rec in doubles:
        c.point(flipped(rec), score=5)
        c.point(rec, score=1)
    keys = set(r["key"] for r in doubles)
    dcells = set(c.cell_of(sc, r) for r in doubles)
    singles = []
    for rec in U:
        if rec["key"] not in keys and c.cell_of(sc, rec) not in dcells and len(singles) < 100:
            c.point(rec, score=2)
            singles.append(rec)
    # cells in visiting order: 127 doubles (254 candidates), ONE single (position 254), then a double at 255 | 256
    rng = np.random.default_rng(32)
    dorder = [c.cell_of(sc, r) for r in doubles]
    scells = []
    for r in singles:
        k = c.cell_of(sc, r)
        if k not in scells:
            scells.append(k)
    per_cell = Counter(c.cell_of(sc, r) for r in singles)
    lone = [k for k in scells if per_cell[k] == 1]
    head = dorder[:127] + [lone[0]] + [dorder[127]]
    rest = [k for k in range(N_CELLS) if k not in head]
    c.order = head + [int(k) for k in rng.permutation(rest)]
    c.claims = dict(straddle=dorder[127])
    out.append(c)

    # -- the largest feature list the alignment takes (2048 rows, stride 2048: 53 KB of dynamic LDS in track_project), 100 of them with
    #    points.  (The form beyond 60 KB needs more than 2360 rows and cannot be reached: see test_more_features_than_the_alignment_takes)
    c = Case("rows-2048", "moved", seed=41, order_seed=41)
    L = live["moved"]
    k = 0
    for i in range(2048):
        if i % 20 == 7 and k < 100:
            c.point(L[k % len(L)], score=k % 5)      # (beyond len(L): a second point at the place of an earlier one)
            k += 1
        else:
            c.feature(R[i % len(R)], -1)
    out.append(c)
    # -- live: real motion.  The alignment starts at the identity with the default parameters and has to find the k = 4 pose itself;
    #    the search answers are the oracle's for the pose it arrives at
    c = Case("live", "moved", seed=51, order_seed=51)
    c.T0 = ID
    for k, rec in enumerate(live["moved"][:180]):
        c.point(rec, score=k % 4)
    lost = [R[i] for i in sc["usable"] if not found(sc, "moved", R[i])][:20]
    for rec in lost:
        c.point(rec, score=1, n_failed=3)
    out.append(c)
    # the same behind 220 features without a point: above 384 features the plain alignment and the table's run in one form (four waves)
    wide = Case("live-wide", "moved", seed=52, order_seed=52)
    wide.T0 = ID
    for k in range(220):
        wide.feature(R[(7 * k) % len(R)], -1)
        if k < len(c.points):
            wide.point(c.points[k]["rec"], score=c.points[k]["score"], n_failed=c.points[k]["n_failed"])
    out.append(wide)

    # -- the first of two steps in a row: hits, misses, a point deleted, a trash point
    c = Case("step-one", "moved", seed=61, order_seed=61)
    for k, rec in enumerate(live["moved"][60:100]):
        c.point(rec, score=k % 3)
    for k, rec in enumerate(live["moved"][100:106]):
        c.point(flipped(rec), n_failed=MAX_FAILED - 2 + k % 4)
    c.point(live["moved"][106], status=TRASH | P_FOUND)
    out.append(c)
    _made["cases"] = out
    return out


def seed_on_view(sc, view, pose, n, skip=37):
    """n records first seen in the view's image at `pose`: points of the plane z = 2 behind every skip-th of its corners"""
    orc = sc["orc"]
    pyr = orc.pyramid(sc["img"][view], LEVELS)
    inv = orc.se3_inv(np.array(pose))
    Rw, tw = np.array(tr.rotation(tuple(inv[:4]))), inv[4:]
    out = []
    for i in range(5, len(sc["corners"][view]), skip):
        x, y, l = (int(v) for v in sc["corners"][view][i])
        px = (float(x << l), float(y << l))
        if not (64 <= px[0] < W - 64 and 64 <= px[1] < H - 64):
            continue
        b = tr.unproject(CAM, px)
        rw = Rw @ np.array(b)
        s = (2.0 - tw[2]) / rw[2]
        Pw = Rw @ (np.array(b) * s) + tw
        desc, _ = orc.orb_describe(pyr[l], [[x, y]])
        out.append(dict(key=("seeded", view, i), P=tuple(float(v) for v in Pw), px=px, bearing=b, level=l, desc=desc[0], idepth=float(1.0 / s),
                        istd=float(0.05 / s), fixed=1))
        if len(out) == n:
            break
    assert len(out) == n
    return out


# the shifted points of "all-outliers": metres on the plane z = 2 (1 px = 1 / 256 m), chosen on the CPU with the oracle
ALL_OUTLIERS_N = 3
ALL_OUTLIERS_SHIFT = ((0.012, 0.0), (-0.012, 0.0), (0.0, 0.012))

SMALL = ("thresholds", "tie-ab", "tie-ba", "cap-10-of-40", "failures", "nothing-found", "survivors-21", "survivors-22", "all-outliers", "some-outliers",
         "features-1", "features-7", "features-8", "features-9")      # <= 256 candidates: together in the sets of 5 and 33


def by_name(cs):
    return {c.name: c for c in cs}


def restated_trace(sc, cs):
    trace = Counter()
    for c in cs:
        restate(sc, c, trace=trace)
    return trace


def check_cases(sc, cs):
    """every case is what it claims, by the oracle's answers alone"""
    C = by_name(cs)
    assert set(SMALL) <= set(C) and len(C) == len(cs)
    res = {}
    for c in cs:
        t = Counter()
        res[c.name] = restate(sc, c, trace=t) + (t,)
        assert len(c.features) <= 2048 and max(c.order) == N_CELLS - 1 and sorted(c.order) == list(range(N_CELLS)), c.name
        for f in c.features:
            assert f["point"] < 0 or (f["point"] & (DUPLICATE - 1)) < len(c.points), c.name

    r, new, stats, pts, t = res["thresholds"]
    c = C["thresholds"]
    names = {p["rec"]["key"][1]: i for i, p in enumerate(c.points) if p["rec"]["key"][0] == "hand"}
    for n in c.claims["unseen"]:
        assert stats[names[n]][3] & 0xFF == tr.P_UNSEEN, n
    for n in c.claims["seen"]:
        assert stats[names[n]][3] & 0xFF != tr.P_UNSEEN and stats[names[n]][2] == FRAME_ID, n
    for n, (u, v) in (("x8", (8, 100)), ("x631", (631, 100)), ("y8", (100, 8)), ("y471", (100, 471)), ("cell-corner", (352, 96)),
                      ("before-cell-corner", (351, 95))):
        assert _px0(sc, "same", c.points[names[n]]["rec"]) == (float(u), float(v)), n      # exactly
    assert c.cell_of(sc, c.points[names["cell-corner"]]["rec"]) == 3 * 20 + 11 and c.cell_of(sc, c.points[names["before-cell-corner"]]["rec"]) == 2 * 20 + 10
    for b in ("behind-camera", "deleted-point", "trash-seen", "trash-unseen", "last-frame-is-this-frame", "feature-without-point",
              "duplicate-feature", "trash-becomes-deleted"):
        assert t[b] >= 1, b
    assert t["outside-margin"] == 7 and t["behind-camera"] == 1 and t["trash-becomes-deleted"] == 2 and r["matches"] >= 30
    assert c.order != list(range(N_CELLS))                    # a shuffled cell order

    for name in ("tie-ab", "tie-ba"):
        r, new, stats, pts, t = res[name]
        c = C[name]
        assert t["equal-scores-in-a-cell"] >= 1 and t["hit-behind-a-miss"] == 1
        hit, untried = c.claims["tried"][1], c.claims["untried"]
        assert stats[0][:2] == (7, 1) and stats[hit][:2] == (6, 0) and stats[hit][3] == tr.P_FOUND, name
        assert stats[untried] == (5, 0, FRAME_ID, tr.P_SEEN), name
        assert [f.point for f in new].count(hit) == 1 and untried not in [f.point for f in new]

    r, new, stats, pts, t = res["cap-10-of-40"]
    assert r["matches"] == 10 and t["cap-reached-before-the-last-cell"] == 1 and r["attempts"] == 10
    assert sum(1 for s in stats if s[3] == tr.P_SEEN) == 30          # 30 cells with a findable point were never visited (>= 25)

    r, new, stats, pts, t = res["failures"]
    assert r["matches"] == 12 == C["failures"].max_matches and t["cap-reached"] == 1 and t["cap-reached-before-the-last-cell"] == 0
    assert t["hit-behind-a-miss"] == 1 and t["cell-of-misses"] >= 5 and t["miss-at-max-failed"] == 1 and r["n_deleted"] == 3
    assert [s[1] for s in stats[:8]] == [1, 0, 1, 3, MAX_FAILED, MAX_FAILED + 1, MAX_FAILED + 2, MAX_FAILED + 1]
    assert [bool(s[3] & DELETED) for s in stats[:8]] == [False, False, False, False, False, True, True, True]

    r, new, stats, pts, t = res["nothing-found"]
    assert (r["matches"], r["attempts"], r["scene_depth"], r["n_draws"]) == (0, 9, 0.0, 0) and t["no-depth"] == 1

    parity = set()
    for name in ("survivors-21", "survivors-22"):
        r, new, stats, pts, t = res[name]
        assert r["matches"] == int(name[-2:]) and r["n_points"] >= 15
        parity.add(r["n_points"] % 2)
        assert t["median-of-even" if r["n_points"] % 2 == 0 else "median-of-odd"] == 1
    assert parity == {0, 1}

    r, new, stats, pts, t = res["all-outliers"]
    assert r["matches"] == ALL_OUTLIERS_N == r["n_outliers"] and r["n_inliers"] == 0 and r["n_points"] == 0 and r["scene_depth"] == 0.0
    assert t["every-match-an-outlier"] == 1 and all(f.point == -1 for f in new) and all(s[3] == tr.P_NOT_FOUND and s[0] == 1 for s in stats)

    r, new, stats, pts, t = res["some-outliers"]
    assert r["n_inliers"] == 20 and r["n_outliers"] >= 2 and r["matches"] == 20 + r["n_outliers"] and t["outlier"] == r["n_outliers"]
    assert sorted(f.point for f in new) == [-1] * r["n_outliers"] + list(range(20))        # the outliers are the shifted points,
    assert r["outliers"] != list(range(20, 20 + r["n_outliers"]))                           # and not at the end of the match list

    for n in (1, 7, 8, 9):
        r = res["features-%d" % n][0]
        assert r["n_features"] == n == r["matches"]

    r, new, stats, pts, t = res["over-256"]
    c = C["over-256"]
    assert r["n_requests"] > 256 and 256 < len(c.features) <= 704
    grid = tr.project_points(sc["start"]["moved"], [tr.Feature(f["px"], f["level"], f["point"]) for f in c.features],
                             [tr.Point(p["rec"]["P"], p["score"], p["n_failed"], p["last_frame"], p["status"]) for p in c.points], FRAME_ID, CAM, CELL,
                             PATCH)
    at = 0
    for k in c.order:
        if k == c.claims["straddle"]:
            break
        at += len(grid[k])
    cell = sorted(grid[c.claims["straddle"]], key=lambda e: -c.points[e[0]]["score"])
    assert at == 255 and len(cell) == 2, (at, len(cell))               # candidates 255 and 256
    assert [found(sc, "moved", c.points[e[0]]["rec"]) for e in cell] == [False, True]
    assert 150 <= r["matches"] < MAX_MATCHES

    r, new, stats, pts, t = res["rows-2048"]
    assert r["n_features"] == 2048 and 0 < r["n_requests"] <= 120 and r["matches"] >= 50

    r, new, stats, pts, t = res["live"]          # (restated here from the true pose; the GPU test restates from the aligned one)
    assert r["matches"] >= 100 and t["miss"] >= 10 and len(C["live"].features) == 200
    assert res["live-wide"][0]["matches"] >= 100 and 384 < len(C["live-wide"].features) == 420 <= 704
    r, new, stats, pts, t = res["step-one"]
    assert r["matches"] == 41 and r["n_deleted"] >= 2 and t["trash-becomes-deleted"] == 1 and t["miss"] == 6
    over = Counter()
    for v in res.values():
        over.update(v[4])
    return over
