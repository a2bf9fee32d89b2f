"""The visiting order track_project (csrc/sdvl_track.hip) leaves on the device — request order, cand_first, cand_feat, the block table —
read back with sdvl_track_read_order and compared slot by slot with tests/track_restatement.py: ProjectPoints' grid walked in the
case's cell order, every cell sorted by descending score, stably.  The attempts and matches of the step are the restatement's too.

The kernel finds a candidate's position as (candidates in cells of smaller rank) + (smaller keys among the candidates of its own
cell) through a histogram over the cell ranks; grids of more than 2048 cells keep the count of smaller keys over the whole list.  Its
launch is one wave for sets of more than 32 trackers up to stride 512; otherwise 256 threads, and 512 for stride > 256.  The cases
below are table sets made by hand, as tests/track_cases.py makes them, on its scene (view "moved", alignment of max_its = 0, so
the pose of every projection is known beforehand).

Not covered: the bucket of rank 0xFFFF (a projection in a cell k >= cells).  No call reaches it: sdvl_track_align refuses a set
whose cell count is not ceil(width / cell) * ceil(height / cell) (tests/test_gpu_track_tables.py, "the set's grid does not match
camera / cell size"), and a projection that passes Camera::IsInsideImage lies inside that grid.  The restatement has no such cell."""
import ctypes as C
import importlib
from collections import Counter

import numpy as np
import pytest

import track_cases as tc
import track_restatement as tr

pytestmark = pytest.mark.gpu

MAX_POINTS, MAX_MATCHES = 768, 256                       # (a set's max_matches is at most its feature rows)
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 256)        # 256: the full stride of a set of 256 feature rows
BUCKET_BOUND = 2048                                      # kProjBuckets of csrc/sdvl_track.hip
ONE_WAVE_STRIDE = 512                                    # kProjOneWaveStride
FINE_CELL, FINE_CELLS = 8, 4800                          # 640x480 at cell 8: 80 x 60 cells, above the bound
PX0_TOL = 1e-9      # the projection restated in Python against the device's: a dozen FP64 operations on values below 640 (ulp 1.1e-13)
BRANCHES = tuple("count-%d" % n for n in COUNTS) + (
    "count-300", "count-600", "one-cell-equal-scores", "one-cell-descending", "one-cell-ascending", "cell-of-its-own", "interleaved",
    "order-by-index-differs-from-point-order", "cell-of-three-or-more", "deleted-point", "duplicate-feature", "last-frame-is-this-frame", "behind-camera",
    "feature-without-point", "different-counts-in-one-set", "set-of-3", "set-of-33", "one-wave-form", "256-thread-form", "512-thread-form", "stride-above-256",
    "one-wave-form-above-stride-256", "set-of-33-above-the-one-wave-stride",
    "grid-above-the-bucket-bound", "grid-within-the-bucket-bound", "dead-slots", "no-dead-slot", "partial-block", "hit-behind-a-miss")
_w = {"met": Counter()}


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    for s in _w.get("sets", {}).values():
        s.close()
    for f in _w.get("frames", {}).values():
        f.close()
    c.close()


def _clear_fine(sc, rec):
    x, y = tc._px0(sc, "moved", rec)
    return all(abs(v - FINE_CELL * round(v / FINE_CELL)) > 1e-3 for v in (x, y))


class Case(tc.Case):
    """a case of tests/track_cases.py on a grid of its own"""

    def __init__(self, name, cell=tc.CELL, order_seed=1):
        tc.Case.__init__(self, name, "moved", max_matches=MAX_MATCHES)
        self.cell, self.n_cells = cell, tc.N_CELLS if cell == tc.CELL else FINE_CELLS
        self.order = [int(c) for c in np.random.default_rng(order_seed).permutation(self.n_cells)]

    def rank(self):
        r = np.zeros(self.n_cells, np.uint16)
        r[np.array(self.order)] = np.arange(self.n_cells, dtype=np.uint16)
        return r


def make_cases(sc, cell):
    """-> name -> Case.  Records come from the usable ones of the scene (away from every cell edge of the grid in use)"""
    U = [sc["records"][i] for i in sc["usable"]]
    if cell == FINE_CELL:
        U = [r for r in U if _clear_fine(sc, r)]
    U = U[:96]
    assert len(U) == 96
    out = {}

    def add(c):
        out[c.name] = c
        return c

    # feature counts: every feature a candidate; beyond the 96 records a second (third) point at the place of an earlier one; every
    # fourth point is one the search cannot find
    for n in COUNTS + (300, 600):
        c = add(Case("count-%d" % n, cell, order_seed=100 + n))
        if n == 0:
            c.point(U[0], feature=False)           # a table of one point and no feature
        for i in range(n):
            rec = U[(7 * i) % len(U)]
            c.point(tc.flipped(rec) if i % 4 == 1 else rec, score=(5 * i) % 3)
    # every candidate in ONE cell: 70 points at one place, the feature list in another order than the point rows, the even rows not findable
    for mode in ("equal-scores", "descending", "ascending"):
        c = add(Case("one-cell-" + mode, cell, order_seed=7))
        n = 70
        for i in range(n):
            c.point(tc.flipped(U[3]) if i % 2 == 0 else U[3], score=dict(equal=3, descending=n - i, ascending=i)[mode.split("-")[0]], feature=False)
        for p in np.random.default_rng(11).permutation(n).tolist():
            c.feature(c.points[p]["rec"], p)
    # every candidate in a cell of its own
    c = add(Case("cell-of-its-own", cell, order_seed=8))
    seen = set()
    for rec in U:
        k = _cell(sc, rec, cell)
        if k not in seen:
            seen.add(k)
            c.point(rec, score=len(seen) % 2)
    # non-candidates between the candidates: deleted points, duplicates, points already seen this frame, points behind the camera,
    # features without a point
    c = add(Case("interleaved", cell, order_seed=9))
    for i in range(90):
        rec = U[(5 * i) % len(U)]
        kind = i % 6
        if kind == 0:
            c.point(rec, status=tr.DELETED | tr.P_FOUND, last_frame=tc.FRAME_ID - 3)
        elif kind == 1:
            c.point(rec, last_frame=tc.FRAME_ID)
        elif kind == 2:
            c.point(dict(tc.hand("behind-%d" % i, 100 + i, 100, -1.0)))
        elif kind == 3:
            c.feature(rec, -1)
        else:
            p = c.point(rec, score=i % 5)
            if kind == 5:
                c.feature(rec, p | tr.DUPLICATE)
    return out


def _cell(sc, rec, cell):
    x, y = tc._px0(sc, "moved", rec)
    return int(y / cell) * int(np.ceil(tc.W / cell)) + int(x / cell)


@pytest.fixture(scope="module")
def world(ctx, sdvl, orc, synth):
    if "sc" not in _w:
        sc = tc.scene(orc, synth)
        _w.update(sc=sc, frames={}, sets={}, cases={tc.CELL: make_cases(sc, tc.CELL), FINE_CELL: make_cases(sc, FINE_CELL)})
        _w["frames"]["ref"] = ctx.frame(sc["img"]["same"])
        _w["frames"]["ref"].set_corners(sc["corners"]["same"])
        ctx.register([_w["frames"]["ref"]], [tc.ID])
        _w["cam"] = sdvl.Camera(tc.W, tc.H, *tc.CAM4)
        _w["raw"] = orc.rand_stream(tc.MAX_RANSAC_ITS, 1)
        fn = ctx.lib.sdvl_track_read_order
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8
    return _w


def params(sdvl, orc, cell):
    p = sdvl.TrackParams()
    p.align = sdvl.default_align_params()
    p.align.max_its = 0
    p.search = sdvl.default_search_params()
    p.pose = sdvl.PoseParams(orc.params.max_ransac_points, orc.params.max_ransac_its, orc.params.max_optim_pose_its, 0,
                             orc.params.inlier_error_threshold / tc.CAM4[0], tc.CAM4[0])
    p.cell_size, p.patch_size, p.max_failed = cell, tc.PATCH, tc.MAX_FAILED
    return p


def point_rows(sdvl, ref, rows):
    out = []
    for p in rows:
        r = p["rec"]
        t = sdvl.TrackPoint()
        t.position[:] = r["P"]
        t.px[:] = r["px"]
        t.bearing[:] = r["bearing"]
        t.idepth, t.idepth_std = r["idepth"], r["istd"]
        t.ref = ref.h.value
        t.level, t.fixed = r["level"], r["fixed"]
        t.score, t.n_failed, t.last_frame, t.status = p["score"], p["n_failed"], p["last_frame"], p["status"]
        t.desc[:] = [int(b) for b in r["desc"]]
        out.append(t)
    return out


def feature_rows(sdvl, rows):
    out = []
    for f in rows:
        t = sdvl.TrackFeature()
        t.px[:] = f["px"]
        t.bearing[:] = f["bearing"]
        t.level, t.point = f["level"], f["point"]
        out.append(t)
    return out


def restated(sc, case):
    """-> (visiting order: rows (feature row, point row, px0, first slot of its cell), matches, attempts, trace)"""
    def rows():
        return ([tr.Point(p["rec"]["P"], p["score"], p["n_failed"], p["last_frame"], p["status"]) for p in case.points],
                [tr.Feature(f["px"], f["level"], f["point"]) for f in case.features])
    points, features = rows()
    grid = tr.project_points(sc["start"]["moved"], features, points, tc.FRAME_ID, tc.CAM, case.cell, tc.PATCH)
    assert len(grid) == case.n_cells
    feature_of = {}
    for i, f in enumerate(case.features):
        if f["point"] >= 0 and not f["point"] & tr.DUPLICATE:
            assert f["point"] not in feature_of
            feature_of[f["point"]] = i
    visit = []
    for c in case.order:
        first = len(visit)
        for pt, px0 in sorted(grid[c], key=lambda e: -case.points[e[0]]["score"]):        # stable
            visit.append((feature_of[pt], pt, px0, first))
    points, features = rows()
    trace = Counter()

    def search(pt, px0):
        return tc.answer(sc, "moved", case.points[pt]["rec"])

    def pose(start, obs):      # (neither count depends on the pose stage)
        return dict(pose=start, n_draws=0, inliers=[], outliers=[], refined=0)
    want, _, _ = tr.step(points, features, sc["T0"]["moved"], tc.ID, tc.FRAME_ID, case.max_matches, case.order, tc.CAM, case.cell, tc.PATCH,
                         tc.MAX_FAILED, search, pose, trace)
    assert want["n_requests"] == len(visit)
    return visit, want["matches"], want["attempts"], trace, grid


def run_and_compare(w, ctx, sdvl, orc, n_trackers, max_features, cell, names):
    """one step of a set: job j runs case names[j] on tracker n_trackers - 1 - j; every slot of every job against the restatement"""
    sc, met = w["sc"], w["met"]
    cases = [w["cases"][cell][n] for n in names]
    n_cells = cases[0].n_cells
    key = (n_trackers, max_features, n_cells)
    if key not in w["sets"]:
        w["sets"][key] = ctx.track_set(n_trackers, MAX_POINTS, max_features, n_cells, MAX_MATCHES, tc.MAX_RANSAC_ITS)
    s = w["sets"][key]
    ref = w["frames"]["ref"]
    trackers = [n_trackers - 1 - j for j in range(len(names))]
    s.upload(trackers, [0] * len(names), [point_rows(sdvl, ref, c.points) for c in cases], [feature_rows(sdvl, c.features) for c in cases])
    jobs = (sdvl.TrackJob * len(names))()
    for j, c in enumerate(cases):
        if ("cur", j) not in w["frames"]:
            w["frames"]["cur", j] = ctx.frame(sc["img"]["moved"])
            w["frames"]["cur", j].set_corners(sc["corners"]["moved"])
        jobs[j].tracker, jobs[j].feat_buf = trackers[j], 0
        jobs[j].last, jobs[j].cur = ref.h.value, w["frames"]["cur", j].h.value
        jobs[j].T[:] = sc["T0"]["moved"]
        jobs[j].last_pose[:] = tc.ID
        jobs[j].frame_id, jobs[j].max_matches = tc.FRAME_ID, c.max_matches
    res, _, _ = s.step(jobs, np.stack([c.rank() for c in cases]), np.stack([w["raw"]] * len(names)), w["cam"], params(sdvl, orc, cell))
    n = len(names)
    cap = n * ((max_features + 3) // 4 * 4)
    stride = C.c_int32(0)
    first, feat, level, bfirst, bcount = (np.full(cap, -7, np.int32) for _ in range(5))
    px, px0 = np.zeros((cap, 2)), np.zeros((cap, 2))
    ctx._check(ctx.lib.sdvl_track_read_order(ctx.h, s.h, n, cap, C.addressof(stride), *(a.ctypes.data for a in (first, feat, level, px, px0, bfirst, bcount))))
    stride = stride.value
    longest = max(len(c.features) for c in cases)
    assert stride == max(4, (longest + 3) // 4 * 4), (stride, longest)
    counts = set()
    for j, (name, c) in enumerate(zip(names, cases)):
        label = "%s as job %d of a set of %d (stride %d, %d cells)" % (name, j, n_trackers, stride, n_cells)
        visit, matches, attempts, trace, grid = restated(sc, c)
        base, nc = j * stride, len(visit)
        print("%s: %d features, %d candidates, %d matches, %d attempts" % (label, len(c.features), nc, matches, attempts))
        assert res[j].n_features == len(c.features) and res[j].n_requests == nc, (label, res[j].n_features, res[j].n_requests)
        assert feat[base:base + nc].tolist() == [v[0] for v in visit], label
        assert first[base:base + nc].tolist() == [base + v[3] for v in visit], label
        assert level[base:base + nc].tolist() == [c.points[v[1]]["rec"]["level"] for v in visit], label        # request order: the
        assert px[base:base + nc].tolist() == [list(c.points[v[1]]["rec"]["px"]) for v in visit], label           # point's own record
        if nc:
            assert np.abs(px0[base:base + nc] - np.array([v[2] for v in visit])).max() <= PX0_TOL, label
        assert (level[base + nc:base + stride] == -1).all(), label                                               # dead slots
        nb = stride // 4
        assert bfirst[j * nb:(j + 1) * nb].tolist() == [base + 4 * b for b in range(nb)], label
        assert bcount[j * nb:(j + 1) * nb].tolist() == [min(4, max(0, nc - 4 * b)) for b in range(nb)], label
        assert (res[j].matches, res[j].attempts) == (matches, attempts), (label, res[j].matches, res[j].attempts, matches, attempts)
        # what this comparison has been through
        counts.add(len(c.features))
        met[name] += 1
        for b in ("deleted-point", "duplicate-feature", "last-frame-is-this-frame", "behind-camera", "feature-without-point", "hit-behind-a-miss"):
            met[b] += trace[b]
        largest = max(len(g) for g in grid)
        met["cell-of-three-or-more"] += largest >= 3
        if name.startswith("one-cell"):
            assert largest == nc == 70, label
            met["order-by-index-differs-from-point-order"] += [v[0] for v in visit] != [v[1] for v in visit]
        if name == "cell-of-its-own":
            assert largest == 1 and nc >= 40, (label, nc)
        if name == "interleaved":
            assert 0 < nc < len(c.features), label
        met["dead-slots" if nc < stride else "no-dead-slot"] += 1
        met["partial-block"] += nc % 4 != 0
        met["set-of-%d" % n_trackers] += 1
        one_wave = n_trackers > 32 and stride <= ONE_WAVE_STRIDE
        met["one-wave-form" if one_wave else ("512-thread-form" if stride > 256 else "256-thread-form")] += 1
        met["stride-above-256"] += stride > 256
        met["one-wave-form-above-stride-256"] += one_wave and stride > 256
        met["set-of-33-above-the-one-wave-stride"] += n_trackers > 32 and not one_wave
        met["grid-above-the-bucket-bound" if n_cells > BUCKET_BOUND else "grid-within-the-bucket-bound"] += 1
    met["different-counts-in-one-set"] += len(counts) > 1


ALL = tuple("count-%d" % n for n in COUNTS) + ("one-cell-equal-scores", "one-cell-descending", "one-cell-ascending", "cell-of-its-own", "interleaved")


def test_set_of_33_one_wave_every_case_in_one_step(world, ctx, sdvl, orc):
    run_and_compare(world, ctx, sdvl, orc, 33, 256, tc.CELL, ALL)


@pytest.mark.parametrize("lo", range(0, len(ALL), 3))
def test_set_of_3_three_cases_a_step(world, ctx, sdvl, orc, lo):
    run_and_compare(world, ctx, sdvl, orc, 3, 256, tc.CELL, ALL[lo:lo + 3])


def test_stride_above_256(world, ctx, sdvl, orc):
    run_and_compare(world, ctx, sdvl, orc, 3, 704, tc.CELL, ("count-300", "count-65", "one-cell-equal-scores"))
    run_and_compare(world, ctx, sdvl, orc, 33, 704, tc.CELL, ("interleaved", "count-300", "count-0", "one-cell-ascending", "cell-of-its-own"))
    run_and_compare(world, ctx, sdvl, orc, 33, 704, tc.CELL, ("count-64", "count-600", "one-cell-descending"))


@pytest.mark.parametrize("n_trackers", [3, 33])
def test_grid_above_the_bucket_bound(world, ctx, sdvl, orc, n_trackers):
    """4800 cells: the count of smaller keys over the whole list, and the walk back to the cell's first candidate"""
    assert FINE_CELLS > BUCKET_BOUND >= tc.N_CELLS
    names = ("count-129", "one-cell-equal-scores", "interleaved", "count-256", "cell-of-its-own", "count-0", "one-cell-descending", "count-2")
    for lo in range(0, len(names) if n_trackers == 3 else 1, 3):
        run_and_compare(world, ctx, sdvl, orc, n_trackers, 256, FINE_CELL, names[lo:lo + 3] if n_trackers == 3 else names)


def test_every_case_was_compared_and_every_branch_met(world):
    """last in the module: nothing above was skipped on the way"""
    met = world["met"]
    assert set(ALL) | {"count-300", "count-600"} <= set(BRANCHES)          # every case counts as a branch of its own
    missing = [b for b in BRANCHES if not met[b]]
    assert not missing, missing
