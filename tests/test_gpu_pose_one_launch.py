"""The pose stage in one launch (csrc/sdvl_pose.hip: pose_refine_kernel with the match selection and the RANSAC draws inside, for sets
of more than 4 trackers), where tests/test_gpu_parity.py's chain test, with its four trackers, does not reach:

  the selection by one wave, candidates in rounds of 64, against the host replay of SelectPoints (first found candidate per cell, at
      most max_matches) followed by ctx.pose_from_matches on the replay's observations — 5 trackers (three-wave body) and 33 (one-wave
      body), candidate lists built around the rounds: counts 0, 1, 63, 64, 65, 130, a cell across a round boundary, caps reached inside
      and at the end of a round, candidates without a request, nothing found.  Everything equal, the poses bit for bit.
  `cand_req == nullptr` (candidate k = request cand_begin + k): a closed loop of the tabled step on a farm group of 33 trackers
      against the CPU oracle, as tests/test_gpu_tracker.py holds its farm loops.
  the draw batches (kFirstDraws draws converged at a time): 33 jobs whose oracle draw counts fall below the first batch, inside the
      second and beyond 64, accepted as tests/test_gpu_pose.py accepts.
  the capacity limits of the chain call, and that the context survives a refusal."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import test_gpu_parity as par
import test_gpu_pose as tp
from oraclelib import TUM_CAM, XI, trajectory_pose

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "..", "slam-sdvl_amd", "csrc", "sdvl_pose.hip")) as _f:
    FIRST_DRAWS = int(re.search(r"#define SDVL_POSE_FIRST_DRAWS (\d+)", _f.read()).group(1))
assert FIRST_DRAWS in (16, 32, 64)
CHAIN_MAX_CAND = 16384          # kChainMaxCand, csrc/sdvl_search_types.h

_shared = {}


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    for f in _shared.get("frames", ()):
        f.close()
    c.close()


def chain_inputs(ctx, sdvl, orc, synth):
    """one frame pair with ~300 requests as par.chain_case makes them, their points, and which of them the search finds; made once"""
    if "reqs" not in _shared:
        img_ref, img_cur = par.frames_of(synth, orc, TUM_CAM, 640, 480, [0, 5])
        T_ref, T_cur = trajectory_pose(orc, 0), trajectory_pose(orc, 5)
        reqs, meta, ccur, f_ref, f_cur = par.search_requests(sdvl, orc, ctx, img_ref, img_cur, T_ref, T_cur, TUM_CAM, 300, 21, True, 0.0, describe=False)
        for r in list(reqs)[-12:]:          # a dozen requests nobody can find: every bit of the point's descriptor turned over
            for k in range(32):
                r.desc[k] ^= 0xFF
        from oraclelib import quat_to_R
        Tw = orc.se3_inv(T_ref)
        Rw, tw = quat_to_R(Tw[:4]), Tw[4:]
        pts = np.stack([Rw @ (m["bearing"] / m["idepth"]) + tw for m in meta])
        cam = sdvl.Camera(640, 480, *TUM_CAM)
        sp = sdvl.default_search_params()
        res = ctx.search_points(reqs, cam, sp)
        found = np.array([bool(r.found) for r in res])
        _shared.update(reqs=reqs, pts=pts, cam=cam, sp=sp, found=found, T_cur=T_cur, frames=(f_ref, f_cur))
    s = _shared
    return s["reqs"], s["pts"], s["cam"], s["sp"], s["found"], s["T_cur"]


def shapes(found):
    """name -> (cells, max_matches): candidate lists that meet the selection's rounds of 64 where they can go wrong.  F and N deal out
    found and not-found requests in turn."""
    F, N = list(np.flatnonzero(found)), list(np.flatnonzero(~found))
    assert len(F) >= 70 and len(N) >= 3, (len(F), len(N))
    state = {"f": 0, "n": 0}

    def f():
        state["f"] += 1
        return int(F[state["f"] % len(F)])

    def n():
        state["n"] += 1
        return int(N[state["n"] % len(N)])

    def mixed(count):      # cells of 1 to 3 candidates, found and not, `count` candidates in all
        cells, k = [], 0
        while k < count:
            size = min(1 + (k * 7) % 3, count - k)
            cells.append([f() if (k + j) % 4 != 1 else n() for j in range(size)])
            k += size
        return cells

    out = {
        "count-0": ([], 200),
        "count-1": ([[f()]], 200),
        "count-63": (mixed(63), 200),
        "count-64": (mixed(64), 200),
        "count-65": (mixed(65), 200),
        # 130 candidates: positions 62..66 are ONE cell, found at 63 (first round: the match) and at 65 (second round: not a match);
        # positions 126..129 are one cell whose candidates of the second round (126, 127) are not found and whose hit is 128, in the third
        "count-130": (mixed(62) + [[n(), f(), n(), f(), n()]] + mixed(59) + [[n(), n(), f(), n()]], 200),
        "no-request-only": ([[-1], [-1, -1], [-1] * 70], 200),
        "no-request-among": ([[-1, f()], [f(), -1], [-1, -1, n()], [-1] * 64 + [f()], [n(), -1, f()]] + mixed(20), 200),
        "cap-40-inside-a-round": ([[f()] for _ in range(50)], 40),
        "cap-64-at-a-round-end": ([[f()] for _ in range(70)], 64),
        "none-found": ([[n(), n()], [n()], [-1, n()]] * 25, 200),
    }
    # the shapes are what they claim
    flat = {k: [r for c in v[0] for r in c] for k, v in out.items()}
    isf = lambda r: r >= 0 and bool(found[r])
    assert [len(flat[k]) for k in ("count-0", "count-1", "count-63", "count-64", "count-65", "count-130")] == [0, 1, 63, 64, 65, 130]
    c130 = out["count-130"][0]
    starts = np.cumsum([0] + [len(c) for c in c130])
    straddle = list(starts).index(62)
    assert len(c130[straddle]) == 5 and [isf(r) for r in c130[straddle]] == [False, True, False, True, False]      # 63 | 65
    last = list(starts).index(126)
    assert len(c130[last]) == 4 and [isf(r) for r in c130[last]] == [False, False, True, False]                      # 126, 127 | 128
    assert all(r == -1 for r in flat["no-request-only"]) and len(flat["no-request-only"]) > 64
    assert -1 in flat["no-request-among"] and any(isf(r) for r in flat["no-request-among"])
    assert sum(any(isf(r) for r in c) for c in out["cap-40-inside-a-round"][0]) > 40 and out["cap-40-inside-a-round"][1] == 40
    c64 = out["cap-64-at-a-round-end"][0]
    assert all(len(c) == 1 and isf(c[0]) for c in c64) and len(c64) > 64 and out["cap-64-at-a-round-end"][1] == 64   # match 64 = candidate 63
    assert len(flat["none-found"]) > 64 and not any(isf(r) for r in flat["none-found"])
    return out


def replay(cells, max_matches, found, res, pts):
    """the second half of SelectPoints on the host, as par.test_search_chain_equals_search_then_select_then_pose replays it"""
    sel = []
    for cell in cells:
        if len(sel) >= max_matches:
            break
        for r in cell:
            if r >= 0 and found[r]:
                sel.append(r)
                break
    obs = []
    for r in sel:
        x, y = (res[r].px[0] - TUM_CAM[2]) / TUM_CAM[0], (res[r].px[1] - TUM_CAM[3]) / TUM_CAM[1]
        nrm = np.sqrt(x * x + y * y + 1.0)
        v = np.array([x / nrm, y / nrm, 1.0 / nrm])          # Camera::Unproject
        obs.append([v[0] / v[2], v[1] / v[2], pts[r, 0], pts[r, 1], pts[r, 2], res[r].level])
    return np.array(obs).reshape(-1, 6)


def check_chain(ctx, trackers, reqs, pts, cam, sp, found):
    res, got = ctx.search_chain(reqs, cam, sp, trackers, pts, fx=TUM_CAM[0])
    assert np.array_equal(np.array([bool(r.found) for r in res]), found)
    jobs = [(replay(t["cells"], t["max_matches"], found, res, pts), t["pose"], t["draws"]) for t in trackers]
    want = ctx.pose_from_matches(jobs, fx=TUM_CAM[0])
    for g, w, j, t in zip(got, want, jobs, trackers):
        assert g["n_obs"] == len(j[0]), t["name"]
        assert g["n_draws"] == w["n_draws"] and g["refined"] == w["refined"], t["name"]
        assert np.array_equal(g["inliers"], w["inliers"]) and np.array_equal(g["outliers"], w["outliers"]), t["name"]
        assert np.array_equal(g["pose"], w["pose"]), t["name"]
        if len(j[0]) == 0:      # nothing selected: the pose comes back untouched, nothing is drawn
            assert g["n_draws"] == 0 and g["refined"] == 0 and len(g["inliers"]) == 0 and len(g["outliers"]) == 0, t["name"]
            assert np.array_equal(g["pose"], np.asarray(t["pose"], np.float64)), t["name"]
    return got


@pytest.mark.parametrize("n_trackers", [5, 33])
def test_fused_selection_equals_the_host_replay(ctx, sdvl, orc, synth, n_trackers):
    """5 trackers: more than 4, at most 32 — the three-wave body selects in wave 0 while the helpers wait; 33 trackers of at most 200
    matches: the one-wave body.  Every shape of shapes() in both."""
    reqs, pts, cam, sp, found, T_cur = chain_inputs(ctx, sdvl, orc, synth)
    sh = shapes(found)
    rng = np.random.default_rng(7)
    names = list(sh)
    assert n_trackers > 4 and (n_trackers <= 32) == (n_trackers == 5) and max(v[1] for v in sh.values()) <= 256
    seen = {}
    for lo in range(0, len(names) if n_trackers == 5 else 1, n_trackers):
        batch = [names[(lo + i) % len(names)] for i in range(n_trackers)]
        trackers = [dict(name=n, cells=sh[n][0], max_matches=sh[n][1], pose=T_cur, draws=rng.integers(0, 2**31 - 1, 100)) for n in batch]
        for t, g in zip(trackers, check_chain(ctx, trackers, reqs, pts, cam, sp, found)):
            seen[t["name"]] = g["n_obs"]
    assert set(seen) == set(names)
    assert seen["cap-40-inside-a-round"] == 40 and seen["cap-64-at-a-round-end"] == 64 and seen["count-1"] == 1
    assert seen["count-0"] == seen["no-request-only"] == seen["none-found"] == 0


def test_chain_limits_are_refused_and_the_context_stays_usable(ctx, sdvl, orc, synth):
    reqs, pts, cam, sp, found, T_cur = chain_inputs(ctx, sdvl, orc, synth)
    rng = np.random.default_rng(8)
    Fs = [int(r) for r in np.flatnonzero(found)]
    F = Fs[0]
    ok = [dict(name="ok-%d" % i, cells=[[r] for r in Fs[i:i + 20]], max_matches=100, pose=T_cur, draws=rng.integers(0, 2**31 - 1, 100)) for i in range(5)]
    many = dict(name="many", cells=[[F] * (CHAIN_MAX_CAND + 1)], max_matches=100, pose=T_cur, draws=rng.integers(0, 2**31 - 1, 100))
    with pytest.raises(sdvl.SdvlError, match="too many candidates for one tracker"):
        ctx.search_chain(reqs, cam, sp, ok + [many], pts, fx=TUM_CAM[0])
    big = dict(ok[0], name="big", max_matches=1025)
    with pytest.raises(sdvl.SdvlError, match=r"max_matches outside the device pose stage's range \(1024\)"):
        ctx.search_chain(reqs, cam, sp, ok + [big], pts, fx=TUM_CAM[0])
    full = dict(name="full", cells=[[F] * CHAIN_MAX_CAND], max_matches=100, pose=T_cur, draws=rng.integers(0, 2**31 - 1, 100))
    got = check_chain(ctx, ok + [full], reqs, pts, cam, sp, found)      # exactly the capacity passes; one cell: one match
    assert [g["n_obs"] for g in got] == [20] * 5 + [1]


def test_draw_batches_below_inside_and_beyond(ctx, orc):
    """33 jobs of at most 256 matches under the default limits (one-wave body; draws in batches of FIRST_DRAWS).  Which batch the
    replay stops in is the oracle's n_draws alone."""
    names = (tp.FILLERS * 3)[:33]
    assert tp.forms_of(names) == (False, False) and set(names) == set(tp.FILLERS)
    draws = {n: tp.wanted(orc, n)["n_draws"] for n in set(names)}
    assert any(d < FIRST_DRAWS for d in draws.values()), draws
    assert any(FIRST_DRAWS < d <= 2 * FIRST_DRAWS for d in draws.values()), draws
    assert any(d > 64 for d in draws.values()), draws
    got = tp.run(ctx, orc, names, tp.DEFAULTS)
    bad = [d for n, g in zip(names, got) for d in tp.differences(orc, n, g)]
    assert not bad, bad


def test_tabled_step_on_a_group_of_33(orc, synth):
    """cand_req == nullptr: the tracked step's candidates are its requests.  One farm group of 33 trackers (one-wave body), 3 distinct
    sequences replicated, 6 frames at 640x480: replicas agree bit for bit, the distinct ones equal the CPU oracle (decisions exact, poses
    within 1e-4), as tests/test_gpu_tracker.py::test_farm_at_bench_size_replicas_agree_and_match_the_oracle holds them."""
    sdvl = importlib.import_module("slam-sdvl_amd")
    trk = importlib.import_module("slam-sdvl_amd.tracker")
    import bench as B
    G, Bg, n_steps, distinct = 1, 33, 6, 3
    n = G * Bg
    trk.configure()
    farm = trk.TrackerFarm(0, G, Bg, 640, 480, TUM_CAM)
    c = B.CtxView(sdvl, farm.ctx_handle(0))
    fb = 640 * 480
    xis = [XI * (1.0 + 0.2 * i) * (1 if i % 2 == 0 else -1) for i in range(distinct)]
    which = [(i * 2) % distinct for i in range(n)]
    buf = c.malloc(n * n_steps * fb)
    for k in range(n_steps):
        views = [B.make_view(sdvl, trajectory_pose(orc, k, xis[which[i]]), 20260101 + which[i], k) for i in range(n)]
        c.render(views, buf + k * n * fb)
    ptrs = (buf + (np.arange(n_steps, dtype=np.uint64)[:, None] * n + np.arange(n, dtype=np.uint64)[None, :]) * fb).astype(np.uint64)
    farm.reserve(Bg * 6)
    st = farm.run(ptrs, G)
    rec = [(s.state, s.quality, s.keyframe, s.n_corners, s.matches, s.attempts, s.inliers, s.outliers, s.align_meas, tuple(s.pose[:])) for s in st]
    first = {}
    for k in range(n_steps):
        for i in range(n):
            first.setdefault((k, which[i]), rec[k * n + i])
            assert rec[k * n + i] == first[(k, which[i])], (k, i)
    for d in range(distinct):
        o = orc.tracker(640, 480, TUM_CAM)
        i0 = which.index(d)
        for k in range(n_steps):
            want = o.handle_frame(c.download(buf + (k * n + i0) * fb, fb).reshape(480, 640))
            g = first[(k, d)]
            assert g[:9] == (want.state, want.quality, want.keyframe, want.n_corners, want.matches, want.attempts, want.inliers, want.outliers,
                             want.align_meas), (k, d)
            assert np.abs(np.array(g[9]) - np.array(want.pose[:])).max() <= 1e-4
            if k > 0:
                assert g[1] == 0 and g[4] >= 100
        o.close()
    farm.close()
