"""The kernel forms and memory layouts the host dispatch picks by size, and the edges between them, against the CPU oracle.

Each entry point behind include/sdvl_hip.h that changes its launch with the size of a call is run at the sizes on both sides of
every threshold: image-alignment feature counts around kLdsMaxF and the SDVL_MAX_ALIGN_FEATURES cap, mixed batches of small and
big jobs, the align store, a search frame table over its staging cap, search workgroups of every run length, the three
filter-corners forms, undistort batches that fill and do not fill a frame group, and align-patches tails.  Tolerance classes
are those of the parity test of each entry point (tests/test_gpu_parity.py).  Each test that aims at a form asserts that it
reached it: the host condition restated the way the dispatch computes it (the line is cited), or the kernel timer's names."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

from oraclelib import TUM_CAM, TUM_DIST, quat_rot, trajectory_pose
from test_gpu_parity import POSE_TOL, align_inputs, frames_of, search_requests

pytestmark = pytest.mark.gpu

T_ID = np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
K_LDS_MAX_F = 384          # csrc/sdvl_image_align.hip:26 (one wave per job up to this many features)
MAX_ALIGN_FEATURES = 2048  # SDVL_MAX_ALIGN_FEATURES, include/sdvl_hip.h:37
SEARCH_TAB_CAP = 2048      # kSearchTabCap, csrc/sdvl_search.hip
WAVES_PER_BLOCK = 4        # kWavesPerBlock: requests per search workgroup, patch jobs per align-patches workgroup
BIN_CELLS_SMALL, BIN_CORNERS_SMALL, BIN_CELLS = 512, 2048, 2048   # csrc/sdvl_orb.hip:234-235
REMAP_FRAMES = 4           # kRemapFrames, csrc/sdvl_undistort.hip:194

ALIGN_COUNTS = [1, 63, 64, 65, 128, 129, 383, 384, 385, 767, 768, 769, 2048]


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ image alignment
@pytest.fixture(scope="module")
def ia(sdvl, orc, synth, ctx):
    """frames 0, 2, 3, 5 of the trajectory and 4096 features of frame 0; feature 0 made valid so that a one-feature job measures"""
    ks = [0, 2, 3, 5]
    imgs = frames_of(synth, orc, TUM_CAM, 640, 480, ks)
    px, bearing, depth, valid, feats = align_inputs(sdvl, orc, imgs[0], TUM_CAM, 4096, 20260400)
    valid[0] = 1
    feats[0].valid = 1
    fr = [ctx.frame(im) for im in imgs]
    yield dict(imgs=imgs, frames=fr, px=px, bearing=bearing, depth=depth, valid=valid, feats=feats,
               cam=sdvl.Camera(640, 480, *TUM_CAM))
    for f in fr:
        f.close()


def result_fields(r):
    return (tuple(r.T), r.error, r.chi2, r.n_meas, tuple(r.its), r.stop, r.iters_run)


def align_timed(ctx, jobs, feats, cam, ap):
    """image_align with the kernel timer on -> (results, names of the Gauss-Newton forms that ran)"""
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        res = ctx.image_align(jobs, feats, cam, ap)
        names = {k for k, (_, launches) in ctx.timing_get().items() if launches > 0}
    finally:
        ctx.timing_enable(False)
    return res, names & {"image_align", "image_align_big"}


def oracle_align(orc, d, cur, b, e, T0=T_ID, min_level=2, max_level=4, max_its=30):
    p = orc.params
    old = (p.min_align_level, p.max_align_level, p.max_img_align_its)
    p.min_align_level, p.max_align_level, p.max_img_align_its = min_level, max_level, max_its
    try:
        return orc.image_align(d["imgs"][0], d["imgs"][cur], TUM_CAM, d["px"][b:e], d["bearing"][b:e], d["depth"][b:e],
                               d["valid"][b:e], T0)
    finally:
        p.min_align_level, p.max_align_level, p.max_img_align_its = old


def assert_align_matches(r, want):
    """the class of test_image_align_pose_within_tolerance: pose within POSE_TOL, n_meas exact, its within +-1"""
    assert np.abs(np.array(r.T[:]) - want["T"]).max() <= POSE_TOL, (list(r.T), want["T"])
    assert r.n_meas == want["n"], (r.n_meas, want["n"])
    assert np.abs(np.array(r.its[:]) - want["its"]).max() <= 1, (list(r.its), want["its"])


@pytest.mark.parametrize("n_feat", ALIGN_COUNTS)
def test_image_align_feature_counts(ctx, sdvl, orc, ia, n_feat):
    """one job at every count on both sides of a wave (64), of two rounds, of kLdsMaxF (one wave per job up to 384, four waves
    beyond: csrc/sdvl_image_align.hip:859) and at the SDVL_MAX_ALIGN_FEATURES cap"""
    res, forms = align_timed(ctx, [(ia["frames"][0], ia["frames"][2], 0, n_feat, T_ID)], ia["feats"], ia["cam"], sdvl.default_align_params())
    assert forms == {"image_align" if n_feat <= K_LDS_MAX_F else "image_align_big"}
    want = oracle_align(orc, ia, 2, 0, n_feat)
    assert want["n"] > 0
    if n_feat > 1:
        assert_align_matches(res[0], want)
        return
    # A lone feature fixes the 2-D motion of its projection, not the six pose parameters: H has rank 2, and the LDLT
    # pseudo-solve fills the null space from rounding (the oracle's and the kernel's differ by 0.09 there).  What is determined
    # is where the feature lands, and how many features were measured.
    assert res[0].n_meas == want["n"]
    P = ia["bearing"][0] * ia["depth"][0]
    land = []
    for T in (np.array(res[0].T[:]), want["T"]):
        pc = quat_rot(T[:4]) @ P + T[4:]
        land.append([TUM_CAM[0] * pc[0] / pc[2] + TUM_CAM[2], TUM_CAM[1] * pc[1] / pc[2] + TUM_CAM[3]])
    assert np.abs(np.subtract(*land)).max() < 0.05, land
    assert np.abs(np.array(land[1]) - ia["px"][0]).max() > 0.2        # (the feature did move)


def test_image_align_capacity_is_reported_and_the_context_stays_usable(ctx, sdvl, orc, ia):
    ap = sdvl.default_align_params()
    job = (ia["frames"][0], ia["frames"][2], 0, MAX_ALIGN_FEATURES + 1, T_ID)
    lib = ctx.lib
    res = (sdvl.AlignResult * 1)()
    rc = lib.sdvl_image_align(ctx.h, 1, ctx._align_jobs([job]), len(ia["feats"]), ia["feats"], C.byref(ia["cam"]), C.byref(ap), res)
    assert rc == -3                                                      # SDVL_ERR_CAPACITY
    assert "SDVL_MAX_ALIGN_FEATURES" in lib.sdvl_last_error(ctx.h).decode()
    with pytest.raises(sdvl.SdvlError, match="too many features"):      # and as the binding reports it
        ctx.image_align([job], ia["feats"], ia["cam"], ap)
    got = ctx.image_align([(ia["frames"][0], ia["frames"][2], 0, 300, T_ID)], ia["feats"], ia["cam"], ap)[0]
    assert_align_matches(got, oracle_align(orc, ia, 2, 0, 300))


def mixed_jobs(ia):
    """every count of ALIGN_COUNTS once, interleaved small / big / empty, at distinct feature offsets and current frames"""
    small = [n for n in ALIGN_COUNTS if n <= K_LDS_MAX_F]
    big = [n for n in ALIGN_COUNTS if n > K_LDS_MAX_F]
    order = []
    while small or big:
        if small:
            order.append(small.pop(0))
        if big:
            order.append(big.pop(0))
        order.append(0)
    fr = ia["frames"]
    jobs = []
    for j, n in enumerate(order):
        b = (j * 97) % (len(ia["feats"]) - n)
        jobs.append((fr[0], fr[1 + j % 3], b, b + n, T_ID))
    return jobs


def test_image_align_mixed_batch_equals_each_job_alone(ctx, sdvl, ia):
    """small and big jobs in one call: small-first reorder, results scattered back through IaJob::out_index, the big jobs'
    precompute behind the small jobs' (csrc/sdvl_image_align.hip:855-921).  max_f only sets the LDS / precompute pitch, the
    sums run in the same order: every result is bit-identical to the job run alone"""
    jobs = mixed_jobs(ia)
    ap = sdvl.default_align_params()
    res, forms = align_timed(ctx, jobs, ia["feats"], ia["cam"], ap)
    assert forms == {"image_align", "image_align_big"}
    n_small = sum(1 for j in jobs if j[3] - j[2] <= K_LDS_MAX_F)
    assert 0 < n_small < len(jobs) and any(j[3] == j[2] for j in jobs)
    for j, (job, r) in enumerate(zip(jobs, res)):
        alone = ctx.image_align([job], ia["feats"], ia["cam"], ap)[0]
        assert result_fields(r) == result_fields(alone), (j, job[3] - job[2])
        if job[3] == job[2]:
            assert tuple(r.T) == tuple(T_ID) and r.n_meas == 0


@pytest.mark.parametrize("min_level,max_level,max_its", [(0, 0, 30), (0, 4, 30), (3, 3, 30), (2, 4, 0)])
def test_image_align_levels_and_iterations(ctx, sdvl, orc, ia, min_level, max_level, max_its):
    ap = sdvl.AlignParams(max_level=max_level, min_level=min_level, max_its=max_its, patch_size=4, fast=0)
    jobs = [(ia["frames"][0], ia["frames"][2], 0, 300, T_ID), (ia["frames"][0], ia["frames"][3], 300, 800, T_ID)]
    res = ctx.image_align(jobs, ia["feats"], ia["cam"], ap)
    for (ref, cur, b, e, T), r, k in zip(jobs, res, (2, 3)):
        want = oracle_align(orc, ia, k, b, e, min_level=min_level, max_level=max_level, max_its=max_its)
        assert_align_matches(r, want)
        if max_its == 0:
            assert tuple(r.T) == tuple(T_ID) and not any(r.its)


def test_image_align_refuses_levels_beyond_the_pyramid(ctx, sdvl, orc, ia):
    f0, f1 = ctx.frame(ia["imgs"][0], levels=3), ctx.frame(ia["imgs"][2], levels=3)
    try:
        with pytest.raises(sdvl.SdvlError, match="pyramid depth"):
            ctx.image_align([(f0, f1, 0, 100, T_ID)], ia["feats"], ia["cam"], sdvl.AlignParams(3, 2, 30, 4, 0))
        with pytest.raises(sdvl.SdvlError, match="bad align levels"):
            ctx.image_align([(ia["frames"][0], ia["frames"][2], 0, 100, T_ID)], ia["feats"], ia["cam"], sdvl.AlignParams(8, 2, 30, 4, 0))
        got = ctx.image_align([(f0, f1, 0, 200, T_ID)], ia["feats"], ia["cam"], sdvl.AlignParams(2, 0, 30, 4, 0))[0]
        assert_align_matches(got, oracle_align(orc, ia, 2, 0, 200, min_level=0, max_level=2))
    finally:
        f0.close(); f1.close()


def edge_features(sdvl, cam, w, h, level, rng):
    """features a thousandth of a level pixel on either side of the border tests at `level`: ui - 3 < 0 / ui + 3 >= W of
    PrecomputePatches (image_align.cc: border = 3) and u - (half_patch + 1) < 0 / u + half_patch + 1 >= W of ComputeResiduals, on
    all four sides, at random positions along the edge"""
    s = float(1 << level)
    lw, lh = w >> level, h >> level
    eps = 1e-3
    xs = [3 - eps, 3 + eps, lw - 3 - eps, lw - 3 + eps]
    ys = [3 - eps, 3 + eps, lh - 3 - eps, lh - 3 + eps]
    pts = []
    for x in xs:
        for _ in range(4):
            pts.append((x * s, rng.uniform(8, lh - 8) * s))
    for y in ys:
        for _ in range(4):
            pts.append((rng.uniform(8, lw - 8) * s, y * s))
    px = np.array(pts, np.float64)
    n = len(px)
    ray = np.stack([(px[:, 0] - cam[2]) / cam[0], (px[:, 1] - cam[3]) / cam[1], np.ones(n)], 1)
    bearing = ray / np.linalg.norm(ray, axis=1, keepdims=True)
    depth = 2.0 / bearing[:, 2]
    valid = np.ones(n, np.uint8)
    feats = (sdvl.AlignFeature * n)()
    for i in range(n):
        feats[i].px, feats[i].py = px[i]
        feats[i].fx, feats[i].fy, feats[i].fz = bearing[i]
        feats[i].depth = depth[i]
        feats[i].valid = 1
    return px, bearing, depth, valid, feats


@pytest.mark.parametrize("level", [0, 2, 3, 4])
def test_image_align_features_on_the_border_tests(ctx, sdvl, orc, ia, level):
    """frame aligned with itself from the identity at one level: the projections stay where the features are, so n_meas counts
    exactly the features inside both border tests — half of those placed here"""
    img = ia["imgs"][0]
    px, bearing, depth, valid, feats = edge_features(sdvl, TUM_CAM, 640, 480, level, np.random.default_rng(level))
    ap = sdvl.AlignParams(max_level=level, min_level=level, max_its=30, patch_size=4, fast=0)
    r = ctx.image_align([(ia["frames"][0], ia["frames"][0], 0, len(px), T_ID)], feats, ia["cam"], ap)[0]
    p = orc.params
    old = (p.min_align_level, p.max_align_level)
    p.min_align_level, p.max_align_level = level, level
    try:
        want = orc.image_align(img, img, TUM_CAM, px, bearing, depth, valid, T_ID)
    finally:
        p.min_align_level, p.max_align_level = old
    assert want["n"] == 2 * 2 * 4, want["n"]          # 3 + eps and lw - 3 - eps are inside (floor: 3, lw - 4), 3 - eps and lw - 3 + eps not
    assert_align_matches(r, want)


def test_image_align_motion_carries_features_out(ctx, sdvl, orc, synth, ia):
    """half of the features within 12.5-30 px of the four edges, half inside; the current view is the plane seen from 6 cm right
    and 3 cm down (15 and 8 px at level 0): the pose is recovered, and part of the edge features end outside the current image at
    the finest level (ComputeResiduals' border test) — n_meas exact"""
    T_cur = orc.se3_exp(np.array([0.06, 0.03, 0, 0, 0, 0]))
    img_cur = synth.render(T_cur, TUM_CAM, 640, 480, seed=20260001, frame_id=1)
    rng = np.random.default_rng(77)
    n = 240
    side = np.arange(n) % 8
    near = rng.uniform(12.5, 30, n)
    xs = np.select([side == 0, side == 1, side >= 4], [near, 640 - near, rng.uniform(60, 580, n)], rng.uniform(20, 620, n))
    ys = np.select([side == 2, side == 3, side >= 4], [near, 480 - near, rng.uniform(60, 420, n)], rng.uniform(20, 460, n))
    px = np.stack([xs, ys], 1)
    ray = np.stack([(px[:, 0] - TUM_CAM[2]) / TUM_CAM[0], (px[:, 1] - TUM_CAM[3]) / TUM_CAM[1], np.ones(n)], 1)
    bearing = ray / np.linalg.norm(ray, axis=1, keepdims=True)
    depth = 2.0 / bearing[:, 2]
    valid = np.ones(n, np.uint8)
    feats = (sdvl.AlignFeature * n)()
    for i in range(n):
        feats[i].px, feats[i].py = px[i]
        feats[i].fx, feats[i].fy, feats[i].fz = bearing[i]
        feats[i].depth = depth[i]
        feats[i].valid = 1
    fk = ctx.frame(img_cur)
    r = ctx.image_align([(ia["frames"][0], fk, 0, n, T_ID)], feats, ia["cam"], sdvl.default_align_params())[0]
    fk.close()
    want = orc.image_align(ia["imgs"][0], img_cur, TUM_CAM, px, bearing, depth, valid, T_ID)
    assert n // 2 <= want["n"] <= n - 20, want["n"]     # a good part of the edge features carried out
    assert np.abs(want["T"] - T_cur).max() < 5e-3       # and the motion recovered
    assert_align_matches(r, want)


def test_align_store_equals_image_align(ctx, sdvl, ia):
    """sdvl_align_store_write in two calls at a non-zero offset, then sdvl_image_align_begin_stored + _end with jobs naming store
    records: the results of sdvl_image_align on the same features, bit for bit (small and big jobs, an empty one)"""
    base, n_store = 1000, 3000
    store = sdvl.AlignStore(ctx, base + n_store + 16)
    try:
        store.write(base, ia["feats"], 0, 1234)
        store.write(base + 1234, ia["feats"], 1234, n_store)
        fr = ia["frames"]
        spans = [(0, 300), (300, 1069), (1069, 1069), (1100, 1101), (1500, 3000), (2000, 2384)]
        plain_jobs = [(fr[0], fr[1 + j % 3], b, e, T_ID) for j, (b, e) in enumerate(spans)]
        stored_jobs = [(r, c, base + b, base + e, T) for (r, c, b, e, T) in plain_jobs]
        ap = sdvl.default_align_params()
        want = ctx.image_align(plain_jobs, ia["feats"], ia["cam"], ap)
        got = ctx.image_align_stored(stored_jobs, store, ia["cam"], ap)
        for j, (g, w) in enumerate(zip(got, want)):
            assert result_fields(g) == result_fields(w), j
        assert sum(w.n_meas > 0 for w in want) == len(spans) - 1
    finally:
        store.close()


# ------------------------------------------------------------------------------------------------ search
def search_table_size(reqs):
    """entries of the batch's frame table: sdvl_search_slot (csrc/sdvl_search.hip) for the current then the reference
    (frame, pose) of every request, in request order (sdvl_search_pack_requests)"""
    table, where, last, last2 = [], {}, -1, -1
    for r in reqs:
        for f, pose in ((r.cur, tuple(r.cur_pose)), (r.ref, tuple(r.ref_pose))):
            if last >= 0 and table[last] == (f, pose):
                continue
            if last2 >= 0 and table[last2] == (f, pose):
                last, last2 = last2, last
                continue
            last2 = last
            if f in where and table[where[f]] == (f, pose):
                last = where[f]
                continue
            table.append((f, pose))
            where[f] = last = len(table) - 1
    return len(table)


@pytest.fixture(scope="module")
def many(sdvl, orc, synth, ctx):
    """2100 requests between frames 0 and 5: 700 seeded points three times over, every request's reference pose turned by a
    twist of its own (1e-9 rad), and the oracle's answer to each"""
    img_ref, img_cur = frames_of(synth, orc, TUM_CAM, 640, 480, [0, 5])
    T_ref, T_cur = trajectory_pose(orc, 0), trajectory_pose(orc, 5)
    base, meta0, ccur, f_ref, f_cur = search_requests(sdvl, orc, ctx, img_ref, img_cur, T_ref, T_cur, TUM_CAM, 700, 41, True, 0.0, False)
    n = 2100
    reqs = (sdvl.SearchReq * n)()
    meta, poses = [], []
    for i in range(n):
        copy_req(reqs, i, base, i % len(base))
        tw = np.array([0, 0, 0, 1e-9 * (1 + i), -7e-10 * (1 + i % 13), 3e-10 * (1 + i % 7)])
        Tr = orc.se3_mul(orc.se3_exp(tw), T_ref)
        for k in range(7):
            reqs[i].ref_pose[k] = Tr[k]
        meta.append(meta0[i % len(base)])
        poses.append(Tr)
    want = [orc.search_point(img_ref, img_cur, TUM_CAM, poses[i], T_cur, m["px"], m["bearing"], m["level"], m["desc"],
                             m["idepth"], m["istd"], True, ccur, m["px0"]) for i, m in enumerate(meta)]
    yield dict(reqs=reqs, meta=meta, poses=poses, want=want, T_cur=T_cur, cam=sdvl.Camera(640, 480, *TUM_CAM))
    f_ref.close(); f_cur.close()


def copy_req(dst, j, src, i):
    size = C.sizeof(dst._type_)
    C.memmove(C.addressof(dst) + j * size, C.addressof(src) + i * size, size)


def sub_requests(sdvl, reqs, idx):
    out = (sdvl.SearchReq * len(idx))()
    for j, i in enumerate(idx):
        copy_req(out, j, reqs, i)
    return out


def raw_bytes(arr):
    return C.string_at(C.addressof(arr), C.sizeof(arr))


SEARCH_FIRST_RUN = {}   # n_req -> the result bytes of the module's first run at that size


@pytest.mark.parametrize("n_req", [SEARCH_TAB_CAP - 1, SEARCH_TAB_CAP, 2100, 1, 32, 33, 64, 65, pytest.param(32, id="32-again")])
def test_search_points_frame_table_over_the_staging_cap(ctx, sdvl, many, n_req):
    """a frame table of 2048, 2049 and 2101 (frame, pose) entries: up to kSearchTabCap it rides in the staging copy, beyond it goes
    through the work buffer with a copy of its own (sdvl_search_enqueue, csrc/sdvl_search.hip).  Found, level and offsets bit-equal to the
    oracle; the chosen corner equals that of the same requests run in batches whose tables stay under the cap.
    Behind the large batches, in buffers that have grown: 1 request, and 32 / 33 and 64 / 65, where the packed requests (120 B:
    32 are 15 x 256) and the results (40 B: 32 are 5 x 256) fill their part of a buffer to the last byte and run one record over;
    32 a second time answers bit for bit as the first"""
    reqs = sub_requests(sdvl, many["reqs"], range(n_req))
    n_tab = search_table_size(reqs)
    assert n_tab == n_req + 1                                   # the current frame once, every reference pose its own entry
    sp = sdvl.default_search_params()
    res = ctx.search_points(reqs, many["cam"], sp)
    assert raw_bytes(res) == SEARCH_FIRST_RUN.setdefault(n_req, raw_bytes(res))
    chunks = [ctx.search_points(sub_requests(sdvl, reqs, range(b, min(b + 1000, n_req))), many["cam"], sp) for b in range(0, n_req, 1000)]
    n_found = 0
    for i in range(n_req):
        r, w, s = res[i], many["want"][i], chunks[i // 1000][i % 1000]
        assert r.found == w["found"], i
        assert (r.found, r.best_corner, tuple(r.px), r.level, r.slevel) == (s.found, s.best_corner, tuple(s.px), s.level, s.slevel), i
        if w["found"]:
            n_found += 1
            assert r.level == w["level"] and np.array_equal(np.array(r.px[:]), w["px"]), i
    assert n_found >= n_req // 4


def depth_states(sdvl, meta, max_failed):
    """a depth-filter state per request: the seed's depth, random counters, every 7th far away, every 11th fixed"""
    rng = np.random.default_rng(8)
    states = (sdvl.DepthState * len(meta))()
    for i, m in enumerate(meta):
        s = states[i]
        s.rho, s.sigma2 = m["idepth"], m["istd"] ** 2
        s.a, s.b = 10.0 + 5.0 * rng.random(), 10.0 + 8.0 * rng.random()
        s.z_range = 6.0
        s.cos_alpha, s.last_distance = 1.0, 1.0
        s.depth_mean = 2.0 if i % 7 else 40.0
        s.fixed = 1 if i % 11 == 3 else 0
        for k in range(3):
            s.position[k] = [0.1 * (i % 5), -0.05 * (i % 3), 2.0][k]
        s.n_failed = int(rng.integers(0, max_failed + 1))
        s.track_row = -1
    return states


def check_search_points_filter(ctx, sdvl, orc, many, n):
    """the first n requests of `many` through sdvl_search_points_filter: outcomes and counters exact, filter state within 1e-11
    relative, as test_depth_filter_behind_the_search -> the outcomes seen"""
    reqs, meta = sub_requests(sdvl, many["reqs"], range(n)), many["meta"][:n]
    max_failed = 15
    states = depth_states(sdvl, meta, max_failed)
    fp = sdvl.DepthParams()
    fp.px_error_angle = math.atan(1.0 / (2.0 * TUM_CAM[0])) * 2.0
    fp.min_depth, fp.scale_min_dist, fp.max_failed = 0.25, 0.25, max_failed
    res, fout = ctx.search_points_filter(reqs, many["cam"], sdvl.default_search_params(), states, fp)
    ref = orc.tracker(640, 480, TUM_CAM)
    ref.use_mapper(True)
    outcomes = set()
    try:
        for i in range(n):
            r, o, s, w = res[i], fout[i], states[i], many["want"][i]
            assert r.found == w["found"], i
            if w["found"]:
                assert np.array_equal(np.array(r.px[:]), w["px"]), i
            st0 = [s.rho, s.sigma2, s.a, s.b, s.z_range, s.cos_alpha, s.last_distance, s.position[0], s.position[1], s.position[2],
                   s.fixed, s.n_failed]
            want, st1 = ref.depth_filter(many["T_cur"], many["poses"][i], meta[i]["bearing"], r.found, r.px[:], s.depth_mean, st0)
            assert o.outcome == want, (i, o.outcome, want)
            assert o.n_failed == int(st1[11]), i
            got = np.array([o.rho, o.sigma2, o.a, o.b])
            assert np.all(np.abs(got - st1[:4]) <= 1e-11 * np.abs(st1[:4])), (i, got, st1[:4])
            outcomes.add(want & 0xFF)
    finally:
        ref.close()
    return outcomes


def test_search_points_filter_frame_table_over_the_staging_cap(ctx, sdvl, orc, many):
    """sdvl_search_points_filter with 2101 table entries: depth_filter_kernel (csrc/sdvl_depth_filter.hip) reads the frame table
    where the search left it, in the work buffer.  Outcomes and counters exact, filter state within 1e-11 relative, as test_depth_filter_behind_the_search"""
    assert search_table_size(many["reqs"]) > SEARCH_TAB_CAP
    outcomes = check_search_points_filter(ctx, sdvl, orc, many, len(many["reqs"]))
    assert len(outcomes) >= 3, outcomes


@pytest.mark.parametrize("n", [32, 33])
def test_search_points_filter_states_that_fill_their_part(ctx, sdvl, orc, many, n):
    """32 depth-filter states (104 B each) are 13 x 256 bytes: their part of the staged block has no padding behind it; 33 run one
    record over.  The outcome records (80 B) follow the search's own parts in the result buffers.  Same acceptance as above"""
    check_search_points_filter(ctx, sdvl, orc, many, n)


def search_blocks(cur_of_request):
    """the search's workgroups: runs of up to kWavesPerBlock consecutive requests of one current frame (sdvl_search_enqueue, csrc/sdvl_search.hip)"""
    blocks, i, n = [], 0, len(cur_of_request)
    while i < n:
        cnt = 1
        while i + cnt < n and cnt < WAVES_PER_BLOCK and cur_of_request[i + cnt] == cur_of_request[i]:
            cnt += 1
        blocks.append(cnt)
        i += cnt
    return blocks


@pytest.mark.parametrize("binned", [True, False], ids=["detected-frames", "set-corners-frames"])
def test_search_points_workgroups_of_every_run_length(ctx, sdvl, orc, synth, binned):
    """requests in runs of 1..9 of one current frame, alternating between two current frames: workgroups of 1..4 requests, runs
    split across workgroups.  Every frame from sdvl_detect_corners (binned): search_points_kernel<false, 1>; frames with
    set_corners: <true, kWavesPerBlock> (sdvl_search_launch_device, csrc/sdvl_search.hip).  Results equal the oracle's and those of the same
    requests in sorted order"""
    imgs = frames_of(synth, orc, TUM_CAM, 640, 480, [0, 4, 7])
    T = [trajectory_pose(orc, k) for k in (0, 4, 7)]
    cam = sdvl.Camera(640, 480, *TUM_CAM)
    sets = [search_requests(sdvl, orc, ctx, imgs[0], imgs[c], T[0], T[c], TUM_CAM, 45, 50 + c, c == 1, 0.01, False) for c in (1, 2)]
    extra = []
    if binned:
        fb = [ctx.frame(im) for im in imgs]
        got = ctx.detect_corners(fb, sdvl.default_detect_params(), 1000)
        assert np.array_equal(got[1], sets[0][2]) and np.array_equal(got[2], sets[1][2])
        for c, (reqs, _, _, _, _) in zip((1, 2), sets):
            for r in reqs:
                r.ref, r.cur = fb[0].h.value, fb[c].h.value
        extra = fb
    # interleave: B x1, C x2, B x3, ... C x8, B x9, then the other way round, so that each frame has a run of every length
    order, pos = [], [0, 0]
    for sweep in (0, 1):
        for length in range(1, 10):
            s = (length + sweep + 1) % 2
            order += [(s, pos[s] + k) for k in range(length)]
            pos[s] += length
    assert pos == [45, 45]
    inter = (sdvl.SearchReq * 90)()
    for j, (s, k) in enumerate(order):
        copy_req(inter, j, sets[s][0], k)
    blocks = search_blocks([inter[j].cur for j in range(90)])
    assert sorted(set(blocks)) == [1, 2, 3, 4] and len(blocks) > 90 // 4
    res = ctx.search_points(inter, cam, sdvl.default_search_params())
    sorted_res = [ctx.search_points(sets[s][0], cam, sdvl.default_search_params()) for s in (0, 1)]
    n_found = 0
    for j, (s, k) in enumerate(order):
        reqs, meta, ccur, _, _ = sets[s]
        m, r, q = meta[k], res[j], sorted_res[s][k]
        c = s + 1
        want = orc.search_point(imgs[0], imgs[c], TUM_CAM, T[0], T[c], m["px"], m["bearing"], m["level"], m["desc"], m["idepth"],
                                m["istd"], c == 1, ccur, m["px0"])
        assert r.found == want["found"], j
        if want["found"]:
            n_found += 1
            assert r.level == want["level"] and np.array_equal(np.array(r.px[:]), want["px"]), j
        assert (r.found, r.best_corner, tuple(r.px), r.level, r.slevel) == (q.found, q.best_corner, tuple(q.px), q.level, q.slevel), j
    assert n_found >= 20
    for st in sets:
        st[3].close(); st[4].close()
    for f in extra:
        f.close()


# ------------------------------------------------------------------------------------------------ filter corners
@pytest.mark.parametrize("w,h,cell,n_corners,form", [
    (1024, 512, 32, None, "small"),      # 512 cells
    (864, 608, 32, None, "large"),       # 513 cells
    (640, 480, 32, 2048, "small"),       # 300 cells, ccap on the small form's limit
    (640, 480, 32, 2049, "large"),       # 300 cells, one corner more
    (1024, 512, 16, None, "large"),      # 2048 cells
    (800, 656, 16, None, "unbinned"),    # 2050 cells
    (1024, 1024, 16, None, "unbinned"),  # 4096 cells, the grid's limit
])
def test_filter_corners_forms(ctx, sdvl, orc, synth, w, h, cell, n_corners, form):
    """the three forms of filter_select (csrc/sdvl_orb.hip:663-674): binned with 512 cells and 2048 corners at most, binned with
    2048 cells at most, unbinned beyond.  Kept indices, their truncated scores and ORB descriptors as the oracle's (the checks of
    test_filter_corners_selection_on_the_device), with a few cells locked"""
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    cam4 = np.array(TUM_CAM) * (w / 640.0)
    img = frames_of(synth, orc, cam4, w, h, [2])[0]
    if n_corners is None:
        corners = orc.detect_pyramid(img, nfeatures=2000)
    else:
        dense = orc.fast(img, thr=10, nonmax=True)
        dense = dense[(dense[:, 0] >= 20) & (dense[:, 0] < w - 20) & (dense[:, 1] >= 20) & (dense[:, 1] < h - 20)]
        assert len(dense) >= n_corners
        corners = np.concatenate([dense[:n_corners, :2], np.zeros((n_corners, 1), np.int32)], 1).astype(np.int32)
    n_cells, ccap = gw * gh, max(len(corners), 1)
    # the dispatch's condition, restated
    got_form = "small" if n_cells <= BIN_CELLS_SMALL and ccap <= BIN_CORNERS_SMALL else ("large" if n_cells <= BIN_CELLS else "unbinned")
    assert got_form == form, (n_cells, ccap)
    locked = [[cell * 1.5, cell * 2.5], [w - 1.0, h - 1.0], [w / 2.0, h / 3.0]]
    f = ctx.frame(img)
    f.set_corners(corners)
    try:
        idx, xyl, score, desc = ctx.filter_corners([f], [locked], cell_size=cell)[0]
    finally:
        f.close()
    old = orc.params.cell_size
    orc.params.cell_size = cell
    try:
        want = orc.filter_corners(img, corners, locked)
    finally:
        orc.params.cell_size = old
    assert len(want) > 30
    assert np.array_equal(idx, want), (len(idx), len(want))
    assert np.array_equal(xyl, corners[want])
    pyr = orc.pyramid(img, 5)
    for k in range(0, len(idx), 5):
        x, y, l = xyl[k]
        assert score[k] == int(orc.shi_tomasi(pyr[l], x, y))
        d, _ = orc.orb_describe(pyr[l], [[x, y]])
        inside = 19 <= x < pyr[l].shape[1] - 19 and 19 <= y < pyr[l].shape[0] - 19
        assert np.array_equal(desc[k], d[0] if inside else np.zeros(32, np.uint8))


# ------------------------------------------------------------------------------------------------ undistort
@pytest.mark.parametrize("h,w", [(61, 128), (70, 129), (131, 255), (483, 752)])
def test_undistort_batches_fill_and_miss_frame_groups(ctx, sdvl, orc, h, w):
    """batches of 1, 3, 4, 5, 8 and 9 distinct images: frame groups of kRemapFrames (4) that are complete (the kFull branch) and
    a last group of 1..3 (csrc/sdvl_undistort.hip:272-282); widths of one tile, one pixel over, not a multiple of four, and the
    EuRoC width; heights that leave a partial tile row.  Plain form and fused upload, every frame byte for byte as the oracle's"""
    cam4 = np.array([0.8 * w, 0.82 * w, w / 2.0 - 0.4, h / 2.0 + 0.3])
    dist = TUM_DIST if w >= 640 else np.array([-0.45, 0.3, 0.01, -0.008, 0.05])
    rng = np.random.default_rng(w * 1000 + h)
    imgs = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(9)]
    want = [orc.undistort(im, cam4, dist) for im in imgs]
    assert all((wnt != im).mean() > 0.3 for wnt, im in zip(want, imgs))
    c = sdvl.Camera(w, h, *cam4)
    batches = (1, 3, 4, 5, 8, 9)
    # frames of each workgroup's group: nf = min(n - f0, kRemapFrames) (csrc/sdvl_undistort.hip:272); kFull where nf == 4
    assert {min(n - f0, REMAP_FRAMES) for n in batches for f0 in range(0, n, REMAP_FRAMES)} == {1, 3, 4}
    for n in batches:
        got = ctx.undistort(imgs[:n], c, dist)
        for i in range(n):
            assert np.array_equal(got[i], want[i]), (n, i, int((got[i] != want[i]).sum()))
        fr = [ctx.frame(width=w, height=h, levels=1, pyramid=False) for _ in range(n)]
        try:
            ctx.undistort(imgs[:n], c, dist, frames=fr)
            for i in range(n):
                assert np.array_equal(fr[i].level(0), want[i]), ("fused", n, i)
        finally:
            for f in fr:
                f.close()


# ------------------------------------------------------------------------------------------------ align patches
@pytest.fixture(scope="module")
def patch_scene(orc, synth):
    """three frames of the trajectory, their pyramids and corners"""
    imgs = frames_of(synth, orc, TUM_CAM, 640, 480, [0, 3, 6])
    return imgs, [orc.pyramid(im, 5) for im in imgs], [orc.detect_pyramid(im) for im in imgs]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 8, 16, 17, 64, 65])
def test_align_patches_workgroup_tails(ctx, orc, patch_scene, n):
    """kWavesPerBlock patch jobs per workgroup (sdvl_align_patches, csrc/sdvl_search.hip): a lone job, a partial, a full, one over and two full
    workgroups plus one; each job on its own frame and pyramid level, bit-exact against the oracle.  Then the counts at which a part
    of the staged block or of the results is a whole number of 256-byte units, and one job more: 8 job records (32 B), 16 start
    points (16 B), 64 borders (100 B: 25 x 256)"""
    imgs, pyrs, corners = patch_scene
    fr = [ctx.frame(im) for im in imgs]
    rng = np.random.default_rng(300 + n)
    frames, levels, border, patch, uv0, meta = [], [], [], [], [], []
    for i in range(n):
        fi, l = i % 3, (i // 3 + i) % 3
        cl = corners[fi][corners[fi][:, 2] == l]
        x, y, _ = cl[int(rng.integers(0, len(cl)))]
        img = pyrs[fi][l]
        frames.append(fr[fi]); levels.append(l)
        border.append(img[y - 5:y + 5, x - 5:x + 5].reshape(-1))
        patch.append(img[y - 4:y + 4, x - 4:x + 4].reshape(-1))
        uv0.append(np.array([x, y], np.float64) + rng.uniform(-1.5, 1.5, 2))
        meta.append(fi)
    assert len(set(zip(meta, levels))) == min(n, 9)
    assert (n + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK == {1: 1, 3: 1, 4: 1, 5: 2, 9: 3, 8: 2, 16: 4, 17: 5, 64: 16, 65: 17}[n]
    uv, conv, its = ctx.align_patches(frames, levels, np.stack(border), np.stack(patch), np.stack(uv0))
    n_conv = 0
    for i in range(n):
        ok, px = orc.align_patch(pyrs[meta[i]][levels[i]], border[i], patch[i], uv0[i])
        assert bool(conv[i]) == bool(ok), i
        assert np.array_equal(uv[i], px), i
        n_conv += bool(ok)
    assert n_conv >= (n + 1) // 2
    for f in fr:
        f.close()
