"""Stereo rigs as calibrated, on the MI355X: the map kernel rectify_map and the remap behind it (sdvl_rectify, sdvl_frames_upload_rectified,
the colour route) byte for byte and word for word against tests/rectify_restatement.py at the sizes where the launches change form; the
context's cache of maps; the composition plan -> rectify -> sdvl_stereo_depth against an ideal pair rendered directly."""
import ctypes as C
import importlib

import numpy as np
import pytest

import rectify_cases as rc
import rectify_restatement as rr
from oraclelib import TUM_CAM, TUM_DIST
from raw_restatement import RAW_FORMATS, bayer_to_gray
from test_color_cpu import to_gray

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def rectification(pkg, c):
    return pkg.rectification(c["K"], c["D"], c["R"], c["rect"], c["w"], c["h"])


def undistort_maps_built(ctx):
    counters = (C.c_int64 * 4)()
    ctx.lib.sdvl_ctx_counters.argtypes = [C.c_void_p, C.c_void_p]
    assert ctx.lib.sdvl_ctx_counters(ctx.h, counters) == 0
    return counters[2]


# ---- bytes and words
@pytest.mark.parametrize("deg", rc.ROLLS)
@pytest.mark.parametrize("w,h", rc.SIZES)
def test_map_words_are_the_restatements(ctx, pkg, w, h, deg):
    c = rc.byte_case(w, h, deg)
    got = ctx.rectify_map_words(rectification(pkg, c), w, h)
    assert np.array_equal(got, rr.words(c["iu"], c["iv"], w, h))
    assert ctx.rectify_stats()[1] == c["no_source"]


@pytest.mark.parametrize("deg", rc.ROLLS)
@pytest.mark.parametrize("w,h", rc.SIZES)
def test_rectify_bytes_are_the_restatements(ctx, pkg, w, h, deg):
    """n = 1, 4, 5 frames (full and partial frame groups), from host memory, from device memory and from rows wider than the image"""
    import torch
    c = rc.byte_case(w, h, deg)
    r = rectification(pkg, c)
    stride = w + 5
    raws = [rc.raw_image(w, h, 20261300 + k, stride=stride) for k in range(5)]
    want = [rr.remap(np.ascontiguousarray(im[:, :w]), c["iu"], c["iv"]) for im in raws]
    for n in (1, 4, 5):
        dense = [np.ascontiguousarray(im[:, :w]) for im in raws[:n]]
        got = ctx.rectify(dense, r)
        for i in range(n):
            assert np.array_equal(got[i], want[i]), ("host", n, i)
        got = ctx.rectify(raws[:n], r, width=w)                      # host rows of w + 5 bytes
        for i in range(n):
            assert np.array_equal(got[i], want[i]), ("host stride", n, i)
        dev = [torch.from_numpy(np.array(im)).cuda() for im in raws[:n]]
        torch.cuda.synchronize()
        got = ctx.rectify(dev, r, width=w)                           # device rows of w + 5 bytes: a map of its own (the quads hold offsets)
        for i in range(n):
            assert np.array_equal(got[i], want[i]), ("device stride", n, i)
        dev = [torch.from_numpy(im).cuda() for im in dense]
        torch.cuda.synchronize()
        got = ctx.rectify(dev, r)
        for i in range(n):
            assert np.array_equal(got[i], want[i]), ("device", n, i)


@pytest.mark.parametrize("w,h", rc.SIZES)
def test_pixels_without_a_source_read_zero_and_are_counted(ctx, pkg, w, h):
    """rectified intrinsics that see past the raw image (the plan's override): zeros there, and the count is the restatement's"""
    c = rc.byte_case(w, h, 6.0, zoom=0.7)
    assert 0 < c["no_source"] < w * h
    r = rectification(pkg, c)
    raws = [np.full((h, w), 255, np.uint8), np.array(rc.raw_image(w, h, 20261400))]
    got = ctx.rectify(raws, r)
    assert ctx.rectify_stats()[1] == c["no_source"]
    for im, g in zip(raws, got):
        assert np.array_equal(g, rr.remap(im, c["iu"], c["iv"]))
    sx, sy, _, _ = rr.positions(c["iu"], c["iv"])
    all_out = (sx < -1) | (sy < -1) | (sx >= w) | (sy >= h)
    assert all_out.any() and not got[0][all_out].any() and (got[0][~all_out & (sx >= 0) & (sy >= 0) & (sx + 1 < w) & (sy + 1 < h)] == 255).all()
    assert np.array_equal(ctx.rectify_map_words(r, w, h), rr.words(c["iu"], c["iv"], w, h))


def test_rays_that_do_not_point_forward_have_no_source(ctx, pkg):
    """a rectified camera turned 80 degrees about y: on one side w = M (j, i, 1)_z is zero or negative.  Those pixels are "outside" by
    the rule, not by what x / w converts to: the restatement's words and count, zeros in the image"""
    c = rc.turned_away_case()
    w, h = c["w"], c["h"]
    r = rectification(pkg, c)
    assert np.array_equal(ctx.rectify_map_words(r, w, h), rr.words(c["iu"], c["iv"], w, h))
    assert ctx.rectify_stats()[1] == c["no_source"]
    got = ctx.rectify([np.full((h, w), 255, np.uint8)], r)[0]
    assert np.array_equal(got, rr.remap(np.full((h, w), 255, np.uint8), c["iu"], c["iv"]))
    assert not got[c["iu"] == -64].any()


def test_planned_rig_has_a_source_for_every_pixel(ctx, pkg):
    """the library's plan of the tum rig, both cameras: the restatement's words, no pixel without a source"""
    g, p = rc.rigs()["tum"], rc.planned("tum")
    out = pkg.stereo_rectify_plan(g["K1"], g["D1"], g["K2"], g["D2"], g["R"], g["T"], g["w"], g["h"])
    assert ctx.stereo_rectify_plan is pkg.stereo_rectify_plan
    for side, (K, D, Ri) in zip((out.left, out.right), rc.sides(g, p)):
        iu, iv = rr.map_fixed(K, D, Ri, p["rect"], g["w"], g["h"])
        assert np.array_equal(ctx.rectify_map_words(side, g["w"], g["h"]), rr.words(iu, iv, g["w"], g["h"]))
        assert ctx.rectify_stats()[1] == 0


# ---- the cache
def test_cache_builds_one_map_per_camera_and_leaves_undistortion_alone(pkg):
    w, h = 130, 70
    cams = [rectification(pkg, rc.byte_case(w, h, deg)) for deg in (0.5, 6.0)] + [rectification(pkg, rc.byte_case(w, h, 6.0, zoom=0.7))]
    img = np.array(rc.raw_image(w, h, 20261500))
    cam = pkg.Camera(w, h, *rc.byte_case(w, h, 0.5)["K"])
    other = pkg.Camera(w, h, *(rc.byte_case(w, h, 0.5)["K"] + 1.0))

    def run(with_rectify):
        ctx = pkg.Context(0)
        try:
            ctx.timing_enable()
            outs = []
            step = lambda r: outs.append(ctx.rectify([img], r)[0]) if with_rectify else None
            built = lambda: ctx.rectify_stats()[0]
            step(cams[0]); step(cams[1]); step(cams[0]); step(cams[1])
            if with_rectify:
                assert built() == 2                               # left, right, left, right: each map once
            outs.append(ctx.undistort([img], cam, TUM_DIST)[0])
            step(cams[2])
            if with_rectify:
                assert built() == 3                               # a third rig
            outs.append(ctx.undistort([img], cam, TUM_DIST)[0])    # reused
            step(cams[0])
            outs.append(ctx.undistort([img], other, TUM_DIST)[0])  # rebuilt
            step(cams[1])
            outs.append(ctx.undistort([img], cam, TUM_DIST)[0])    # rebuilt: the slot holds one map
            if with_rectify:
                assert built() == 3
                # four slots: a fourth camera takes the free one, a fifth evicts the least recently used map (cams[2]), not the pair in use
                step(rectification(pkg, rc.byte_case(w, h, 0.5, zoom=0.7)))
                step(rectification(pkg, rc.byte_case(w, h, 0.5, zoom=0.9)))
                assert built() == 5
                step(cams[0]); step(cams[1])
                assert built() == 5
                step(cams[2])
                assert built() == 6
            ctx.synchronize()
            launches = {k: v[1] for k, v in ctx.timing_get().items()}
            return undistort_maps_built(ctx), outs, launches
        finally:
            ctx.close()

    n_with, outs_with, launches = run(True)
    n_without, outs_without, _ = run(False)
    assert n_with == n_without == 3
    assert launches["rectify_map"] == 6
    c0, c1 = rc.byte_case(w, h, 0.5), rc.byte_case(w, h, 6.0)
    assert np.array_equal(outs_with[0], rr.remap(img, c0["iu"], c0["iv"])) and np.array_equal(outs_with[2], outs_with[0])
    assert np.array_equal(outs_with[1], rr.remap(img, c1["iu"], c1["iv"])) and np.array_equal(outs_with[3], outs_with[1])
    und_with = [outs_with[k] for k in (4, 6, 8, 10)]
    for a, b in zip(und_with, outs_without):
        assert np.array_equal(a, b)


# ---- uploads
def test_uploads_give_rectify_of_gray(ctx, pkg):
    """sdvl_frames_upload_rectified: level 0 = rectify(raw); through the colour route with "bgr" and "bayer_rggb": rectify(gray(raw))"""
    w, h = 130, 70
    c = rc.byte_case(w, h, 6.0)
    r = rectification(pkg, c)
    rng = np.random.default_rng(20261600)
    grays = [np.array(rc.raw_image(w, h, 20261601 + k)) for k in range(5)]
    frames = [ctx.frame(width=w, height=h, levels=3) for _ in grays]
    try:
        ctx.rectify(grays, r, frames=frames)
        for f, g in zip(frames, grays):
            assert np.array_equal(f.level(0), rr.remap(g, c["iu"], c["iv"]))
        bgr = [np.clip(g[..., None].astype(np.int32) + rng.integers(-40, 41, (3,)) + rng.integers(-6, 7, g.shape + (3,)), 0, 255).astype(np.uint8)
               for g in grays]
        ctx.upload_color_rectified(frames, bgr, pkg.SDVL_BGR8, r)
        for f, im in zip(frames, bgr):
            assert np.array_equal(f.level(0), rr.remap(to_gray(im, "bgr"), c["iu"], c["iv"]))
        ctx.upload_color_rectified(frames, grays, RAW_FORMATS["bayer_rggb"][0], r)
        for f, im in zip(frames, grays):
            assert np.array_equal(f.level(0), rr.remap(bayer_to_gray(im, "bayer_rggb"), c["iu"], c["iv"]))
        ctx.upload_color_rectified(frames, grays, pkg.SDVL_GRAY8, r)              # exactly the gray producer
        for f, g in zip(frames, grays):
            assert np.array_equal(f.level(0), rr.remap(g, c["iu"], c["iv"]))
        ctx.pyramid_build(frames)                                                  # the frames go on as after any upload
        assert frames[0].level(1).shape == (h // 2, w // 2)
    finally:
        for f in frames:
            f.close()


def test_refuses_bad_arguments(ctx, pkg):
    lib = ctx.lib
    c = rc.byte_case(38, 22, 0.5)
    r = rectification(pkg, c)
    img = np.zeros((22, 38), np.uint8)
    buf = ctx.device_malloc(38 * 22)
    try:
        src, dst = (C.c_void_p * 1)(img.ctypes.data), (C.c_void_p * 1)(buf)
        lib.sdvl_rectify.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        assert lib.sdvl_rectify(ctx.h, 1, src, 38, 0, 38, 22, None, dst, 38) == -1
        assert lib.sdvl_rectify(ctx.h, 1, src, 37, 0, 38, 22, C.byref(r), dst, 38) == -1 and b"stride" in lib.sdvl_last_error(ctx.h)
        assert lib.sdvl_rectify(ctx.h, 1, src, 38, 0, 38, 1, C.byref(r), dst, 38) == -1 and b"size" in lib.sdvl_last_error(ctx.h)
        assert lib.sdvl_rectify(ctx.h, 1, src, 4096, 0, 4096, 22, C.byref(r), dst, 4096) == -1 and b"size" in lib.sdvl_last_error(ctx.h)
        assert lib.sdvl_rectify(ctx.h, 1, dst, 38, 1, 38, 22, C.byref(r), dst, 38) == -1 and b"in-place" in lib.sdvl_last_error(ctx.h)
        bad = pkg.rectification(c["K"], c["D"], c["R"], (0.0, 100.0, 19.0, 11.0), 38, 22)
        assert lib.sdvl_rectify(ctx.h, 1, src, 38, 0, 38, 22, C.byref(bad), dst, 38) == -1 and b"focal" in lib.sdvl_last_error(ctx.h)
        bad = pkg.rectification(c["K"], c["D"], np.asarray(c["R"]) * (1 + 1e-8), c["rect"], 38, 22)
        assert lib.sdvl_rectify(ctx.h, 1, src, 38, 0, 38, 22, C.byref(bad), dst, 38) == -1 and b"rotation" in lib.sdvl_last_error(ctx.h)
        bad = pkg.rectification(c["K"], c["D"], np.full((3, 3), np.nan), c["rect"], 38, 22)
        assert lib.sdvl_rectify(ctx.h, 1, src, 38, 0, 38, 22, C.byref(bad), dst, 38) == -1 and b"finite" in lib.sdvl_last_error(ctx.h)
        assert lib.sdvl_rectify(ctx.h, 0, None, 38, 0, 38, 22, C.byref(r), None, 38) == 0
    finally:
        ctx.device_free(buf)


# ---- composition: plan -> rectify -> sdvl_stereo_depth, beside the ideal pair rendered directly
def stereo_figures(ctx, pkg, orc, left_img, right_img, depth, rect, baseline):
    import stereo_cases as stc
    h, w = left_img.shape
    xyl = stc.filtered_corners(orc, left_img)
    left = ctx.frame(np.array(left_img), pyramid=False)
    try:
        z, disp, status, ok = ctx.stereo_depth([(left, np.array(right_img), 0, len(xyl))], xyl, pkg.Camera(w, h, *rect), baseline)
    finally:
        left.close()
    return rc.disparity_figures(status, disp, xyl, depth, rect[0], baseline), (status, disp)


@pytest.mark.parametrize("k", rc.COMPOSITION_FRAMES)
def test_composition_with_the_stereo_matcher(ctx, pkg, orc, k):
    """`shelf` through the tum rig (raw pairs through config_tum_f1.cfg's lens, the right camera turned): the library's plan, both images
    rectified on the device, the matcher at the oracle's filtered corners of the rectified left image.  The yardstick is the ideal pair
    rendered directly at R1 T_cw with the rectified camera; the bound is the ideal pair's figures loosened by rectify_cases' margins,
    which were measured on the host (test_rectify_restatement_cpu.py), not here"""
    g, p, v = rc.rigs()["tum"], rc.planned("tum"), rc.shelf_rig_pair(orc, k)
    out = pkg.stereo_rectify_plan(g["K1"], g["D1"], g["K2"], g["D2"], g["R"], g["T"], g["w"], g["h"])
    rect, baseline = out.camera(), out.baseline
    assert np.abs(rect - np.array(p["rect"])).max() <= 1e-12
    left = ctx.rectify([np.array(v["raw_left"])], out.left)[0]
    right = ctx.rectify([np.array(v["raw_right"])], out.right)[0]
    ref = rc.composition_reference(orc, k)
    assert np.array_equal(left, ref["left"]) and np.array_equal(right, ref["right"])
    rectified, _ = stereo_figures(ctx, pkg, orc, left, right, v["depth"], rect, baseline)
    ideal, _ = stereo_figures(ctx, pkg, orc, v["ideal_left"], v["ideal_right"], v["depth"], rect, baseline)
    print("frame %d: rectified pair OK %.4f median %.4f px; ideal pair OK %.4f median %.4f px" % ((k,) + rectified + ideal))
    rc.assert_composition(rectified, ideal)


# ---- the closed loop, mirroring test_gpu_stereo_map_loop.py: two trackers, 40 raw pairs of `shelf`, a deliberately wrong plane
import json
import os
import subprocess

import scene_cases as sc
from oraclelib import quat_to_R, trajectory_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, W, H = 2, sc.N_FRAMES, sc.W, sc.H
FB = W * H
WRONG_PLANE = (0, 0, 1, 5.0)
SIGMA = 0.3


@pytest.fixture(scope="module")
def trk():
    importlib.import_module("slam-sdvl_amd")
    return importlib.import_module("slam-sdvl_amd.tracker")


def tum_rig():
    g = rc.rigs()["tum"]
    return (g["K1"], g["D1"], g["K2"], g["D2"], g["R"], g["T"])


class RenderedRigPairs:
    """N pairs of B trackers in HBM, rendered on the device: the raw left and right images of the tum rig and the ideal pair"""

    def __init__(self, ctx, orc):
        ss = sc.scene_synth()
        views = {name: [] for name in ("raw_left", "raw_right", "ideal_left", "ideal_right")}
        for i in range(B):
            for k in range(N):
                for name, (T, cam, dist) in rc.rig_views(trajectory_pose(orc, k, sc.tracker_twist(i))).items():
                    views[name].append(ss.scene(T, cam=cam, preset="shelf", seed=sc.SEED + i, frame_id=k, dist=dist))
        self.ctx = ctx
        self.buf = {name: ctx.device_malloc(B * N * FB) for name in views}
        for name, scenes in views.items():
            ctx.synth_render_scene(scenes, W, H, self.buf[name])
        ctx.synchronize()

    def ptrs(self, name, k):
        return [self.buf[name] + (i * N + k) * FB for i in range(B)]

    def close(self):
        for p in self.buf.values():
            self.ctx.device_free(p)


@pytest.fixture(scope="module")
def rig_pairs(ctx, orc):
    r = RenderedRigPairs(ctx, orc)
    yield r
    r.close()


def make_batch(trk, cam, n=B, mapper=True):
    trk.configure()
    trk.set_mapper(mapper)
    try:
        dev = trk.HostDevice(0)
        return dev, trk.TrackerBatch(dev, n, W, H, cam, plane4=WRONG_PLANE, host_threads=1)
    finally:
        trk.set_mapper(False)


def launch_counter(dev):
    lib = importlib.import_module("slam-sdvl_amd").load_library()
    ctx = dev.ctx_handle()
    assert lib.sdvl_ctx_timing_enable(C.c_void_p(ctx), 1) == 0

    def launches(name):
        nm = ((C.c_char * 32) * 64)()
        ms = (C.c_double * 64)()
        la = (C.c_int64 * 64)()
        cnt = C.c_int()
        assert lib.sdvl_ctx_timing_get(C.c_void_p(ctx), 64, nm, ms, la, C.byref(cnt)) == 0
        return {nm[i].value.decode(): la[i] for i in range(cnt.value)}.get(name, 0)
    return launches


_loop_runs = {}


def loop_run(trk, rig_pairs, pairs, mapping, mapper=True):
    """the batch over the N pairs, once per process.  pairs: "raw" (set_stereo_rectification, the rig's raw images) or "ideal" (the
    ideal pairs of the rectified camera: the yardstick); mapping: set_stereo_mapping on or not; mapper: the reference's mapper or the plane map"""
    key = (pairs, mapping, mapper)
    if key not in _loop_runs:
        p = rc.planned("tum")
        dev, batch = make_batch(trk, np.array(p["rect"]), mapper=mapper)
        try:
            batch.set_stereo(p["baseline"])
            if pairs == "raw":
                cam, baseline = batch.set_stereo_rectification(tum_rig())
                assert np.array_equal(cam, np.array(p["rect"])) and baseline == p["baseline"]
            if mapping:
                batch.set_stereo_mapping(disparity_sigma=SIGMA)
            launches = launch_counter(dev)
            left, right = ("raw_left", "raw_right") if pairs == "raw" else ("ideal_left", "ideal_right")
            out = dict(states=[], poses=[], remaps=[])
            for k in range(N):
                before = launches("undistort")
                st = batch.step_device(rig_pairs.ptrs(left, k), right_ptrs=rig_pairs.ptrs(right, k))
                out["remaps"].append(launches("undistort") - before)
                out["states"].append([(st[i].state, st[i].quality, st[i].keyframe) for i in range(B)])
                out["poses"].append([np.array(st[i].pose[:]) for i in range(B)])
            out["points"] = [batch.map_points(i) for i in range(B)] if mapper else None
            out["stats"] = [batch.stereo_stats(i) for i in range(B)]
            _loop_runs[key] = out
        finally:
            batch.close()
            dev.close()
    return _loop_runs[key]


def raw_left_pose(T, R1):
    """a pose the tracker reports — the rectified left camera's, in the world the first rectified camera spans — taken back to the raw
    left camera and the raw left camera's world with R1^T: R = R1^T R_est R1, t = R1^T t_est"""
    return R1.T @ quat_to_R(np.asarray(T[:4])) @ R1, R1.T @ np.asarray(T[4:7])


def worst_centre_error(run, orc, R1):
    worst = 0.0
    for i in range(B):
        for k in range(N):
            R, t = raw_left_pose(run["poses"][k][i], R1)
            truth = trajectory_pose(orc, k, sc.tracker_twist(i))
            c_true = -quat_to_R(np.asarray(truth[:4])).T @ np.asarray(truth[4:7])
            worst = max(worst, float(np.linalg.norm(-R.T @ t - c_true)))
    return worst


@pytest.mark.parametrize("mapping", [True, False])
def test_closed_loop_on_raw_pairs(trk, orc, rig_pairs, mapping):
    R1 = rc.planned("tum")["R1"]
    raw, ideal = loop_run(trk, rig_pairs, "raw", mapping), loop_run(trk, rig_pairs, "ideal", mapping)
    scene = sc.shelf_scene(orc)
    for i in range(B):
        assert raw["states"][0][i] == (0, 0, 1), raw["states"][0][i]
        for k in range(1, N):
            assert raw["states"][k][i][:2] == (2, 0), (i, k, raw["states"][k][i])          # every frame is tracked
        pts = raw["points"][i].copy()
        pts[:, :3] = pts[:, :3] @ R1                                                        # X_world = R1^T X (rows: X^T R1)
        rep = sc.geometry_report(scene, pts)
        print("tracker %d, stereo mapping %s: %d points %s" % (i, mapping, len(pts), rep))
        sc.assert_geometry(rep)
    e_raw, e_ideal = worst_centre_error(raw, orc, R1), worst_centre_error(ideal, orc, R1)
    print("stereo mapping %s: worst camera-centre error over %d frames: raw pairs rectified on the device %.4g m, ideal pairs %.4g m" % (mapping, N, e_raw, e_ideal))
    assert e_raw <= 2.0 * e_ideal, (e_raw, e_ideal)
    # the remap launches of a step: the left images always (one launch for the batch); the right images in one more launch, and only in a
    # step that reads them — with stereo mapping the steps whose mapper update works on the step's frame, without it the bootstrap alone
    # (the mapper's later keyframes are monocular)
    assert ideal["remaps"] == [0] * N
    print("remap launches per step:", raw["remaps"])
    if mapping:
        assert raw["remaps"][0] == 2 and set(raw["remaps"]) <= {1, 2} and raw["remaps"].count(2) > N // 2, raw["remaps"]
    else:
        assert raw["remaps"] == [2] + [1] * (N - 1), raw["remaps"]


def test_right_images_are_rectified_only_in_steps_that_seed_a_keyframe(trk, rig_pairs):
    """the plane map: every keyframe is seeded from the pair.  A step without a keyframe issues the left images' remap alone"""
    run = loop_run(trk, rig_pairs, "raw", False, mapper=False)
    kf_steps = [any(s[2] for s in row) for row in run["states"]]
    assert kf_steps[0] and any(kf_steps[1:]) and not all(kf_steps), kf_steps
    assert run["remaps"] == [2 if kf else 1 for kf in kf_steps], (run["remaps"], kf_steps)
    assert all(row[i][:2] == (2, 0) for row in run["states"][1:] for i in range(B))
    assert all(run["stats"][i]["keyframes"] == sum(row[i][2] for row in run["states"]) and run["stats"][i]["no_image"] == 0 for i in range(B))


def test_every_combination_that_throws(trk):
    p = rc.planned("tum")
    rect = np.array(p["rect"])
    g = rc.rigs()["tum"]
    cases = [
        # (camera, mapper, what comes first, what must then raise, a word of the message)
        (rect, False, lambda b: None, lambda b: b.set_stereo_rectification(tum_rig()), "stereo seeding"),
        (rect, False, lambda b: (b.set_stereo(p["baseline"]), b.set_distortion(g["D1"])), lambda b: b.set_stereo_rectification(tum_rig()), "lens of its own"),
        (np.array(g["K1"]), False, lambda b: b.set_stereo(p["baseline"]), lambda b: b.set_stereo_rectification(tum_rig()), "intrinsics or size"),
        (rect + np.array([0, 0, 1e-9, 0]), False, lambda b: b.set_stereo(p["baseline"]), lambda b: b.set_stereo_rectification(tum_rig()), "intrinsics or size"),
        (rect, False, lambda b: b.set_stereo(0.11), lambda b: b.set_stereo_rectification(tum_rig()), "baseline"),
        (rect, False, lambda b: b.set_stereo(p["baseline"] * (1 + 1e-11)), lambda b: b.set_stereo_rectification(tum_rig()), "baseline"),
        (rect, False, lambda b: b.set_stereo(p["baseline"]),
         lambda b: b.set_stereo_rectification((g["K1"], g["D1"], g["K2"], g["D2"], g["R"], (0.11, 0.0, 0.0))), "swap the cameras"),
    ]
    for n, (cam, mapper, first, then, word) in enumerate(cases):
        dev, batch = make_batch(trk, cam, n=1, mapper=mapper)
        try:
            first(batch)
            with pytest.raises(RuntimeError, match=word):
                then(batch)
        except BaseException:
            print("case %d" % n)
            raise
        finally:
            batch.close()
            dev.close()
    # what the switch leaves alone: planning on any batch, on, off, on again, and stereo seeding off behind it
    dev, batch = make_batch(trk, rect, n=1)
    try:
        cam, baseline = batch.set_stereo_rectification(tum_rig(), plan_only=True)
        assert np.array_equal(cam, rect) and baseline == p["baseline"]
        batch.set_stereo(baseline)
        batch.set_stereo_rectification(tum_rig())
        batch.set_stereo_rectification(on=False)
        batch.set_stereo_rectification(tum_rig())
        batch.set_stereo_mapping(disparity_sigma=SIGMA)
        batch.set_stereo_mapping(on=False)
        batch.set_stereo(baseline, on=False)
    finally:
        batch.close()
        dev.close()
    # the mapper thread can only be started from C++
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "rectify_check")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rectify_check: 0 failed" in r.stdout, r.stdout + r.stderr


def test_track_sequence_with_a_rig(tmp_path):
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    assert os.path.exists(exe), "build() makes it (make -C slam-sdvl_amd/host)"
    g = rc.rigs()["tum"]
    rig = tmp_path / "rig.cfg"
    lines = ["%YAML:1.0", "# the right camera and the rig"]
    lines += ["Camera.%s: %r" % (k, float(v)) for k, v in zip(("fx", "fy", "u0", "v0"), g["K2"])]
    lines += ["Camera.d%d: %r" % (i + 1, float(v)) for i, v in enumerate(g["D2"])]
    lines += ["Rig.r%d%d: %r" % (r + 1, c + 1, float(g["R"][r, c])) for r in range(3) for c in range(3)]
    lines += ["Rig.t%s: %r" % (a, float(v)) for a, v in zip("xyz", g["T"])]
    rig.write_text("\n".join(lines) + "\n")
    n = 12
    r = subprocess.run([exe, "--synthetic", str(n), "--scene", "shelf", "--stereo", "--rig", str(rig), "--dist"] + [repr(float(d)) for d in g["D1"]] + ["--json"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out_lines = r.stdout.strip().splitlines()
    rows = [l.split() for l in out_lines[:-1]]
    assert len(rows) == n and all([int(v) for v in row[1:3]] == [2, 0] for row in rows[1:]), rows
    assert json.loads(out_lines[-1])["tracked"] == n - 1
    p = rc.planned("tum")
    assert "rectified camera: fx %.6f" % p["rect"][0] in r.stderr and "stereo seeding:" in r.stderr, r.stderr
    # without the rig the lens is refused, and the message names the switch
    r = subprocess.run([exe, "--synthetic", "2", "--scene", "shelf", "--stereo", "--baseline", "0.11", "--dist"] + [repr(float(d)) for d in g["D1"]],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--rig" in r.stderr
