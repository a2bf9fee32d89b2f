"""sdvl_stereo_depth on the MI355X (kernel stereo_depth, slam-sdvl_amd/csrc/sdvl_stereo.hip) against its specification, the numpy
restatement tests/stereo_restatement.py: statuses equal, disparities and depths bit-equal (the costs are integers; the tail is the same
float64 operations in the same order, built without contraction).  The entry returns no d0 of its own: for an OK corner it is
ceil(disparity - 0.5), compared with the restatement's; for the others the status is what the rule leaves of it.
160 x 120 pairs with corners of levels 0 - 3 at every border and at X - 4 s in {1, 2, 3}; searched ranges of 3, 63, 64, 65, 128, 129 and
512 disparities (the lane rounds and the cap); equal costs; max_depth; 0 and 1 corners; an empty job and a corner no job names; the right
image in HBM, pinned, pageable and with padded rows; two jobs of different pairs in one call; a `shelf` pair at 640 x 480; every refusal
of the entry point, and the sizes of the two new structures."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import stereo_cases as stc
import stereo_restatement as sr
from oraclelib import TUM_CAM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def camera(pkg, cam4, w, h):
    return pkg.Camera(w, h, *[float(c) for c in cam4])


def check(got, want):
    """got: the entry's (z, disparity, status, ok); want: the restatement's dict"""
    z, disp, status, ok = got
    bad = np.flatnonzero(status != want["status"])
    assert len(bad) == 0, (bad[:10], status[bad[:10]], want["status"][bad[:10]])
    assert np.array_equal(disp.view(np.uint64), want["disparity"].view(np.uint64)), np.abs(disp - want["disparity"]).max()
    assert np.array_equal(z.view(np.uint64), want["z"].view(np.uint64)), np.abs(z - want["z"]).max()
    good = status == sr.OK
    assert np.array_equal(sr.d0_of(disp[good]), want["d0"][good])
    assert int(ok.sum()) == int(good.sum())


def run_case(pkg, ctx, c):
    h, w = c["left"].shape
    left = ctx.frame(np.array(c["left"]), pyramid=False)
    right = np.array(c["right"])    # (a writable, pageable copy)
    return ctx.stereo_depth([(left, right, 0, len(c["xyl"]))], c["xyl"], camera(pkg, c["cam"], w, h), c["baseline"], **c["rule"])


@pytest.mark.parametrize("name", ["integer", "noise", "half", "constant", "constant1", "periodic", "outside", "edge", "dlo", "dlo_miss", "end0",
                                  "end1", "end2"])
def test_designed_cases(pkg, ctx, name):
    c = stc.designed_cases()[name]
    got = run_case(pkg, ctx, c)
    if c["want"] is not None:
        assert np.array_equal(got[2], c["want"]), (got[2], c["want"])
    check(got, stc.restate(c))
    assert ctx.lib.sdvl_ctx_health(ctx.h) == 0


@pytest.mark.parametrize("n_range", stc.RANGES)
def test_lane_rounds(pkg, ctx, n_range):
    """exactly n_range disparities searched: one lane short of a round, a full round, one lane into the next, and the cap of 8 rounds"""
    c = stc.range_case(n_range)
    want = stc.restate(c)
    check(run_case(pkg, ctx, c), want)
    if n_range > 3:
        assert (want["status"] == sr.OK).sum() >= 6


def test_no_corner_and_one(pkg, ctx):
    c = stc.designed_cases()["noise"]
    h, w = c["left"].shape
    left, right, cam = ctx.frame(np.array(c["left"]), pyramid=False), np.array(c["right"]), camera(pkg, c["cam"], w, h)
    z, disp, status, ok = ctx.stereo_depth([(left, right, 0, 0)], np.zeros((0, 3), np.int32), cam, c["baseline"])
    assert len(z) == 0 and len(disp) == 0 and len(status) == 0 and list(ok) == [0]
    one = c["xyl"][17:18]
    check(ctx.stereo_depth([(left, right, 0, 1)], one, cam, c["baseline"]), sr.stereo_depth(c["left"], c["right"], one, c["cam"], c["baseline"]))


def test_jobs_of_two_pairs_an_empty_one_and_unnamed_corners(pkg, ctx):
    """three jobs over two different pairs in ONE call, one of them empty; the corners no job names come back NOMATCH"""
    a, b = stc.designed_cases()["noise"], stc.designed_cases()["integer"]
    h, w = a["left"].shape
    na, nb = 40, 30
    xyl = np.concatenate([a["xyl"][:na], b["xyl"][:2], b["xyl"][:nb], a["xyl"][:1]])
    fa, fb_ = ctx.frame(np.array(a["left"]), pyramid=False), ctx.frame(np.array(b["left"]), pyramid=False)
    ra, rb = np.array(a["right"]), np.array(b["right"])
    jobs = [(fa, ra, 0, na), (fb_, rb, na + 2, na + 2), (fb_, rb, na + 2, na + 2 + nb)]
    z, disp, status, ok = ctx.stereo_depth(jobs, xyl, camera(pkg, TUM_CAM, w, h), stc.BASELINE)
    wz, wd, ws, wok = sr.stereo_jobs([(a["left"], a["right"], 0, na), (b["left"], b["right"], na + 2, na + 2),
                                      (b["left"], b["right"], na + 2, na + 2 + nb)], xyl, TUM_CAM, stc.BASELINE)
    assert np.array_equal(status, ws) and list(status[na:na + 2]) == [sr.NOMATCH] * 2 and status[-1] == sr.NOMATCH
    assert np.array_equal(z.view(np.uint64), wz.view(np.uint64)) and np.array_equal(disp.view(np.uint64), wd.view(np.uint64))
    assert list(ok) == list(wok) == [na, 0, nb]


def test_right_image_sources_give_the_same_bytes(pkg, ctx, orc):
    """one `shelf` pair at 640 x 480 with the oracle's filtered corners against the restatement, its right image in HBM, in pinned and
    in pageable host memory, dense and with rows 24 bytes longer than the image: six calls, one answer"""
    import torch
    c, _ = stc.shelf_pair(orc, 13)
    want = stc.restate(c)
    assert (want["status"] == sr.OK).sum() >= 150
    h, w = c["left"].shape
    left, cam, n = ctx.frame(np.array(c["left"]), pyramid=False), camera(pkg, c["cam"], w, h), len(c["xyl"])
    first = None
    for pitch in (w, w + 24):
        padded = np.full((h, pitch), 0xA5, np.uint8)
        padded[:, :w] = c["right"]
        for where in ("hbm", "pinned", "pageable"):
            keep = None
            if where == "hbm":
                keep = torch.from_numpy(padded).cuda()
                ptr = keep.data_ptr()
            elif where == "pinned":
                keep = torch.from_numpy(padded).pin_memory()
                ptr = keep.data_ptr()
            else:
                ptr = padded.ctypes.data
            got = ctx.stereo_depth([pkg.StereoJob(left.h, ptr, 1 if where == "hbm" else 0, pitch, 0, n)], c["xyl"], cam, c["baseline"])
            check(got, want)
            if first is None:
                first = got
            for x, y in zip(got, first):
                assert x.tobytes() == y.tobytes(), (pitch, where)
            assert ctx.lib.sdvl_ctx_health(ctx.h) == 0
            del keep
    # between sdvl_depth_stage_begin and _end an image staged once is not staged again, and the answer is the same
    ctx.lib.sdvl_depth_stage_begin(ctx.h)
    right = np.array(c["right"])
    for _ in range(2):
        check(ctx.stereo_depth([(left, right, 0, n)], c["xyl"], cam, c["baseline"]), want)
    ctx.lib.sdvl_depth_stage_end(ctx.h)


def test_depth_entries_refuse_a_right_image(pkg, ctx):
    """the right image travels in the depth image's slot: the entries that read depths refuse its format with a message"""
    w, h = 64, 48
    img = np.zeros((h, w), np.uint8)
    job = pkg.DepthJob(img.ctypes.data, 0, w, pkg.SDVL_DEPTH_RIGHT8, 0, 1.0, 0, 1)
    with pytest.raises(pkg.SdvlError, match="SDVL_DEPTH_RIGHT8"):
        ctx.depth_seed([job], w, h, np.array([[10, 10, 0]], np.int32), camera(pkg, TUM_CAM, w, h))
    with pytest.raises(pkg.SdvlError, match="SDVL_DEPTH_RIGHT8"):
        ctx.depth_lookup([job], w, h, np.array([[10.0, 10.0]]), [0], camera(pkg, TUM_CAM, w, h))
    assert ctx.lib.sdvl_ctx_health(ctx.h) == 0


def test_refusals(pkg, ctx):
    """every refusal returns SDVL_ERR_INVALID with a message and leaves the context healthy"""
    lib = ctx.lib
    w, h = stc.W, stc.H
    limg = stc.ramp()
    rimg = np.array(stc.shifted(limg, 7))
    left = ctx.frame(np.array(limg), pyramid=False)
    other = pkg.Context(0)
    foreign = other.frame(np.array(limg), pyramid=False)
    xyl = np.array([[80, 60, 0], [40, 30, 1]], np.int32)
    cam = camera(pkg, TUM_CAM, w, h)
    z, disp, status, ok = np.zeros(2), np.zeros(2), np.zeros(2, np.uint8), np.zeros(2, np.int32)
    lib.sdvl_stereo_depth.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    lens = pkg.Distortion((C.c_double * 5)(0.1, 0, 0, 0, 0))
    nolens = pkg.Distortion((C.c_double * 5)(0.0, 0.3, 0, 0, 0))

    def call(job=None, rule=None, null=None, corners_=xyl, n_jobs=1, second=None):
        j = dict(left=left.h, right=rimg.ctypes.data, on_device=0, stride=w, c_begin=0, c_end=2)
        j.update(job or {})
        jobs = (pkg.StereoJob * 2)(pkg.StereoJob(**j), pkg.StereoJob(**dict(j, **(second or {}))))
        r = dict(baseline=0.11)
        r.update(rule or {})
        p = pkg.StereoParams(**r)
        args = dict(jobs=C.addressof(jobs), xyl=corners_.ctypes.data, cam=C.addressof(cam), p=C.addressof(p), z=z.ctypes.data, disp=disp.ctypes.data,
                    status=status.ctypes.data, ok=ok.ctypes.data)
        if null:
            args[null] = None
        rc = lib.sdvl_stereo_depth(ctx.h, n_jobs, args["jobs"], len(corners_), args["xyl"], args["cam"], args["p"], args["z"], args["disp"],
                                   args["status"], args["ok"])
        return rc, lib.sdvl_last_error(ctx.h).decode()

    assert call()[0] == 0 and list(status) == [0, 0] and list(disp) == [7.0, 7.0]
    assert call(rule=dict(dist=C.addressof(nolens)))[0] == 0      # d[0] == 0: no lens
    refused = [dict(null="jobs"), dict(null="xyl"), dict(null="cam"), dict(null="p"), dict(null="z"), dict(null="disp"), dict(null="status"),
               dict(null="ok"), dict(job=dict(left=None)), dict(job=dict(right=None)),
               dict(rule=dict(baseline=0.0)), dict(rule=dict(baseline=-0.11)), dict(rule=dict(baseline=float("nan"))),
               dict(rule=dict(baseline=float("inf"))),
               dict(rule=dict(max_disparity=512)), dict(rule=dict(max_disparity=-1)),
               dict(rule=dict(uniqueness=101)), dict(rule=dict(uniqueness=-1)),
               dict(rule=dict(max_sad=256)), dict(rule=dict(max_sad=-1)),
               dict(rule=dict(min_depth=-0.1)), dict(rule=dict(max_depth=float("nan"))),
               dict(job=dict(stride=w - 1)),
               dict(corners_=np.array([[10, 10, 5]], np.int32), job=dict(c_end=1)), dict(corners_=np.array([[10, 10, -1]], np.int32), job=dict(c_end=1)),
               dict(job=dict(c_begin=2, c_end=1)), dict(job=dict(c_end=3)), dict(job=dict(c_begin=-1)),
               dict(n_jobs=2, job=dict(c_end=2), second=dict(c_begin=1, c_end=2)),      # overlapping ranges
               dict(job=dict(left=foreign.h)),
               dict(rule=dict(dist=C.addressof(lens)))]
    for kw in refused:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("sdvl_stereo_depth:"), (kw, rc, msg)
        assert lib.sdvl_ctx_health(ctx.h) == 0
    # nothing to do
    assert call(n_jobs=0)[0] == 0 and call(corners_=np.zeros((0, 3), np.int32), job=dict(c_end=0))[0] == 0
    # and the context still computes
    z[:], disp[:] = 0.0, 0.0
    assert call()[0] == 0 and list(status) == [0, 0] and list(disp) == [7.0, 7.0] and list(z) == [TUM_CAM[0] * 0.11 / 7.0] * 2
    other.close()


def test_struct_sizes_match_the_compiled_header(pkg, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx
    names = {"sdvl_stereo_job": pkg.StereoJob, "sdvl_stereo_params": pkg.StereoParams}
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "sdvl_hip.h"', 'int main() {']
    for c_name, cls in names.items():
        src.append('  printf("%s %%zu", sizeof(%s));' % (c_name, c_name))
        for field in cls._fields_:
            src.append('  printf(" %s:%%zu", offsetof(%s, %s));' % (field[0], c_name, field[0]))
        src.append('  printf("\\n");')
    src += ['  return 0;', '}']
    path = tmp_path / "stereo_abi.cc"
    path.write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "stereo_abi")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(path), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    for line, (c_name, cls) in zip(out, names.items()):
        words = line.split()
        assert words[0] == c_name and int(words[1]) == C.sizeof(cls), line
        assert words[2:] == ["%s:%d" % (f[0], getattr(cls, f[0]).offset) for f in cls._fields_], line
    assert C.sizeof(pkg.StereoJob) == 32 and C.sizeof(pkg.StereoParams) == 48
    assert (pkg.STEREO_OK, pkg.STEREO_NOMATCH, pkg.STEREO_AMBIGUOUS, pkg.STEREO_EDGE, pkg.STEREO_OUTSIDE) == (sr.OK, sr.NOMATCH, sr.AMBIGUOUS, sr.EDGE,
                                                                                                           sr.OUTSIDE)
