"""sdvl_depth_seed on the MI355X (kernel depth_seed, slam-sdvl_amd/csrc/sdvl_depth.hip) against its specification, the numpy restatement
tests/depth_seed_restatement.py: statuses equal, depths bit-equal (both sides convert one stored sample to double, and the centre's
arithmetic is built without contraction).  Corner counts around the launch's block of 256 and the wave of 64, several jobs over different
images in one call, 16 x 12 and 640 x 480, float and 16-bit, sources in HBM / pinned / pageable memory, padded rows, with and without a
lens, non-finite samples, levels 0 - 4; every refusal of the entry point, and the sizes of the two new structures."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_seed_cases as dc
import depth_seed_restatement as dr
from oraclelib import TUM_CAM, TUM2_CAM, TUM2_DIST

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
    z, status, ok = got
    wz, wstatus, _ = want
    assert np.array_equal(status, wstatus), (np.flatnonzero(status != wstatus)[:10], status[status != wstatus][:10], wstatus[status != wstatus][:10])
    assert np.array_equal(z.view(np.uint64), wz.view(np.uint64)), np.abs(z - wz).max()
    assert int(ok.sum()) == int((wstatus == dr.OK).sum())


def run_case(pkg, ctx, c):
    h, w = c["depth"].shape
    depth = np.array(c["depth"])   # (a writable, pageable copy)
    return ctx.depth_seed([(depth, 0, len(c["xyl"]), c["scale"])], w, h, c["xyl"], camera(pkg, c["cam"], w, h), c["dist"], **c["rule"])


@pytest.mark.parametrize("name", ["plane", "step1", "step20", "holes", "few6", "few5", "border", "range"])
def test_designed_cases(pkg, ctx, name):
    c = dc.designed_cases()[name]
    got = run_case(pkg, ctx, c)
    if c["want"] is not None:
        assert np.array_equal(got[1], c["want"])
    check(got, dc.restate(c))


def rough_image(w, h, seed, u16=False):
    """depths of 0.5 - 4 m in smooth patches with steps between them, and every kind of sample the rule names: zero, NaN, +inf, negative
    (float), zero (16-bit)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    z = 1.5 + 0.002 * xx + 0.001 * yy + 1.0 * ((xx // 37 + yy // 29) % 3)
    bad = rng.random((h, w))
    if u16:
        d = np.round(z * 5000).astype(np.uint16)
        d[bad < 0.02] = 0
        return d
    d = z.astype(np.float32)
    d[bad < 0.008] = 0.0
    d[(bad >= 0.008) & (bad < 0.016)] = np.nan
    d[(bad >= 0.016) & (bad < 0.02)] = np.inf
    d[(bad >= 0.02) & (bad < 0.024)] = -1.0
    d[(bad >= 0.024) & (bad < 0.03)] = 0.04     # below min_depth
    return d


def corners(w, h, n, seed, max_level=4):
    """n corners of levels 0 .. max_level anywhere in the image, the borders included"""
    rng = np.random.default_rng(seed)
    l = rng.integers(0, max_level + 1, n)
    x = (rng.integers(0, w, n) >> l)
    y = (rng.integers(0, h, n) >> l)
    if n >= 4:
        x[:4], y[:4], l[:4] = [0, (w - 1), 0, (w - 1)], [0, 0, (h - 1), (h - 1)], 0     # the four corners of the image
    return np.stack([x, y, l], 1).astype(np.int32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
@pytest.mark.parametrize("u16", [False, True])
def test_corner_counts(pkg, ctx, n, u16):
    w, h = 640, 480
    d = rough_image(w, h, 20261010, u16)
    scale = 1.0 / 5000 if u16 else 1.0
    xyl = corners(w, h, n, 20261011 + n)
    got = ctx.depth_seed([(d, 0, n, scale)], w, h, xyl, camera(pkg, TUM_CAM, w, h))
    want = dr.depth_seed(d, xyl, TUM_CAM, scale=scale)
    check(got, want)
    if n == 300:
        counts = np.bincount(want[1], minlength=5)
        assert counts[dr.OK] > 50 and counts[dr.HOLE] > 3 and counts[dr.EDGE] > 10 and counts[dr.FEW] > 0, counts   # the case exercises the rule
        assert set(xyl[:, 2]) == {0, 1, 2, 3, 4}


def test_small_image_all_levels(pkg, ctx):
    w, h = 16, 12
    d = rough_image(w, h, 20261020)
    xyl = np.array([(x >> l, y >> l, l) for l in range(5) for y in range(0, h, 3) for x in range(0, w, 3)], np.int32)
    check(ctx.depth_seed([(d, 0, len(xyl))], w, h, xyl, camera(pkg, TUM_CAM, w, h), min_valid=4), dr.depth_seed(d, xyl, TUM_CAM, min_valid=4))


def test_three_jobs_two_images(pkg, ctx):
    """jobs of 0, 1 and 300 corners over two different images in ONE call; a corner no job names comes back HOLE"""
    w, h = 640, 480
    a, b = rough_image(w, h, 20261030), rough_image(w, h, 20261031, u16=True)
    xyl = corners(w, h, 303, 20261032)
    got = ctx.depth_seed([(a, 0, 0), (b, 0, 1, 1.0 / 5000), (a, 1, 301)], w, h, xyl, camera(pkg, TUM_CAM, w, h))
    z, status, ok = got
    wb = dr.depth_seed(b, xyl[:1], TUM_CAM, scale=1.0 / 5000)
    wa = dr.depth_seed(a, xyl[1:301], TUM_CAM)
    assert np.array_equal(status, np.concatenate([wb[1], wa[1], [dr.HOLE, dr.HOLE]]))
    assert np.array_equal(z.view(np.uint64), np.concatenate([wb[0], wa[0], [0.0, 0.0]]).view(np.uint64))
    assert list(ok) == [0, int((wb[1] == 0).sum()), int((wa[1] == 0).sum())]


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("where", ["hbm", "pinned", "pageable"])
def test_sources_and_padded_rows(pkg, ctx, where, u16):
    """the same image in HBM, in pinned and in pageable host memory, its rows 24 bytes longer than its samples"""
    import torch
    w, h = 640, 480
    d = rough_image(w, h, 20261040, u16)
    bps = d.itemsize
    pitch = w * bps + 24
    padded = np.full((h, pitch), 0xA5, np.uint8)
    padded[:, :w * bps] = d.view(np.uint8).reshape(h, w * bps)
    keep = None
    if where == "hbm":
        keep = torch.from_numpy(padded).cuda()
        ptr = keep.data_ptr()
    elif where == "pinned":
        keep = torch.from_numpy(padded).pin_memory()
        ptr = keep.data_ptr()
    else:
        ptr = padded.ctypes.data
    scale = 1.0 / 5000 if u16 else 1.0
    xyl = corners(w, h, 300, 20261041)
    job = pkg.DepthJob(ptr, 1 if where == "hbm" else 0, pitch, 1 if u16 else 0, 0, scale, 0, 300)
    got = ctx.depth_seed([job], w, h, xyl, camera(pkg, TUM_CAM, w, h))
    check(got, dr.depth_seed(d, xyl, TUM_CAM, scale=scale))
    assert ctx.lib.sdvl_ctx_health(ctx.h) == 0
    del keep


def test_lens(pkg, ctx, orc):
    """`shelf` through the lens of config_tum_f2.cfg: the centre is the raw pixel of the corner's ray, ties included"""
    c, _ = dc.lens_case(orc)
    want = dc.restate(c)
    assert (want[1] == dr.OK).sum() >= 150
    check(run_case(pkg, ctx, c), want)
    # a lens that throws rays off the image: OUTSIDE, and nothing is read out of bounds
    w, h = 640, 480
    d = rough_image(w, h, 20261050)
    xyl = corners(w, h, 300, 20261051)
    strong = np.array([0.9, 2.5, 0.01, -0.02, 4.0])
    want = dr.depth_seed(d, xyl, TUM2_CAM, strong)
    assert (want[1] == dr.OUTSIDE).sum() > 5
    check(ctx.depth_seed([(d, 0, 300)], w, h, xyl, camera(pkg, TUM2_CAM, w, h), strong), want)
    # d[0] == 0: no lens, whatever the other coefficients say
    nolens = np.array([0.0, 2.5, 0.01, -0.02, 4.0])
    check(ctx.depth_seed([(d, 0, 300)], w, h, xyl, camera(pkg, TUM2_CAM, w, h), nolens), dr.depth_seed(d, xyl, TUM2_CAM, None))


@pytest.mark.parametrize("i,k", [(0, 0), (1, 39)])
def test_shelf_frames(pkg, ctx, orc, i, k):
    c = dc.shelf_case(orc, i, k)
    check(run_case(pkg, ctx, c), dc.restate(c))


def test_refusals(pkg, ctx):
    """every refusal returns SDVL_ERR_INVALID with a message and leaves the context healthy"""
    lib = ctx.lib
    w, h = 64, 48
    d = np.full((h, w), 1.0, np.float32)
    xyl = np.array([[10, 10, 0], [5, 5, 1]], np.int32)
    cam = camera(pkg, TUM_CAM, w, h)
    z, status, ok = np.zeros(2), np.zeros(2, np.uint8), np.zeros(1, np.int32)
    lib.sdvl_depth_seed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]

    def call(job=None, rule=None, null=None, corners_=xyl, n_jobs=1):
        j = dict(depth=d.ctypes.data, on_device=0, stride=w * 4, format=0, pad_=0, scale=1.0, c_begin=0, c_end=2)
        j.update(job or {})
        jobs = (pkg.DepthJob * 1)(pkg.DepthJob(**j))
        p = pkg.DepthSeedParams(**(rule or {}))
        args = dict(jobs=C.addressof(jobs), xyl=corners_.ctypes.data, cam=C.addressof(cam), z=z.ctypes.data, status=status.ctypes.data,
                    ok=ok.ctypes.data)
        if null:
            args[null] = None
        rc = lib.sdvl_depth_seed(ctx.h, n_jobs, args["jobs"], w, h, len(corners_), args["xyl"], args["cam"], None, C.addressof(p), args["z"],
                                 args["status"], args["ok"])
        return rc, lib.sdvl_last_error(ctx.h).decode()

    assert call()[0] == 0 and list(status) == [0, 0]
    refused = [dict(null="jobs"), dict(null="xyl"), dict(null="cam"), dict(null="z"), dict(null="status"), dict(null="ok"),
               dict(job=dict(depth=None)),
               dict(job=dict(format=2)), dict(job=dict(format=-1)),
               dict(job=dict(stride=w * 4 - 1)), dict(job=dict(format=1, stride=w * 2 - 1)),
               dict(job=dict(format=1, stride=w * 2, scale=0.0)), dict(job=dict(format=1, stride=w * 2, scale=-1.0)),
               dict(rule=dict(edge_ratio=-0.01)), dict(rule=dict(min_valid=10)), dict(rule=dict(min_valid=-1)),
               dict(job=dict(c_begin=2, c_end=1)), dict(job=dict(c_end=3)), dict(job=dict(c_begin=-1)),
               dict(corners_=np.array([[10, 10, 8]], np.int32), job=dict(c_end=1)), dict(corners_=np.array([[10, 10, -1]], np.int32), job=dict(c_end=1))]
    for kw in refused:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("sdvl_depth_seed:"), (kw, rc, msg)
        assert lib.sdvl_ctx_health(ctx.h) == 0
    # nothing to do
    assert call(n_jobs=0)[0] == 0 and call(corners_=np.zeros((0, 3), np.int32), job=dict(c_end=0))[0] == 0
    # and the context still computes
    assert call()[0] == 0 and list(status) == [0, 0] and list(z) == [1.0, 1.0]


def test_struct_sizes_match_the_compiled_header(pkg, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx
    names = {"sdvl_depth_job": pkg.DepthJob, "sdvl_depth_seed_params": pkg.DepthSeedParams}
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "sdvl_hip.h"', 'int main() {']
    for c_name, cls in names.items():
        src.append('  printf("%s %%zu", sizeof(%s));' % (c_name, c_name))
        for field in cls._fields_:
            src.append('  printf(" %s:%%zu", offsetof(%s, %s));' % (field[0], c_name, field[0]))
        src.append('  printf("\\n");')
    src += ['  return 0;', '}']
    path = tmp_path / "depth_abi.cc"
    path.write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "depth_abi")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(path), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    for line, (c_name, cls) in zip(out, names.items()):
        words = line.split()
        assert words[0] == c_name and int(words[1]) == C.sizeof(cls), line
        assert words[2:] == ["%s:%d" % (f[0], getattr(cls, f[0]).offset) for f in cls._fields_], line
    assert C.sizeof(pkg.DepthJob) == 40 and C.sizeof(pkg.DepthSeedParams) == 32
    assert (pkg.SDVL_DEPTH_F32, pkg.SDVL_DEPTH_U16) == (0, 1)
