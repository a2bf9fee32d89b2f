"""sdvl_depth_lookup on the device against tests/depth_lookup_restatement.py on the images and positions of tests/depth_lookup_cases.py:
a float and a 16-bit image with a hole, a step edge and the border; positions at .0 and .5, levels 0 .. 2, with and without a lens, and
positions in no job.  Statuses are equal; z is equal bit for bit (a sample is read, not computed)."""
import importlib

import numpy as np
import pytest

import depth_lookup_cases as lc
import depth_lookup_restatement as dl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


def camera(sdvl):
    return sdvl.Camera(lc.CAM["width"], lc.CAM["height"], lc.CAM["fx"], lc.CAM["fy"], lc.CAM["u0"], lc.CAM["v0"])


@pytest.mark.parametrize("dist", [None, lc.LENS], ids=["pinhole", "lens"])
def test_lookup_equals_the_restatement(sdvl, ctx, dist):
    f, u = lc.images()
    px, lv = lc.positions()
    n = len(px)
    # both images in one call: the float image serves the first part, the 16-bit image the second; the last two positions are in no job
    px2, lv2 = np.concatenate([px[:-2], px]), np.concatenate([lv[:-2], lv])
    jobs = [(f, 0, n - 2), (u, n - 2, 2 * n - 4, lc.U16_SCALE)]
    z, st, ok = ctx.depth_lookup(jobs, lc.W, lc.H, px2, lv2, camera(sdvl), dist)
    zr, sr, okr = dl.depth_lookup(jobs, px2, lv2, lc.CAM, dist)
    print("statuses %s, ok per job %s" % (np.bincount(st, minlength=5), ok))
    assert np.array_equal(st, sr)
    assert z.tobytes() == zr.tobytes()
    assert np.array_equal(ok, okr)
    assert set(st) == {dl.OK, dl.HOLE, dl.FEW, dl.EDGE, dl.OUTSIDE}
    assert list(st[-2:]) == [dl.HOLE, dl.HOLE] and not z[-2:].any()


def test_rule_fields_and_refusals(sdvl, ctx):
    f, _ = lc.images()
    px, lv = lc.positions()
    jobs = [(f, 0, len(px))]
    for rule in (dict(min_valid=9), dict(edge_ratio=0.6), dict(max_depth=2.5), dict(min_depth=2.02)):
        z, st, ok = ctx.depth_lookup(jobs, lc.W, lc.H, px, lv, camera(sdvl), None, **rule)
        zr, sr, okr = dl.depth_lookup(jobs, px, lv, lc.CAM, None, **rule)
        assert np.array_equal(st, sr) and z.tobytes() == zr.tobytes() and np.array_equal(ok, okr), rule
    with pytest.raises(sdvl.SdvlError, match="level"):
        ctx.depth_lookup(jobs, lc.W, lc.H, px, np.full(len(px), 99, np.int32), camera(sdvl))
    with pytest.raises(sdvl.SdvlError, match="range"):
        ctx.depth_lookup([(f, 0, len(px) + 1)], lc.W, lc.H, px, lv, camera(sdvl))
    with pytest.raises(sdvl.SdvlError, match="min_valid"):
        ctx.depth_lookup(jobs, lc.W, lc.H, px, lv, camera(sdvl), None, min_valid=10)
    z, st, ok = ctx.depth_lookup([], lc.W, lc.H, px, lv, camera(sdvl))
    assert not z.any() and len(ok) == 0
