"""Stereo rectification without a GPU: the plan's restatement (tests/rectify_restatement.py) against closed-form geometry, the map's
restatement against the code that exists (the oracle's cv::undistort), and the host plan in C++ (csrc/rectify_plan.cc, through the
library and compiled on its own as host/rectify_plan_check) against the restatement."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import oraclelib as ol
import rectify_cases as rc
import rectify_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slam-sdvl_amd", "host")
RIGS = ("euroc", "tum", "ideal", "roll5")


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


# ---- the plan
@pytest.mark.parametrize("name", RIGS)
def test_plan_rotations_are_orthonormal_and_rows_and_disparities_are_those_of_an_ideal_rig(name):
    g, p = rc.rigs()[name], rc.planned(name)
    for Ri in (p["R1"], p["R2"]):
        assert np.abs(Ri.T @ Ri - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Ri) - 1) <= 1e-12
    f, fy, u0, v0 = p["rect"]
    assert f == fy
    rng = np.random.default_rng(1)
    P = np.stack([rng.uniform(-1, 1, 1000), rng.uniform(-.7, .7, 1000), rng.uniform(1, 5, 1000)])
    a = p["R1"] @ P
    b = p["R2"] @ (g["R"] @ P + g["T"][:, None])
    assert a[2].min() > 0 and b[2].min() > 0                      # in front of both cameras
    rows = np.abs((f * a[1] / a[2] + v0) - (f * b[1] / b[2] + v0)).max()
    disp = np.abs((f * a[0] / a[2] - f * b[0] / b[2]) - f * p["baseline"] / a[2]).max()
    print("%s: f %.6f u0 %.6f v0 %.6f B %.6f rows %.3g px disparity %.3g px" % (name, f, u0, v0, p["baseline"], rows, disp))
    assert rows <= 1e-9 and disp <= 1e-9
    assert p["baseline"] == pytest.approx(np.linalg.norm(g["T"]), abs=1e-15)


@pytest.mark.parametrize("name", RIGS)
def test_plan_leaves_no_pixel_of_either_map_with_a_tap_outside(name):
    g, p = rc.rigs()[name], rc.planned(name)
    for K, D, Ri in rc.sides(g, p):
        iu, iv = rr.map_fixed(K, D, Ri, p["rect"], g["w"], g["h"])
        assert rr.no_source(iu, iv, g["w"], g["h"]) == 0
        assert iu.min() >= 32 and iv.min() >= 32 and iu.max() <= 32 * (g["w"] - 2) and iv.max() <= 32 * (g["h"] - 2)   # a pixel to spare


def test_plan_of_the_ideal_rig_is_the_identity():
    p = rc.planned("ideal")
    assert np.array_equal(p["R1"], np.eye(3)) and np.array_equal(p["R2"], np.eye(3))
    assert p["baseline"] == 0.11


def refused(code, **change):
    g = dict(rc.rigs()["tum"])
    override = change.pop("override", None)
    g.update(change)
    with pytest.raises(rr.Refused) as e:
        rc.plan_of(g, override)
    assert e.value.code == code
    return g, override


REFUSALS = {
    "T_zero": (rr.PLAN_T, dict(T=np.zeros(3))),
    "T_nan": (rr.PLAN_T, dict(T=np.array([-0.11, math.nan, 0.0]))),
    "T_inf": (rr.PLAN_T, dict(T=np.array([-math.inf, 0.0, 0.0]))),
    "vertical": (rr.PLAN_VERTICAL, dict(T=np.array([-0.01, -0.11, 0.0]))),
    "order": (rr.PLAN_ORDER, dict(T=np.array([0.11, 0.0, 0.0]))),
    "R_scaled": (rr.PLAN_R, dict(R=np.eye(3) * (1 + 1e-8))),
    "R_sheared": (rr.PLAN_R, dict(R=np.array([[1, 1e-8, 0], [0, 1, 0], [0, 0, 1.0]]))),
    "R_nan": (rr.PLAN_R, dict(R=np.full((3, 3), math.nan))),
    "R_backwards": (rr.PLAN_R, dict(R=np.diag([-1.0, 1.0, -1.0]))),
    "w_small": (rr.PLAN_SIZE, dict(w=1)),
    "h_small": (rr.PLAN_SIZE, dict(h=1)),
    "w_large": (rr.PLAN_SIZE, dict(w=4096)),
    "h_large": (rr.PLAN_SIZE, dict(h=4096)),
    "empty": (rr.PLAN_EMPTY, dict(K2=np.array([517.3, 516.5, 318.6 + 4000.0, 255.3]))),   # the right camera looks past the left one's view
    "forward": (rr.PLAN_EMPTY, dict(R=np.eye(3), T=np.array([0.0, 0.0, 0.11]))),         # one camera behind the other: a quarter turn
    "focal": (rr.PLAN_INTRINSICS, dict(K1=np.array([0.0, 516.5, 318.6, 255.3]))),
    "override_focal": (rr.PLAN_INTRINSICS, dict(override=(500.0, -1.0, 320.0, 240.0))),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_plan_refusals(name, sdvl):
    """every refusal, in the restatement and in the library with the same code and a message"""
    code, change = REFUSALS[name]
    g, override = refused(code, **dict(change))
    with pytest.raises(sdvl.RectifyPlanError) as e:
        sdvl.stereo_rectify_plan(g["K1"], g["D1"], g["K2"], g["D2"], g["R"], g["T"], g["w"], g["h"], override)
    assert e.value.code == code and "sdvl_stereo_rectify_plan" in str(e.value) and "unknown" not in str(e.value)


def test_plan_is_refused_for_a_null_rig(sdvl):
    lib = sdvl.load_library()
    assert lib.sdvl_stereo_rectify_plan(None, 640, 480, None, None) == rr.PLAN_NULL


def test_barely_acceptable_rotation_is_accepted():
    g = dict(rc.rigs()["tum"])
    g["R"] = g["R"] * (1 + 1e-10)          # R^T R - I = 2e-10
    rc.plan_of(g)


def test_override_sets_the_intrinsics_and_keeps_the_rotations():
    g, p = rc.rigs()["tum"], rc.planned("tum")
    q = rc.plan_of(g, override=(400.0, 410.0, 300.0, 250.0))
    assert q["rect"] == (400.0, 410.0, 300.0, 250.0)
    assert np.array_equal(q["R1"], p["R1"]) and np.array_equal(q["R2"], p["R2"])
    iu, iv = rr.map_fixed(g["K1"], g["D1"], q["R1"], q["rect"], g["w"], g["h"])
    assert rr.no_source(iu, iv, g["w"], g["h"]) > 0                 # a wider view than the raw image holds


# ---- the host plan in C++ against the restatement
def plan_values(p):
    return np.concatenate([p["R1"].ravel(), p["R2"].ravel(), p["rect"], [p["baseline"]]])


def library_plan_values(out):
    c = out.left.rect
    assert bytes(out.left.rect) == bytes(out.right.rect)
    return np.array(list(out.left.R) + list(out.right.R) + [c.fx, c.fy, c.u0, c.v0, out.baseline])


PLAN_CASES = [(n, None) for n in RIGS] + [("tum", (400.0, 410.0, 300.0, 250.0)), ("euroc", (458.654, 457.296, 367.215, 248.375))]


@pytest.mark.parametrize("name,override", PLAN_CASES)
def test_library_plan_agrees_with_the_restatement(name, override, sdvl):
    g = rc.rigs()[name]
    want = plan_values(rc.plan_of(g, override))
    out = sdvl.stereo_rectify_plan(g["K1"], g["D1"], g["K2"], g["D2"], g["R"], g["T"], g["w"], g["h"], override)
    got = library_plan_values(out)
    print(name, "worst difference", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(out.camera(), got[18:22])
    assert list(out.left.dist.d) == list(g["D1"]) and list(out.right.dist.d) == list(g["D2"])
    assert (out.left.raw.fx, out.left.raw.v0, out.right.raw.fy, out.right.raw.u0) == (g["K1"][0], g["K1"][3], g["K2"][1], g["K2"][2])
    assert (out.left.rect.width, out.left.rect.height) == (g["w"], g["h"])


@pytest.fixture(scope="module")
def plan_check():
    subprocess.run(["make", "-s", "-C", HOST, "rectify_plan_check"], check=True)
    return os.path.join(HOST, "rectify_plan_check")


def run_plan_check(exe, g, override):
    nums = list(g["K1"]) + list(g["D1"]) + list(g["K2"]) + list(g["D2"]) + list(np.asarray(g["R"]).ravel()) + list(g["T"]) + [g["w"], g["h"]]
    nums += list(override) if override is not None else []
    out = subprocess.run([exe] + [repr(float(v)) for v in nums], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.split("\n")


@pytest.mark.parametrize("name,override", PLAN_CASES)
def test_standalone_plan_program_agrees_with_the_restatement(name, override, plan_check):
    """csrc/rectify_plan.cc compiled by the host compiler alone, with nothing of the device layer"""
    g = rc.rigs()[name]
    want = plan_values(rc.plan_of(g, override))
    lines = run_plan_check(plan_check, g, override)
    got = np.array([float(v) for v in lines[:23]])
    assert np.abs(got - want).max() <= 1e-12


def test_standalone_plan_program_refuses_and_needs_no_project_library(plan_check):
    g = dict(rc.rigs()["tum"], T=np.array([0.11, 0.0, 0.0]))
    lines = run_plan_check(plan_check, g, None)
    assert lines[0] == "refused %d" % rr.PLAN_ORDER and "swap the cameras" in lines[1]
    needed = subprocess.run(["ldd", plan_check], capture_output=True, text=True, timeout=60).stdout
    assert "sdvl" not in needed and "amdhip" not in needed


# ---- the map against the code that exists
CAMERAS = {"tum_f1": (ol.TUM_CAM, ol.TUM_DIST, 640, 480), "euroc": (ol.EUROC_CAM, ol.EUROC_DIST, 752, 480)}


@pytest.fixture(scope="module")
def orc():
    return ol.Oracle()


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_map_with_identity_rotation_and_the_raw_camera_is_undistortion(name, orc):
    """R_i = I and a rectified camera equal to the raw K: the map is cv::undistort's, except where 32 u or 32 v lies within 1e-6 of a
    half-integer — the two evaluation orders (direct, and the library's accumulation along the row) differ by about 1e-12, so elsewhere
    they round alike.  The library's order is restated from the device code's tables; that restatement reproduces the oracle's
    cv::undistort byte for byte, which ties it to the code that exists."""
    K, D, w, h = CAMERAS[name]
    lib_iu, lib_iv = rr.undistort_fixed(K, D, w, h)
    img = np.array(rc.raw_image(w, h, 20261201))
    assert np.array_equal(rr.remap(img, lib_iu, lib_iv), orc.undistort(img, K, D))
    iu, iv = rr.map_fixed(K, D, np.eye(3), K, w, h)
    differ = (iu != lib_iu) | (iv != lib_iv)
    # where the restatement itself sits within 1e-6 of a rounding boundary: recomputed in the map's own arithmetic
    M = rr.rays_matrix(np.eye(3), K)
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y, ww = (M[r][0] * j + M[r][1] * i + M[r][2] for r in range(3))
    xd, yd = rr.distort(x / ww, y / ww, D)
    u32, v32 = (K[0] * xd + K[2]) * 32, (K[1] * yd + K[3]) * 32
    near = (np.abs(u32 - np.floor(u32) - 0.5) <= 1e-6) | (np.abs(v32 - np.floor(v32) - 0.5) <= 1e-6)
    print("%s: %d pixels differ, %d near a half-integer, of %d" % (name, differ.sum(), near.sum(), w * h))
    assert not np.any(differ & ~near)
    assert near.sum() <= 0.001 * w * h
    assert np.abs(iu.astype(np.int64) - lib_iu).max() <= 1 and np.abs(iv.astype(np.int64) - lib_iv).max() <= 1


def test_rays_that_do_not_point_forward_have_no_source():
    """a turn of 80 degrees about y: where w = M (j, i, 1)_z <= 0 the entry is "outside" (sx = sy = -2, fractions 0), and counted"""
    c = rc.turned_away_case()
    w, h = c["w"], c["h"]
    M = rr.rays_matrix(c["R"], c["rect"])
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    behind = ~(M[2][0] * j + M[2][1] * i + M[2][2] > 0)
    assert 0 < behind.sum() < w * h
    assert (c["iu"][behind] == -64).all() and (c["iv"][behind] == -64).all()
    assert (rr.words(c["iu"], c["iv"], w, h)[behind] == 0).all()
    assert c["no_source"] >= behind.sum()
    assert not rr.remap(np.full((h, w), 255, np.uint8), c["iu"], c["iv"])[behind].any()


def test_words_narrow_and_wide_carry_the_same_entries():
    c = rc.byte_case(38, 22, 6.0, zoom=0.8)
    wd = rr.words(c["iu"], c["iv"], 38, 22)
    sx, sy, a, b = rr.positions(c["iu"], c["iv"])
    assert wd.dtype == np.uint32 and wd.shape == (22, 38)
    assert np.array_equal(wd & 31, a) and np.array_equal((wd >> 5) & 31, b)
    assert np.array_equal(((wd >> 10) & 2047).astype(np.int32) - 2, np.clip(sx, -2, 38)) and np.array_equal((wd >> 21).astype(np.int32) - 2, np.clip(sy, -2, 22))
    c = rc.byte_case(2048, 10, 0.5)
    wd = rr.words(c["iu"], c["iv"], 2048, 10)
    sx, sy, a, b = rr.positions(c["iu"], c["iv"])
    assert wd.shape == (10, 2048, 2)
    assert np.array_equal((wd[..., 1] & 0xFFFF).astype(np.int32) - 2, np.clip(sx, -2, 2048)) and np.array_equal(wd[..., 0], a | b << 5)


def test_remap_of_an_identity_map_is_the_image_and_outside_reads_zero():
    img = np.array(rc.raw_image(38, 22, 5))
    j, i = np.meshgrid(np.arange(38, dtype=np.int32), np.arange(22, dtype=np.int32))
    assert np.array_equal(rr.remap(img, j * 32, i * 32), img)
    half = rr.remap(img, j * 32 + 16, i * 32)                       # half a pixel to the right: the mean of two neighbours, rounded half up
    want = (img[:, :-1].astype(np.int32) + img[:, 1:] + 1) >> 1
    assert np.array_equal(half[:, :-1], want) and np.array_equal(half[:, -1], (img[:, -1].astype(np.int32) + 1) >> 1)
    assert not rr.remap(img, j * 32 + 32 * 38, i * 32).any()
    assert rr.no_source(j * 32, i * 32, 38, 22) == 38 + 22 - 1       # the last row and column: their right / lower taps lie outside


def test_struct_sizes_match_the_header(sdvl, tmp_path):
    """the new structures, field for field, against a program that includes include/sdvl_hip.h"""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx
    structs = {"sdvl_stereo_rig": sdvl.StereoRig, "sdvl_rectification": sdvl.Rectification, "sdvl_stereo_rectified": sdvl.StereoRectified}
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "sdvl_hip.h"', 'int main() {']
    for c_name, cls in structs.items():
        src.append('  printf("%s %%zu", sizeof(%s));' % (c_name, c_name))
        for field in cls._fields_:
            src.append('  printf(" %s:%%zu", offsetof(%s, %s));' % (field[0], c_name, field[0]))
        src.append('  printf("\\n");')
    src += ['  return 0;', '}']
    path = tmp_path / "rectify_abi.cc"
    path.write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "rectify_abi")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(path), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    for line, (c_name, cls) in zip(out, structs.items()):
        words = line.split()
        assert words[0] == c_name and int(words[1]) == C.sizeof(cls), line
        assert words[2:] == ["%s:%d" % (f[0], getattr(cls, f[0]).offset) for f in cls._fields_], line
    assert C.sizeof(sdvl.Rectification) == 48 + 40 + 72 + 48 and C.sizeof(sdvl.StereoRig) == 2 * 88 + 96
    assert C.sizeof(sdvl.StereoRectified) == 2 * 208 + 8


# ---- the composition's margin, measured without the device
@pytest.mark.parametrize("k", rc.COMPOSITION_FRAMES)
def test_composition_margin_on_the_host(k, orc):
    """`shelf` through the tum rig, host-rendered: plan, rectify (restatement), the matcher's restatement at the oracle's filtered corners of
    the rectified left image, beside the ideal pair rendered directly with the rectified camera.  The figures rectify_cases' margins
    come from: frame 0 OK 0.8717 / 0.0621 px (ideal 0.8647 / 0.0680 px), frame 26 OK 0.8588 / 0.0586 px (ideal 0.8731 / 0.0638 px)"""
    ref = rc.composition_reference(orc, k)
    print("frame %d: rectified OK %.4f median %.4f px; ideal OK %.4f median %.4f px" % ((k,) + ref["rectified"] + ref["ideal"]))
    assert ref["ideal"][0] >= 0.8 and ref["ideal"][1] <= 0.1          # the yardstick itself is a working pair
    assert ref["ideal"][0] - ref["rectified"][0] <= rc.SHARE_MARGIN / 2      # the deficit the margin doubles
    assert ref["rectified"][1] - ref["ideal"][1] <= 0.0
    rc.assert_composition(ref["rectified"], ref["ideal"])
