"""CPU checks of the two-frame initialisation's specification (tests/klt_restatement.py, tests/homography_restatement.py) on the
scenes of tests/init_cases.py, and of the new records of the C-ABI.  Nothing here needs a GPU.

What was measured with the restatements when the bounds below were written (float64 unless said otherwise):
  scene A  279 of 284 points kept (5 leave the image), all 271 interior points within 0.5 px of the truth (median 0.059, p90 0.104 px);
           H fit 279 of 279; pose: rotation 0.0092 deg, translation direction 0.047 deg off; visibility scores 279 against 200
  scene B  261 kept, all 252 interior points within 0.5 px (median 0.16, p90 0.27 px);
           pose: rotation 0.0079 deg, translation direction 0.056 deg off; visibility scores 261 against 183
  float32 against float64 run of the KLT restatement: status equal everywhere, largest position gap g = 8.35e-4 px on A and
  4.9e-4 px on B (init_cases.G_F32 = 8.4e-4; the device is held to max(4 g, 0.01 px) = 0.01 px).
  |C2 - C1| against map_scale |t_true| / median true depth: 0.04096 against 0.04153 on A (1.37 % low), 0.1205 against 0.1235 on B
  (2.43 % low; the median of the triangulated depths is taken in frame 2, which has moved): asserted within 4 x that, 5.5 % and 9.7 %."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import init_cases as ic
from homography_restatement import init_from_tracks, ransac, update_num_iters, homography4, refit_dlt
from oraclelib import TUM_CAM
from pose_restatement import quat_to_rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE_GAP = {"A": 4 * 0.0137, "B": 4 * 0.0243}


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


def _init(orc, synth, name):
    key = ("init", name)
    if key not in ic._made:
        f0, ref = ic.frame0(orc, synth), ic.klt_reference(orc, synth, name)
        ok = ref["status"]
        draws = ic.draws_table(int(ok.sum()), 2000, 1)
        ic._made[key] = (init_from_tracks(f0["px"][ok], ref["xy"][ok].astype(np.float32), TUM_CAM, draws), ok)
    return ic._made[key]


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_tracks_the_truth(orc, synth, name):
    s, ref = ic.scene(orc, synth, name), ic.klt_reference(orc, synth, name)
    assert s["shift"] >= ic.MIN_AVG_SHIFT
    e = np.linalg.norm(ref["xy"] - s["truth"], axis=1)
    m = s["interior"]
    good = (ref["status"] & (e <= 0.5))[m]
    print(name, "kept", int(ref["status"].sum()), "interior", int(m.sum()), "within 0.5 px", int(good.sum()), "median", float(np.median(e[m])))
    assert good.sum() >= 0.95 * m.sum()


@pytest.mark.parametrize("name", ["A", "B"])
def test_float32_run_stays_within_g(orc, synth, name):
    r64, r32 = ic.klt_reference(orc, synth, name), ic.klt_reference(orc, synth, name, dtype=np.float32)
    assert (r64["status"] == r32["status"]).all()
    both = r64["status"]
    g = float(np.abs(r64["xy"][both] - r32["xy"][both].astype(np.float64)).max())
    print(name, "g =", g)
    assert g <= ic.G_F32


@pytest.mark.parametrize("name,w,h", [("A", ic.W, ic.H), ("B", ic.W, ic.H), ("SMALL", ic.SMALL_W, ic.SMALL_H)])
@pytest.mark.parametrize("init", ["prev", "truth+3"])
def test_few_points_sit_on_a_decision(orc, synth, name, w, h, init):
    """the GPU test may except at most 2 % of the points: the scenes must stay under that"""
    ref = ic.klt_reference(orc, synth, name, init)
    ex = ic.klt_excepted(ref, w, h)
    print(name, init, "excepted", int(ex.sum()), "of", len(ex), "kept", int(ref["status"].sum()))
    assert ex.sum() <= 0.02 * len(ex)
    assert ref["status"].sum() >= 0.5 * len(ex)      # the scene tracks: a comparison on it says something


@pytest.mark.parametrize("name", ["A", "B"])
def test_chosen_pose(orc, synth, name):
    q, _ = _init(orc, synth, name)
    assert "failed" not in q, q
    s = ic.scene(orc, synth, name)
    assert q["scores"][1] / q["scores"][0] < 0.9          # the visibility test alone decides
    rot, tdir = ic.pose_errors(q["R"], q["t"], s["T"])
    print(name, "rotation", rot, "translation direction", tdir, "scores", q["scores"], "inliers", len(q["inliers"]), "n_its", q["n_its"])
    assert rot <= 0.1 and tdir <= 0.5
    assert len(q["inliers"]) >= 0.9 * q["n_h_inliers"]


@pytest.mark.parametrize("name", ["A", "B"])
def test_baseline_is_scaled_to_the_map(orc, synth, name):
    q, ok = _init(orc, synth, name)
    f0, s = ic.frame0(orc, synth), ic.scene(orc, synth, name)
    baseline = np.linalg.norm(-q["R"].T @ q["t"])
    t_true = np.linalg.norm(-quat_to_rot(s["T"][:4]).T @ s["T"][4:])
    want = 1.0 * t_true / np.median(f0["depth"][ok])
    print(name, "baseline", baseline, "expected", want)
    assert abs(baseline / want - 1.0) <= SCALE_GAP[name]


def test_budget():
    assert update_num_iters(0.995, 0.0, 4, 2000) == 0
    assert update_num_iters(0.995, 1.0, 4, 2000) == 2000
    assert update_num_iters(0.995, 0.5, 4, 2000) == int(np.rint(math.log(0.005) / math.log(1 - 0.5 ** 4))) == 82
    assert update_num_iters(0.995, 0.5, 4, 50) == 50


def test_four_point_homography_maps_its_points():
    rng = np.random.default_rng(3)
    for _ in range(20):
        s, d = rng.uniform(-1, 1, (4, 2)), rng.uniform(-1, 1, (4, 2))
        H = homography4(s, d)
        q = np.c_[s, np.ones(4)] @ H.T
        assert np.abs(q[:, :2] / q[:, 2:3] - d).max() < 1e-9


@pytest.mark.parametrize("n,share", [(4, 0.0), (5, 0.0), (64, 0.3), (65, 0.3), (300, 0.0), (300, 0.3)])
def test_ransac_restatement_finds_the_plane(n, share):
    c = ic.ransac_case(n, share, 11 + n)
    r = ransac(c["src"], c["dst"], c["draws"], c["threshold"])
    assert r["best_draw"] >= 2 or n == 4              # draw 0 repeats an index, draw 1 is collinear
    assert r["n_its"] <= 2000 and r["best_draw"] < r["n_its"]
    good = ~c["bad"]
    assert set(r["inliers"]) <= set(np.nonzero(good)[0])            # no gross outlier passes 2 px
    assert len(r["inliers"]) >= 0.8 * good.sum() or n <= 5
    if n >= 64:
        H = refit_dlt(c["src"][r["inliers"]], c["dst"][r["inliers"]])
        assert np.abs(ic.unit_h(H) - ic.unit_h(c["H"])).max() < 2e-3


def test_degenerate_draws_count_as_iterations():
    c = ic.ransac_case(65, 0.3, 5)
    r_all = ransac(c["src"], c["dst"], c["draws"], c["threshold"])
    r_cut = ransac(c["src"], c["dst"], c["draws"][:2], c["threshold"])
    assert r_cut["best_draw"] == -1 and r_cut["n_its"] == 2 and len(r_cut["inliers"]) == 0
    assert r_all["n_its"] > 2


def test_abi_of_the_new_records(sdvl):
    assert C.sizeof(sdvl.KltJob) == 8 + 8 + 4 + 4
    assert C.sizeof(sdvl.KltParams) == 4 * 4 + 8 + 8
    assert C.sizeof(sdvl.HomographyJob) == 16
    assert C.sizeof(sdvl.HomographyResult) == 72 + 16
    lib = sdvl.load_library()
    src = open(os.path.join(ROOT, "include", "sdvl_hip.h")).read()
    for name in ("sdvl_klt_track", "sdvl_homography_ransac"):
        assert hasattr(lib, name) and name in sdvl.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % name, src)
    # a null context is refused before anything touches a device
    assert lib.sdvl_klt_track(None, 0, None, 0, None, None, None, None, None) == -1
    assert lib.sdvl_homography_ransac(None, 0, None, 0, None, None, 0, None, C.c_double(0.0), 0, C.c_double(0.0), None, None) == -1


# ---- host/homography_init.cc (libsdvl_host.so) against the restatement: the same statements, Jacobi in place of LAPACK
@pytest.fixture(scope="module")
def host():
    return ic.host_library()


def test_jacobi_routines(host):
    rng = np.random.default_rng(5)
    for n in (3, 9):
        M = rng.normal(size=(n, n))
        S = M @ M.T
        A, V, eig = S.copy(), np.zeros((n, n)), np.zeros(n)
        host.sdvlh_jacobi_eigen_sym(n, A.ctypes.data, V.ctypes.data, eig.ctypes.data)
        assert np.abs(eig - np.linalg.eigvalsh(S)).max() <= 1e-12 * eig.max()
        assert np.abs(V @ np.diag(eig) @ V.T - S).max() <= 1e-12 * eig.max() and np.abs(V.T @ V - np.eye(n)).max() <= 1e-13
    for _ in range(10):
        A = np.eye(3) + 0.1 * rng.normal(size=(3, 3))
        U, s, V = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3))
        host.sdvlh_jacobi_svd3(A.ctypes.data, U.ctypes.data, s.ctypes.data, V.ctypes.data)
        assert np.abs(s - np.linalg.svd(A)[1]).max() <= 1e-13 and s[0] >= s[1] >= s[2]
        assert np.abs(U @ np.diag(s) @ V.T - A).max() <= 1e-13
        assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-12 and np.abs(V.T @ V - np.eye(3)).max() <= 1e-13


def test_host_matches_are_rounded_to_float(host, orc, synth):
    f0, ref = ic.frame0(orc, synth), ic.klt_reference(orc, synth, "A")
    ok = ref["status"]
    px1, px2 = np.ascontiguousarray(f0["px"][ok]), np.ascontiguousarray(ref["xy"][ok].astype(np.float32))
    n = len(px1)
    src, dst = np.zeros((n, 2)), np.zeros((n, 2))
    cam = np.ascontiguousarray(TUM_CAM, np.float64)
    assert host.sdvlh_homography_matches(n, px1.ctypes.data, px2.ctypes.data, cam.ctypes.data, src.ctypes.data, dst.ctypes.data) == 0
    want = ((px1.astype(np.float64) - TUM_CAM[2:]) / TUM_CAM[:2])
    assert np.array_equal(src, src.astype(np.float32).astype(np.float64))          # cv::Point2f
    assert np.abs(src - want).max() <= 1e-7 and np.abs(src - want).max() > 0


@pytest.mark.parametrize("name", ["A", "B"])
def test_host_arithmetic_equals_the_restatement(host, orc, synth, name):
    q, ok = _init(orc, synth, name)
    f0, ref = ic.frame0(orc, synth), ic.klt_reference(orc, synth, name)
    px1, px2 = f0["px"][ok], ref["xy"][ok].astype(np.float32)
    draws = ic.draws_table(int(ok.sum()), 2000, 1)
    # the RANSAC's inliers as the restatement finds them (on the device: sdvl_homography_ransac)
    from homography_restatement import ransac as rs
    n = len(px1)
    src, dst = np.zeros((n, 2)), np.zeros((n, 2))
    cam = np.ascontiguousarray(TUM_CAM, np.float64)
    host.sdvlh_homography_matches(n, np.ascontiguousarray(px1).ctypes.data, np.ascontiguousarray(px2).ctypes.data, cam.ctypes.data,
                                  src.ctypes.data, dst.ctypes.data)
    inl = rs(src, dst, draws, 2.0 / TUM_CAM[0])["inliers"]
    g = ic.host_init(host, px1, px2, TUM_CAM, inl)
    assert g["rc"] == 1
    print(name, "H gap", np.abs(ic.unit_h(g["H"]) - ic.unit_h(q["H"])).max(), "R gap", np.abs(g["R"] - q["R"]).max(), "t gap", np.abs(g["t"] - q["t"]).max())
    assert np.abs(ic.unit_h(g["H"]) - ic.unit_h(q["H"])).max() <= 1e-9
    assert g["scores"] == tuple(q["scores"]) and g["n_h_inliers"] == q["n_h_inliers"]
    assert np.array_equal(g["inliers"], q["inliers"])
    assert np.abs(g["R"] - q["R"]).max() <= 1e-8 and np.abs(g["t"] - q["t"]).max() <= 1e-8
    assert abs(g["depth_median"] / q["depth_median"] - 1) <= 1e-8 and np.abs(g["tri"] - q["tri"]).max() <= 1e-7
    rot, tdir = ic.pose_errors(g["R"], g["t"], ic.scene(orc, synth, name)["T"])
    assert rot <= 0.1 and tdir <= 0.5


def test_host_refuses_what_the_reference_refuses(host, orc, synth):
    f0, ref = ic.frame0(orc, synth), ic.klt_reference(orc, synth, "A")
    ok = ref["status"]
    px1, px2 = f0["px"][ok], ref["xy"][ok].astype(np.float32)
    everything = np.arange(len(px1), dtype=np.int32)
    assert ic.host_init(host, px1, px2, TUM_CAM, everything, min_init_corners=len(px1) + 1)["rc"] == 0      # too few inliers, :276-279
    assert ic.host_init(host, px1, px2, TUM_CAM, everything[:3])["rc"] == 0                                   # no model from three matches
    assert ic.host_init(host, px1, px2, TUM_CAM, np.array([0, 1, 2, 9999], np.int32))["rc"] == 0               # an index outside the tracks


def test_two_frame_switch_is_exported(host):
    """the public switch exists and refuses a null batch before anything touches a device"""
    host.sdvlh_batch_set_two_frame_init.argtypes = [C.c_void_p, C.c_int]
    assert host.sdvlh_batch_set_two_frame_init(None, 1) == -1
    trk = importlib.import_module("slam-sdvl_amd.tracker")
    assert callable(trk.TrackerBatch.set_two_frame_init)
    import subprocess
    exe = os.path.join(ROOT, "slam-sdvl_amd", "host", "track_sequence")
    r = subprocess.run([exe, "--synthetic", "2", "--init", "sideways"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "unknown --init" in r.stderr
