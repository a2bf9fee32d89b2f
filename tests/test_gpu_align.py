"""sdvl_image_align against the CPU oracle on the named cases of tests/align_cases.py: reference keyframes away from the world frame,
a tilted plane, features leaving the current image at a level's first evaluation and later, a far start, every level range, both
branches of a fast call, nothing measured, the sticky stop, a NaN system, flat images, depth edges and points on the current
camera plane, and frames whose level widths are no multiples of 4 — the inputs on which tests/test_oracle_align_independent.py
holds the oracle itself against an independent restatement and shows that each planted fault is separated.

Forms: each case alone (one wave per job); every group of cases that shares its limits, camera and frame size as one batch with an
empty job between them; the 385 to 450-feature variants (four waves per job); a batch of both kinds; three cases through the align
store.  Tolerance classes: multi-iteration cases as tests/test_gpu_parity.py holds the alignment (pose within POSE_TOL, its within
+-1 per level, error by its rule) with n_meas, stop and the fast / stop branch exact; one-evaluation cases n_meas, its and stop
exact, the pose within ONE_EVAL_BOUND and chi2 within the rounding of the oracle's float running sum; the cases whose pose must not
move: bit-equal to the start.  Run with -s, the tests print each distance and the largest of each class."""
import importlib

import numpy as np
import pytest

from align_cases import BIG_CASES, CASES, MULTI_CASES, ONE_EVAL_CASES, case, frames, oracle_answer
from pose_restatement import se3_matrix
from test_gpu_forms import K_LDS_MAX_F, align_timed, result_fields
from test_gpu_parity import POSE_TOL
from test_oracle_align_independent import ONE_EVAL_BOUND

pytestmark = pytest.mark.gpu

UNMOVED = {"nothing-measured": 1e10, "band-no-level4": 1e10, "nan-depth0": 1e10, "flat-reference": 0.0}   # case -> its exact `error`
STORED = ["ref-roll30", "far-start", "ref-tilt25"]
MIXED = ["ref-roll30", "ref-tilt25", "leaving", "nothing-measured"]      # default limits, one camera: small and big variant of each
_largest = {"pose, multi-iteration": 0.0, "pose, one evaluation": 0.0, "chi2 (relative), one evaluation": 0.0}


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(sdvl, ctx, synth):
    """the device side of the cases: every view uploaded once, feature records, the result of each case run alone (shared)"""
    d = _Device(sdvl, ctx, synth)
    yield d
    for _, f in d.uploaded.values():
        f.close()


class _Device:
    def __init__(self, sdvl, ctx, synth):
        self.sdvl, self.ctx, self.synth = sdvl, ctx, synth
        self.uploaded, self.alone_, self.forms_ = {}, {}, {}

    def frame_pair(self, c):
        out = []
        for img in frames(self.synth, c):
            if id(img) not in self.uploaded:
                self.uploaded[id(img)] = (img, self.ctx.frame(img, levels=5 if min(img.shape) >= 256 else 4))
            out.append(self.uploaded[id(img)][1])
        return out

    def records(self, feats_list):
        """one AlignFeature array of several feature sets -> (array, offsets)"""
        n = sum(len(f["px"]) for f in feats_list)
        arr = (self.sdvl.AlignFeature * max(n, 1))()
        offs, i = [], 0
        for f in feats_list:
            offs.append(i)
            for k in range(len(f["px"])):
                a = arr[i]
                a.px, a.py = f["px"][k]
                a.fx, a.fy, a.fz = f["bearing"][k]
                a.depth = f["depth"][k]
                a.valid = int(f["valid"][k])
                i += 1
        return arr, offs

    def params(self, c):
        L = c["limits"]
        return self.sdvl.AlignParams(max_level=L["max_level"], min_level=L["min_level"], max_its=L["max_its"], patch_size=4, fast=int(c["fast"]))

    def camera(self, c):
        return self.sdvl.Camera(c["size"][0], c["size"][1], *c["cam"])

    def alone(self, name, big=False):
        if (name, big) not in self.alone_:
            c = case(name)
            f = c["feats_big"] if big else c["feats"]
            arr, _ = self.records([f])
            ref, cur = self.frame_pair(c)
            res, forms = align_timed(self.ctx, [(ref, cur, 0, len(f["px"]), c["start"])], arr, self.camera(c), self.params(c))
            self.alone_[(name, big)], self.forms_[(name, big)] = res[0], forms
        return self.alone_[(name, big)]


_wanted = {}


def wanted(orc, synth, name, big=False):
    if (name, big) not in _wanted:
        _wanted[(name, big)] = oracle_answer(orc, synth, case(name), big=big)
    return _wanted[(name, big)]


def pose_distance(r, want):
    return float(np.abs(se3_matrix(np.array(r.T[:])) - se3_matrix(want["T"])).max())


def assert_matches(name, big, r, want):
    c = case(name)
    got_T, its = np.array(r.T[:]), np.array(r.its[:])
    d = pose_distance(r, want)
    print("%s%s: n %d, its %s / %s, stop %d, error %.3e / %.3e, chi2 %.6g / %.6g, pose %.1e from the oracle's"
          % (name, "+" if big else "", r.n_meas, its[:5].tolist(), want["its"][:5].tolist(), r.stop, r.error, want["error"], r.chi2, want["chi2"], d))
    assert r.n_meas == want["n"], (r.n_meas, want["n"])
    assert r.stop == want["stop"], (r.stop, want["stop"])
    assert (r.error == 1e10) == (want["error"] == 1e10), (r.error, want["error"])           # the fast / stop branch
    if c["one_eval"]:
        assert np.array_equal(its, want["its"]), (its, want["its"])
        assert r.iters_run == want["evals"] == 1
        assert d <= ONE_EVAL_BOUND, d
        rel = abs(r.chi2 - want["chi2"]) / want["chi2"] if want["chi2"] else abs(r.chi2)
        # the oracle's float running sum over 16 n_meas terms (image_align.cc:192); the kernel sums the same terms in double
        assert rel <= 16 * want["n"] * 2.0 ** -24, (r.chi2, want["chi2"])
        _largest["pose, one evaluation"] = max(_largest["pose, one evaluation"], d)
        _largest["chi2 (relative), one evaluation"] = max(_largest["chi2 (relative), one evaluation"], rel)
    else:
        assert np.abs(got_T - want["T"]).max() <= POSE_TOL, (got_T, want["T"])
        assert np.abs(its - want["its"]).max() <= 1, (its, want["its"])                      # +-1 GN step near convergence is allowed
        assert abs(r.error - want["error"]) <= 1e-4 * max(1.0, abs(want["error"])) or (r.error >= 1e9 and want["error"] >= 1e9)
        _largest["pose, multi-iteration"] = max(_largest["pose, multi-iteration"], d)
    if name in UNMOVED:
        assert tuple(r.T) == tuple(c["start"]) and np.array_equal(want["T"], c["start"])    # bit for bit
        assert r.error == UNMOVED[name] == want["error"]
        assert np.array_equal(its, want["its"])


@pytest.mark.parametrize("name", list(CASES))
def test_each_case_alone(dev, orc, synth, name):
    r = dev.alone(name)
    assert dev.forms_[(name, False)] == {"image_align"} and case(name)["n"] <= K_LDS_MAX_F
    assert_matches(name, False, r, wanted(orc, synth, name))


@pytest.mark.parametrize("name", BIG_CASES)
def test_big_variants_run_the_four_wave_form(dev, orc, synth, name):
    r = dev.alone(name, big=True)
    assert dev.forms_[(name, True)] == {"image_align_big"} and 385 <= case(name)["big"] <= 450
    assert_matches(name, True, r, wanted(orc, synth, name, big=True))


def batch_groups():
    """the one-wave cases grouped by what a call shares: limits, fast, camera, frame size"""
    groups = {}
    for name in CASES:
        c = case(name)
        key = (tuple(sorted(c["limits"].items())), c["fast"], tuple(c["cam"]), c["size"])
        groups.setdefault(key, []).append(name)
    return [g for g in groups.values() if len(g) > 1]


def run_batch(dev, members):
    """members: (name, big) -> each job with its own start pose and frame pair, an empty job after every one"""
    cs = [case(n) for n, _ in members]
    arr, offs = dev.records([c["feats_big"] if b else c["feats"] for c, (_, b) in zip(cs, members)])
    jobs = []
    for c, (_, b), o in zip(cs, members, offs):
        ref, cur = dev.frame_pair(c)
        n = len((c["feats_big"] if b else c["feats"])["px"])
        jobs += [(ref, cur, o, o + n, c["start"]), (ref, cur, o + n // 2, o + n // 2, c["start"])]
    res, forms = align_timed(dev.ctx, jobs, arr, dev.camera(cs[0]), dev.params(cs[0]))
    for k, (name, b) in enumerate(members):
        assert result_fields(res[2 * k]) == result_fields(dev.alone(name, b)), (name, b)
        empty = res[2 * k + 1]
        assert tuple(empty.T) == tuple(cs[k]["start"]) and empty.n_meas == 0 and not any(empty.its)
    return forms


def test_cases_that_share_their_limits_as_one_batch(dev):
    """every result bit-identical to the job alone, as test_image_align_mixed_batch_equals_each_job_alone holds"""
    groups = batch_groups()
    in_a_batch = {n for g in groups for n in g}
    print("batches: %s" % groups)
    assert len(groups) >= 3 and len(in_a_batch) >= 15 and max(len(g) for g in groups) >= 8
    for g in groups:
        assert run_batch(dev, [(n, False) for n in g]) == {"image_align"}


def test_small_and_big_jobs_in_one_batch(dev):
    members = [m for n in MIXED for m in ((n, False), (n, True))]
    assert all(case(n)["big"] and case(n)["limits"] == case(MIXED[0])["limits"] for n in MIXED)
    assert run_batch(dev, members) == {"image_align", "image_align_big"}


def test_through_the_align_store(dev, sdvl, ctx):
    """sdvl_align_store_write + sdvl_image_align_begin_stored + _end on three cases away from the identity: bit-identical to the
    plain call"""
    base = 700
    for name in STORED:
        c = case(name)
        assert np.abs(se3_matrix(c["start"]) - np.eye(4)).max() > 0.005 and np.abs(se3_matrix(c["T_ref"]) - np.eye(4)).max() > 0.4
        arr, _ = dev.records([c["feats"]])
        n = len(c["feats"]["px"])
        store = sdvl.AlignStore(ctx, base + n + 16)
        try:
            store.write(base, arr, 0, n // 3)
            store.write(base + n // 3, arr, n // 3, n)
            ref, cur = dev.frame_pair(c)
            got = ctx.image_align_stored([(ref, cur, base, base + n, c["start"])], store, dev.camera(c), dev.params(c))[0]
            assert result_fields(got) == result_fields(dev.alone(name)), name
        finally:
            store.close()


def test_every_case_was_compared_and_the_largest_distances(dev):
    """(last in the module) the largest device-to-oracle distances of each class, for DESIGN.md"""
    for name in CASES:
        dev.alone(name)
    assert set(MULTI_CASES) | set(ONE_EVAL_CASES) == set(CASES) and len(dev.alone_) >= len(CASES)
    print("largest device-to-oracle distances: %s" % {k: "%.2e" % v for k, v in _largest.items()})
