"""csrc/sdvl_depth_filter.h, the one statement of the depth filter's arithmetic for the device kernels and the host mapper, checked
without a GPU: tests/depth_filter_math_check.cc is built with the host compiler (-O2 -ffp-contract=off, as the host layer is) and fed
every case of tests/depth_cases.py and tests/depth_measure_cases.py in one run each.

The plain cases are held to what tests/test_gpu_depth_filter.py holds the kernel to: depth_cases.differences against
depth_restatement.tolerance, outcomes and n_failed exact.  A measured case takes the lookup's status and sample from
tests/depth_lookup_restatement.py (the lookup is not this header's business) and is held to depth_measure_cases.differences, as
tests/test_gpu_depth_measure.py holds the measured kernel.  No bound of this file's own."""
import os
import shutil
import subprocess

import pytest

import depth_cases as dc
import depth_lookup_restatement as dl
import depth_measure_cases as mc
import depth_measure_restatement as dmr
from depth_restatement import CONVERGED, FIXED_STALE, UPDATED

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "slam-sdvl_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the host compiler that builds libsdvl_host.so is missing"
    exe = str(tmp_path_factory.mktemp("depth_filter_math") / "depth_filter_math_check")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(HERE, "depth_filter_math_check.cc"), "-o", exe])
    return exe


def line_of(c, measured=False, z_c=0.0, noise_abs=0.0, noise_quad=0.0):
    st, cam, p = c["state"], c.get("cam", dc.CAM), c["params"]
    v = list(c["cur_pose"]) + list(c["ref_pose"]) + list(c["bearing"]) + [1.0 if c["found"] else 0.0] + list(c["px"])
    v += [st[k] for k in ("rho", "sigma2", "a", "b", "z_range", "cos_alpha", "last_distance", "depth_mean")] + list(st["position"]) + [st["fixed"], st["n_failed"]]
    v += [cam[k] for k in ("width", "height", "fx", "fy", "u0", "v0")] + [p[k] for k in ("px_error_angle", "min_depth", "scale_min_dist", "max_failed")]
    v += [1.0 if measured else 0.0, z_c, noise_abs, noise_quad]
    return " ".join(float(x).hex() for x in v)


def run(program, lines):
    out = subprocess.run([program], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [r.split() for r in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def as_result(row, **more):
    """a line of the program's output in the restatement's form, as tests/test_gpu_depth_filter.py makes it of a DepthOut"""
    outcome, n_failed = int(row[0]), int(row[1])
    rho, sigma2, a, b, cos_alpha, last_distance, px, py, pz = (float.fromhex(t) for t in row[2:])
    told = outcome in (UPDATED, CONVERGED, FIXED_STALE)
    return dict(outcome=outcome, n_failed=n_failed, rho=rho, sigma2=sigma2, a=a, b=b, cos_alpha=cos_alpha if told else None,
                last_distance=last_distance if told else None, position=(px, py, pz) if told else None, row={}, **more)


def test_plain_cases(program):
    cases = dc.all_cases()
    rows = run(program, [line_of(c) for c in cases])
    for c, row in zip(cases, rows):
        bad, _ = dc.differences(c, as_result(row), with_row=False)
        assert not bad, (c["name"], c["purpose"], bad)


def test_measured_cases(program):
    cases = mc.all_cases()
    lines, statuses = [], []
    for c in cases:
        status, z = dmr.NO_LOOKUP, 0.0
        if c["found"] and c["depth"] is not None:
            zs, ss, _ = dl.depth_lookup([(c["depth"], 0, 1, c["scale"])], [c["px"]], [c["level"]], c["cam"], c["dist"], **c["rule"])
            status, z = int(ss[0]), float(zs[0])
        statuses.append(status)
        lines.append(line_of(c, status == dl.OK, z, **dmr.noise(c["noise_abs"], c["noise_quad"])))
    assert statuses.count(dl.OK) >= 20 and len(set(statuses)) == 6             # every status, and most cases measure
    rows = run(program, lines)
    for c, row, status in zip(cases, rows, statuses):
        bad, _ = mc.differences(c, as_result(row, status=status), with_row=False)
        assert not bad, (c["name"], c["purpose"], bad)
