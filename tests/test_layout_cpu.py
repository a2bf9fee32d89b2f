"""csrc/sdvl_layout.h, the one statement of how the launch code cuts its buffers into 256-byte aligned parts, checked on its own
(no GPU, nothing loaded into Python): tests/layout_check.cc is built with the host compiler under AddressSanitizer and UBSan and run."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "slam-sdvl_amd", "csrc")


def test_layout_offsets_alignment_and_no_overlap_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the host compiler that builds libsdvl_synth.so is missing"
    exe = str(tmp_path / "layout_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing depends on library order
                           "-I", CSRC, os.path.join(HERE, "layout_check.cc"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "layout ok" in run.stdout
