"""The pose stage's parts of a track set's scratch (csrc/sdvl_track.hip): job and hypothesis records exist only for sets of at most 4
trackers, whose pose stage runs on separate launches; for larger sets both parts are empty and the rest moves up by exactly the bytes
saved.  tests/track_scratch_check.cc states it with csrc/sdvl_layout.h, built with the host compiler under AddressSanitizer and UBSan
(no GPU, nothing loaded into Python) — next to tests/test_layout_cpu.py, which holds the layout arithmetic itself."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "slam-sdvl_amd", "csrc")


def test_track_scratch_has_no_job_or_hypothesis_records_for_sets_of_more_than_4(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the host compiler that builds libsdvl_synth.so is missing"
    exe = str(tmp_path / "track_scratch_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing depends on library order
                           "-I", CSRC, os.path.join(HERE, "track_scratch_check.cc"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "track scratch ok" in run.stdout


def test_the_statement_names_the_rule_the_library_uses():
    """the threshold in the check is the library's: sdvl_pose_separate_launches (csrc/sdvl_pose.hip) and both callers size their parts by it"""
    with open(os.path.join(CSRC, "sdvl_pose.hip")) as f:
        assert "bool sdvl_pose_separate_launches(int batch_size) { return batch_size <= 4; }" in f.read()
    with open(os.path.join(CSRC, "sdvl_track.hip")) as f:
        src = f.read()
    assert "s->pjobs = L.take<PoseJobDev>(separate ? N : 0);" in src
    assert "s->hyp = L.take<uint8_t>(separate ? sdvl_pose_hyp_bytes() * N * s->max_its : 0);" in src
