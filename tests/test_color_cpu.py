"""Colour input (cv::cvtColor(frame, img, CV_RGB2GRAY), video_source.cc:63) without a GPU: the numpy restatement of OpenCV's 8-bit
luma that the GPU tests check against, the C-ABI declarations and exports, argument validation, and the host layer's Image type."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slam-sdvl_amd", "host")
HEADER = os.path.join(ROOT, "include", "sdvl_hip.h")
ENTRIES = ("sdvl_convert_gray", "sdvl_frames_upload_color")
FORMATS = {"rgb": 1, "bgr": 2, "rgba": 3, "bgra": 4}


def to_gray(img, fmt):
    """cv::cvtColor *2GRAY for 8-bit input: Y = (c0 w0 + c1 w1 + c2 w2 + 8192) >> 14, R 4899 G 9617 B 1868; RGB orders put R on
    byte 0, BGR orders on byte 2; a fourth byte is ignored"""
    c = img.astype(np.int64)
    w0, w2 = (4899, 1868) if fmt in ("rgb", "rgba") else (1868, 4899)
    return ((c[..., 0] * w0 + c[..., 1] * 9617 + c[..., 2] * w2 + 8192) >> 14).astype(np.uint8)


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


def test_luma_known_values():
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], np.uint8)
    assert to_gray(rgb, "rgb").tolist() == [[76, 150, 29, 255, 0]]
    # the BGR order reads the same bytes the other way round
    assert to_gray(rgb, "bgr").tolist() == [[29, 150, 76, 255, 0]]
    assert 4899 + 9617 + 1868 == 1 << 14


def test_gray_maps_to_itself_and_alpha_is_ignored():
    v = np.arange(256, dtype=np.uint8)
    g = np.stack([v, v, v], -1)[None]
    for fmt in ("rgb", "bgr"):
        assert np.array_equal(to_gray(g, fmt)[0], v)
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    for alpha in (0, 255):
        rgba = np.concatenate([img, np.full((17, 23, 1), alpha, np.uint8)], -1)
        assert np.array_equal(to_gray(rgba, "rgba"), to_gray(img, "rgb"))
        assert np.array_equal(to_gray(rgba, "bgra"), to_gray(img, "bgr"))
    assert np.array_equal(to_gray(img[..., ::-1], "bgr"), to_gray(img, "rgb"))
    assert not np.array_equal(to_gray(img, "bgr"), to_gray(img, "rgb"))


def test_header_declares_the_colour_entries_and_the_format_enum():
    text = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    m = re.search(r"enum\s+sdvl_pixel_format\s*\{([^}]*)\}", text)
    assert m, "enum sdvl_pixel_format"
    vals = dict((k.strip(), int(v)) for k, v in re.findall(r"(SDVL_\w+)\s*=\s*(\d+)", m.group(1)))
    assert vals == {"SDVL_GRAY8": 0, "SDVL_RGB8": 1, "SDVL_BGR8": 2, "SDVL_RGBA8": 3, "SDVL_BGRA8": 4}
    assert "video_source.cc:63" in text


def test_library_exports_the_colour_entries(sdvl):
    lib = sdvl.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in sdvl.ABI_SYMBOLS, name
    assert (sdvl.SDVL_GRAY8, sdvl.SDVL_RGB8, sdvl.SDVL_BGR8, sdvl.SDVL_RGBA8, sdvl.SDVL_BGRA8) == (0, 1, 2, 3, 4)
    host = importlib.import_module("slam-sdvl_amd.tracker").load_host_library()
    for name in ("sdvlh_batch_set_color", "sdvlh_farm_set_color"):
        assert hasattr(host, name), name


def test_argument_validation_without_a_gpu(sdvl):
    lib = sdvl.load_library()
    img = np.zeros((4, 8, 3), np.uint8)
    out = np.zeros((4, 8), np.uint8)
    src = (C.c_void_p * 1)(img.ctypes.data)
    dst = (C.c_void_p * 1)(out.ctypes.data)
    lib.sdvl_convert_gray.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.sdvl_frames_upload_color.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    # null context (every call below has one: no GPU is needed to refuse), unknown format, short stride
    for fmt, stride in ((1, 24), (7, 24), (-1, 24), (1, 23), (4, 24)):
        assert lib.sdvl_convert_gray(None, 1, src, stride, 0, 8, 4, fmt, dst, 8) == -1
        assert lib.sdvl_frames_upload_color(None, 1, src, src, stride, 0, fmt, None, None) == -1
    host = importlib.import_module("slam-sdvl_amd.tracker").load_host_library()
    host.sdvlh_batch_set_color.argtypes = [C.c_void_p, C.c_int]
    host.sdvlh_farm_set_color.argtypes = [C.c_void_p, C.c_int]
    assert host.sdvlh_batch_set_color(None, 1) == -1
    assert host.sdvlh_farm_set_color(None, 1) == -1


def test_tracker_pixel_format_names():
    trk = importlib.import_module("slam-sdvl_amd.tracker")
    assert [trk.pixel_format(n) for n in ("gray", "RGB", "bgr", "rgba", "bgra")] == [0, 1, 2, 3, 4]
    assert trk.pixel_format(2) == 2
    for bad in ("yuv", 5, -1):
        with pytest.raises(ValueError):
            trk.pixel_format(bad)


IMAGE_PROBE = r"""
#include <cstdio>
#include "types.h"
using namespace sdvl;
int main() {
  static unsigned char px[4 * 6 * 5];
  Image g(4, 6, 0, px), c3(4, 6, 16, px), c4(4, 6, 24, px), pad(4, 6, 16, px, 20);
  std::printf("%d %d %d|%d %d %d|%d %d %d|%d|%d %d\n", g.format, g.channels(), g.step, c3.format, c3.channels(), c3.step,
              c4.format, c4.channels(), c4.step, pad.step, c3.bgr().format, c4.bgr().format);
  Image k = pad.clone();
  std::printf("%d %d %d\n", k.step, k.format, g.bgr().format);
#ifdef SDVL_HAVE_OPENCV
  cv::Mat m3(4, 6, 16, px), m4(4, 6, 24, px), m1(4, 6, CV_8UC1, px);
  Image i3(m3), i4(m4), i1(m1);
  std::printf("%d %d %d %d %d %d\n", i3.format, i3.empty() ? 1 : 0, i4.format, i4.empty() ? 1 : 0, i1.format, i1.empty() ? 1 : 0);
  cv::Mat back = i3;
  std::printf("%d\n", back.type());
#endif
  return 0;
}
"""


@pytest.mark.parametrize("third_party", [False, True])
def test_image_honours_colour_types(tmp_path, third_party):
    """Image(rows, cols, type, pixels, step) reads type 16 / 24 (CV_8UC3 / CV_8UC4) as colour in the reference's order, bgr() picks
    the other one, clone() copies whole colour rows; with OpenCV a 3- / 4-channel cv::Mat is accepted"""
    src = tmp_path / "probe.cc"
    src.write_text(IMAGE_PROBE)
    exe = tmp_path / "probe"
    inc = ["-I" + HOST]
    if third_party:
        inc = ["-I" + os.path.join(ROOT, "tests", "mock_third_party")] + inc
    else:
        inc = ["-DSDVL_NO_THIRD_PARTY_TYPES"] + inc
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), str(src)] + inc, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert lines[0] == "0 1 6|1 3 18|3 4 24|20|2 4"
    assert lines[1] == "18 1 0"
    if third_party:
        assert lines[2] == "1 0 3 0 0 0"
        assert lines[3] == "16"
