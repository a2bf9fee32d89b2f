"""numpy restatement of the raw camera formats' conversion to 8-bit gray (enum sdvl_raw_format, include/sdvl_hip.h).  It is the
specification of bayer_gray_kernel and wide_gray_kernel (csrc/sdvl_color.hip): the device gives these bytes exactly.  The rules are
stated HERE and not pinned to OpenCV: OpenCV's CV_Bayer??2GRAY names follow another convention and its border
handling differs, so no OpenCV Bayer parity is claimed.  YUYV / UYVY do equal cv::cvtColor(COLOR_YUV2GRAY_YUY2 / _UYVY).

Bayer (one byte per pixel; the name states the 2x2 tile at the image's top-left corner in reading order).  m(r, c) is the mosaic with
out-of-range indices reflected without repeating the edge (-1 -> 1, n -> n - 2), which keeps the Bayer parity.  Bilinear, times 4:
  R or B site (own colour X, opposite colour Z):  X4 = 4 m(r, c),  G4 = the four edge neighbours,  Z4 = the four diagonal neighbours
  G site (row neighbours of colour H, column neighbours of colour V):  G4 = 4 m(r, c),  H4 = 2 (m(r, c-1) + m(r, c+1)),
                                                                       V4 = 2 (m(r-1, c) + m(r+1, c))
  Y = (4899 R4 + 9617 G4 + 1868 B4 + 2^15) >> 16          (to_gray's weights; below 2^32)
YUYV / UYVY (two bytes per pixel, even width): gray is the Y byte, unscaled.
16-bit gray (little-endian uint16 of 10, 12 or 16 significant bits): s = bits - 8, Y = min(255, (v + (1 << (s - 1))) >> s): rounds
half up, saturates; values above the nominal depth saturate."""
import numpy as np

# enum sdvl_raw_format: name -> (code, bytes per pixel)
RAW_FORMATS = {
    "bayer_rggb": (16, 1), "bayer_grbg": (17, 1), "bayer_gbrg": (18, 1), "bayer_bggr": (19, 1),
    "yuyv": (20, 2), "uyvy": (21, 2), "gray10": (22, 2), "gray12": (23, 2), "gray16": (24, 2),
}
BAYER = ("bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr")
# (row, column) of the red site inside the 2x2 tile; blue sits diagonally opposite
RED_SITE = {"bayer_rggb": (0, 0), "bayer_grbg": (0, 1), "bayer_gbrg": (1, 0), "bayer_bggr": (1, 1)}
GRAY_BITS = {"gray10": 10, "gray12": 12, "gray16": 16}
WR, WG, WB = 4899, 9617, 1868


def bayer_sample(rgb, fmt):
    """the mosaic a sensor of order `fmt` sees of an RGB image [..., h, w, 3]: at each site the byte of that site's colour"""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[-3:-1]
    r0, c0 = RED_SITE[fmt]
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    red = ((rr & 1) == r0) & ((cc & 1) == c0)
    blue = ((rr & 1) != r0) & ((cc & 1) != c0)
    return np.where(red, rgb[..., 0], np.where(blue, rgb[..., 2], rgb[..., 1])).astype(np.uint8)


def bayer_to_gray(mosaic, fmt):
    """mosaic uint8 [..., h, w], h >= 2 and w >= 2 -> gray uint8 of the same shape"""
    m = np.asarray(mosaic)
    assert m.dtype == np.uint8 and m.shape[-1] >= 2 and m.shape[-2] >= 2
    h, w = m.shape[-2:]
    p = np.pad(m.astype(np.int64), [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)], mode="reflect")
    mid = p[..., 1:-1, 1:-1]
    left, right = p[..., 1:-1, :-2], p[..., 1:-1, 2:]
    up, down = p[..., :-2, 1:-1], p[..., 2:, 1:-1]
    diag = p[..., :-2, :-2] + p[..., :-2, 2:] + p[..., 2:, :-2] + p[..., 2:, 2:]
    r0, c0 = RED_SITE[fmt]
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    red_row, red_col = (rr & 1) == r0, (cc & 1) == c0
    red, blue = red_row & red_col, ~red_row & ~red_col
    own4, edge4 = 4 * mid, left + right + up + down
    hor4, ver4 = 2 * (left + right), 2 * (up + down)
    # at a G site of a red row the row neighbours are red and the column neighbours blue; in a blue row the other way round
    R4 = np.where(red, own4, np.where(blue, diag, np.where(red_row, hor4, ver4)))
    B4 = np.where(blue, own4, np.where(red, diag, np.where(red_row, ver4, hor4)))
    G4 = np.where(red | blue, edge4, own4)
    return ((WR * R4 + WG * G4 + WB * B4 + (1 << 15)) >> 16).astype(np.uint8)


def yuv422_to_gray(buf, fmt):
    """uint8 [..., h, w, 2] (w even: Y0 U Y1 V or U Y0 V Y1 per pixel pair) -> the Y bytes [..., h, w]"""
    b = np.asarray(buf)
    assert b.dtype == np.uint8 and b.shape[-1] == 2 and b.shape[-2] % 2 == 0
    return b[..., 0 if fmt == "yuyv" else 1].copy()


def gray16_to_gray(v, fmt):
    """uint16 [...] of GRAY_BITS[fmt] significant bits -> uint8, rounded half up and saturated"""
    v = np.asarray(v)
    assert v.dtype == np.uint16
    s = GRAY_BITS[fmt] - 8
    return np.minimum(255, (v.astype(np.int64) + (1 << (s - 1))) >> s).astype(np.uint8)


def raw_to_gray(img, fmt):
    """an image of any raw format, as its natural numpy array (Bayer uint8 [h, w]; YUYV / UYVY uint8 [h, w, 2]; 16-bit gray
    uint16 [h, w]) -> gray uint8 [h, w]"""
    if fmt in BAYER:
        return bayer_to_gray(img, fmt)
    if fmt in GRAY_BITS:
        return gray16_to_gray(img, fmt)
    return yuv422_to_gray(img, fmt)
