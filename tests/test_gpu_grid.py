"""Detection grids beyond the 640x480 / cell 32 range: cell sizes 8 .. 64 (cells wider than 32 take the wide-tile FAST kernel and
16-bit list positions in the selection), more than 2048 cells and 4096 candidates per pyramid level, filter grids beyond 4096 cells,
frames up to 3840x2160.  Every layer against the CPU oracle through the C-ABI, with the parity classes of test_gpu_parity.py and
test_gpu_tracker.py: FAST lists, DetectPyramid, FilterCorners and ORB bit-exact, tracked frames with identical decisions and poses
within 1e-4.  Each case here was refused before (cell_size > 32, > 2048 cells in a level, > 4096 filter cells)."""
import importlib

import numpy as np
import pytest

from oraclelib import TUM_CAM, TUM_DIST, XI, trajectory_pose
from test_gpu_parity import rand_img, sparse_corner_image

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def trk(sdvl):
    return importlib.import_module("slam-sdvl_amd.tracker")


def cam_for(w, h):
    """TUM_CAM's field of view at another frame size"""
    f = np.array(TUM_CAM, np.float64)
    return np.array([f[0] * w / 640.0, f[1] * w / 640.0, f[2] * w / 640.0, f[3] * h / 480.0])


def render(synth, orc, w, h, k, xi=XI, seed=20260001, dist=None):
    if dist is None:
        return synth.render(trajectory_pose(orc, k, xi), cam_for(w, h), w, h, seed=seed, frame_id=k)
    return synth.render(trajectory_pose(orc, k, xi), cam_for(w, h), w, h, seed=seed, frame_id=k, dist=dist)


class oracle_cell:
    """the oracle's cell size for the duration of a block"""
    def __init__(self, orc, cell):
        self.orc, self.cell = orc, cell

    def __enter__(self):
        self.old = self.orc.params.cell_size
        self.orc.params.cell_size = self.cell

    def __exit__(self, *a):
        self.orc.params.cell_size = self.old


# ------------------------------------------------------------------------------------------------ FAST per-cell lists
def fast_lists_match(ctx, sdvl, orc, img, cell, thr, margin):
    """sdvl_fast_cells against the oracle's cv::FAST-per-ROI on every detection level: keypoints, scores, order and cell offsets.
    Returns (keypoints in all, longest cell list)."""
    dp = sdvl.default_detect_params()
    dp.margin, dp.fast_threshold, dp.cell_size = margin, thr, cell
    saved = (orc.params.fast_threshold, orc.params.use_orb)
    orc.params.fast_threshold = thr
    orc.params.use_orb = 1 if margin == 19 else 0
    f = ctx.frame(img, levels=5)
    try:
        with oracle_cell(orc, cell):
            got, cpl = ctx.fast_cells([f], dp)
            kps, offs = got[0]
            pyr = orc.pyramid(img, 5)
            base, total, longest = 0, 0, 0
            for l in range(dp.max_fast_levels):
                wk, woffs, _ = orc.fast_cells(pyr[l], cap=400000)
                g = kps[kps[:, 3] == l]
                assert np.array_equal(g[:, :3], wk), "cell %d level %d keypoints (x,y,score) incl. order" % (cell, l)
                assert np.array_equal(offs[base:base + cpl[l] + 1] - offs[base], woffs), "cell %d level %d cell offsets" % (cell, l)
                base += cpl[l]
                total += len(wk)
                longest = max(longest, int(np.diff(woffs).max()))
    finally:
        f.close()
        orc.params.fast_threshold, orc.params.use_orb = saved
    return total, longest


@pytest.mark.parametrize("cell", [8, 16, 24, 40, 48, 63, 64])
def test_fast_cells_any_cell_size(ctx, sdvl, orc, cell):
    """dense noise (the packed-halves path up to 32, the wide tile beyond) and a sparse-corner image (the candidate-list path up to
    32); 640 is no multiple of 24, 48 or 63: the last cell column is narrower"""
    dense = rand_img(8, 480, 640)
    sparse = sparse_corner_image(3, 480, 640)
    n_dense, longest = fast_lists_match(ctx, sdvl, orc, dense, cell, thr=10, margin=5)
    assert n_dense > 1000
    if cell == 64:
        assert longest > 255, longest      # positions beyond a byte: the 16-bit form of select_cells
    n_sparse, _ = fast_lists_match(ctx, sdvl, orc, sparse, cell, thr=10, margin=19)
    assert 100 < n_sparse < 30000, n_sparse


def test_fast_cells_wide_cells_on_an_odd_frame(ctx, sdvl, orc):
    """a frame whose sides are no multiple of the cell nor of 4: narrow last cells, unaligned level rows"""
    img = rand_img(11, 363, 557)
    for cell in (40, 64):
        n, _ = fast_lists_match(ctx, sdvl, orc, img, cell, thr=20, margin=5)
        assert n > 500, (cell, n)


# ------------------------------------------------------------------------------------------------ DetectPyramid
@pytest.mark.parametrize("w,h,cell", [
    (1920, 1200, 32),    # 60 x 38 = 2280 cells in level 0
    (2560, 1440, 32),    # 80 x 45 = 3600
    (3840, 2160, 32),    # 120 x 68 = 8160
    (3840, 2160, 64),    # wide cells on the largest frame
    (640, 480, 16),      # 1200 cells of 16 px
])
def test_detect_corners_large_grids(ctx, sdvl, orc, synth, w, h, cell):
    """FastDetector::DetectPyramid on the device: the same corners in the same order as the oracle, on a rendered frame and on noise
    (many ties: level lists that outgrow the LDS go through the spill area)"""
    imgs = [render(synth, orc, w, h, 3), rand_img(w + cell, h, w)]
    dp = sdvl.default_detect_params()
    dp.cell_size = cell
    fr = [ctx.frame(im) for im in imgs]
    try:
        got = ctx.detect_corners(fr, dp, 1000)
        with oracle_cell(orc, cell):
            if cell > 32:  # a level-0 cell of the noise frame lists more than 255 corners: select_cells' retainBest on 16-bit positions
                _, woffs, _ = orc.fast_cells(imgs[1], cap=((w + cell - 1) // cell) * ((h + cell - 1) // cell) * 841)
                assert np.diff(woffs).max() > 255, np.diff(woffs).max()
            for k, (im, g) in enumerate(zip(imgs, got)):
                want = orc.detect_pyramid(im, nfeatures=1000)
                assert len(want) >= 900, (k, len(want))
                assert np.array_equal(g, want), (k, len(g), len(want))
    finally:
        for f in fr:
            f.close()


# ------------------------------------------------------------------------------------------------ FilterCorners + ORB
def test_filter_corners_on_an_8160_cell_grid(ctx, sdvl, orc, synth):
    """Frame::FilterCorners at 3840x2160, cell 32 (the fourth filter_select form), a few cells locked: kept indices, truncated
    Shi-Tomasi scores and ORB descriptors as the oracle's"""
    w, h, cell = 3840, 2160, 32
    img = render(synth, orc, w, h, 2)
    with oracle_cell(orc, cell):
        corners = orc.detect_pyramid(img, nfeatures=2000)
    # ten level-0 FAST corners crowded into the one cell that has the most: more than the form's four slots, the scan fallback
    fast = orc.fast(img, thr=10, nonmax=True)
    fast = fast[(fast[:, 0] >= 40) & (fast[:, 0] < w - 40) & (fast[:, 1] >= 40) & (fast[:, 1] < h - 40)]
    cid = (fast[:, 1] // cell) * ((w + cell - 1) // cell) + fast[:, 0] // cell
    busiest = np.bincount(cid).argmax()
    crowd = fast[cid == busiest][:10, :2]
    assert len(crowd) > 4, len(crowd)
    corners = np.concatenate([corners, np.concatenate([crowd, np.zeros((len(crowd), 1), np.int32)], 1)]).astype(np.int32)
    locked = [[cell * 1.5, cell * 2.5], [w - 1.0, h - 1.0], [w / 2.0, h / 3.0]]
    locked += [[float(x), float(y)] for x, y in corners[:40:4, :2]]       # cells that hold a corner
    f = ctx.frame(img)
    f.set_corners(corners)
    try:
        idx, xyl, score, desc = ctx.filter_corners([f], [locked], cell_size=cell)[0]
    finally:
        f.close()
    with oracle_cell(orc, cell):
        want = orc.filter_corners(img, corners, locked)
    assert len(want) > 100
    assert np.array_equal(idx, want), (len(idx), len(want))
    assert np.array_equal(xyl, corners[want])
    pyr = orc.pyramid(img, 5)
    for k in range(0, len(idx), 7):
        x, y, l = xyl[k]
        assert score[k] == int(orc.shi_tomasi(pyr[l], x, y))
        d, _ = orc.orb_describe(pyr[l], [[x, y]])
        inside = 19 <= x < pyr[l].shape[1] - 19 and 19 <= y < pyr[l].shape[0] - 19
        assert np.array_equal(desc[k], d[0] if inside else np.zeros(32, np.uint8))


# ------------------------------------------------------------------------------------------------ undistortion
@pytest.mark.parametrize("w,h", [(3840, 2160), (2560, 1440), (2045, 64), (130, 2100)])
def test_undistort_wide_map(ctx, sdvl, orc, w, h):
    """frames with a side above 2044 take the two-word map (integer parts of 16 bits): cv::undistort byte for byte, the plain form
    and fused into the frames' upload (sdvl_frames_upload_undistorted), TUM fr1's lens at the camera's field of view"""
    cam4 = cam_for(w, h) if w >= 640 and h >= 480 else np.array([0.8 * w, 0.82 * w, w / 2.0 - 0.4, h / 2.0 + 0.3])
    dist = TUM_DIST if w >= 640 and h >= 480 else np.array([-0.45, 0.3, 0.01, -0.008, 0.05])
    rng = np.random.default_rng(w + 7 * h)
    imgs = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(5)]
    want = [orc.undistort(im, cam4, dist) for im in imgs]
    assert all((wnt != im).mean() > 0.3 for wnt, im in zip(want, imgs))
    c = sdvl.Camera(w, h, *cam4)
    got = ctx.undistort(imgs, c, dist)
    for i in range(len(imgs)):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    fr = [ctx.frame(width=w, height=h, levels=1, pyramid=False) for _ in range(2)]
    try:
        ctx.undistort(imgs[:2], c, dist, frames=fr)
        for i in range(2):
            assert np.array_equal(fr[i].level(0), want[i]), ("fused", i)
    finally:
        for f in fr:
            f.close()


# ------------------------------------------------------------------------------------------------ closed loop
def closed_loop(trk, orc, synth, B, w, h, cell, n_frames, mapper=False, dist=None):
    """TrackerBatch against the oracle tracker at this frame size and cell size: per-frame decisions identical, poses within 1e-4
    (with the mapper: map counters identical too), every step on the device-resident tables (host_path 0).  dist: frames rendered
    through that lens go in raw and are undistorted inside the step; the oracle gets its own cv::undistort of the same bytes."""
    over = dict(trk.TUM_OVERRIDES)
    over["SDVL.cell_size"] = cell
    trk.configure(over)
    cam = cam_for(w, h)
    xis = [XI * (1.0 + 0.2 * i) * (1 if i % 2 == 0 else -1) for i in range(B)]
    seeds = [20260001 + i for i in range(B)]
    old = orc.params.cell_size
    orc.params.cell_size = cell
    dev = batch = None
    oracles = []
    try:
        if mapper:
            trk.set_mapper(True)
        try:
            dev = trk.HostDevice(0)
            batch = trk.TrackerBatch(dev, B, w, h, cam)
        finally:
            trk.set_mapper(False)
        if dist is not None:
            batch.set_distortion(dist)
        oracles = [orc.tracker(w, h, cam) for _ in range(B)]
        for o in oracles:
            o.use_mapper(mapper)
        worst = 0.0
        for k in range(n_frames):
            imgs = [render(synth, orc, w, h, k, xis[i], seeds[i], dist) for i in range(B)]
            got = batch.step_host(imgs)
            for i in range(B):
                want = oracles[i].handle_frame(imgs[i] if dist is None else orc.undistort(imgs[i], cam, dist))
                g = got[i]
                assert g.host_path == 0, (k, i)
                assert (g.state, g.quality, g.keyframe, g.n_corners) == (want.state, want.quality, want.keyframe, want.n_corners), (k, i)
                assert (g.matches, g.attempts, g.inliers, g.outliers) == (want.matches, want.attempts, want.inliers, want.outliers), (k, i)
                assert g.align_meas == want.align_meas, (k, i)
                d = float(np.abs(np.array(g.pose[:]) - np.array(want.pose[:])).max())
                worst = max(worst, d)
                assert d <= POSE_TOL, (k, i, d)
                if mapper:
                    assert batch.map_stats(i) == oracles[i].map_stats(), (k, i)
                if k > 0:
                    assert g.quality == 0 and g.matches >= 50, (k, i, g.quality, g.matches)
    finally:
        if batch is not None:
            batch.close()
        for o in oracles:
            o.close()
        if dev is not None:
            dev.close()
        orc.params.cell_size = old
        trk.configure()
    return worst


def test_closed_loop_3840x2160_cell_64_two_trackers_through_the_lens(trk, orc, synth):
    """raw frames of a camera with config_tum_f1.cfg's lens coefficients: the wide undistortion map inside the step"""
    assert closed_loop(trk, orc, synth, B=2, w=3840, h=2160, cell=64, n_frames=12, dist=TUM_DIST) <= POSE_TOL


def test_closed_loop_640x480_cell_16(trk, orc, synth):
    assert closed_loop(trk, orc, synth, B=1, w=640, h=480, cell=16, n_frames=12) <= POSE_TOL


def test_closed_loop_with_mapper_1920x1200_cell_32(trk, orc, synth):
    assert closed_loop(trk, orc, synth, B=1, w=1920, h=1200, cell=32, n_frames=12, mapper=True) <= POSE_TOL


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_limit_and_leave_the_context_usable(ctx, sdvl, orc, synth):
    img = render(synth, orc, 640, 480, 1)
    f = ctx.frame(img)
    dp = sdvl.default_detect_params()
    dp.cell_size = 65
    with pytest.raises(sdvl.SdvlError, match=r"cell_size must be in \[8,64\]"):
        ctx.detect_corners([f], dp, 1000)
    with pytest.raises(sdvl.SdvlError, match=r"cell_size must be in \[8,64\]"):
        ctx.fast_cells([f], dp, cap=1000)
    big = ctx.frame(width=4000, height=2400)     # 125 x 75 cells of 32 px in level 0
    dp.cell_size = 32
    with pytest.raises(sdvl.SdvlError, match="too many cells in one level.*8192"):
        ctx.detect_corners([big], dp, 1000)
    with pytest.raises(sdvl.SdvlError, match="too many cells in one level.*8192"):
        ctx.fast_cells([big], dp, cap=1000)
    big.close()
    with pytest.raises(sdvl.SdvlError, match="frame size out of range"):
        ctx.frame(width=4096, height=2160)
    got = ctx.detect_corners([f], dp, 1000)[0]
    assert np.array_equal(got, orc.detect_pyramid(img, nfeatures=1000))
    f.close()
