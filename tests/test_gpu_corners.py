"""Corner scores, ORB descriptors and the per-cell corner selection (csrc/sdvl_orb.hip) against the CPU oracle on the designed inputs of
tests/corner_cases.py: both sides of every border test, chosen orientations, batches of frames, ties and full bins in every form of the
selection, corner counts only the device knows, sdvl_filter_inputs, and the search's ORB threshold one bit at a time.  All of it is integer
or byte work: every comparison is exact.  tests/test_corner_cases_cpu.py asserts on the oracle alone that the inputs hit what they claim."""
import ctypes as C
import importlib

import numpy as np
import pytest

import corner_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


@pytest.fixture(scope="module")
def ctx(sdvl):
    c = sdvl.Context(0)
    yield c
    c.close()


def handles(frames):
    return (C.c_void_p * len(frames))(*[f.h for f in frames])


# ------------------------------------------------------------------------------------------------ 1. chosen points
@pytest.mark.parametrize("name", sorted(cc.NOISE))
def test_shi_tomasi_on_both_sides_of_its_limit_at_every_level(ctx, orc, name):
    img = cc.noise_image(name)
    pyr = cc.pyramid_of(orc, img)
    f = ctx.frame(img)
    try:
        for l in range(cc.LEVELS):
            assert np.array_equal(f.level(l), pyr[l]), "level %d" % l        # odd sizes: the premise of everything below
        xyl = cc.shi_points(name)
        f.set_corners(xyl)
        got = ctx.shi_tomasi([f])[0]
    finally:
        f.close()
    want = cc.shi_want(orc, pyr, xyl)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def test_shi_tomasi_four_corners_per_wave(ctx, orc):
    """lists that fill a wave's four 16-lane groups partly, exactly and with one corner over, inside and outside points in every pattern"""
    img = cc.noise_image("P")
    xyl = cc.shi_wave_list()
    want = cc.shi_want(orc, cc.pyramid_of(orc, img), xyl)
    f = ctx.frame(img)
    try:
        for n in cc.SHI_WAVE_LENGTHS:
            f.set_corners(xyl[:n])
            got = ctx.shi_tomasi([f])[0]
            assert np.array_equal(got, want[:n]), n
        f.set_corners(xyl[::-1])                         # every group's neighbours changed
        assert np.array_equal(ctx.shi_tomasi([f])[0], want[::-1])
    finally:
        f.close()


@pytest.mark.parametrize("name", sorted(cc.NOISE))
def test_orb_on_both_sides_of_its_limits_at_every_level(ctx, orc, name):
    img = cc.noise_image(name)
    xyl = cc.orb_points(name)
    want_d, want_a = cc.orb_want(orc, cc.pyramid_of(orc, img), xyl)
    f = ctx.frame(img)
    try:
        f.set_corners(xyl)
        got = ctx.orb_describe([f])[0]
        assert np.array_equal(got, want_d), np.nonzero((got != want_d).any(axis=1))[0][:8]
        assert np.array_equal(f.descriptors(), want_d)
        gd, ga = ctx.orb_describe_points(f, xyl)
        assert np.array_equal(gd, want_d) and np.array_equal(ga, want_a), np.nonzero(ga != want_a)[0][:8]
    finally:
        f.close()


@pytest.mark.parametrize("name", sorted(cc.RAMP_ANGLES))
def test_orb_orientations(ctx, orc, name):
    """quadrant boundaries, the |m10| == |m01| tie and a flat patch: angle and descriptor bit for bit"""
    img = cc.ramp_images()[name]
    want_d, want_a = cc.orb_want(orc, cc.pyramid_of(orc, img, cc.RAMP_LEVELS), cc.RAMP_POINTS)
    f = ctx.frame(img, levels=cc.RAMP_LEVELS)
    try:
        f.set_corners(cc.RAMP_POINTS)
        gd, ga = ctx.orb_describe_points(f, cc.RAMP_POINTS)
        assert np.array_equal(ga, want_a), (ga, want_a)
        assert np.array_equal(gd, want_d)
        assert np.array_equal(ctx.orb_describe([f])[0], want_d)
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------ 2. batches
@pytest.fixture(scope="module")
def batch(ctx, orc):
    """the 17 frames of corner_cases.batch_frame with their corners set, and the oracle's scores and descriptors of each"""
    frames, want = [], []
    for k in range(max(cc.BATCH_SIZES)):
        img, xyl = cc.batch_frame(k)
        f = ctx.frame(img)
        f.set_corners(xyl)
        frames.append(f)
        pyr = cc.pyramid_of(orc, img)
        want.append((cc.shi_want(orc, pyr, xyl), cc.orb_want(orc, pyr, xyl)[0]))
    yield frames, want
    for f in frames:
        f.close()


@pytest.mark.parametrize("n", cc.BATCH_SIZES)
def test_scores_and_descriptors_of_a_batch_of_frames(ctx, sdvl, batch, n):
    """n frames of two sizes and ragged counts in one call: the block-to-frame map with its padding blocks, the ragged copy back; the
    output capacity exactly the largest count, and one less (refused, and the context works afterwards)"""
    frames, want = batch[0][:n], batch[1][:n]
    largest = max(len(w[0]) for w in want)
    for cap in (max(largest, 1), sdvl.MAX_CORNERS):
        scores = ctx.shi_tomasi(frames, cap=cap)
        desc = ctx.orb_describe(frames, cap=cap)
        for k in range(n):
            assert np.array_equal(scores[k], want[k][0]), (cap, k)
            assert desc[k].shape == want[k][1].shape and np.array_equal(desc[k], want[k][1]), (cap, k)
    if largest >= 2:
        for call in (ctx.shi_tomasi, ctx.orb_describe):
            with pytest.raises(sdvl.SdvlError, match="capacity"):
                call(frames, cap=largest - 1)
            got = call(frames, cap=largest)
            assert all(np.array_equal(g, w[0] if call == ctx.shi_tomasi else w[1]) for g, w in zip(got, want))


def test_each_frame_of_the_batch_alone_and_a_batch_without_corners(ctx, batch):
    frames, want = batch
    for k, f in enumerate(frames):
        assert np.array_equal(ctx.shi_tomasi([f])[0], want[k][0]), k
        assert np.array_equal(ctx.orb_describe([f])[0], want[k][1]), k
    none = [f for f, w in zip(frames, want) if len(w[0]) == 0]
    assert len(none) >= 4
    assert all(s.shape == (0,) for s in ctx.shi_tomasi(none)) and all(d.shape == (0, 32) for d in ctx.orb_describe(none))
    assert all(s.shape == (0,) for s in ctx.shi_tomasi(none, cap=1))
    assert np.array_equal(ctx.shi_tomasi(frames[:9])[7], want[7][0])          # and the context goes on


# ------------------------------------------------------------------------------------------------ 3. selection
def check_filter(ctx, orc, cases, cell, margin=19, min_score=50, frames=None):
    """cases = [(image, corners, locked positions)] of one size in ONE call of the device's FilterCorners: kept indices, their corners,
    truncated scores and descriptors of every kept corner as the oracle's.  -> kept indices per frame"""
    own = frames is None
    if own:
        frames = []
        for img, corners, _ in cases:
            frames.append(ctx.frame(img))
            frames[-1].set_corners(corners)
    try:
        got = ctx.filter_corners(frames, [c[2] for c in cases], cell_size=cell, margin=margin, min_feature_score=min_score)
    finally:
        if own:
            for f in frames:
                f.close()
    kept = []
    for k, ((img, corners, locked), (idx, xyl, score, desc)) in enumerate(zip(cases, got)):
        want = cc.oracle_filter(orc, img, corners, locked, cell=cell, min_score=min_score, use_orb=1 if margin == 19 else 0)
        assert np.array_equal(idx, want), (k, len(idx), len(want))
        assert np.array_equal(xyl, np.asarray(corners).reshape(-1, 3)[want]), k
        pyr = cc.pyramid_of(orc, img)
        assert np.array_equal(score, cc.shi_want(orc, pyr, xyl).astype(np.int32)), k       # the truncated scores
        assert np.array_equal(desc, cc.orb_want(orc, pyr, xyl)[0]), k                        # zeros outside ORB's limits
        kept.append(want)
    return kept


@pytest.mark.parametrize("form", sorted(cc.FORMS))
def test_selection_forms_with_ties_and_full_bins(ctx, orc, form):
    """every form of filter_select on a small image: a point listed twice and three times (the last occurrence wins: `score >
    truncated best`), cells holding one corner fewer than a bin, exactly a bin, one more and many more, the winner last"""
    c = cc.selection_case(orc, form)
    assert cc.select_form(c["n_cells"], max(len(c["corners"]), 1)) == form
    kept = check_filter(ctx, orc, [(c["img"], c["corners"], np.zeros((0, 2)))], c["cell"])[0]
    assert all(occ[-1] in kept for occ in c["ties"].values())


def test_selection_at_the_score_threshold(ctx, orc):
    """scores around min_feature_score: a score in (50, 51) passes `score > best` and is dropped by `best > 50`"""
    c = cc.threshold_case(orc)
    case = [(c["img"], c["corners"], np.zeros((0, 2)))]
    n50 = len(check_filter(ctx, orc, case, c["cell"])[0])
    n0 = len(check_filter(ctx, orc, case, c["cell"], min_score=0)[0])
    assert n0 > n50 > 0
    assert len(check_filter(ctx, orc, case, c["cell"], min_score=c["above"])[0]) == 0


@pytest.mark.parametrize("margin", [19, 5])
def test_selection_margin_levels_and_locked_cells(ctx, orc, margin):
    """corners on both sides of the margin on levels 0 to 2, corners of levels 1 and 2 in locked cells and (margin 5) in the last row and
    column of cells, kept corners outside ORB's limits (margin 5: zero descriptors)"""
    c = cc.margin_case(orc)
    none = np.zeros((0, 2))
    first = check_filter(ctx, orc, [(c["img"], c["corners"], none)], c["cell"], margin=margin)[0]
    assert np.array_equal(first, c[margin]["first"])
    second, again = check_filter(ctx, orc, [(c["img"], c["corners"], c[margin]["locked"]), (c["img"], c["corners"], none)], c["cell"], margin=margin)
    assert len(second) < len(first) and np.array_equal(again, first)


def test_selection_of_a_batch_with_a_lock_mask_per_frame(ctx, orc):
    cases = cc.selection_batch()
    together = check_filter(ctx, orc, cases, 32)
    assert len(together[4]) == 0
    for k in (0, 4, 8):
        assert np.array_equal(check_filter(ctx, orc, cases[k:k + 1], 32)[0], together[k])


def detect_on_device(ctx, sdvl, frames):
    """sdvl_detect_corners without asking for the counts: the frames' corner counts stay on the device"""
    dp = sdvl.default_detect_params()
    ctx._check(ctx.lib.sdvl_detect_corners(ctx.h, len(frames), handles(frames), C.byref(dp), cc.DEVICE_COUNT_FEATURES))
    for f in frames:
        assert ctx.lib.sdvl_frame_num_corners(f.h) == -1


def download_corners(ctx, f):
    xyl = np.zeros((6144, 3), np.int32)
    k = C.c_int()
    ctx._check(ctx.lib.sdvl_frame_download_corners(ctx.h, f.h, len(xyl), xyl.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k)))
    return xyl[:k.value].copy()


def test_selection_when_only_the_device_knows_the_count(ctx, sdvl, orc):
    """detection straight into the filter (the production path): the launches are cut for 1280 corners and stride over the rest"""
    img = cc.device_count_image()
    other = cc.selection_batch()[8]
    other_img = cc.noise(77, 480, 640)
    other_xyl = np.array([(x, y, 0) for x, y, _ in other[1]] + [(150 + x, 100 + y, 1) for x, y, _ in other[1][:50]], np.int32)
    f, g = ctx.frame(img), ctx.frame(other_img)
    try:
        detect_on_device(ctx, sdvl, [f])
        alone = ctx.filter_corners([f], [np.zeros((0, 2))])[0]
        corners = download_corners(ctx, f)
        assert len(corners) > 1280 and np.array_equal(corners, orc.detect_pyramid(img, nfeatures=cc.DEVICE_COUNT_FEATURES))
        check_filter(ctx, orc, [(img, corners, np.zeros((0, 2)))], 32, frames=[f])           # the count is known now
        want = cc.oracle_filter(orc, img, corners)
        assert np.array_equal(alone[0], want) and np.array_equal(alone[1], corners[want])
        pyr = cc.pyramid_of(orc, img)
        assert np.array_equal(alone[2], cc.shi_want(orc, pyr, corners[want]).astype(np.int32))
        assert np.array_equal(alone[3], cc.orb_want(orc, pyr, corners[want])[0])
        assert (want >= 1280).any()                           # kept corners beyond the launch bound
        # again, unknown once more, in one batch with a frame whose count the host knows
        detect_on_device(ctx, sdvl, [f])
        g.set_corners(other_xyl)
        locked = [[100.0, 100.0], [333.3, 250.1]]
        both = ctx.filter_corners([g, f], [np.zeros((0, 2)), locked])
        want_f = cc.oracle_filter(orc, img, corners, locked)
        want_g = cc.oracle_filter(orc, other_img, other_xyl)
        assert len(want_g) > 10 and len(want_f) < len(want)
        for got, wnt, im, xyl in ((both[0], want_g, other_img, other_xyl), (both[1], want_f, img, corners)):
            assert np.array_equal(got[0], wnt) and np.array_equal(got[1], xyl[wnt])
            p = cc.pyramid_of(orc, im)
            assert np.array_equal(got[2], cc.shi_want(orc, p, xyl[wnt]).astype(np.int32))
            assert np.array_equal(got[3], cc.orb_want(orc, p, xyl[wnt])[0])
    finally:
        f.close(); g.close()


def test_selection_after_a_new_image_finds_no_corners(ctx, orc):
    """a frame that had corners and then got a new image has none until it is detected again"""
    cases = cc.selection_batch()
    f, g = ctx.frame(cases[0][0]), ctx.frame(cases[1][0])
    try:
        f.set_corners(cases[0][1]); g.set_corners(cases[1][1])
        f.upload(cases[2][0])
        ctx.pyramid_build([f])
        got = ctx.filter_corners([f, g], [np.zeros((0, 2))] * 2)
        assert len(got[0][0]) == 0
        assert np.array_equal(got[1][0], cc.oracle_filter(orc, cases[1][0], cases[1][1])) and len(got[1][0]) > 3
        assert [len(x[0]) for x in ctx.filter_inputs([f, g])] == [0, len(cases[1][1])]
    finally:
        f.close(); g.close()


# ------------------------------------------------------------------------------------------------ 4. sdvl_filter_inputs
def check_inputs(orc, got, cases, with_desc):
    assert len(got) == len(cases)
    for k, ((xyl, scores, desc), (img, corners)) in enumerate(zip(got, cases)):
        pyr = cc.pyramid_of(orc, img)
        assert np.array_equal(xyl, np.asarray(corners).reshape(-1, 3)), k
        assert np.array_equal(scores, cc.shi_want(orc, pyr, corners)), k
        if with_desc:
            assert np.array_equal(desc, cc.orb_want(orc, pyr, corners)[0]), k
        else:
            assert desc is None


@pytest.mark.parametrize("with_desc", [True, False], ids=["descriptors", "no-descriptors"])
@pytest.mark.parametrize("n", [1, 9])
def test_filter_inputs_of_ragged_batches(ctx, sdvl, orc, n, with_desc):
    """counts, corners, scores and descriptors in one round trip.  Every count is known to the host: the rows shorten to the largest"""
    cases = cc.inputs_frames(n)
    largest = max(len(c[1]) for c in cases)
    frames = [ctx.frame(img) for img, _ in cases]
    try:
        for f, (_, xyl) in zip(frames, cases):
            f.set_corners(xyl)
        for cap in (sdvl.MAX_CORNERS, largest + 50, largest):
            check_inputs(orc, ctx.filter_inputs(frames, cap, with_desc), cases, with_desc)
        with pytest.raises(sdvl.SdvlError, match="capacity"):
            ctx.filter_inputs(frames, largest - 1, with_desc)
        check_inputs(orc, ctx.filter_inputs(frames, largest, with_desc), cases, with_desc)
        empty = [f for f, c in zip(frames, cases) if len(c[1]) == 0]
        if empty:                                            # nothing but a frame without corners: rows of one record
            check_inputs(orc, ctx.filter_inputs(empty, 16, with_desc), [c for c in cases if len(c[1]) == 0], with_desc)
    finally:
        for f in frames:
            f.close()


def test_filter_inputs_with_a_count_only_the_device_knows(ctx, sdvl, orc):
    """one frame straight from detection: the rows are as long as the capacity says; a capacity below its count is refused"""
    img = cc.device_count_image()
    small = cc.inputs_frames(9)[4]
    f, g = ctx.frame(img), ctx.frame(small[0])
    try:
        g.set_corners(small[1])
        corners = orc.detect_pyramid(img, nfeatures=cc.DEVICE_COUNT_FEATURES)
        for with_desc in (True, False):
            detect_on_device(ctx, sdvl, [f])
            check_inputs(orc, ctx.filter_inputs([g, f], sdvl.MAX_CORNERS, with_desc), [small, (img, corners)], with_desc)
        detect_on_device(ctx, sdvl, [f])
        check_inputs(orc, ctx.filter_inputs([f, g], len(corners), True), [(img, corners), small], True)
        detect_on_device(ctx, sdvl, [f])
        with pytest.raises(sdvl.SdvlError, match="capacity"):
            ctx.filter_inputs([f, g], len(corners) - 1, True)
        check_inputs(orc, ctx.filter_inputs([f, g], len(corners), False), [(img, corners), small], False)
    finally:
        f.close(); g.close()


def test_filter_inputs_end_needs_its_begin(ctx, sdvl, orc):
    cases = cc.inputs_frames(9)[:3]
    frames = [ctx.frame(img) for img, _ in cases]
    lib, n, cap = ctx.lib, 3, 64
    xyl, scores, desc = np.zeros((n, cap, 3), np.int32), np.zeros((n, cap), np.float64), np.zeros((n, cap, 32), np.uint8)
    counts = np.zeros(n, np.int32)

    def end(m, d):
        return lib.sdvl_filter_inputs_end(ctx.h, m, handles(frames[:m]), cap, xyl.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p),
                                          desc.ctypes.data_as(C.c_void_p) if d else None, counts.ctypes.data_as(C.c_void_p))
    try:
        for f, (_, c) in zip(frames, cases):
            f.set_corners(c)
        check_inputs(orc, ctx.filter_inputs(frames, cap, True), cases, True)        # a complete pair leaves nothing pending
        assert end(n, True) != 0
        for with_desc in (1, 0):
            assert lib.sdvl_filter_inputs_begin(ctx.h, n, handles(frames), cap, with_desc) == 0
            assert end(n, not with_desc) != 0                # the other descriptor choice
            assert b"matching" in lib.sdvl_last_error(ctx.h)
            assert lib.sdvl_filter_inputs_begin(ctx.h, n, handles(frames), cap, with_desc) == 0
            assert end(n - 1, bool(with_desc)) != 0          # another number of frames
            check_inputs(orc, ctx.filter_inputs(frames, cap, bool(with_desc)), cases, bool(with_desc))
        assert lib.sdvl_filter_inputs_begin(ctx.h, n, handles(frames), cap, 1) == 0
        assert end(n, True) == 0 and counts.tolist() == [len(c[1]) for c in cases]
        assert np.array_equal(xyl[1, :counts[1]], cases[1][1])
    finally:
        for f in frames:
            f.close()


# ------------------------------------------------------------------------------------------------ 5. the search's threshold
@pytest.mark.parametrize("describe", [True, False], ids=["descriptors-in-hbm", "descriptors-on-demand"])
def test_search_threshold_one_bit_at_a_time(ctx, sdvl, orc, synth, describe):
    """2048 requests whose descriptors lie at Hamming distance 99 and 100 from their corner's, the 100th bit at every position of the
    256: one wrong descriptor bit or a misplaced nibble turns a match into a miss or a miss into a match"""
    from oraclelib import fill_search_reqs
    c = cc.search_bit_case(orc, synth)
    want = cc.search_bit_wants(orc, c)
    f_ref, f_cur = ctx.frame(c["img_ref"]), ctx.frame(c["img_cur"])
    try:
        f_cur.set_corners(c["ccur"])
        if describe:
            ctx.orb_describe([f_cur], want=False)
        reqs = fill_search_reqs(sdvl, c["meta"], f_ref, f_cur, c["T_ref"], c["T_cur"], True)
        res = ctx.search_points(reqs, sdvl.Camera(640, 480, *c["cam"]), sdvl.default_search_params())
    finally:
        f_ref.close(); f_cur.close()
    bad = [(k, (r.stage, r.best_corner, r.found, tuple(r.px)), (w["stage"], w["best_corner"], w["found"], tuple(w["px"])))
           for k, (r, w) in enumerate(zip(res, want))
           if (r.stage, r.best_corner, r.found, tuple(r.px)) != (w["stage"], w["best_corner"], w["found"], tuple(w["px"]))]
    assert not bad, (len(bad), bad[:4])
    assert all(w["stage"] >= 2 for w in want[0::2]) and all(w["stage"] == 1 for w in want[1::2])
