"""tests/corner_cases.py hits what it claims: asserted on the oracle alone, without a GPU.  tests/test_gpu_corners.py then holds the device to
the oracle on the same inputs."""
import numpy as np
import pytest

import corner_cases as cc


# ------------------------------------------------------------------------------------------------ 1. chosen points
@pytest.mark.parametrize("name", sorted(cc.NOISE))
def test_shi_tomasi_lists_hold_both_sides_of_the_limit_at_every_level(orc, name):
    img = cc.noise_image(name)
    pyr = cc.pyramid_of(orc, img)
    assert [p.shape for p in pyr] == cc.level_shapes(*img.shape)
    xyl = cc.shi_points(name)
    want = cc.shi_want(orc, pyr, xyl)
    for l, (H, W) in enumerate(cc.level_shapes(*img.shape)):
        m = xyl[:, 2] == l
        inside = np.array([cc.shi_inside(x, y, W, H) for x, y, _ in xyl[m]])
        assert np.all(want[m][~inside] == 0.0) and np.all(want[m][inside] > 0.0)          # the limit is where the restatement says
        assert (~inside).sum() >= 4
        if name == "P" and l == 4:
            assert (H, W) == (6, 8) and not inside.any()
        else:
            assert inside.sum() >= 4, (name, l)
    if name == "P":
        assert [w for _, w in cc.level_shapes(*img.shape)] == [131, 65, 32, 16, 8]


def test_shi_tomasi_wave_list_runs_through_all_sixteen_patterns(orc):
    xyl = cc.shi_wave_list()
    h, w, _ = cc.NOISE["P"]
    want = cc.shi_want(orc, cc.pyramid_of(orc, cc.noise_image("P")), xyl)
    inside = np.array([cc.shi_inside(x, y, w, h) for x, y, _ in xyl])
    assert np.array_equal(inside, want > 0.0) and len(xyl) == 65 == max(cc.SHI_WAVE_LENGTHS)
    patterns = {tuple(inside[4 * g:4 * g + 4]) for g in range(16)}
    assert len(patterns) == 16


@pytest.mark.parametrize("name", sorted(cc.NOISE))
def test_orb_lists_hold_both_sides_of_the_limits(orc, name):
    img = cc.noise_image(name)
    pyr = cc.pyramid_of(orc, img)
    xyl = cc.orb_points(name)
    desc, ang = cc.orb_want(orc, pyr, xyl)
    empty_levels = []
    for l, (H, W) in enumerate(cc.level_shapes(*img.shape)):
        m = xyl[:, 2] == l
        inside = np.array([cc.orb_inside(x, y, W, H) for x, y, _ in xyl[m]])
        assert m.sum() >= 3 and (~inside).sum() >= 3
        assert np.all(ang[m][~inside] == -1.0) and not desc[m][~inside].any()
        assert np.all(ang[m][inside] >= 0.0) and np.all(desc[m][inside].any(axis=1))
        if W >= 39 and H >= 39:
            assert inside.sum() >= 9          # the four corners of the inside set and the interior points
        else:
            empty_levels.append(l)
    assert empty_levels == {"P": [2, 3, 4], "Q": [4], "R": [4]}[name]
    if name == "Q":      # level 3 is 40 x 41: the inside set is x in {19, 20, 21}, y in {19, 20}
        assert pyr[3].shape == (40, 41)
        m = xyl[:, 2] == 3
        ins = [(x, y) for x, y, _ in xyl[m] if cc.orb_inside(x, y, 41, 40)]
        assert set(ins) <= {(x, y) for x in (19, 20, 21) for y in (19, 20)} and {(19, 19), (21, 20)} <= set(ins)
    if name == "R":
        assert pyr[3].shape == (60, 80) and pyr[4].shape == (30, 40)


def test_orb_ramps_have_the_angles_they_are_built_for(orc):
    ramps = cc.ramp_images()
    assert sorted(ramps) == sorted(cc.RAMP_ANGLES)
    for name, img in ramps.items():
        assert img.shape == (64, 80)
        pyr = cc.pyramid_of(orc, img, cc.RAMP_LEVELS)
        for x, y, l in cc.RAMP_POINTS:
            assert cc.orb_inside(x, y, 80, 64) and l == 0
        desc, ang = cc.orb_want(orc, pyr, cc.RAMP_POINTS)
        a = float(ang[0])                                   # at (30, 30)
        if name in cc.RAMP_AXIS:
            assert a == cc.RAMP_ANGLES[name], (name, a)       # a quadrant boundary, exactly
        elif name in cc.RAMP_DIAGONAL:
            assert abs(a - cc.RAMP_ANGLES[name]) <= 0.02, (name, a)      # |m10| == |m01|: the `ax >= ay` branch of cv::fastAtan2
        elif name == "77":
            assert np.all(ang == 0.0) and not desc.any()    # told apart from "outside" by the angle alone
        if name != "77":
            assert np.all(desc.any(axis=1))


# ------------------------------------------------------------------------------------------------ 2. batches
def test_batch_frames_mix_sizes_lengths_and_sides(orc):
    assert max(cc.BATCH_SIZES) == 17
    inside_shi = outside_shi = inside_orb = outside_orb = 0
    for k in range(17):
        img, xyl = cc.batch_frame(k)
        assert img.shape == ((99, 131) if k % 2 == 0 else (120, 160)) and len(xyl) == cc.BATCH_LENGTHS[k % 8]
        for x, y, l in xyl:
            H, W = img.shape[0] >> l, img.shape[1] >> l
            inside_shi += cc.shi_inside(x, y, W, H); outside_shi += not cc.shi_inside(x, y, W, H)
            inside_orb += cc.orb_inside(x, y, W, H); outside_orb += not cc.orb_inside(x, y, W, H)
    assert min(inside_shi, outside_shi, inside_orb, outside_orb) >= 50


# ------------------------------------------------------------------------------------------------ 3. selection
def test_the_reference_keeps_the_last_of_equal_scores(orc):
    """the issue's own example: a point listed twice wins with its last occurrence"""
    img = cc.noise(5, 96, 128)
    corners = np.array([(40, 40, 0), (41, 41, 0), (40, 40, 0), (70, 40, 0), (70, 40, 0)], np.int32)
    assert cc.oracle_filter(orc, img, corners).tolist() == [2, 4]
    assert cc.oracle_filter(orc, img, corners[[1, 0, 2, 3, 4]]).tolist() == [2, 4]


@pytest.mark.parametrize("form", sorted(cc.FORMS))
def test_selection_cases_take_their_form_and_hold_ties_and_full_bins(orc, form):
    c = cc.selection_case(orc, form)
    corners, cell, gw = c["corners"], c["cell"], c["gw"]
    h, w = c["img"].shape
    assert cc.select_form(c["n_cells"], len(corners)) == form and len(corners) <= 6144
    if form == "large":
        assert len(corners) > 2048 and c["n_cells"] <= 512       # the corner count alone takes it out of the small form
    elif form == "unbinned":
        assert c["n_cells"] == 2080
    elif form == "four-slot":
        assert c["n_cells"] == 4800
    kept = cc.oracle_filter(orc, c["img"], corners, cell=cell)
    assert len(kept) > 10
    elig = cc.is_eligible(corners, h, w)
    cells = np.where(elig, cc.cell_of(corners, cell, gw), -1)
    scores = cc.shi_want(orc, cc.pyramid_of(orc, c["img"]), corners)
    assert sorted(c["counted"].values()) == sorted(cc.FORMS[form][4])
    slots = 4 if form == "four-slot" else 10
    assert {k - slots for k in c["counted"].values()} >= {-1, 0, 1}          # below, at and above the bins' capacity
    for cl, k in c["counted"].items():
        members = np.nonzero(cells == cl)[0]
        assert len(members) == k
        assert np.argmax(scores[members]) == k - 1 and members[-1] in kept        # the winner is the cell's last entry
    for cl, occ in c["ties"].items():
        members = np.nonzero(cells == cl)[0]
        assert len(members) == 2 * len(occ) - 1
        assert all(tuple(corners[i]) == tuple(corners[occ[0]]) for i in occ)
        assert all(b - a > 1 for a, b in zip(occ, occ[1:]))                         # not adjacent in the list
        s = scores[occ[0]]
        assert s != int(s) and s == scores[members].max()
        assert occ[-1] in kept and not set(occ[:-1]) & set(kept.tolist())           # the LAST occurrence
    assert sorted(len(o) for o in c["ties"].values()) == [2, 3]
    # cells of other sizes too: emptier than a bin, and (where the grid is coarse) fuller
    sizes = np.bincount(cells[cells >= 0])
    assert (sizes == 1).any() or form in ("small", "large")
    assert (sizes[sizes > 0] <= slots).any() and (sizes > slots).any()


def test_threshold_case_sits_on_the_score_threshold(orc):
    c = cc.threshold_case(orc)
    assert c["A"] in (12, 13, 14) and abs(c["img"].astype(int) - 128).max() == c["A"]
    kept = cc.oracle_filter(orc, c["img"], c["corners"], cell=c["cell"])
    assert 4 * len(kept) >= c["n_cells"] and 4 * (c["n_cells"] - len(kept)) >= c["n_cells"]
    assert c["near"] >= 5
    assert cc.select_form(-(-128 // c["cell"]) * -(-96 // c["cell"]), len(c["corners"])) == "large"
    # a score in (50, 51) alone in its cell is dropped at 50 and kept at 0
    gw = -(-128 // c["cell"])
    cells = cc.cell_of(c["corners"], c["cell"], gw)
    lone = [i for i in np.nonzero((c["scores"] > 50) & (c["scores"] < 51))[0] if (c["scores"][cells == cells[i]] < 51).all()]
    assert lone and not set(lone) & set(kept.tolist())
    kept0 = cc.oracle_filter(orc, c["img"], c["corners"], cell=c["cell"], min_score=0)
    assert len(kept0) > len(kept)
    assert len(cc.oracle_filter(orc, c["img"], c["corners"], cell=c["cell"], min_score=c["above"])) == 0


def test_margin_case_reaches_locked_cells_and_the_last_row_and_column(orc):
    c = cc.margin_case(orc)
    corners, cell, gw, gh = c["corners"], c["cell"], c["gw"], c["gh"]
    h, w = c["img"].shape
    for l in range(3):
        for x in (18, 19, (w >> l) - 20, (w >> l) - 19):
            for y in (18, 19, (h >> l) - 20, (h >> l) - 19):
                assert (corners == (x, y, l)).all(axis=1).any()
    for margin, use_orb in ((19, 1), (5, 0)):
        first, locked = c[margin]["first"], c[margin]["locked"]
        second = cc.oracle_filter(orc, c["img"], corners, locked, cell=cell, use_orb=use_orb)
        assert len(first) > 10 and len(second) < len(first) and set(second.tolist()) < set(first.tolist())      # locking changes the result
        locked_cells = {int(y / cell) * gw + int(x / cell) for x, y in locked}
        elig = cc.is_eligible(corners, h, w, margin)
        cells = cc.cell_of(corners, cell, gw)
        for l in (0, 1, 2):
            m = elig & (corners[:, 2] == l)
            assert m.sum() >= 10
            assert np.isin(cells[m], list(locked_cells)).any(), (margin, l)        # corners of this level in a locked cell
            if margin == 5 and l > 0:
                assert (cells[m] % gw == gw - 1).any() and (cells[m] // gw == gh - 1).any()       # last column, last row
        if margin == 5:
            pyr_shapes = cc.level_shapes(h, w)
            outside = [i for i in first if not cc.orb_inside(corners[i, 0], corners[i, 1], pyr_shapes[corners[i, 2]][1], pyr_shapes[corners[i, 2]][0])]
            assert len(outside) >= 5          # kept corners whose descriptor is zeros


def test_selection_batch_and_inputs_frames(orc):
    frames = cc.selection_batch()
    assert len(frames) == 9 and len(frames[4][1]) == 0 and len(frames[6][2]) == 0
    assert len({f[0].shape for f in frames}) == 1
    n_kept = [len(cc.oracle_filter(orc, img, xyl, locked)) for img, xyl, locked in frames]
    assert n_kept[4] == 0 and min(n_kept[:4] + n_kept[5:]) >= 3
    changed = sum(len(cc.oracle_filter(orc, img, xyl)) != k for (img, xyl, locked), k in zip(frames, n_kept))
    assert changed >= 4                         # the lock masks matter
    counts = [len(x) for _, x in cc.inputs_frames(9)]
    assert 0 in counts and len(set(counts)) == 9 and max(counts) == 150


def test_device_count_frame_has_more_corners_than_the_launch_bound(orc):
    corners = orc.detect_pyramid(cc.device_count_image(), nfeatures=cc.DEVICE_COUNT_FEATURES)
    assert 1280 < len(corners) <= 6144, len(corners)
    kept = cc.oracle_filter(orc, cc.device_count_image(), corners)
    assert (kept >= 1280).sum() >= 20 and (kept < 1280).sum() >= 20          # corners beyond the bound decide cells


# ------------------------------------------------------------------------------------------------ 5. the search's threshold
def test_search_bit_case_straddles_the_threshold(orc, synth):
    """every A_i (distance 99) is matched to the same corner, every B_i (distance 100) stops at the match: checked here for the 512
    requests of the first base request; tests/test_gpu_corners.py computes the oracle's answer to all 2048 anyway"""
    c = cc.search_bit_case(orc, synth)
    assert len(c["base"]) == 4 and len(c["meta"]) == 2048
    for b, base in enumerate(c["base"]):
        for i in (0, 100, 157, 255):
            a, bb = c["meta"][512 * b + 2 * i]["desc"], c["meta"][512 * b + 2 * i + 1]["desc"]
            assert orc.orb_distance(a, base["D"]) == 99 and orc.orb_distance(bb, base["D"]) == 100
            assert int(np.unpackbits(a ^ bb).sum()) == 1 and (a ^ bb)[i >> 3] == 1 << (i & 7)
    j = c["base"][0]["want"]["best_corner"]
    for k, m in enumerate(c["meta"][:512]):
        want = cc.search_want(orc, c, m)
        if k % 2 == 0:
            assert want["stage"] >= 2 and want["best_corner"] == j, k
        else:
            assert want["stage"] == 1 and want["best_corner"] == -1 and want["found"] == 0, k
            assert np.array_equal(want["px"], m["px0"])
