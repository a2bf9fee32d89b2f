"""tests/depth_lookup_restatement.py against depth_seed_restatement where the two meet, and the cases of tests/depth_lookup_cases.py
against what they are for.  No GPU."""
import numpy as np

import depth_lookup_cases as lc
import depth_lookup_restatement as dl
import depth_seed_restatement as dsr

CAM4 = (lc.CAM["fx"], lc.CAM["fy"], lc.CAM["u0"], lc.CAM["v0"])


def test_at_whole_level_coordinates_it_is_depth_seeding():
    f, u = lc.images()
    rng = np.random.default_rng(3)
    xyl = np.array([(rng.integers(0, lc.W >> l), rng.integers(0, lc.H >> l), l) for l in (0, 1, 2) for _ in range(60)], np.int32)
    px = xyl[:, :2].astype(np.float64) * (1 << xyl[:, 2])[:, None]
    for img, scale in ((f, 1.0), (u, lc.U16_SCALE)):
        for dist in (None, lc.LENS):
            z, st, ok = dl.depth_lookup([(img, 0, len(px), scale)], px, xyl[:, 2], lc.CAM, dist)
            z2, st2, _ = dsr.depth_seed(img, xyl, CAM4, dist, scale)
            assert np.array_equal(st, st2) and z.tobytes() == np.asarray(z2, np.float64).tobytes()
            assert ok[0] == (st == dl.OK).sum() > 60


def test_positions_reach_every_status_at_every_level():
    f, u = lc.images()
    px, lv = lc.positions()
    z, st, ok = dl.depth_lookup([(f, 0, len(px) - 5), (u, len(px) - 5, len(px) - 2, lc.U16_SCALE)], px, lv, lc.CAM)
    for level in (0, 1, 2):
        assert set(st[lv == level]) >= {dl.OK, dl.HOLE, dl.FEW, dl.EDGE, dl.OUTSIDE}, level
    assert (z[st != dl.OK] == 0).all() and (z[st == dl.OK] > 1.9).all()
    # the centre rounds half up: -0.5 is column 0, -0.51 is off the image
    i = [k for k in range(len(px)) if tuple(px[k]) == (-0.5, 10.0)][0]
    assert st[i] != dl.OUTSIDE and st[i + 1] == dl.OUTSIDE
    # the step is an edge only at the stride that reaches it
    at = {(tuple(px[k]), int(lv[k])): int(st[k]) for k in range(len(px))}
    assert at[((38.0, 10.0), 0)] == dl.OK and at[((38.0, 10.0), 1)] == dl.OK and at[((38.0, 10.0), 2)] == dl.EDGE
    assert at[((40.0, 10.0), 0)] == dl.EDGE
    assert list(st[-2:]) == [dl.HOLE, dl.HOLE] and st[-3] == dl.OUTSIDE      # in no job; not finite
    assert ok.sum() == (st == dl.OK).sum()
