"""tests/track_restatement.py on hand-written micro-cases whose answers are written out here, with a scripted search and a scripted
pose; and tests/track_cases.py: every case of the GPU module is what it claims to be (no GPU, the oracle's cached answers only)."""
from collections import Counter

import pytest

import track_restatement as tr
from track_restatement import DELETED, DUPLICATE, P_FOUND, P_NOT_FOUND, P_SEEN, P_UNSEEN, TRASH, Feature, Point

CAM = dict(width=640.0, height=480.0, fx=512.0, fy=512.0, u0=320.0, v0=240.0)
ID = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
CELL, PATCH, MAX_FAILED = 32, 8, 15


def at(u, v, z=2.0, **kw):
    """a point that projects exactly onto pixel (u, v) from the identity pose: every step of the projection is exact in binary"""
    return Point(((u - 320.0) / 512.0 * z, (v - 240.0) / 512.0 * z, z), **kw)


def cell(u, v):
    return (v // 32) * 20 + u // 32


def scripted(answers):
    calls = []

    def search(pt, px0):
        calls.append((pt, px0))
        return answers[pt]
    return search, calls


def keep_pose(outliers=()):
    def pose(start, obs):
        out = [i for i in outliers if i < len(obs)]
        return dict(pose=start, n_draws=3, inliers=[i for i in range(len(obs)) if i not in out], outliers=out, refined=1)
    return pose


def run(points, features, order, search, max_matches=100, frame_id=7, pose=None, trace=None):
    return tr.step(points, features, ID, ID, frame_id, max_matches, order, CAM, CELL, PATCH, MAX_FAILED, search, pose or keep_pose(), trace)


def test_projection_is_exact_and_the_grid_is_the_references():
    assert tr.grid_width(CAM, CELL) == 20 and tr.grid_cells(CAM, CELL) == 300
    for u, v in ((8, 8), (100, 200), (631, 471), (352, 96)):
        p = at(u, v)
        assert tr.project(CAM, tr.relative_pos(ID, p.P)) == (float(u), float(v))
    assert tr.se3_mul(ID, ID) == ID
    q = (0.5, 0.5, 0.5, 0.5)      # x -> y -> z -> x
    assert tr.rotate(tr.rotation(q), (1.0, 2.0, 3.0)) == (3.0, 1.0, 2.0)


def test_three_cells_with_a_cap_of_two():
    points = [at(40, 40, score=1), at(200, 40, score=2), at(400, 300, score=3)]
    feats = [Feature((0, 0), 0, i) for i in range(3)]
    cells = [cell(40, 40), cell(200, 40), cell(400, 300)]
    assert cells == [21, 26, 192]
    search, calls = scripted({0: (True, (41.5, 40.25), 0), 1: (True, (201.0, 39.0), 1), 2: (True, (399.0, 301.0), 2)})
    order = [192, 21, 26] + [c for c in range(300) if c not in cells]
    trace = Counter()
    res, new, stats = run(points, feats, order, search, max_matches=2, trace=trace)
    assert [c[0] for c in calls] == [2, 0] and calls[0][1] == (400.0, 300.0) and calls[1][1] == (40.0, 40.0)
    assert (res["matches"], res["attempts"], res["n_requests"], res["n_features"], res["n_points"], res["n_deleted"]) == (2, 2, 3, 3, 2, 0)
    assert [(f.px, f.level, f.point) for f in new] == [((399.0, 301.0), 2, 2), ((41.5, 40.25), 0, 0)]
    # score, n_failed, last_frame, status: the point of the cell that was never visited stays seen
    assert stats == [(2, 0, 7, P_FOUND), (2, 0, 7, P_SEEN), (4, 0, 7, P_FOUND)]
    assert trace["cap-reached-before-the-last-cell"] == 1 and trace["hit"] == 2
    assert res["scene_depth"] == 2.0


@pytest.mark.parametrize("flip", [False, True])
def test_a_tie_keeps_list_order_and_the_cell_stops_at_its_first_hit(flip):
    # one cell: scores 5, 7, 5.  Visiting order: the 7, then the two 5s as the FEATURE LIST names them
    points = [at(100, 100, score=5), at(101, 101, score=7), at(102, 102, score=5, n_failed=3), at(500, 400, score=0)]
    feats = [Feature((0, 0), 0, i) for i in ((2, 1, 0, 3) if flip else (0, 1, 2, 3))]
    first, second = (2, 0) if flip else (0, 2)
    search, calls = scripted({1: (False, (0, 0), -1), first: (True, (100.5, 100.5), 1), second: (True, (9.0, 9.0), 0), 3: (False, (0, 0), -1)})
    trace = Counter()
    res, new, stats = run(points, feats, list(range(300)), search, trace=trace)
    assert [c[0] for c in calls] == [1, first, 3]
    assert (res["matches"], res["attempts"], res["n_requests"]) == (1, 3, 4)
    assert [(f.point, f.level) for f in new] == [(first, 1)]
    want = {1: (7, 1, 7, P_NOT_FOUND), first: (6, 0, 7, P_FOUND), second: (5, 3 if second == 2 else 0, 7, P_SEEN), 3: (0, 1, 7, P_NOT_FOUND)}
    assert stats == [want[i] for i in range(4)]
    assert trace["equal-scores-in-a-cell"] == 1 and trace["hit-behind-a-miss"] == 1 and trace["cell-of-misses"] == 1


def test_a_point_is_deleted_beyond_max_failed_and_not_at_it():
    points = [at(40, 40, n_failed=MAX_FAILED - 1), at(200, 40, n_failed=MAX_FAILED), at(400, 300, n_failed=MAX_FAILED + 1),
              at(400, 40, n_failed=MAX_FAILED, status=TRASH | P_FOUND)]
    feats = [Feature((0, 0), 0, i) for i in range(4)]
    search, _ = scripted({i: (False, (0, 0), -1) for i in range(4)})
    res, new, stats = run(points, feats, list(range(300)), search)
    assert (res["matches"], res["attempts"], res["n_deleted"], res["scene_depth"], res["n_points"]) == (0, 4, 3, 0.0, 0)
    assert new == []
    assert stats == [(0, MAX_FAILED, 7, P_NOT_FOUND), (0, MAX_FAILED + 1, 7, P_NOT_FOUND | DELETED),
                     (0, MAX_FAILED + 2, 7, P_NOT_FOUND | DELETED), (0, MAX_FAILED + 1, 7, P_NOT_FOUND | DELETED)]
    # the next frame does not look at them any more
    res, new, stats2 = run(points, feats, list(range(300)), search, frame_id=8)
    assert res["attempts"] == 1 and res["n_requests"] == 1 and res["n_deleted"] == 1
    assert stats2[1:] == stats[1:] and stats2[0] == (0, MAX_FAILED + 1, 8, P_NOT_FOUND | DELETED)


def test_who_is_projected_and_who_is_not():
    points = [at(100, 100, z=-1e-3),                      # just behind the camera
              at(100, 100, z=1e-3),                       # just in front
              at(7, 100), at(8, 100), at(631, 100), at(632, 100), at(100, 7), at(100, 8), at(100, 471), at(100, 472),    # the margin
              at(300, 300, status=DELETED | P_FOUND, last_frame=3),
              at(310, 300, status=TRASH | P_FOUND), at(2, 2, status=TRASH | P_FOUND),
              at(320, 300, last_frame=7),
              at(352, 96), at(351, 95),                    # on the corner of cell (3, 11) and just before it
              at(330, 300)]
    feats = [Feature((0, 0), 0, i) for i in range(len(points))] + [Feature((0, 0), 0, -1), Feature((0, 0), 0, 16 | DUPLICATE)]
    search, calls = scripted({i: (False, (0, 0), -1) for i in range(len(points))})
    trace = Counter()
    grid = tr.project_points(ID, feats, points, 7, CAM, CELL, PATCH, trace)
    status = [p.status for p in points]
    assert status == [P_UNSEEN, P_SEEN, P_UNSEEN, P_SEEN, P_SEEN, P_UNSEEN, P_UNSEEN, P_SEEN, P_SEEN, P_UNSEEN, DELETED | P_FOUND,
                      TRASH | P_SEEN, TRASH | P_UNSEEN, P_FOUND, P_SEEN, P_SEEN, P_SEEN]
    assert [p.last_frame for p in points] == [7] * 10 + [3] + [7] * 6
    where = {pt: k for k, c in enumerate(grid) for pt, _ in c}
    assert where == {1: 63, 3: 60, 4: 79, 7: 3, 8: 14 * 20 + 3, 11: 9 * 20 + 9, 14: 3 * 20 + 11, 15: 2 * 20 + 10, 16: 9 * 20 + 10}
    assert [pt for pt, _ in grid[9 * 20 + 10]] == [16]          # once, not twice: the duplicate feature is skipped
    assert dict(trace) == {"behind-camera": 1, "outside-margin": 5, "seen": 9, "deleted-point": 1, "trash-seen": 1, "trash-unseen": 1,
                           "last-frame-is-this-frame": 1, "feature-without-point": 1, "duplicate-feature": 1}
    tr.end_of_step(points)
    assert points[11].status == DELETED | P_SEEN and points[12].status == DELETED | P_UNSEEN and points[10].status == DELETED | P_FOUND


def test_outliers_lose_their_point_and_the_median_is_nth_element_at_half():
    for depths, outliers, want_depth, want_feature in (([3.0, 1.0, 4.0, 2.0], (), 3.0, 0),           # sorted 1 2 [3] 4
                                                       ([5.0, 1.0, 4.0, 2.0, 9.0], (), 4.0, 2),      # sorted 1 2 [4] 5 9
                                                       ([5.0, 1.0, 4.0, 2.0, 9.0], (2,), 5.0, 0),    # sorted 1 2 [5] 9
                                                       ([5.0, 1.0], (0, 1), 0.0, -1)):
        points = [at(40 + 64 * i, 40, z=z) for i, z in enumerate(depths)]
        feats = [Feature((0, 0), 0, i) for i in range(len(points))]
        search, _ = scripted({i: (True, (40.0 + 64 * i, 40.0), 0) for i in range(len(points))})
        trace = Counter()
        res, new, stats = run(points, feats, list(range(300)), search, pose=keep_pose(outliers), trace=trace)
        assert res["matches"] == len(depths) and res["n_outliers"] == len(outliers) and res["n_points"] == len(depths) - len(outliers)
        assert (res["scene_depth"], res["scene_depth_feature"]) == (want_depth, want_feature)
        assert [f.point for f in new] == [-1 if i in outliers else i for i in range(len(depths))]
        assert [s[3] for s in stats] == [P_NOT_FOUND if i in outliers else P_FOUND for i in range(len(depths))]
        assert [s[0] for s in stats] == [1] * len(depths)            # promoted all the same
        if len(outliers) == len(depths):
            assert trace["every-match-an-outlier"] == 1 and trace["no-depth"] == 1


def test_an_empty_frame():
    search, calls = scripted({})
    res, new, stats = run([], [], list(range(300)), search)
    assert (res["matches"], res["attempts"], res["n_requests"], res["n_features"], res["scene_depth"], res["n_points"]) == (0, 0, 0, 0, 0.0, 0)
    assert new == [] and stats == [] and calls == [] and res["pose"] == ID
    # and one whose features have no points
    res, new, stats = run([at(100, 100)], [Feature((0, 0), 0, -1)] * 3, list(range(300)), search)
    assert (res["matches"], res["n_requests"], res["n_features"]) == (0, 0, 3) and stats == [(0, 0, -1, P_FOUND)] and calls == []


def test_observation_rows_are_the_pose_stages():
    obs = tr.observations(CAM, [Feature((320.0 + 512.0, 240.0), 2, 0)], [at(100, 100)])
    assert len(obs) == 1 and abs(obs[0][0] - 1.0) < 1e-15 and obs[0][1] == 0.0 and obs[0][5] == 2 and tuple(obs[0][2:5]) == at(100, 100).P


# ---- the cases of the GPU module
def test_every_case_is_what_it_claims(orc, synth):
    import track_cases as tc
    scene = tc.scene(orc, synth)
    cases = tc.cases(scene)
    tc.check_cases(scene, cases)
    trace = tc.restated_trace(scene, cases)
    missing = [b for b in tc.BRANCHES if not trace[b]]
    assert not missing, missing
