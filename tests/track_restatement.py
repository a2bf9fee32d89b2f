"""The bookkeeping of one tracked frame, restated from the reference's statements as a plain sequential loop: what
FeatureAlign::ProjectPoints / ProjectPoint / SelectPoints / RemoveOutliers (feature_align.cc:88-150, 245-256, 296-339), Frame::Project and
Frame::GetSceneDepth (frame.cc:70-103), Point::Promote / Unpromote (point.cc:103-116) and the deferred Map::DeletePoint do to the points
and to the new frame's feature list.  Python floats (IEEE doubles, one rounding per operation, in the order the statements are written)
and Python lists; no keys, no prefix sums, no ballots.  The search and the pose estimation are callables: the CPU tests script them,
the GPU tests feed them the oracle's answers.

This is the specification tests/test_gpu_track_tables.py holds csrc/sdvl_track.hip to.  Test infrastructure only."""
import math
from collections import Counter

# Point::PointStatus (point.h) in the status byte; above it the two bits the tables add
P_FOUND, P_NOT_FOUND, P_SEEN, P_UNSEEN = 0, 1, 2, 3
DELETED = 0x100      # Point::ToDelete()
TRASH = 0x200        # deleted by the mapper during the previous frame's update: the queue is emptied after this frame has been tracked
KEEP = DELETED | TRASH
DUPLICATE = 0x40000000   # feature flag: an earlier feature of the list has the same point


class Point:
    __slots__ = ("P", "score", "n_failed", "last_frame", "status")

    def __init__(self, P, score=0, n_failed=0, last_frame=-1, status=P_FOUND):
        self.P = (float(P[0]), float(P[1]), float(P[2]))
        self.score, self.n_failed, self.last_frame, self.status = int(score), int(n_failed), int(last_frame), int(status)

    def copy(self):
        return Point(self.P, self.score, self.n_failed, self.last_frame, self.status)

    def stat(self):
        return (self.score, self.n_failed, self.last_frame, self.status)


class Feature:
    __slots__ = ("px", "level", "point")

    def __init__(self, px, level, point):
        self.px, self.level, self.point = (float(px[0]), float(px[1])), int(level), int(point)


def set_status(p, status):
    """Point::SetStatus: the status byte; the bits above it survive"""
    p.status = (p.status & ~0xFF) | status


# ---- extra/se3: unit quaternion (w, x, y, z) and translation
def rotation(q):
    """Eigen::Quaterniond::toRotationMatrix"""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return ((1.0 - (tyy + tzz), txy - twz, txz + twy),
            (txy + twz, 1.0 - (txx + tzz), tyz - twx),
            (txz - twy, tyz + twx, 1.0 - (txx + tyy)))


def rotate(R, v):
    return tuple(R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3))


def relative_pos(pose, P):
    """Frame::GetRelativePos: pose * P"""
    r = rotate(rotation(pose[:4]), P)
    return (r[0] + pose[4], r[1] + pose[5], r[2] + pose[6])


def se3_mul(a, b):
    """SE3::operator* (extra/se3.cc:166-177): the product quaternion is normalised"""
    w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3]
    x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2]
    y = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3]
    z = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]
    n = math.sqrt(w * w + x * x + y * y + z * z)
    r = rotate(rotation(a[:4]), b[4:7])
    return (w / n, x / n, y / n, z / n, a[4] + r[0], a[5] + r[1], a[6] + r[2])


def _div(a, b):
    """a / b as IEEE 754 has it (Python raises where C++ gives an infinity or a NaN)"""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return float("nan")
    return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def project(cam, rel):
    """Camera::Project"""
    return (cam["u0"] + _div(cam["fx"] * rel[0], rel[2]), cam["v0"] + _div(cam["fy"] * rel[1], rel[2]))


def unproject(cam, px):
    """Camera::Unproject: the unit bearing of a pixel"""
    v = ((px[0] - cam["u0"]) / cam["fx"], (px[1] - cam["v0"]) / cam["fy"], 1.0)
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / n, v[1] / n, v[2] / n)


def is_inside_image(cam, x, y, m):
    """Camera::IsInsideImage(p.cast<int>(), m), camera.h:93-95"""
    return x >= m and x < cam["width"] - m and y >= m and y < cam["height"] - m


def grid_width(cam, cell_size):
    return int(math.ceil(cam["width"] / cell_size))


def grid_cells(cam, cell_size):
    return grid_width(cam, cell_size) * int(math.ceil(cam["height"] / cell_size))


# ---- feature_align.cc:296-339
def project_points(pose, features, points, frame_id, cam, cell_size, patch, trace=None):
    """ProjectPoints: -> grid, a list per cell of (point index, projection) in the order the feature list names them"""
    trace = Counter() if trace is None else trace
    gw = grid_width(cam, cell_size)
    grid = [[] for _ in range(grid_cells(cam, cell_size))]
    for f in features:
        if f.point < 0:                     # !point
            trace["feature-without-point"] += 1
            continue
        if f.point & DUPLICATE:             # the same Point object again: its last_frame is already this frame's
            trace["duplicate-feature"] += 1
            continue
        p = points[f.point]
        if p.status & DELETED:              # point->ToDelete()
            trace["deleted-point"] += 1
            continue
        if frame_id == p.last_frame:        # already projected in this frame
            trace["last-frame-is-this-frame"] += 1
            continue
        # ProjectPoint
        rel = relative_pos(pose, p.P)
        if rel[2] < 0.0:                    # Frame::Project: behind the camera
            set_status(p, P_UNSEEN)
            trace["behind-camera"] += 1
        else:
            px = project(cam, rel)
            # (a point ON the camera plane, z = 0, is not behind it and projects to an infinity or a NaN: p.cast<int>() of those is
            #  undefined in C++, and every conversion in use gives INT_MIN, INT_MAX or 0, none of them inside a margin of a pixel or more)
            if not (math.isfinite(px[0]) and math.isfinite(px[1])) or not is_inside_image(cam, int(px[0]), int(px[1]), patch):
                set_status(p, P_UNSEEN)
                trace["outside-margin"] += 1
            else:
                k = int(px[1] / cell_size) * gw + int(px[0] / cell_size)
                grid[k].append((f.point, px))
                set_status(p, P_SEEN)
                trace["seen"] += 1
        if p.status & TRASH:
            trace["trash-seen" if (p.status & 0xFF) == P_SEEN else "trash-unseen"] += 1
        p.last_frame = frame_id             # not relocalising
    return grid


# ---- feature_align.cc:99-149
def select_points(grid, cell_order, max_matches, max_failed, search, points, trace=None):
    """SelectPoints behind ProjectPoints, cells in the given (already shuffled) order.  search(point index, px0) -> (found, px, level).
    -> (new features, matches, attempts, points deleted)"""
    trace = Counter() if trace is None else trace
    found_features = []
    matches = attempts = deleted = 0
    for visited, c in enumerate(cell_order):
        if not matches < max_matches:
            if any(grid[d] for d in cell_order[visited:]):
                trace["cap-reached-before-the-last-cell"] += 1
            break
        cell = sorted(grid[c], key=lambda e: -points[e[0]].score)      # list::sort(CompareQuality) is stable
        if any(points[a[0]].score == points[b[0]].score for a, b in zip(cell, cell[1:])):
            trace["equal-scores-in-a-cell"] += 1
        found = False
        tried = 0
        for pt, px0 in cell:
            if found:
                break
            p = points[pt]
            if p.status & DELETED:
                continue
            attempts += 1
            tried += 1
            found, px, level = search(pt, px0)
            if found:
                p.score += 1            # Point::Promote
                p.n_failed = 0
                found_features.append(Feature(px, level, pt))
                set_status(p, P_FOUND)
                matches += 1
                trace["hit"] += 1
                if tried > 1:
                    trace["hit-behind-a-miss"] += 1
            else:
                p.n_failed += 1         # Point::Unpromote
                if p.n_failed > max_failed:
                    p.status |= DELETED     # Map::DeletePoint
                    deleted += 1
                    trace["deleted-beyond-max-failed"] += 1
                elif p.n_failed == max_failed:
                    trace["miss-at-max-failed"] += 1
                set_status(p, P_NOT_FOUND)
                trace["miss"] += 1
        if cell and not found:
            trace["cell-of-misses"] += 1
    if matches == max_matches and matches > 0:
        trace["cap-reached"] += 1
    return found_features, matches, attempts, deleted


# ---- feature_align.cc:245-256
def remove_outliers(features, outlier_indices, points, trace=None):
    trace = Counter() if trace is None else trace
    for i in outlier_indices:
        f = features[i]
        if f.point < 0:
            continue
        p = points[f.point]
        f.point = -1
        set_status(p, P_NOT_FOUND)
        trace["outlier"] += 1


# ---- frame.cc:70-92, extra/utils.cc:215-220
def scene_depth(pose, features, points, trace=None):
    """-> (median depth, index of the feature it belongs to or -1): nth_element at n / 2"""
    trace = Counter() if trace is None else trace
    depth = []
    for i, f in enumerate(features):
        if f.point < 0:
            continue
        depth.append((relative_pos(pose, points[f.point].P)[2], i))
    if not depth:
        trace["no-depth"] += 1
        return 0.0, -1
    trace["median-of-even" if len(depth) % 2 == 0 else "median-of-odd"] += 1
    depth.sort()
    return depth[len(depth) // 2]


def end_of_step(points, trace=None):
    """the map's deletion queue is emptied after the frame has been tracked (sdvl.cc:127)"""
    trace = Counter() if trace is None else trace
    for p in points:
        if p.status & TRASH:
            p.status = (p.status & ~TRASH) | DELETED
            trace["trash-becomes-deleted"] += 1


def observations(cam, features, points):
    """what SelectInliers / OptimizePose read of the selected features: rows ax, ay, X, Y, Z, level"""
    obs = []
    for f in features:
        v = unproject(cam, f.px)
        P = points[f.point].P
        obs.append([v[0] / v[2], v[1] / v[2], P[0], P[1], P[2], f.level])
    return obs


def step(points, features, T, last_pose, frame_id, max_matches, cell_order, cam, cell_size, patch, max_failed, search, pose, trace=None,
         final_pose=None):
    """One tracked frame.  points are changed in place.  pose(start pose, observation rows) -> dict(pose, n_draws, inliers, outliers,
    refined).  final_pose, where given, is the pose the scene depth is restated from (the device's own) instead of pose()'s.
    -> (result dict, new feature list, point statistics rows)"""
    trace = Counter() if trace is None else trace
    start = se3_mul(T, last_pose)       # frame2.pose = T * frame1.pose, image_align.cc:79
    grid = project_points(start, features, points, frame_id, cam, cell_size, patch, trace)
    n_requests = sum(len(c) for c in grid)
    new, matches, attempts, deleted = select_points(grid, cell_order, max_matches, max_failed, search, points, trace)
    obs = observations(cam, new, points)
    est = pose(start, obs)
    remove_outliers(new, est["outliers"], points, trace)
    if new and len(est["outliers"]) == len(new):
        trace["every-match-an-outlier"] += 1
    depth, depth_feature = scene_depth(tuple(est["pose"]) if final_pose is None else tuple(final_pose), new, points, trace)
    end_of_step(points, trace)
    result = dict(start_pose=start, pose=tuple(est["pose"]), scene_depth=depth, scene_depth_feature=depth_feature, n_features=len(features),
                  n_requests=n_requests, matches=matches, attempts=attempts, n_draws=int(est["n_draws"]), n_inliers=len(est["inliers"]),
                  n_outliers=len(est["outliers"]), refined=int(est["refined"]), n_points=sum(1 for f in new if f.point >= 0),
                  n_deleted=deleted, inliers=[int(i) for i in est["inliers"]], outliers=[int(i) for i in est["outliers"]], observations=obs)
    return result, new, [p.stat() for p in points]
