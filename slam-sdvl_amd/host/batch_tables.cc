// batch_tables.cc — SDVLBatch's device-resident tracking tables: the counters that come back from them (SyncStats, SyncHostState), a
// tracker's last_frame as table rows (PointRow, BuildTable, AppendSeeds), their way to the device (GatherRows, UploadTables), the set
// itself (EnsureTrackSet) and when a table no longer holds what the host objects say (InvalidateStaleTables).
#include "batch_internal.h"

#include <algorithm>
#include <cstring>

namespace sdvl {

using std::shared_ptr;
using std::vector;

// The counters the device advanced (Promote / Unpromote / SetLastFrame / status) reach the Point objects.
void SDVLBatch::SyncStats(SDVL &t) {
  SDVL::TrackState &ts = t.track_;
  if (!ts.stats_dirty || !ts.points) return;
  const size_t n = std::min(ts.stats.size(), ts.points->size());
  for (size_t p = 0; p < n; p++) {
    const sdvl_track_point_stat &s = ts.stats[p];
    (*ts.points)[p]->SetTrackCounters(s.score, s.n_failed, s.last_frame, static_cast<Point::PointStatus>(s.status & 0xFF));
  }
  ts.stats_dirty = false;
}

void SDVLBatch::SyncHostState() {
  for (SDVL *t : trk_) {
    SyncStats(*t);
    if (t->last_frame_ && t->last_frame_->HasFlatFeatures()) t->last_frame_->GetFeatures();
  }
}

// a point, first observed as feature `init` of keyframe `ref`, as a table row (include/sdvl_hip.h: sdvl_track_point)
static inline void PointRow(Point *pt, Feature *init, Frame *ref, sdvl_track_point *row) {
  sdvl_track_point &tp = *row;
  const Vector3d P = pt->GetPosition();
  tp.position[0] = P(0); tp.position[1] = P(1); tp.position[2] = P(2);
  tp.px[0] = init->GetPosition()(0); tp.px[1] = init->GetPosition()(1);
  tp.bearing[0] = init->GetVector()(0); tp.bearing[1] = init->GetVector()(1); tp.bearing[2] = init->GetVector()(2);
  tp.idepth = pt->GetInverseDepth();
  tp.idepth_std = pt->GetStd();
  tp.ref = ref->device();
  tp.level = init->GetLevel();
  tp.fixed = pt->IsFixed() ? 1 : 0;
  tp.score = pt->Score();
  tp.n_failed = pt->GetFailed();
  tp.last_frame = pt->GetLastFrame();
  tp.status = static_cast<int32_t>(pt->GetStatus());
  if (init->HasDescriptor()) std::memcpy(tp.desc, init->DescriptorData().data(), 32);
  else std::memset(tp.desc, 0, 32);
}

// last_frame's features and the points behind them as table rows (include/sdvl_hip.h: sdvl_track_point / _feature).
// false: something the tables cannot express (a point without a first observation or whose keyframe is gone) — the step
// then runs on the host path.
bool SDVLBatch::BuildTable(SDVL &t) {
  SyncStats(t);
  vector<sdvl_track_point> *points = &t.track_.up_points;
  vector<sdvl_track_feature> *feats = &t.track_.up_feats;
  points->clear();
  feats->clear();
  t.track_.up_register.clear();
  vector<shared_ptr<Feature>> &features = t.last_frame_->GetFeatures();
  // the alignment stage takes at most SDVL_MAX_ALIGN_FEATURES features per job: a frame with more (a keyframe of configuration C
  // that has gathered matches + connections + candidates) goes through the host-driven step instead of failing the batch
  if (static_cast<int>(features.size()) > std::min(tables_.cap, static_cast<int>(SDVL_MAX_ALIGN_FEATURES))) return false;
  if (t.track_.points)
    for (const shared_ptr<Point> &old : *t.track_.points) old->SetTrackRow(-1);
  const int row_base = t.track_.slot * tables_.cap;
  auto table = std::make_shared<Frame::PointTable>();
  table->reserve(features.size());
  // a point may sit behind several features of a keyframe: ProjectPoints takes the first and skips the rest
  // (feature_align.cc:310: the point already carries this frame's id)
  struct Slot { Point *p; int idx; };
  static thread_local vector<Slot> hash;
  size_t hcap = 64;
  while (hcap < features.size() * 2) hcap *= 2;
  hash.assign(hcap, Slot{nullptr, -1});
  const size_t n_features = features.size();
  for (size_t fi = 0; fi < n_features; fi++) {
    // Feature -> Point -> first Feature -> keyframe: four dependent loads per row, asked for a few features ahead
    if (fi + 8 < n_features) __builtin_prefetch(features[fi + 8].get());
    if (fi + 4 < n_features && features[fi + 4]) {
      const Point *p4 = features[fi + 4]->GetPointRaw();
      __builtin_prefetch(p4);
      if (p4) __builtin_prefetch(reinterpret_cast<const char *>(p4) + 64);
    }
    if (fi + 2 < n_features && features[fi + 2]) {
      const Point *p2 = features[fi + 2]->GetPointRaw();
      if (p2) __builtin_prefetch(p2->GetInitFeatureRaw());
    }
    const shared_ptr<Feature> &ftp = features[fi];
    Feature *ft = ftp.get();
    sdvl_track_feature f;
    if (!ft) return false;
    f.px[0] = ft->GetPosition()(0); f.px[1] = ft->GetPosition()(1);
    f.bearing[0] = ft->GetVector()(0); f.bearing[1] = ft->GetVector()(1); f.bearing[2] = ft->GetVector()(2);
    f.level = ft->GetLevel();
    f.point = -1;
    Point *pt = ft->GetPointRaw();
    if (pt && !pt->ToDelete()) {
      size_t h = (reinterpret_cast<uintptr_t>(pt) >> 4) & (hcap - 1);
      while (hash[h].p && hash[h].p != pt) h = (h + 1) & (hcap - 1);
      if (hash[h].p) {
        f.point = hash[h].idx | SDVL_TRACK_DUPLICATE;
      } else {
        Feature *init = pt->GetInitFeatureRaw();
        Frame *ref = init ? init->GetFrameRaw() : nullptr;
        if (!init || !ref || ref->owner() != dev_) return false;
        const int idx = static_cast<int>(table->size());
        hash[h] = Slot{pt, idx};
        f.point = idx;
        table->push_back(ft->GetPoint());
        pt->SetTrackRow(row_base + idx);
        points->emplace_back();
        PointRow(pt, init, ref, &points->back());
        // a keyframe that never was the current frame of a tracked step (bootstrap, host-path steps): the caller registers
        // it (device calls of one context come from one thread)
        if (!ref->IsRegistered()) t.track_.up_register.push_back(ref);
      }
    }
    feats->push_back(f);
  }
  if (static_cast<int>(points->size()) > tables_.cap) return false;
  t.track_.points = table;
  t.track_.stats.clear();
  t.track_.stats_dirty = false;
  return true;
}

// The points PlaneMap::SeedFromFiltered has just put on keyframe `kf` (its object features from track_.first_seed on) as table rows
// behind the rows the tables hold: point index = position in the tracker's point table, which grows by the same points.
bool SDVLBatch::AppendSeeds(SDVL &t, const shared_ptr<Frame> &kf) {
  SDVL::TrackState &ts = t.track_;
  if (!ts.points) return false;
  ts.up_points.clear();
  ts.up_feats.clear();
  const vector<shared_ptr<Feature>> &objs = kf->ObjectFeatures();
  const int row_base = ts.slot * tables_.cap;
  if (static_cast<int>(ts.points->size() + (objs.size() - ts.first_seed)) > tables_.cap) return false;
  if (kf->NumFlatFeatures() + static_cast<int>(objs.size()) > std::min(tables_.cap, static_cast<int>(SDVL_MAX_ALIGN_FEATURES))) return false;
  if (kf->owner() != dev_ || !kf->IsRegistered()) return false;
  ts.up_points.reserve(objs.size() - ts.first_seed);
  ts.up_feats.reserve(objs.size() - ts.first_seed);
  for (size_t fi = ts.first_seed; fi < objs.size(); fi++) {
    Feature *ft = objs[fi].get();
    Point *pt = ft ? ft->GetPointRaw() : nullptr;
    if (!ft || !pt || pt->GetInitFeatureRaw() != ft) return false;  // a seed is the first observation of its own point
    sdvl_track_feature f;
    f.px[0] = ft->GetPosition()(0); f.px[1] = ft->GetPosition()(1);
    f.bearing[0] = ft->GetVector()(0); f.bearing[1] = ft->GetVector()(1); f.bearing[2] = ft->GetVector()(2);
    f.level = ft->GetLevel();
    const int idx = static_cast<int>(ts.points->size());
    f.point = idx;
    ts.points->push_back(ft->GetPoint());
    pt->SetTrackRow(row_base + idx);
    ts.up_points.emplace_back();
    PointRow(pt, ft, kf.get(), &ts.up_points.back());
    ts.up_feats.push_back(f);
  }
  return true;
}

// The rows the trackers `up` have ready (track_.up_points / up_feats) behind each other, as sdvl_track_upload / sdvl_track_append take
// them.  own_buf: for each tracker's current feature buffer (rows appended to a live table) instead of buffer 0 (a rebuilt table).
void SDVLBatch::GatherRows(const vector<int> &up, bool own_buf) {
  tables_.up_points.clear();
  tables_.up_feats.clear();
  for (vector<int32_t> *v : {&tables_.up_trk, &tables_.up_buf, &tables_.up_np, &tables_.up_nf}) v->clear();
  for (int i : up) {
    const SDVL::TrackState &ts = trk_[i]->track_;
    tables_.up_trk.push_back(i);
    tables_.up_buf.push_back(own_buf ? ts.feat_buf : 0);
    tables_.up_np.push_back(static_cast<int32_t>(ts.up_points.size()));
    tables_.up_nf.push_back(static_cast<int32_t>(ts.up_feats.size()));
    tables_.up_points.insert(tables_.up_points.end(), ts.up_points.begin(), ts.up_points.end());
    tables_.up_feats.insert(tables_.up_feats.end(), ts.up_feats.begin(), ts.up_feats.end());
  }
}

// Tables of the trackers `need` rebuilt from their last_frame's host objects and sent to the device in ONE submission.
// built == nullptr: all or nothing (false, nothing uploaded, if one of them cannot be expressed as a table);
// otherwise the expressible ones are uploaded and (*built)[q] says which.
bool SDVLBatch::UploadTables(const vector<int> &need, vector<char> *built) {
  vector<char> ok(need.size(), 0);
  ParallelFor(static_cast<int>(need.size()), [&](int q) { ok[q] = BuildTable(*trk_[need[q]]) ? 1 : 0; });
  if (!built)
    for (char o : ok)
      if (!o) return false;
  vector<int> up;
  vector<const sdvl_frame *> reg_frames;   // every reference frame the rebuilt tables name for the first time: ONE submission
  vector<double> reg_poses;
  for (size_t q = 0; q < need.size(); q++) {
    if (!ok[q]) continue;
    for (Frame *ref : trk_[need[q]]->track_.up_register)
      if (!ref->IsRegistered()) {
        double pose[7];
        ref->GetPose().ToArray(pose);
        reg_frames.push_back(ref->device());
        reg_poses.insert(reg_poses.end(), pose, pose + 7);
        ref->SetRegistered();
      }
    up.push_back(need[q]);
  }
  GatherRows(up, false);
  if (!reg_frames.empty())
    dev_->Check(sdvl_frames_register(dev_->ctx(), static_cast<int>(reg_frames.size()), reg_frames.data(), reg_poses.data()), "sdvl_frames_register");
  if (!up.empty())
    dev_->Check(sdvl_track_upload(dev_->ctx(), tables_.set, static_cast<int>(up.size()), tables_.up_trk.data(), tables_.up_buf.data(), tables_.up_np.data(),
                                  tables_.up_points.data(), tables_.up_nf.data(), tables_.up_feats.data()), "sdvl_track_upload");
  for (int i : up) {
    trk_[i]->track_.feat_buf = 0;
    trk_[i]->track_.valid = true;
  }
  if (built) *built = ok;
  return true;
}

// the set of tables, made at the first tracked step; false: the detection grid is one the set cannot serve
bool SDVLBatch::EnsureTrackSet() {
  const int cells = trk_[0]->feature_align_.GridCells();
  if (cells > 65535) return false;
  if (!tables_.set) {
    // a keyframe holds its matches plus what the mapper adds (one seed per free grid cell with the plane map): twice that
    // leaves room for the reference mapper's connection points; a frame that outgrows it is tracked on the host path
    int mm = 1;
    for (SDVL *t : trk_) mm = std::max(mm, t->feature_align_.MaxMatches());
    // (large grids, e.g. 8160 cells at 3840x2160 / 32: the cap stays 4096 rows; a keyframe with more goes to the host path)
    tables_.cap = std::min(4096, 2 * (mm + cells));
    tables_.cells = cells;
    dev_->Check(sdvl_track_create(dev_->ctx(), static_cast<int>(trk_.size()), tables_.cap, tables_.cap, cells, mm, Config::MaxRansacIts(), &tables_.set),
                "sdvl_track_create");
  }
  return cells == tables_.cells;
}

// With the reference's mapper the tracker follows CANDIDATES too (Map::InitCandidates links them to the keyframe at once,
// map.cc:379-390), and the depth filter rewrites their inverse depth, variance, position, failure count and finally
// `fixed` after every frame (point.cc:64-100,164-178).  With the filter on the device (depth_filter_kernel) the rows are
// patched where they lie, in the same stream, and the table stays valid; it is rebuilt from the objects when the filter ran
// on the host or on another context (threaded mode), and whenever a point with a row died behind the device's back.
void SDVLBatch::InvalidateStaleTables() {
  for (SDVL *tp : trk_) {
    SDVL &t = *tp;
    MapperMap *m = AsMapperMap(t.map_);
    if (m && (m->IsThreaded() || !MapperMap::DeviceFilter())) t.track_.valid = false;
    if (t.map_->TakeTablesDirty()) t.track_.valid = false;
    // tracking lost: last_frame stays, but the mapper has had it and trashed it — its features are gone from the host
    // (MapperMap::EmptyTrash, map.cc:207-259) and the next step must not find them in the table either
    if (t.last_frame_ && t.last_frame_->FeaturesRemoved()) t.track_.valid = false;
  }
}

}  // namespace sdvl
