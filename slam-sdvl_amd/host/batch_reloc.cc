// batch_reloc.cc — SDVLBatch: relocalisation inside the tabled step, and the HBM store of keyframe feature records it keeps
// (SDVLBatch::RelocStore; no other file names the store's members).
#include "batch_internal.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <iostream>
#include <stdexcept>

namespace sdvl {

using std::shared_ptr;
using std::vector;

// -------------------------------------------------------------------------------- SDVLBatch: relocalisation inside the tabled step
static std::atomic<unsigned long long> g_reloc_epoch{1};  // process-wide: a cache never mistakes another batch's store for its own

SDVLBatch::RelocStore::~RelocStore() {
  if (store) {
    Device::SetCurrent(dev);
    (void)sdvl_align_store_destroy(dev->ctx(), store);
  }
}

// The alignments of RelocalizeLost: jobs whose feature ranges name records of the batch's store, in launches of bounded size
// (a farm whose trackers are all lost asks for B x |keyframes| alignments per step).
void SDVLBatch::RelocAlign(const vector<sdvl_align_job> &jobs, const sdvl_align_params &ap, vector<sdvl_align_result> *res) {
  res->resize(jobs.size());
  const sdvl_camera cam = trk_[0]->camera_->abi();
  const size_t kChunk = 4096;
  for (size_t b = 0; b < jobs.size(); b += kChunk) {
    const int n = static_cast<int>(std::min(jobs.size(), b + kChunk) - b);
    dev_->Check(sdvl_image_align_begin_stored(dev_->ctx(), n, jobs.data() + b, reloc_store_.store, &cam, &ap), "sdvl_image_align_begin_stored");
    dev_->Check(sdvl_image_align_end(dev_->ctx(), n, res->data() + b), "sdvl_image_align_end");
  }
}

// t.reloc_ of the keyframes of t's map, newest first (the order Relocalize visits them in); their feature records go behind *packed
void SDVLBatch::PackRelocCache(SDVL &t, vector<sdvl_align_feature> *packed) {
  SDVL::RelocCache &rc = t.reloc_;
  rc.kfs.clear();
  rc.begin.assign(1, 0);
  rc.T.clear();
  vector<shared_ptr<Frame>> &kfs = t.map_->GetKeyframes();
  for (auto it = kfs.rbegin(); it != kfs.rend(); it++) {
    rc.kfs.push_back(*it);
    // (a keyframe holds its matches plus at most one seed per free grid cell, and the seeds are filtered corners: <= max_matches +
    // num_features whatever the grid, 1200 with the TUM settings even on 8160 cells; a keyframe beyond SDVL_MAX_ALIGN_FEATURES (2048)
    // makes the stored alignment report SDVL_ERR_CAPACITY, at any frame size)
    ImageAlign::PackFeatures(**it, packed);
    rc.begin.push_back(static_cast<int32_t>(packed->size()));
    double T7[7];
    ((*it)->GetPose() * (*it)->GetPose().Inverse()).ToArray(T7);  // current_frame_->SetPose(cframe->GetPose()), then image_align.cc:66
    rc.T.insert(rc.T.end(), T7, T7 + 7);
  }
}

// The keyframes' feature records of the trackers `lost`: they do not change while a tracker is lost (no tracked step, the mapper stands
// still), so they are packed once and stay in HBM (sdvl_align_store; SDVL::RelocCache remembers where) — packed again only for the
// trackers whose map changed since, or that were not lost before.  Per frame only the job records cross the link.
void SDVLBatch::RefreshRelocStore(const vector<int> &lost) {
  RelocStore &rs = reloc_store_;
  const int L = static_cast<int>(lost.size());
  vector<vector<sdvl_align_feature>> fresh(L);
  vector<char> stale(L, 0);
  for (int q = 0; q < L; q++) {
    SDVL &t = *trk_[lost[q]];
    SyncStats(t);  // the Point objects Reproject reads catch up with the device's counters
    t.StartRelocalizing();
    const SDVL::RelocCache &rc = t.reloc_;
    stale[q] = (!rs.store || rc.owner != this || rc.epoch != rs.epoch || rc.version != t.map_->Version()) ? 1 : 0;
  }
  ParallelFor(L, [&](int q) {
    if (stale[q]) PackRelocCache(*trk_[lost[q]], &fresh[q]);
  });
  size_t need = 0;
  for (int q = 0; q < L; q++)
    if (stale[q]) need += fresh[q].size();
  if (need == 0) return;  // also when every keyframe is empty — with no store yet none is made, and RelocAlign meets a null one
  if (!rs.store || rs.used + need > static_cast<size_t>(rs.cap)) {
    // no room behind the records in use: a new store for what is live now (the other trackers' caches are void: epoch)
    size_t live = need;
    for (int q = 0; q < L; q++)
      if (!stale[q]) {
        stale[q] = 1;  // repack: its records die with the old store
        PackRelocCache(*trk_[lost[q]], &fresh[q]);
        live += fresh[q].size();
      }
    if (rs.store) dev_->Check(sdvl_align_store_destroy(dev_->ctx(), rs.store), "sdvl_align_store_destroy");
    rs.store = nullptr;
    rs.epoch = g_reloc_epoch++;
    rs.used = 0;
    const size_t cap = std::max<size_t>(2 * live, 65536);
    if (cap > 0x7fffffffu) throw std::runtime_error("SDVLBatch: relocalisation store too large");
    dev_->Check(sdvl_align_store_create(dev_->ctx(), static_cast<int>(cap), &rs.store), "sdvl_align_store_create");
    rs.cap = static_cast<int>(cap);
  }
  vector<sdvl_align_feature> all;
  const int base = rs.used;
  for (int q = 0; q < L; q++) {
    if (!stale[q]) continue;
    SDVL &t = *trk_[lost[q]];
    SDVL::RelocCache &rc = t.reloc_;
    const int32_t off = base + static_cast<int32_t>(all.size());
    for (int32_t &b : rc.begin) b += off;
    all.insert(all.end(), fresh[q].begin(), fresh[q].end());
    rc.owner = this;
    rc.epoch = rs.epoch;
    rc.version = t.map_->Version();
  }
  dev_->Check(sdvl_align_store_write(dev_->ctx(), rs.store, base, static_cast<int>(all.size()), all.data()), "sdvl_align_store_write");
  rs.used = base + static_cast<int>(all.size());
}

// The alignment of every lost tracker's current frame against EVERY keyframe of its map (each started from that keyframe's pose, fast
// mode): independent of each other, one launch for all (tracker, keyframe) pairs.  (*first)[q] = the first job of tracker lost[q].
// Fast mode gives up behind the coarsest level when the update there is still > 0.01 (image_align.cc:73-76), and on a frame that shows
// something else nearly every keyframe does: the launch runs that level ONLY (a third of PrecomputePatches); the few jobs that pass it
// are run again in full — same start, same arithmetic, so both passes leave what one full pass would.
void SDVLBatch::RelocAlignKeyframes(const vector<int> &lost, vector<int> *first, vector<sdvl_align_result> *res) {
  const int L = static_cast<int>(lost.size());
  vector<sdvl_align_job> jobs;
  first->assign(L + 1, 0);
  for (int q = 0; q < L; q++) {
    SDVL &t = *trk_[lost[q]];
    const SDVL::RelocCache &rc = t.reloc_;
    (*first)[q] = static_cast<int>(jobs.size());
    for (size_t j = 0; j < rc.kfs.size(); j++) {
      if (rc.begin[j + 1] == rc.begin[j]) std::cerr << "[ERROR] No points to track!" << std::endl;  // image_align.cc:55-58
      sdvl_align_job jb;
      jb.ref = rc.kfs[j]->device();
      jb.cur = t.current_frame_->device();
      jb.feat_begin = rc.begin[j];
      jb.feat_end = rc.begin[j + 1];
      std::memcpy(jb.T, rc.T.data() + 7 * j, sizeof(jb.T));
      jobs.push_back(jb);
    }
  }
  (*first)[L] = static_cast<int>(jobs.size());
  if (jobs.empty()) return;
  sdvl_align_params ap = AlignParams(true);
  const int min_level = ap.min_level;
  ap.min_level = ap.max_level;  // the coarsest level alone
  RelocAlign(jobs, ap, res);
  if (min_level >= ap.max_level) return;
  vector<int> pass;
  for (size_t j = 0; j < jobs.size(); j++)
    if ((*res)[j].error <= 0.01) pass.push_back(static_cast<int>(j));  // image_align.cc:73-76 did not give up: the finer levels follow
  if (pass.empty()) return;
  vector<sdvl_align_job> again;
  for (int j : pass) again.push_back(jobs[j]);
  vector<sdvl_align_result> full;
  ap.min_level = min_level;
  RelocAlign(again, ap, &full);
  for (size_t k = 0; k < pass.size(); k++) (*res)[pass[k]] = full[k];
}

// SDVL::Relocalize (sdvl.cc:73-89,205-238) for the trackers `lost` of a batch, inside the tabled step: the other trackers of the batch
// are not touched.  (*found)[q]: tracker lost[q] has relocalised — last_frame_ = last_kf_ = the keyframe it landed on (sdvl.cc:84-86).
// The keyframe loop, sdvl.cc:209-235, runs over the alignments' results in the reference's order (newest first).  Reproject(reloc = true)
// draws from rand() and stops at the first keyframe that gathers MinMatches, so it stays sequential per tracker — but the trackers
// advance together: one search launch per ROUND (a round = every unresolved tracker's next keyframe with error < 0.001; almost always
// there is one round).
void SDVLBatch::RelocalizeLost(const vector<int> &lost, FrameStats *stats, vector<char> *found) {
  found->assign(lost.size(), 0);
  RefreshRelocStore(lost);
  vector<int> first;
  vector<sdvl_align_result> res;
  RelocAlignKeyframes(lost, &first, &res);
  const int L = static_cast<int>(lost.size());
  vector<int> cursor(first.begin(), first.end() - 1);
  vector<char> open_(L, 1);
  vector<vector<sdvl_search_req>> per(L);
  vector<sdvl_search_req> reqs;
  vector<sdvl_search_res> sres;
  vector<size_t> begin(L + 1, 0);
  for (;;) {
    bool any = false;
    reqs.clear();
    for (int q = 0; q < L; q++) {
      per[q].clear();
      if (!open_[q]) continue;
      SDVL &t = *trk_[lost[q]];
      const SDVL::RelocCache &rc = t.reloc_;
      // every keyframe visited leaves its aligned pose on the frame (image_align.cc:79); those with error >= 0.001 are passed over
      while (cursor[q] < first[q + 1]) {
        const int j = cursor[q] - first[q];
        if (rc.begin[j + 1] > rc.begin[j])  // (ComputePose returns before touching the pose when frame1 has no features)
          t.current_frame_->SetPose(SE3::FromArray(res[cursor[q]].T) * rc.kfs[j]->GetPose());
        else
          t.current_frame_->SetPose(rc.kfs[j]->GetPose());
        const double err = rc.begin[j + 1] > rc.begin[j] ? res[cursor[q]].error : 1e10;
        if (err < 0.001) break;
        cursor[q]++;
      }
      if (cursor[q] >= first[q + 1]) {
        open_[q] = 0;
        continue;
      }
      const shared_ptr<Frame> &cframe = rc.kfs[cursor[q] - first[q]];
      t.feature_align_.PrepareReproject(t.current_frame_, cframe, true, &per[q]);
      any = true;
    }
    if (!any) break;
    Concatenate(per, &reqs, &begin);
    Matcher::SearchPoints(dev_, reqs, *trk_[lost[0]]->camera_, &sres);
    for (int q = 0; q < L; q++) {
      if (!open_[q] || cursor[q] >= first[q + 1]) continue;
      SDVL &t = *trk_[lost[q]];
      t.feature_align_.FinishReproject(t.current_frame_, sres.data() + begin[q]);
      t.matches_ = t.feature_align_.GetMatches();
      t.attempts_ = t.feature_align_.GetAttempts();
      if (t.matches_ >= Config::MinMatches()) {
        t.Relocalized(t.reloc_.kfs[cursor[q] - first[q]], stats[lost[q]]);
        (*found)[q] = 1;
        open_[q] = 0;
      } else {
        cursor[q]++;
      }
    }
  }
}

}  // namespace sdvl
