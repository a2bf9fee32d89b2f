// batch_depth.cc — SDVLBatch, the second image of a frame (a registered depth image, a stereo pair's right image): the device calls of a
// step that read it, each ONE call for all trackers — the keyframes the driver seeds (SeedKeyframesFromDepth: sdvl_depth_seed or
// sdvl_stereo_depth), and for the sequential mappers (batch_mapper.cc) the corners of their new keyframes (MeasureKeyframeCorners), the
// features bundle adjustment's depth edges carry (LookupKeyframeFeatures) and the jobs of a measured filter pass (MeasuredFilterJobs).
// Every job list is made by DepthJobs (depth_jobs.h).
#include "batch_internal.h"
#include "depth_jobs.h"

#include <algorithm>
#include <cstring>

namespace sdvl {

using std::shared_ptr;
using std::vector;

namespace {

// the filtered corners of a keyframe behind those in xyl (x, y, level each); -> their number
int AppendFilteredCorners(const Frame &kf, vector<int32_t> *xyl) {
  const int n = kf.NumFiltered();
  for (int c = 0; c < n; c++) {
    const Vector3i corner = kf.FilteredCorner(c);
    xyl->insert(xyl->end(), {corner(0), corner(1), corner(2)});
  }
  return n;
}

}  // namespace

SDVLBatch::CameraAndLens SDVLBatch::BatchCamera() const {
  const Camera &camera = *trk_[0]->camera_;
  return CameraAndLens{camera.abi(), camera.distortion(), camera.HasDistortion()};
}

const DepthImage *SDVLBatch::DepthOf(int i) {
  if (!step_depths_ || step_depths_->empty() || (*step_depths_)[i].empty()) return nullptr;
  if (!trk_[i]->StereoRectification()) return &(*step_depths_)[i];
  if (!rights_rectified_) RectifyRights();
  return &rectified_rights_[i];
}

// Stereo rigs as calibrated (SDVL::SetStereoRectification): the step's right images are RAW images of the right camera.  They are
// rectified into HBM here, all trackers' in ONE sdvl_rectify call, when the step's first consumer asks for one (DepthOf), and every
// consumer of the step — sdvl_stereo_depth, sdvl_search_run_filter_stereo — is handed the rectified image on the device.
void SDVLBatch::RectifyRights() {
  const int B = static_cast<int>(trk_.size());
  rectified_rights_.assign(B, DepthImage());
  vector<int> who;
  vector<const void *> src;
  for (int i = 0; i < B; i++) {
    const DepthImage &d = (*step_depths_)[i];
    if (d.empty() || !trk_[i]->StereoRectification()) continue;
    if (d.format != DEPTH_RIGHT8)
      throw std::runtime_error("SDVLBatch: a tracker that seeds from a stereo pair takes a right image (DEPTH_RIGHT8), not a depth image");
    if (!who.empty()) {
      const DepthImage &first = (*step_depths_)[who[0]];
      if (d.cols != first.cols || d.rows != first.rows || d.step != first.step || d.on_device != first.on_device)
        throw std::runtime_error("SDVLBatch: the raw right images of a step share size, row pitch and memory kind");
      if (std::memcmp(&trk_[i]->camera_->rectified_pair()->right, &trk_[who[0]]->camera_->rectified_pair()->right, sizeof(sdvl_rectification)) != 0)
        throw std::runtime_error("SDVLBatch: the trackers of a batch share the rectified pair");
    }
    who.push_back(i);
    src.push_back(d.data);
  }
  rights_rectified_ = true;
  if (who.empty()) return;
  const DepthImage &first = (*step_depths_)[who[0]];
  const size_t image_bytes = static_cast<size_t>(first.cols) * first.rows, need = image_bytes * B;
  if (d_rights_bytes_ < need) {
    if (d_rights_) dev_->Check(sdvl_device_free(dev_->ctx(), d_rights_), "sdvl_device_free");
    d_rights_ = nullptr;
    d_rights_bytes_ = 0;
    dev_->Check(sdvl_device_malloc(dev_->ctx(), static_cast<int64_t>(need), &d_rights_), "sdvl_device_malloc");
    d_rights_bytes_ = need;
  }
  vector<void *> dst;
  for (int i : who) dst.push_back(static_cast<uint8_t *>(d_rights_) + image_bytes * i);
  dev_->Check(sdvl_rectify(dev_->ctx(), static_cast<int>(who.size()), src.data(), first.step, first.on_device ? 1 : 0, first.cols, first.rows,
                           &trk_[who[0]]->camera_->rectified_pair()->right, dst.data(), first.cols),
              "sdvl_rectify");
  for (size_t k = 0; k < who.size(); k++)
    rectified_rights_[who[k]] = DepthImage::Wrap(dst[k], first.cols, first.rows, first.cols, DEPTH_RIGHT8, 1.0, true);
}

void SDVLBatch::SizeDepthResults(int n) {
  depth_z_.assign(std::max(n, 1), 0.0);
  depth_status_.assign(std::max(n, 1), 0);
}

// The corners xyl (x, y, level each) that `jobs` lists, through the jobs' producer — sdvl_stereo_depth for pairs, sdvl_depth_seed for depth
// images, ONE call — into depth_z_ / depth_status_; -> the corners with a depth per job.  No job: no call
vector<int32_t> SDVLBatch::MeasureCorners(const DepthJobs &jobs, const vector<int32_t> &xyl) {
  const int n_corners = jobs.items();
  SizeDepthResults(n_corners);
  vector<int32_t> ok(std::max(jobs.size(), 1), 0);
  if (jobs.empty()) return ok;
  const CameraAndLens c = BatchCamera();
  if (jobs.stereo()) {
    sdvl_stereo_params sp = *jobs.stereo_rule();
    sp.dist = c.lens();  // (refused: rectified pairs only)
    vector<double> disparity(n_corners, 0.0);
    dev_->Check(sdvl_stereo_depth(dev_->ctx(), jobs.size(), jobs.stereo_jobs(), n_corners, xyl.data(), &c.cam, &sp, depth_z_.data(), disparity.data(),
                                  depth_status_.data(), ok.data()),
                "sdvl_stereo_depth");
  } else {
    dev_->Check(sdvl_depth_seed(dev_->ctx(), jobs.size(), jobs.depth_jobs(), jobs.width(), jobs.height(), n_corners, xyl.data(), &c.cam, c.lens(),
                                jobs.rule(), depth_z_.data(), depth_status_.data(), ok.data()),
                "sdvl_depth_seed");
  }
  return ok;
}

// Depth cameras: the filtered corners of the step's keyframes whose tracker seeds from depth (SDVL::SetDepthSeeding) are looked up in
// their frames' depth images by ONE sdvl_depth_seed call.  (*z)[k] / (*status)[k]: keyframe k's results, null for a keyframe that is not
// seeded from depth.  A keyframe that came without a depth image seeds nothing and is counted.  A first frame becomes the first keyframe
// here if at least SDVL.min_init_corners of its corners have a depth; otherwise it is not kept (its entry of s.kfs becomes null).
// (a stereo tracker's second image is the pair's right image, SDVL::SetStereoSeeding: the same jobs with sdvl_stereo_depth as the producer)
void SDVLBatch::SeedKeyframesFromDepth(Step &s, vector<const double *> *z, vector<const uint8_t *> *status) {
  const size_t K = s.kfs.size();
  z->assign(K, nullptr);
  status->assign(K, nullptr);
  bool any = false;
  for (size_t k = 0; k < K; k++) any = any || trk_[s.kf_owner[k]]->depth_seeding_;
  if (!any) return;
  DepthJobs jobs;
  vector<int32_t> xyl;
  for (size_t k = 0; k < K; k++) {
    SDVL &t = *trk_[s.kf_owner[k]];
    if (!t.depth_seeding_) continue;
    const DepthImage *d = DepthOf(s.kf_owner[k]);  // (none: counted below)
    const Frame &kf = *s.kfs[k];
    const int owner = static_cast<int>(k), n = kf.NumFiltered();
    if (t.stereo_seeding_ ? jobs.AddStereo(owner, kf.device(), d, t.stereo_rule_, n, kf.GetWidth(), kf.GetHeight())
                          : jobs.AddDepth(owner, d, t.depth_rule_, n, kf.GetWidth(), kf.GetHeight()))
      AppendFilteredCorners(kf, &xyl);
  }
  const vector<int32_t> ok = MeasureCorners(jobs, xyl);
  for (const DepthJobs::Range &r : jobs.ranges()) {
    (*z)[r.owner] = depth_z_.data() + r.begin;
    (*status)[r.owner] = depth_status_.data() + r.begin;
  }
  for (size_t k = 0; k < K; k++) {
    SDVL &t = *trk_[s.kf_owner[k]];
    if (!t.depth_seeding_) continue;
    const int j = jobs.JobOf(static_cast<int>(k));
    if (j < 0)
      if (PlaneMap *pm = dynamic_cast<PlaneMap *>(t.map_)) pm->CountNoDepth();
    if (!t.first_frame_waiting_) continue;
    if (j >= 0 && ok[j] >= Config::MinInitCorners()) {
      t.CommitFirstFrame(s.stats[s.kf_owner[k]]);
    } else {  // too few corners with a depth: the frame is not kept, the next one starts over
      t.first_frame_waiting_ = false;
      t.init_failed_ = true;
      t.pending_kf_ = nullptr;
      s.kfs[k] = nullptr;
    }
  }
}

// Depth cameras inside the mapper: the filtered corners of all the step's new keyframes whose mapper measures, looked up in their frames'
// depth images by ONE sdvl_depth_seed call (as SeedKeyframesFromDepth does for the keyframes the driver seeds) and handed to the mappers.
// Stereo mapping: matched in their frames' right images by ONE sdvl_stereo_depth call, z / status handed over unchanged
void SDVLBatch::MeasureKeyframeCorners(MapStep &m, const vector<char> &need) {
  DepthJobs jobs;
  vector<int32_t> xyl;
  for (size_t q = 0; q < m.kf_idx.size(); q++) {
    const int k = m.kf_idx[q];
    if (!need[q] || !m.mm[k]->Measuring()) continue;
    const Frame &kf = *m.mm[k]->CurrentFrame();
    if (m.mm[k]->StereoMapping() ? jobs.AddStereo(k, kf.device(), m.depth_of[k], trk_[m.trk[k]]->stereo_rule_, kf.NumFiltered(), kf.GetWidth(), kf.GetHeight())
                                 : jobs.AddDepth(k, m.depth_of[k], trk_[m.trk[k]]->depth_rule_, kf.NumFiltered(), kf.GetWidth(), kf.GetHeight()))
      AppendFilteredCorners(kf, &xyl);
    else
      m.mm[k]->SetCornerDepths(nullptr, nullptr);
  }
  if (jobs.empty()) return;
  MeasureCorners(jobs, xyl);
  for (const DepthJobs::Range &r : jobs.ranges()) m.mm[r.owner]->SetCornerDepths(depth_z_.data() + r.begin, depth_status_.data() + r.begin);
}

// Depth edges in bundle adjustment (SDVL::SetDepthBundle): the features the step's new keyframes hold when their mapper takes them up —
// the tracked matches, at their found pixel and level — are looked up in their frames' depth images by ONE sdvl_depth_lookup call, inside
// the step's sdvl_depth_stage_begin / _end bracket like the sdvl_depth_seed calls beside it.  A keyframe that is not the step's own frame
// (or came without an image) is not looked up: its image is gone.
void SDVLBatch::LookupKeyframeFeatures(MapStep &m) {
  DepthJobs jobs;
  vector<double> px2;
  vector<int32_t> level;
  for (int k : m.kf_idx) {
    if (!m.mm[k]->DepthBundleOn() || m.mm[k]->CurrentFrame().get() != trk_[m.trk[k]]->step_frame_) continue;
    const DepthImage *d = DepthOf(m.trk[k]);
    if (!d) continue;
    const sdvl_depth_seed_params &rule = trk_[m.trk[k]]->depth_rule_;
    jobs.ShareDepthRule(rule);  // (of a keyframe without such features too)
    const int n = m.mm[k]->EmitDepthLookups(&px2, &level);
    if (n > 0) jobs.AddDepth(k, d, rule, n, m.mm[k]->CurrentFrame()->GetWidth(), m.mm[k]->CurrentFrame()->GetHeight());
  }
  if (jobs.empty()) return;
  SizeDepthResults(jobs.items());
  vector<int32_t> ok(jobs.size(), 0);
  const CameraAndLens c = BatchCamera();
  dev_->Check(sdvl_depth_lookup(dev_->ctx(), jobs.size(), jobs.depth_jobs(), jobs.width(), jobs.height(), jobs.items(), px2.data(), level.data(), &c.cam,
                                c.lens(), jobs.rule(), depth_z_.data(), depth_status_.data(), ok.data()),
              "sdvl_depth_lookup");
  for (const DepthJobs::Range &r : jobs.ranges()) m.mm[r.owner]->ApplyDepthLookups(depth_z_.data() + r.begin, depth_status_.data() + r.begin);
}

// The measured form of PackAndSearch (batch_mapper.cc): the requests m.begin[k] .. m.begin[k + 1] of every mapper whose update works on
// the step's frame are looked up in that frame's depth image; the requests of every other mapper are in no job.  Stereo mapping: matched
// against that frame's right image (sdvl_search_run_filter_stereo), the frame being the jobs' left one
void SDVLBatch::SearchFilterMeasured(MapStep &m, int total, const sdvl_camera &cam, const sdvl_search_params &sp) {
  DepthJobs jobs;
  const bool stereo = m.measuring->StereoMapping();
  for (int k = 0; k < m.M(); k++) {
    const int n = static_cast<int>(m.begin[k + 1] - m.begin[k]);
    if (!m.depth_of[k] || n == 0) {
      jobs.Skip(n);
      continue;
    }
    if (stereo)
      jobs.AddStereo(k, m.mm[k]->CurrentFrame()->device(), m.depth_of[k], trk_[m.trk[k]]->stereo_rule_, n, m.mm[k]->CurrentFrame()->GetWidth(),
                     m.mm[k]->CurrentFrame()->GetHeight());
    else
      jobs.AddDepth(k, m.depth_of[k], trk_[m.trk[k]]->depth_rule_, n, m.mm[k]->CurrentFrame()->GetWidth(), m.mm[k]->CurrentFrame()->GetHeight());
  }
  m.depth_status.resize(total);
  if (stereo) {  // (no request has a pair: nothing is matched; the rule is still checked, so it is the measuring tracker's)
    sdvl_stereo_measure_params mp = {jobs.stereo_rule() ? *jobs.stereo_rule() : trk_[m.measuring_trk]->stereo_rule_, m.measuring->DisparitySigma()};
    const CameraAndLens c = BatchCamera();
    mp.rule.dist = c.lens();  // (refused: rectified pairs only)
    dev_->Check(sdvl_search_run_filter_stereo(dev_->ctx(), total, &cam, &sp, m.states.data(), &m.fparams, tables_.set, jobs.size(), jobs.stereo_jobs(), &mp,
                                              m.res.data(), m.fout.data(), m.depth_status.data()),
                "sdvl_search_run_filter_stereo");
    return;
  }
  // (no request has an image: nothing is looked up, and the call names an image of one pixel)
  const int width = jobs.empty() ? 1 : jobs.width(), height = jobs.empty() ? 1 : jobs.height();
  const sdvl_depth_measure_params mp = m.measuring->DepthMeasureParams(jobs.rule() ? *jobs.rule() : sdvl_depth_seed_params{0.0, 0.0, 0.0, 0, 0});
  const CameraAndLens c = BatchCamera();
  dev_->Check(sdvl_search_run_filter_measured(dev_->ctx(), total, &cam, &sp, m.states.data(), &m.fparams, tables_.set, jobs.size(), jobs.depth_jobs(), width,
                                              height, c.lens(), &mp, m.res.data(), m.fout.data(), m.depth_status.data()),
              "sdvl_search_run_filter_measured");
}

}  // namespace sdvl
