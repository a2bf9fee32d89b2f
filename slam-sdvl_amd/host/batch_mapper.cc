// batch_mapper.cc — SDVLBatch, stage 5 of a step: SDVL::Mapping() of sequential mode (main.cc:148-149) for the trackers that own a real
// mapper.  The phases of Map::UpdateMap run in lock step over a MapStep (batch_internal.h), every phase's SearchPoint requests of ALL
// trackers in one K7 launch: the candidate passes, the new keyframes' connections and candidates, the finish, and the bundle windows of
// all mappers in one sdvl_bundle_adjust call.  What reads a frame's depth image on the way is in batch_depth.cc.
#include "batch_internal.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace sdvl {

using std::shared_ptr;
using std::vector;

void SDVLBatch::RunMappers() {
  MapStep m;
  if (!CollectMappers(m)) return;
  SetUpMeasuring(m);
  CandidatePasses(m);
  KeyframePasses(m);
  m.sub.reset(new StageClock(ST_MAP_FINISH));
  ParallelFor(m.M(), [&](int k) { m.mm[k]->FinishUpdate(); });
  BundleWindows(m);
}

// the mappers that begin an update this step, and the lists of a MapStep sized for them; false: none
bool SDVLBatch::CollectMappers(MapStep &m) {
  {
    StageClock begin_clk(ST_MAP_BEGIN);
    for (size_t i = 0; i < trk_.size(); i++) {
      MapperMap *mp = AsMapperMap(trk_[i]->map_);
      if (mp && !mp->IsThreaded() && mp->BeginUpdate()) {  // a started mapper thread does its own UpdateMap
        m.mm.push_back(mp);
        m.trk.push_back(static_cast<int>(i));
      }
    }
  }
  const int M = m.M();
  if (M == 0) return false;
  m.per.resize(M);
  m.begin.assign(M + 1, 0);
  // UpdateCandidates with the depth filter on the device: one filter state per request, outcomes beside the search results;
  // the rows of the points the trackers follow are patched in the same submission (same context, same stream)
  m.dev_filter = MapperMap::DeviceFilter();
  m.per_st.resize(M);
  m.fparams = m.mm[0]->FilterParams();
  m.depth_of.assign(M, nullptr);
  return true;
}

// Depth cameras (SDVL::SetDepthMapping): when a mapper of the step has the switch on, the candidate passes go through the measured
// filter — still one launch for all trackers.  depth_of[k]: the depth image of the step's frame, for a mapper with the switch on whose
// update works on that very frame; the requests of every other mapper are in no job and take the triangulated rule.
// Stereo cameras (SDVL::SetStereoMapping): the same with the step frame's right image in depth_of[k] and the matcher as the producer.
void SDVLBatch::SetUpMeasuring(MapStep &m) {
  for (int k = 0; k < m.M(); k++) {
    if (!m.mm[k]->Measuring()) continue;
    if (!m.dev_filter) throw std::runtime_error("mapper: depth mapping (SDVL::SetDepthMapping, SetStereoMapping) needs the depth filter on the device");
    if (m.measuring && m.measuring->StereoMapping() != m.mm[k]->StereoMapping())
      throw std::runtime_error("SDVLBatch: a batch does not mix depth mapping and stereo mapping");
    if (m.mm[k]->StereoMapping()) {
      if (m.measuring && m.measuring->DisparitySigma() != m.mm[k]->DisparitySigma())
        throw std::runtime_error("SDVLBatch: the trackers of a batch share the disparity noise");
    } else if (m.measuring) {
      const sdvl_depth_measure_params a = m.mm[k]->DepthMeasureParams(trk_[m.trk[k]]->depth_rule_);
      const sdvl_depth_measure_params b = m.measuring->DepthMeasureParams(trk_[m.trk[k]]->depth_rule_);
      if (a.noise_abs != b.noise_abs || a.noise_quad != b.noise_quad) throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth noise parameters");
    }
    m.measuring = m.mm[k];
    m.measuring_trk = m.trk[k];
    if (m.mm[k]->CurrentFrame().get() == trk_[m.trk[k]]->step_frame_) m.depth_of[k] = DepthOf(m.trk[k]);
  }
}

// search everything the maps emitted, leave the offsets in m.begin; filter: with the depth filter behind the search (measured, when a
// mapper of the step measures)
void SDVLBatch::PackAndSearch(MapStep &m, bool filter) {
  // the requests go from the maps' lists straight into the context's pinned batch (device layout, frames by slot)
  const int M = m.M();
  Concatenate(m.per, nullptr, &m.begin);
  const size_t total = m.begin[M];
  m.states.clear();
  m.res.resize(std::max<size_t>(total, 1));   // every record is written by the call below (no clearing pass over MBs)
  m.fout.resize(std::max<size_t>(filter ? total : 0, 1));
  if (total == 0) return;
  sdvl_ctx *ctx = dev_->ctx();
  sdvl_search_req_packed *packed = nullptr;
  dev_->Check(sdvl_search_begin(ctx, static_cast<int>(total), &packed), "sdvl_search_begin");
  size_t o = 0;
  for (int k = 0; k < M; k++) {
    for (const sdvl_search_req &r : m.per[k]) {
      sdvl_search_req_packed &d = packed[o++];
      d.cur = sdvl_search_slot(ctx, r.cur, r.cur_pose);
      d.ref = sdvl_search_slot(ctx, r.ref, r.ref_pose);
      if (d.cur < 0 || d.ref < 0) dev_->Check(d.cur < 0 ? d.cur : d.ref, "sdvl_search_slot");
      d.level = r.level; d.fixed = r.fixed;
      d.px[0] = r.px[0]; d.px[1] = r.px[1];
      d.bearing[0] = r.bearing[0]; d.bearing[1] = r.bearing[1]; d.bearing[2] = r.bearing[2];
      d.idepth = r.idepth; d.idepth_std = r.idepth_std;
      d.px0[0] = r.px0[0]; d.px0[1] = r.px0[1];
      std::memcpy(d.desc, r.desc, 32);
    }
    m.per[k].clear();
    if (filter) {
      m.states.insert(m.states.end(), m.per_st[k].begin(), m.per_st[k].end());
      m.per_st[k].clear();
    }
  }
  const sdvl_camera c = trk_[0]->camera_->abi();
  const sdvl_search_params sp = SearchParams();
  if (filter && m.states.size() != total) throw std::runtime_error("mapper: one filter state per candidate request");
  if (filter && m.measuring)
    SearchFilterMeasured(m, static_cast<int>(total), c, sp);
  else if (filter)
    dev_->Check(sdvl_search_run_filter(ctx, static_cast<int>(total), &c, &sp, m.states.data(), &m.fparams, tables_.set, m.res.data(), m.fout.data()),
                "sdvl_search_run_filter");
  else
    dev_->Check(sdvl_search_run(ctx, static_cast<int>(total), &c, &sp, m.res.data()), "sdvl_search_run");
}

// UpdateCandidates, one occurrence pass at a time
void SDVLBatch::CandidatePasses(MapStep &m) {
  const int M = m.M();
  m.sub.reset(new StageClock(ST_MAP_CANDIDATES));
  for (;;) {
    vector<char> more(M, 0);
    {
      StageClock c(ST_MAP_EMIT);
      ParallelFor(M, [&](int k) { more[k] = m.mm[k]->EmitCandidates(&m.per[k], m.dev_filter ? &m.per_st[k] : nullptr) ? 1 : 0; });
    }
    if (std::find(more.begin(), more.end(), 1) == more.end()) break;
    {
      StageClock c(ST_MAP_SEARCH);
      PackAndSearch(m, m.dev_filter);
    }
    StageClock c(ST_MAP_APPLY);
    ParallelFor(M, [&](int k) {
      if (more[k]) m.mm[k]->ApplyCandidates(m.res.data() + m.begin[k], m.dev_filter ? m.fout.data() + m.begin[k] : nullptr,
                                            m.measuring && !m.depth_status.empty() ? m.depth_status.data() + m.begin[k] : nullptr);
    });
  }
}

// the mappers whose update takes a new keyframe: its connections (Map::CheckConnections) and its candidates (Map::InitCandidates)
void SDVLBatch::KeyframePasses(MapStep &m) {
  for (int k = 0; k < m.M(); k++)
    if (m.mm[k]->IsKeyframeUpdate()) m.kf_idx.push_back(k);
  const vector<int> &kf_idx = m.kf_idx;
  const int K = static_cast<int>(kf_idx.size());
  m.sub.reset(new StageClock(ST_MAP_CONNECTIONS));
  if (K == 0) return;
  LookupKeyframeFeatures(m);  // (returns at once unless a mapper has depth edges on)
  ParallelFor(K, [&](int q) {
    MapperMap *mp = m.mm[kf_idx[q]];
    mp->CheckConnections();
    mp->EmitConnectionsPoints(&m.per[kf_idx[q]]);
  });
  PackAndSearch(m, false);
  vector<char> need(K, 0);
  ParallelFor(K, [&](int q) {
    MapperMap *mp = m.mm[kf_idx[q]];
    mp->ApplyConnectionsPoints(m.res.data() + m.begin[kf_idx[q]]);
    need[q] = mp->PrepareInitCandidates() ? 1 : 0;
  });
  m.sub.reset(new StageClock(ST_MAP_INIT));
  vector<shared_ptr<Frame>> to_filter;
  for (int q = 0; q < K; q++)
    if (need[q]) to_filter.push_back(m.mm[kf_idx[q]]->CurrentFrame());
  if (to_filter.empty()) return;
  Frame::FilterCornersBatch(to_filter);
  if (m.measuring) MeasureKeyframeCorners(m, need);
  ParallelFor(K, [&](int q) { if (need[q]) m.mm[kf_idx[q]]->EmitInitCandidates(&m.per[kf_idx[q]]); });
  PackAndSearch(m, false);
  ParallelFor(K, [&](int q) { if (need[q]) m.mm[kf_idx[q]]->ApplyInitCandidates(m.res.data() + m.begin[kf_idx[q]]); });
}

// local bundle adjustment (map.cc:130-137): the windows of all the step's mappers in ONE sdvl_bundle_adjust call
void SDVLBatch::BundleWindows(MapStep &m) {
  const int M = m.M();
  bool any_bundle = false;
  for (int k = 0; k < M; k++) any_bundle = any_bundle || m.mm[k]->BundleAdjustmentOn();
  if (!any_bundle) return;
  m.sub.reset(new StageClock(ST_MAP_BUNDLE));
  vector<BundleProblem> windows(M);
  vector<char> has(M, 0);
  ParallelFor(M, [&](int k) { has[k] = m.mm[k]->PrepareBundle(&windows[k]) ? 1 : 0; });
  vector<BundleProblem *> problems;
  vector<int> whose;
  for (int k = 0; k < M; k++)
    if (has[k]) {
      problems.push_back(&windows[k]);
      whose.push_back(k);
    }
  if (problems.empty()) return;
  vector<sdvl_bundle_result> results;
  vector<vector<Frame *>> moved;
  double bf = 0.0;  // depth edges: the windows of the mappers that have them on carry depths; the trackers of a batch share bf
  for (int k : whose) {
    if (!m.mm[k]->DepthBundleOn()) continue;
    if (bf > 0.0 && bf != m.mm[k]->DepthBundleBf()) throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth edges' bf");
    bf = m.mm[k]->DepthBundleBf();
  }
  Bundle::Solve(dev_, *trk_[0]->camera_, problems, &results, &moved, bf);
  for (size_t j = 0; j < problems.size(); j++) m.mm[whose[j]]->FinishBundle(windows[whose[j]], results[j], moved[j]);
}

}  // namespace sdvl
