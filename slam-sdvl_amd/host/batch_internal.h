// batch_internal.h — what the translation units of SDVLBatch (batch.cc, batch_tables.cc, batch_reloc.cc, batch_tracked.cc,
// batch_host_step.cc, batch_depth.cc, batch_mapper.cc) share besides batch.h (not installed).  Helpers that run once per request or per
// tracker in a loop are inline here: the build has no link-time optimisation.
#ifndef SDVL_BATCH_INTERNAL_H_
#define SDVL_BATCH_INTERNAL_H_

#include <memory>
#include <vector>

#include "sdvl_host.h"
#include "host_internal.h"

namespace sdvl {

// the reference's mapper behind a tracker's Map pointer, or null (the plane-map stub, another Map implementation)
static inline MapperMap *AsMapperMap(Map *map) { return dynamic_cast<MapperMap *>(map); }

// What the stages of one step hand to each other.
struct SDVLBatch::Step {
  Step(const std::vector<Image> &i, FrameStats *st, int B) : imgs(i), stats(st), decision(B, 0) {}
  const std::vector<Image> &imgs;
  FrameStats *stats;
  std::vector<std::shared_ptr<Frame>> frames;  // this step's frame of every tracker
  // trackers that execute ProcessFrame this step / that relocalise first / that relocalised onto a keyframe no table can express
  std::vector<int> run, lost, host_run;
  std::vector<int> init;                  // trackers in the first-frame / second-frame state of the two-frame initialisation
  std::vector<char> decision;             // per tracker: 0 = tracking lost / not tracked, 1 = ordinary frame, 2 = new keyframe
  std::vector<std::shared_ptr<Frame>> kfs;     // the keyframes the mapping stage seeds, and whose they are
  std::vector<int> kf_owner;
  bool filter_begun = false;         // FilterCornersBegin(kfs) is queued
  // the frames' corner detection is queued: set by whoever queues it first — the look-ahead of the step before (TakeLookAhead), a
  // relocalisation (Reproject searches the new frame's corners), or the step itself behind its image alignment
  bool detected = false;
  std::unique_ptr<StageClock> clk;   // the host stage the step is in
  void Stage(int id) { clk.reset(new StageClock(id)); }
  int R() const { return static_cast<int>(run.size()); }
};

// What the stages of the sequential mappers' update (batch_mapper.cc) hand to each other.  Indices k run over the mappers that began an
// update this step.
struct SDVLBatch::MapStep {
  std::vector<MapperMap *> mm;
  std::vector<int> trk;  // whose mapper mm[k] is
  int M() const { return static_cast<int>(mm.size()); }
  std::vector<std::vector<sdvl_search_req>> per;  // the requests each mapper emitted for the next search
  std::vector<size_t> begin;                      // where those of mapper k lay in the last search, M + 1 entries
  std::vector<sdvl_search_res> res;               // its results
  bool dev_filter = false;                        // the candidate passes run the depth filter on the device:
  std::vector<std::vector<sdvl_depth_state>> per_st;  // one filter state per request, as emitted
  std::vector<sdvl_depth_state> states;               // ... of the last search
  std::vector<sdvl_depth_out> fout;                   // its outcomes
  sdvl_depth_params fparams;
  const MapperMap *measuring = nullptr;        // a mapper with depth or stereo mapping on (SDVL::SetDepthMapping, SetStereoMapping), if the step has one
  int measuring_trk = -1;                      // whose it is
  std::vector<const DepthImage *> depth_of;    // the depth image (stereo mapping: the right image) mapper k's requests are measured in, null: none
  std::vector<uint8_t> depth_status;           // per candidate request, with `measuring`
  std::vector<int> kf_idx;                     // the mappers whose update takes a new keyframe
  std::unique_ptr<StageClock> sub;             // the ST_MAP_* stage the update is in
};

// the requests of per.size() sources behind each other: (*begin)[k] = where those of source k start, the last entry = their number.
// all == nullptr: the offsets alone (the caller packs the requests itself)
static inline void Concatenate(const std::vector<std::vector<sdvl_search_req>> &per, std::vector<sdvl_search_req> *all, std::vector<size_t> *begin) {
  begin->resize(per.size() + 1);
  size_t total = 0;
  for (size_t k = 0; k < per.size(); k++) {
    (*begin)[k] = total;
    total += per[k].size();
    if (all) all->insert(all->end(), per[k].begin(), per[k].end());
  }
  (*begin)[per.size()] = total;
}

}  // namespace sdvl

#endif  // SDVL_BATCH_INTERNAL_H_
