// depth_jobs.h — the job list of ONE device call that reads a second image per frame: a registered depth image (sdvl_depth_seed,
// sdvl_depth_lookup, sdvl_search_run_filter_measured) or a stereo pair's right image (sdvl_stereo_depth, sdvl_search_run_filter_stereo).  The callers (batch_depth.cc)
// name the owners of a call — keyframes, mappers — in the order their items lie in the call's item list; the builder makes the jobs,
// checks what the owners of one call must share, and hands each owner's range of the results back.  It includes nothing of the device
// layer beyond the C-ABI's structs, so host/depth_jobs_check.cc drives it without a device.
#ifndef SDVL_DEPTH_JOBS_H_
#define SDVL_DEPTH_JOBS_H_

#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/sdvl_hip.h"
#include "types.h"

namespace sdvl {

class DepthJobs {
 public:
  struct Range { int owner, begin, end; };  // the items [begin, end) of the call's list are owner's; ranges()[j] belongs to job j

  // What the owners of one call share: one producer, and that producer's rule (compared as bytes; the rule is kept by address)
  void ShareDepthRule(const sdvl_depth_seed_params &rule) {
    if (stereo_rule_ || (rule_ && std::memcmp(rule_, &rule, sizeof(rule)) != 0))
      throw std::runtime_error("SDVLBatch: the trackers of a batch share the depth seeding rule");
    rule_ = &rule;
  }
  void ShareStereoRule(const sdvl_stereo_params &rule) {
    if (rule_ || (stereo_rule_ && std::memcmp(stereo_rule_, &rule, sizeof(rule)) != 0))
      throw std::runtime_error("SDVLBatch: the trackers of a batch share the stereo baseline and rule");
    stereo_rule_ = &rule;
  }
  // The next n items of the list are owner's, read in depth image d of a width x height frame.  false: no image (d null), no job, and
  // the list does not advance
  bool AddDepth(int owner, const DepthImage *d, const sdvl_depth_seed_params &rule, int n, int width, int height) {
    if (!d) return false;
    ShareDepthRule(rule);
    if (d->format == DEPTH_RIGHT8)
      throw std::runtime_error("SDVLBatch: a right image (DEPTH_RIGHT8) is no depth image: a tracker that seeds from a stereo pair reads it");
    depth_.push_back(sdvl_depth_job{d->data, d->on_device ? 1 : 0, d->step, d->format, 0, d->scale, at_, at_ + n});
    Record(owner, n, width, height);
    return true;
  }
  // the same for a stereo pair: `left` the frame whose corners the items are, d its right image
  bool AddStereo(int owner, const sdvl_frame *left, const DepthImage *d, const sdvl_stereo_params &rule, int n, int width, int height) {
    if (!d) return false;
    ShareStereoRule(rule);
    if (d->format != DEPTH_RIGHT8)
      throw std::runtime_error("SDVLBatch: a tracker that seeds from a stereo pair takes a right image (DEPTH_RIGHT8), not a depth image");
    stereo_.push_back(sdvl_stereo_job{left, d->data, d->on_device ? 1 : 0, d->step, at_, at_ + n});
    Record(owner, n, width, height);
    return true;
  }
  void Skip(int n) { at_ += n; }  // n items of the list that no job names

  bool empty() const { return ranges_.empty(); }
  int size() const { return static_cast<int>(ranges_.size()); }
  int items() const { return at_; }  // the length of the list so far
  bool stereo() const { return stereo_rule_ != nullptr; }
  const sdvl_depth_job *depth_jobs() const { return depth_.data(); }
  const sdvl_stereo_job *stereo_jobs() const { return stereo_.data(); }
  const sdvl_depth_seed_params *rule() const { return rule_; }  // null: no depth job yet
  const sdvl_stereo_params *stereo_rule() const { return stereo_rule_; }
  int width() const { return width_; }  // of the first job's frame (the frames of a batch have one size); 0 without a job
  int height() const { return height_; }
  const std::vector<Range> &ranges() const { return ranges_; }
  int JobOf(int owner) const {  // -1: the owner has none
    for (size_t j = 0; j < ranges_.size(); j++)
      if (ranges_[j].owner == owner) return static_cast<int>(j);
    return -1;
  }

 private:
  void Record(int owner, int n, int width, int height) {
    if (ranges_.empty()) { width_ = width; height_ = height; }
    ranges_.push_back(Range{owner, at_, at_ + n});
    at_ += n;
  }
  std::vector<sdvl_depth_job> depth_;
  std::vector<sdvl_stereo_job> stereo_;
  std::vector<Range> ranges_;
  const sdvl_depth_seed_params *rule_ = nullptr;
  const sdvl_stereo_params *stereo_rule_ = nullptr;
  int at_ = 0, width_ = 0, height_ = 0;
};

}  // namespace sdvl

#endif  // SDVL_DEPTH_JOBS_H_
