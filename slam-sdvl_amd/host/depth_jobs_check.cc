// depth_jobs_check.cc — DepthJobs (depth_jobs.h) driven the way batch_depth.cc drives it, with fake DepthImage headers over dummy
// pointers: no image is read, no GPU, none of the project's libraries.  Prints "depth_jobs_check: ok" and returns 0, or names the first
// broken expectation and returns 1.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "depth_jobs.h"

using sdvl::DepthImage;
using sdvl::DepthJobs;

namespace {

#define EXPECT(cond)                                                                    \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      std::fprintf(stderr, "depth_jobs_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                     \
    }                                                                                   \
  } while (0)

// whether fn throws a std::runtime_error whose text holds `part`
bool Throws(const std::function<void()> &fn, const char *part) {
  try {
    fn();
  } catch (const std::runtime_error &e) {
    return std::string(e.what()).find(part) != std::string::npos;
  }
  return false;
}

char pixels[4];  // addresses only
const DepthImage kF32 = DepthImage::Wrap(pixels, 640, 480, 2560, sdvl::DEPTH_F32, 1.0, false);
const DepthImage kU16 = DepthImage::Wrap(pixels + 1, 640, 480, 1408, sdvl::DEPTH_U16, 0.0002, true);
const DepthImage kRight = DepthImage::Wrap(pixels + 2, 640, 480, 704, sdvl::DEPTH_RIGHT8, 1.0, false);
const sdvl_depth_seed_params kRule = {0.1, 8.0, 0.05, 6, 0}, kOtherRule = {0.1, 9.0, 0.05, 6, 0};
const sdvl_stereo_params kStereo = {0.11, 0.3, 0.0, 192, 20, 80, 0, nullptr}, kOtherStereo = {0.12, 0.3, 0.0, 192, 20, 80, 0, nullptr};
const sdvl_frame *const kLeft = reinterpret_cast<const sdvl_frame *>(pixels + 3), *const kLeft2 = reinterpret_cast<const sdvl_frame *>(pixels);

void DepthList() {
  DepthJobs jobs;
  EXPECT(jobs.empty() && jobs.size() == 0 && jobs.items() == 0 && !jobs.rule() && !jobs.stereo() && jobs.width() == 0);
  EXPECT(jobs.AddDepth(7, &kF32, kRule, 5, 640, 480));
  EXPECT(!jobs.AddDepth(8, nullptr, kOtherRule, 9, 640, 480));  // no image: no job, the list does not advance, nothing is compared
  EXPECT(jobs.AddDepth(9, &kU16, kRule, 0, 640, 480));          // an empty range is a job
  jobs.Skip(4);
  EXPECT(jobs.AddDepth(2, &kU16, kRule, 3, 320, 240));
  EXPECT(jobs.size() == 3 && jobs.items() == 12 && !jobs.stereo() && jobs.rule() == &kRule && !jobs.stereo_rule());
  EXPECT(jobs.width() == 640 && jobs.height() == 480);  // the first job's
  const int owner[3] = {7, 9, 2}, begin[3] = {0, 5, 9}, end[3] = {5, 5, 12};
  const DepthImage *image[3] = {&kF32, &kU16, &kU16};
  for (int j = 0; j < 3; j++) {
    const DepthJobs::Range &r = jobs.ranges()[j];
    const sdvl_depth_job &jb = jobs.depth_jobs()[j];
    EXPECT(r.owner == owner[j] && r.begin == begin[j] && r.end == end[j] && jobs.JobOf(owner[j]) == j);
    EXPECT(jb.c_begin == begin[j] && jb.c_end == end[j]);
    EXPECT(jb.depth == image[j]->data && jb.on_device == (image[j]->on_device ? 1 : 0) && jb.stride == image[j]->step);
    EXPECT(jb.format == image[j]->format && jb.scale == image[j]->scale && jb.pad_ == 0);
  }
  EXPECT(jobs.JobOf(8) == -1 && jobs.JobOf(0) == -1);
}

void StereoList() {
  DepthJobs jobs;
  EXPECT(!jobs.AddStereo(0, kLeft, nullptr, kStereo, 4, 640, 480));
  EXPECT(jobs.AddStereo(1, kLeft, &kRight, kStereo, 4, 640, 480));
  EXPECT(jobs.AddStereo(3, kLeft2, &kRight, kStereo, 2, 640, 480));
  EXPECT(jobs.size() == 2 && jobs.items() == 6 && jobs.stereo() && jobs.stereo_rule() == &kStereo && !jobs.rule());
  const sdvl_stereo_job *jb = jobs.stereo_jobs();
  EXPECT(jb[0].left == kLeft && jb[0].right == kRight.data && jb[0].on_device == 0 && jb[0].stride == 704 && jb[0].c_begin == 0 && jb[0].c_end == 4);
  EXPECT(jb[1].left == kLeft2 && jb[1].stride == 704 && jb[1].c_begin == 4 && jb[1].c_end == 6);
  EXPECT(jobs.JobOf(0) == -1 && jobs.JobOf(1) == 0 && jobs.JobOf(3) == 1);
}

void Refusals() {
  EXPECT(Throws([] {
    DepthJobs jobs;
    jobs.AddDepth(0, &kF32, kRule, 1, 640, 480);
    jobs.AddDepth(1, &kF32, kOtherRule, 1, 640, 480);
  }, "the trackers of a batch share the depth seeding"));
  EXPECT(Throws([] {
    DepthJobs jobs;
    jobs.ShareDepthRule(kRule);
    jobs.ShareDepthRule(kOtherRule);
  }, "depth seeding rule"));
  EXPECT(Throws([] {
    DepthJobs jobs;
    jobs.AddStereo(0, kLeft, &kRight, kStereo, 1, 640, 480);
    jobs.AddStereo(1, kLeft, &kRight, kOtherStereo, 1, 640, 480);
  }, "share the stereo baseline and rule"));
  EXPECT(Throws([] { DepthJobs().AddDepth(0, &kRight, kRule, 1, 640, 480); }, "DEPTH_RIGHT8"));
  EXPECT(Throws([] { DepthJobs().AddStereo(0, kLeft, &kU16, kStereo, 1, 640, 480); }, "takes a right image (DEPTH_RIGHT8), not a depth image"));
  EXPECT(Throws([] {  // never both producers in one call: the one that comes second is refused, by its own message
    DepthJobs jobs;
    jobs.AddStereo(0, kLeft, &kRight, kStereo, 1, 640, 480);
    jobs.AddDepth(1, &kF32, kRule, 1, 640, 480);
  }, "depth seeding rule"));
  EXPECT(Throws([] {
    DepthJobs jobs;
    jobs.AddDepth(0, &kF32, kRule, 1, 640, 480);
    jobs.AddStereo(1, kLeft, &kRight, kStereo, 1, 640, 480);
  }, "share the stereo baseline and rule"));
  DepthJobs same;  // equal rules at two addresses are one rule
  const sdvl_depth_seed_params copy = kRule;
  EXPECT(same.AddDepth(0, &kF32, kRule, 1, 640, 480) && same.AddDepth(1, &kU16, copy, 1, 640, 480) && same.size() == 2);
}

}  // namespace

int main() {
  DepthList();
  StereoList();
  Refusals();
  std::printf("depth_jobs_check: ok\n");
  return 0;
}
