// track_scratch_check.cc — the tail of a track set's scratch (csrc/sdvl_track.hip, sdvl_track_create: ... | chain | pjobs | obs | hyp | pres |
// lists | nobs) as sdvl_layout.h cuts it, for a set whose pose stage runs on separate launches (<= 4 trackers: job and hypothesis records
// lie between them) and for one whose pose stage is one launch (more than 4: both parts are empty).  Built with the host compiler under
// AddressSanitizer and UBSan (test_track_scratch_layout_cpu.py).  Record sizes are parameters: the statement is about the parts, that an
// empty part takes nothing and shares its offset with the next one, and that nothing else moves except by the bytes saved.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "sdvl_layout.h"

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

template <int N>
struct Rec {
  uint8_t b[N];
};
typedef Rec<88> ChainRec;    // ChainFrameDev
typedef Rec<80> JobRec;      // PoseJobDev
typedef Rec<48> ObsRec;      // sdvl_pose_obs
typedef Rec<64> HypRec;      // one hypothesis record (sdvl_pose_hyp_bytes())
typedef Rec<72> ResultRec;   // sdvl_pose_result

struct Tail {
  sdvl_part<ChainRec> chain;
  sdvl_part<JobRec> pjobs;
  sdvl_part<ObsRec> obs;
  sdvl_part<uint8_t> hyp;
  sdvl_part<ResultRec> pres;
  sdvl_part<int32_t> lists, nobs;
  size_t bytes;
};

static bool separate_launches(size_t n) { return n <= 4; }  // sdvl_pose_separate_launches

static Tail take_tail(size_t n, size_t mm, size_t max_its) {
  sdvl_layout L;
  Tail t;
  const bool separate = separate_launches(n);
  t.chain = L.take<ChainRec>(n);
  t.pjobs = L.take<JobRec>(separate ? n : 0);
  t.obs = L.take<ObsRec>(n * mm);
  t.hyp = L.take<uint8_t>(separate ? sizeof(HypRec) * n * max_its : 0);
  t.pres = L.take<ResultRec>(n);
  t.lists = L.take<int32_t>(n * mm);
  t.nobs = L.take<int32_t>(n);
  t.bytes = L.bytes();
  return t;
}

// every part filled with a pattern of its own and read back: overlapping parts would disturb each other, a part outside the block is
// what the sanitizer reports
static void fill_and_read_back(const Tail &t) {
  uint8_t *block = static_cast<uint8_t *>(malloc(t.bytes ? t.bytes : 1));
  CHECK(block != nullptr);
  const size_t off[7] = {t.chain.off, t.pjobs.off, t.obs.off, t.hyp.off, t.pres.off, t.lists.off, t.nobs.off};
  const size_t len[7] = {t.chain.bytes(), t.pjobs.bytes(), t.obs.bytes(), t.hyp.bytes(), t.pres.bytes(), t.lists.bytes(), t.nobs.bytes()};
  for (int i = 0; i < 7; i++) memset(block + off[i], 0x11 * (i + 1), len[i]);
  for (int i = 0; i < 7; i++)
    for (size_t k = 0; k < len[i]; k++) CHECK(block[off[i] + k] == static_cast<uint8_t>(0x11 * (i + 1)));
  free(block);
}

int main() {
  const size_t mm = 200, its = 100;
  for (size_t n : {1, 4}) {  // separate launches: both record parts exist
    const Tail t = take_tail(n, mm, its);
    CHECK(t.pjobs.bytes() == 80 * n && t.hyp.bytes() == 64 * n * its);
    CHECK(t.obs.off == t.pjobs.off + sdvl_align256(t.pjobs.bytes()));
    CHECK(t.pres.off == t.hyp.off + sdvl_align256(t.hyp.bytes()));
    fill_and_read_back(t);
  }
  for (size_t n : {5, 16, 33, 256}) {  // one launch: no job records, no hypothesis records
    const Tail t = take_tail(n, mm, its);
    CHECK(t.pjobs.count == 0 && t.pjobs.bytes() == 0 && t.pjobs.off == t.obs.off);
    CHECK(t.hyp.count == 0 && t.hyp.bytes() == 0 && t.hyp.off == t.pres.off);
    // against the same set with the records: smaller by exactly their padded sizes, every part 256-aligned
    const size_t saved = sdvl_align256(80 * n) + sdvl_align256(64 * n * its);
    sdvl_layout F;
    F.take<ChainRec>(n); F.take<JobRec>(n); F.take<ObsRec>(n * mm); F.take<uint8_t>(sizeof(HypRec) * n * its);
    F.take<ResultRec>(n); F.take<int32_t>(n * mm); F.take<int32_t>(n);
    CHECK(F.bytes() == t.bytes + saved);
    if (n == 256) CHECK(64 * n * its == 1638400);  // the 1.6 MB per group of 256 at 100 draws
    for (size_t o : {t.chain.off, t.pjobs.off, t.obs.off, t.hyp.off, t.pres.off, t.lists.off, t.nobs.off}) CHECK(o % 256 == 0);
    fill_and_read_back(t);
  }
  printf("track scratch ok\n");
  return 0;
}
