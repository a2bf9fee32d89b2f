// farm_schedule_check.cc — FarmSchedule (farm_schedule.h) driven the way TrackerFarm drives it (farm.cc: RunShare, RunFeeder, the host-fed
// group-step), with fake group-steps: a sleep of a few pseudo-random microseconds instead of the device work.  No GPU, standard library
// only.  Prints "farm_schedule_check: ok" and returns 0, or names the first broken expectation and returns 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <thread>

#include "farm_schedule.h"

using sdvl::FarmSchedule;

namespace {

#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      std::fprintf(stderr, "farm_schedule_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

constexpr int kRingSlots = 3;

struct Case {
  int G, workers, n_steps;
  bool feeder = false;
  int fail_group = -1, fail_step = -1;  // that group-step reports failure
};

struct Executed { int g, s, thread; };

// One run of a case.  What the fake steps and the fake feeder see is checked where they see it; what was executed is checked at the end.
struct Run {
  const Case c;
  FarmSchedule sched;
  std::vector<std::atomic<int>> inside;  // [group] threads inside a step of the group
  std::vector<std::atomic<int>> booked;  // [group] transfers the feeder has queued (counted BEFORE it books them)
  std::vector<std::atomic<int>> slot;    // [group * kRingSlots + slot] the step whose images the slot holds
  std::vector<std::atomic<int>> begun;   // [group] steps the workers have finished (counted BEFORE the schedule is told)
  std::vector<std::atomic<int>> ended;   // [group] ... (counted AFTER the schedule was told)
  std::mutex log_m;
  std::vector<Executed> log;
  std::atomic<bool> feeder_returned{false};

  explicit Run(const Case &cs)
      : c(cs), inside(cs.G), booked(cs.G), slot(cs.G * kRingSlots), begun(cs.G), ended(cs.G) {
    for (auto &v : slot) v = -1;
  }

  static void Nap(std::minstd_rand *rng) { std::this_thread::sleep_for(std::chrono::microseconds(20 + (*rng)() % 200)); }

  // TrackerFarm::StepAndFinish with a fake StepGroup
  bool StepAndFinish(int g, int s, int thread, std::minstd_rand *rng) {
    int rc = 0;
    std::string message;
    if (c.feeder && !sched.WaitIssued(g, s)) {
      rc = -1;  // an echo of the failure that ended the run
    } else {
      EXPECT(inside[g].fetch_add(1) == 0);  // nobody else is inside a step of this group
      if (c.feeder) {
        EXPECT(booked[g].load() > s);                          // the step starts only after its transfer was queued
        EXPECT(slot[g * kRingSlots + s % kRingSlots] == s);    // ... and finds its own images in its slot
      }
      Nap(rng);
      if (c.feeder) EXPECT(slot[g * kRingSlots + s % kRingSlots] == s);  // still there: the feeder never ran a ring's length ahead
      {
        std::lock_guard<std::mutex> lk(log_m);
        log.push_back(Executed{g, s, thread});
      }
      if (g == c.fail_group && s == c.fail_step) {
        rc = -1;
        message = "step " + std::to_string(s) + " of group " + std::to_string(g) + " failed";
      }
      EXPECT(inside[g].fetch_sub(1) == 1);
    }
    begun[g]++;
    sched.Finish(g, rc, message);
    ended[g]++;
    return rc == 0;
  }

  // TrackerFarm::RunShare
  void Worker(int worker) {
    std::minstd_rand rng(20260000u + worker);
    if (c.workers == c.G) {  // owned: the worker's own group, all steps
      for (int s = 0; s < c.n_steps && !sched.Failed(); s++)
        if (!StepAndFinish(worker, s, worker, &rng)) return;
      return;
    }
    for (;;) {  // dynamic
      int s = -1;
      const int g = sched.TakeGroup(true, &s);
      if (g < 0) return;
      StepAndFinish(g, s, worker, &rng);
    }
  }

  // TrackerFarm::RunFeeder.  The schedule's counters change under its lock while this thread looks on, so the feeder's choice is
  // checked against bounds: `ended` never exceeds the schedule's count of completed steps and `begun` is never below it, and only this
  // thread changes the count of issued steps.
  void Feeder() {
    std::minstd_rand rng(20269999u);
    std::vector<int> issued(c.G, 0), ended_before(c.G);
    for (;;) {
      for (int k = 0; k < c.G; k++) ended_before[k] = ended[k];
      int s = -1;
      const int g = sched.NextFeed(true, &s);
      if (g < 0) break;
      EXPECT(g < c.G && s == issued[g] && s < c.n_steps);
      EXPECT(issued[g] - begun[g] < kRingSlots);  // the slot was free when it was chosen: issued - done <= 3 once it is booked
      for (int k = 0; k < c.G; k++)               // whoever was eligible before the choice was not passed over for a later step
        if (issued[k] < c.n_steps && issued[k] - ended_before[k] < kRingSlots) EXPECT(issued[g] <= issued[k]);
      Nap(&rng);
      slot[g * kRingSlots + s % kRingSlots] = s;
      booked[g]++;
      issued[g]++;
      sched.BookFeed(g, 0, "");
    }
    feeder_returned = true;
  }

  void Go() {
    sched.Reset(c.G, c.n_steps, kRingSlots);
    std::thread feeder;
    if (c.feeder) feeder = std::thread([this] { Feeder(); });
    std::vector<std::thread> threads;
    for (int w = 0; w < c.workers; w++) threads.emplace_back([this, w] { Worker(w); });
    for (auto &t : threads) t.join();
    if (feeder.joinable()) {
      feeder.join();  // it returns by itself: every step is issued, or the failure woke it
      EXPECT(feeder_returned);
    }
    // every group's executed steps are 0 .. k in order, each exactly once
    std::vector<int> next(c.G, 0);
    for (const Executed &e : log) {
      EXPECT(e.s == next[e.g]);
      next[e.g]++;
      if (c.workers == c.G) EXPECT(e.thread == e.g);  // owned: a group never leaves its thread
    }
    if (c.fail_group < 0) {
      EXPECT(!sched.Failed());
      for (int g = 0; g < c.G; g++) EXPECT(next[g] == c.n_steps);
    } else {
      EXPECT(sched.Failed());
      EXPECT(sched.Error() == "step " + std::to_string(c.fail_step) + " of group " + std::to_string(c.fail_group) + " failed");
      EXPECT(next[c.fail_group] == c.fail_step + 1);  // the failed group stopped there; the others stopped wherever they were
      for (int g = 0; g < c.G; g++) EXPECT(next[g] <= c.n_steps);
    }
  }
};

// the non-blocking forms, from one thread: every answer is known exactly
void SingleThreaded() {
  FarmSchedule sched;
  int s = -1;
  sched.Reset(2, 2, kRingSlots);
  EXPECT(sched.TakeGroup(false, &s) == 0 && s == 0);
  EXPECT(sched.TakeGroup(false, &s) == 1 && s == 0);
  EXPECT(sched.TakeGroup(false, &s) == FarmSchedule::kNotNow);  // everything that remains is busy
  sched.Finish(1, 0, "");
  EXPECT(sched.TakeGroup(false, &s) == 1 && s == 1);
  sched.Finish(0, 0, "");
  sched.Finish(1, 0, "");
  EXPECT(sched.TakeGroup(false, &s) == 0 && s == 1);  // group 1 is through; group 0 is what is left
  EXPECT(sched.TakeGroup(false, &s) == FarmSchedule::kNotNow);
  sched.Finish(0, 0, "");
  EXPECT(sched.TakeGroup(false, &s) == FarmSchedule::kNothingLeft);
  EXPECT(sched.TakeGroup(true, &s) == FarmSchedule::kNothingLeft);
  EXPECT(!sched.Failed());

  // the furthest behind first, the lower group among equals
  sched.Reset(3, 4, kRingSlots);
  EXPECT(sched.TakeGroup(false, &s) == 0);
  sched.Finish(0, 0, "");
  EXPECT(sched.TakeGroup(false, &s) == 1 && s == 0);
  EXPECT(sched.TakeGroup(false, &s) == 2 && s == 0);
  EXPECT(sched.TakeGroup(false, &s) == 0 && s == 1);

  // the feeder: the earliest unissued step among the groups with a free slot; a full ring waits for a finished step
  sched.Reset(2, 5, kRingSlots);
  for (int round = 0; round < kRingSlots; round++)
    for (int g = 0; g < 2; g++) {
      EXPECT(sched.NextFeed(false, &s) == g && s == round);
      sched.BookFeed(g, 0, "");
    }
  EXPECT(sched.NextFeed(false, &s) == FarmSchedule::kNotNow);  // issued - done == 3 in both groups
  EXPECT(sched.WaitIssued(1, 2));
  sched.Finish(1, 0, "");
  EXPECT(sched.NextFeed(false, &s) == 1 && s == 3);
  sched.BookFeed(1, 0, "");
  EXPECT(sched.NextFeed(false, &s) == FarmSchedule::kNotNow);
  sched.Finish(0, 0, "");
  sched.Finish(1, 0, "");
  EXPECT(sched.NextFeed(false, &s) == 0 && s == 3);  // both have a free slot: group 0's step 3 is earlier than group 1's step 4
  sched.BookFeed(0, 0, "");
  EXPECT(sched.NextFeed(false, &s) == 1 && s == 4);
  sched.BookFeed(1, 0, "");
  sched.Finish(0, 0, "");
  EXPECT(sched.NextFeed(false, &s) == 0 && s == 4);
  sched.BookFeed(0, 0, "");
  EXPECT(sched.NextFeed(false, &s) == FarmSchedule::kNothingLeft);
  EXPECT(sched.NextFeed(true, &s) == FarmSchedule::kNothingLeft);

  // the first failure is the cause, whoever reports it; it ends every wait
  sched.Reset(2, 3, kRingSlots);
  sched.Fail("first");
  sched.Fail("second");
  sched.BookFeed(0, -1, "third");
  sched.Finish(1, -1, "fourth");
  EXPECT(sched.Failed() && sched.Error() == "first");
  EXPECT(sched.TakeGroup(true, &s) == FarmSchedule::kNothingLeft);
  EXPECT(sched.NextFeed(true, &s) == FarmSchedule::kNothingLeft);
  EXPECT(!sched.WaitIssued(1, 2));
  sched.Reset(2, 3, kRingSlots);  // and a new run starts clean
  EXPECT(!sched.Failed() && sched.Error().empty());
}

}  // namespace

int main() {
  SingleThreaded();
  const Case cases[] = {
      {1, 1, 1},                  // the smallest run
      {3, 2, 0},                  // no steps
      {4, 4, 6},                  // owned
      {5, 2, 6},                  // dynamic
      {3, 2, 7, true},            // dynamic, host-fed: a feeder and rings of three slots
      {3, 2, 6, false, 1, 3},     // a failing group-step
      {3, 2, 6, true, 1, 3},      // ... with a feeder that has to return
      {3, 3, 6, true, 1, 3},      // ... owned
  };
  for (const Case &c : cases) {
    Run run(c);
    run.Go();
  }
  std::printf("farm_schedule_check: ok\n");
  return 0;
}
