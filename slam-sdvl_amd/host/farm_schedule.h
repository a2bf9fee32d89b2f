// farm_schedule.h — the bookkeeping the threads of one farm run share (farm.h: the workers and the feeder of a TrackerFarm): which step
// every group has reached, which groups are taken, which transfers the feeder has queued, and the first failure.  Standard library
// only — no device call in here — so that host/farm_schedule_check.cc can drive it with fake group-steps on a CPU.
#ifndef SDVL_FARM_SCHEDULE_H_
#define SDVL_FARM_SCHEDULE_H_

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

namespace sdvl {

class FarmSchedule {
 public:
  static constexpr int kNothingLeft = -1;  // TakeGroup, NextFeed: every step is done / issued, or the run has failed
  static constexpr int kNotNow = -2;       // their non-blocking forms: every remaining group is busy / has a full ring

  void Reset(int n_groups, int n_steps, int ring_slots) {
    std::lock_guard<std::mutex> lk(m_);
    n_steps_ = n_steps;
    ring_slots_ = ring_slots;
    done_.assign(n_groups, 0);
    busy_.assign(n_groups, 0);
    issued_.assign(n_groups, 0);
    failed_ = false;
    error_.clear();
    work_wait_s_ = feed_wait_s_ = 0.0;
  }

  // Dynamic mode: the next (group, *step) for a worker — the idle group that is furthest behind, so that a descheduled or throttled
  // thread delays one group-step, not a whole group.  The group is the caller's until its Finish.  kNothingLeft; kNotNow only with
  // `may_block` false (otherwise it waits for a group to come free).
  int TakeGroup(bool may_block, int *step) {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      if (failed_) return kNothingLeft;
      int best = -1, remaining = 0;
      for (int k = 0; k < static_cast<int>(done_.size()); k++) {
        if (done_[k] < n_steps_) remaining++;
        if (!busy_[k] && done_[k] < n_steps_ && (best < 0 || done_[k] < done_[best])) best = k;
      }
      if (remaining == 0) return kNothingLeft;
      if (best >= 0) {
        busy_[best] = 1;
        *step = done_[best];
        return best;
      }
      if (!may_block) return kNotNow;
      cv_work_.wait(lk);
    }
  }

  // A group-step has returned, with status `rc` (0 = fine) and its message: the first failure is the cause, later ones are its echoes.
  // One form for a taken group and for a group its thread or fiber owns for the whole run (never marked busy, and nobody waits for it
  // in TakeGroup): a waiting worker may take the group, the feeder may refill the slot the step has read.
  void Finish(int g, int rc, const std::string &message) {
    {
      std::lock_guard<std::mutex> lk(m_);
      if (rc != 0) FailLocked(message);
      done_[g]++;
      busy_[g] = 0;
    }
    NotifyAll();
  }

  // Host-fed runs: wait until the feeder has queued the images of step s of group g.  False: the run has failed.
  bool WaitIssued(int g, int s) {
    std::unique_lock<std::mutex> lk(m_);
    const auto tw = std::chrono::steady_clock::now();
    cv_feed_.wait(lk, [&] { return issued_[g] > s || failed_; });
    work_wait_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    return !failed_;
  }

  // The feeder's next transfer: the group whose next step (*step) is the earliest among those with a free ring slot — step s may go
  // into its slot once step s - ring_slots is complete.  kNothingLeft; kNotNow only with `may_block` false.
  int NextFeed(bool may_block, int *step) {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      if (failed_) return kNothingLeft;
      bool left = false;
      int g = -1;
      for (int k = 0; k < static_cast<int>(issued_.size()); k++) {
        if (issued_[k] >= n_steps_) continue;
        left = true;
        if (issued_[k] - done_[k] < ring_slots_ && (g < 0 || issued_[k] < issued_[g])) g = k;
      }
      if (!left) return kNothingLeft;
      if (g >= 0) {
        *step = issued_[g];
        return g;
      }
      if (!may_block) return kNotNow;
      const auto tw = std::chrono::steady_clock::now();
      cv_feed_.wait(lk);
      feed_wait_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    }
  }

  // the transfer NextFeed chose has been queued (`rc` != 0: it could not be; the workers waiting for it see the failure)
  void BookFeed(int g, int rc, const std::string &message) {
    {
      std::lock_guard<std::mutex> lk(m_);
      if (rc != 0) FailLocked(message);
      issued_[g]++;
    }
    NotifyAll();
  }

  void Fail(const std::string &message) {
    {
      std::lock_guard<std::mutex> lk(m_);
      FailLocked(message);
    }
    NotifyAll();
  }

  bool Failed() {
    std::lock_guard<std::mutex> lk(m_);
    return failed_;
  }
  // the cause of a failed run, and the waiting times of the last run (seconds): read them once the run's threads have been joined
  const std::string &Error() const { return error_; }
  double work_wait_s() const { return work_wait_s_; }  // workers, inside WaitIssued (summed over groups)
  double feed_wait_s() const { return feed_wait_s_; }  // feeder, inside NextFeed

 private:
  void FailLocked(const std::string &message) {
    if (failed_) return;
    failed_ = true;
    error_ = message;
  }
  // Every change of state wakes both sides: a finished step frees a group for a worker and a ring slot for the feeder, a queued
  // transfer and a failure concern whoever waits.  A notify without a waiter costs no system call.
  void NotifyAll() {
    cv_work_.notify_all();
    cv_feed_.notify_all();
  }

  std::mutex m_;
  std::condition_variable cv_work_;  // workers waiting in TakeGroup
  std::condition_variable cv_feed_;  // feeder <-> workers: NextFeed, WaitIssued
  int n_steps_ = 0, ring_slots_ = 0;
  std::vector<int> done_;    // [group] completed steps
  std::vector<char> busy_;   // [group] taken by a worker (dynamic mode)
  std::vector<int> issued_;  // [group] steps whose images the feeder has queued
  bool failed_ = false;
  std::string error_;
  double work_wait_s_ = 0.0, feed_wait_s_ = 0.0;
};

}  // namespace sdvl

#endif  // SDVL_FARM_SCHEDULE_H_
