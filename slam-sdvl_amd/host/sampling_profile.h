// sampling_profile.h — SDVL_PROFILE=1: a sampling profile of the host threads during TrackerFarm::Run (the boxes have no perf): SIGPROF
// every millisecond of a thread's CPU time, the handler records the call stack, the run prints self / inclusive shares on stderr.
#ifndef SDVL_SAMPLING_PROFILE_H_
#define SDVL_SAMPLING_PROFILE_H_

#include <time.h>

namespace sdvl {

void SamplingProfileStart();  // once, before the threads to be sampled start: installs the handler, forgets earlier samples
// one CPU-time timer per sampled thread (a process-wide ITIMER_PROF fires once per scheduler tick for the whole process): called by the
// thread itself when it starts and before it ends; a null timer (it could not be created) is accepted
timer_t SamplingProfileThreadStart();
void SamplingProfileThreadStop(timer_t t);
void SamplingProfileStopAndPrint();  // once the sampled threads have ended

}  // namespace sdvl

#endif  // SDVL_SAMPLING_PROFILE_H_
