// sampling_profile.cc — the SIGPROF sampler behind SDVL_PROFILE (sampling_profile.h)
#include "sampling_profile.h"

#include <cxxabi.h>
#include <dlfcn.h>
#include <execinfo.h>
#include <signal.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace sdvl {
namespace {
constexpr int kProfDepth = 24, kProfMax = 400000;
struct ProfSample { int n; void *pc[kProfDepth]; };
ProfSample *g_prof = nullptr;
std::atomic<int> g_prof_n{0};
void ProfHandler(int) {
  const int i = g_prof_n.fetch_add(1);
  if (i >= kProfMax) return;
  g_prof[i].n = backtrace(g_prof[i].pc, kProfDepth);
}
std::string ProfName(void *pc) {
  Dl_info info;
  if (dladdr(pc, &info) && info.dli_sname) {
    int st = 0;
    char *d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
    std::string r = (st == 0 && d) ? d : info.dli_sname;
    free(d);
    if (r.size() > 90) r.resize(90);
    return r;
  }
  if (dladdr(pc, &info) && info.dli_fname) {
    std::string f = info.dli_fname;
    const size_t k = f.rfind('/');
    return "[" + (k == std::string::npos ? f : f.substr(k + 1)) + "]";
  }
  return "[?]";
}
}  // namespace

void SamplingProfileStart() {
  if (!g_prof) g_prof = new ProfSample[kProfMax];
  g_prof_n = 0;
  void *warm[4];
  backtrace(warm, 4);  // loads libgcc outside the handler
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_handler = ProfHandler;
  sa.sa_flags = SA_RESTART;
  sigaction(SIGPROF, &sa, nullptr);
}

timer_t SamplingProfileThreadStart() {
  struct sigevent sev;
  memset(&sev, 0, sizeof(sev));
  sev.sigev_notify = SIGEV_THREAD_ID;
  sev.sigev_signo = SIGPROF;
  sev._sigev_un._tid = static_cast<pid_t>(syscall(SYS_gettid));
  timer_t t = nullptr;
  if (timer_create(CLOCK_THREAD_CPUTIME_ID, &sev, &t) != 0) return nullptr;
  struct itimerspec its = {{0, 1000000}, {0, 1000000}};
  timer_settime(t, 0, &its, nullptr);
  return t;
}

void SamplingProfileThreadStop(timer_t t) {
  if (t) timer_delete(t);
}

void SamplingProfileStopAndPrint() {
  const int n = std::min(g_prof_n.load(), kProfMax);
  std::map<std::string, int> self, incl, own;
  for (int i = 0; i < n; i++) {
    std::set<std::string> seen;
    bool mine = false;
    for (int d = 2; d < g_prof[i].n; d++) {  // 0 = handler, 1 = signal trampoline
      const std::string name = ProfName(g_prof[i].pc[d]);
      if (d == 2) self[name]++;
      if (seen.insert(name).second) incl[name]++;
      if (!mine && (name.compare(0, 4, "sdvl") == 0 || name.compare(0, 5, "void ") == 0 || name.compare(0, 5, "std::") == 0)) {
        // innermost frame of this repo's code (or a libstdc++ template instantiated in it): everything below it, HIP / HSA
        // / libc included, is charged to it
        if (name.compare(0, 4, "sdvl") == 0) { own[name]++; mine = true; }
      }
    }
    if (!mine) own[g_prof[i].n > 2 ? "(other threads) " + ProfName(g_prof[i].pc[g_prof[i].n - 1]) : "(empty)"]++;
  }
  auto dump = [&](const char *title, std::map<std::string, int> &m, int top) {
    std::vector<std::pair<int, std::string>> v;
    for (auto &kv : m) v.push_back({kv.second, kv.first});
    std::sort(v.rbegin(), v.rend());
    fprintf(stderr, "---- %s (%d samples of 1 ms CPU)\n", title, n);
    for (int i = 0; i < top && i < static_cast<int>(v.size()); i++) fprintf(stderr, "%6.2f%%  %s\n", 100.0 * v[i].first / std::max(1, n), v[i].second.c_str());
  };
  dump("charged to the innermost sdvl function (callees in HIP / HSA / libc included)", own, 40);
  dump("self", self, 25);
  dump("inclusive", incl, 30);
}

}  // namespace sdvl
