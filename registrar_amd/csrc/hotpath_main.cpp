// hotpath_main.cpp — per-thread profile of the re-register + heartbeat cycle.
//
// Runs the same workload bench.py times (one ZkClient against an in-process
// one-IO-thread Ensemble; domain rank0.bench.mi355x, hostname + N-1 aliases,
// settleMs 0) and reports, per step and per thread (ensemble IO, client
// loop, caller):
//   - CPU µs from /proc/self/task/<tid>/schedstat,
//   - allocation count and bytes from the counting operator new below
//     (defined in this program only; deterministic, so it is the noise-free
//     before/after figure),
//   - wall ms per step.
// The ensemble thread's allocations are also split by phase: the register
// phase, the heartbeat phase (exists only) and a delete-only batch, so the
// per-op allocation cost of each handler can be read off directly.
//
// Usage: hotpath [N znodes = 1000] [K steps = 200] [warmup = 20]
// Output: a human-readable table on stderr, one JSON line on stdout.
//
// Threads are told apart by diffing /proc/self/task around Ensemble::start()
// and ZkClient::start() and are then given names (ens-io / zk-loop / caller)
// through /proc/self/task/<tid>/comm, so the tool needs nothing from the
// library and can be built against any revision of it.
//
// Built with -DHOTPATH_PROF (make hotpath-prof, which adds -rdynamic
// -fno-omit-frame-pointer) the same program is also a sampling profiler of
// the ensemble IO thread: ITIMER_PROF ticks, the handler keeps the samples
// that land on that thread (PC from the ucontext plus up to four return
// addresses found by walking frame pointers inside that thread's stack; no
// libc calls in the handler), and at exit self time per symbol and the most
// common 4-deep chains are printed to stderr. The timer is tick-based: run
// enough steps for a few thousand samples.
#include <dirent.h>
#include <signal.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "ensemble.hpp"
#include "registrar.hpp"
#include "zkclient.hpp"

#ifdef HOTPATH_PROF
#if !defined(__x86_64__)
#error "hotpath-prof reads x86-64 registers from the signal context"
#endif
#include <cxxabi.h>
#include <dlfcn.h>
#include <sys/time.h>
#include <ucontext.h>

#include <algorithm>
#include <map>
#endif

using namespace registrar;

// ---------------------------------------------------------------------------
// counting allocator: one slot per thread, claimed on the thread's first
// allocation; only the owning thread writes its slot

namespace {
struct AllocSlot {
  std::atomic<long> tid{0};
  std::atomic<uint64_t> count{0};
  std::atomic<uint64_t> bytes{0};
};
constexpr int kMaxSlots = 256;
AllocSlot g_slots[kMaxSlots];
std::atomic<int> g_next_slot{0};
thread_local AllocSlot* t_slot = nullptr;

inline void count_alloc(size_t n) {
  AllocSlot* s = t_slot;
  if (!s) {
    int i = g_next_slot.fetch_add(1);
    if (i >= kMaxSlots) return;
    s = &g_slots[i];
    s->tid.store(syscall(SYS_gettid));
    t_slot = s;
  }
  s->count.store(s->count.load(std::memory_order_relaxed) + 1, std::memory_order_relaxed);
  s->bytes.store(s->bytes.load(std::memory_order_relaxed) + n, std::memory_order_relaxed);
}

void* counted_alloc(size_t n) {
  count_alloc(n);
  void* p = malloc(n ? n : 1);
  if (!p) throw std::bad_alloc();
  return p;
}
void* counted_alloc_aligned(size_t n, size_t al) {
  count_alloc(n);
  void* p = nullptr;
  if (posix_memalign(&p, al < sizeof(void*) ? sizeof(void*) : al, n ? n : 1) != 0) throw std::bad_alloc();
  return p;
}
}  // namespace

void* operator new(size_t n) { return counted_alloc(n); }
void* operator new[](size_t n) { return counted_alloc(n); }
void* operator new(size_t n, std::align_val_t al) { return counted_alloc_aligned(n, static_cast<size_t>(al)); }
void* operator new[](size_t n, std::align_val_t al) { return counted_alloc_aligned(n, static_cast<size_t>(al)); }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
void operator delete[](void* p, size_t) noexcept { free(p); }
void operator delete(void* p, std::align_val_t) noexcept { free(p); }
void operator delete[](void* p, std::align_val_t) noexcept { free(p); }
void operator delete(void* p, size_t, std::align_val_t) noexcept { free(p); }
void operator delete[](void* p, size_t, std::align_val_t) noexcept { free(p); }

namespace {

std::set<long> list_tids() {
  std::set<long> out;
  DIR* d = opendir("/proc/self/task");
  if (!d) return out;
  while (struct dirent* e = readdir(d))
    if (e->d_name[0] != '.') out.insert(atol(e->d_name));
  closedir(d);
  return out;
}

std::vector<long> new_tids(const std::set<long>& before) {
  std::vector<long> out;
  for (long t : list_tids())
    if (!before.count(t)) out.push_back(t);
  return out;
}

void name_thread(long tid, const char* name) {
  char path[64];
  snprintf(path, sizeof(path), "/proc/self/task/%ld/comm", tid);
  if (FILE* f = fopen(path, "w")) {
    fputs(name, f);
    fclose(f);
  }
}

// on-CPU time of one thread in ns (first field of schedstat)
uint64_t cpu_ns(long tid) {
  char path[64];
  snprintf(path, sizeof(path), "/proc/self/task/%ld/schedstat", tid);
  unsigned long long run = 0;
  if (FILE* f = fopen(path, "r")) {
    if (fscanf(f, "%llu", &run) != 1) run = 0;
    fclose(f);
  }
  return run;
}

struct Sample {
  uint64_t cpu = 0, allocs = 0, bytes = 0;
};

// allocation counters only (no /proc read: cheap enough to take per phase)
Sample sample_allocs(long tid) {
  Sample s;
  for (int i = 0; i < kMaxSlots; i++) {
    if (g_slots[i].tid.load() == tid) {
      s.allocs = g_slots[i].count.load(std::memory_order_relaxed);
      s.bytes = g_slots[i].bytes.load(std::memory_order_relaxed);
      break;
    }
  }
  return s;
}

Sample sample(long tid) {
  Sample s = sample_allocs(tid);
  s.cpu = cpu_ns(tid);
  return s;
}

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

#ifdef HOTPATH_PROF
// ---------------------------------------------------------------------------
// sampler (see the header comment)

namespace {
constexpr int kChain = 5;  // PC + 4 return addresses
constexpr size_t kMaxSamples = 1 << 18;
struct ProfSample {
  uintptr_t pc[kChain];
};
ProfSample* g_samples = nullptr;
volatile size_t g_nsamples = 0;
volatile size_t g_other_thread = 0;  // ticks that landed elsewhere
uintptr_t g_stack_lo = 0, g_stack_hi = 0;  // the ens-io thread's stack mapping

// Async-signal-safe by construction: reads registers, reads words inside
// [g_stack_lo, g_stack_hi), writes preallocated memory. Nothing else.
void on_sigprof(int, siginfo_t*, void* uc_) {
  ucontext_t* uc = static_cast<ucontext_t*>(uc_);
  uintptr_t sp = static_cast<uintptr_t>(uc->uc_mcontext.gregs[REG_RSP]);
  if (sp < g_stack_lo || sp >= g_stack_hi) {  // not the ens-io thread
    g_other_thread = g_other_thread + 1;
    return;
  }
  size_t i = g_nsamples;
  if (i >= kMaxSamples) return;
  ProfSample& s = g_samples[i];
  s.pc[0] = static_cast<uintptr_t>(uc->uc_mcontext.gregs[REG_RIP]);
  uintptr_t fp = static_cast<uintptr_t>(uc->uc_mcontext.gregs[REG_RBP]);
  uintptr_t floor = sp;
  for (int d = 1; d < kChain; d++) {
    s.pc[d] = 0;
    // a frame record is two words, above everything already walked
    if (fp < floor || fp + 16 > g_stack_hi || (fp & 7) != 0) {
      fp = 0;
      continue;
    }
    const uintptr_t* rec = reinterpret_cast<const uintptr_t*>(fp);
    s.pc[d] = rec[1];
    floor = fp + 16;
    fp = rec[0];
  }
  g_nsamples = i + 1;
}

// The stack of a thread that is blocked in a system call: its stack pointer
// from /proc/self/task/<tid>/syscall, widened to the readable mapping that
// holds it.
bool find_stack(long tid, uintptr_t* lo, uintptr_t* hi) {
  char path[64], line[512];
  snprintf(path, sizeof(path), "/proc/self/task/%ld/syscall", tid);
  uintptr_t sp = 0;
  for (int attempt = 0; attempt < 50 && !sp; attempt++) {
    if (FILE* f = fopen(path, "r")) {
      if (fgets(line, sizeof(line), f)) {
        // "<nr> <6 args> <sp> <pc>", or "running"
        std::vector<std::string> tok;
        for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.size() >= 3) sp = strtoull(tok[tok.size() - 2].c_str(), nullptr, 16);
      }
      fclose(f);
    }
    if (!sp) usleep(2000);
  }
  if (!sp) return false;
  FILE* f = fopen("/proc/self/maps", "r");
  if (!f) return false;
  bool ok = false;
  while (fgets(line, sizeof(line), f)) {
    unsigned long long a = 0, b = 0;
    char perms[8] = {0};
    if (sscanf(line, "%llx-%llx %7s", &a, &b, perms) == 3 && sp >= a && sp < b && perms[0] == 'r') {
      *lo = a;
      *hi = b;
      ok = true;
      break;
    }
  }
  fclose(f);
  return ok;
}

bool prof_arm(long ens_tid) {
  if (!find_stack(ens_tid, &g_stack_lo, &g_stack_hi)) {
    fprintf(stderr, "hotpath-prof: cannot locate the ens-io thread's stack\n");
    return false;
  }
  g_samples = static_cast<ProfSample*>(calloc(kMaxSamples, sizeof(ProfSample)));
  if (!g_samples) return false;
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_sigaction = on_sigprof;
  sa.sa_flags = SA_SIGINFO | SA_RESTART;
  sigemptyset(&sa.sa_mask);
  sigaction(SIGPROF, &sa, nullptr);
  struct itimerval it;
  it.it_interval.tv_sec = 0;
  it.it_interval.tv_usec = 1000;
  it.it_value = it.it_interval;
  return setitimer(ITIMER_PROF, &it, nullptr) == 0;
}

void prof_disarm() {
  struct itimerval it;
  memset(&it, 0, sizeof(it));
  setitimer(ITIMER_PROF, &it, nullptr);
  signal(SIGPROF, SIG_IGN);
}

// is_return: a return address names the instruction AFTER the call
std::string symbol_of(uintptr_t pc, bool is_return) {
  if (!pc) return "-";
  Dl_info info;
  memset(&info, 0, sizeof(info));
  void* addr = reinterpret_cast<void*>(is_return ? pc - 1 : pc);
  char buf[96];
  if (dladdr(addr, &info) && info.dli_sname) {
    int st = 0;
    char* dem = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
    std::string out = (st == 0 && dem) ? dem : info.dli_sname;
    free(dem);
    if (out.size() > 110) out = out.substr(0, 107) + "...";
    return out;
  }
  if (info.dli_fname) {
    // no dynamic symbol (a local function, an IFUNC variant): the module
    // offset, rounded down to 256 bytes so one function's samples add up;
    // addr2line -e <module> <offset> names it
    const char* base = strrchr(info.dli_fname, '/');
    snprintf(buf, sizeof(buf), "%s+0x%llx..", base ? base + 1 : info.dli_fname,
             static_cast<unsigned long long>((pc - reinterpret_cast<uintptr_t>(info.dli_fbase)) & ~0xFFull));
  } else {
    snprintf(buf, sizeof(buf), "0x%llx", static_cast<unsigned long long>(pc));
  }
  return buf;
}

void prof_report() {
  size_t n = g_nsamples;
  fprintf(stderr,
          "\nhotpath-prof: %zu samples on ens-io, %zu ticks on other threads (ITIMER_PROF asked for 1 ms; the kernel "
          "delivers at its own tick rate)\n",
          n, static_cast<size_t>(g_other_thread));
  if (!n) return;
  std::map<std::string, size_t> self, chains;
  for (size_t i = 0; i < n; i++) {
    const ProfSample& s = g_samples[i];
    self[symbol_of(s.pc[0], false)]++;
    std::string c = symbol_of(s.pc[0], false);
    for (int d = 1; d < 4; d++) c += " <- " + symbol_of(s.pc[d], true);
    chains[c]++;
  }
  auto top = [&](const std::map<std::string, size_t>& m, size_t k, const char* title) {
    std::vector<std::pair<size_t, std::string>> v;
    for (auto& kv : m) v.push_back({kv.second, kv.first});
    std::sort(v.begin(), v.end(), [](auto& a, auto& b) { return a.first > b.first; });
    fprintf(stderr, "--- %s ---\n", title);
    for (size_t i = 0; i < v.size() && i < k; i++)
      fprintf(stderr, "%6.2f%% %6zu  %s\n", 100.0 * v[i].first / n, v[i].first, v[i].second.c_str());
  };
  top(self, 40, "self time per symbol");
  top(chains, 25, "most common 4-deep chains (leaf <- callers)");
}
}  // namespace
#endif  // HOTPATH_PROF

int main(int argc, char** argv) {
  signal(SIGPIPE, SIG_IGN);
  int n = argc > 1 ? atoi(argv[1]) : 1000;
  int steps = argc > 2 ? atoi(argv[2]) : 200;
  int warmup = argc > 3 ? atoi(argv[3]) : 20;
  if (n < 1 || steps < 1 || warmup < 0) {
    fprintf(stderr, "usage: hotpath [N znodes >= 1] [K steps >= 1] [warmup >= 0]\n");
    return 2;
  }

  Logger log("hotpath");
  log.set_level(LogLevel::Warn);
  long caller_tid = syscall(SYS_gettid);
  name_thread(caller_tid, "caller");

  zk::EnsembleConfig ecfg;
  ecfg.ports = {0};
  ecfg.io_threads = 1;
  ecfg.max_session_timeout_ms = 60000;
  zk::Ensemble ens(ecfg);
  std::set<long> before = list_tids();
  ens.start();
  std::vector<long> ens_tids = new_tids(before);
  if (ens_tids.size() != 1) {
    fprintf(stderr, "hotpath: expected 1 ensemble IO thread, found %zu\n", ens_tids.size());
    return 1;
  }
  long ens_tid = ens_tids[0];
  name_thread(ens_tid, "ens-io");

  zk::ZkClientConfig ccfg;
  ccfg.servers.push_back({"127.0.0.1", ens.ports()[0]});
  ccfg.session_timeout_ms = 40000;
  ccfg.randomize_start = false;
  zk::ZkClient client(std::move(ccfg), log);
  before = list_tids();
  client.start();
  std::vector<long> cli_tids = new_tids(before);
  if (cli_tids.size() != 1 || !client.wait_connected(10000)) {
    fprintf(stderr, "hotpath: client did not start/connect\n");
    return 1;
  }
  long cli_tid = cli_tids[0];
  name_thread(cli_tid, "zk-loop");

  RegistrationConfig reg;
  reg.domain = "rank0.bench.mi355x";
  reg.type = "host";
  reg.admin_ip = "127.0.0.1";
  reg.hostname = "bench-r0";
  reg.settle_ms = 0;
  for (int i = 0; i < n - 1; i++) {
    char buf[64];
    snprintf(buf, sizeof(buf), "a%04d.rank0.bench.mi355x", i);
    reg.aliases.push_back(buf);
  }
  PreparedRegistration prep = prepare_registration(reg);
  zk::RetryPolicy retry;

  auto step = [&](Sample* ens_mid) -> bool {
    RegisterResult res = register_prepared(client, prep, log);
    if (res.rc != zk::kZOk) {
      fprintf(stderr, "hotpath: register failed: %s\n", res.error.c_str());
      return false;
    }
    if (ens_mid) *ens_mid = sample_allocs(ens_tid);
    int64_t rtt = 0;
    int rc = heartbeat_prepared(client, prep, retry, &rtt);
    if (rc != zk::kZOk) {
      fprintf(stderr, "hotpath: heartbeat failed: %s\n", zk::error_name(rc));
      return false;
    }
    return true;
  };

  for (int i = 0; i < warmup; i++)
    if (!step(nullptr)) return 1;

#ifdef HOTPATH_PROF
  if (!prof_arm(ens_tid)) return 1;
#endif

  const long tids[3] = {ens_tid, cli_tid, caller_tid};
  const char* names[3] = {"ens-io", "zk-loop", "caller"};
  Sample s0[3], s1[3];
  uint64_t ens_reg_allocs = 0, ens_hb_allocs = 0;
  // tree locks over the timed steps: read outside the sampled window (the
  // counter map allocates on the calling thread)
  auto c0 = ens.counters();
  for (int t = 0; t < 3; t++) s0[t] = sample(tids[t]);
  double t0 = now_s();
  for (int i = 0; i < steps; i++) {
    Sample a = sample_allocs(ens_tid), mid;
    if (!step(&mid)) return 1;
    Sample b = sample_allocs(ens_tid);
    ens_reg_allocs += mid.allocs - a.allocs;
    ens_hb_allocs += b.allocs - mid.allocs;
  }
  double wall = now_s() - t0;
  for (int t = 0; t < 3; t++) s1[t] = sample(tids[t]);
  auto c1 = ens.counters();
  // every exists takes exactly one shard lock and the heartbeat is nothing
  // but exists, so the rest of a step's locks belong to its register phase
  double locks_step = static_cast<double>(c1["tree_locks"] - c0["tree_locks"]) / steps;
  double locks_register = locks_step - static_cast<double>(c1["exists"] - c0["exists"]) / steps;
#ifdef HOTPATH_PROF
  prof_disarm();
#endif

  // delete-only batches (the unregister path), re-registering in between;
  // only the delete batch is counted
  int del_rounds = steps < 5 ? steps : 5;
  uint64_t ens_del_allocs = 0;
  for (int i = 0; i < del_rounds; i++) {
    Sample a = sample_allocs(ens_tid);
    std::vector<int> rcs = client.delete_many(prep.nodes);
    Sample b = sample_allocs(ens_tid);
    for (int rc : rcs)
      if (rc != zk::kZOk) {
        fprintf(stderr, "hotpath: delete failed: %s\n", zk::error_name(rc));
        return 1;
      }
    ens_del_allocs += b.allocs - a.allocs;
    if (!step(nullptr)) return 1;
  }

  auto counters = ens.counters();
  client.close();
  ens.stop();

  double k = static_cast<double>(steps);
  fprintf(stderr, "hotpath: N=%d znodes, %d steps (+%d warmup), wall %.3f ms/step\n", n, steps, warmup,
          wall / k * 1e3);
  fprintf(stderr, "%-8s %12s %14s %14s\n", "thread", "cpu_us/step", "allocs/step", "bytes/step");
  for (int t = 0; t < 3; t++)
    fprintf(stderr, "%-8s %12.1f %14.1f %14.0f\n", names[t], (s1[t].cpu - s0[t].cpu) / k / 1e3,
            (s1[t].allocs - s0[t].allocs) / k, (s1[t].bytes - s0[t].bytes) / k);
  fprintf(stderr, "ens-io allocs by phase: register %.1f/step, heartbeat(exists) %.1f/step, delete-only %.1f/batch\n",
          ens_reg_allocs / k, ens_hb_allocs / k, ens_del_allocs / static_cast<double>(del_rounds));
  fprintf(stderr, "tree locks: %.1f/step, of which register %.1f/step\n", locks_step, locks_register);

  printf("{\"tool\": \"hotpath\", \"znodes\": %d, \"steps\": %d, \"warmup\": %d, \"wall_ms_per_step\": %.4f", n,
         steps, warmup, wall / k * 1e3);
  const char* keys[3] = {"ens_io", "zk_loop", "caller"};
  for (int t = 0; t < 3; t++)
    printf(", \"%s\": {\"cpu_us_per_step\": %.1f, \"allocs_per_step\": %.1f, \"bytes_per_step\": %.0f}", keys[t],
           (s1[t].cpu - s0[t].cpu) / k / 1e3, (s1[t].allocs - s0[t].allocs) / k, (s1[t].bytes - s0[t].bytes) / k);
  printf(", \"ens_io_allocs_register_per_step\": %.1f, \"ens_io_allocs_heartbeat_per_step\": %.1f"
         ", \"ens_io_allocs_delete_per_batch\": %.1f",
         ens_reg_allocs / k, ens_hb_allocs / k, ens_del_allocs / static_cast<double>(del_rounds));
  printf(", \"tree_locks_per_step\": %.1f, \"tree_locks_register_per_step\": %.1f", locks_step, locks_register);
  printf(", \"requests\": {\"create\": %llu, \"delete\": %llu, \"exists\": %llu}}\n",
         static_cast<unsigned long long>(counters["create"]), static_cast<unsigned long long>(counters["delete"]),
         static_cast<unsigned long long>(counters["exists"]));
#ifdef HOTPATH_PROF
  prof_report();
#endif
  return 0;
}
