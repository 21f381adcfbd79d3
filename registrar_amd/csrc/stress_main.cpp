// stress_main.cpp — native concurrency stress driver for sanitizer builds.
//
// The reference is single-threaded JS and needed no sanitizers; this build's
// core is heavily multi-threaded (IO-loop pool, sharded state, cross-thread
// watch delivery), so TSan/ASan passes run this driver in CI
// (make tsan / make asan):
//   - an in-process 3-server ensemble,
//   - N concurrent registrar clients doing register → heartbeat → unregister
//     cycles with watches armed,
//   - a chaos thread expiring random sessions and kill/restarting servers,
//   - then a contested phase: PAIRS of clients register the same domain, host
//     and aliases, so each cleans up and recreates the other's znodes (one of
//     a pair by atomic swap, one by cleanup + create) while the chaos thread
//     goes on expiring sessions. A register or heartbeat that loses to its
//     peer there is expected and not counted,
//   - then a crossed-parents phase on a two-loop ensemble of its own (see
//     crossed_phase): the locks a drain carries, under contention,
//   - then the tree's lock type on its own (see treelock_phase): eight
//     threads, one TreeLock, one plain counter,
//   - then a quorum phase on a 3-server quorum-mode ensemble of its own (see
//     quorum_phase): registered clients heartbeat while the chaos thread
//     crosses the majority boundary in both directions,
//   - then a resolver phase on a 3-server ensemble of its own (see
//     resolver_phase): one Resolver keeps a view of a domain that several
//     sessions register and unregister under, while servers die and return
//     and the resolver's own session is expired.
// At the end, with every client closed and every session gone, the tree must
// pass Ensemble::audit() and hold no ephemeral.
// Exit code 0 = every cycle behaved and the end state is sound; sanitizers
// report races/leaks.
#include <dirent.h>
#include <execinfo.h>
#include <signal.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "ensemble.hpp"
#include "node_store.hpp"
#include "registrar.hpp"
#include "resolver.hpp"
#include "zkclient.hpp"

using namespace registrar;

namespace {
// Hang diagnosis: STRESS_WATCHDOG=<sec> arms a watchdog that, if the run
// overshoots, SIGUSR1s every thread (whose handler prints a backtrace) and
// aborts. Diagnostic aid; off by default.
void dump_backtrace(int) {
  void* frames[48];
  int n = backtrace(frames, 48);
  char hdr[64];
  int len = snprintf(hdr, sizeof(hdr), "--- thread %ld backtrace ---\n", syscall(SYS_gettid));
  ssize_t r = write(2, hdr, len);
  (void)r;
  backtrace_symbols_fd(frames, n, 2);
}

void arm_watchdog(int seconds) {
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_handler = dump_backtrace;
  sigaction(SIGUSR1, &sa, nullptr);
  std::thread([seconds] {
    std::this_thread::sleep_for(std::chrono::seconds(seconds));
    fprintf(stderr, "WATCHDOG: run overshot %ds; dumping all threads\n", seconds);
    DIR* d = opendir("/proc/self/task");
    if (d) {
      while (struct dirent* e = readdir(d)) {
        if (e->d_name[0] == '.') continue;
        long tid = atol(e->d_name);
        syscall(SYS_tgkill, getpid(), tid, SIGUSR1);
        std::this_thread::sleep_for(std::chrono::milliseconds(150));
      }
      closedir(d);
    }
    std::this_thread::sleep_for(std::chrono::seconds(1));
    _exit(42);
  }).detach();
}
// Crossed-parents phase, on an ensemble of its own with two IO loops. Two
// sessions, one per loop, pipeline batches of ephemeral creates and deletes
// that alternate between their own parent and the other session's, so each
// drain carries one parent's shard lock and the session's eph_mu while the
// other loop wants them. A third thread reads through the public API, sends
// exists through a client of its own and runs audit() all the while, and the
// second session is expired half way. Returns true when every thread came back
// and what is left is exactly the surviving session's last batch.
bool crossed_phase(int seconds, const Logger& log) {
  zk::EnsembleConfig ecfg;
  ecfg.ports = {0};
  ecfg.io_threads = 2;
  ecfg.tick_ms = 50;
  ecfg.log_level = LogLevel::Error;
  zk::Ensemble ens(ecfg);
  ens.start();
  int port = ens.ports()[0];
  auto make_client = [&] {
    zk::ZkClientConfig ccfg;
    ccfg.servers.push_back({"127.0.0.1", port});
    ccfg.session_timeout_ms = 30000;
    ccfg.log_level = LogLevel::Fatal;
    auto c = std::make_unique<zk::ZkClient>(std::move(ccfg), log);
    c->start();
    return c;
  };
  // connections go to the loops round-robin: 0 and 1 land on different loops
  std::unique_ptr<zk::ZkClient> cl[2] = {make_client(), nullptr};
  if (!cl[0]->wait_connected(5000)) return false;
  cl[1] = make_client();
  if (!cl[1]->wait_connected(5000)) return false;
  auto reader = make_client();
  if (!reader->wait_connected(5000)) return false;
  const std::string parent[2] = {"/x/p0", "/x/p1"};
  if (cl[0]->mkdirp(parent[0]) != zk::kZOk || cl[0]->mkdirp(parent[1]) != zk::kZOk) return false;

  constexpr int kBatch = 96;  // three carries' worth per parent switch pattern
  auto batch_of = [&](int who) {
    std::vector<std::string> paths;
    for (int j = 0; j < kBatch; j++) {
      // runs of 8 under one parent, then 8 under the other
      int under = ((j / 8) % 2 == 0) ? who : 1 - who;
      paths.push_back(parent[under] + "/s" + std::to_string(who) + "_" + std::to_string(j));
    }
    return paths;
  };
  std::atomic<bool> stop{false};
  std::atomic<uint64_t> rounds[2] = {{0}, {0}};
  std::atomic<int> bad{0};
  auto worker = [&](int who) {
    std::vector<std::string> paths = batch_of(who);
    std::vector<std::string> datas(paths.size(), "crossed");
    while (!stop.load() && cl[who]->state() == zk::SessionState::Connected) {
      std::vector<int> rcs = cl[who]->create_many(paths, datas, zk::kEphemeral);
      bool lost = false;
      for (int rc : rcs) {
        if (rc == zk::kZConnectionLoss || rc == zk::kZSessionExpired)
          lost = true;
        else if (rc != zk::kZOk)
          bad.fetch_add(1);
      }
      if (lost) break;
      rcs = cl[who]->delete_many(paths);
      for (int rc : rcs) {
        if (rc == zk::kZConnectionLoss || rc == zk::kZSessionExpired)
          lost = true;
        else if (rc == zk::kZNoNode && who == 1)
          lost = true;  // the expiry's drain got to the node first
        else if (rc != zk::kZOk)
          bad.fetch_add(1);
      }
      if (lost) break;
      rounds[who].fetch_add(1);
    }
  };
  auto observer = [&] {
    while (!stop.load()) {
      for (int p = 0; p < 2; p++) {
        reader->exists(parent[p]);
        reader->exists(parent[p] + "/s" + std::to_string(p) + "_0");
        ens.get(parent[p]);
      }
      ens.audit();  // mid-expiry findings are expected; it must only return
    }
  };
  std::thread t0(worker, 0), t1(worker, 1), t2(observer);
  std::this_thread::sleep_for(std::chrono::milliseconds(seconds * 500));
  ens.expire_session(cl[1]->session_id());
  std::this_thread::sleep_for(std::chrono::milliseconds(seconds * 500));
  stop.store(true);
  t0.join();
  t1.join();
  t2.join();

  // the survivor leaves one last batch behind
  std::vector<std::string> last = batch_of(0);
  std::vector<int> rcs = cl[0]->create_many(last, std::vector<std::string>(last.size(), "last"), zk::kEphemeral);
  bool ok = true;
  for (int rc : rcs) ok = ok && rc == zk::kZOk;
  size_t want[2] = {0, 0};
  for (int j = 0; j < kBatch; j++) want[((j / 8) % 2 == 0) ? 0 : 1]++;
  std::vector<std::string> violations = ens.audit();
  size_t have0 = ens.children(parent[0]).size(), have1 = ens.children(parent[1]).size();
  size_t eph = ens.ephemeral_count();
  printf("stress: crossed phase: %llu + %llu rounds, %d unexpected rcs, %zu + %zu survivors, %zu ephemerals\n",
         static_cast<unsigned long long>(rounds[0].load()), static_cast<unsigned long long>(rounds[1].load()),
         bad.load(), have0, have1, eph);
  for (const auto& v : violations) printf("stress: crossed phase: audit: %s\n", v.c_str());
  ok = ok && violations.empty() && bad.load() == 0 && rounds[0].load() > 0 && have0 == want[0] &&
       have1 == want[1] && eph == static_cast<size_t>(kBatch);
  reader->close();
  cl[0]->close();
  cl[1]->close();
  ens.stop();
  return ok;
}

// TreeLock on its own: eight threads add to a PLAIN counter under one lock,
// so a lost update (or, under the thread sanitizer, a missing acquire/release
// edge) shows. Most sections are a bare increment, which keeps the word
// contended and the spin path busy; every 512th holds the lock across a short
// sleep, so the others run out of spins, mark sleepers and wait in the kernel
// until the unlock wakes them. try_lock takes part too. Returns true when the
// count is exact.
bool treelock_phase() {
  constexpr int kThreads = 8;
  constexpr uint64_t kPerThread = 20000;
  zk::detail::TreeLock mu;
  uint64_t counter = 0;  // guarded by mu, deliberately not atomic
  std::atomic<uint64_t> tried{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; t++) {
    threads.emplace_back([&, t] {
      for (uint64_t i = 0; i < kPerThread; i++) {
        if ((i + static_cast<uint64_t>(t)) % 7 == 0) {
          // the handlers' own pattern: try first, block only when taken
          if (mu.try_lock())
            tried.fetch_add(1, std::memory_order_relaxed);
          else
            mu.lock();
          counter++;
          mu.unlock();
        } else {
          std::lock_guard<zk::detail::TreeLock> g(mu);
          counter++;
          if (i % 512 == static_cast<uint64_t>(t)) std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
      }
    });
  }
  for (auto& th : threads) th.join();
  bool held = !mu.try_lock();  // must be free at the end
  if (!held) mu.unlock();
  printf("stress: tree lock phase: count %llu of %llu, %llu by try_lock\n", static_cast<unsigned long long>(counter),
         static_cast<unsigned long long>(kThreads * kPerThread), static_cast<unsigned long long>(tried.load()));
  return !held && counter == kThreads * kPerThread;
}

// Quorum phase, on a 3-server quorum-mode ensemble of its own. Each client
// registers once and then heartbeats, re-registering only if its session was
// lost. The chaos thread meanwhile loses the majority and regains it, kills
// the leader during the election pause that follows, kills the leader with
// the majority intact, and does a rolling restart, over and over. Whenever
// the ensemble is below a majority the chaos thread also checks that zxid
// stands still. At the end, with every server back, the ensemble serving and
// every client connected (so no expiry is in flight), audit() must be empty
// and every client's znodes present. Returns true when all of that held.
bool quorum_phase(int nclients, int seconds, const Logger& log) {
  zk::EnsembleConfig ecfg;
  ecfg.ports = {0, 0, 0};
  ecfg.tick_ms = 50;
  ecfg.min_session_timeout_ms = 300;
  ecfg.election_ms = 100;
  ecfg.quorum = true;
  ecfg.log_level = LogLevel::Error;
  zk::Ensemble ens(ecfg);
  ens.start();
  std::vector<int> ports = ens.ports();

  std::atomic<bool> stop{false};
  std::atomic<uint64_t> heartbeats{0}, registers{0}, bad{0};
  std::atomic<int> settled_count{0};
  std::atomic<bool> release{false};
  std::vector<std::vector<std::string>> held(static_cast<size_t>(nclients));
  std::vector<int> settled(static_cast<size_t>(nclients), 0);

  auto client_fn = [&](int idx) {
    RegistrationConfig reg;
    reg.domain = "q" + std::to_string(idx) + ".quorum.stress.test";
    reg.type = "host";
    reg.admin_ip = "127.0.0.1";
    reg.hostname = "h" + std::to_string(idx);
    reg.settle_ms = 0;
    for (int a = 0; a < 20; a++) reg.aliases.push_back("a" + std::to_string(a) + "." + reg.domain);
    zk::RetryPolicy rp;
    rp.max_attempts = 1;
    rp.initial_delay_ms = 10;

    std::unique_ptr<zk::ZkClient> client;
    std::vector<std::string> znodes;
    // one step towards "connected, registered, heartbeat answered"
    auto step = [&]() -> bool {
      if (!client || client->state() == zk::SessionState::Expired || client->state() == zk::SessionState::Closed) {
        if (client) client->close();
        znodes.clear();
        zk::ZkClientConfig ccfg;
        for (int p : ports) ccfg.servers.push_back({"127.0.0.1", p});
        ccfg.session_timeout_ms = 4000;
        ccfg.connect_timeout_ms = 1000;
        ccfg.connect_initial_delay_ms = 20;
        ccfg.connect_max_delay_ms = 100;
        ccfg.log_level = LogLevel::Fatal;
        client = std::make_unique<zk::ZkClient>(std::move(ccfg), log);
        client->start();
      }
      if (!client->wait_connected(200)) return false;
      if (znodes.empty()) {
        RegisterResult res = register_node(*client, reg, log);
        if (res.rc != zk::kZOk) return false;  // the ensemble went away mid-register
        znodes = res.znodes();
        registers.fetch_add(1);
      }
      int rc = client->heartbeat(znodes, rp, nullptr);
      if (rc == zk::kZOk) {
        heartbeats.fetch_add(1);
        return true;
      }
      if (rc == zk::kZNoNode)
        znodes.clear();  // the session was lost and its znodes with it: register again
      else if (rc != zk::kZConnectionLoss && rc != zk::kZSessionExpired)
        bad.fetch_add(1);
      return false;
    };
    while (!stop.load()) {
      step();
      std::this_thread::sleep_for(std::chrono::milliseconds(10));
    }
    // the chaos thread has restored every server by now: settle
    auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(20);
    bool ok = false;
    while (!(ok = step()) && std::chrono::steady_clock::now() < deadline)
      std::this_thread::sleep_for(std::chrono::milliseconds(10));
    held[static_cast<size_t>(idx)] = znodes;
    settled[static_cast<size_t>(idx)] = ok ? 1 : 0;
    settled_count.fetch_add(1);  // publishes the two writes above
    // stay connected until the end state has been checked
    while (!release.load()) std::this_thread::sleep_for(std::chrono::milliseconds(10));
    if (client) client->close();
  };

  std::atomic<uint64_t> crossings{0};
  auto nap = [](int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); };
  auto restore = [&] {
    for (size_t i = 0; i < 3; i++)
      if (!ens.server_up(i)) ens.restart_server(i);
  };
  auto lost = [&] {
    if (!ens.has_quorum()) crossings.fetch_add(1);
  };
  // below a majority nothing may commit
  auto frozen = [&](int ms) {
    int64_t z = ens.zxid();
    nap(ms);
    if (!ens.has_quorum() && ens.zxid() != z) bad.fetch_add(1);
  };
  auto chaos_fn = [&] {
    while (!stop.load()) {
      nap(250);
      // lose the majority, hold, regain it
      ens.kill_server(2);
      ens.kill_server(1);
      lost();
      frozen(200);
      ens.restart_server(1);
      // ... and kill the leader during the election pause: if the last
      // leader is the server still up, this loses the majority again
      ens.kill_leader();
      lost();
      frozen(100);
      restore();
      nap(300);
      // leader loss with the majority intact, then a second server lost
      // during the pause: below a majority with an election pending
      ens.kill_leader();
      for (size_t i = 0; i < 3; i++) {
        if (ens.server_up(i)) {
          ens.kill_server(i);
          break;
        }
      }
      lost();
      frozen(150);
      restore();
      nap(200);
      // rolling restart: never below a majority
      for (size_t i = 0; i < 3 && !stop.load(); i++) {
        ens.kill_server(i);
        nap(150);
        ens.restart_server(i);
        nap(150);
      }
    }
    restore();
  };

  std::vector<std::thread> threads;
  for (int i = 0; i < nclients; i++) threads.emplace_back(client_fn, i);
  std::thread chaos(chaos_fn);
  std::this_thread::sleep_for(std::chrono::seconds(seconds));
  stop.store(true);
  chaos.join();
  // every server is back; wait for the election to end and for every client
  // to have had a heartbeat answered on a registered session
  auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(30);
  while ((!ens.quorum_state().serving || settled_count.load() < nclients) &&
         std::chrono::steady_clock::now() < deadline)
    nap(10);
  zk::QuorumState qs = ens.quorum_state();
  bool all_settled = settled_count.load() == nclients;
  size_t total = 0, missing = 0;
  if (all_settled) {
    for (int i = 0; i < nclients; i++) {
      if (!settled[static_cast<size_t>(i)]) all_settled = false;
      for (const auto& z : held[static_cast<size_t>(i)]) {
        total++;
        if (!ens.get(z).exists) missing++;
      }
    }
  }
  // every session is connected and heartbeating: no expiry is in flight
  std::vector<std::string> violations = ens.audit();
  size_t eph = ens.ephemeral_count();
  release.store(true);
  for (auto& t : threads) t.join();
  ens.stop();

  printf("stress: quorum phase: %llu heartbeats, %llu registers by %d clients, %llu majority losses seen, "
         "%llu counted, %llu refused connects, %llu dropped connections, %llu unexpected, %zu of %zu znodes missing, "
         "%zu ephemerals\n",
         static_cast<unsigned long long>(heartbeats.load()), static_cast<unsigned long long>(registers.load()),
         nclients, static_cast<unsigned long long>(crossings.load()), static_cast<unsigned long long>(qs.losses),
         static_cast<unsigned long long>(qs.refused_connects), static_cast<unsigned long long>(qs.dropped_connections),
         static_cast<unsigned long long>(bad.load()), missing, total, eph);
  for (const auto& v : violations) printf("stress: quorum phase: audit: %s\n", v.c_str());
  if (!all_settled) printf("stress: quorum phase: not every client got back to a registered, answered heartbeat\n");
  return qs.serving && qs.has_quorum && all_settled && violations.empty() && bad.load() == 0 && missing == 0 &&
         total == static_cast<size_t>(nclients) * 21 && eph == total && qs.losses == crossings.load() &&
         crossings.load() > 0 && heartbeats.load() > 0;
}

// Resolver phase, on a 3-server ensemble of its own. `nclients` sessions create,
// rewrite and delete ephemeral host records under one domain (neighbouring
// sessions share some names), a chaos thread kills and restarts servers,
// always leaving one up, the resolver's own session is expired once half way,
// and a reader thread takes snapshots all the while: generation must never
// fall, hosts must be sorted and unique (local ones first when asked so), and
// no host may have an empty payload. At the end, with the writers quiet, their
// sessions still open and every server back, the view must equal the tree,
// name for name and byte for byte, and audit() must be empty.
bool resolver_phase(int nclients, int seconds, const Logger& log) {
  zk::EnsembleConfig ecfg;
  ecfg.ports = {0, 0, 0};
  ecfg.tick_ms = 50;
  ecfg.min_session_timeout_ms = 300;
  ecfg.log_level = LogLevel::Error;
  zk::Ensemble ens(ecfg);
  ens.start();
  std::vector<int> ports = ens.ports();
  auto client_cfg = [&] {
    zk::ZkClientConfig ccfg;
    for (int p : ports) ccfg.servers.push_back({"127.0.0.1", p});
    ccfg.session_timeout_ms = 4000;
    ccfg.connect_timeout_ms = 1000;
    ccfg.connect_initial_delay_ms = 20;
    ccfg.connect_max_delay_ms = 100;
    ccfg.log_level = LogLevel::Fatal;
    return ccfg;
  };
  const std::string domain = "res.stress.test";
  const std::string path = domain_to_path(domain);
  {
    zk::ZkClient setup(client_cfg(), log);
    setup.start();
    if (!setup.wait_connected(5000) || setup.mkdirp(path) != zk::kZOk) return false;
    setup.put(path, R"({"type":"service","service":{"type":"service","service":{"srvce":"_s","proto":"_tcp","port":80}}})");
    setup.close();
  }

  ResolverConfig rcfg;
  rcfg.client = client_cfg();
  rcfg.local_address = "10.0.0.1";
  Resolver resolver(rcfg, log);
  resolver.start();
  ResolverSnapshot first;
  if (resolver.lookup(domain, 10000, &first) != LookupStatus::Ok) return false;

  std::atomic<bool> stop{false};
  std::atomic<uint64_t> writes{0}, snapshots{0}, bad{0};
  std::vector<std::unique_ptr<zk::ZkClient>> held(static_cast<size_t>(nclients));
  auto writer_fn = [&](int idx) {
    uint64_t rng = 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(idx + 1);
    auto next = [&rng] {
      rng ^= rng << 13;
      rng ^= rng >> 7;
      rng ^= rng << 17;
      return rng;
    };
    std::unique_ptr<zk::ZkClient>& client = held[static_cast<size_t>(idx)];
    while (!stop.load()) {
      if (!client || client->state() == zk::SessionState::Expired || client->state() == zk::SessionState::Closed) {
        if (client) client->close();
        client = std::make_unique<zk::ZkClient>(client_cfg(), log);
        client->start();
      }
      if (!client->wait_connected(200)) continue;
      // six names per writer, two of them shared with the next writer
      int slot = (idx * 4 + static_cast<int>(next() % 6)) % (nclients * 4);
      std::string node = path + "/h" + std::to_string(slot);
      std::string rec = "{\"type\":\"host\",\"address\":\"10.0.0." + std::to_string(next() % 4) +
                        "\",\"host\":{\"seq\":" + std::to_string(next() % 1000000) + "}}";
      switch (next() % 3) {
        case 0:
          client->create(node, rec, zk::kEphemeral);
          break;
        case 1:
          client->set(node, rec, -1);
          break;
        default:
          client->del(node, -1);
          break;
      }
      writes.fetch_add(1);
      std::this_thread::sleep_for(std::chrono::microseconds(200 + next() % 800));
    }
  };
  auto reader_fn = [&] {
    uint64_t last = 0;
    bool local_first = false;
    while (!stop.load()) {
      ResolverSnapshot s = resolver.snapshot(domain, local_first);
      if (!s.exists || !s.synced || s.generation < last) bad.fetch_add(1);
      last = s.generation;
      for (size_t i = 0; i < s.hosts.size(); i++) {
        const ResolvedHost& h = s.hosts[i];
        if (h.payload.empty() || !h.has_address || h.ports != std::vector<int64_t>{80}) bad.fetch_add(1);
        if (h.local != (h.address == "10.0.0.1")) bad.fetch_add(1);
        if (i == 0) continue;
        const ResolvedHost& p = s.hosts[i - 1];
        bool ordered = local_first ? (p.local != h.local ? p.local : p.name < h.name) : p.name < h.name;
        if (!ordered) bad.fetch_add(1);
      }
      resolver.poll_events();  // an observer that keeps up
      local_first = !local_first;
      snapshots.fetch_add(1);
      std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
  };
  auto chaos_fn = [&] {
    size_t victim = 0;
    while (!stop.load()) {
      std::this_thread::sleep_for(std::chrono::milliseconds(200));
      ens.kill_server(victim);
      std::this_thread::sleep_for(std::chrono::milliseconds(150));
      ens.restart_server(victim);
      victim = (victim + 1) % 3;
    }
    for (size_t i = 0; i < 3; i++)
      if (!ens.server_up(i)) ens.restart_server(i);
  };

  std::vector<std::thread> threads;
  for (int i = 0; i < nclients; i++) threads.emplace_back(writer_fn, i);
  std::thread reader(reader_fn), chaos(chaos_fn);
  std::this_thread::sleep_for(std::chrono::milliseconds(seconds * 500));
  int64_t old_session = resolver.session_id();
  ens.expire_session(old_session);
  std::this_thread::sleep_for(std::chrono::milliseconds(seconds * 500));
  stop.store(true);
  for (auto& t : threads) t.join();
  reader.join();
  chaos.join();

  // everything is quiet: the writers' sessions are still open, so the tree
  // holds whatever they created last. The view has to get there by itself.
  auto matches = [&] {
    ResolverSnapshot s = resolver.snapshot(domain);
    std::vector<std::string> names = ens.children(path);
    std::sort(names.begin(), names.end());
    if (s.stale || !s.synced || s.hosts.size() != names.size()) return false;
    for (size_t i = 0; i < names.size(); i++)
      if (s.hosts[i].name != names[i] || s.hosts[i].payload != ens.get(path + "/" + names[i]).data) return false;
    return true;
  };
  auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(20);
  bool equal = false;
  while (!(equal = matches()) && std::chrono::steady_clock::now() < deadline)
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  ResolverStats rs = resolver.stats();
  ResolverSnapshot last = resolver.snapshot(domain);
  bool new_session = resolver.session_id() != old_session && resolver.session_id() != 0;
  // a writer that replaced an expired session shortly before the end may
  // still have that session's drain in flight; a real violation stays
  std::vector<std::string> violations = ens.audit();
  deadline = std::chrono::steady_clock::now() + std::chrono::seconds(2);
  while (!violations.empty() && std::chrono::steady_clock::now() < deadline) {
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    violations = ens.audit();
  }
  resolver.stop();
  for (auto& c : held)
    if (c) c->close();
  ens.stop();

  printf("stress: resolver phase: %llu writes by %d sessions, %llu snapshots, %llu passes, %llu changes applied, "
         "%llu resyncs after expiry, %zu hosts at generation %llu, %llu unexpected\n",
         static_cast<unsigned long long>(writes.load()), nclients, static_cast<unsigned long long>(snapshots.load()),
         static_cast<unsigned long long>(rs.passes), static_cast<unsigned long long>(rs.events_applied),
         static_cast<unsigned long long>(rs.resyncs_after_expiry), last.hosts.size(),
         static_cast<unsigned long long>(last.generation), static_cast<unsigned long long>(bad.load()));
  for (const auto& v : violations) printf("stress: resolver phase: audit: %s\n", v.c_str());
  if (!equal) printf("stress: resolver phase: the view did not converge to the tree\n");
  if (!new_session) printf("stress: resolver phase: the resolver did not get a new session after its expiry\n");
  return equal && new_session && violations.empty() && bad.load() == 0 && rs.resyncs_after_expiry >= 1 &&
         rs.events_applied > 0 && writes.load() > 0 && snapshots.load() > 0;
}
}  // namespace

int main(int argc, char** argv) {
  signal(SIGPIPE, SIG_IGN);  // belt: library writes already use MSG_NOSIGNAL
  int nclients = 4;
  int seconds = 8;
  int contested_seconds = -1;  // default: half of -t
  if (const char* wd = getenv("STRESS_WATCHDOG")) arm_watchdog(atoi(wd));
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "-c") && i + 1 < argc) nclients = atoi(argv[++i]);
    if (!strcmp(argv[i], "-t") && i + 1 < argc) seconds = atoi(argv[++i]);
    if (!strcmp(argv[i], "-p") && i + 1 < argc) contested_seconds = atoi(argv[++i]);
  }
  if (contested_seconds < 0) contested_seconds = seconds / 2;
  int crossed_secs = seconds > 0 ? std::max(2, seconds / 4) : 0;

  Logger log("stress");
  log.set_level(LogLevel::Error);

  zk::EnsembleConfig ecfg;
  ecfg.ports = {0, 0, 0};
  ecfg.tick_ms = 50;
  ecfg.min_session_timeout_ms = 300;
  ecfg.log_level = LogLevel::Error;
  zk::Ensemble ens(ecfg);
  ens.start();

  std::vector<std::pair<std::string, int>> servers;
  for (int p : ens.ports()) servers.push_back({"127.0.0.1", p});

  std::atomic<bool> stop{false};
  std::atomic<uint64_t> cycles{0};
  std::atomic<uint64_t> failures{0};
  std::atomic<uint64_t> contested_cycles{0};

  // contested: clients 2k and 2k+1 share one registration (see the header)
  auto client_fn = [&](int idx, bool contested) {
    int who = contested ? idx / 2 : idx;
    std::string tag = std::string(contested ? "p" : "c") + std::to_string(who);
    while (!stop.load()) {
      zk::ZkClientConfig ccfg;
      for (auto& s : servers) ccfg.servers.push_back({s.first, s.second});
      ccfg.session_timeout_ms = 2000;
      ccfg.connect_timeout_ms = 1000;
      ccfg.connect_initial_delay_ms = 20;
      ccfg.connect_max_delay_ms = 100;
      ccfg.log_level = LogLevel::Fatal;
      zk::ZkClient client(std::move(ccfg), log);
      client.start();
      if (!client.wait_connected(5000)) continue;

      RegistrationConfig reg;
      reg.domain = tag + ".stress.test";
      reg.type = "host";
      reg.admin_ip = "127.0.0.1";
      reg.hostname = "h" + std::to_string(who);
      reg.settle_ms = 0;
      reg.atomic_swap = contested && idx % 2 == 0;
      for (int a = 0; a < 20; a++) reg.aliases.push_back("a" + std::to_string(a) + "." + tag + ".stress.test");

      while (!stop.load() && client.state() == zk::SessionState::Connected) {
        RegisterResult res = register_node(client, reg, log);
        if (res.rc != zk::kZOk) {
          if (!contested) failures.fetch_add(1);
          break;
        }
        // arm some watches like a Binder reader would
        client.exists(res.znodes()[0], nullptr, true);
        std::vector<std::string> ch;
        client.get_children(domain_to_path(reg.domain), &ch, true);
        // exercise multi under chaos too: atomic delete+create of one node
        {
          std::vector<zk::ZkClient::MixedOp> mops;
          zk::ZkClient::MixedOp d;
          d.op = zk::kOpDelete;
          d.path = res.znodes()[0];
          mops.push_back(d);
          zk::ZkClient::MixedOp cr;
          cr.op = zk::kOpCreate;
          cr.path = res.znodes()[0];
          cr.data = "swap";
          cr.flags = zk::kEphemeral;
          mops.push_back(cr);
          client.multi(mops, nullptr);  // rc may be conn-loss under chaos
        }
        // setData past the node block's inline capacity and back (the node
        // stays put; its data moves out of line and in again)
        client.set(res.znodes()[0], std::string(6000, 'g'), -1, nullptr);
        client.set(res.znodes()[0], "small", -1, nullptr);
        zk::RetryPolicy rp;
        rp.max_attempts = 1;
        rp.initial_delay_ms = 10;
        int rc = client.heartbeat(res.znodes(), rp, nullptr);
        // contested: the peer may have replaced or removed any of the nodes
        if (!contested && rc != zk::kZOk && rc != zk::kZConnectionLoss && rc != zk::kZSessionExpired)
          failures.fetch_add(1);
        unregister_node(client, res.znodes(), log);
        (contested ? contested_cycles : cycles).fetch_add(1);
      }
      client.close();
    }
  };

  auto chaos_fn = [&] {
    uint64_t rng = 0x12345678;
    auto next = [&rng] {
      rng ^= rng << 13;
      rng ^= rng >> 7;
      rng ^= rng << 17;
      return rng;
    };
    while (!stop.load()) {
      std::this_thread::sleep_for(std::chrono::milliseconds(150 + next() % 250));
      switch (next() % 4) {
        case 0: {
          auto sids = ens.session_ids();
          if (!sids.empty()) ens.expire_session(sids[next() % sids.size()]);
          break;
        }
        case 1: {
          size_t idx = next() % 3;
          if (ens.server_up(idx)) {
            // keep at least one server up
            int up = 0;
            for (size_t i = 0; i < 3; i++) up += ens.server_up(i) ? 1 : 0;
            if (up > 1) ens.kill_server(idx);
          }
          break;
        }
        case 2: {
          for (size_t i = 0; i < 3; i++)
            if (!ens.server_up(i)) ens.restart_server(i);
          break;
        }
        default:
          ens.set_latency_ms(static_cast<int>(next() % 3));
          break;
      }
    }
    ens.set_latency_ms(0);
    for (size_t i = 0; i < 3; i++)
      if (!ens.server_up(i)) ens.restart_server(i);
  };

  for (int phase = 0; phase < 2; phase++) {
    bool contested = phase == 1;
    int secs = contested ? contested_seconds : seconds;
    if (secs <= 0) continue;
    stop.store(false);
    std::vector<std::thread> threads;
    for (int i = 0; i < nclients; i++) threads.emplace_back(client_fn, i, contested);
    std::thread chaos(chaos_fn);
    std::this_thread::sleep_for(std::chrono::seconds(secs));
    stop.store(true);
    for (auto& t : threads) t.join();
    chaos.join();
  }

  // crossed parents (carried locks under contention), on its own ensemble
  bool crossed_ok = crossed_secs <= 0 || crossed_phase(crossed_secs, log);
  bool treelock_ok = treelock_phase();
  bool quorum_ok = seconds <= 0 || quorum_phase(nclients, std::max(3, seconds / 2), log);
  bool resolver_ok = seconds <= 0 || resolver_phase(nclients, std::max(3, seconds / 2), log);

  // End state. Every client is closed, so every session ends: by its close,
  // or (where the close was lost to a killed server) by the expiry sweep. A
  // close is acknowledged before the ensemble has drained the session's
  // ephemerals, and the audit is only meaningful with no drain in flight, so
  // wait for the sessions to go and give the last drain a moment to finish.
  // A real violation does not go away by waiting.
  auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(15);
  while (!ens.session_ids().empty() && std::chrono::steady_clock::now() < deadline)
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  size_t sessions_left = ens.session_ids().size();
  std::vector<std::string> violations = ens.audit();
  deadline = std::chrono::steady_clock::now() + std::chrono::seconds(2);
  while (!violations.empty() && std::chrono::steady_clock::now() < deadline) {
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    violations = ens.audit();
  }
  size_t ephemerals_left = ens.ephemeral_count();
  ens.stop();

  printf("stress: %llu cycles, %llu hard failures, %llu contested cycles\n",
         static_cast<unsigned long long>(cycles.load()), static_cast<unsigned long long>(failures.load()),
         static_cast<unsigned long long>(contested_cycles.load()));
  bool sound = true;
  if (sessions_left != 0) {
    printf("stress: %zu sessions still alive after every client closed\n", sessions_left);
    sound = false;
  }
  if (ephemerals_left != 0) {
    printf("stress: %zu ephemerals left\n", ephemerals_left);
    sound = false;
  }
  for (const auto& v : violations) {
    printf("stress: audit: %s\n", v.c_str());
    sound = false;
  }
  if (contested_seconds > 0 && contested_cycles.load() == 0) {
    printf("stress: the contested phase completed no cycle\n");
    sound = false;
  }
  // hard failures are register errors while connected — tolerate a few from
  // chaos timing, fail on systematic breakage
  bool behaved = cycles.load() > 0 && failures.load() < cycles.load() / 4 + 16;
  if (!crossed_ok) printf("stress: the crossed-parents phase failed\n");
  if (!treelock_ok) printf("stress: the tree lock phase failed\n");
  if (!quorum_ok) printf("stress: the quorum phase failed\n");
  if (!resolver_ok) printf("stress: the resolver phase failed\n");
  return (behaved && sound && crossed_ok && treelock_ok && quorum_ok && resolver_ok) ? 0 : 1;
}
