// ensemble.cpp — synthetic in-process ZooKeeper ensemble (see ensemble.hpp).
//
// Threading model (the scaling core of the whole framework): an IO-loop
// thread POOL (connections assigned round-robin, independent of which
// server socket accepted them — like ZooKeeper's selector threads) for
// parallel socket I/O, and SHARDED state so concurrent registrar processes
// (which write disjoint domain subtrees) never contend:
//
//   - znodes + their watch maps live in 64 hash shards, each under its own
//     lock (a TreeLock, node_store.hpp); an op locks only the shard(s) of the
//     paths it touches (create/delete lock child+parent shards in index
//     order),
//   - sessions live under one session mutex, but per-request touch is a
//     lock-free atomic store through the connection's cached session pointer,
//   - zxid is a global atomic counter,
//   - per-connection output buffers have their own mutex; replies queue per
//     event drain and flush as a few large writes.
//
// Global lock order: shard(s) by ascending index → one session's eph_mu →
// session_mu → conns_mu → conn->out_mu. A thread blocks on a mutex only while
// everything it holds comes earlier in that order; a drain that carries its
// parent shard and eph_mu across sibling requests takes child shards with
// try_lock (struct Carry). kill_session drains the ephemeral set with no
// other lock held before taking shard locks (see the phase comments).
//
// admin_mu (servers, leader, election, quorum state) stands outside that
// chain: a thread takes it while holding none of the locks above. Under it a
// thread may take session_mu (resume_serving restarts every session's timer),
// and nothing else. Order: admin_mu → session_mu.
//
// Quorum mode (EnsembleConfig::quorum). The ensemble has quorum while more
// than half of its servers are up; it serves while it has quorum, a leader,
// and no election pause. Service is withheld at the door only, never per
// request: `not_serving` (one atomic, written under admin_mu) is read by
// accept, by the handshake and by the expiry sweep, and the call that stops
// service closes every connection before it returns (kill_server: a barrier
// through every IO loop, so that no accept, drain or sweep that began while
// serving is still running, then a close of each connection on its own loop).
// From then on no request handler runs, so the tree and zxid stand still
// until resume_serving, which elects the lowest up index, sets every live
// session's last_touch to now and only then clears `not_serving`. With the
// mode off `not_serving` is never set and none of this runs.
#include "ensemble.hpp"

#include "node_store.hpp"

#include <arpa/inet.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <future>

namespace registrar {
namespace zk {

// paths, ZNode, NodeStore, Session and the link helpers (node_store.hpp)
using namespace detail;

namespace {

void set_nonblock(int fd) {
  int fl = fcntl(fd, F_GETFL, 0);
  fcntl(fd, F_SETFL, fl | O_NONBLOCK);
}

void set_nodelay(int fd) {
  int one = 1;
  setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
}

inline void spin_pause() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}

int64_t wall_ms() {
  struct timespec ts;
  clock_gettime(CLOCK_REALTIME, &ts);
  return static_cast<int64_t>(ts.tv_sec) * 1000 + ts.tv_nsec / 1000000;
}

// Write data[*off..len) to a non-blocking socket until it is all out, the
// socket would block, or it fails; *off moves past what was written.
enum class SendResult { kDone, kWouldBlock, kError };
SendResult send_some(int fd, const char* data, size_t len, size_t* off) {
  while (*off < len) {
    ssize_t n = send(fd, data + *off, len - *off, MSG_NOSIGNAL);
    if (n > 0)
      *off += static_cast<size_t>(n);
    else if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK))
      return SendResult::kWouldBlock;
    else if (!(n < 0 && errno == EINTR))
      return SendResult::kError;
  }
  return SendResult::kDone;
}

}  // namespace

struct Ensemble::Impl {
  static constexpr size_t kShards = 64;

  struct Carry;

  using SessionPtr = std::shared_ptr<Session>;
  using WatchMap = std::unordered_map<PathKey, std::set<int64_t>, PathHash, PathEq>;

  struct Shard {
    TreeLock mu;
    // threads waiting in lock_shard; a drain that carries mu reads it before
    // every request (acquire_for)
    std::atomic<uint32_t> waiters{0};
    NodeStore nodes;
    WatchMap data_watches;
    WatchMap child_watches;
  };

  struct Conn {
    uint64_t id = 0;
    int fd = -1;
    size_t server_idx = 0;  // which server (port) accepted it — kill semantics
    size_t io_idx = 0;      // which IO loop owns its events
    // owner-loop-thread only:
    RecvBuf inbuf;
    bool handshaken = false;
    SessionPtr session;  // cached after handshake (lock-free touch)
    bool flush_scheduled = false;
    // per event drain (on_conn_event): both clocks are read once, and the
    // last parent path seen is remembered as (view into inbuf, hash) so a run
    // of siblings hashes its parent once. Only the path's hash is cached,
    // nothing about the tree.
    int64_t drain_mono_ms = 0;
    int64_t drain_wall_ms = 0;
    PathRef last_parent{std::string_view(), 0};
    Carry* carry = nullptr;  // the running drain's carried locks (process_frames)
    std::string scratch;  // variable-size replies are built here, then staged
    // replies produced during a drain are staged here without a lock and
    // move to outbuf once, at the flush that ends the drain
    ByteBuf stage;
    std::atomic<size_t> stage_pub{0};  // stage.size() after the last whole packet
    // shared output state (out_mu):
    std::mutex out_mu;
    ByteBuf outbuf;
    // true while the owner loop is inside a drain (written under out_mu by
    // the owner; the owner may read it without the lock)
    bool draining = false;
    // packets delivered by OTHER threads during a drain, each with the stage
    // position it arrived at, so the flush can interleave them exactly where
    // a locked append would have put them
    std::vector<std::pair<size_t, std::string>> xq;
    bool epollout_armed = false;
    bool closing = false;  // close once outbuf drains
    std::atomic<bool> dead{false};
  };
  using ConnPtr = std::shared_ptr<Conn>;

  struct Server {
    int listen_fd = -1;
    int port = 0;
    bool up = false;
  };

  // One counter block per IO loop, each on cache lines of its own, allocated
  // by start() once the pool's size is known. A block has exactly one writer,
  // its loop's thread, so an increment is a relaxed load and a relaxed store
  // (bump below), not an atomic read-modify-write; counters() sums the blocks
  // with relaxed loads from any thread and stays exact.
  // tree_locks: shard and eph_mu acquisitions made by request handlers.
  struct alignas(128) OpCounters {
    std::atomic<uint64_t> connect{0}, create{0}, del{0}, exists{0}, get_data{0}, set_data{0},
        get_children{0}, ping{0}, close_session{0}, unknown{0}, tree_locks{0};
  };
  static void bump(std::atomic<uint64_t>& a, uint64_t by = 1) {
    a.store(a.load(std::memory_order_relaxed) + by, std::memory_order_relaxed);
  }

  // Most create/delete requests one drain serves under the same carried
  // locks before it lets them go and takes them afresh (see Carry). It bounds
  // how long another connection waits for a shard or for a session's eph_mu.
  static constexpr uint32_t kCarryBound = 32;

  // The locks a drain carries from one create / create2 / delete frame to the
  // next, so a run of siblings locks its parent's shard and its own session's
  // eph_mu once per run, not once per request.
  //
  // Canonical lock order: shards by ascending index, then ONE eph_mu (two are
  // never held at once), then session_mu → conns_mu → conn->out_mu. The shard
  // locks and eph_mu are TreeLocks (node_store.hpp: try_lock and unlock are
  // one inline atomic each); the rest are std::mutex.
  // Blocking rule: a thread may BLOCK on a mutex only if everything it holds
  // comes earlier in that order. A carrying thread holds the parent's shard
  // and possibly eph_mu, so it takes a child shard with try_lock only; if
  // that fails it releases everything it carries and takes the locks in
  // canonical order (acquire_for below). Taking eph_mu while holding shards,
  // and the watch path's session_mu/conns_mu/out_mu while holding all of
  // them, blocks in order.
  //
  // A carry also ends at a parent in another shard, after kCarryBound
  // requests, and as soon as another thread is seen waiting for the carried
  // shard (Shard::waiters, lock_shard): with several connections at work a
  // shard changes hands within about one request.
  //
  // process_frames owns the one Carry of a drain; its destructor releases, so
  // no way out of the drain leaves a mutex locked. Everything that is not a
  // plain create/create2/delete releases first (handle_frame): any other op
  // may lock the carried shard itself (an exists on the parent's own shard
  // would otherwise deadlock on a TreeLock this thread holds), and
  // closeSession runs kill_session, which wants eph_mu with nothing held.
  struct Carry {
    TreeLock* shard_mu = nullptr;  // the parent shard's lock, held
    size_t shard_idx = 0;
    Session* eph = nullptr;  // the session whose eph_mu is held
    uint32_t served = 0;     // requests served since shard_mu was taken

    Carry() = default;
    Carry(const Carry&) = delete;
    Carry& operator=(const Carry&) = delete;
    ~Carry() { release(); }

    void drop_eph() {
      if (eph) {
        eph->eph_mu.unlock();
        eph = nullptr;
      }
    }
    void release() {
      drop_eph();
      if (shard_mu) {
        shard_mu->unlock();
        shard_mu = nullptr;
      }
      served = 0;
    }
  };

  EnsembleConfig cfg;
  Logger log;
  std::vector<std::unique_ptr<EventLoop>> loops;  // IO pool (>= #servers)
  std::vector<std::thread> threads;
  std::atomic<size_t> next_io{0};
  std::atomic<bool> started{false};
  std::atomic<int> latency_ms{0};
  std::atomic<int64_t> zxid_counter{0};
  std::unique_ptr<OpCounters[]> ops;  // loops.size() blocks, made by the first start()
  size_t n_ops = 0;
  OpCounters& cnt(const Conn* c) { return ops[c->io_idx]; }

  std::array<Shard, kShards> shards;

  mutable std::mutex session_mu;
  std::unordered_map<int64_t, SessionPtr> sessions;
  // no tombstone set needed: session ids are monotonic and never reused, so
  // an expired/closed id simply misses `sessions` ⇒ expired handshake
  int64_t next_session = 0x100000;

  mutable std::mutex conns_mu;
  std::unordered_map<uint64_t, ConnPtr> conns;
  std::atomic<uint64_t> next_conn_id{1};

  mutable std::mutex admin_mu;  // servers / leader / election
  std::vector<Server> servers;
  size_t leader_idx = 0;
  int64_t election_until = 0;  // monotonic ms; connects refused until then
  // quorum mode only (see the header comment). Written under admin_mu.
  std::atomic<bool> not_serving{false};
  bool has_leader = true;  // false from a quorum or leader loss until resume_serving
  uint64_t quorum_losses = 0;
  uint64_t dropped_conns = 0;
  std::atomic<uint64_t> refused_connects{0};

  explicit Impl(EnsembleConfig c) : cfg(std::move(c)), log(Logger("zk-ensemble").child("ensemble")) {
    log.set_level(cfg.log_level);
    latency_ms.store(cfg.latency_ms);
    PathRef root = ref_of("/");
    shards[root.hash % kShards].nodes.create(root, std::string_view());
  }

  Shard& shard_of(const PathRef& r) { return shards[r.hash % kShards]; }
  Shard& shard_of(std::string_view path) { return shard_of(ref_of(path)); }

  // Lock two shards without deadlock (index order; may be the same shard).
  struct TwoShardLock {
    std::unique_lock<TreeLock> a, b;
    Shard* first;   // shard i1
    Shard* second;  // shard i2
    TwoShardLock(Impl& impl, size_t i1, size_t i2) {
      first = &impl.shards[i1];
      second = &impl.shards[i2];
      if (i1 == i2) {
        a = std::unique_lock<TreeLock>(impl.shards[i1].mu);
      } else {
        a = std::unique_lock<TreeLock>(impl.shards[std::min(i1, i2)].mu);
        b = std::unique_lock<TreeLock>(impl.shards[std::max(i1, i2)].mu);
      }
    }
    TwoShardLock(Impl& impl, const PathRef& p1, const PathRef& p2)
        : TwoShardLock(impl, p1.hash % kShards, p2.hash % kShards) {}
  };

  // ---------------- tree primitives (shard locks held) ----------------

  // the node at r in whichever shard r hashes to, or null
  ZNode* find_node(const PathRef& r) { return shard_of(r).nodes.find(r); }

  // The mutations below are the only code that writes a znode's Stat (setACL's
  // aversion aside) or changes a link. The single-op handlers and multi's
  // apply phase both go through them. They mutate only: the caller holds the
  // shard locks of the node and of its parent, and fires the watches.

  // the only place a zxid is spent
  int64_t next_zxid() { return zxid_counter.fetch_add(1, std::memory_order_relaxed) + 1; }
  // what a reply that committed nothing reports
  int64_t last_zxid() const { return zxid_counter.load(std::memory_order_relaxed); }

  // A new node at cref (validated absent) under par, committed at zxid z: one
  // block for header, path and payload, linked into par's children.
  static ZNode& insert_node(Shard& csh, const PathRef& cref, std::string_view data, ZNode& par, int64_t z,
                            int64_t wall) {
    ZNode& n = *csh.nodes.create(cref, data);
    n.stat.czxid = z;
    n.stat.mzxid = z;
    n.stat.ctime = wall;
    n.stat.mtime = wall;
    n.stat.data_length = static_cast<int32_t>(data.size());
    link_child(par, n);
    child_list_changed(par, z);
    return n;
  }

  // par gained or lost a child at zxid z
  static void child_list_changed(ZNode& par, int64_t z) {
    par.stat.cversion++;
    par.stat.pzxid = z;
    par.stat.num_children = par.nchildren;
  }

  // Make the fresh node n an ephemeral of s; the caller holds s.eph_mu and
  // passes what it read from s.alive inside that same critical section.
  //
  // Ephemeral creates and session death. kill_session clears `alive`
  // under eph_mu and only then drains the session's index, one node at
  // a time, each pop under eph_mu again. A create reads `alive` and links
  // the new node inside ONE eph_mu critical section, so exactly one of two
  // things happens:
  //   - it saw alive: the node is in the index before the kill can
  //     take eph_mu to clear the flag, so the drain finds and removes
  //     it;
  //   - it saw !alive: the node is not linked, and must not stay.
  // handle_create reads `alive` before it inserts: on !alive nothing is
  // inserted and the create fails with SESSION_EXPIRED, so unlike a
  // create-then-roll-back no half-registered node is ever visible. Its
  // section is the drain's carried one: eph_mu is taken if the
  // carry does not hold it yet and stays held for the creates and
  // deletes that follow, at most kCarryBound of them. `alive` is still
  // read for EVERY ephemeral create, under the held mutex: a kill that
  // is waiting for eph_mu has not cleared it yet, and one that got in
  // between two carries is seen by the next read. The kill waits for at
  // most one carry.
  // handle_multi has inserted already (a transaction applies whole) and takes
  // eph_mu per node: on !alive it sets the owner on the unlinked node and
  // rolls that node back once the shard locks are released.
  // No ephemeral can therefore outlive its session.
  // Lock order: shard(s) → eph_mu (kill_session takes eph_mu alone).
  static void own_ephemeral(ZNode& n, Session& s, bool alive) {
    n.stat.ephemeral_owner = s.id;
    n.owner = &s;
    if (alive) eph_link(s, n);
  }

  // Take n (no children) out of its owner's ephemeral index and out of its
  // parent's children, at zxid z; returns the parent. Runs inside the node's
  // shard lock, BEFORE the erase: the index holds node pointers, so a node
  // must never be freed (or, worse, recycled) while linked.
  // `eph_held`: the session whose eph_mu the caller holds already (a drain's
  // carry), or null; *locks grows by the number of mutexes taken here.
  static ZNode* detach_node(ZNode& n, int64_t z, Session* eph_held, int* locks) {
    if (Session* o = n.owner) {
      if (o == eph_held) {
        eph_unlink(*o, n);
      } else {
        std::lock_guard<TreeLock> eg(o->eph_mu);
        eph_unlink(*o, n);
        ++*locks;
      }
    }
    ZNode* par = n.parent;
    if (par) {
      unlink_child(n);
      child_list_changed(*par, z);
    }
    return par;
  }

  static void apply_set_data(ZNode& n, std::string_view data, int64_t z, int64_t wall) {
    n.set_data(data);  // in place while it fits; the node never moves
    n.stat.mzxid = z;
    n.stat.mtime = wall;
    n.stat.version++;
    n.stat.data_length = static_cast<int32_t>(data.size());
  }

  // Remove node n (no children; its shard csh and its parent's shard psh
  // both locked): detach, watches (parent's child watch first, then
  // NodeDeleted), erase. Returns the zxid the removal committed at.
  int64_t remove_node_locked(Shard& csh, ZNode* np, Shard& psh, Session* eph_held, int* locks) {
    int64_t z = next_zxid();
    if (ZNode* par = detach_node(*np, z, eph_held, locks)) fire_child_watches_locked(psh, par->ref());
    fire_deleted_watches_locked(csh, np->ref());  // n's own path bytes: before the erase
    csh.nodes.erase(np);
    return z;
  }

  // The parent of a request path, hashed once per run of siblings within one
  // drain (pv must point into the connection's receive buffer).
  PathRef parent_ref(Conn* c, std::string_view pv) {
    if (c->last_parent.path.data() == nullptr || c->last_parent.path != pv) c->last_parent = ref_of(pv);
    return c->last_parent;
  }

  // The shard locks of one create/delete under the carry k. The parent's
  // shard (index pidx) ends up held in k: found there from the previous
  // request, or taken now. The child's shard (cidx) is returned as a lock of
  // the caller's scope, empty when the child lives in the parent's shard.
  // While k holds anything the child is only tried; see Carry for the rule.
  std::unique_lock<TreeLock> acquire_for(Carry& k, size_t cidx, size_t pidx, int* locks) {
    // the carry ends at its bound, at a parent in another shard, and as soon
    // as anybody is seen waiting for the carried shard (lock_shard)
    if (k.shard_mu && (k.shard_idx != pidx || k.served >= kCarryBound ||
                       shards[k.shard_idx].waiters.load(std::memory_order_relaxed) != 0))
      k.release();
    std::unique_lock<TreeLock> child;
    if (k.shard_mu && cidx != pidx) {
      child = std::unique_lock<TreeLock>(shards[cidx].mu, std::try_to_lock);
      if (child.owns_lock())
        ++*locks;
      else
        k.release();  // contended: let go of everything, then queue in order
    }
    if (!k.shard_mu) {
      // nothing is held here (release drops eph_mu too): ascending, blocking
      if (cidx < pidx) {
        child = lock_shard(shards[cidx]);
        ++*locks;
      }
      lock_shard(shards[pidx]).release();  // the carry owns it from here
      k.shard_mu = &shards[pidx].mu;
      k.shard_idx = pidx;
      ++*locks;
      if (cidx > pidx) {
        child = lock_shard(shards[cidx]);
        ++*locks;
      }
    }
    k.served++;
    return child;
  }

  // A blocking shard acquisition by a request handler (the caller holds
  // nothing later in the lock order). Uncontended it is one try_lock. When
  // the shard is taken, the holder may be a drain carrying it across many
  // requests, so the wait is announced in sh.waiters: a carrying thread looks
  // at that count before each request and lets go at once. That takes it
  // about one request, so spinning for a moment first is cheaper than going
  // to sleep in the kernel and being woken.
  static std::unique_lock<TreeLock> lock_shard(Shard& sh) {
    std::unique_lock<TreeLock> lk(sh.mu, std::try_to_lock);
    if (lk.owns_lock()) return lk;
    sh.waiters.fetch_add(1, std::memory_order_relaxed);
    for (int i = 0; i < 512 && !lk.owns_lock(); i++) {
      spin_pause();
      lk.try_lock();
    }
    if (!lk.owns_lock()) lk.lock();
    sh.waiters.fetch_sub(1, std::memory_order_relaxed);
    return lk;
  }

  // The one-path ops: hash the path once, lock its shard, look the node up,
  // and run fn(shard, ref, node-or-null) under that lock (one tree_locks).
  // Returns what fn returns, with the lock released.
  template <typename Fn>
  auto with_node(Conn* c, std::string_view path, Fn fn) {
    PathRef ref = ref_of(path);
    Shard& sh = shard_of(ref);
    std::unique_lock<TreeLock> lk = lock_shard(sh);
    bump(cnt(c).tree_locks);
    return fn(sh, ref, sh.nodes.find(ref));
  }

  // s->eph_mu into the carry. The caller holds shard locks only (all earlier
  // in the order), so this may block. Never two eph_mu at once.
  static void carry_eph(Carry& k, Session* s, int* locks) {
    if (k.eph == s) return;
    k.drop_eph();
    s->eph_mu.lock();
    k.eph = s;
    ++*locks;
  }

  // ---------------- lifecycle ----------------

  void start() {
    if (started.exchange(true)) return;
    size_t n = cfg.ports.size();
    size_t io = static_cast<size_t>(cfg.io_threads);
    if (io == 0) {
      unsigned hw = std::thread::hardware_concurrency();
      io = std::max(n, std::min<size_t>(8, hw ? hw / 4 : 2));
      if (io == 0) io = 1;
    }
    loops.clear();
    for (size_t i = 0; i < io; i++) loops.push_back(std::make_unique<EventLoop>());
    if (n_ops != io) {
      // the pool's size follows from cfg alone, so a restart keeps its counts
      ops = std::make_unique<OpCounters[]>(io);
      n_ops = io;
    }
    {
      std::lock_guard<std::mutex> g(admin_mu);
      servers.resize(n);
      for (size_t i = 0; i < n; i++) open_listener(i, cfg.ports[i]);
      if (cfg.quorum) {  // every server is up: server 0 leads, no pause
        leader_idx = 0;
        has_leader = true;
        election_until = 0;
        not_serving.store(false, std::memory_order_relaxed);
      }
    }
    for (size_t i = 0; i < io; i++) {
      threads.emplace_back([this, i] {
        if (i == 0) schedule_sweep();
        loops[i]->run();
      });
    }
  }

  void stop() {
    if (!started.load()) return;
    std::vector<std::promise<void>> done(loops.size());
    for (size_t i = 0; i < loops.size(); i++) {
      loops[i]->post([this, i, &done] {
        std::vector<ConnPtr> victims;
        {
          std::lock_guard<std::mutex> g(conns_mu);
          for (auto& kv : conns)
            if (kv.second->io_idx == i) victims.push_back(kv.second);
        }
        for (auto& c : victims) close_conn(c.get());
        {
          std::lock_guard<std::mutex> g(admin_mu);
          for (size_t srv = 0; srv < servers.size(); srv++) {
            if (srv % loops.size() == i && servers[srv].listen_fd >= 0) {
              loops[i]->del_fd(servers[srv].listen_fd);
              ::close(servers[srv].listen_fd);
              servers[srv].listen_fd = -1;
              servers[srv].up = false;
            }
          }
        }
        done[i].set_value();
      });
    }
    for (auto& d : done) d.get_future().wait();
    for (auto& l : loops) l->stop();
    for (auto& t : threads) t.join();
    threads.clear();
    started.store(false);
  }

  // admin_mu held
  void open_listener(size_t idx, int port) {
    int fd = socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (fd < 0) throw std::runtime_error("ensemble: socket() failed");
    int one = 1;
    setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    struct sockaddr_in addr;
    memset(&addr, 0, sizeof(addr));
    addr.sin_family = AF_INET;
    addr.sin_port = htons(static_cast<uint16_t>(port));
    inet_pton(AF_INET, cfg.bind_host.c_str(), &addr.sin_addr);
    if (bind(fd, reinterpret_cast<struct sockaddr*>(&addr), sizeof(addr)) < 0) {
      ::close(fd);
      throw std::runtime_error("ensemble: bind failed on port " + std::to_string(port));
    }
    if (listen(fd, 512) < 0) {
      ::close(fd);
      throw std::runtime_error("ensemble: listen failed");
    }
    socklen_t alen = sizeof(addr);
    getsockname(fd, reinterpret_cast<struct sockaddr*>(&addr), &alen);
    set_nonblock(fd);
    servers[idx].listen_fd = fd;
    servers[idx].port = ntohs(addr.sin_port);
    servers[idx].up = true;
    size_t srv = idx;
    size_t lidx = idx % loops.size();
    auto install = [this, fd, srv, lidx] {
      loops[lidx]->add_fd(fd, EPOLLIN, [this, fd, srv](uint32_t) { on_accept(fd, srv); });
    };
    if (loops[lidx]->on_loop_thread()) {
      install();
    } else if (started.load() && loops[lidx]->running()) {
      loops[lidx]->post(install);
    } else {
      install();  // loop thread not started yet: direct registration is safe
    }
  }

  // ---------------- socket handling (owner loop thread) ----------------

  void on_accept(int listen_fd, size_t server_idx) {
    while (true) {
      int fd = accept4(listen_fd, nullptr, nullptr, SOCK_NONBLOCK | SOCK_CLOEXEC);
      if (fd < 0) break;
      {
        std::lock_guard<std::mutex> g(admin_mu);
        if (now_ms() < election_until || not_serving.load(std::memory_order_relaxed)) {
          // mid-election, or (quorum mode) below a majority: nobody serves
          // (BASELINE config 4 storm realism)
          ::close(fd);
          refused_connects.fetch_add(1, std::memory_order_relaxed);
          continue;
        }
        // quorum mode chooses its leader when service resumes (resume_serving)
        if (!cfg.quorum) maybe_elect_leader_locked();
      }
      set_nodelay(fd);
      auto conn = std::make_shared<Conn>();
      conn->id = next_conn_id.fetch_add(1);
      conn->fd = fd;
      conn->server_idx = server_idx;
      conn->io_idx = next_io.fetch_add(1) % loops.size();
      uint64_t cid = conn->id;
      size_t io_idx = conn->io_idx;
      {
        std::lock_guard<std::mutex> g(conns_mu);
        conns[cid] = conn;
      }
      loops[io_idx]->add_fd(fd, EPOLLIN, [this, cid](uint32_t ev) { on_conn_event(cid, ev); });
    }
  }

  ConnPtr lookup(uint64_t cid) {
    std::lock_guard<std::mutex> g(conns_mu);
    auto it = conns.find(cid);
    return it == conns.end() ? nullptr : it->second;
  }

  void on_conn_event(uint64_t cid, uint32_t ev) {
    ConnPtr c = lookup(cid);
    if (!c) return;
    if (c->dead.load() || (ev & (EPOLLHUP | EPOLLERR))) {
      close_conn(c.get());
      return;
    }
    if (ev & EPOLLIN) {
      // read straight into the receive buffer's tail; frames are parsed in
      // place and the buffer only moves here, before the handlers run
      bool eof = false;
      while (true) {
        size_t room = 0;
        char* dst = c->inbuf.tail(65536, &room);
        ssize_t n = read(c->fd, dst, room);
        if (n > 0) {
          c->inbuf.commit(static_cast<size_t>(n));
        } else if (n == 0) {
          eof = true;  // process buffered frames (e.g. closeSession) first
          break;
        } else {
          if (errno == EAGAIN || errno == EWOULDBLOCK) break;
          if (errno == EINTR) continue;
          eof = true;
          break;
        }
      }
      // once per drain: both clocks, the parent-hash cache, the staging state
      c->drain_mono_ms = now_ms();
      c->drain_wall_ms = wall_ms();
      c->last_parent = PathRef{std::string_view(), 0};
      {
        std::lock_guard<std::mutex> og(c->out_mu);
        c->draining = true;
      }
      if (!process_frames(c.get())) return;
      // replies staged during this drain go out in one flush (syscall
      // batching: 1k pipelined creates ⇒ a handful of large writes)
      flush_out(c.get(), /*end_drain=*/true);
      if (c->dead.load()) return;  // flush_out may close on error/closing
      if (eof) {
        close_conn(c.get());
        return;
      }
      return;
    }
    if (ev & EPOLLOUT) flush_out(c.get());
  }

  // returns false if the conn was closed
  bool process_frames(Conn* c) {
    // the drain's carried locks: released by every op that is not a plain
    // create/delete, by close_conn, and by this holder's destructor on every
    // way out of the drain
    struct CarryScope {
      Conn* c;
      Carry carry;
      explicit CarryScope(Conn* cc) : c(cc) { c->carry = &carry; }
      ~CarryScope() {
        carry.release();
        c->carry = nullptr;
      }
    } scope(c);
    while (!c->dead.load()) {
      size_t avail = c->inbuf.size();
      if (avail < 4) break;
      const unsigned char* p = reinterpret_cast<const unsigned char*>(c->inbuf.ptr());
      uint32_t len = (static_cast<uint32_t>(p[0]) << 24) | (static_cast<uint32_t>(p[1]) << 16) |
                     (static_cast<uint32_t>(p[2]) << 8) | static_cast<uint32_t>(p[3]);
      if (len > 4 * 1024 * 1024) {  // jute.maxbuffer-ish sanity cap
        close_conn(c);
        return false;
      }
      if (avail < 4 + len) break;
      // consumed frames stay where they are until the next read's tail():
      // handlers hold views into them for the rest of the drain
      const char* body = c->inbuf.ptr() + 4;
      c->inbuf.consume(4 + len);
      if (!handle_frame(c, body, len)) {
        close_conn(c);
        return false;
      }
    }
    return true;
  }

  void touch(Conn* c) {
    if (c->session) c->session->last_touch.store(c->drain_mono_ms, std::memory_order_relaxed);
  }

  // returns false ⇒ caller closes the conn (protocol error)
  bool handle_frame(Conn* c, const char* body, size_t len) {
    try {
      JuteReader r(body, len);
      if (!c->handshaken) return handle_connect(c, r);
      RequestHeader hdr;
      hdr.deserialize(r);
      touch(c);
      // only consecutive create / create2 / delete frames carry locks; every
      // other op (unknown ones included) runs with nothing held
      if (hdr.type != kOpCreate && hdr.type != kOpCreate2 && hdr.type != kOpDelete) c->carry->release();
      switch (hdr.type) {
        case kOpPing:
          bump(cnt(c).ping);
          send_ack(c, kXidPing);
          break;
        case kOpCreate:
          handle_create(c, hdr.xid, r);
          break;
        case kOpCreate2:  // create + Stat in the response (3.5+ clients)
          handle_create(c, hdr.xid, r, /*with_stat=*/true);
          break;
        case kOpDelete:
          handle_delete(c, hdr.xid, r);
          break;
        case kOpExists:
          handle_exists(c, hdr.xid, r);
          break;
        case kOpGetData:
          handle_get_data(c, hdr.xid, r);
          break;
        case kOpSetData:
          handle_set_data(c, hdr.xid, r);
          break;
        case kOpGetChildren:
          handle_get_children(c, hdr.xid, r);
          break;
        case kOpGetACL:
          handle_get_acl(c, hdr.xid, r);
          break;
        case kOpSetACL:
          handle_set_acl(c, hdr.xid, r);
          break;
        case kOpGetChildren2:  // children + the node's Stat (3.4+ clients use it by default)
          handle_get_children(c, hdr.xid, r, /*with_stat=*/true);
          break;
        case kOpSync:
          handle_sync(c, hdr.xid, r);
          break;
        case kOpSetWatches:
          handle_set_watches(c, hdr.xid, r);
          break;
        case kOpMulti:
          handle_multi(c, hdr.xid, r);
          break;
        case kOpCloseSession:
          handle_close_session(c, hdr.xid);
          break;
        case kOpAuth:  // auth packet (xid -4): ACLs are open here, ack and ignore
                       // so real third-party clients that always send auth work
          send_ack(c, hdr.xid);
          break;
        default:
          bump(cnt(c).unknown);
          send_error(c, hdr.xid, kZSystemError);
          break;
      }
      return true;
    } catch (const std::exception& e) {
      c->carry->release();
      log.warn("ensemble: malformed frame, closing conn", {{"err", Json(e.what())}});
      return false;
    } catch (...) {
      // never unwind out of a drain: its staged replies would go unflushed
      c->carry->release();
      return false;
    }
  }

  // returns false ⇒ caller closes the conn with no ConnectResponse sent
  bool handle_connect(Conn* c, JuteReader& r) {
    if (not_serving.load(std::memory_order_relaxed)) {
      // quorum mode: accepted while serving, but service stopped since
      refused_connects.fetch_add(1, std::memory_order_relaxed);
      return false;
    }
    ConnectRequest req;
    req.deserialize(r);
    bump(cnt(c).connect);
    ConnectResponse resp;
    resp.has_read_only = req.has_read_only;
    bool expired_handshake = false;
    ConnPtr old_conn;
    {
      std::lock_guard<std::mutex> g(session_mu);
      if (req.session_id != 0) {
        auto sit = sessions.find(req.session_id);
        if (sit == sessions.end() || sit->second->passwd != req.passwd) {
          // unknown/expired/bad-passwd session ⇒ the canonical "expired"
          // ConnectResponse: sessionId=0, timeOut=0
          resp.session_id = 0;
          resp.time_out_ms = 0;
          expired_handshake = true;
          log.info("connect: session expired/unknown", {{"session", Json(req.session_id)}});
        } else {
          SessionPtr s = sit->second;
          uint64_t prev = s->conn_id.exchange(c->id);
          if (prev != 0) {
            std::lock_guard<std::mutex> cg(conns_mu);
            auto old = conns.find(prev);
            if (old != conns.end()) old_conn = old->second;
          }
          s->last_touch.store(now_ms());
          c->session = s;
          resp.session_id = s->id;
          resp.time_out_ms = s->timeout_ms;
          resp.passwd = s->passwd;
          log.info("connect: session re-attached", {{"session", Json(s->id)}});
        }
      } else {
        auto s = std::make_shared<Session>();
        s->id = next_session++;
        s->passwd.resize(16);
        uint64_t seed = static_cast<uint64_t>(s->id) * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
        for (int i = 0; i < 16; i++) {
          seed ^= seed >> 27;
          seed *= 0x94D049BB133111EBull;
          s->passwd[i] = static_cast<char>(seed >> (8 * (i % 8)));
        }
        int req_to = req.time_out_ms > 0 ? req.time_out_ms : 30000;
        s->timeout_ms = std::max(cfg.min_session_timeout_ms, std::min(cfg.max_session_timeout_ms, req_to));
        s->last_touch.store(now_ms());
        s->conn_id.store(c->id);
        c->session = s;
        resp.session_id = s->id;
        resp.time_out_ms = s->timeout_ms;
        resp.passwd = s->passwd;
        sessions[s->id] = s;
        log.info("connect: new session",
                 {{"session", Json(s->id)}, {"timeout_ms", Json(static_cast<int64_t>(s->timeout_ms))}});
      }
    }
    if (old_conn) {
      // session moved: retire the old connection without detaching
      old_conn->dead.store(true);
      post_close(old_conn);
    }
    c->handshaken = true;
    std::string pkt;
    begin_packet(&pkt);
    JuteWriter w(&pkt);
    resp.serialize(w);
    frame_packet(&pkt);
    if (expired_handshake) {
      std::lock_guard<std::mutex> og(c->out_mu);
      c->closing = true;  // expired handshake: notify, then close
    }
    send_packet(c, std::move(pkt));
    return true;
  }

  int64_t sid_of(Conn* c) const { return c->session ? c->session->id : 0; }

  // --- ops ---

  void handle_create(Conn* c, int32_t xid, JuteReader& r, bool with_stat = false) {
    bump(cnt(c).create);
    // parse in place: path and payload are views of the frame, which stays
    // put in c->inbuf for the whole drain. The ACL vector is validated and
    // skipped (the open-ACL server discards it).
    std::string_view path = r.read_string_view();
    std::string_view data = r.read_buffer_view();
    int32_t nacl = r.read_vec_count(12);
    for (int32_t i = 0; i < nacl; i++) {
      r.read_int();     // perms
      r.skip_string();  // scheme
      r.skip_string();  // id
    }
    int32_t flags = r.read_int();
    int32_t err = kZOk;
    int64_t op_zxid = 0;  // the zxid THIS create committed at
    Stat created_stat;    // snapshot for create2 replies
    std::string seq_path;  // SEQUENCE only: the path with its suffix
    std::string_view final_path = path;
    int locks = 0;  // mutexes this request took (tree_locks)
    size_t last_slash = 0;  // one pass validates the path and finds its parent
    if (!scan_path(path, &last_slash) || path.size() == 1) {  // "/" is the one valid path of a byte
      err = kZMarshallingError;
    } else {
      // one hash per path: it picks the shard and probes the map
      PathRef cref = ref_of(path);
      PathRef pref = parent_ref(c, parent_of(path, last_slash));
      // A SEQUENCE create carries nothing: it lets go of the drain's locks
      // and runs under a carry of its own, which this scope releases.
      Carry own_locks;
      if (flags & kSequence) c->carry->release();
      Carry& k = (flags & kSequence) ? own_locks : *c->carry;
      Shard* first_csh = &shard_of(cref);
      std::unique_lock<TreeLock> child_lk = acquire_for(k, cref.hash % kShards, pref.hash % kShards, &locks);
      Shard& psh = shard_of(pref);
      ZNode* parp = psh.nodes.find(pref);
      if (!parp) {
        err = kZNoNode;
      } else if (parp->stat.ephemeral_owner != 0) {
        err = kZNoChildrenForEphemerals;
      } else {
        ZNode& par = *parp;
        Shard* csh = first_csh;
        std::unique_lock<TreeLock> extra;
        if (flags & kSequence) {
          char suffix[16];
          snprintf(suffix, sizeof(suffix), "%010d", par.stat.cversion);
          seq_path.reserve(path.size() + 10);
          seq_path.assign(path);
          seq_path += suffix;
          final_path = seq_path;
          cref = ref_of(final_path);
          // NB: with SEQUENCE the final path may hash to a different shard
          // than the request path; lock it too in that (registrar-unused)
          // corner
          csh = &shard_of(cref);
          if (csh != first_csh && csh != &psh) {
            extra = std::unique_lock<TreeLock>(csh->mu, std::try_to_lock);
            if (!extra.owns_lock())
              err = kZSystemError;  // pathological shard collision
            else
              locks++;
          }
        }
        // an ephemeral is created only while its session is seen alive under
        // the carried eph_mu (own_ephemeral has the argument)
        Session* owner = nullptr;
        if (err == kZOk && (flags & kEphemeral)) {
          owner = c->session.get();
          if (owner) {
            carry_eph(k, owner, &locks);
            if (!owner->alive.load(std::memory_order_relaxed)) owner = nullptr;
          }
          if (!owner) err = kZSessionExpired;
        }
        if (err == kZOk && csh->nodes.find(cref)) err = kZNodeExists;
        if (err == kZOk) {
          op_zxid = next_zxid();
          ZNode& n = insert_node(*csh, cref, data, par, op_zxid, c->drain_wall_ms);
          if (owner) own_ephemeral(n, *owner, /*alive=*/true);
          fire_data_watches_locked(*csh, cref, kEventNodeCreated);
          fire_child_watches_locked(psh, pref);
          created_stat = n.stat;
        }
      }
    }
    if (locks) bump(cnt(c).tree_locks, static_cast<uint64_t>(locks));
    // mutating replies carry the op's OWN zxid (a fresh counter read could
    // exceed what this client actually observed — ADVICE r1). The path goes
    // out straight from the request bytes (or the SEQUENCE path).
    if (err != kZOk) return send_error(c, xid, err);
    send_fixed_reply(c, xid, op_zxid, 4 + final_path.size() + (with_stat ? Stat::kWireSize : 0), [&](auto& w) {
      w.write_string(final_path);                // CreateResponse
      if (with_stat) created_stat.serialize(w);  // Create2Response
    });
  }

  void handle_delete(Conn* c, int32_t xid, JuteReader& r) {
    bump(cnt(c).del);
    std::string_view path = r.read_string_view();
    int32_t version = r.read_int();
    int32_t err = kZOk;
    int64_t op_zxid = 0;
    int locks = 0;
    {
      // one critical section: both shards locked (the parent's carried from
      // the previous sibling where there was one), checks and removal together
      PathRef cref = ref_of(path);
      PathRef pref = parent_ref(c, parent_view(path));
      Carry& k = *c->carry;
      std::unique_lock<TreeLock> child_lk = acquire_for(k, cref.hash % kShards, pref.hash % kShards, &locks);
      Shard& csh = shard_of(cref);
      ZNode* n = csh.nodes.find(cref);
      if (!n || path == "/") {
        err = kZNoNode;
      } else if (n->nchildren != 0) {
        err = kZNotEmpty;
      } else if (version != -1 && version != n->stat.version) {
        err = kZBadVersion;
      } else {
        // The node leaves its owner's index under that owner's eph_mu. Our
        // own session's is carried (taken now if need be). Another
        // session's is taken for this node alone, and the carried one is
        // dropped first: two eph_mu are never held at once.
        if (Session* o = n->owner) {
          if (o == c->session.get())
            carry_eph(k, o, &locks);
          else
            k.drop_eph();
        }
        op_zxid = remove_node_locked(csh, n, shard_of(pref), k.eph, &locks);
      }
    }
    if (locks) bump(cnt(c).tree_locks, static_cast<uint64_t>(locks));
    send_reply(c, xid, op_zxid ? op_zxid : last_zxid(), err, nullptr);
  }

  // Full node removal for the callers that have only a path (session kill,
  // rollback): locks child+parent shards, updates parent, fires watches,
  // detaches from the owner session. Returns false if missing or not empty.
  // only_owner: remove the node only if it is that session's ephemeral.
  bool delete_node(std::string_view path, int64_t* out_zxid = nullptr, const Session* only_owner = nullptr) {
    PathRef cref = ref_of(path);
    PathRef pref = ref_of(parent_view(path));
    TwoShardLock lk(*this, cref, pref);
    Shard& csh = *lk.first;
    ZNode* n = csh.nodes.find(cref);
    if (!n) return false;
    if (n->nchildren != 0 || n->parent == nullptr) return false;
    if (only_owner && n->owner != only_owner) return false;
    int locks = 0;  // not a request handler: nothing counts them
    int64_t z = remove_node_locked(csh, n, *lk.second, nullptr, &locks);
    if (out_zxid) *out_zxid = z;
    return true;
  }

  void handle_exists(Conn* c, int32_t xid, JuteReader& r) {
    bump(cnt(c).exists);
    std::string_view path = r.read_string_view();
    bool watch = r.read_bool();
    Stat stat;
    int32_t err = with_node(c, path, [&](Shard& sh, const PathRef& ref, const ZNode* n) {
      // the watch registers even on a missing node: that is what it waits for
      if (watch) watch_set(sh.data_watches, ref).insert(sid_of(c));
      if (!n) return kZNoNode;
      stat = n->stat;
      return kZOk;
    });
    if (err != kZOk) return send_error(c, xid, err);
    send_stat_reply(c, xid, last_zxid(), stat);
  }

  void handle_get_data(Conn* c, int32_t xid, JuteReader& r) {
    bump(cnt(c).get_data);
    std::string_view path = r.read_string_view();
    bool watch = r.read_bool();
    GetDataResponse resp;
    int32_t err = with_node(c, path, [&](Shard& sh, const PathRef& ref, const ZNode* n) {
      if (!n) return kZNoNode;
      if (watch) watch_set(sh.data_watches, ref).insert(sid_of(c));
      resp.data = n->data();
      resp.stat = n->stat;
      return kZOk;
    });
    send_reply(c, xid, last_zxid(), err, [&](JuteWriter& w) { resp.serialize(w); });
  }

  void handle_set_data(Conn* c, int32_t xid, JuteReader& r) {
    bump(cnt(c).set_data);
    std::string_view path = r.read_string_view();
    std::string_view data = r.read_buffer_view();
    int32_t version = r.read_int();
    Stat stat;
    int64_t op_zxid = 0;
    int32_t err = with_node(c, path, [&](Shard& sh, const PathRef& ref, ZNode* n) {
      if (!n) return kZNoNode;
      if (version != -1 && version != n->stat.version) return kZBadVersion;
      op_zxid = next_zxid();
      apply_set_data(*n, data, op_zxid, c->drain_wall_ms);
      fire_data_watches_locked(sh, ref, kEventNodeDataChanged);
      stat = n->stat;
      return kZOk;
    });
    if (err != kZOk) return send_error(c, xid, err);
    send_stat_reply(c, xid, op_zxid, stat);
  }

  // getChildren, and getChildren2 (with_stat): the listing, then the node's Stat
  void handle_get_children(Conn* c, int32_t xid, JuteReader& r, bool with_stat = false) {
    bump(cnt(c).get_children);
    std::string_view path = r.read_string_view();
    bool watch = r.read_bool();
    GetChildrenResponse resp;
    Stat stat;
    int32_t err = with_node(c, path, [&](Shard& sh, const PathRef& ref, const ZNode* n) {
      if (!n) return kZNoNode;
      if (watch) watch_set(sh.child_watches, ref).insert(sid_of(c));
      list_children(*n, &resp.children);
      stat = n->stat;
      return kZOk;
    });
    send_reply(c, xid, last_zxid(), err, [&](JuteWriter& w) {
      resp.serialize(w);
      if (with_stat) stat.serialize(w);
    });
  }

  // multi (op 14): apply a create/delete/setData/check transaction
  // atomically. All involved shards are locked in index order (a large multi
  // effectively serializes — transactions are a correctness feature, not the
  // throughput path), ops are validated against an overlay of the
  // transaction's own effects, then applied; watches fire only on success.
  struct MultiOpParsed {
    int32_t type = 0;
    std::string path;
    std::string data;
    int32_t flags = 0;
    int32_t version = -1;
  };

  void handle_multi(Conn* c, int32_t xid, JuteReader& r) {
    std::vector<MultiOpParsed> mops;
    while (true) {
      MultiHeader mh;
      mh.deserialize(r);
      if (mh.done) break;
      MultiOpParsed mo;
      mo.type = mh.type;
      switch (mh.type) {
        case kOpCreate: {
          CreateRequest req;
          req.deserialize(r);
          mo.path = std::move(req.path);
          mo.data = std::move(req.data);
          mo.flags = req.flags;
          break;
        }
        case kOpDelete: {
          DeleteRequest req;
          req.deserialize(r);
          mo.path = std::move(req.path);
          mo.version = req.version;
          break;
        }
        case kOpSetData: {
          SetDataRequest req;
          req.deserialize(r);
          mo.path = std::move(req.path);
          mo.data = std::move(req.data);
          mo.version = req.version;
          break;
        }
        case kOpCheck: {  // check(path, version)
          mo.path = r.read_string();
          mo.version = r.read_int();
          break;
        }
        default:
          return send_error(c, xid, kZMarshallingError);
      }
      mops.push_back(std::move(mo));
    }

    std::vector<int32_t> results(mops.size(), kZOk);
    std::vector<std::string> created_paths(mops.size());
    // setData Stat snapshots taken while the shard locks are held — the
    // reply body must NOT re-read the tree after the locks are released
    // (concurrent create/delete on the shard would race the read)
    std::vector<Stat> setdata_stats(mops.size());
    int64_t txn_zxid = 0;  // zxid of the LAST op applied by this txn
    std::vector<std::pair<std::string, int32_t>> data_events;   // path, event type
    std::vector<std::string> child_events;                      // parent paths
    std::vector<std::string> deleted_paths;                     // NodeDeleted → own child watchers
    // ephemerals this txn created but could not index because the session
    // died mid-txn: rolled back after the shard locks are released
    std::vector<std::string> rollback;
    SessionPtr mine = c->session;
    int32_t txn_err = kZOk;

    {
      // lock every involved shard (paths + parents) in index order
      std::set<size_t> idxs;
      for (const auto& mo : mops) {
        idxs.insert(ref_of(mo.path).hash % kShards);
        idxs.insert(ref_of(parent_view(mo.path)).hash % kShards);
      }
      std::vector<std::unique_lock<TreeLock>> locks;
      locks.reserve(idxs.size());
      for (size_t i : idxs) locks.emplace_back(shards[i].mu);
      bump(cnt(c).tree_locks, locks.size());

      // ---- validate against tree + overlay of txn effects ----
      struct Overlay {
        // path -> (exists, ephemeral); absent = defer to tree
        std::unordered_map<std::string, std::pair<bool, bool>> state;
        std::unordered_map<std::string, int> child_delta;
        std::unordered_map<std::string, int32_t> version;  // post-op versions
      } ov;
      auto tree_node = [&](const std::string& p) -> ZNode* { return find_node(ref_of(p)); };
      auto ov_exists = [&](const std::string& p) -> bool {
        auto it = ov.state.find(p);
        if (it != ov.state.end()) return it->second.first;
        return tree_node(p) != nullptr;
      };
      auto ov_ephemeral = [&](const std::string& p) -> bool {
        auto it = ov.state.find(p);
        if (it != ov.state.end()) return it->second.second;
        ZNode* n = tree_node(p);
        return n && n->stat.ephemeral_owner != 0;
      };
      auto ov_child_count = [&](const std::string& p) -> int {
        ZNode* n = tree_node(p);
        int base = n ? static_cast<int>(n->nchildren) : 0;
        auto it = ov.child_delta.find(p);
        return base + (it == ov.child_delta.end() ? 0 : it->second);
      };
      auto ov_version = [&](const std::string& p) -> int32_t {
        auto it = ov.version.find(p);
        if (it != ov.version.end()) return it->second;
        bool created_in_txn = ov.state.count(p) && ov.state[p].first && !tree_node(p);
        if (created_in_txn) return 0;
        ZNode* n = tree_node(p);
        return n ? n->stat.version : 0;
      };

      for (size_t i = 0; i < mops.size(); i++) {
        const auto& mo = mops[i];
        int32_t err = kZOk;
        if (!valid_path(mo.path) || mo.path == "/") {
          err = (mo.type == kOpCreate && mo.path == "/") ? kZNodeExists : kZMarshallingError;
        } else {
          std::string parent(parent_view(mo.path));
          switch (mo.type) {
            case kOpCreate:
              if (mo.flags & kSequence) {
                err = kZMarshallingError;  // sequence-in-multi unsupported
              } else if (!ov_exists(parent)) {
                err = kZNoNode;
              } else if (ov_ephemeral(parent)) {
                err = kZNoChildrenForEphemerals;
              } else if (ov_exists(mo.path)) {
                err = kZNodeExists;
              } else {
                ov.state[mo.path] = {true, (mo.flags & kEphemeral) != 0};
                ov.version[mo.path] = 0;
                ov.child_delta[parent]++;
              }
              break;
            case kOpDelete: {
              if (!ov_exists(mo.path)) {
                err = kZNoNode;
              } else if (ov_child_count(mo.path) > 0) {
                err = kZNotEmpty;
              } else {
                if (mo.version != -1 && mo.version != ov_version(mo.path)) {
                  err = kZBadVersion;
                } else {
                  ov.state[mo.path] = {false, false};
                  ov.version.erase(mo.path);
                  ov.child_delta[parent]--;
                }
              }
              break;
            }
            case kOpSetData: {
              if (!ov_exists(mo.path)) {
                err = kZNoNode;
              } else if (mo.version != -1 && mo.version != ov_version(mo.path)) {
                err = kZBadVersion;
              } else {
                ov.version[mo.path] = ov_version(mo.path) + 1;  // txn-internal increment
              }
              break;
            }
            case kOpCheck: {
              if (!ov_exists(mo.path))
                err = kZNoNode;
              else if (mo.version != -1 && mo.version != ov_version(mo.path))
                err = kZBadVersion;
              break;
            }
          }
        }
        if (err != kZOk && txn_err == kZOk) {
          txn_err = err;
          results[i] = err;
        } else if (txn_err != kZOk) {
          results[i] = kZRuntimeInconsistency;
        }
      }
      if (txn_err != kZOk) {
        // everything before the failure reports RuntimeInconsistency too
        for (size_t i = 0; i < mops.size(); i++)
          if (results[i] == kZOk) results[i] = kZRuntimeInconsistency;
      } else {
        // ---- apply (all locks still held) ----
        for (size_t i = 0; i < mops.size(); i++) {
          const auto& mo = mops[i];
          std::string parent(parent_view(mo.path));
          switch (mo.type) {
            case kOpCreate: {
              bump(cnt(c).create);
              txn_zxid = next_zxid();
              PathRef cref = ref_of(mo.path);
              // validated above: the path is absent and the parent is there
              ZNode& n = insert_node(shard_of(cref), cref, mo.data, *find_node(ref_of(parent)), txn_zxid,
                                     c->drain_wall_ms);
              if ((mo.flags & kEphemeral) && mine) {
                // a create that finds its session dead is rolled back once
                // the locks are released (own_ephemeral has the argument)
                std::lock_guard<TreeLock> eg(mine->eph_mu);
                bump(cnt(c).tree_locks);
                bool alive = mine->alive.load(std::memory_order_relaxed);
                own_ephemeral(n, *mine, alive);
                if (!alive) rollback.push_back(mo.path);
              }
              data_events.push_back({mo.path, kEventNodeCreated});
              child_events.push_back(parent);
              created_paths[i] = mo.path;
              break;
            }
            case kOpDelete: {
              bump(cnt(c).del);
              txn_zxid = next_zxid();
              PathRef cref = ref_of(mo.path);
              Shard& csh = shard_of(cref);
              if (ZNode* n = csh.nodes.find(cref)) {
                // may be ANOTHER session's ephemeral: leaves its owner's index
                int took = 0;
                detach_node(*n, txn_zxid, nullptr, &took);
                bump(cnt(c).tree_locks, static_cast<uint64_t>(took));
                csh.nodes.erase(n);
              }
              data_events.push_back({mo.path, kEventNodeDeleted});
              child_events.push_back(parent);
              deleted_paths.push_back(mo.path);
              break;
            }
            case kOpSetData: {
              bump(cnt(c).set_data);
              txn_zxid = next_zxid();
              if (ZNode* n = find_node(ref_of(mo.path))) {
                apply_set_data(*n, mo.data, txn_zxid, c->drain_wall_ms);
                setdata_stats[i] = n->stat;
              }
              data_events.push_back({mo.path, kEventNodeDataChanged});
              break;
            }
            default:
              break;  // check: no effect
          }
        }
        // fire watches while holding the shard locks (same discipline as
        // the single-op handlers: shard → session_mu → conns_mu → out_mu)
        for (auto& [path, ev] : data_events) {
          PathRef ref = ref_of(path);
          if (ev != kEventNodeDeleted) fire_data_watches_locked(shard_of(ref), ref, ev);
        }
        for (auto& path : deleted_paths) {
          PathRef ref = ref_of(path);
          fire_deleted_watches_locked(shard_of(ref), ref);
        }
        std::set<std::string> fired;
        for (auto& parent : child_events) {
          PathRef ref = ref_of(parent);
          if (fired.insert(parent).second) fire_child_watches_locked(shard_of(ref), ref);
        }
      }
    }

    // our session died mid-txn: remove the ephemerals it created but could
    // not index (the session's drain never saw them). After the shard locks
    // are released — delete_node takes them itself.
    for (const auto& path : rollback) delete_node(path, nullptr, mine.get());

    // reply with THIS txn's last zxid (not a fresh counter read, which may
    // already reflect other connections' later commits)
    int64_t z = txn_zxid ? txn_zxid : last_zxid();
    send_reply_with_body(c, xid, z, txn_err, [&](JuteWriter& w) {
      for (size_t i = 0; i < mops.size(); i++) {
        MultiHeader mh;
        mh.done = false;
        if (txn_err != kZOk) {
          mh.type = -1;
          mh.err = results[i];
          mh.serialize(w);
          w.write_int(results[i]);  // ErrorResult
        } else {
          mh.type = mops[i].type;
          mh.err = 0;
          mh.serialize(w);
          if (mops[i].type == kOpCreate) w.write_string(created_paths[i]);
          if (mops[i].type == kOpSetData) setdata_stats[i].serialize(w);
        }
      }
      MultiHeader end;
      end.type = -1;
      end.done = true;
      end.err = -1;
      end.serialize(w);
    });
  }

  // setWatches: re-arm a reconnected session's watches, firing synthetic
  // events for anything that changed past relative_zxid while it was away
  void handle_set_watches(Conn* c, int32_t xid, JuteReader& r) {
    SetWatchesRequest req;
    req.deserialize(r);
    int64_t sid = sid_of(c);
    // `missed` names the event a node's state calls for, or kEventNone to arm
    // the watch in `map`. The event goes out once the shard lock is released.
    auto rearm = [&](const std::vector<std::string>& paths, WatchMap Shard::*map, auto missed) {
      for (const auto& path : paths) {
        int32_t ev = with_node(c, path, [&](Shard& sh, const PathRef& ref, const ZNode* n) {
          int32_t e = missed(n);
          if (e == kEventNone) watch_set(sh.*map, ref).insert(sid);
          return e;
        });
        if (ev != kEventNone) deliver_watch({sid}, path, ev);
      }
    };
    int64_t since = req.relative_zxid;
    rearm(req.data_watches, &Shard::data_watches, [&](const ZNode* n) {
      return !n ? kEventNodeDeleted : n->stat.mzxid > since ? kEventNodeDataChanged : kEventNone;
    });
    rearm(req.exist_watches, &Shard::data_watches, [](const ZNode* n) {
      return n ? kEventNodeCreated : kEventNone;  // appeared while the client was away
    });
    rearm(req.child_watches, &Shard::child_watches, [&](const ZNode* n) {
      return !n ? kEventNodeDeleted : n->stat.pzxid > since ? kEventNodeChildrenChanged : kEventNone;
    });
    send_ack(c, xid);
  }

  // sync: single-copy tree ⇒ always in sync; echo the path back
  void handle_sync(Conn* c, int32_t xid, JuteReader& r) {
    std::string path = r.read_string();
    send_reply(c, xid, last_zxid(), kZOk, [&](JuteWriter& w) { w.write_string(path); });
  }

  // ACLs: everything is world:anyone (matching the reference's deployments);
  // getACL reports the open ACL, setACL acks without enforcement
  void handle_get_acl(Conn* c, int32_t xid, JuteReader& r) {
    std::string path = r.read_string();
    Stat stat;
    int32_t err = with_node(c, path, [&](Shard&, const PathRef&, const ZNode* n) {
      if (!n) return kZNoNode;
      stat = n->stat;
      return kZOk;
    });
    send_reply(c, xid, last_zxid(), err, [&](JuteWriter& w) {
      write_acl_vector(w, {ACL{}});
      stat.serialize(w);
    });
  }

  void handle_set_acl(Conn* c, int32_t xid, JuteReader& r) {
    std::string path = r.read_string();
    (void)read_acl_vector(r);
    r.read_int();  // version
    Stat stat;
    int32_t err = with_node(c, path, [&](Shard&, const PathRef&, ZNode* n) {
      if (!n) return kZNoNode;
      n->stat.aversion++;
      stat = n->stat;
      return kZOk;
    });
    send_reply(c, xid, last_zxid(), err, [&](JuteWriter& w) { stat.serialize(w); });
  }

  void handle_close_session(Conn* c, int32_t xid) {
    bump(cnt(c).close_session);
    int64_t sid = sid_of(c);
    {
      std::lock_guard<std::mutex> og(c->out_mu);
      c->closing = true;  // close after the reply drains
    }
    send_ack(c, xid);
    if (sid != 0) kill_session(sid, /*close_conn_too=*/false);
  }

  // ---------------- session lifecycle ----------------

  // Expire/close a session: remove ephemerals (firing watches), tombstone it,
  // optionally retire its connection. Lock discipline: session_mu alone, then
  // eph_mu alone, then per-path shard locks via delete_node; it never holds
  // two of them at once, so it blocks on each with nothing held, which the
  // blocking rule (struct Carry) always allows. A drain of this session's
  // connection may be carrying eph_mu: each wait here lasts at most one
  // carry, kCarryBound requests. A caller on an IO loop (closeSession) has
  // released its own carry first (handle_frame), or the eph_mu lock below
  // would be a self-deadlock.
  // `s` stays on this stack until the drain below is through: that is what
  // lets ZNode::owner be a plain pointer (see there).
  void kill_session(int64_t sid, bool close_conn_too) {
    SessionPtr s;
    {
      std::lock_guard<std::mutex> g(session_mu);
      auto it = sessions.find(sid);
      if (it == sessions.end()) return;
      s = it->second;
      sessions.erase(it);
    }
    {
      // under eph_mu: a create links a node only if it reads alive==true
      // inside its own eph_mu section, so everything ever linked is linked
      // before this store and is found by the drain below (handle_create
      // has the full argument)
      std::lock_guard<TreeLock> eg(s->eph_mu);
      s->alive.store(false, std::memory_order_release);
    }
    // Drain one node at a time: pop it under eph_mu (a linked node cannot be
    // freed — whoever removes it must take eph_mu to unlink it first), copy
    // its path, then delete by path with no lock held, as before.
    // INVARIANT: between the pop and the delete no lock is held, and
    // delete_node looks the PATH up again. The node it finds may no longer be
    // the one popped: another session can have deleted the stale node and
    // created its own at the same path in that window (the registrar's
    // takeover of a dead predecessor's paths does exactly this). So the
    // delete is conditional on the node still being owned by the dying
    // session; anything else at that path is somebody else's and stays.
    std::string p;
    while (true) {
      {
        std::lock_guard<TreeLock> eg(s->eph_mu);
        ZNode* n = s->eph_head;
        if (!n) break;
        p.assign(n->path());
        eph_unlink(*s, *n);
      }
      delete_node(p, nullptr, s.get());
    }
    // stale watch registrations for this session are skipped at fire time
    uint64_t cid = s->conn_id.load();
    if (close_conn_too && cid != 0) {
      ConnPtr cp = lookup(cid);
      if (cp) {
        cp->dead.store(true);
        post_close(cp);
      }
    }
  }

  void schedule_sweep() {
    loops[0]->schedule(cfg.tick_ms, [this] {
      std::vector<int64_t> expired;
      // quorum mode: only a leader expires sessions, and resume_serving has
      // restarted every timer before this reads false again
      if (!not_serving.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> g(session_mu);
        int64_t now = now_ms();
        for (const auto& kv : sessions)
          if (now - kv.second->last_touch.load(std::memory_order_relaxed) > kv.second->timeout_ms)
            expired.push_back(kv.first);
      }
      for (int64_t sid : expired) {
        log.info("session expired", {{"session", Json(sid)}});
        kill_session(sid, /*close_conn_too=*/true);
      }
      schedule_sweep();
    });
  }

  // ---------------- structural audit (tests, stress driver) ----------------

  // Every structural invariant of the tree, checked against the stored
  // state; one line per violation, none when the tree is sound. Never on a
  // request path. Locks: all shards in index order, then session_mu for a
  // snapshot, then every snapshotted session's eph_mu (shard → eph_mu, as the
  // handlers). kill_session moves a session's list and `alive` under eph_mu
  // alone, so while an expiry is in flight the list-against-node checks can
  // name a node that has been popped and not yet deleted: callers audit only
  // when no expiry is running. Marked cold so that its bulk stays out of the
  // handlers' text.
  __attribute__((cold, noinline)) std::vector<std::string> audit() {
    std::vector<std::string> out;
    auto bad = [&out](std::string_view where, const std::string& what) {
      out.push_back(std::string(where) + ": " + what);
    };
    std::vector<std::unique_lock<TreeLock>> locks;
    locks.reserve(kShards);
    for (auto& sh : shards) locks.emplace_back(sh.mu);
    std::vector<SessionPtr> snap;
    {
      std::lock_guard<std::mutex> g(session_mu);
      for (const auto& kv : sessions) {
        if (kv.first != kv.second->id) bad("session " + std::to_string(kv.first), "keyed under another id");
        snap.push_back(kv.second);
      }
    }
    std::sort(snap.begin(), snap.end(), [](const SessionPtr& a, const SessionPtr& b) { return a->id < b->id; });
    std::vector<std::unique_lock<TreeLock>> eph_locks;
    eph_locks.reserve(snap.size());
    std::unordered_set<const Session*> known;
    for (const auto& s : snap) {
      eph_locks.emplace_back(s->eph_mu);
      known.insert(s.get());
    }

    size_t total = 0;
    for (auto& sh : shards) total += sh.nodes.count;

    for (size_t si = 0; si < kShards; si++) {
      NodeStore& st = shards[si].nodes;
      std::string shard_name = "shard " + std::to_string(si);
      size_t seen = 0;
      for (size_t b = 0; b < st.nbuckets; b++) {
        for (ZNode* n = st.buckets[b]; n && seen <= st.count; n = n->chain) {
          seen++;
          std::string_view path = n->path();
          if (!valid_path(path)) {
            bad(shard_name, "node with an invalid path in bucket " + std::to_string(b));
            continue;
          }
          if (n->hash != std::hash<std::string_view>{}(path)) bad(path, "stored hash is not the hash of the path");
          if (n->hash % kShards != si) bad(path, "sits in shard " + std::to_string(si) + ", not the one its hash selects");
          if (st.bucket_of(n->hash) != b) bad(path, "sits in bucket " + std::to_string(b) + ", not the one its hash selects");

          // parent link
          if (path == "/") {
            if (n->parent) bad(path, "root has a parent");
          } else if (!n->parent) {
            bad(path, "no parent link");
          } else if (find_node(ref_of(parent_view(path))) != n->parent) {
            bad(path, "parent link is not the node at the parent path");
          }

          // children: the sibling list, its links, both counts
          int32_t walked = 0;
          const ZNode* prev = nullptr;
          for (const ZNode* c = n->first_child; c; c = c->sib_next) {
            if (static_cast<size_t>(walked) > total) {
              bad(path, "sibling list does not end");
              break;
            }
            walked++;
            if (c->parent != n) bad(path, "child " + std::string(c->path()) + " points at another parent");
            if (c->sib_prev != prev) bad(path, "child " + std::string(c->path()) + " has a wrong sib_prev");
            prev = c;
          }
          if (walked != n->nchildren)
            bad(path, "sibling list has " + std::to_string(walked) + " nodes, nchildren is " +
                          std::to_string(n->nchildren));
          if (n->stat.num_children != n->nchildren)
            bad(path, "stat.num_children " + std::to_string(n->stat.num_children) + " != nchildren " +
                          std::to_string(n->nchildren));

          // data placement
          if (n->stat.data_length != static_cast<int32_t>(n->data_len))
            bad(path, "stat.data_length " + std::to_string(n->stat.data_length) + " != data_len " +
                          std::to_string(n->data_len));
          if (n->path_len > n->inline_cap) {
            bad(path, "path longer than the block");
          } else {
            bool fits = n->data_len <= n->inline_cap - n->path_len;
            if (fits && n->ext) bad(path, "data fits the block but is out of line");
            if (!fits && !n->ext) bad(path, "data does not fit the block but there is no out-of-line buffer");
            if (n->ext && n->ext_cap < n->data_len) bad(path, "out-of-line buffer smaller than the data");
          }

          // ownership
          Session* owner = n->owner;
          bool linked = false;
          if (owner) {
            if (known.count(owner)) {
              linked = n->eph_linked;  // its eph_mu is held
            } else {
              std::lock_guard<TreeLock> eg(owner->eph_mu);
              linked = n->eph_linked;
            }
          }
          if ((n->stat.ephemeral_owner != 0) != (owner != nullptr && linked))
            bad(path, "stat.ephemeral_owner " + std::to_string(n->stat.ephemeral_owner) + " but owner " +
                          (owner ? "set" : "unset") + ", " + (linked ? "linked" : "not linked"));
          if (owner) {
            if (!known.count(owner)) bad(path, "owner session " + std::to_string(owner->id) + " is not in sessions");
            if (!owner->alive.load(std::memory_order_acquire))
              bad(path, "owner session " + std::to_string(owner->id) + " is not alive");
            if (owner->id != n->stat.ephemeral_owner)
              bad(path, "owner session " + std::to_string(owner->id) + " != stat.ephemeral_owner " +
                            std::to_string(n->stat.ephemeral_owner));
          }
        }
      }
      if (seen != st.count)
        bad(shard_name, "chains hold " + std::to_string(seen) + " nodes, count is " + std::to_string(st.count));

      // free lists
      size_t sum = 0;
      for (size_t c = 0; c < kNumClasses; c++) {
        sum += st.free_count[c];
        if (st.free_count[c] > kMaxCachedPerClass)
          bad(shard_name, "class " + std::to_string(c) + " caches " + std::to_string(st.free_count[c]) + " blocks");
        size_t len = 0;
        for (NodeStore::FreeBlock* f = st.free_head[c]; f && len <= st.free_count[c]; f = f->next) len++;
        if (len != st.free_count[c])
          bad(shard_name, "class " + std::to_string(c) + " free list length differs from free_count " +
                              std::to_string(st.free_count[c]));
      }
      if (sum != st.cached)
        bad(shard_name, "cached " + std::to_string(st.cached) + " != sum of free_count " + std::to_string(sum));
    }

    // each session's ephemeral list against the table
    for (const auto& s : snap) {
      std::string name = "session " + std::to_string(s->id);
      size_t len = 0;
      const ZNode* prev = nullptr;
      for (ZNode* n = s->eph_head; n; n = n->eph_next) {
        if (len > total) {
          bad(name, "ephemeral list does not end");
          break;
        }
        len++;
        if (n->eph_prev != prev) bad(name, "ephemeral list has a wrong eph_prev");
        prev = n;
        if (find_node(n->ref()) != n) {
          bad(name, "listed node is not in the table at its path");
          continue;
        }
        if (n->owner != s.get()) bad(name, "lists " + std::string(n->path()) + ", which has another owner");
        if (!n->eph_linked) bad(name, "lists " + std::string(n->path()) + ", which is not marked linked");
      }
      if (len != s->eph_count)
        bad(name, "ephemeral list has " + std::to_string(len) + " nodes, eph_count is " +
                      std::to_string(s->eph_count));
    }
    return out;
  }

  // ---------------- watches (shard lock held) ----------------

  // the watcher set for `ref`, created on first use
  static std::set<int64_t>& watch_set(WatchMap& m, const PathRef& ref) {
    auto it = m.find(ref);
    if (it == m.end()) it = m.emplace(PathKey{std::string(ref.path), ref.hash}, std::set<int64_t>()).first;
    return it->second;
  }

  // A shard with no watches at all (the registration hot path) skips the
  // probes.
  void fire_data_watches_locked(Shard& sh, const PathRef& ref, int32_t event_type) {
    if (sh.data_watches.empty()) return;
    auto it = sh.data_watches.find(ref);
    if (it == sh.data_watches.end()) return;
    std::set<int64_t> watchers = std::move(it->second);
    sh.data_watches.erase(it);
    deliver_watch(watchers, ref.path, event_type);
  }

  void fire_child_watches_locked(Shard& sh, const PathRef& ref) {
    if (sh.child_watches.empty()) return;
    auto it = sh.child_watches.find(ref);
    if (it == sh.child_watches.end()) return;
    std::set<int64_t> watchers = std::move(it->second);
    sh.child_watches.erase(it);
    deliver_watch(watchers, ref.path, kEventNodeChildrenChanged);
  }

  // NodeDeleted goes to data watchers AND child watchers of the deleted
  // node, deduplicated per session — ZooKeeper's DataTree passes the
  // already-triggered set to the child-watch trigger so a session holding
  // both watch kinds gets ONE event
  void fire_deleted_watches_locked(Shard& sh, const PathRef& ref) {
    if (sh.data_watches.empty() && sh.child_watches.empty()) return;
    std::set<int64_t> watchers;
    if (auto it = sh.data_watches.find(ref); it != sh.data_watches.end()) {
      watchers = std::move(it->second);
      sh.data_watches.erase(it);
    }
    if (auto it = sh.child_watches.find(ref); it != sh.child_watches.end()) {
      watchers.insert(it->second.begin(), it->second.end());
      sh.child_watches.erase(it);
    }
    if (!watchers.empty()) deliver_watch(watchers, ref.path, kEventNodeDeleted);
  }

  // One event packet, built once; every live watcher gets a copy.
  void deliver_watch(const std::set<int64_t>& watchers, std::string_view path, int32_t event_type) {
    std::string pkt;
    build_packet(&pkt, kXidWatcherEvent, -1, kZOk, [&](JuteWriter& w) {
      WatcherEvent ev;
      ev.type = event_type;
      ev.state = kStateSyncConnected;
      ev.path = std::string(path);
      ev.serialize(w);
    });
    for (int64_t sid : watchers) {
      uint64_t cid = 0;
      {
        std::lock_guard<std::mutex> g(session_mu);
        auto sit = sessions.find(sid);
        if (sit == sessions.end()) continue;  // stale registration
        cid = sit->second->conn_id.load();
      }
      if (cid == 0) continue;
      ConnPtr cp = lookup(cid);
      if (cp) send_packet(cp.get(), pkt);
    }
  }

  // ---------------- response sending ----------------

  // Every reply and every watch event starts with this header; the two
  // functions below are the only encoders of it.
  // (inlined always, as ReplyHeader::serialize is: out of line it costs the
  // in-place path a call per reply)
  template <typename W>
  [[gnu::always_inline]] static inline void write_reply_header(W& w, int32_t xid, int64_t zxid, int32_t err) {
    ReplyHeader hdr;
    hdr.xid = xid;
    hdr.zxid = zxid;
    hdr.err = err;
    hdr.serialize(w);
  }

  // A whole framed packet into *pkt (overwritten): length prefix, header,
  // then whatever body writes.
  template <typename BodyFn>
  static void build_packet(std::string* pkt, int32_t xid, int64_t zxid, int32_t err, BodyFn body) {
    begin_packet(pkt);
    JuteWriter w(pkt);
    write_reply_header(w, xid, zxid, err);
    body(w);
    frame_packet(pkt);
  }

  // true: replies are laid straight into the connection's staging buffer
  // (handlers run on the owner loop inside a drain) — no lock, no allocation,
  // no timer; the flush that ends the drain moves it to outbuf once
  bool staging(const Conn* c) const { return c->draining && latency_ms.load(std::memory_order_relaxed) == 0; }

  // A reply whose body (nullptr: none) goes out only when err is OK.
  template <typename BodyFn>
  void send_reply(Conn* c, int32_t xid, int64_t zxid, int32_t err, BodyFn body) {
    constexpr bool kHasBody = !std::is_same_v<BodyFn, std::nullptr_t>;
    auto body_if_ok = [&](JuteWriter& w) {
      if constexpr (kHasBody) {
        if (err == kZOk) body(w);
      }
    };
    if (staging(c)) {
      if (c->dead.load(std::memory_order_relaxed)) return;
      if (!kHasBody || err != kZOk) {
        // header-only reply (acks and every error): fixed 20 bytes
        stage_fixed(c, xid, zxid, err, 0, [](RawWriter&) {});
      } else {
        // variable-size bodies (getData, listings, ACLs): the generic writer
        // into a scratch string, then one append
        build_packet(&c->scratch, xid, zxid, err, body_if_ok);
        c->stage.append(c->scratch);
        c->stage_pub.store(c->stage.size(), std::memory_order_release);
      }
      return;
    }
    std::string pkt;
    build_packet(&pkt, xid, zxid, err, body_if_ok);
    send_packet(c, std::move(pkt));
  }

  // header-only replies at a fresh zxid read (nothing was committed)
  void send_error(Conn* c, int32_t xid, int32_t err) { send_reply(c, xid, last_zxid(), err, nullptr); }
  void send_ack(Conn* c, int32_t xid) { send_error(c, xid, kZOk); }

  // Owner loop, inside a drain, no latency injection: lay one reply of known
  // size down in the staging buffer. Room for the frame prefix, the
  // ReplyHeader and body_size body bytes is made once; the fields go in as
  // big-endian stores through a bump pointer. body must write exactly
  // body_size bytes when err is OK (and is not called otherwise).
  template <typename BodyFn>
  void stage_fixed(Conn* c, int32_t xid, int64_t zxid, int32_t err, size_t body_size, BodyFn body) {
    size_t n = ReplyHeader::kWireSize + (err == kZOk ? body_size : 0);
    RawWriter w(c->stage.reserve(4 + n));
    w.write_int(static_cast<int32_t>(n));
    write_reply_header(w, xid, zxid, err);
    if (err == kZOk) body(w);
    c->stage.commit(4 + n);
    c->stage_pub.store(c->stage.size(), std::memory_order_release);
  }

  // An OK reply whose body has a fixed layout of body_size bytes (a Stat, a
  // created path, both): encoded in place on the fast path; the same body
  // function drives the generic writer everywhere else (latency injection,
  // sends from outside a drain), so the field order lives in one place.
  template <typename BodyFn>
  void send_fixed_reply(Conn* c, int32_t xid, int64_t zxid, size_t body_size, BodyFn body) {
    if (staging(c)) {
      if (c->dead.load(std::memory_order_relaxed)) return;
      stage_fixed(c, xid, zxid, kZOk, body_size, body);
      return;
    }
    send_reply(c, xid, zxid, kZOk, body);
  }

  void send_stat_reply(Conn* c, int32_t xid, int64_t zxid, const Stat& stat) {
    send_fixed_reply(c, xid, zxid, Stat::kWireSize, [&](auto& w) { stat.serialize(w); });
  }

  // multi replies carry a body even on failure (per-op error results)
  template <typename BodyFn>
  void send_reply_with_body(Conn* c, int32_t xid, int64_t zxid, int32_t err, BodyFn body) {
    std::string pkt;
    build_packet(&pkt, xid, zxid, err, body);
    send_packet(c, std::move(pkt));
  }

  // Any thread. Latency injection routes through the owner loop's timers
  // (FIFO for equal deadlines), preserving per-conn response order.
  void send_packet(Conn* c, std::string pkt) {
    int lat = latency_ms.load();
    if (lat > 0) {
      uint64_t cid = c->id;
      loops[c->io_idx]->schedule_from_any(lat, [this, cid, pkt = std::move(pkt)]() mutable {
        ConnPtr cp = lookup(cid);
        if (cp) deliver(cp.get(), std::move(pkt));
      });
      return;
    }
    if (loops[c->io_idx]->on_loop_thread()) {
      if (c->draining) {
        // the connection being drained right now (multi / connect replies,
        // watch events its own request fired): stage behind the replies
        // already staged, so per-connection order is generation order
        if (c->dead.load()) return;
        c->stage.append(pkt);
        c->stage_pub.store(c->stage.size(), std::memory_order_release);
        return;
      }
      // another connection of this loop: queue only; flushed by a
      // same-iteration 0 ms timer (also the safety net for sends outside the
      // event path, e.g. sweep-timer watch deliveries)
      {
        std::lock_guard<std::mutex> og(c->out_mu);
        if (c->dead.load()) return;
        c->outbuf.append(pkt);
      }
      ensure_flush_scheduled(c);
      return;
    }
    deliver(c, std::move(pkt));
  }

  // owner loop thread only
  void ensure_flush_scheduled(Conn* c) {
    if (c->flush_scheduled) return;
    c->flush_scheduled = true;
    uint64_t cid = c->id;
    loops[c->io_idx]->schedule(0, [this, cid] {
      ConnPtr cp = lookup(cid);
      if (!cp) return;
      cp->flush_scheduled = false;
      if (!cp->dead.load()) flush_out(cp.get());
    });
  }

  // Cross-thread delivery: direct write when the buffer is clear, else
  // buffer + arm EPOLLOUT on the owner loop.
  void deliver(Conn* c, std::string pkt) {
    std::lock_guard<std::mutex> og(c->out_mu);
    if (c->dead.load()) return;
    if (c->draining && !loops[c->io_idx]->on_loop_thread()) {
      // The owner loop is mid-drain with replies staged outside this lock.
      // Record the stage position this packet arrived at; the drain's flush
      // interleaves it there. That is where a locked append would have put
      // it: a reply the owner stages after taking a shard lock we released
      // (e.g. a read of data whose watch we are delivering) is published
      // after this load and so stays behind the event.
      c->xq.emplace_back(c->stage_pub.load(std::memory_order_acquire), std::move(pkt));
      return;
    }
    if (c->outbuf.empty()) {
      size_t off = 0;
      if (send_some(c->fd, pkt.data(), pkt.size(), &off) == SendResult::kError) {
        mark_dead(c);
        return;
      }
      if (off < pkt.size()) {
        c->outbuf.append(pkt.data() + off, pkt.size() - off);  // outbuf is empty here
        arm_epollout(c);
      } else if (c->closing) {
        mark_dead(c);
      }
      return;
    }
    c->outbuf.append(pkt);
  }

  // out_mu held
  void arm_epollout(Conn* c) {
    if (!c->epollout_armed) {
      c->epollout_armed = true;
      loops[c->io_idx]->mod_fd(c->fd, EPOLLIN | EPOLLOUT);
    }
  }

  // Marks the conn for closure; the owner loop performs the actual close.
  void mark_dead(Conn* c) {
    if (c->dead.exchange(true)) return;
    uint64_t cid = c->id;
    loops[c->io_idx]->post([this, cid] {
      ConnPtr cp = lookup(cid);
      if (cp) close_conn(cp.get());
    });
  }

  // end_drain: the owner loop finished a drain — move the staged replies
  // (and whatever other threads delivered meanwhile, at their recorded
  // positions) into outbuf under the one lock this flush takes anyway.
  void flush_out(Conn* c, bool end_drain = false) {
    bool close_now = false;
    {
      std::lock_guard<std::mutex> og(c->out_mu);
      if (end_drain) {
        c->draining = false;
        if (c->xq.empty()) {
          if (c->outbuf.empty())
            c->outbuf.swap(c->stage);  // steady state: buffers trade places, no copy
          else
            c->outbuf.append(c->stage, 0, c->stage.size());
        } else {
          size_t pos = 0;
          for (auto& x : c->xq) {
            size_t at = std::min(x.first, c->stage.size());
            if (at > pos) {
              c->outbuf.append(c->stage, pos, at - pos);
              pos = at;
            }
            c->outbuf.append(x.second);
          }
          c->outbuf.append(c->stage, pos, c->stage.size() - pos);
          c->xq.clear();
        }
        c->stage.clear();
        c->stage_pub.store(0, std::memory_order_relaxed);
      }
      size_t off = 0;
      close_now = send_some(c->fd, c->outbuf.data(), c->outbuf.size(), &off) == SendResult::kError;
      if (!close_now) {
        c->outbuf.erase_front(off);
        if (c->outbuf.empty()) {
          if (c->epollout_armed) {
            c->epollout_armed = false;
            loops[c->io_idx]->mod_fd(c->fd, EPOLLIN);
          }
          if (c->closing) close_now = true;
        } else {
          arm_epollout(c);
        }
      }
    }
    if (close_now) close_conn(c);
  }

  // MUST run on the owner loop thread.
  void close_conn(Conn* c) {
    if (c->carry) c->carry->release();  // closing mid-drain: nothing stays locked
    c->dead.store(true);
    {
      std::lock_guard<std::mutex> g(conns_mu);
      auto it = conns.find(c->id);
      if (it == conns.end()) return;  // already closed
      conns.erase(it);
    }
    if (c->session) {
      uint64_t expected = c->id;
      c->session->conn_id.compare_exchange_strong(expected, 0);
    }
    {
      // out_mu serializes against a cross-thread deliver() mid-write: the fd
      // must not be closed (and possibly reused) under a concurrent write
      std::lock_guard<std::mutex> og(c->out_mu);
      loops[c->io_idx]->del_fd(c->fd);
      ::close(c->fd);
      c->fd = -1;
    }
  }

  // queue a close on the conn's owner loop
  void post_close(const ConnPtr& c) {
    uint64_t cid = c->id;
    size_t srv = c->io_idx;
    loops[srv]->post([this, cid] {
      ConnPtr cp = lookup(cid);
      if (cp) close_conn(cp.get());
    });
  }

  // ---------------- quorum mode (see the header comment) ----------------

  enum class Stop { kNone, kQuorumLost, kLeaderLost };

  // admin_mu held
  size_t servers_up_locked() const {
    size_t up = 0;
    for (const auto& s : servers) up += s.up ? 1 : 0;
    return up;
  }

  // admin_mu held; quorum mode; server idx has just gone from up to down.
  // Says whether that ends service, and if so marks it ended.
  Stop server_went_down_locked(size_t idx) {
    size_t n = servers.size();
    size_t up = servers_up_locked();
    bool had = 2 * (up + 1) > n;
    bool has = 2 * up > n;
    if (had && !has) {
      not_serving.store(true, std::memory_order_release);
      has_leader = false;
      quorum_losses++;
      log.warn("quorum lost: serving nobody, expiring nobody",
               {{"servers_up", Json(static_cast<int64_t>(up))}, {"needed", Json(static_cast<int64_t>(n / 2 + 1))}});
      return Stop::kQuorumLost;
    }
    if (has && has_leader && idx == leader_idx) {
      not_serving.store(true, std::memory_order_release);
      has_leader = false;
      election_until = now_ms() + std::max(0, cfg.election_ms);
      log.info("leader lost: election started", {{"server", Json(static_cast<int64_t>(idx))}});
      return Stop::kLeaderLost;
    }
    return Stop::kNone;
  }

  // admin_mu held; quorum mode; server idx has just gone from down to up.
  // True if that regained the majority, which starts an election.
  bool server_came_up_locked() {
    size_t n = servers.size();
    size_t up = servers_up_locked();
    if (!(2 * up > n) || 2 * (up - 1) > n) return false;
    election_until = now_ms() + std::max(0, cfg.election_ms);
    log.info("quorum regained: election started", {{"servers_up", Json(static_cast<int64_t>(up))}});
    return true;
  }

  // Resume service if it is stopped and nothing stands against it any more;
  // otherwise the milliseconds left of the election pause, or 0 if there is
  // nothing to wait for (already serving, or no quorum).
  int64_t resume_serving() {
    std::lock_guard<std::mutex> g(admin_mu);
    if (!not_serving.load(std::memory_order_relaxed)) return 0;
    if (!(2 * servers_up_locked() > servers.size())) return 0;
    int64_t now = now_ms();
    if (now < election_until) return election_until - now;
    for (size_t i = 0; i < servers.size(); i++) {
      if (servers[i].up) {
        leader_idx = i;
        break;
      }
    }
    has_leader = true;
    size_t nsess = 0;
    {
      // the new leader gives every session a fresh timeout
      std::lock_guard<std::mutex> sg(session_mu);
      for (const auto& kv : sessions) kv.second->last_touch.store(now, std::memory_order_relaxed);
      nsess = sessions.size();
    }
    not_serving.store(false, std::memory_order_release);
    log.info("leader elected: serving again, session timers restarted",
             {{"leader", Json(static_cast<int64_t>(leader_idx))}, {"sessions", Json(static_cast<int64_t>(nsess))}});
    return 0;
  }

  // An election has begun (election_until is set): resume when it is over.
  void resume_after_election() {
    int64_t wait = resume_serving();
    if (wait > 0) loops[0]->schedule_from_any(wait, [this] { resume_after_election(); });
  }

  // Run an empty task on every IO loop and wait for it: whatever a loop was
  // in the middle of (an accept, a drain, the sweep) has finished.
  void loops_barrier() {
    std::vector<std::promise<void>> done(loops.size());
    for (size_t i = 0; i < loops.size(); i++) loops[i]->post([&done, i] { done[i].set_value(); });
    for (auto& d : done) d.get_future().wait();
  }

  // ---------------- control (any thread but the IO loops') ----------------

  void kill_server(size_t idx) {
    {
      std::lock_guard<std::mutex> g(admin_mu);
      if (idx >= servers.size()) return;
    }
    size_t lidx = idx % loops.size();
    std::promise<void> done;
    Stop stop = Stop::kNone;
    loops[lidx]->post([this, idx, lidx, &done, &stop] {
      {
        std::lock_guard<std::mutex> g(admin_mu);
        if (idx < servers.size() && servers[idx].up) {
          Server& s = servers[idx];
          loops[lidx]->del_fd(s.listen_fd);
          ::close(s.listen_fd);
          s.listen_fd = -1;
          s.up = false;
          if (cfg.quorum) stop = server_went_down_locked(idx);
        }
      }
      done.set_value();
    });
    done.get_future().wait();
    // quorum mode, service ended: every accept from now on is refused; wait
    // out the ones that were let in, so that they are among the victims
    if (stop != Stop::kNone) loops_barrier();
    // retire this server's connections (everybody's, if service ended) on
    // their own IO loops
    std::vector<ConnPtr> victims;
    {
      std::lock_guard<std::mutex> g(conns_mu);
      for (auto& kv : conns)
        if (stop != Stop::kNone || kv.second->server_idx == idx) victims.push_back(kv.second);
    }
    std::vector<std::promise<void>> vdone(victims.size());
    for (size_t i = 0; i < victims.size(); i++) {
      ConnPtr c = victims[i];
      c->dead.store(true);
      loops[c->io_idx]->post([this, c, &vdone, i] {
        close_conn(c.get());
        vdone[i].set_value();
      });
    }
    for (auto& d : vdone) d.get_future().wait();
    {
      std::lock_guard<std::mutex> g(admin_mu);
      dropped_conns += victims.size();
    }
    log.info("server killed", {{"server", Json(static_cast<int64_t>(idx))}});
    if (stop == Stop::kLeaderLost) resume_after_election();
  }

  void restart_server(size_t idx) {
    {
      std::lock_guard<std::mutex> g(admin_mu);
      if (idx >= servers.size()) return;
    }
    std::promise<void> done;
    bool regained = false;
    loops[idx % loops.size()]->post([this, idx, &done, &regained] {
      {
        std::lock_guard<std::mutex> g(admin_mu);
        if (idx < servers.size() && !servers[idx].up) {
          open_listener(idx, servers[idx].port);
          log.info("server restarted", {{"server", Json(static_cast<int64_t>(idx))}});
          if (cfg.quorum) regained = server_came_up_locked();
        }
      }
      done.set_value();
    });
    done.get_future().wait();
    if (regained) resume_after_election();
  }

  // admin_mu held
  void maybe_elect_leader_locked() {
    if (leader_idx < servers.size() && servers[leader_idx].up) return;
    for (size_t i = 0; i < servers.size(); i++) {
      if (servers[i].up) {
        leader_idx = i;
        log.info("leader elected", {{"leader", Json(static_cast<int64_t>(i))}});
        return;
      }
    }
  }

  size_t kill_leader() {
    size_t victim;
    {
      std::lock_guard<std::mutex> g(admin_mu);
      victim = leader_idx;
    }
    kill_server(victim);
    // quorum mode: kill_server has started the election itself, so that
    // kill_server(leader()) and kill_leader() are one thing
    if (cfg.quorum) return victim;
    std::lock_guard<std::mutex> g(admin_mu);
    if (cfg.election_ms > 0) election_until = now_ms() + cfg.election_ms;
    maybe_elect_leader_locked();
    return victim;
  }
};

// ---------------- public API ----------------

Ensemble::Ensemble(EnsembleConfig cfg) : impl_(std::make_unique<Impl>(std::move(cfg))) {}

Ensemble::~Ensemble() {
  try {
    stop();
  } catch (...) {
  }
}

void Ensemble::start() { impl_->start(); }
void Ensemble::stop() { impl_->stop(); }

std::vector<int> Ensemble::ports() const {
  std::lock_guard<std::mutex> g(impl_->admin_mu);
  std::vector<int> out;
  for (const auto& s : impl_->servers) out.push_back(s.port);
  return out;
}

std::string Ensemble::connect_string() const {
  std::string out;
  for (int p : ports()) {
    if (!out.empty()) out += ',';
    out += impl_->cfg.bind_host + ":" + std::to_string(p);
  }
  return out;
}

void Ensemble::kill_server(size_t idx) { impl_->kill_server(idx); }
void Ensemble::restart_server(size_t idx) { impl_->restart_server(idx); }

bool Ensemble::server_up(size_t idx) const {
  std::lock_guard<std::mutex> g(impl_->admin_mu);
  return idx < impl_->servers.size() && impl_->servers[idx].up;
}

size_t Ensemble::leader() const {
  std::lock_guard<std::mutex> g(impl_->admin_mu);
  return impl_->leader_idx;
}

size_t Ensemble::kill_leader() { return impl_->kill_leader(); }

void Ensemble::expire_session(int64_t session_id) { impl_->kill_session(session_id, /*close_conn_too=*/true); }

void Ensemble::set_latency_ms(int ms) { impl_->latency_ms.store(ms); }

bool Ensemble::has_quorum() const { return quorum_state().has_quorum; }

QuorumState Ensemble::quorum_state() const {
  QuorumState q;
  std::lock_guard<std::mutex> g(impl_->admin_mu);
  q.enabled = impl_->cfg.quorum;
  q.servers = impl_->servers.size();
  q.servers_up = impl_->servers_up_locked();
  q.needed = q.servers / 2 + 1;
  bool leader_up = impl_->leader_idx < q.servers && impl_->servers[impl_->leader_idx].up;
  if (q.enabled) {
    q.has_quorum = 2 * q.servers_up > q.servers;
    q.serving = !impl_->not_serving.load(std::memory_order_relaxed);
    q.leader = impl_->has_leader ? static_cast<int>(impl_->leader_idx) : -1;
  } else {
    q.has_quorum = q.servers_up > 0;
    q.serving = q.has_quorum && now_ms() >= impl_->election_until;
    q.leader = leader_up ? static_cast<int>(impl_->leader_idx) : -1;
  }
  q.losses = impl_->quorum_losses;
  q.refused_connects = impl_->refused_connects.load(std::memory_order_relaxed);
  q.dropped_connections = impl_->dropped_conns;
  return q;
}

NodeInfo Ensemble::get(const std::string& path) const {
  PathRef ref = ref_of(path);
  auto& sh = impl_->shard_of(ref);
  std::lock_guard<TreeLock> g(sh.mu);
  NodeInfo info;
  if (const auto* n = sh.nodes.find(ref)) {
    info.exists = true;
    info.data = n->data();
    info.stat = n->stat;
  }
  return info;
}

std::vector<std::string> Ensemble::children(const std::string& path) const {
  std::vector<std::string> out;
  PathRef ref = ref_of(path);
  auto& sh = impl_->shard_of(ref);
  std::lock_guard<TreeLock> g(sh.mu);
  if (const auto* n = sh.nodes.find(ref)) list_children(*n, &out);
  return out;
}

size_t Ensemble::node_count() const {
  size_t n = 0;
  for (auto& sh : impl_->shards) {
    std::lock_guard<TreeLock> g(sh.mu);
    n += sh.nodes.size();
  }
  return n - 1;  // exclude root
}

size_t Ensemble::ephemeral_count() const {
  std::vector<Impl::SessionPtr> snap;
  {
    std::lock_guard<std::mutex> g(impl_->session_mu);
    for (const auto& kv : impl_->sessions) snap.push_back(kv.second);
  }
  size_t n = 0;
  for (const auto& s : snap) {
    std::lock_guard<TreeLock> eg(s->eph_mu);
    n += s->eph_count;
  }
  return n;
}

std::vector<int64_t> Ensemble::session_ids() const {
  std::lock_guard<std::mutex> g(impl_->session_mu);
  std::vector<int64_t> out;
  for (const auto& kv : impl_->sessions) out.push_back(kv.first);
  return out;
}

int64_t Ensemble::zxid() const { return impl_->zxid_counter.load(); }

std::map<std::string, uint64_t> Ensemble::counters() const {
  std::map<std::string, uint64_t> out;
  constexpr auto rlx = std::memory_order_relaxed;
  for (size_t i = 0; i < impl_->n_ops; i++) {  // sum over the per-loop blocks
    const auto& o = impl_->ops[i];
    out["connect"] += o.connect.load(rlx);
    out["create"] += o.create.load(rlx);
    out["delete"] += o.del.load(rlx);
    out["exists"] += o.exists.load(rlx);
    out["getData"] += o.get_data.load(rlx);
    out["setData"] += o.set_data.load(rlx);
    out["getChildren"] += o.get_children.load(rlx);
    out["ping"] += o.ping.load(rlx);
    out["closeSession"] += o.close_session.load(rlx);
    out["unknown"] += o.unknown.load(rlx);
    out["tree_locks"] += o.tree_locks.load(rlx);
  }
  for (auto it = out.begin(); it != out.end();) {
    if (it->second == 0)
      it = out.erase(it);
    else
      ++it;
  }
  uint64_t cached = 0;
  for (auto& sh : impl_->shards) {
    std::lock_guard<TreeLock> g(sh.mu);
    cached += sh.nodes.cached;
  }
  out["node_blocks_cached"] = cached;
  return out;
}

std::vector<std::string> Ensemble::audit() const { return impl_->audit(); }

NodeStoreLayout Ensemble::node_store_layout() {
  NodeStoreLayout l;
  l.shards = Impl::kShards;
  l.header_bytes = sizeof(ZNode);
  l.max_cached_per_class = kMaxCachedPerClass;
  l.classes.assign(std::begin(kBlockClasses), std::end(kBlockClasses));
  return l;
}

}  // namespace zk
}  // namespace registrar
