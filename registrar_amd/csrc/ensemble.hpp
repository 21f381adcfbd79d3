// ensemble.hpp — synthetic in-process ZooKeeper ensemble.
//
// The reference's tests require a real ZooKeeper on localhost
// (test/helper.js:57-62 in the reference). This build instead
// ships a from-scratch in-process ensemble that speaks the real jute wire
// protocol over TCP (so the native client, or any ZK client, can talk to
// it), with:
//   - a shared data tree across N "servers" (1- and 3-node modes),
//   - real session semantics: negotiation, touch-on-request, expiry sweep,
//     ephemeral-node deletion on expiry/close, reconnect-with-same-session,
//   - leader-kill with an optional election pause (storm testing,
//     BASELINE.json config 4),
//   - an optional quorum mode: no service, and no session expiry, below a
//     majority of servers,
//   - per-response latency injection,
//   - one-shot data/child watches (Binder-style readers).
//
// Threading: an IO-loop pool (like ZooKeeper's selector threads) with
// connections assigned round-robin, over 64-way sharded tree/watch state —
// see ensemble.cpp's header comment for the full model and lock order. The
// control/introspection API is thread-safe.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "jute.hpp"
#include "log.hpp"
#include "loop.hpp"

namespace registrar {
namespace zk {

struct EnsembleConfig {
  std::vector<int> ports{0};        // 0 = auto-assign; one entry per server
  std::string bind_host = "127.0.0.1";
  int tick_ms = 100;                // expiry sweep granularity
  int min_session_timeout_ms = 400;  // negotiated floor (2*tick in real ZK)
  int max_session_timeout_ms = 60000;
  int latency_ms = 0;               // fixed artificial delay per response
  int election_ms = 0;              // pause after leader kill before failover serves
  // IO loop threads (0 = auto). Like real ZooKeeper's selector threads, IO
  // parallelism is independent of ensemble size: connections are assigned
  // round-robin across the pool regardless of which server accepted them.
  int io_threads = 0;
  // Quorum mode (off by default): below a majority of servers the ensemble
  // serves nobody and expires nobody; see "Quorum mode" in ensemble.cpp.
  bool quorum = false;
  LogLevel log_level = LogLevel::Warn;
};

struct NodeInfo {  // introspection result
  bool exists = false;
  std::string data;
  Stat stat;
};

// Geometry of the node store (see ensemble.cpp): a znode is one block of
// header + path + data, blocks come in size classes and each shard keeps at
// most max_cached_per_class released blocks per class for reuse.
struct NodeStoreLayout {
  size_t shards = 0;
  size_t header_bytes = 0;
  size_t max_cached_per_class = 0;
  std::vector<size_t> classes;  // block sizes, ascending; larger blocks are never cached
};

// Quorum introspection (Ensemble::quorum_state). With the mode off the
// ensemble "has quorum" while any server is up.
struct QuorumState {
  bool enabled = false;
  size_t servers = 0;
  size_t servers_up = 0;
  size_t needed = 0;      // servers / 2 + 1
  bool has_quorum = false;
  bool serving = false;   // has quorum and no election pause is running
  int leader = -1;        // index, or -1 while there is none
  uint64_t losses = 0;    // times quorum was lost
  // connections closed at accept or handshake because the ensemble was not
  // serving (an election pause, or no quorum)
  uint64_t refused_connects = 0;
  // connections closed by kill_server / kill_leader, whether they were the
  // killed server's own or everybody's (quorum or leader lost)
  uint64_t dropped_connections = 0;
};

class Ensemble {
 public:
  explicit Ensemble(EnsembleConfig cfg);
  ~Ensemble();

  Ensemble(const Ensemble&) = delete;
  Ensemble& operator=(const Ensemble&) = delete;

  void start();
  void stop();

  // Bound ports after start() (auto-assigned resolved).
  std::vector<int> ports() const;
  std::string connect_string() const;  // "host:port,host:port,..."

  // --- fault injection / control (thread-safe) ---
  // close listener + connections; sessions persist. In quorum mode, losing
  // the majority or the leader drops every server's connections before this
  // returns (call it from outside the IO loops, like all of this block).
  void kill_server(size_t idx);
  void restart_server(size_t idx);   // re-listen on the same port
  bool server_up(size_t idx) const;
  size_t leader() const;
  // Kill the current leader; remaining servers refuse connects for
  // election_ms, then one becomes leader. Returns the killed index.
  size_t kill_leader();
  void expire_session(int64_t session_id);  // force-expire (ephemerals vanish)
  void set_latency_ms(int ms);

  // --- introspection (thread-safe) ---
  NodeInfo get(const std::string& path) const;
  std::vector<std::string> children(const std::string& path) const;
  size_t node_count() const;             // all znodes (excl. root)
  size_t ephemeral_count() const;
  std::vector<int64_t> session_ids() const;
  int64_t zxid() const;
  // cumulative request counters by opcode name ("create", "exists", ...),
  // zero ones left out; plus "node_blocks_cached", the number of released
  // node blocks the shards currently hold for reuse (always present)
  std::map<std::string, uint64_t> counters() const;
  bool has_quorum() const;
  QuorumState quorum_state() const;
  static NodeStoreLayout node_store_layout();
  // Structural audit of the whole tree (parent/sibling links, counts, data
  // placement, hashes and buckets, ephemeral ownership against the sessions,
  // free lists): one human-readable line per violation, empty when sound.
  // Takes every shard lock; for tests and the stress driver, never for a
  // request path. Call it only while no session expiry is in flight.
  std::vector<std::string> audit() const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace zk
}  // namespace registrar
