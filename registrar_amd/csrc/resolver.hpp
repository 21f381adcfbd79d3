// resolver.hpp — a watch-maintained view of registration domains: the consumer
// side of the discovery triangle (what the real Binder's ZooKeeper cache does).
//
// One Resolver owns one ZkClient, so one session, and any number of domain
// views. A view holds the domain's service record and its host records, is
// built with one getData, one getChildren and one pipelined get_many, and is
// kept current by one-shot watches from then on. Readers take consistent
// copies (snapshot) under one mutex and never touch the network.
//
// Per domain the state machine is (docs/architecture.md, "Resolver"):
//
//   (none) --lookup/watch: exists--> building --pass done--> synced
//   synced --watch event--> dirty --pass--> synced          (one pass at a time)
//   synced --Disconnected--> stale --Connected + pass--> synced
//   any    --domain node gone--> dropped (not cached, no watch left behind)
//
// A watch event never reads anything itself: it marks what changed (service
// record, child list, one child) and starts a pass unless one runs. A pass
// takes the marks it finds and clears them; events that arrive meanwhile set
// new marks, and the end of the pass starts the next one. So no event is lost
// and no two passes of one domain overlap.
//
// Everything network-side runs on the client's loop thread through the async
// verbs; no callback calls a sync verb or close(). A session expiry is
// recovered on a thread of the resolver's own, which opens a fresh client and
// re-reads every viewed domain, emitting events for real differences only.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "log.hpp"
#include "zkclient.hpp"

namespace registrar {

struct ResolverConfig {
  zk::ZkClientConfig client;  // queue_watches is turned off by the resolver
  // hosts whose address equals this are flagged local ("same node": the
  // payload carries no hive id, so this is all "xGMI-local" can honestly mean)
  std::string local_address;
  // views kept at most; a lookup of a further domain is answered by a direct,
  // un-cached and un-watched read through the same code. Nothing is evicted.
  size_t max_domains = 1024;
};

struct ResolvedService {
  bool present = false;
  std::string json;  // the inner service object ({"srvce","proto","port","ttl"}), as JSON text
  bool has_port = false;
  int64_t port = 0;
  bool has_ttl = false;
  int64_t ttl = 0;
};

struct ResolvedHost {
  std::string name;
  bool has_address = false;
  std::string address;
  bool has_ttl = false;
  int64_t ttl = 0;             // as stored in the host record
  std::vector<int64_t> ports;  // the record's own, else the service record's port
  std::string type;
  std::string gpu_json;  // the typed sub-object's "gpu" block as JSON text; empty = none
  int64_t ephemeral_owner = 0;
  int64_t mzxid = 0;
  std::string payload;  // raw znode data
  bool local = false;
};

struct ResolverSnapshot {
  bool exists = false;  // a view of the domain is held
  bool synced = false;  // its first pass completed
  bool stale = false;   // disconnected since the last completed pass
  uint64_t generation = 0;
  ResolvedService service;
  std::vector<ResolvedHost> hosts;  // by name (local ones first with local_first)
};

struct ResolverEvent {
  // synced | added | removed | changed | service | stale | fresh | dropped
  std::string type;
  std::string domain;
  std::string name;  // the host, for added / removed / changed
  uint64_t generation = 0;
};

struct ResolverStats {
  uint64_t passes = 0;
  uint64_t events_applied = 0;
  uint64_t direct_reads = 0;
  uint64_t resyncs_after_expiry = 0;
};

enum class LookupStatus { Ok, Absent, Unavailable };

class Resolver {
 public:
  Resolver(ResolverConfig cfg, Logger log);
  ~Resolver();
  Resolver(const Resolver&) = delete;
  Resolver& operator=(const Resolver&) = delete;

  void start();  // non-blocking: begins connecting
  void stop();

  // Start a view on first use and block until it is synced. Absent: the domain
  // node does not exist (nothing is cached, no watch is armed). Unavailable:
  // timeout, or disconnected with no view yet. Never a half-filled view.
  LookupStatus lookup(const std::string& domain, int64_t timeout_ms, ResolverSnapshot* out,
                      bool local_first = false);
  // Start a view without waiting for it.
  void watch(const std::string& domain);
  ResolverSnapshot snapshot(const std::string& domain, bool local_first = false) const;
  std::vector<std::string> domains() const;
  std::vector<ResolverEvent> poll_events();
  int64_t session_id() const;
  bool connected() const;
  ResolverStats stats() const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace registrar
