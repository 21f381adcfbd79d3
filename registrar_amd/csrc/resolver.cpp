// resolver.cpp — see resolver.hpp.
#include "resolver.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <set>
#include <thread>

#include "json.hpp"
#include "registrar.hpp"

namespace registrar {

namespace {

// the event queue is for observers; one that never polls must not grow it
// without bound, so the oldest entries go first past this many
constexpr size_t kMaxQueuedEvents = 65536;

struct View {
  std::string domain;
  std::string path;
  bool watch = true;  // false: a direct read past the view limit (never in the map)
  bool synced = false;
  bool stale = false;
  bool dropped = false;
  uint64_t generation = 0;
  std::string service_raw;
  ResolvedService service;
  std::map<std::string, ResolvedHost> hosts;  // ports: the record's own only; the fallback is copy()'s
  std::set<std::string> listed;  // the last child list, skipped names included
  // marks left by events (and failed passes) for the next pass
  bool dirty_svc = true;
  bool dirty_list = true;
  bool dirty_full = false;  // re-get every listed child (a fresh session has no watches)
  std::set<std::string> dirty_children;
  bool running = false;
};
using ViewPtr = std::shared_ptr<View>;

// what one pass took from the view's marks
struct Pass {
  bool svc = false;
  bool list = false;
  bool full = false;
  std::set<std::string> children;
  std::vector<std::string> names;  // the get_many in flight
};
using PassPtr = std::shared_ptr<Pass>;

struct Probe {
  bool done = false;
  int rc = zk::kZConnectionLoss;
};

// The one parser of a service record (the direct binder path's rules: the
// record's type must be "service"; anything malformed means "no service").
ResolvedService parse_service(const std::string& data) {
  ResolvedService s;
  if (data.empty()) return s;
  try {
    Json rec = Json::parse(data);
    if (!rec.is_object() || rec.get_string("type", "") != "service") return s;
    const Json& inner = rec.get("service").get("service");
    if (!inner.is_object()) return s;
    s.present = true;
    s.json = inner.dump();
    const Json& port = inner.get("port");
    if (port.is_number()) {
      s.has_port = true;
      s.port = port.as_int();
    }
    const Json& ttl = inner.get("ttl");
    if (ttl.is_number()) {
      s.has_ttl = true;
      s.ttl = ttl.as_int();
    }
  } catch (const std::exception&) {
    return ResolvedService{};
  }
  return s;
}

// The one parser of a host record. False: not a host record (empty, not JSON,
// not an object, or a nested domain's service record) and so skipped.
bool parse_host(const std::string& name, const std::string& data, const zk::Stat& st, ResolvedHost* out) {
  if (data.empty()) return false;
  try {
    Json rec = Json::parse(data);
    if (!rec.is_object()) return false;
    std::string type = rec.get_string("type", "");
    if (type == "service") return false;
    ResolvedHost h;
    h.name = name;
    h.type = type;
    const Json& addr = rec.get("address");
    if (addr.is_string()) {
      h.has_address = true;
      h.address = addr.as_string();
    }
    const Json& ttl = rec.get("ttl");
    if (ttl.is_number()) {
      h.has_ttl = true;
      h.ttl = ttl.as_int();
    }
    const Json& typed = rec.get(type);
    if (typed.is_object()) {
      const Json& ports = typed.get("ports");
      if (ports.is_array())
        for (const auto& p : ports.items())
          if (p.is_number()) h.ports.push_back(p.as_int());
      const Json& gpu = typed.get("gpu");
      if (gpu.is_object()) h.gpu_json = gpu.dump();
    }
    h.ephemeral_owner = st.ephemeral_owner;
    h.mzxid = st.mzxid;
    h.payload = data;
    *out = std::move(h);
    return true;
  } catch (const std::exception&) {
    return false;
  }
}

}  // namespace

struct Resolver::Impl {
  ResolverConfig cfg;
  Logger log;

  mutable std::mutex mu;
  std::condition_variable cv;
  std::shared_ptr<zk::ZkClient> client;  // replaced after an expiry
  uint64_t epoch = 0;                    // callbacks of an earlier client are ignored
  bool started = false;
  bool stopping = false;
  bool connected = false;
  bool reopen = false;         // the session expired: the recovery thread opens a new client
  bool after_expiry = false;   // the next Connected is a fresh session: full re-read
  int64_t session = 0;
  std::map<std::string, ViewPtr> views;    // by domain
  std::map<std::string, ViewPtr> by_path;  // the same views by znode path
  std::set<std::string> wanted;  // watch() of domains not probed yet
  std::deque<ResolverEvent> events;
  ResolverStats stats;
  std::thread recovery;

  Impl(ResolverConfig c, Logger l) : cfg(std::move(c)), log(l.child("resolver")) {
    cfg.client.queue_watches = false;
  }

  // ---------------- helpers (mu held) ----------------

  void emit(const View& v, const char* type, const std::string& name) {
    if (!v.watch) return;
    if (events.size() >= kMaxQueuedEvents) events.pop_front();
    events.push_back({type, v.domain, name, v.generation});
  }

  // one applied change to a synced view
  void applied(View& v, const char* type, const std::string& name) {
    if (!v.synced) return;  // the first build shows as one "synced"
    v.generation++;
    stats.events_applied++;
    emit(v, type, name);
  }

  void remove_host(View& v, const std::string& name) {
    auto it = v.hosts.find(name);
    if (it == v.hosts.end()) return;
    v.hosts.erase(it);
    applied(v, "removed", name);
  }

  void drop(const ViewPtr& v) {
    if (v->dropped) return;
    v->dropped = true;
    v->running = false;
    auto it = views.find(v->domain);
    if (it != views.end() && it->second == v) {
      views.erase(it);
      by_path.erase(v->path);
    }
    if (v->synced) {
      v->generation++;
      emit(*v, "dropped", "");
    }
    cv.notify_all();
  }

  void open_client() {
    epoch++;
    uint64_t ep = epoch;
    auto c = std::make_shared<zk::ZkClient>(cfg.client, log);
    c->set_event_callback([this, ep](const zk::SessionEvent& ev) { on_session(ep, ev); });
    c->set_watch_callback([this, ep](const zk::WatcherEvent& ev) { on_watch(ep, ev); });
    client = c;
    c->start();
  }

  ViewPtr make_view(const std::string& domain, bool watch) {
    auto v = std::make_shared<View>();
    v->domain = domain;
    v->path = domain_to_path(domain);
    v->watch = watch;
    return v;
  }

  // ---------------- session and watch events (loop thread) ----------------

  void on_session(uint64_t ep, const zk::SessionEvent& ev) {
    std::lock_guard<std::mutex> g(mu);
    if (ep != epoch || stopping) return;
    switch (ev.type) {
      case zk::SessionEvent::Type::Connected: {
        connected = true;
        session = ev.session_id;
        bool full = after_expiry;
        if (after_expiry) {
          after_expiry = false;
          stats.resyncs_after_expiry++;
        }
        // The service record and the child list are read again (two requests
        // per domain): they are queued behind setWatches, so the events the
        // server synthesizes for what was missed arrive first, mark their
        // children, and "fresh" is reported only once those are applied. A
        // fresh session has no watches at all and re-reads every child.
        for (auto& kv : views) {
          View& v = *kv.second;
          v.dirty_svc = v.dirty_list = true;
          if (full) v.dirty_full = true;
          start_pass(kv.second);
        }
        std::set<std::string> w;
        w.swap(wanted);
        for (const auto& d : w) probe(d, nullptr);
        break;
      }
      case zk::SessionEvent::Type::Disconnected:
        connected = false;
        mark_stale();
        break;
      case zk::SessionEvent::Type::Expired:
        connected = false;
        mark_stale();
        reopen = true;
        break;
      default:
        break;
    }
    cv.notify_all();
  }

  void mark_stale() {
    for (auto& kv : views) {
      View& v = *kv.second;
      if (v.synced && !v.stale) {
        v.stale = true;
        emit(v, "stale", "");
      }
    }
  }

  void on_watch(uint64_t ep, const zk::WatcherEvent& ev) {
    std::lock_guard<std::mutex> g(mu);
    if (ep != epoch || stopping) return;
    // one path can be a domain of its own and a child of its parent domain's
    // view at once (nested domains), and the server sends one event for both
    if (ViewPtr v = path_view(ev.path)) {
      if (ev.type == zk::kEventNodeChildrenChanged) {
        v->dirty_list = true;
      } else {
        // changed, or deleted (the re-read then finds no node and drops the view)
        v->dirty_svc = true;
        if (ev.type == zk::kEventNodeDeleted) v->dirty_list = true;
      }
      start_pass(v);
    }
    if (ev.type == zk::kEventNodeChildrenChanged) return;
    size_t slash = ev.path.rfind('/');
    if (slash == std::string::npos || slash == 0) return;
    if (ViewPtr v = path_view(ev.path.substr(0, slash))) {
      // changed or deleted alike: the re-get tells which, in order with every
      // other reply of this session
      v->dirty_children.insert(ev.path.substr(slash + 1));
      start_pass(v);
    }
  }

  ViewPtr path_view(const std::string& path) {
    auto it = by_path.find(path);
    return it == by_path.end() ? nullptr : it->second;
  }

  // ---------------- a pass (steps chained on the loop thread) ----------------

  void start_pass(const ViewPtr& v) {
    if (v->running || v->dropped || !connected) return;
    if (!v->dirty_svc && !v->dirty_list && !v->dirty_full && v->dirty_children.empty()) return;
    v->running = true;
    stats.passes++;
    auto p = std::make_shared<Pass>();
    p->svc = v->dirty_svc;
    p->list = v->dirty_list || v->dirty_full;
    p->full = v->dirty_full;
    p->children.swap(v->dirty_children);
    v->dirty_svc = v->dirty_list = v->dirty_full = false;
    step_service(v, p);
  }

  // the pass could not finish (connection or session lost): its marks go back
  // and the next Connected runs it again
  void fail_pass(const ViewPtr& v, const PassPtr& p) {
    v->dirty_svc |= p->svc;
    v->dirty_list |= p->list;
    v->dirty_full |= p->full;
    v->dirty_children.insert(p->children.begin(), p->children.end());
    v->dirty_children.insert(p->names.begin(), p->names.end());
    v->running = false;
    cv.notify_all();
  }

  void step_service(const ViewPtr& v, const PassPtr& p) {
    if (!p->svc) return step_list(v, p);
    uint64_t ep = epoch;
    client->aget(v->path, v->watch, [this, ep, v, p](int rc, const std::string& data, const zk::Stat&) {
      std::lock_guard<std::mutex> g(mu);
      if (ep != epoch || v->dropped) return;
      if (rc == zk::kZNoNode) return drop(v);
      if (rc != zk::kZOk) return fail_pass(v, p);
      if (data != v->service_raw || !v->synced) {
        bool differs = data != v->service_raw;
        v->service_raw = data;
        v->service = parse_service(data);
        if (differs) applied(*v, "service", "");
      }
      step_list(v, p);
    });
  }

  void step_list(const ViewPtr& v, const PassPtr& p) {
    if (!p->list) return step_fetch(v, p);
    uint64_t ep = epoch;
    client->achildren(v->path, v->watch, [this, ep, v, p](int rc, const std::vector<std::string>& children) {
      std::lock_guard<std::mutex> g(mu);
      if (ep != epoch || v->dropped) return;
      if (rc == zk::kZNoNode) return drop(v);
      if (rc != zk::kZOk) return fail_pass(v, p);
      std::set<std::string> now(children.begin(), children.end());
      for (auto it = v->listed.begin(); it != v->listed.end();) {
        if (!now.count(*it)) {
          remove_host(*v, *it);
          it = v->listed.erase(it);
        } else {
          ++it;
        }
      }
      for (const auto& name : now)
        if (v->listed.insert(name).second) p->children.insert(name);
      step_fetch(v, p);
    });
  }

  void step_fetch(const ViewPtr& v, const PassPtr& p) {
    p->names.clear();
    if (p->full) {
      p->names.assign(v->listed.begin(), v->listed.end());
    } else {
      for (const auto& name : p->children)
        if (v->listed.count(name)) p->names.push_back(name);
    }
    p->children.clear();
    if (p->names.empty()) return finish_pass(v);
    std::vector<std::string> paths;
    paths.reserve(p->names.size());
    for (const auto& name : p->names) paths.push_back(v->path + "/" + name);
    uint64_t ep = epoch;
    client->aget_many(std::move(paths), v->watch,
                      [this, ep, v, p](std::vector<int>& rcs, std::vector<std::string>& datas,
                                       std::vector<zk::Stat>& stats_) {
                        std::lock_guard<std::mutex> g(mu);
                        if (ep != epoch || v->dropped) return;
                        for (int rc : rcs)
                          if (rc != zk::kZOk && rc != zk::kZNoNode) return fail_pass(v, p);
                        for (size_t i = 0; i < rcs.size(); i++) apply_child(*v, p->names[i], rcs[i], datas[i], stats_[i]);
                        p->names.clear();
                        finish_pass(v);
                      });
  }

  void apply_child(View& v, const std::string& name, int rc, std::string& data, const zk::Stat& st) {
    if (rc == zk::kZNoNode) {
      // listed a moment ago, gone now: normal. Off the list too, so that a
      // node of the same name created later counts as new in the next listing
      // (no watch was armed by this reply).
      remove_host(v, name);
      v.listed.erase(name);
      return;
    }
    ResolvedHost h;
    if (!parse_host(name, data, st, &h)) {
      remove_host(v, name);  // stays listed: its data watch is armed
      return;
    }
    h.local = !cfg.local_address.empty() && h.has_address && h.address == cfg.local_address;
    auto it = v.hosts.find(name);
    if (it == v.hosts.end()) {
      v.hosts[name] = std::move(h);
      applied(v, "added", name);
    } else if (it->second.payload == h.payload) {
      // the same bytes (a re-read after a reconnect or an expiry, or a record
      // written again unchanged): no event
      it->second.ephemeral_owner = h.ephemeral_owner;
      it->second.mzxid = h.mzxid;
    } else {
      it->second = std::move(h);
      applied(v, "changed", name);
    }
  }

  void finish_pass(const ViewPtr& v) {
    v->running = false;
    if (!v->synced) {
      v->synced = true;
      v->generation++;
      emit(*v, "synced", "");
    }
    bool more = v->dirty_svc || v->dirty_list || v->dirty_full || !v->dirty_children.empty();
    if (more && v->watch) {
      start_pass(v);
    } else if (v->stale && connected) {
      v->stale = false;
      emit(*v, "fresh", "");
    }
    cv.notify_all();
  }

  // ---------------- starting a view ----------------

  // One un-watched exists decides whether the domain gets a view at all.
  void probe(const std::string& domain, std::shared_ptr<Probe> pr) {
    uint64_t ep = epoch;
    client->aexists(domain_to_path(domain), false, [this, ep, domain, pr](int rc, const zk::Stat&) {
      std::lock_guard<std::mutex> g(mu);
      if (ep != epoch) return;
      if (rc == zk::kZOk && !views.count(domain) && views.size() < cfg.max_domains) {
        ViewPtr v = make_view(domain, true);
        views[domain] = v;
        by_path[v->path] = v;
        start_pass(v);
      }
      if (pr) {
        pr->rc = rc;
        pr->done = true;
      }
      cv.notify_all();
    });
  }

  ResolverSnapshot copy(const View& v, bool local_first) const {
    ResolverSnapshot s;
    s.exists = !v.dropped;
    s.synced = v.synced;
    s.stale = v.stale;
    s.generation = v.generation;
    s.service = v.service;
    s.hosts.reserve(v.hosts.size());
    for (const auto& kv : v.hosts) {
      s.hosts.push_back(kv.second);
      ResolvedHost& h = s.hosts.back();
      if (h.ports.empty() && v.service.present && v.service.has_port) h.ports.push_back(v.service.port);
    }
    if (local_first)
      std::stable_partition(s.hosts.begin(), s.hosts.end(), [](const ResolvedHost& h) { return h.local; });
    return s;
  }

  void recovery_loop() {
    std::unique_lock<std::mutex> g(mu);
    while (true) {
      cv.wait(g, [this] { return stopping || reopen; });
      if (stopping) return;
      reopen = false;
      std::shared_ptr<zk::ZkClient> old = client;
      // whatever the old client still had in flight will never be answered to
      // this epoch: its passes count as failed
      epoch++;
      for (auto& kv : views) {
        View& v = *kv.second;
        v.running = false;
        v.dirty_svc = v.dirty_list = v.dirty_full = true;
      }
      after_expiry = true;
      g.unlock();
      old->close();  // joins its loop thread: never under mu
      g.lock();
      if (stopping) return;
      open_client();
    }
  }
};

Resolver::Resolver(ResolverConfig cfg, Logger log) : impl_(std::make_unique<Impl>(std::move(cfg), log)) {
  if (impl_->cfg.client.servers.empty()) throw std::runtime_error("Resolver: options.servers empty");
}

Resolver::~Resolver() {
  try {
    stop();
  } catch (...) {
  }
}

void Resolver::start() {
  std::lock_guard<std::mutex> g(impl_->mu);
  if (impl_->started) return;
  impl_->started = true;
  impl_->stopping = false;
  impl_->open_client();
  impl_->recovery = std::thread([this] { impl_->recovery_loop(); });
}

void Resolver::stop() {
  std::shared_ptr<zk::ZkClient> c;
  {
    std::lock_guard<std::mutex> g(impl_->mu);
    if (!impl_->started || impl_->stopping) return;
    impl_->stopping = true;
    impl_->cv.notify_all();
  }
  if (impl_->recovery.joinable()) impl_->recovery.join();
  {
    std::lock_guard<std::mutex> g(impl_->mu);
    c = impl_->client;
  }
  if (c) c->close();
  std::lock_guard<std::mutex> g(impl_->mu);
  impl_->client.reset();
  impl_->connected = false;
  impl_->started = false;
  impl_->cv.notify_all();
}

LookupStatus Resolver::lookup(const std::string& domain, int64_t timeout_ms, ResolverSnapshot* out,
                              bool local_first) {
  Impl& m = *impl_;
  auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms < 0 ? 0 : timeout_ms);
  std::unique_lock<std::mutex> g(m.mu);
  if (out) *out = ResolverSnapshot{};
  if (!m.started || m.stopping) return LookupStatus::Unavailable;
  ViewPtr v;
  auto it = m.views.find(domain);
  if (it != m.views.end()) v = it->second;
  if (!v) {
    if (!m.cv.wait_until(g, deadline, [&] { return m.connected || m.stopping; }) || m.stopping)
      return LookupStatus::Unavailable;
    auto pr = std::make_shared<Probe>();
    m.probe(domain, pr);
    if (!m.cv.wait_until(g, deadline, [&] { return pr->done || m.stopping; }) || m.stopping)
      return LookupStatus::Unavailable;
    if (pr->rc == zk::kZNoNode) return LookupStatus::Absent;
    if (pr->rc != zk::kZOk) return LookupStatus::Unavailable;
    it = m.views.find(domain);
    if (it != m.views.end()) {
      v = it->second;
    } else {
      // past the view limit: the same pass, on a view nobody keeps or watches
      if (!m.connected) return LookupStatus::Unavailable;
      v = m.make_view(domain, false);
      m.stats.direct_reads++;
      m.start_pass(v);
    }
  }
  bool done = m.cv.wait_until(g, deadline, [&] { return v->synced || v->dropped || m.stopping; });
  if (v->dropped) return LookupStatus::Absent;
  if (!done || !v->synced) return LookupStatus::Unavailable;
  if (out) *out = m.copy(*v, local_first);
  return LookupStatus::Ok;
}

void Resolver::watch(const std::string& domain) {
  Impl& m = *impl_;
  std::lock_guard<std::mutex> g(m.mu);
  if (!m.started || m.stopping || m.views.count(domain)) return;
  if (m.connected)
    m.probe(domain, nullptr);
  else
    m.wanted.insert(domain);
}

ResolverSnapshot Resolver::snapshot(const std::string& domain, bool local_first) const {
  std::lock_guard<std::mutex> g(impl_->mu);
  auto it = impl_->views.find(domain);
  if (it == impl_->views.end()) return ResolverSnapshot{};
  return impl_->copy(*it->second, local_first);
}

std::vector<std::string> Resolver::domains() const {
  std::lock_guard<std::mutex> g(impl_->mu);
  std::vector<std::string> out;
  for (const auto& kv : impl_->views) out.push_back(kv.first);
  return out;
}

std::vector<ResolverEvent> Resolver::poll_events() {
  std::lock_guard<std::mutex> g(impl_->mu);
  std::vector<ResolverEvent> out(impl_->events.begin(), impl_->events.end());
  impl_->events.clear();
  return out;
}

int64_t Resolver::session_id() const {
  std::lock_guard<std::mutex> g(impl_->mu);
  return impl_->session;
}

bool Resolver::connected() const {
  std::lock_guard<std::mutex> g(impl_->mu);
  return impl_->connected;
}

ResolverStats Resolver::stats() const {
  std::lock_guard<std::mutex> g(impl_->mu);
  return impl_->stats;
}

}  // namespace registrar
