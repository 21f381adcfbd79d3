// node_store.hpp — the ensemble's znode storage: path keys, the one-block
// ZNode, a shard's intrusive hash table with its recycled blocks, and the
// pointer links between nodes (children of a parent, ephemerals of a session).
//
// Nothing in this header takes a lock or starts a thread. Every structure
// here is guarded by a lock its user holds; which one is stated at each
// field. ensemble.cpp is that user (its Shard owns a NodeStore and the shard
// lock; Session::eph_mu is declared here next to the list it guards). The
// type of those two locks, TreeLock, is defined here as well.
#pragma once

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <string_view>
#include <vector>

#include "jute.hpp"

namespace registrar {
namespace zk {
namespace detail {

// The lock of a shard (Shard::mu) and of a session's ephemeral list
// (Session::eph_mu): the two a request handler takes, thousands of times per
// drain and nearly always uncontended. It is the classic three-state futex
// mutex. One word: 0 free, 1 held, 2 held and somebody may be asleep on it.
// try_lock is one acquire compare-and-swap and unlock one release exchange,
// both inline; only a lock() that finds the word taken leaves the line, and
// only an unlock() that finds 2 enters the kernel.
// No wake-up is lost: a thread sleeps only after it has itself written 2, and
// FUTEX_WAIT returns at once unless the word still is 2; the unlock that
// follows reads that 2 in its exchange and wakes one sleeper. A woken thread
// takes the lock as 2 again, since others may still be asleep.
// BasicLockable and Lockable, so std::lock_guard and std::unique_lock work.
// Not recursive, no timed waits. Every other mutex here stays std::mutex.
class TreeLock {
 public:
  TreeLock() = default;
  TreeLock(const TreeLock&) = delete;
  TreeLock& operator=(const TreeLock&) = delete;

  bool try_lock() noexcept {
    uint32_t expect = kFree;
    return word_.compare_exchange_strong(expect, kHeld, std::memory_order_acquire, std::memory_order_relaxed);
  }
  void lock() noexcept {
    if (!try_lock()) lock_slow();
  }
  void unlock() noexcept {
    if (word_.exchange(kFree, std::memory_order_release) == kSleepers) wake_one();
  }

 private:
  static constexpr uint32_t kFree = 0, kHeld = 1, kSleepers = 2;
  static_assert(std::atomic<uint32_t>::is_always_lock_free && sizeof(std::atomic<uint32_t>) == sizeof(uint32_t),
                "the futex word is the atomic itself");

  long futex(int op, uint32_t val) noexcept {
    return syscall(SYS_futex, reinterpret_cast<uint32_t*>(&word_), op, val, nullptr, nullptr, 0);
  }
  __attribute__((noinline, cold)) void lock_slow() noexcept {
    // a holder keeps the lock for a request or a short run of them: look
    // again a few times before paying for a sleep and a wake-up
    for (int i = 0; i < 64; i++) {
#if defined(__x86_64__) || defined(__i386__)
      __builtin_ia32_pause();
#endif
      if (word_.load(std::memory_order_relaxed) == kFree && try_lock()) return;
    }
    while (word_.exchange(kSleepers, std::memory_order_acquire) != kFree) futex(FUTEX_WAIT_PRIVATE, kSleepers);
  }
  __attribute__((noinline, cold)) void wake_one() noexcept { futex(FUTEX_WAKE_PRIVATE, 1); }

  std::atomic<uint32_t> word_{kFree};
};

// Parent of a path as a view of the same bytes ("/" for depth-1 paths). The
// basename is short, so the last '/' is found by walking back from the end.
inline std::string_view parent_view(std::string_view p) {
  size_t pos = p.size();
  while (pos > 0 && p[pos - 1] != '/') pos--;
  if (pos <= 1) return "/";  // no '/' at all, or only the leading one
  return p.substr(0, pos - 1);
}

// One pass over a path: true when it is not empty, starts with '/', does not
// end in '/' unless it is "/" itself, and holds no "//". *last_slash is then
// the index of its last '/', which is all parent_of needs.
inline bool scan_path(std::string_view p, size_t* last_slash) {
  const size_t n = p.size();
  if (n == 0 || p[0] != '/') return false;
  size_t last = 0;
  for (size_t i = 1; i < n; i++) {
    if (p[i] == '/') {
      if (last + 1 == i) return false;
      last = i;
    }
  }
  if (n > 1 && last + 1 == n) return false;
  *last_slash = last;
  return true;
}

inline bool valid_path(std::string_view p) {
  size_t last_slash;
  return scan_path(p, &last_slash);
}

// parent_view of a path scan_path accepted, from the index it reported
inline std::string_view parent_of(std::string_view p, size_t last_slash) {
  return p.substr(0, last_slash ? last_slash : 1);
}

// The node table and the watch maps are keyed by (path, hash of path). A
// request hashes its path once: the same value picks the shard and probes the
// table, and lookups go by view so no std::string is built to find a node.
// A node's path lives once, inline in the node's block (NodeStore below); the
// watch maps own their keys (PathKey, C++20 heterogeneous lookup).
struct PathKey {
  std::string path;
  size_t hash;
};
struct PathRef {
  std::string_view path;
  size_t hash;
};
inline PathRef ref_of(std::string_view p) { return {p, std::hash<std::string_view>{}(p)}; }
inline PathRef ref_of(const PathKey& k) { return {k.path, k.hash}; }
struct PathHash {
  using is_transparent = void;
  size_t operator()(const PathKey& k) const noexcept { return k.hash; }
  size_t operator()(const PathRef& r) const noexcept { return r.hash; }
};
struct PathEq {
  using is_transparent = void;
  bool operator()(const PathKey& a, const PathKey& b) const noexcept { return a.path == b.path; }
  bool operator()(const PathKey& a, const PathRef& b) const noexcept { return a.path == b.path; }
  bool operator()(const PathRef& a, const PathKey& b) const noexcept { return a.path == b.path; }
};

struct Session;

// A znode is ONE block: this header, then its path bytes, then its data
// bytes. Blocks never move, so the tree links nodes by pointer:
//   - hash / chain / path_len are the node's place in its shard's table
//     (shard lock); the path is immutable,
//   - first_child / nchildren and the children's parent / sib_prev /
//     sib_next are guarded by THIS node's shard lock (a child is only ever
//     created or removed with its parent's shard locked, and a node with
//     children cannot be removed),
//   - owner / eph_prev / eph_next / eph_linked are guarded by the owner
//     session's eph_mu (taken inside the shard locks: shard → eph_mu),
//   - data lives inline behind the path while it fits the block; a setData
//     that outgrows the block moves it to `ext`, a buffer this node owns
//     (the node itself stays where it is).
struct ZNode {
  Stat stat;
  uint64_t hash = 0;       // full hash of the path
  ZNode* chain = nullptr;  // next node in the bucket
  ZNode* parent = nullptr;
  ZNode* first_child = nullptr;
  ZNode* sib_prev = nullptr;
  ZNode* sib_next = nullptr;
  // Ephemeral owner (null for persistent nodes). A plain pointer: the node
  // never keeps its session alive, the session outlives the node instead.
  //   - handle_create sets it only after reading alive==true under eph_mu,
  //     and links the node in that same section; a create that sees !alive
  //     links nothing and sets nothing.
  //   - kill_session holds the SessionPtr on its stack until its drain has
  //     removed every node linked to the session: a linked node is in the
  //     drain's list, and a node the drain has popped is deleted (by the
  //     drain, or by another request that takes the node's shard lock
  //     first) before the drain moves on, since both need that shard lock.
  //   - handle_multi may set it on an unlinked node when the session died
  //     mid-transaction; it keeps the SessionPtr on its stack until the
  //     rollback has removed that node (same shard-lock argument).
  //   - until kill_session runs, `sessions` holds the session.
  // It is dereferenced only with the node's shard locked, i.e. while the
  // node is in the table. Teardown (~NodeStore, release) never reads it.
  Session* owner = nullptr;
  ZNode* eph_prev = nullptr;
  ZNode* eph_next = nullptr;
  char* ext = nullptr;     // out-of-line data, null while the data is inline
  uint32_t path_len = 0;
  uint32_t data_len = 0;
  uint32_t inline_cap = 0;  // bytes behind the header (path + inline data)
  uint32_t ext_cap = 0;
  int32_t nchildren = 0;
  uint8_t size_class = 0;  // kNoClass: block was sized exactly, never cached
  bool eph_linked = false;

  char* tail() { return reinterpret_cast<char*>(this) + sizeof(ZNode); }
  const char* tail() const { return reinterpret_cast<const char*>(this) + sizeof(ZNode); }
  std::string_view path() const { return {tail(), path_len}; }
  PathRef ref() const { return {path(), static_cast<size_t>(hash)}; }
  std::string_view data() const { return {ext ? ext : tail() + path_len, data_len}; }
  std::string_view name() const {
    std::string_view p = path();
    return p.substr(p.rfind('/') + 1);
  }

  void set_data(std::string_view d) {
    if (d.size() <= inline_cap - path_len) {
      if (ext) {
        ::operator delete(ext);
        ext = nullptr;
        ext_cap = 0;
      }
      if (!d.empty()) memcpy(tail() + path_len, d.data(), d.size());
    } else {
      if (d.size() > ext_cap) {
        char* nb = static_cast<char*>(::operator new(d.size()));
        if (ext) ::operator delete(ext);
        ext = nb;
        ext_cap = static_cast<uint32_t>(d.size());
      }
      memcpy(ext, d.data(), d.size());
    }
    data_len = static_cast<uint32_t>(d.size());
  }
};

// Block size classes (header + path + data, rounded up). The registrar's
// own nodes (a ~25-byte path, a ~100-byte JSON record) land in the second.
inline constexpr size_t kBlockClasses[] = {256, 384, 512, 768, 1024, 1536, 2048, 4096};
inline constexpr size_t kNumClasses = sizeof(kBlockClasses) / sizeof(kBlockClasses[0]);
inline constexpr uint8_t kNoClass = 0xFF;
// Most released blocks a shard keeps per class. A re-register cycle at 8
// ranks x 1000 nodes frees, then re-creates, ~125 blocks per shard at
// uniform hashing; 256 covers that with room for skew. Retained at most:
// 64 shards x 256 x 384 bytes = ~6 MB for the class the registrar uses
// (~174 MB only if every class of every shard fills).
inline constexpr size_t kMaxCachedPerClass = 256;
static_assert(sizeof(ZNode) < kBlockClasses[0], "smallest class must hold a header");

// One shard's nodes: an intrusive chained hash table (power-of-two bucket
// array of ZNode*, the chain link and the full hash live in the node) plus
// the shard's free lists of released blocks. Everything here is guarded by
// the shard's lock. Growth relinks nodes and never moves them.
struct NodeStore {
  ZNode** buckets = nullptr;
  size_t nbuckets = 0;  // power of two
  size_t count = 0;

  // INVARIANT: a block goes onto a free list only after its node has left
  // the hash chain, its parent's sibling list and its owner's ephemeral
  // list (release() asserts the last two; erase() does the first), and no
  // ZNode* is dereferenced outside the lock that guards the link it was
  // read through. A recycled block is worse than a freed one: a stale
  // pointer would read a live, different node and no sanitizer would see it.
  struct FreeBlock {
    FreeBlock* next;
  };
  FreeBlock* free_head[kNumClasses] = {};
  size_t free_count[kNumClasses] = {};
  size_t cached = 0;  // sum of free_count

  NodeStore() = default;
  NodeStore(const NodeStore&) = delete;
  NodeStore& operator=(const NodeStore&) = delete;

  ~NodeStore() {
    for (size_t b = 0; b < nbuckets; b++) {
      for (ZNode* n = buckets[b]; n;) {
        ZNode* next = n->chain;
        if (n->ext) ::operator delete(n->ext);
        n->~ZNode();
        ::operator delete(n);
        n = next;
      }
    }
    ::operator delete(buckets);
    for (size_t c = 0; c < kNumClasses; c++) {
      for (FreeBlock* f = free_head[c]; f;) {
        FreeBlock* next = f->next;
        ::operator delete(f);
        f = next;
      }
    }
  }

  size_t size() const { return count; }

  // The shard index is hash % kShards (the low 6 bits), so the bucket index
  // takes its bits from further up.
  size_t bucket_of(uint64_t h) const { return (h >> 8) & (nbuckets - 1); }

  ZNode* find(const PathRef& r) const {
    if (nbuckets == 0) return nullptr;
    for (ZNode* n = buckets[bucket_of(r.hash)]; n; n = n->chain) {
      // the stored hash settles nearly every chain step without touching
      // the path bytes
      if (n->hash == r.hash && n->path_len == r.path.size() &&
          memcmp(n->tail(), r.path.data(), r.path.size()) == 0)
        return n;
    }
    return nullptr;
  }

  void grow() {
    size_t nn = nbuckets ? nbuckets * 2 : 16;
    ZNode** nb = static_cast<ZNode**>(::operator new(nn * sizeof(ZNode*)));
    memset(nb, 0, nn * sizeof(ZNode*));
    ZNode** old = buckets;
    size_t on = nbuckets;
    buckets = nb;
    nbuckets = nn;
    for (size_t b = 0; b < on; b++) {
      for (ZNode* n = old[b]; n;) {
        ZNode* next = n->chain;
        size_t i = bucket_of(n->hash);
        n->chain = buckets[i];
        buckets[i] = n;
        n = next;
      }
    }
    ::operator delete(old);
  }

  static uint8_t class_for(size_t bytes) {
    for (size_t c = 0; c < kNumClasses; c++)
      if (bytes <= kBlockClasses[c]) return static_cast<uint8_t>(c);
    return kNoClass;
  }

  // A new node for r (which must not be in the table) holding `data`:
  // exactly one block, from the free list of its class when there is one.
  ZNode* create(const PathRef& r, std::string_view data) {
    if (count >= nbuckets) grow();
    size_t need = sizeof(ZNode) + r.path.size() + data.size();
    uint8_t cls = class_for(need);
    size_t bytes = cls == kNoClass ? need : kBlockClasses[cls];
    void* mem;
    if (cls != kNoClass && free_head[cls]) {
      FreeBlock* f = free_head[cls];
      free_head[cls] = f->next;
      free_count[cls]--;
      cached--;
      mem = f;
    } else {
      mem = ::operator new(bytes);
    }
    ZNode* n = new (mem) ZNode();
    n->hash = r.hash;
    n->size_class = cls;
    n->path_len = static_cast<uint32_t>(r.path.size());
    n->inline_cap = static_cast<uint32_t>(bytes - sizeof(ZNode));
    n->data_len = static_cast<uint32_t>(data.size());
    memcpy(n->tail(), r.path.data(), r.path.size());
    if (!data.empty()) memcpy(n->tail() + r.path.size(), data.data(), data.size());
    size_t i = bucket_of(r.hash);
    n->chain = buckets[i];
    buckets[i] = n;
    count++;
    return n;
  }

  // Take n out of the table and release its block (and its out-of-line
  // data). The caller has already unlinked it from its parent and from its
  // owner's ephemeral list — see the invariant above.
  void erase(ZNode* n) {
    ZNode** pp = &buckets[bucket_of(n->hash)];
    while (*pp != n) pp = &(*pp)->chain;
    *pp = n->chain;
    count--;
    release(n);
  }

  void release(ZNode* n) {
    if (n->parent || n->eph_linked || n->first_child) std::abort();  // invariant
    if (n->ext) ::operator delete(n->ext);
    uint8_t cls = n->size_class;
    n->~ZNode();
    if (cls != kNoClass && free_count[cls] < kMaxCachedPerClass) {
      FreeBlock* f = reinterpret_cast<FreeBlock*>(n);
      f->next = free_head[cls];
      free_head[cls] = f;
      free_count[cls]++;
      cached++;
    } else {
      ::operator delete(n);
    }
  }
};

// A client session and the head of its ephemeral list. A node holds only a
// Session* (ZNode::owner has the lifetime argument).
struct Session {
  int64_t id = 0;
  std::string passwd;
  int timeout_ms = 30000;
  std::atomic<int64_t> last_touch{0};  // monotonic ms, lock-free touch
  std::atomic<uint64_t> conn_id{0};    // 0 = detached
  // false once kill_session starts; written under eph_mu, so a create that
  // reads it under eph_mu either links before the kill's drain or not at all
  std::atomic<bool> alive{true};
  TreeLock eph_mu;
  // this session's ephemerals: intrusive list through ZNode::eph_prev/next
  // (no per-create allocation, no second copy of the path)
  ZNode* eph_head = nullptr;
  size_t eph_count = 0;
};

// ---------------- links (the guarding lock is the caller's) ----------------

// par's shard lock held
inline void link_child(ZNode& par, ZNode& ch) {
  ch.parent = &par;
  ch.sib_prev = nullptr;
  ch.sib_next = par.first_child;
  if (par.first_child) par.first_child->sib_prev = &ch;
  par.first_child = &ch;
  par.nchildren++;
}

// the parent's shard lock held
inline void unlink_child(ZNode& ch) {
  ZNode* par = ch.parent;
  if (!par) return;
  if (ch.sib_prev)
    ch.sib_prev->sib_next = ch.sib_next;
  else
    par->first_child = ch.sib_next;
  if (ch.sib_next) ch.sib_next->sib_prev = ch.sib_prev;
  par->nchildren--;
  ch.parent = ch.sib_prev = ch.sib_next = nullptr;
}

// sorted child names (listings sort on demand; create/delete are O(1))
inline void list_children(const ZNode& n, std::vector<std::string>* out) {
  out->clear();
  out->reserve(static_cast<size_t>(n.nchildren));
  for (const ZNode* c = n.first_child; c; c = c->sib_next) out->emplace_back(c->name());
  std::sort(out->begin(), out->end());
}

// s.eph_mu held
inline void eph_link(Session& s, ZNode& n) {
  n.eph_prev = nullptr;
  n.eph_next = s.eph_head;
  if (s.eph_head) s.eph_head->eph_prev = &n;
  s.eph_head = &n;
  n.eph_linked = true;
  s.eph_count++;
}

// s.eph_mu held
inline void eph_unlink(Session& s, ZNode& n) {
  if (!n.eph_linked) return;
  if (n.eph_prev)
    n.eph_prev->eph_next = n.eph_next;
  else
    s.eph_head = n.eph_next;
  if (n.eph_next) n.eph_next->eph_prev = n.eph_prev;
  n.eph_prev = n.eph_next = nullptr;
  n.eph_linked = false;
  s.eph_count--;
}

}  // namespace detail
}  // namespace zk
}  // namespace registrar
