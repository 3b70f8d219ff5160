// Drives analiticcl_amd/csrc/block_cache.hpp -- the cache policy of the device memory pool and of the pinned result cache -- without
// HIP: a counting fake allocator (malloc / free + the set of live pointers) stands in for hipMalloc / hipHostMalloc, an owner shaped
// like the two in runtime.hip (a mutex, one cache, the allocator calls outside the lock) for DevPool and HostCache.
//   main policy  : the policy under both parameter sets (tests/test_block_cache_cpu.py builds it with ASan + UBSan)
//   main threads : four threads take and give back through one owner (built with TSan)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "block_cache.hpp"

using anx::BlockCache;
using Given = BlockCache::Given;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

namespace {
constexpr size_t MB = (size_t)1 << 20;

struct FakeAlloc {
  std::mutex mu;
  std::set<void*> live;
  size_t allocs = 0, frees = 0;
  void* get() {
    void* p = malloc(32);
    CHECK(p);
    std::lock_guard<std::mutex> g(mu);
    CHECK(live.insert(p).second);
    ++allocs;
    return p;
  }
  void put(void* p) {
    {
      std::lock_guard<std::mutex> g(mu);
      CHECK(live.erase(p) == 1);  // a double free, or a pointer that never came from here
      ++frees;
    }
    free(p);
  }
  bool is_live(void* p) { std::lock_guard<std::mutex> g(mu); return live.count(p) != 0; }
  size_t n_live() { std::lock_guard<std::mutex> g(mu); return live.size(); }
};

// the two parameter sets of runtime.hip for a cache limit of `limit` bytes
struct Set { const char* name; size_t slack_add; size_t (*bound)(size_t limit); size_t (*round)(size_t bytes); bool pinned_only; };
size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t round_mb(size_t b) { return ((b < 64 ? 64 : b) + MB - 1) & ~(MB - 1); }
const Set kDevice{"device", MB, [](size_t l) { return l / 2; }, round256, false};
const Set kHost{"host", 0, [](size_t l) { return l; }, round_mb, true};
BlockCache::Policy policy_of(const Set& s, size_t limit) { return BlockCache::Policy{limit, s.slack_add, s.bound(limit)}; }

// a thin owner, as DevPool / HostCache: every allocator call is made outside the lock
struct Owner {
  const Set& set;
  FakeAlloc& fa;
  std::mutex mu;
  BlockCache cache;
  size_t hits = 0, misses = 0;
  Owner(const Set& s, size_t limit, FakeAlloc& a) : set(s), fa(a), cache(policy_of(s, limit)) {}
  void put_all(const std::vector<void*>& v) { for (void* p : v) fa.put(p); }
  void* alloc(size_t bytes, bool cacheable = true) {
    bytes = set.round(bytes);
    std::vector<void*> drop;
    {
      std::lock_guard<std::mutex> g(mu);
      if (void* p = cache.take(bytes)) { ++hits; return p; }
      ++misses;
      cache.reap(drop);
    }
    put_all(drop);
    void* p = fa.get();
    std::lock_guard<std::mutex> g(mu);
    cache.add(p, bytes, cacheable);
    return p;
  }
  Given release(void* p) {
    std::vector<void*> drop;
    Given given;
    { std::lock_guard<std::mutex> g(mu); given = cache.give(p, drop); }
    put_all(drop);
    if (given != Given::Kept) fa.put(p);
    return given;
  }
  void trim() {
    std::vector<void*> drop;
    { std::lock_guard<std::mutex> g(mu); cache.drain(drop); }
    put_all(drop);
  }
};

bool has(const std::vector<void*>& v, void* p) { for (void* q : v) if (q == p) return true; return false; }

// a request is served from the cache exactly when a block within the slack exists, and not one byte beyond
void check_slack(const Set& s) {
  FakeAlloc fa;
  BlockCache c(policy_of(s, 64 * MB));
  std::vector<void*> rel;
  const size_t S = 4 * MB;
  void* p = fa.get();
  c.add(p, S);
  CHECK(c.take(S) == nullptr);  // handed out, not cached
  auto served = [&](size_t bytes) {
    void* q = c.take(bytes);
    if (!q) return false;
    CHECK(q == p);
    CHECK(c.give(q, rel) == Given::Kept);
    return true;
  };
  CHECK(c.give(p, rel) == Given::Kept && c.cached_bytes() == S);
  CHECK(served(S));          // the block's own size
  CHECK(!served(S + 1));     // never a block smaller than the request
  const size_t lo = (S - s.slack_add + 1) / 2;  // the smallest request with 2 * request + slack_add >= S
  CHECK(2 * lo + s.slack_add >= S && 2 * (lo - 1) + s.slack_add < S);
  CHECK(served(lo));
  CHECK(!served(lo - 1));
  CHECK(s.slack_add == (s.pinned_only ? 0 : MB) && lo == (s.pinned_only ? 2 * MB : 3 * MB / 2));
  // best fit: the smallest block that holds the request
  void* small = fa.get();
  c.add(small, 2 * MB);
  CHECK(c.give(small, rel) == Given::Kept);
  CHECK(c.take(2 * MB) == small && c.take(2 * MB) == p && c.take(2 * MB) == nullptr);
  CHECK(c.give(small, rel) == Given::Kept && c.give(p, rel) == Given::Kept);
  // through an owner: its rounding comes first
  Owner o(s, 64 * MB, fa);
  void* a = o.alloc(3 * MB);
  CHECK(o.release(a) == Given::Kept);
  CHECK(o.alloc(3 * MB - 100) == a && o.hits == 1);  // (both roundings reach 3 MB or just below it: within the slack)
  CHECK(o.release(a) == Given::Kept);
  void* b = o.alloc(MB - 1000);                       // 3 MB > 2 * request + slack_add under both sets: a miss
  CHECK(b != a && o.misses == 2);
  CHECK(o.release(b) == Given::Kept);
  o.trim();
  CHECK(rel.empty());
  c.drain(rel);
  CHECK(rel.size() == 2);
  for (void* q : rel) fa.put(q);
  CHECK(fa.n_live() == 0 && fa.allocs == fa.frees);
}

// blocks leave oldest first (by when they came back, not by size); an evicted block is not released by the give-back that evicted it
// until the deferred bound is passed; a miss and a drain release it
void check_eviction(const Set& s) {
  FakeAlloc fa;
  const size_t U = MB, limit = 6 * U;
  BlockCache c(policy_of(s, limit));
  std::vector<void*> rel;
  void *A = fa.get(), *B = fa.get(), *C = fa.get(), *D = fa.get(), *E = fa.get();
  c.add(A, 3 * U); c.add(B, 1 * U); c.add(C, 2 * U); c.add(D, 1 * U); c.add(E, 3 * U);
  CHECK(c.give(A, rel) == Given::Kept && c.give(B, rel) == Given::Kept && c.give(C, rel) == Given::Kept);
  CHECK(c.cached_bytes() == limit && c.deferred_bytes() == 0 && rel.empty());
  CHECK(c.give(D, rel) == Given::Kept);  // full: the oldest, A, makes room -- onto the deferred list
  CHECK(rel.empty() && c.deferred_bytes() == 3 * U && c.cached_bytes() == 4 * U);
  CHECK(!c.known(A) && c.known(B) && c.known(C) && c.known(D));
  CHECK(c.take(3 * U) == nullptr);       // A is gone from the cache
  CHECK(c.take(U) == B);                 // (equal sizes: in the order they came back)
  CHECK(c.give(B, rel) == Given::Kept);  // B is the youngest now, C the oldest
  CHECK(c.give(E, rel) == Given::Kept);  // 4 + 3 > 6: C leaves, B stays
  CHECK(!c.known(C) && c.known(B) && c.known(D) && c.known(E) && c.cached_bytes() == 5 * U);
  if (!s.pinned_only) {  // device set: the bound is limit / 2 = 3 U; A alone did not pass it, A + C = 5 U does
    CHECK(rel.size() == 2 && has(rel, A) && has(rel, C) && c.deferred_bytes() == 0);
  } else {               // host set: the bound is the limit = 6 U: both wait
    CHECK(rel.empty() && c.deferred_bytes() == 5 * U);
    c.reap(rel);         // what a miss does
    CHECK(rel.size() == 2 && has(rel, A) && has(rel, C) && c.deferred_bytes() == 0);
  }
  CHECK(fa.is_live(A) && fa.is_live(C));  // the cache itself released nothing
  for (void* q : rel) fa.put(q);
  rel.clear();
  c.drain(rel);
  CHECK(rel.size() == 3 && has(rel, B) && has(rel, D) && has(rel, E) && c.cached_bytes() == 0);
  for (void* q : rel) fa.put(q);
  CHECK(fa.n_live() == 0);

  // the same through an owner with a limit of three blocks: a miss releases the evicted block, and so does a trim
  Owner o(s, 3 * MB, fa);
  void* blk[4];
  for (void*& p : blk) p = o.alloc(MB);
  for (void* p : blk) CHECK(o.release(p) == Given::Kept);  // the fourth evicts blk[0]: 1 MB is within either bound
  CHECK(fa.is_live(blk[0]) && fa.n_live() == 4);
  void* big = o.alloc(16 * MB);                            // a miss
  CHECK(!fa.is_live(blk[0]) && fa.n_live() == 4);
  CHECK(o.release(big) == Given::TooLarge && fa.n_live() == 3);  // above the limit: never cached
  std::set<void*> got;
  for (int i = 0; i < 3; ++i) got.insert(o.alloc(MB));
  CHECK(got == std::set<void*>({blk[1], blk[2], blk[3]}) && o.hits == 3);
  void* fresh = o.alloc(MB);
  CHECK(!got.count(fresh) && fa.n_live() == 4);
  for (void* p : got) CHECK(o.release(p) == Given::Kept);
  CHECK(o.release(fresh) == Given::Kept);                  // evicts once more
  CHECK(fa.n_live() == 4);
  o.trim();                                                // the cached three and the deferred one
  CHECK(fa.n_live() == 0 && fa.allocs == fa.frees);
}

// a block above the limit, and for the host set an unpinned one, is never cached; an unknown pointer is reported as unknown
void check_refusals(const Set& s) {
  FakeAlloc fa;
  Owner o(s, 4 * MB, fa);
  void* big = o.alloc(4 * MB + 1);
  CHECK(o.release(big) == Given::TooLarge && !fa.is_live(big));
  void* big2 = o.alloc(4 * MB + 1);  // (the allocator may hand the same address out again: the cache must not have kept it)
  CHECK(o.hits == 0 && o.misses == 2);
  CHECK(o.release(big2) == Given::TooLarge);
  void* fits = o.alloc(4 * MB);      // exactly the limit: cached
  CHECK(o.release(fits) == Given::Kept && o.alloc(4 * MB) == fits && o.hits == 1);
  CHECK(o.release(fits) == Given::Kept);
  if (s.pinned_only) {
    void* plain = o.alloc(MB, false);  // pinning failed: a malloc block
    bool cacheable = true;
    { std::lock_guard<std::mutex> g(o.mu); CHECK(o.cache.known(plain, &cacheable) && !cacheable); }
    CHECK(o.release(plain) == Given::NotCacheable && !fa.is_live(plain));
    void* again = o.alloc(MB, true);
    CHECK(o.hits == 1);  // not served from the cache
    CHECK(o.release(again) == Given::Kept);
  }
  int on_stack = 0;
  std::vector<void*> rel;
  {
    std::lock_guard<std::mutex> g(o.mu);
    CHECK(o.cache.give(&on_stack, rel) == Given::Unknown && rel.empty() && !o.cache.known(&on_stack));
  }
  void* foreign = fa.get();
  CHECK(o.release(foreign) == Given::Unknown && !fa.is_live(foreign));  // the owner releases it, as pool_free / host_result_free do
  o.trim();
  CHECK(fa.n_live() == 0 && fa.allocs == fa.frees);
  {
    std::lock_guard<std::mutex> g(o.mu);
    CHECK(!o.cache.known(fits) && o.cache.cached_bytes() == 0 && o.cache.deferred_bytes() == 0);
  }
}

int run_policy() {
  for (const Set* s : {&kDevice, &kHost}) {
    check_slack(*s);
    check_eviction(*s);
    check_refusals(*s);
  }
  printf("OK policy\n");
  return 0;
}

int run_threads() {
  constexpr int kThreads = 4, kRounds = 3000;
  for (const Set* s : {&kDevice, &kHost}) {
    FakeAlloc fa;
    Owner o(*s, 6 * MB, fa);  // a few blocks: evictions, deferred releases and misses all happen
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t)
      th.emplace_back([&o, t]() {
        uint32_t x = 12345u + 977u * (uint32_t)t;
        std::vector<void*> held;
        for (int r = 0; r < kRounds; ++r) {
          x = x * 1664525u + 1013904223u;
          if (held.size() < 3 && (x >> 16) % 3u != 0u) {
            void* p = o.alloc(((x >> 8) % 5u + 1u) * (MB / 2), (x >> 24) % 7u != 0u || !o.set.pinned_only);
            memset(p, (int)(x & 0xFF), 32);  // the block is this thread's alone
            held.push_back(p);
          } else if (!held.empty()) {
            o.release(held.back());
            held.pop_back();
          }
        }
        for (void* p : held) o.release(p);
      });
    for (auto& x : th) x.join();
    CHECK(o.hits > 0 && o.misses > 0);
    o.trim();
    CHECK(fa.n_live() == 0 && fa.allocs == fa.frees);
  }
  printf("OK threads\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "policy")) return run_policy();
  if (argc == 2 && !strcmp(argv[1], "threads")) return run_threads();
  fprintf(stderr, "usage: %s policy|threads\n", argv[0]);
  return 2;
}
