// block_cache.hpp -- the cache policy of the device memory pool and of the pinned result cache (runtime.hip), once and without HIP.
// It knows sizes and opaque pointers and never calls an allocator: whatever has to go back to its allocator is RETURNED, so that the
// owner makes the release call (hipFree / hipHostFree wait for the device) outside its lock.  No lock of its own: the owner's holds.
//   * freed blocks are kept and handed out again, best fit within a slack (take);
//   * a full cache makes room by letting its OLDEST blocks go -- onto a deferred list, not to the caller: a give-back is the hot
//     path, the release call belongs to a miss (reap) or a trim (drain).  The list has a bound all the same: beyond it give() hands it out.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <unordered_map>
#include <vector>

namespace anx {

class BlockCache {
 public:
  struct Policy {
    size_t limit;           // bytes of freed blocks kept; a larger block is never cached
    size_t slack_add;       // a request of n bytes takes a cached block of at most 2 n + slack_add
    size_t deferred_bound;  // bytes on the deferred list beyond which give() hands the list out
  };
  enum class Given { Kept, TooLarge, NotCacheable, Unknown };  // all but Kept: the caller releases the block
  explicit BlockCache(const Policy& p) : pol_(p) {}

  // a fresh block, handed out at once
  void add(void* p, size_t bytes, bool cacheable = true) { live_[p] = Live{bytes, cacheable}; }
  // a cached block for a request of `bytes`, or nullptr
  void* take(size_t bytes) {
    auto it = free_.lower_bound(bytes);
    if (it == free_.end() || it->first > 2 * bytes + pol_.slack_add) return nullptr;
    void* p = it->second.p;
    cached_ -= it->first;
    free_.erase(it);
    return p;
  }
  // A block comes back.  Kept: it is cached; `release` may have received the deferred list.
  Given give(void* p, std::vector<void*>& release) {
    auto it = live_.find(p);
    if (it == live_.end()) return Given::Unknown;
    const size_t bytes = it->second.bytes;
    if (!it->second.cacheable || bytes > pol_.limit) {
      const Given g = it->second.cacheable ? Given::TooLarge : Given::NotCacheable;
      live_.erase(it);
      return g;
    }
    while (cached_ + bytes > pol_.limit && !free_.empty()) {
      auto old = free_.begin();
      for (auto jt = free_.begin(); jt != free_.end(); ++jt)
        if (jt->second.at < old->second.at) old = jt;
      cached_ -= old->first;
      deferred_.push_back(old->second.p);
      deferred_bytes_ += old->first;
      live_.erase(old->second.p);
      free_.erase(old);
    }
    if (deferred_bytes_ > pol_.deferred_bound) reap(release);
    free_.emplace(bytes, Cached{p, ++clock_});
    cached_ += bytes;
    return Given::Kept;
  }
  // the deferred list: the caller releases it
  void reap(std::vector<void*>& release) {
    release.insert(release.end(), deferred_.begin(), deferred_.end());
    deferred_.clear();
    deferred_bytes_ = 0;
  }
  // every cached block: the caller releases them (blocks handed out stay known)
  void drop_cached(std::vector<void*>& release) {
    for (auto& kv : free_) { release.push_back(kv.second.p); live_.erase(kv.second.p); }
    free_.clear();
    cached_ = 0;
  }
  void drain(std::vector<void*>& release) { drop_cached(release); reap(release); }

  bool known(void* p, bool* cacheable = nullptr) const {
    auto it = live_.find(p);
    if (it != live_.end() && cacheable) *cacheable = it->second.cacheable;
    return it != live_.end();
  }
  size_t cached_bytes() const { return cached_; }
  size_t deferred_bytes() const { return deferred_bytes_; }

 private:
  struct Live { size_t bytes; bool cacheable; };
  struct Cached { void* p; uint64_t at; };          // at: when the block came back (the oldest leave first)
  Policy pol_;
  std::multimap<size_t, Cached> free_;              // size -> cached block
  std::unordered_map<void*, Live> live_;            // every block handed out or cached
  std::vector<void*> deferred_;                     // evicted, not yet released
  size_t cached_ = 0, deferred_bytes_ = 0;
  uint64_t clock_ = 0;
};

}  // namespace anx
