// dsx_devmem.h -- who owns a context's HBM: one ledger (DevMem) that every
// device allocation goes through, and the typed handle into it (DevBuf<T>).
// No HIP in here: the ledger is given its allocate and free functions (the
// library hands it hipMalloc and hipFree, dsx_engine.h; tests/devmem_model.cpp
// a recording fake under the host sanitizers).  dsx_stats_t.device_bytes is
// the ledger's total, and dsx_ctx_destroy frees whatever it still holds.
//
// No lock: every ensure, grow and release runs on the thread that makes the
// context's call (the reader, tail and pool threads of dsx_index.cpp,
// dsx_hosttail.cpp and dsx_stream.cpp allocate no device memory), and
// dsx_get_stats, unlike dsx_progress and dsx_cancel, is not documented as
// callable from a second thread (include/dsx.h: a context is not thread-safe).
#ifndef DSX_DEVMEM_H_
#define DSX_DEVMEM_H_
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>

namespace dsx_host {

class DevMem {
 public:
  // hipMalloc's and hipFree's shapes; 0 is success
  using AllocFn = int (*)(void** p, size_t bytes);
  using FreeFn = int (*)(void* p);

  DevMem(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;

  // *p = a new allocation of `bytes` bytes, recorded; on an error *p = nullptr
  int alloc(size_t bytes, void** p) {
    *p = nullptr;
    void* q = nullptr;
    const int e = alloc_(&q, bytes);
    if (e != 0) return e;
    live_[q] = bytes;
    total_ += bytes;
    *p = q;
    return 0;
  }
  // Frees and forgets p.  Null, or a pointer the ledger does not hold (the
  // second release of a copied handle): nothing, and nothing reaches the device.
  void free(void* p) {
    if (!p) return;
    const auto it = live_.find(p);
    if (it == live_.end()) return;
    total_ -= it->second;
    live_.erase(it);
    (void)free_(p);
  }
  uint64_t bytes() const { return total_; }
  size_t count() const { return live_.size(); }
  bool holds(const void* p) const { return live_.count(const_cast<void*>(p)) != 0; }
  // frees everything still held (the handles that pointed there dangle)
  void release_all() {
    for (const auto& kv : live_) (void)free_(kv.first);
    live_.clear();
    total_ = 0;
  }

 private:
  AllocFn alloc_;
  FreeFn free_;
  std::unordered_map<void*, size_t> live_;  // live pointer -> bytes
  uint64_t total_ = 0;
};

// n elements of T at p, allocated from (and charged n * sizeof(T) in) *mem.
// Trivially copyable, no destructor: ownership is the ledger's, keyed by the
// pointer, so a handle may be moved (KeptPiece lives in a std::vector) and a
// copy's second release is harmless.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevMem* mem = nullptr;
  // At least max(want, 16) elements; contents are not kept when it reallocates.
  // A failed allocation leaves p == nullptr, n == 0 and returns its error.
  int ensure(DevMem& m, size_t want) {
    if (want <= n && p) return 0;
    release();
    const size_t sz = want < 16 ? 16 : want;
    void* q = nullptr;
    const int e = m.alloc(sz * sizeof(T), &q);
    if (e != 0) return e;
    p = static_cast<T*>(q);
    n = sz;
    mem = &m;
    return 0;
  }
  void release() {
    if (mem) mem->free(p);
    p = nullptr;
    n = 0;
  }
};

}  // namespace dsx_host
#endif  // DSX_DEVMEM_H_
