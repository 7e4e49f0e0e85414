// devmem_model.cpp -- a context's device-memory ledger on the CPU.
//
// A stand-alone host program over desync_amd/csrc/dsx_devmem.h: DevMem, the
// ledger every device allocation of a context goes through, and DevBuf<T>, the
// typed handle into it.  tests/test_host_logic.py builds it with
// -fsanitize=address,undefined and runs it.  The allocator is a fake on
// malloc/free that records every call, fails the k-th allocation on request
// and aborts on a free of a pointer it did not hand out or already took back.
// Seeded scripts of ensure, growth, release, copied handles and failed
// allocations run over 20 buffers of mixed element types; after every step the
// ledger's total is the sum of n * sizeof(T) over the handles and its live set
// is the fake's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <type_traits>
#include <vector>

#include "dsx_devmem.h"

using namespace dsx_host;

static int failures = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      if (++failures <= 40) {                          \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                      \
        std::printf("\n");                             \
      }                                                \
    }                                                  \
  } while (0)
typedef unsigned long long ull;

static uint64_t rng_state = 0;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- the fake device ------------------------------------------------------------
constexpr int kFakeNoMem = 2;  // (any non-zero code)
struct Fake {
  std::map<void*, size_t> live;
  uint64_t allocs = 0, frees = 0, bytes = 0;
  uint64_t fail_in = 0;  // k > 0: the k-th allocation from now fails
} fake;

static int fake_alloc(void** p, size_t bytes) {
  ++fake.allocs;
  if (fake.fail_in && --fake.fail_in == 0) return kFakeNoMem;
  void* q = std::malloc(bytes);
  if (!q) std::abort();
  fake.live[q] = bytes;
  fake.bytes += bytes;
  *p = q;
  return 0;
}

static int fake_free(void* p) {
  ++fake.frees;
  const auto it = fake.live.find(p);
  if (it == fake.live.end()) {
    std::printf("FAIL: free of %p, which the fake does not hold\n", p);
    std::abort();
  }
  fake.bytes -= it->second;
  fake.live.erase(it);
  std::free(p);
  return 0;
}

// ---- 20 handles of mixed element types --------------------------------------
struct Seg {  // (a 24-byte element, like the engine's per-segment records)
  uint64_t a, b, c;
};

struct Slot {
  virtual ~Slot() {}
  virtual int ensure(DevMem& m, size_t want) = 0;
  virtual void release() = 0;
  virtual void release_a_copy_too() = 0;  // copy the handle, release both
  virtual const void* p() const = 0;
  virtual size_t n() const = 0;
  virtual size_t elem() const = 0;
  uint64_t bytes() const { return (uint64_t)n() * elem(); }
};

template <class T>
struct TypedSlot : Slot {
  static_assert(std::is_trivially_copyable<DevBuf<T>>::value &&
                    std::is_trivially_destructible<DevBuf<T>>::value,
                "DevBuf is a plain handle");
  DevBuf<T> b;
  int ensure(DevMem& m, size_t want) override { return b.ensure(m, want); }
  void release() override { b.release(); }
  void release_a_copy_too() override {
    DevBuf<T> copy = b;
    if (rnd() & 1) {
      b.release();
      copy.release();
    } else {
      copy.release();
      b.release();
    }
    CHECK(!copy.p && !copy.n, "a released copy is empty");
  }
  const void* p() const override { return b.p; }
  size_t n() const override { return b.n; }
  size_t elem() const override { return sizeof(T); }
};

static std::vector<std::unique_ptr<Slot>> make_slots() {
  std::vector<std::unique_ptr<Slot>> s;
  for (int i = 0; i < 5; ++i) {
    s.emplace_back(new TypedSlot<uint8_t>);
    s.emplace_back(new TypedSlot<uint32_t>);
    s.emplace_back(new TypedSlot<uint64_t>);
    s.emplace_back(new TypedSlot<Seg>);
  }
  return s;
}

static uint64_t n_steps = 0, n_realloc = 0, n_failed = 0, n_copies = 0;

// the ledger against the handles and against the fake
static void check_all(const DevMem& mem, const std::vector<std::unique_ptr<Slot>>& slots, ull seed,
                      ull step) {
  uint64_t sum = 0, live = 0;
  for (const auto& s : slots) {
    CHECK((s->p() == nullptr) == (s->n() == 0), "seed %llu step %llu: p and n disagree", seed, step);
    if (!s->p()) continue;
    sum += s->bytes();
    ++live;
    CHECK(s->n() >= 16, "seed %llu step %llu: n %llu below the minimum", seed, step, (ull)s->n());
    CHECK(mem.holds(s->p()), "seed %llu step %llu: a live handle the ledger does not hold", seed, step);
    const auto it = fake.live.find(const_cast<void*>(s->p()));
    CHECK(it != fake.live.end() && it->second == s->bytes(),
          "seed %llu step %llu: the fake's size of a live handle", seed, step);
  }
  CHECK(mem.bytes() == sum, "seed %llu step %llu: bytes() %llu, handles %llu", seed, step,
        (ull)mem.bytes(), (ull)sum);
  CHECK(mem.count() == live && fake.live.size() == live && fake.bytes == sum,
        "seed %llu step %llu: ledger holds %llu, fake %llu (%llu bytes), handles %llu", seed, step,
        (ull)mem.count(), (ull)fake.live.size(), (ull)fake.bytes, (ull)live);
}

static void run_script(ull seed, int steps) {
  rng_state = seed * 0x2545F4914F6CDD1Dull + 1;
  DevMem mem(fake_alloc, fake_free);
  auto slots = make_slots();
  for (int step = 0; step < steps; ++step, ++n_steps) {
    Slot& s = *slots[rnd() % slots.size()];
    const uint64_t before = mem.bytes(), old_bytes = s.bytes();
    const uint64_t allocs = fake.allocs, frees = fake.frees;
    const void* old_p = s.p();
    const size_t old_n = s.n();
    switch (rnd() % 8) {
      case 0:
      case 1: {  // ensure: any size, below the minimum and below n included
        const size_t want = rnd() % 4 == 0 ? rnd() % 20 : rnd() % 5000;
        const int e = s.ensure(mem, want);
        CHECK(e == 0, "seed %llu step %d: ensure failed", seed, step);
        if (old_p && want <= old_n) {
          CHECK(s.p() == old_p && s.n() == old_n && fake.allocs == allocs && fake.frees == frees,
                "seed %llu step %d: an ensure that fits touched the buffer", seed, step);
        } else {
          CHECK(s.n() == (want < 16 ? 16 : want) && fake.allocs == allocs + 1 &&
                    fake.frees == frees + (old_p ? 1 : 0),
                "seed %llu step %d: ensure(%llu) left n %llu", seed, step, (ull)want, (ull)s.n());
        }
        break;
      }
      case 2:
      case 3: {  // growth that reallocates
        const size_t want = old_n + 1 + rnd() % 3000;
        const int e = s.ensure(mem, want);
        ++n_realloc;
        CHECK(e == 0 && s.n() == (want < 16 ? 16 : want) && fake.allocs == allocs + 1 &&
                  fake.frees == frees + (old_p ? 1 : 0),
              "seed %llu step %d: growth to %llu left n %llu", seed, step, (ull)want, (ull)s.n());
        CHECK(mem.bytes() == before - old_bytes + s.bytes(), "seed %llu step %d: growth's charge", seed,
              step);
        break;
      }
      case 4:  // release (of an empty handle too)
        s.release();
        CHECK(!s.p() && !s.n() && fake.frees == frees + (old_p ? 1 : 0) && mem.bytes() == before - old_bytes,
              "seed %llu step %d: release", seed, step);
        break;
      case 5:  // a copied handle, both released: one free reaches the device
        s.release_a_copy_too();
        ++n_copies;
        CHECK(!s.p() && !s.n() && fake.frees == frees + (old_p ? 1 : 0) && mem.bytes() == before - old_bytes,
              "seed %llu step %d: a copy's release freed twice or not at all", seed, step);
        break;
      case 6: {  // a failed allocation: the handle empty, only the old buffer gone
        fake.fail_in = 1;
        const int e = s.ensure(mem, old_n + 1 + rnd() % 3000);
        ++n_failed;
        CHECK(e == kFakeNoMem && !s.p() && !s.n(), "seed %llu step %d: a failed ensure left p %p n %llu",
              seed, step, s.p(), (ull)s.n());
        CHECK(mem.bytes() == before - old_bytes && fake.frees == frees + (old_p ? 1 : 0) &&
                  fake.fail_in == 0,
              "seed %llu step %d: a failed ensure's total", seed, step);
        break;
      }
      case 7: {  // the ledger alone: a pointer it does not hold, and null
        int local = 0;
        mem.free(&local);
        mem.free(nullptr);
        CHECK(fake.frees == frees && mem.bytes() == before, "seed %llu step %d: a foreign free reached the device",
              seed, step);
        break;
      }
    }
    check_all(mem, slots, seed, (ull)step);
  }
  // the end of a context: everything still held goes back, once
  const uint64_t frees = fake.frees, held = mem.count();
  mem.release_all();
  CHECK(fake.live.empty() && fake.bytes == 0 && mem.bytes() == 0 && mem.count() == 0 &&
            fake.frees == frees + held,
        "seed %llu: release_all left %llu allocations", seed, (ull)fake.live.size());
  for (auto& s : slots) s->release();  // the handles dangle: their release reaches nothing
  CHECK(fake.frees == frees + held, "seed %llu: a release after release_all reached the device", seed);
  for (void* p = nullptr; !fake.live.empty();) {  // (after a failure: leave the sanitizer's report clean)
    p = fake.live.begin()->first;
    fake_free(p);
  }
}

int main() {
  for (ull seed = 1; seed <= 8; ++seed) run_script(seed, 4000);
  if (failures) {
    std::printf("devmem model: %d failures\n", failures);
    return 1;
  }
  std::printf("devmem model ok: %llu steps, %llu reallocations, %llu failed allocations, %llu copied handles\n",
              (ull)n_steps, (ull)n_realloc, (ull)n_failed, (ull)n_copies);
  return 0;
}
