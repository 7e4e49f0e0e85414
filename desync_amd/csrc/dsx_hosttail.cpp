// dsx_hosttail.cpp -- the host tail of the file pipeline (dsx_hosttail.h):
// which chunks of a window the host hashes, the hashing itself, and the
// feeder thread that follows the stitches of a call's last window.
#include "dsx_hosttail.h"

#include <algorithm>
#include <chrono>
#include <deque>

double host_ns_per_byte() {
  static const double v = [] {
    if (!host_sha_vec()) return 4.0 * kHostNsPerByte;  // (the scalar path)
    constexpr uint64_t n = 128 << 10;
    std::vector<uint8_t> buf(8 * n, 0x5a), out(8 * 32);
    const uint8_t* p[8];
    uint64_t len[8];
    uint8_t* o[8];
    for (int i = 0; i < 8; ++i) p[i] = buf.data() + i * n, len[i] = n, o[i] = out.data() + 32 * i;
    host_sha512_256_x8(p, len, o);  // (warm)
    const auto t0 = std::chrono::steady_clock::now();
    host_sha512_256_x8(p, len, o);
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    return 1.15 * ns / (8.0 * (double)n);  // (+15 %: the read through `fill`)
  }();
  return std::max(v, kHostNsPerByte);
}

std::vector<TailChunk> plan_tail(const dsx_ctx* c, const std::vector<uint64_t>& e, uint64_t i0,
                                 uint64_t first, int threads, uint64_t* cut) {
  std::vector<TailChunk> t(e.size());
  for (size_t i = 0; i < e.size(); ++i) {
    const uint64_t s = i ? e[i - 1] : first;
    t[i] = {i0 + i, s, e[i] - s};
  }
  std::sort(t.begin(), t.end(), [](const TailChunk& a, const TailChunk& b) { return a.len > b.len; });
  *cut = 0;
  if (t.empty()) return {};
  size_t k = 0;
  if (c->index_host_tail > 0) {  // forced cut (tests)
    while (k < t.size() && t[k].len > (uint64_t)c->index_host_tail) ++k;
    *cut = (uint64_t)c->index_host_tail;
  } else {
    // k chunks to the host: time max(host bytes / threads, GPU's longest chain)
    const double now = kGpuNsPerByte * (double)t[0].len;
    double best = now, bytes = 0;
    for (size_t j = 0; j + 1 < t.size(); ++j) {
      bytes += (double)t[j].len;
      const double tj = std::max(bytes * kHostNsPerByte / threads, kGpuNsPerByte * (double)t[j + 1].len);
      if (tj < best) {
        best = tj;
        k = j + 1;
      }
      if (bytes * kHostNsPerByte / threads > now) break;
    }
    if (now - best < kTailMinGainNs) k = 0;
    // (chunks as long as the first one left to the GPU stay there)
    while (k > 0 && t[k - 1].len == t[k].len) --k;
    if (k) *cut = t[k].len;
  }
  t.resize(k);
  return t;
}

int hash_group(const TailSrc& src, const TailChunk* t, uint64_t cnt, uint8_t* ids,
               std::vector<uint8_t>& buf) {
  const bool vec = host_sha_vec();
  const uint64_t per = vec ? 8 : 1;
  uint64_t total = 0;
  for (uint64_t j = 0; j < cnt; ++j) total += t[j].len;
  if (!src.direct && buf.size() < total + 1) buf.resize(total + 1);
  const uint8_t* p[8];
  uint64_t n[8];
  uint8_t* o[8];
  uint64_t at = 0;
  int rc = DSX_OK;
  for (uint64_t j = 0; j < per; ++j) {
    if (j >= cnt) {
      p[j] = nullptr;
      n[j] = UINT64_MAX;
      o[j] = nullptr;
      continue;
    }
    n[j] = t[j].len;
    o[j] = ids + 32 * j;
    if (src.direct) {
      p[j] = src.direct + t[j].start;
      continue;
    }
    if (t[j].len && rc == DSX_OK) rc = src.fill(src.ud, buf.data() + at, t[j].start, t[j].len);
    p[j] = buf.data() + at;
    at += t[j].len;
  }
  if (rc) return rc;
  if (vec)
    host_sha512_256_x8(p, n, o);
  else
    host_sha512_256_one(p[0], n[0], o[0]);
  return DSX_OK;
}

int hash_tail(const TailSrc& src, const std::vector<TailChunk>& t, uint8_t* ids, int threads,
              const std::atomic<int>* halt, const std::atomic<int>* cancel) {
  const uint64_t per = host_sha_vec() ? 8 : 1;
  const uint64_t groups = (t.size() + per - 1) / per;
  std::atomic<uint64_t> next{0};
  std::atomic<int> err{DSX_OK};
  host_parallel((int)std::min<uint64_t>((uint64_t)threads, groups), [&](int) {
    std::vector<uint8_t> buf;
    for (uint64_t g; err.load() == DSX_OK && (g = next.fetch_add(1)) < groups;) {
      if ((halt && halt->load(std::memory_order_relaxed)) ||
          (cancel && cancel->load(std::memory_order_relaxed))) {
        err.store(DSX_E_INTERRUPTED);
        return;
      }
      const uint64_t j0 = g * per, j1 = std::min<uint64_t>(t.size(), j0 + per);
      const int rc = hash_group(src, t.data() + j0, j1 - j0, ids + 32 * j0, buf);
      if (rc) {
        err.store(rc);
        return;
      }
    }
  });
  return err.load();
}

void TailFeeder::finish(uint64_t total) {
  {
    std::lock_guard<std::mutex> g(m_);
    final_ = total;
    have_final_ = true;
  }
  cv_.notify_all();
}

void TailFeeder::stop() {
  halt_.store(1);  // (the hashers stop at their next group of 8)
  {
    std::lock_guard<std::mutex> g(m_);
    stop_ = true;
  }
  cv_.notify_all();
  if (th_.joinable()) th_.join();
}

uint64_t TailFeeder::published() const {
  const volatile HostState* h = (const volatile HostState*)c_->h_state;
  const uint64_t q0 = h->seq;
  const uint64_t t = h->total;
  const uint64_t q1 = h->seq;
  return (q0 == q1 && q0 > seq0_) ? t : 0;
}

template <class Put>
int TailFeeder::produce(hipStream_t s, Put&& put) {
  std::vector<uint64_t> e;
  uint64_t seen = 0, prev = 0;
  if (start_ev_) {
    uint64_t sn[2] = {0, 0};
    if (hipEventSynchronize(start_ev_) != hipSuccess ||
        hipMemcpyAsync(sn, dsnap_, sizeof sn, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return DSX_E_HIP;
    seen = sn[0];
    prev = sn[1];
  }
  std::vector<Bound> known;  // the boundaries resolved so far (their totals read)
  while (true) {
    uint64_t target;
    bool last;
    std::vector<Bound> fresh;
    {
      std::unique_lock<std::mutex> g(m_);
      cv_.wait_for(g, std::chrono::microseconds(200), [&] { return stop_ || have_final_; });
      if (stop_) return DSX_E_INTERRUPTED;
      last = have_final_;
      // (read with the boundaries under one lock: a total published before
      // add_boundary cannot come from a piece after that snapshot)
      target = last ? final_ : std::max(seen, published());
      fresh.assign(bounds_.begin() + (long)known.size(), bounds_.end());
    }
    for (Bound& b : fresh) {
      uint64_t sn[2] = {0, 0};
      if (hipEventSynchronize(b.ev) != hipSuccess ||
          hipMemcpyAsync(sn, b.snap, sizeof sn, hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess)
        return DSX_E_HIP;
      b.total = sn[0];
      known.push_back(b);
    }
    if (target > seen) {
      e.resize(target - seen);
      if (hipMemcpyAsync(e.data(), c_->out.p + seen, e.size() * 8, hipMemcpyDeviceToHost, s) !=
              hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess)
        return DSX_E_HIP;
      std::vector<TailChunk> batch;
      for (uint64_t i = 0; i < e.size(); ++i) {
        const uint64_t st = i ? e[i - 1] : prev;
        // (a call that overflows its candidate slots reruns and drops these:
        // never read outside the source for them)
        uint64_t cut = cut_;
        for (const Bound& b : known)
          if (seen + i >= b.total) cut = b.cut_after;
        if (e[i] > st && e[i] <= len_ && e[i] - st > cut) batch.push_back({seen + i, st, e[i] - st});
      }
      prev = e.back();
      seen = target;
      if (!batch.empty()) {
        const int rc = put(batch);
        if (rc) return rc;
      }
    }
    if (last) return DSX_OK;
  }
}

// This thread follows the published totals and queues each new batch's
// long chunks, longest first, in groups of 8 (part 0 of the host pool);
// threads_ more parts hash the groups as they come.  (Until round 6 each
// batch was hashed whole before the next was fetched: the threads idled at
// every batch's end, and the call's last batch waited for the one before.)
void TailFeeder::run() {
  if (hipSetDevice(c_->device) != hipSuccess) {
    err_ = DSX_E_HIP;
    return;
  }
  // (default priority: beside the null stream in that pool; `stream` and
  // `copy_stream` are in the high pool, the digests in the low one)
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    err_ = DSX_E_HIP;
    return;
  }
  chunks.reserve(cap_);  // (never reallocated: the hashers read it while it grows)
  ids.assign(32 * cap_, 0);
  const uint64_t per = host_sha_vec() ? 8 : 1;
  std::mutex qm;
  std::condition_variable qcv;
  std::deque<std::pair<size_t, uint64_t>> q;  // {first chunk, count}
  bool qdone = false;
  std::atomic<int> herr{DSX_OK};
  auto fail = [&](int rc) {
    int ok = DSX_OK;
    herr.compare_exchange_strong(ok, rc);
    qcv.notify_all();
  };
  host_parallel(threads_ + 1 + extra_, [&](int part) {
    if (part == 0) {
      const int rc = produce(s, [&](std::vector<TailChunk>& batch) -> int {
        if (chunks.size() + batch.size() > cap_) return DSX_E_INTERNAL;
        std::sort(batch.begin(), batch.end(),
                  [](const TailChunk& a, const TailChunk& b) { return a.len > b.len; });
        {
          std::lock_guard<std::mutex> g(qm);
          const size_t at = chunks.size();
          chunks.insert(chunks.end(), batch.begin(), batch.end());
          for (uint64_t j = 0; j < batch.size(); j += per)
            q.push_back({at + j, std::min<uint64_t>(per, batch.size() - j)});
        }
        qcv.notify_all();
        return herr.load();
      });
      if (rc) fail(rc);
      {
        std::lock_guard<std::mutex> g(qm);
        qdone = true;
      }
      qcv.notify_all();
      return;
    }
    std::vector<uint8_t> buf;
    if (part > threads_) {  // (the readers' CPUs: only once the reads are done)
      std::unique_lock<std::mutex> lk(qm);
      while (!reads_done_.load() && !qdone && herr.load() == DSX_OK)
        qcv.wait_for(lk, std::chrono::microseconds(200));
    }
    for (;;) {
      std::pair<size_t, uint64_t> g;
      {
        std::unique_lock<std::mutex> lk(qm);
        qcv.wait(lk, [&] { return !q.empty() || qdone || herr.load() != DSX_OK; });
        if (herr.load() != DSX_OK || q.empty()) return;
        g = q.front();
        q.pop_front();
      }
      if (halt_.load(std::memory_order_relaxed) || c_->cancel.load(std::memory_order_relaxed)) {
        fail(DSX_E_INTERRUPTED);
        return;
      }
      const int rc = hash_group(src_, chunks.data() + g.first, g.second, ids.data() + 32 * g.first, buf);
      if (rc) {
        fail(rc);
        return;
      }
    }
  });
  ids.resize(32 * chunks.size());
  if (!err_) err_ = herr.load();
  (void)hipStreamDestroy(s);
}
