// chain_owner_model.cpp -- who owns a context's chain state, on the CPU.
//
// A stand-alone host program over desync_amd/csrc/dsx_chain_owner.h (built
// with -fsanitize=address,undefined by tests/test_host_logic.py).  It plays
// every sequence of up to five events on a context: the chain kinds, a
// neutral call, stream begin / finish / end, shard local / resolve /
// resolve_async / collect, dsx_result and dsx_result with a synchronous redo.
// The machine side does what the library's entry points do around the owner
// (dsx_api.cpp, dsx_index.cpp, dsx_stream.cpp).  The expected side keeps no
// state at all: it answers each event from the history of events and their
// outcomes, by the sentences of the contract in include/dsx.h.  The first
// difference in a code or in the protocol a refusal names is a non-zero exit.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dsx_chain_owner.h"

using namespace dsx_host;

namespace {

enum Ev {
  CUT, CUT_QUEUED, MANY, CUT_HOST, CUT_FD, INDEX_HOST, INDEX_FD,  // chain kinds
  NEUTRAL, STREAM_BEGIN, STREAM_FINISH, STREAM_END, LOCAL, RESOLVE, RESOLVE_ASYNC, COLLECT,
  RESULT, RESULT_REDO, NEV
};
const char* kEvName[NEV] = {"cut", "cut_queued", "many", "cut_host", "cut_fd", "index_host",
                            "index_fd", "neutral", "stream_begin", "stream_finish", "stream_end",
                            "local", "resolve", "resolve_async", "collect", "result", "result_redo"};

struct Outcome {
  int code = DSX_OK;
  std::string proto;  // the protocol a DSX_E_STATE names: "stream", "queued calls", "shard", "" (none)
  bool operator==(const Outcome& o) const { return code == o.code && proto == o.proto; }
};

std::string proto_of(const std::string& why) {
  const size_t k = why.find(": ");
  return k == std::string::npos ? std::string("?") : why.substr(0, k);
}

// ------------------------------------------------------------- the machine
struct Machine {
  ChainOwner owner;
  bool stream_unfinished = false;
  uint32_t queued = 0;

  Outcome chain(ChainKind k) {
    std::string why;
    const int rc = owner.begin(k, ChainView{stream_unfinished, queued}, &why);
    return rc ? Outcome{rc, proto_of(why)} : Outcome{};
  }
  Outcome step(Ev e) {
    std::string why;
    switch (e) {
      case CUT: return chain(ChainKind::kCut);
      case MANY: return chain(ChainKind::kMany);
      case CUT_HOST: return chain(ChainKind::kCutHost);
      case CUT_FD: return chain(ChainKind::kCutFd);
      case INDEX_HOST: return chain(ChainKind::kIndexHost);
      case INDEX_FD: return chain(ChainKind::kIndexFd);
      case CUT_QUEUED: {
        const Outcome o = chain(ChainKind::kCutQueued);
        if (o.code == DSX_OK) ++queued;
        return o;
      }
      case NEUTRAL: return Outcome{};
      case STREAM_BEGIN: {
        const Outcome o = chain(ChainKind::kStreamBegin);
        if (o.code == DSX_OK) stream_unfinished = true;
        return o;
      }
      case STREAM_FINISH: {  // the rest of the input: one more batch, every chunk popped
        if (!stream_unfinished) return Outcome{};
        const Outcome o = chain(ChainKind::kStreamBatch);
        stream_unfinished = false;
        return o;
      }
      case STREAM_END: stream_unfinished = false; return Outcome{};
      case LOCAL: {
        const Outcome o = chain(ChainKind::kShardLocal);
        if (o.code == DSX_OK) owner.shard_ready();
        return o;
      }
      case RESOLVE: {
        const int rc = owner.resolve(&why);
        return rc ? Outcome{rc, proto_of(why)} : Outcome{};
      }
      case RESOLVE_ASYNC: {
        const int rc = owner.resolve(&why);
        if (rc) return Outcome{rc, proto_of(why)};
        owner.resolve_launched();
        return Outcome{};
      }
      case COLLECT: {
        const int rc = owner.collect(&why);
        return rc ? Outcome{rc, proto_of(why)} : Outcome{};
      }
      case RESULT:
      case RESULT_REDO:
        if (!queued) return Outcome{DSX_E_STATE, ""};  // (dsx_result's own: nothing queued)
        --queued;
        return e == RESULT ? Outcome{} : chain(ChainKind::kCut);
      default: return Outcome{DSX_E_INTERNAL, "?"};
    }
  }
};

// ------------------------------------------------- the contract, from history
struct Past {
  Ev e;
  int code;
};

bool is_chain_kind(Ev e) { return e <= INDEX_FD; }

// an event that, accepted, ran a chain on the context other than the shard's own
bool ran_foreign_chain(const Past& p) {
  if (p.code != DSX_OK) return false;
  return is_chain_kind(p.e) || p.e == STREAM_BEGIN || p.e == RESULT_REDO;
}

// "while a stream is unfinished": the last of {accepted begin, finish, end} is a begin
bool stream_open(const std::vector<Past>& h) {
  for (size_t i = h.size(); i-- > 0;) {
    if (h[i].e == STREAM_BEGIN && h[i].code == DSX_OK) return true;
    if (h[i].e == STREAM_FINISH || h[i].e == STREAM_END) return false;
  }
  return false;
}

// queued calls not collected: accepted queued cuts minus the results that found one
uint32_t queue_len(const std::vector<Past>& h) {
  uint32_t q = 0;
  for (const Past& p : h) {
    if (p.e == CUT_QUEUED && p.code == DSX_OK) ++q;
    // (a result pops its call whatever its redo then answers)
    if ((p.e == RESULT || p.e == RESULT_REDO) && q) --q;
  }
  return q;
}

// the last accepted local, or -1
long last_local(const std::vector<Past>& h) {
  for (size_t i = h.size(); i-- > 0;)
    if (h[i].e == LOCAL && h[i].code == DSX_OK) return (long)i;
  return -1;
}

// a local that was let in but ... cannot fail here; a refused local (inside a
// stream) leaves the earlier shard as it was
bool shard_stale(const std::vector<Past>& h, long loc) {
  for (size_t i = (size_t)loc + 1; i < h.size(); ++i)
    if (ran_foreign_chain(h[i])) return true;
  return false;
}

Outcome expected(const std::vector<Past>& h, Ev e) {
  const bool open = stream_open(h);
  const uint32_t q = queue_len(h);
  const long loc = last_local(h);
  if (is_chain_kind(e) || e == LOCAL) return open ? Outcome{DSX_E_STATE, "stream"} : Outcome{};
  switch (e) {
    case NEUTRAL:
    case STREAM_FINISH:
    case STREAM_END: return Outcome{};
    case STREAM_BEGIN:
      if (open) return Outcome{DSX_E_STATE, "stream"};
      if (q) return Outcome{DSX_E_STATE, "queued calls"};
      return Outcome{};
    case RESOLVE:
    case RESOLVE_ASYNC:
      if (loc < 0 || shard_stale(h, loc)) return Outcome{DSX_E_STATE, "shard"};
      return Outcome{};
    case COLLECT: {
      // an accepted resolve_async since the last accepted local, not collected yet
      bool waiting = false;
      for (size_t i = loc < 0 ? h.size() : (size_t)loc + 1; i < h.size(); ++i) {
        if (h[i].e == RESOLVE_ASYNC && h[i].code == DSX_OK) waiting = true;
        if (h[i].e == COLLECT) waiting = false;
      }
      if (!waiting) return Outcome{DSX_E_STATE, "shard"};
      if (shard_stale(h, loc)) return Outcome{DSX_E_STATE, "shard"};
      return Outcome{};
    }
    case RESULT:
      return q ? Outcome{} : Outcome{DSX_E_STATE, ""};
    case RESULT_REDO:
      if (!q) return Outcome{DSX_E_STATE, ""};
      return open ? Outcome{DSX_E_STATE, "stream"} : Outcome{};
    default: return Outcome{DSX_E_INTERNAL, "?"};
  }
}

constexpr int kDepth = 5;
unsigned long long g_seqs = 0, g_steps = 0, g_refused[4] = {};

bool walk(Machine m, std::vector<Past>& h) {
  if ((int)h.size() == kDepth) {
    ++g_seqs;
    return true;
  }
  for (int e = 0; e < NEV; ++e) {
    Machine n = m;
    const Outcome want = expected(h, (Ev)e);
    const Outcome got = n.step((Ev)e);
    ++g_steps;
    if (!(got == want)) {
      std::printf("chain owner model: after");
      for (const Past& p : h) std::printf(" %s(%d)", kEvName[p.e], p.code);
      std::printf(": %s answered %d '%s', the contract says %d '%s'\n", kEvName[e], got.code,
                  got.proto.c_str(), want.code, want.proto.c_str());
      return false;
    }
    if (got.code) {
      const char* names[4] = {"stream", "queued calls", "shard", ""};
      for (int k = 0; k < 4; ++k)
        if (got.proto == names[k]) ++g_refused[k];
    }
    h.push_back(Past{(Ev)e, got.code});
    const bool ok = walk(n, h);
    h.pop_back();
    if (!ok) return false;
  }
  return true;
}

}  // namespace

int main() {
  // the refusals' texts name the kind and the protocol
  {
    ChainOwner o;
    std::string why;
    if (o.begin(ChainKind::kCutHost, ChainView{true, 0}, &why) != DSX_E_STATE ||
        why.find("stream: dsx_cut_host") != 0) {
      std::printf("chain owner model: in-stream text '%s'\n", why.c_str());
      return 1;
    }
    (void)o.begin(ChainKind::kShardLocal, ChainView{}, &why);
    o.shard_ready();
    (void)o.begin(ChainKind::kMany, ChainView{}, &why);
    if (o.resolve(&why) != DSX_E_STATE || why.find("shard: dsx_cut_device_many") != 0 ||
        o.shard() != ChainOwner::Shard::kStale) {
      std::printf("chain owner model: stale text '%s'\n", why.c_str());
      return 1;
    }
  }
  std::vector<Past> h;
  if (!walk(Machine{}, h)) return 1;
  for (int k = 0; k < 3; ++k)
    if (!g_refused[k]) {
      std::printf("chain owner model: a protocol was never refused (%d)\n", k);
      return 1;
    }
  std::printf("chain owner model ok: %llu sequences of %d events, %llu answers; refusals: stream %llu, "
              "queued calls %llu, shard %llu, empty queue %llu\n",
              g_seqs, kDepth, g_steps, g_refused[0], g_refused[1], g_refused[2], g_refused[3]);
  return 0;
}
