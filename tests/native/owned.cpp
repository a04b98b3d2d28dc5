// The owners of eskf_lio_amd/csrc/vgicp_owned.h over a counting backend: every block and event that the backend hands
// out is kept in a ledger, an allocation can be made to fail on demand, and every call is written to a trace, so the
// ORDER of a regrow (free first, then allocate) can be asserted.  Prints "ok <cases>"; tests/test_owned_cpu.py runs it
// plain and under the address / undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>

#include "vgicp_owned.h"

namespace {

struct Counting {
  using error = int;
  static constexpr error ok = 0;
  using event = int*;
  using stream = long*;
  static inline std::set<void*> live;
  static inline std::string trace;      // 'A' allocation requested, 'F' free, 'a' alias requested
  static inline int requests = 0;       // allocations and creations requested so far
  static inline int fail_at = 0;        // the request with this number fails (0: none)
  static inline int aliases = 0;
  static inline bool alias_fails = false;

  static error make(void** out, size_t bytes) {
    trace += 'A';
    if (++requests == fail_at) return 2;
    *out = std::malloc(bytes ? bytes : 1);
    live.insert(*out);
    return ok;
  }
  static void drop(void* p) {
    trace += 'F';
    if (live.erase(p) != 1) { std::printf("FAIL: free of a block that is not live\n"); std::exit(1); }
    std::free(p);
  }
  static error device_alloc(void** out, size_t bytes, bool) { return make(out, bytes); }
  static void device_free(void* p) { drop(p); }
  static error pinned_alloc(void** out, size_t bytes) { return make(out, bytes); }
  static void pinned_free(void* p) { drop(p); }
  static error pinned_alias(void** dev, void* host) {
    trace += 'a';
    ++aliases;
    if (alias_fails) return 3;
    *dev = static_cast<char*>(host) + 1;   // any address that is not the host's
    return ok;
  }
  static error event_create(event* e, bool) { void* p = nullptr; const error rc = make(&p, sizeof(int)); if (rc == ok) *e = static_cast<int*>(p); return rc; }
  static void event_destroy(event e) { drop(e); }
  static error stream_create(stream* s) { void* p = nullptr; const error rc = make(&p, sizeof(long)); if (rc == ok) *s = static_cast<long*>(p); return rc; }
  static void stream_destroy(stream s) { drop(s); }
  static void begin() { trace.clear(); requests = fail_at = aliases = 0; alias_fails = false; }
};

template <class T> using Dev = vgicp::owned::DeviceBuf<T, Counting>;
template <class T> using Pin = vgicp::owned::PinnedBuf<T, Counting>;
using Event = vgicp::owned::EventHandle<Counting>;
using Stream = vgicp::owned::StreamHandle<Counting>;

int cases = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)
void begin_case() { CHECK(Counting::live.empty()); Counting::begin(); ++cases; }

// the create_context shape: the stream first, then buffers and events in the order they are filled
struct Eight {
  Stream stream;
  Dev<double> a;
  Pin<int> b;
  Dev<void> c;
  Pin<double> d;
  Event e;
  Dev<char> f;
  Event g;
  int fill() {
    int rc;
    if ((rc = stream.create()) != 0) return rc;
    if ((rc = a.alloc(64)) != 0) return rc;
    if ((rc = b.alloc(64)) != 0) return rc;
    if ((rc = c.alloc(64, true)) != 0) return rc;
    if ((rc = d.alloc_mapped(64)) != 0) return rc;
    if ((rc = e.create()) != 0) return rc;
    if ((rc = f.alloc(64)) != 0) return rc;
    return g.create(false);
  }
};

template <class Buf> void buffer_cases() {
  {  // allocate, then regrow: the old block is freed exactly once, BEFORE the new allocation is requested
    begin_case();
    Buf b;
    CHECK(!b && b.get() == nullptr && b.bytes() == 0);
    CHECK(b.alloc(100) == 0 && b && b.bytes() == 100 && Counting::live.size() == 1);
    auto* first = b.get();
    CHECK(Counting::live.count(first) == 1);
    CHECK(b.alloc(200) == 0 && b.bytes() == 200 && Counting::live.size() == 1);
    CHECK(Counting::trace == "AFA");
    b.reset();
    b.reset();
    CHECK(Counting::trace == "AFAF" && !b && b.bytes() == 0);
  }
  {  // a failed regrow leaves the owner empty and nothing live
    begin_case();
    Buf b;
    CHECK(b.alloc(100) == 0);
    Counting::fail_at = 2;
    CHECK(b.alloc(200) == 2 && !b && b.bytes() == 0 && Counting::live.empty() && Counting::trace == "AFA");
  }
  {  // move construction, move assignment onto an empty and onto a non-empty owner, self-move
    begin_case();
    Buf a;
    CHECK(a.alloc(10) == 0);
    auto* pa = a.get();
    Buf b(std::move(a));
    CHECK(!a && a.bytes() == 0 && b.get() == pa && b.bytes() == 10 && Counting::live.size() == 1);
    Buf c;
    c = std::move(b);
    CHECK(!b && c.get() == pa && Counting::trace == "A");
    Buf d;
    CHECK(d.alloc(20) == 0 && Counting::live.size() == 2);
    d = std::move(c);   // d's own block goes, c's arrives
    CHECK(!c && d.get() == pa && d.bytes() == 10 && Counting::live.size() == 1 && Counting::trace == "AAF");
    Buf& self = d;
    d = std::move(self);
    CHECK(d.get() == pa && d.bytes() == 10 && Counting::live.size() == 1 && Counting::trace == "AAF");
  }
  {  // release() leaves the block live and the owner empty
    begin_case();
    void* kept = nullptr;
    {
      Buf b;
      CHECK(b.alloc(10) == 0);
      kept = b.release();
      CHECK(!b && b.bytes() == 0);
    }
    CHECK(Counting::live.size() == 1 && Counting::live.count(kept) == 1 && Counting::trace == "A");
    Counting::drop(kept);
  }
}

}  // namespace

int main() {
  buffer_cases<Dev<double>>();
  buffer_cases<Pin<double>>();
  {  // a device owner of untyped memory converts like the raw pointer it replaces
    begin_case();
    Dev<void> v;
    Dev<unsigned> w;
    CHECK(v.alloc(16) == 0 && w.alloc(64) == 0);
    void* raw = v;
    unsigned* third = w + 3;
    CHECK(raw == v.get() && third == w.get() + 3 && &w[3] == third);
  }
  for (int k = 1; k <= 8; ++k) {  // eight owners filled in order: failing allocation k leaves nothing once the struct goes
    begin_case();
    {
      Eight s;
      Counting::fail_at = k;
      CHECK(s.fill() == 2);
      CHECK((int)Counting::live.size() == k - 1);
    }
    CHECK(Counting::live.empty());
  }
  {  // ... and all eight live until then
    begin_case();
    {
      Eight s;
      CHECK(s.fill() == 0 && Counting::live.size() == 8);
    }
    CHECK(Counting::live.empty());
  }
  {  // the device alias of a pinned owner: requested once, cleared by reset(), moved with the block
    begin_case();
    Pin<char> p;
    CHECK(p.alloc(32) == 0 && p.dev() == nullptr && Counting::aliases == 0);
    CHECK(p.alloc_mapped(32) == 0 && Counting::aliases == 1 && p.dev() == p.get() + 1);
    CHECK(p.dev() == p.get() + 1 && p.dev() == p.get() + 1 && Counting::aliases == 1);
    Pin<char> q(std::move(p));
    CHECK(p.dev() == nullptr && q.dev() == q.get() + 1 && Counting::aliases == 1);
    q.reset();
    CHECK(q.dev() == nullptr && q.get() == nullptr);
    Counting::alias_fails = true;   // no alias: no block either
    CHECK(q.alloc_mapped(32) == 3 && !q && q.dev() == nullptr && Counting::live.empty());
  }
  {  // events: create, destroy, double reset(), re-creation, move, release
    begin_case();
    Event e;
    CHECK(!e && e.create() == 0 && e && Counting::live.size() == 1);
    e.reset();
    e.reset();
    CHECK(!e && Counting::live.empty() && Counting::trace == "AF");
    CHECK(e.create(false) == 0 && e.create() == 0 && Counting::live.size() == 1 && Counting::trace == "AFAFA");
    Event f(std::move(e));
    CHECK(!e && f);
    Event g;
    CHECK(g.create() == 0);
    g = std::move(f);
    CHECK(!f && g && Counting::live.size() == 1);
    Counting::fail_at = Counting::requests + 1;
    CHECK(g.create() == 2 && !g && Counting::live.empty());
    CHECK(g.create() == 0);
    int* kept = g.release();
    CHECK(!g && Counting::live.count(kept) == 1);
    Counting::drop(kept);
  }
  {  // the stream: the same shape
    begin_case();
    {
      Stream s;
      CHECK(!s && s.create() == 0 && s && Counting::live.size() == 1);
      Stream t(std::move(s));
      CHECK(!s && t);
    }
    CHECK(Counting::live.empty());
  }
  CHECK(Counting::live.empty());
  std::printf("ok %d\n", cases);
  return 0;
}
