// Stand-alone probe of csrc/dev_mem.h for tests/test_dev_mem.py: no HIP runtime, no GPU, never loaded into python.
// The few runtime entry points the header calls are defined HERE, over malloc: they keep the set of live handles by kind, abort on
// a free of something that is not live (a double free, or a block given back to the wrong call), can be told to fail the k-th
// allocation from now, and count the stream waits.  `dev_mem_probe` lists the cases; `dev_mem_probe CASE` runs one and exits 0
// if every check held and nothing is live at the end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../cuda_ray_tracer_amd/csrc/dev_mem.h"

namespace {

enum Kind { DEVICE, PINNED, EVENT, STREAM, KINDS };
std::set<void*> live[KINDS];
int allocations = 0, fail_at = 0;      // fail_at = k > 0: the k-th allocation from now fails
int stream_waits = 0, frees = 0;
std::string last_error;

hipError_t take(Kind k, void** out, size_t bytes, hipError_t failure)
{
  ++allocations;
  if (fail_at > 0 && --fail_at == 0) { *out = (void*)0x1; return failure; }      // (what a failed call leaves in *out must not be kept)
  if (bytes == 0) { fprintf(stderr, "probe: zero-byte allocation reached the runtime\n"); abort(); }
  void* p = malloc(bytes);
  if (!p) abort();
  memset(p, 0xa5, bytes);
  live[k].insert(p);
  *out = p;
  return hipSuccess;
}

hipError_t give(Kind k, void* p)
{
  if (live[k].erase(p) != 1) { fprintf(stderr, "probe: free of %p, which is not live as kind %d\n", p, (int)k); abort(); }
  ++frees;
  free(p);
  return hipSuccess;
}

size_t live_total() { return live[DEVICE].size() + live[PINNED].size() + live[EVENT].size() + live[STREAM].size(); }

} // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return take(DEVICE, p, bytes, hipErrorOutOfMemory); }
hipError_t hipFree(void* p) { return give(DEVICE, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return take(PINNED, p, bytes, hipErrorOutOfMemory); }
hipError_t hipHostFree(void* p) { return give(PINNED, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return take(EVENT, (void**)e, 1, hipErrorInvalidValue); }
hipError_t hipEventDestroy(hipEvent_t e) { return give(EVENT, (void*)e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return take(STREAM, (void**)s, 1, hipErrorInvalidValue); }
hipError_t hipStreamDestroy(hipStream_t s) { return give(STREAM, (void*)s); }
hipError_t hipStreamSynchronize(hipStream_t) { ++stream_waits; return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

namespace mirt {
void set_error(const std::string& s) { last_error = s; }
int hip_fail(hipError_t e, const char* what, const char* file, int line)
{
  char buf[512];
  snprintf(buf, sizeof(buf), "HIP error in %s at line %d: %s (%s)", file, line, hipGetErrorString(e), what);
  set_error(buf);
  return MIRT_ERR_HIP;
}
} // namespace mirt

namespace {

using namespace mirt;

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

template <class B>
bool holds(const B& b, Kind k, size_t cap) { return b.get() && b.cap() == cap && live[k].count(b.get()) == 1; }
template <class B>
bool empty(const B& b) { return b.get() == nullptr && b.cap() == 0; }

// grow below, at and above capacity
template <class B>
void grow_case(Kind k)
{
  B b;
  CHECK(b.alloc(100) == MIRT_OK && holds(b, k, 100) && live[k].size() == 1);
  b.get()[99] = 7;      // (the last element is the block's: the sanitizer sees a short one)
  auto* const p = b.get();
  const int waits = stream_waits, allocs = allocations, freed = frees;
  CHECK(b.grow(99, nullptr) == MIRT_OK && b.get() == p && b.cap() == 100);
  CHECK(b.grow(100, nullptr) == MIRT_OK && b.get() == p && b.cap() == 100);
  CHECK(b.grow(0, nullptr) == MIRT_OK && b.get() == p && b.cap() == 100);
  CHECK(stream_waits == waits && allocations == allocs && frees == freed);      // kept, no wait
  CHECK(b.grow(101, nullptr) == MIRT_OK && holds(b, k, 101));
  b.get()[100] = 7;
  CHECK(stream_waits == waits + 1 && allocations == allocs + 1 && frees == freed + 1);
  CHECK(live[k].count(p) == 0 && live[k].size() == 1);                          // the old block went back
  B fresh;
  CHECK(fresh.grow(0, nullptr) == MIRT_OK && empty(fresh) && stream_waits == waits + 1);
  CHECK(fresh.grow(5, nullptr) == MIRT_OK && holds(fresh, k, 5) && stream_waits == waits + 2);
}

// a failed alloc and a failed grow; the raw form reports nothing
template <class B>
void failure_case(Kind k)
{
  B b;
  CHECK(b.alloc(10) == MIRT_OK);
  fail_at = 1; last_error.clear();
  CHECK(b.alloc(20) == MIRT_ERR_HIP && empty(b) && live[k].empty());
  CHECK(last_error.find("out of memory") != std::string::npos);
  CHECK(b.alloc(10) == MIRT_OK && holds(b, k, 10));      // usable again
  const int waits = stream_waits;
  fail_at = 1; last_error.clear();
  CHECK(b.grow(11, nullptr) == MIRT_ERR_HIP && empty(b) && live[k].empty() && stream_waits == waits + 1);
  CHECK(!last_error.empty());
  CHECK(b.alloc_raw(10) == hipSuccess && holds(b, k, 10));
  fail_at = 1; last_error.clear();
  CHECK(b.alloc_raw(20) == hipErrorOutOfMemory && empty(b) && live[k].empty());
  CHECK(last_error.empty());                              // raw: the status, no message
  // the second of two allocations fails: the first is still owned, and goes back with its owner
  {
    B first, second;
    fail_at = 2;
    CHECK(first.alloc(4) == MIRT_OK && second.alloc(4) == MIRT_ERR_HIP);
    CHECK(holds(first, k, 4) && empty(second) && live[k].size() == 1);
  }
  CHECK(live[k].empty());
}

template <class B>
void move_case(Kind k)
{
  B a;
  CHECK(a.alloc(8) == MIRT_OK);
  auto* const pa = a.get();
  B b(std::move(a));                                      // move construction
  CHECK(empty(a) && b.get() == pa && b.cap() == 8 && live[k].size() == 1);
  B c;
  CHECK(c.alloc(3) == MIRT_OK);
  auto* const pc = c.get();
  c = std::move(b);                                       // move assignment: the target's old block is freed
  CHECK(empty(b) && c.get() == pa && c.cap() == 8 && live[k].count(pc) == 0 && live[k].size() == 1);
  B& self = c;
  c = std::move(self);                                    // onto itself: kept
  CHECK(c.get() == pa && c.cap() == 8 && live[k].size() == 1);
  B d;
  c = std::move(d);                                       // an empty source empties the target
  CHECK(empty(c) && empty(d) && live[k].empty());
}

template <class B>
void reset_case(Kind k)
{
  { B never; CHECK(empty(never)); }                       // destruction of an empty object
  B b;
  b.reset();                                              // reset of an empty object
  CHECK(b.alloc(5) == MIRT_OK);
  b.reset();
  CHECK(empty(b) && live[k].empty());
  b.reset();                                              // twice
  CHECK(empty(b) && live[k].empty());
  const int allocs = allocations;
  CHECK(b.alloc(5) == MIRT_OK && b.alloc(0) == MIRT_OK);  // zero length: frees, stays empty, asks the runtime for nothing
  CHECK(empty(b) && live[k].empty() && allocations == allocs + 1);
  CHECK(b.alloc_raw(0) == hipSuccess && empty(b) && allocations == allocs + 1);
  { B scoped; CHECK(scoped.alloc(2) == MIRT_OK && live[k].size() == 1); }
  CHECK(live[k].empty());                                 // the destructor frees
}

void conversion_case()
{
  DevBuf<int> b;
  CHECK(!b);
  CHECK(b.alloc(4) == MIRT_OK);
  int* p = b;                                             // what `a.samples = cx.samples;` and a kernel launch rely on
  const int* q = b + 1;
  CHECK(p == b.get() && q == p + 1 && b);
  b[2] = 5; *b = 6;
  CHECK(p[2] == 5 && p[0] == 6);
}

void event_case()
{
  {
    Event e;
    CHECK((hipEvent_t)e == nullptr && !e);
    CHECK(e.create() == MIRT_OK && e && live[EVENT].size() == 1);
    const hipEvent_t h = e;
    CHECK(e.create(hipEventDisableTiming) == MIRT_OK && (hipEvent_t)e == h && live[EVENT].size() == 1);      // twice: one event
    Event f(std::move(e));
    CHECK(!e && (hipEvent_t)f == h && live[EVENT].size() == 1);
    Event g;
    CHECK(g.create() == MIRT_OK && live[EVENT].size() == 2);
    g = std::move(f);
    CHECK(!f && (hipEvent_t)g == h && live[EVENT].size() == 1);
    fail_at = 1; last_error.clear();
    Event bad;
    CHECK(bad.create() == MIRT_ERR_HIP && !bad && !last_error.empty());
    CHECK(bad.create() == MIRT_OK && bad);
  }
  CHECK(live[EVENT].empty());
  // a vector that grows past several reallocations destroys each event exactly once (a second destroy aborts in give())
  const int freed = frees;
  {
    std::vector<Event> v;
    size_t moves = 0, cap = v.capacity();
    for (int i = 0; i < 100; ++i) {
      Event e;
      CHECK(e.create() == MIRT_OK);
      v.push_back(std::move(e));
      if (v.capacity() != cap) { cap = v.capacity(); ++moves; }
    }
    CHECK(moves >= 3 && live[EVENT].size() == 100 && frees == freed);
    std::set<void*> distinct;
    for (const Event& e : v) distinct.insert((void*)(hipEvent_t)e);
    CHECK(distinct == live[EVENT]);
  }
  CHECK(live[EVENT].empty() && frees == freed + 100);
}

bool names(int line, const char* what);

void stream_case()
{
  {
    Stream s;
    CHECK((hipStream_t)s == nullptr && !s);
    CHECK(s.create(hipStreamNonBlocking) == MIRT_OK && s && live[STREAM].size() == 1);
    const hipStream_t h = s;
    CHECK(s.create(hipStreamDefault) == MIRT_OK && (hipStream_t)s == h && live[STREAM].size() == 1);      // twice: one stream
    Stream f(std::move(s));
    CHECK(!s && (hipStream_t)f == h && live[STREAM].size() == 1);
    Stream g;
    CHECK(g.create(hipStreamNonBlocking) == MIRT_OK && live[STREAM].size() == 2);
    const hipStream_t old = g;
    g = std::move(f);                                       // move assignment: the target's old stream is destroyed
    CHECK(!f && (hipStream_t)g == h && live[STREAM].count((void*)old) == 0 && live[STREAM].size() == 1);
    g.reset();
    CHECK(!g && live[STREAM].empty());
    g.reset();                                              // twice
    { Stream never; CHECK(!never); }                        // destruction of an empty object
    CHECK(live[STREAM].empty());
    fail_at = 1; last_error.clear();
    Stream bad;
    const int line = __LINE__ + 1;
    CHECK(bad.create(hipStreamNonBlocking) == MIRT_ERR_HIP && !bad);
    CHECK(names(line, "hipStreamCreateWithFlags"));
    CHECK(bad.create(hipStreamNonBlocking) == MIRT_OK && bad);
  }
  CHECK(live[STREAM].empty());
  // a vector sized once (as a slot's are) and one grown past several reallocations: each stream is destroyed exactly once
  const int freed = frees;
  {
    std::vector<Stream> sized(7), v;
    for (Stream& s : sized) CHECK(s.create(hipStreamNonBlocking) == MIRT_OK);
    for (int i = 0; i < 100; ++i) {
      Stream s;
      CHECK(s.create(hipStreamNonBlocking) == MIRT_OK);
      v.push_back(std::move(s));
    }
    CHECK(live[STREAM].size() == 107 && frees == freed);
    std::set<void*> distinct;
    for (const Stream& s : sized) distinct.insert((void*)(hipStream_t)s);
    for (const Stream& s : v) distinct.insert((void*)(hipStream_t)s);
    CHECK(distinct == live[STREAM]);
  }
  CHECK(live[STREAM].empty() && frees == freed + 107);
}

// Four buffers of one length whose LAST capacity stands for all four, as the chunk orders and their cost buffer are kept
// (chunk_order_find, render.hip): all are reset before the first is allocated, so whichever allocation fails, that capacity is 0.
int four_together(DevBuf<int>& cost, DevBuf<int> (&out)[3], size_t n)
{
  if (out[2].cap() >= n) return MIRT_OK;
  cost.reset();
  for (DevBuf<int>& o : out) o.reset();
  if (const int rc = cost.alloc(n)) return rc;
  for (DevBuf<int>& o : out) if (const int rc = o.alloc(n)) return rc;
  return MIRT_OK;
}

// the k-th of the four fails, then a smaller request: it must allocate again, never find a null buffer behind a stale capacity
void together_case()
{
  for (int k = 1; k <= 4; ++k) {
    DevBuf<int> cost, out[3];
    CHECK(four_together(cost, out, 100) == MIRT_OK && live[DEVICE].size() == 4);
    fail_at = k;
    CHECK(four_together(cost, out, 200) == MIRT_ERR_HIP);
    CHECK(out[2].cap() == 0 && live[DEVICE].size() == (size_t)(k - 1));      // nothing of the old four is left, the new ones before k are owned
    fail_at = 0;
    CHECK(four_together(cost, out, 50) == MIRT_OK && live[DEVICE].size() == 4);
    CHECK(holds(cost, DEVICE, 50) && holds(out[0], DEVICE, 50) && holds(out[1], DEVICE, 50) && holds(out[2], DEVICE, 50));
  }
  CHECK(live[DEVICE].empty());
}

// a failure's message names the file and line of the call, and the caller's label where it gave one
bool names(int line, const char* what)
{
  const std::string at = "dev_mem_probe.cpp at line " + std::to_string(line) + ":", label = std::string("(") + what + ")";
  return last_error.find(at) != std::string::npos && last_error.find(label) != std::string::npos && last_error.find("dev_mem.h") == std::string::npos;
}

void message_case()
{
  DevBuf<int> d; PinnedBuf<int> h; Event e;
  int line;
  fail_at = 1; line = __LINE__ + 1;
  CHECK(d.alloc(4) == MIRT_ERR_HIP);
  CHECK(names(line, "hipMalloc"));
  fail_at = 1; line = __LINE__ + 1;
  CHECK(d.alloc(4, "heap") == MIRT_ERR_HIP);
  CHECK(names(line, "hipMalloc(heap)"));
  fail_at = 1; line = __LINE__ + 1;
  CHECK(h.grow(4, nullptr) == MIRT_ERR_HIP);
  CHECK(names(line, "hipHostMalloc"));
  fail_at = 1; line = __LINE__ + 1;
  CHECK(d.grow(4, nullptr, "samples") == MIRT_ERR_HIP);
  CHECK(names(line, "hipMalloc(samples)"));
  fail_at = 1; line = __LINE__ + 1;
  CHECK(e.create() == MIRT_ERR_HIP);
  CHECK(names(line, "hipEventCreate"));
}

struct Case { const char* name; void (*run)(); };
const Case CASES[] = {
  {"grow_device", [] { grow_case<DevBuf<int>>(DEVICE); }}, {"grow_pinned", [] { grow_case<PinnedBuf<int>>(PINNED); }},
  {"failure_device", [] { failure_case<DevBuf<double>>(DEVICE); }}, {"failure_pinned", [] { failure_case<PinnedBuf<double>>(PINNED); }},
  {"move_device", [] { move_case<DevBuf<char>>(DEVICE); }}, {"move_pinned", [] { move_case<PinnedBuf<char>>(PINNED); }},
  {"reset_device", [] { reset_case<DevBuf<int>>(DEVICE); }}, {"reset_pinned", [] { reset_case<PinnedBuf<int>>(PINNED); }},
  {"conversion", conversion_case}, {"event", event_case}, {"stream", stream_case}, {"together", together_case}, {"message", message_case},
};

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) { for (const Case& c : CASES) puts(c.name); return 0; }
  for (const Case& c : CASES) {
    if (strcmp(c.name, argv[1]) != 0) continue;
    c.run();
    if (live_total() != 0) { fprintf(stderr, "%zu handles still live at exit\n", live_total()); ++failures; }
    printf("%s: %d allocations, %d frees, %d stream waits, %d failures\n", c.name, allocations, frees, stream_waits, failures);
    return failures ? 1 : 0;
  }
  fprintf(stderr, "no such case: %s\n", argv[1]);
  return 2;
}
