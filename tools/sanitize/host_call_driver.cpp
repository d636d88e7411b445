// host_call_driver.cpp -- CPU driver of the staging that every host-array
// entry point of libfdcn shares (finite_difference_amd/csrc/fdcn_host_call.h)
// for the sanitizer build (`make host_call`: AddressSanitizer with its leak
// check + UndefinedBehaviorSanitizer, first report aborts).  The library
// instantiates the helper over hipMallocAsync / hipMemcpyAsync on the calling
// thread's stream; here over malloc / memcpy, with a backend that can fail
// any of its calls.  No GPU test can reach those failure paths, so this is
// where "freed exactly once, synchronised before return, first message kept"
// is checked: the region layout, the round trip of every byte, a failure
// injected at every backend call of a staged call and at its launch, and the
// scoped workspace of the `_dev` entry points.  Exit 0 = clean.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../finite_difference_amd/csrc/fdcn_host_call.h"

namespace {

#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      fprintf(stderr, "host_call_driver: %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

// what the backend saw since reset()
struct Trace {
  std::vector<char> steps;  // 'o'pen 'a'lloc 'i'n 'x' out 'f'ree 's'ync, in call order
  std::set<int> fail_at;    // 1-based positions in `steps` that fail
  int allocs = 0, frees = 0, syncs = 0, fails = 0;
  std::string msg;          // the last message recorded
  std::string first_msg;    // the first
  void* live = nullptr;     // the block handed out and not yet released
} g;

void reset(std::set<int> fail_at = {}) {
  CHECK(g.live == nullptr);
  g = Trace();
  g.fail_at = std::move(fail_at);
}

bool fails_now(char step) {
  g.steps.push_back(step);
  return g.fail_at.count((int)g.steps.size()) != 0;
}

struct Fake {
  using Stream = int;
  static constexpr int kStream = 7;
  static int open(int* s) {
    if (fails_now('o')) return fail(FDCN_ENODEV, "no HIP device visible");
    *s = kStream;
    return FDCN_OK;
  }
  static const char* alloc(void** p, size_t n, int s) {
    CHECK(s == kStream && n > 0 && n % 256 == 0 && g.live == nullptr);
    if (fails_now('a')) return "injected: out of memory";
    *p = aligned_alloc(256, n);
    CHECK(*p != nullptr);
    memset(*p, 0xA5, n);
    g.live = *p;
    ++g.allocs;
    return nullptr;
  }
  static const char* release(void* p, int s) {
    CHECK(s == kStream && p != nullptr && p == g.live);
    free(p);  // an injected failure still gives the block back: nothing may leak
    g.live = nullptr;
    ++g.frees;
    return fails_now('f') ? "injected: free" : nullptr;
  }
  static const char* copy_in(void* dev, const void* host, size_t n, int s) {
    CHECK(s == kStream && dev && host && n > 0 && g.live);
    if (fails_now('i')) return "injected: copy in";
    memcpy(dev, host, n);
    return nullptr;
  }
  static const char* copy_out(void* host, const void* dev, size_t n, int s) {
    CHECK(s == kStream && dev && host && n > 0 && g.live);
    if (fails_now('x')) return "injected: copy out";
    memcpy(host, dev, n);
    return nullptr;
  }
  static const char* sync(int s) {
    CHECK(s == kStream);
    ++g.syncs;
    return fails_now('s') ? "injected: sync" : nullptr;
  }
  static int fail(int code, const char* msg) {
    if (g.fails++ == 0) g.first_msg = msg;
    g.msg = msg;
    return code;
  }
};

using Call = fdcn_call::HostCall<Fake>;

std::vector<unsigned char> pattern(size_t n, unsigned seed) {
  std::vector<unsigned char> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (unsigned char)((i * 131u + seed * 29u + 7u) & 0xff);
  return v;
}

// One staged call in the shape of the library's: region sizes that are no
// multiple of 256 B, an optional input and an optional output present or
// absent, monitor-style inputs (room for one entry, copied when n_mon > 0)
// and scratch.  `launch_rc` is what the launch returns (it reports its own
// failure, as the library's launches do).
struct Scenario {
  bool with_opt_in, with_opt_out;
  int n_mon;
  int launch_rc;
};

constexpr unsigned char kUntouched = 0x5C;

struct Result {
  int rc;
  bool launched;
  std::vector<unsigned char> out0, out1;
};

Result staged_call(const Scenario& sc) {
  const std::vector<unsigned char> a = pattern(40, 1), b = pattern(257, 2), opt = pattern(1000, 3);
  const std::vector<unsigned char> mon = pattern(4 * (size_t)(sc.n_mon > 0 ? sc.n_mon : 1), 4);
  Result r{FDCN_OK, false, std::vector<unsigned char>(513, kUntouched),
           std::vector<unsigned char>(24, kUntouched)};
  const size_t mon_bytes = 4 * (size_t)sc.n_mon, mon_room = 4 * (size_t)(sc.n_mon > 0 ? sc.n_mon : 1);
  const size_t scratch = 777;

  Call c("driver_call");
  r.rc = c.open();
  if (r.rc) return r;
  const int rA = c.in(a.data(), a.size());
  const int rB = c.in(b.data(), b.size());
  const int rO0 = c.out(r.out0.data(), r.out0.size());
  const int rOpt = c.in(sc.with_opt_in ? opt.data() : nullptr, opt.size());
  // without monitors the caller may pass no array at all: the region stays
  const int rM = c.in(sc.n_mon > 0 ? mon.data() : nullptr, mon_bytes, mon_room);
  const int rO1 = c.out(sc.with_opt_out ? r.out1.data() : nullptr, r.out1.size());
  const int rW = c.scratch(scratch);

  // layout: aligned, in declaration order, disjoint; absent regions take no room
  struct Span {
    int id;
    size_t room;
    bool present;
  };
  const Span spans[] = {{rA, a.size(), true},          {rB, b.size(), true},
                        {rO0, r.out0.size(), true},    {rOpt, opt.size(), sc.with_opt_in},
                        {rM, mon_room, true},          {rO1, r.out1.size(), sc.with_opt_out},
                        {rW, scratch, true}};
  size_t end = 0;
  for (const Span& s : spans) {
    if (!s.present) continue;
    CHECK(c.offset(s.id) % 256 == 0);
    CHECK(c.offset(s.id) >= end);
    end = c.offset(s.id) + s.room;
  }
  CHECK(c.block_bytes() >= end && c.block_bytes() % 256 == 0);
  CHECK(c.offset(rA) == 0 && c.offset(rB) == 256 && c.offset(rO0) == 768);

  r.rc = c.run([&](int stream) {
    r.launched = true;
    CHECK(stream == Fake::kStream);
    unsigned char* base = c.dev<unsigned char>(rA);
    CHECK(base == g.live && ((uintptr_t)base & 255) == 0);
    for (const Span& s : spans) {
      unsigned char* p = c.dev<unsigned char>(s.id);
      CHECK((p != nullptr) == s.present);
      if (p) CHECK(p == base + c.offset(s.id) && ((uintptr_t)p & 255) == 0);
    }
    // inputs arrived byte-exact, and only they were copied
    CHECK(memcmp(c.dev<unsigned char>(rA), a.data(), a.size()) == 0);
    CHECK(memcmp(c.dev<unsigned char>(rB), b.data(), b.size()) == 0);
    CHECK(c.dev<unsigned char>(rB)[b.size()] == 0xA5);
    if (sc.with_opt_in) CHECK(memcmp(c.dev<unsigned char>(rOpt), opt.data(), opt.size()) == 0);
    if (sc.n_mon > 0) CHECK(memcmp(c.dev<unsigned char>(rM), mon.data(), mon_bytes) == 0);
    else CHECK(c.dev<unsigned char>(rM)[0] == 0xA5);
    CHECK(c.dev<unsigned char>(rO0)[0] == 0xA5);
    memset(c.dev<unsigned char>(rW), 1, scratch);  // every scratch byte is writable
    if (sc.launch_rc) return Fake::fail(sc.launch_rc, "driver_call: launch failed");
    const std::vector<unsigned char> o0 = pattern(r.out0.size(), 8), o1 = pattern(r.out1.size(), 9);
    memcpy(c.dev<unsigned char>(rO0), o0.data(), o0.size());
    if (sc.with_opt_out) memcpy(c.dev<unsigned char>(rO1), o1.data(), o1.size());
    return FDCN_OK;
  });
  return r;
}

bool untouched(const std::vector<unsigned char>& v) {
  for (unsigned char x : v)
    if (x != kUntouched) return false;
  return true;
}

void test_round_trip() {
  for (int mask = 0; mask < 8; ++mask) {
    const Scenario sc{(mask & 1) != 0, (mask & 2) != 0, (mask & 4) ? 3 : 0, FDCN_OK};
    reset();
    const Result r = staged_call(sc);
    CHECK(r.rc == FDCN_OK && r.launched && g.fails == 0);
    CHECK(r.out0 == pattern(r.out0.size(), 8));
    CHECK(sc.with_opt_out ? r.out1 == pattern(r.out1.size(), 9) : untouched(r.out1));
    CHECK(g.allocs == 1 && g.frees == 1 && g.syncs == 1);
    // open, allocate, copies in, (launch), copies out, free, synchronise
    std::string want = "oaii";
    if (sc.with_opt_in) want += 'i';
    if (sc.n_mon > 0) want += 'i';
    want += 'x';
    if (sc.with_opt_out) want += 'x';
    want += "fs";
    CHECK(std::string(g.steps.begin(), g.steps.end()) == want);
  }
}

void test_injection() {
  const Scenario sc{true, true, 3, FDCN_OK};
  reset();
  CHECK(staged_call(sc).rc == FDCN_OK);
  const std::vector<char> clean = g.steps;  // o a i i i i x x f s
  CHECK(clean.size() == 10);
  for (int k = 1; k <= (int)clean.size(); ++k) {
    reset({k});
    const Result r = staged_call(sc);
    const char step = clean[(size_t)k - 1];
    const char* text = "";
    int code = FDCN_EHIP;
    switch (step) {
      case 'o': code = FDCN_ENODEV; text = "no HIP device visible"; break;
      case 'a': code = FDCN_ENOMEM; text = "driver_call: allocation failed: injected: out of memory"; break;
      case 'i': text = "driver_call: copy to the device failed: injected: copy in"; break;
      case 'x': text = "driver_call: copy from the device failed: injected: copy out"; break;
      case 'f': text = "driver_call: free failed: injected: free"; break;
      case 's': text = "driver_call: kernel / copies failed: injected: sync"; break;
    }
    CHECK(r.rc == code);
    CHECK(g.fails == 1 && g.msg == text);
    const bool block = step != 'o' && step != 'a';
    CHECK(g.allocs == (block ? 1 : 0) && g.frees == g.allocs && g.syncs == g.allocs);
    CHECK(g.live == nullptr);
    CHECK(r.launched == (block && step != 'i'));
    if (!r.launched) CHECK(untouched(r.out0) && untouched(r.out1));
    if (step == 'x' && k == 7) CHECK(untouched(r.out0) && untouched(r.out1));  // stops at the first
    if (step == 'i') CHECK((int)g.steps.size() == k + 2);  // then only free and synchronise
  }

  // a launch that fails: its code and message, no copy out, block freed, stream drained
  reset();
  Scenario bad = sc;
  bad.launch_rc = FDCN_EINVAL;
  Result r = staged_call(bad);
  CHECK(r.rc == FDCN_EINVAL && r.launched && g.fails == 1);
  CHECK(g.msg == "driver_call: launch failed");
  CHECK(untouched(r.out0) && untouched(r.out1));
  CHECK(g.allocs == 1 && g.frees == 1 && g.syncs == 1);
  CHECK(std::string(g.steps.begin(), g.steps.end()) == "oaiiiifs");

  // ... and a later failure of the free and the synchronise does not replace it
  reset({7, 8});
  r = staged_call(bad);
  CHECK(r.rc == FDCN_EINVAL && g.fails == 1 && g.first_msg == "driver_call: launch failed");
  CHECK(untouched(r.out0) && untouched(r.out1));
  CHECK(g.allocs == 1 && g.frees == 1 && g.syncs == 1);

  // a failed copy in followed by a failed synchronise: the copy's message
  reset({3, 5});
  r = staged_call(sc);
  CHECK(r.rc == FDCN_EHIP && g.fails == 1 && !r.launched);
  CHECK(g.msg == "driver_call: copy to the device failed: injected: copy in");
  CHECK(g.allocs == 1 && g.frees == 1 && g.syncs == 1);
}

void test_workspace() {
  const int64_t need = 1000;
  std::vector<unsigned char> mine((size_t)need + 8, kUntouched);
  int launches = 0;
  void* seen = nullptr;
  auto launch_ok = [&](void* ws) {
    ++launches;
    seen = ws;
    memset(ws, 2, (size_t)need);  // `need` bytes are writable
    return FDCN_OK;
  };
  auto launch_bad = [&](void* ws) {
    ++launches;
    memset(ws, 3, (size_t)need);
    return Fake::fail(FDCN_EHIP, "driver_dev: launch failed");
  };
  const int st = Fake::kStream;

  // the caller's buffer, large enough (more, and exactly)
  for (int64_t have : {need + 8, need}) {
    reset();
    CHECK(fdcn_call::with_workspace<Fake>("driver_dev", "needed", mine.data(), have, need, st,
                                          launch_ok) == FDCN_OK);
    CHECK(seen == mine.data() && g.steps.empty() && g.fails == 0);
    CHECK(mine[(size_t)need] == kUntouched);
  }
  CHECK(launches == 2);

  // too small (one byte short; a negative size): refused before any launch
  for (int64_t have : {need - 1, (int64_t)-5}) {
    reset();
    CHECK(fdcn_call::with_workspace<Fake>("driver_dev", "this launch needs (a_plan)", mine.data(),
                                          have, need, st, launch_ok) == FDCN_EINVAL);
    char want[160];
    snprintf(want, sizeof want,
             "driver_dev: workspace of %lld B is smaller than the 1000 B this launch needs (a_plan)",
             (long long)have);
    CHECK(g.fails == 1 && g.msg == want && g.steps.empty());
  }
  CHECK(launches == 2);

  // none: a stream-ordered block of the helper's own, released, no host wait
  reset();
  CHECK(fdcn_call::with_workspace<Fake>("driver_dev", "needed", nullptr, 0, 1024, st, launch_ok) ==
        FDCN_OK);
  CHECK(launches == 3 && seen != nullptr && seen != mine.data());
  CHECK(g.allocs == 1 && g.frees == 1 && g.syncs == 0 && g.fails == 0);
  CHECK(std::string(g.steps.begin(), g.steps.end()) == "af");

  // ... also when the launch fails (the path fdcn_vc's launch used to leak on)
  reset();
  CHECK(fdcn_call::with_workspace<Fake>("driver_dev", "needed", nullptr, 0, 1024, st, launch_bad) ==
        FDCN_EHIP);
  CHECK(launches == 4 && g.allocs == 1 && g.frees == 1 && g.syncs == 0);
  CHECK(g.fails == 1 && g.msg == "driver_dev: launch failed");

  // ... and a failed free after it does not replace the launch's message
  reset({2});
  CHECK(fdcn_call::with_workspace<Fake>("driver_dev", "needed", nullptr, 0, 1024, st, launch_bad) ==
        FDCN_EHIP);
  CHECK(g.fails == 1 && g.msg == "driver_dev: launch failed" && g.frees == 1);

  // a failed free alone is reported
  reset({2});
  CHECK(fdcn_call::with_workspace<Fake>("driver_dev", "needed", nullptr, 0, 1024, st, launch_ok) ==
        FDCN_EHIP);
  CHECK(g.fails == 1 && g.msg == "driver_dev: workspace free failed: injected: free");

  // the allocation fails: FDCN_ENOMEM, nothing launched, nothing to free
  reset({1});
  const int before = launches;
  CHECK(fdcn_call::with_workspace<Fake>("driver_dev", "needed", nullptr, 0, 1024, st, launch_ok) ==
        FDCN_ENOMEM);
  CHECK(launches == before && g.allocs == 0 && g.frees == 0 && g.fails == 1);
  CHECK(g.msg == "driver_dev: workspace allocation failed: injected: out of memory");
}

// more regions than a call can hold: refused, nothing allocated
void test_too_many_regions() {
  reset();
  Call c("driver_call");
  CHECK(c.open() == FDCN_OK);
  for (int i = 0; i < 13; ++i) c.scratch(8);
  bool launched = false;
  CHECK(c.run([&](int) {
    launched = true;
    return FDCN_OK;
  }) == FDCN_EINVAL);
  CHECK(!launched && g.allocs == 0 && g.fails == 1);
}

}  // namespace

int main() {
  test_round_trip();
  test_injection();
  test_workspace();
  test_too_many_regions();
  reset();
  printf("host_call_driver: ok\n");
  return 0;
}
