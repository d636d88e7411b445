// qmc_check_driver.cpp -- CPU driver of the host-only table checks of the
// quasi-Monte Carlo path kernel (finite_difference_amd/csrc/fdcn_qmc_table.h)
// for the sanitizer build (`make qmc_check`: AddressSanitizer +
// UndefinedBehaviorSanitizer, first report aborts).  A table that passes the
// check is what keeps every LDS index of qmc_path_kernel in range, so the
// driver (a) feeds it well-formed tables of every length -- bridge and
// incremental, each in an exactly sized heap block so a read past the table
// is an ASan report -- and walks them the way the kernel does, asserting every
// index it forms is in range and defined; (b) feeds it each malformed table of
// include/fdcn.h's rules and checks the refusal and its text; (c) runs the
// weight check over finite and non-finite blocks.  Exit 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../../finite_difference_amd/csrc/fdcn_qmc_table.h"

namespace {

#define CHECK(c)                                                                         \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      fprintf(stderr, "qmc_check_driver: %s:%d: %s\n", __FILE__, __LINE__, #c);          \
      exit(1);                                                                           \
    }                                                                                    \
  } while (0)

using Table = std::vector<int32_t>;  // [n][3], exactly sized on the heap

// breadth-first bisection: row 0 sets n from 0, then (l, r) -> (l + r) / 2
Table bridge(int n) {
  Table t = {n, 0, 0};
  std::vector<std::pair<int, int>> level = {{0, n}}, next;
  while (!level.empty()) {
    next.clear();
    for (auto [l, r] : level) {
      if (r - l < 2) continue;
      const int i = (l + r) / 2;
      t.insert(t.end(), {i, l, r});
      next.push_back({l, i});
      next.push_back({i, r});
    }
    level = next;
  }
  return t;
}

Table incremental(int n) {
  Table t;
  for (int m = 1; m <= n; ++m) t.insert(t.end(), {m, m - 1, m - 1});
  return t;
}

int check(int n, const Table& t, char* why, size_t len) {
  // an exactly sized copy: any read outside [0, 3 n) is a heap overflow
  int32_t* p = static_cast<int32_t*>(malloc(sizeof(int32_t) * (t.empty() ? 1 : t.size())));
  CHECK(p != nullptr);
  if (!t.empty()) memcpy(p, t.data(), sizeof(int32_t) * t.size());
  const int rc = fdcn_qmc::check_bridge_idx(n, p, why, len);
  free(p);
  return rc;
}

// the kernel's walk over an accepted table: W has n + 1 rows
void walk(int n, const Table& t) {
  std::vector<double> W((size_t)n + 1, std::numeric_limits<double>::quiet_NaN());
  W[0] = 0.0;
  for (int j = 0; j < n; ++j) {
    const int32_t tg = t[3 * j], l = t[3 * j + 1], r = t[3 * j + 2];
    CHECK(tg >= 1 && tg <= n && l >= 0 && l <= n && r >= 0 && r <= n);
    CHECK(!isnan(W.at(l)) && !isnan(W.at(r)) && isnan(W.at(tg)));
    W.at(tg) = 0.5 * W[l] + 0.5 * W[r] + 1.0;
  }
  for (int m = 0; m <= n; ++m) CHECK(!isnan(W[m]));
}

void test_good_tables() {
  char why[160];
  for (int n = 1; n <= FDCN_QMC_MAX_STEPS; ++n) {
    for (const Table& t : {bridge(n), incremental(n)}) {
      CHECK((int)t.size() == 3 * n);
      CHECK(check(n, t, why, sizeof why) == 0);
      walk(n, t);
    }
  }
  // a mixed table: an extension from an inner node, then a bridge inside it
  const Table mixed = {2, 0, 0, 4, 2, 2, 3, 2, 4, 1, 0, 2, 5, 4, 4};
  CHECK(check(5, mixed, why, sizeof why) == 0);
  walk(5, mixed);
}

void refuse(int n, const Table& t, const char* expect) {
  char why[160] = "";
  CHECK(check(n, t, why, sizeof why) == -1);
  if (!strstr(why, expect)) {
    fprintf(stderr, "qmc_check_driver: expected \"%s\" in \"%s\"\n", expect, why);
    exit(1);
  }
  // a short message buffer is filled, terminated and not overrun
  char small[8];
  CHECK(check(n, t, small, sizeof small) == -1);
  CHECK(strlen(small) < sizeof small);
}

void test_bad_tables() {
  refuse(3, {3, 0, 0, 1, 0, 3, 1, 0, 3}, "set twice");                  // duplicate target
  refuse(3, {3, 0, 0, 0, 0, 3, 2, 1, 3}, "target 0 is outside");        // target 0
  refuse(3, {4, 0, 0, 1, 0, 3, 2, 1, 3}, "target 4 is outside");        // target > n
  refuse(3, {3, 0, 0, -7, 0, 3, 2, 1, 3}, "is outside");                // negative target
  refuse(3, {3, 0, 0, 2, 1, 3, 1, 0, 2}, "left 1 is not defined");      // undefined left
  refuse(3, {3, 0, 0, 1, 3, 3, 2, 1, 3}, "left 3 is not in");           // left above target
  refuse(3, {3, 0, 0, 1, -1, 3, 2, 1, 3}, "left -1 is not in");         // negative left
  refuse(3, {1, 0, 0, 3, 0, 1, 2, 1, 3}, "right 1 is neither");         // left < right < target
  refuse(3, {2, 0, 0, 1, 0, 3, 3, 2, 2}, "right 3 is not defined");     // undefined right
  refuse(3, {3, 0, 0, 1, 0, 4, 2, 1, 3}, "right 4 is neither");         // right > n
  refuse(3, {3, 0, 0, 1, 0, 2147483647, 2, 1, 3}, "neither");           // no overflow on the way
  refuse(3, {3, 0, 0, 1, 0, INT32_MIN, 2, 1, 3}, "neither");
  refuse(2, {2, 2, 2, 1, 0, 2}, "left 2 is not in");                    // left == target
  refuse(0, {}, "n_steps");
  refuse(FDCN_QMC_MAX_STEPS + 1, bridge(FDCN_QMC_MAX_STEPS), "n_steps");
  char why[160];
  CHECK(fdcn_qmc::check_bridge_idx(3, nullptr, why, sizeof why) == -1 && strstr(why, "NULL"));
}

void test_weights() {
  char why[160];
  const int B = 3, n = 5;
  std::vector<double> w((size_t)B * n * 3, 0.25);
  CHECK(fdcn_qmc::check_bridge_w(B, n, w.data(), why, sizeof why) == 0);
  const double bad[] = {std::numeric_limits<double>::quiet_NaN(),
                        std::numeric_limits<double>::infinity(),
                        -std::numeric_limits<double>::infinity()};
  for (double v : bad)
    for (size_t at : {(size_t)0, (size_t)(1 * n * 3 + 2 * 3 + 1), w.size() - 1}) {
      std::vector<double> x = w;
      x[at] = v;
      CHECK(fdcn_qmc::check_bridge_w(B, n, x.data(), why, sizeof why) == -1);
      CHECK(strstr(why, "not finite"));
    }
  std::vector<double> x = w;
  x[1 * n * 3 + 2 * 3 + 1] = bad[0];
  CHECK(fdcn_qmc::check_bridge_w(B, n, x.data(), why, sizeof why) == -1);
  CHECK(strstr(why, "contract 1, row 2"));
}

}  // namespace

int main() {
  test_good_tables();
  test_bad_tables();
  test_weights();
  printf("qmc_check_driver: OK\n");
  return 0;
}
