// The ranking of the sigma+ sigma- pass (dynamite_amd/csrc/pm_rank.h: the header the kernel and
// dnm_pm_partner_indices include) as a plain C++ program for AddressSanitizer and UndefinedBehaviorSanitizer: no HIP
// runtime, no library, nothing loaded into Python (tests/test_pm_rank_host.py builds and runs it).  For every row of
// the sector with k + 1 set bits of SpinConserve(16, 8) and (34, 2) -- and the edge sectors of 12 spins -- the unranked
// configuration and the index of every partner are compared with a ranking loop written here: next configuration by
// Gosper's step, rank as the sum of C(position, ordinal) computed by multiplication.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dynamite_amd/csrc/pm_rank.h"

static int64_t choose(int n, int m) {
  if (m < 0 || m > n) return 0;
  if (m > n - m) m = n - m;
  int64_t v = 1;
  for (int i = 1; i <= m; ++i) v = v * (n - m + i) / i;       // exact: v is C(n - m + i, i) after each step
  return v;
}

static int64_t plain_rank(uint64_t st) {
  int64_t idx = 0;
  int ord = 0;
  for (int p = 0; p < 64; ++p)
    if ((st >> p) & 1) idx += choose(p, ++ord);
  return idx;
}

static int check(int L, int k) {
  const int K = k + 1, ld = L + 1;
  int failures = 0;
  if (K > L) {
    printf("SpinConserve(%d, %d): no neighbouring sector: ok\n", L, k);
    return 0;
  }
  std::vector<int64_t> t((size_t)(K + 1) * ld);      // exactly the table the kernel gets: every look-up must stay inside
  dnm::pm_binomials(L, K, ld, t.data());
  for (int m = 0; m <= K; ++m)
    for (int n = 0; n <= L; ++n)
      if (t[(size_t)m * ld + n] != choose(n, m)) ++failures;
  const int64_t nrows = choose(L, K);
  uint64_t st = K == 64 ? ~(uint64_t)0 : (((uint64_t)1 << K) - 1);
  int64_t partners = 0;
  for (int64_t row = 0; row < nrows; ++row) {
    if (dnm::pm_unrank(row, L, K, t.data(), ld) != st || plain_rank(st) != row) {
      if (++failures < 5) printf("  row %lld: unranked configuration differs\n", (long long)row);
    }
    uint64_t seen = 0;
    int last = -1;
    dnm::pm_partners(st, t.data(), ld, [&](int j, int64_t idx) {
      if (j <= last || !((st >> j) & 1) || idx != plain_rank(st ^ ((uint64_t)1 << j)) || idx < 0 ||
          idx >= choose(L, k)) {
        if (++failures < 5) printf("  row %lld site %d: partner index %lld\n", (long long)row, j, (long long)idx);
      }
      last = j;
      seen |= (uint64_t)1 << j;
      ++partners;
    });
    if (seen != st) ++failures;
    if (row + 1 < nrows) {          // Gosper: the next configuration with K set bits is the next in colex order
      const uint64_t c = st & (~st + 1), r = st + c;
      st = (((r ^ st) >> 2) / c) | r;
    }
  }
  if (partners != nrows * K) ++failures;
  printf("SpinConserve(%d, %d): %lld rows, %lld partners: %s\n", L, k, (long long)nrows, (long long)partners,
         failures ? "FAILED" : "ok");
  return failures;
}

int main() {
  int failures = 0;
  const int cases[][2] = {{16, 8}, {34, 2}, {12, 0}, {12, 11}, {12, 12}, {63, 1}, {64, 1}};
  for (const auto &c : cases) failures += check(c[0], c[1]);
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
