// The partner arithmetic of the bond-swap pass (dynamite_amd/csrc/swap_rank.h: the header the kernel and
// dnm_swap_partner_indices include) as a plain C++ program for AddressSanitizer and UndefinedBehaviorSanitizer: no HIP
// runtime, no library, nothing loaded into Python (tests/test_swap_rank_host.py builds and runs it).  For every row of
// SpinConserve(16, 8) and (34, 2), of the edge sectors of 12 spins and of one set bit at 63 and 64 spins, and for every
// bond of a fixed set, the index of the swapped configuration is compared with a ranking loop written here: next
// configuration by Gosper's step, rank as the sum of C(position, ordinal) computed by multiplication.  Where L = 2 k the
// rows of the XParity half are walked once more in both sectors against the complement written out.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dynamite_amd/csrc/swap_rank.h"

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

static std::vector<int> bond_set(int L) {
  // adjacent, far, at site 0, at site L - 1, both orders, a repeat
  const int raw[][2] = {{0, 1}, {1, 0}, {0, L - 1}, {L - 1, 0}, {L - 2, L - 1}, {L - 1, L / 2}, {1, L - 2},
                        {L / 2, L / 2 + 1}, {2, L / 2}, {0, L / 2}, {L - 1, 1}, {0, 1}, {3, 7}, {L - 3, 2}};
  std::vector<int> b;
  for (const auto &r : raw) {
    b.push_back(r[0]);
    b.push_back(r[1]);
  }
  return b;
}

static int check(int L, int k) {
  const int ld = L + 1;
  int failures = 0;
  std::vector<int64_t> t((size_t)(k + 1) * ld);      // exactly the table the kernel gets: every look-up must stay inside
  dnm::pm_binomials(L, k, ld, t.data());
  const int64_t dim = choose(L, k);
  const std::vector<int> bonds = bond_set(L);
  const uint64_t all = L == 64 ? ~(uint64_t)0 : (((uint64_t)1 << L) - 1);
  int64_t moved = 0, flips = 0;
  for (int xsec : {0, +1, -1}) {
    if (xsec != 0 && L != 2 * k) continue;
    const int64_t nrows = xsec ? dim / 2 : dim;
    uint64_t st = k == 64 ? ~(uint64_t)0 : (((uint64_t)1 << k) - 1);
    for (int64_t row = 0; row < nrows; ++row) {
      if (dnm::pm_unrank(row, L, k, t.data(), ld) != st || plain_rank(st) != row) {
        if (++failures < 5) printf("  row %lld: unranked configuration differs\n", (long long)row);
      }
      for (size_t m = 0; m < bonds.size() / 2; ++m) {
        const int a = bonds[2 * m], b = bonds[2 * m + 1];
        int fl = -1;
        const int64_t got = dnm::swap_sc_partner(st, row, a, b, L, dim, xsec, t.data(), ld, &fl);
        uint64_t sw = st;
        if (((st >> a) ^ (st >> b)) & 1) sw ^= ((uint64_t)1 << a) ^ ((uint64_t)1 << b);
        const bool top = xsec != 0 && ((sw >> (L - 1)) & 1);
        const int64_t want = plain_rank(top ? sw ^ all : sw);
        if (got != want || fl != (top ? 1 : 0) || got < 0 || got >= nrows) {
          if (++failures < 5)
            printf("  row %lld bond (%d, %d) sector %d: index %lld, flag %d (want %lld, %d)\n", (long long)row, a, b,
                   xsec, (long long)got, fl, (long long)want, top ? 1 : 0);
        }
        moved += sw != st;
        flips += top;
      }
      if (row + 1 < nrows && k > 0) {          // Gosper: the next configuration with k set bits is the next in colex order
        const uint64_t c = st & (~st + 1), r = st + c;
        st = (((r ^ st) >> 2) / c) | r;
      }
    }
  }
  printf("SpinConserve(%d, %d): %lld rows, %lld swaps that move, %lld complements: %s\n", L, k, (long long)dim,
         (long long)moved, (long long)flips, failures ? "FAILED" : "ok");
  return failures;
}

int main() {
  int failures = 0;
  const int cases[][2] = {{16, 8}, {34, 2}, {12, 0}, {12, 1}, {12, 11}, {12, 12}, {12, 6}, {63, 1}, {64, 1}};
  for (const auto &c : cases) failures += check(c[0], c[1]);
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
