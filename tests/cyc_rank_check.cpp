// The partner arithmetic of the three-site rotation pass (dynamite_amd/csrc/cyc_rank.h, on swap_rank.h: the headers the
// kernel and dnm_cyc_partner_indices include) as a plain C++ program for AddressSanitizer and
// UndefinedBehaviorSanitizer: no HIP runtime, no library, nothing loaded into Python (tests/test_cyc_rank_host.py builds
// and runs it).  For every row of SpinConserve(16, 8) and (34, 2), of the edge sectors of 12 spins and of one set bit at
// 63 and 64 spins, and for every triple of a fixed set, the index of the rotated configuration is compared with a
// ranking loop written here: next configuration by Gosper's step, rank as the sum of C(position, ordinal) computed by
// multiplication.  Where L = 2 k the rows of the XParity half are walked once more in both sectors against the
// complement written out.  The Full / Parity form (masks per site) is walked on every configuration of 10 spins.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dynamite_amd/csrc/cyc_rank.h"

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

static std::vector<int> triple_set(int L) {
  // adjacent, far, at site 0, site L - 1 in each of the three places, both senses, a repeat
  const int h = L / 2;
  const int raw[][3] = {{0, 1, 2}, {0, 2, 1}, {2, 1, 0}, {0, h, L - 1}, {0, L - 1, h}, {L - 1, 0, h}, {h, L - 1, 0},
                        {L - 3, L - 2, L - 1}, {L - 1, L - 2, L - 3}, {L - 2, L - 1, 1}, {1, h, h + 1}, {3, 7, 5},
                        {0, 1, 2}, {L - 1, 1, L - 2}, {h, 0, 1}};
  std::vector<int> t;
  for (const auto &r : raw)
    for (int s : r) t.push_back(s);
  return t;
}

// bit a <- bit b, bit b <- bit c, bit c <- bit a
static uint64_t rotated(uint64_t st, int a, int b, int c) {
  const uint64_t xa = (st >> a) & 1, xb = (st >> b) & 1, xc = (st >> c) & 1;
  st &= ~(((uint64_t)1 << a) | ((uint64_t)1 << b) | ((uint64_t)1 << c));
  return st | (xb << a) | (xc << b) | (xa << c);
}

static int check(int L, int k) {
  const int ld = L + 1;
  int failures = 0;
  std::vector<int64_t> t((size_t)(k + 1) * ld);      // exactly the table the kernel gets: every look-up must stay inside
  dnm::pm_binomials(L, k, ld, t.data());
  const int64_t dim = choose(L, k);
  const std::vector<int> triples = triple_set(L);
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
      for (size_t m = 0; m < triples.size() / 3; ++m) {
        const int a = triples[3 * m], b = triples[3 * m + 1], c = triples[3 * m + 2];
        int fl = -1, p = -1, q = -1;
        const int64_t got = dnm::cyc_sc_partner(st, row, a, b, c, L, dim, xsec, t.data(), ld, &fl);
        const uint64_t rot = rotated(st, a, b, c);
        // the rule: no site or exactly two change, and those two are where the rotation differs from the row
        const int d = dnm::cyc_changed(st, a, b, c, &p, &q);
        const uint64_t diff = (d & 1 ? (uint64_t)1 << a : 0) | (d & 2 ? (uint64_t)1 << b : 0) |
                              (d & 4 ? (uint64_t)1 << c : 0);
        if (diff != (rot ^ st) || (d != 0 && (p == q || diff != (((uint64_t)1 << p) | ((uint64_t)1 << q))))) {
          if (++failures < 5) printf("  row %lld triple (%d, %d, %d): changed sites %d (%d, %d)\n", (long long)row, a, b,
                                     c, d, p, q);
        }
        const bool top = xsec != 0 && ((rot >> (L - 1)) & 1);
        const int64_t want = plain_rank(top ? rot ^ all : rot);
        if (got != want || fl != (top ? 1 : 0) || got < 0 || got >= nrows) {
          if (++failures < 5)
            printf("  row %lld triple (%d, %d, %d) sector %d: index %lld, flag %d (want %lld, %d)\n", (long long)row, a,
                   b, c, xsec, (long long)got, fl, (long long)want, top ? 1 : 0);
        }
        moved += rot != st;
        flips += top;
      }
      if (row + 1 < nrows && k > 0) {          // Gosper: the next configuration with k set bits is the next in colex order
        const uint64_t c = st & (~st + 1), r = st + c;
        st = (((r ^ st) >> 2) / c) | r;
      }
    }
  }
  printf("SpinConserve(%d, %d): %lld rows, %lld rotations that move, %lld complements: %s\n", L, k, (long long)dim,
         (long long)moved, (long long)flips, failures ? "FAILED" : "ok");
  return failures;
}

// Full (parity = false) and Parity of L spins: every index, the mask form against the rotation written out
static int check_masks(int L, bool parity, int space) {
  int failures = 0;
  const std::vector<int> triples = triple_set(L);
  const uint64_t all = ((uint64_t)1 << L) - 1;
  const int64_t dim = (int64_t)1 << (L - parity);
  int64_t flips = 0;
  for (int xsec : {0, +1, -1}) {
    if (xsec != 0 && parity && L % 2) continue;
    const int64_t nrows = xsec ? dim / 2 : dim;
    for (int64_t row = 0; row < nrows; ++row) {
      const uint64_t st = parity ? ((uint64_t)row << 1) | (uint64_t)((__builtin_popcountll((uint64_t)row) & 1) ^ space)
                                 : (uint64_t)row;
      for (size_t m = 0; m < triples.size() / 3; ++m) {
        const int a = triples[3 * m], b = triples[3 * m + 1], c = triples[3 * m + 2];
        int p, q;
        const int d = dnm::cyc_changed(st, a, b, c, &p, &q);
        const int fl = dnm::cyc_flipped(d, a, b, c, L, xsec);
        const int64_t got = dnm::cyc_xor_partner(row, d, fl, dnm::cyc_site_mask(parity, a), dnm::cyc_site_mask(parity, b),
                                                 dnm::cyc_site_mask(parity, c), dnm::cyc_all_mask(parity, L));
        uint64_t rot = rotated(st, a, b, c);
        const bool top = xsec != 0 && ((rot >> (L - 1)) & 1);
        if (top) rot ^= all;
        const int64_t want = (int64_t)(parity ? rot >> 1 : rot);
        const bool in_space = !parity || (__builtin_popcountll(rot) & 1) == space;
        if (got != want || !in_space || fl != (top ? 1 : 0) || got < 0 || got >= nrows) {
          if (++failures < 5)
            printf("  index %lld triple (%d, %d, %d) sector %d: index %lld, flag %d (want %lld, %d)\n", (long long)row, a,
                   b, c, xsec, (long long)got, fl, (long long)want, top ? 1 : 0);
        }
        flips += top;
      }
    }
  }
  printf("%s(%d): %lld rows, %lld complements: %s\n", parity ? (space ? "Parity odd" : "Parity even") : "Full", L,
         (long long)dim, (long long)flips, failures ? "FAILED" : "ok");
  return failures;
}

int main() {
  int failures = 0;
  const int cases[][2] = {{16, 8}, {34, 2}, {12, 0}, {12, 1}, {12, 11}, {12, 12}, {12, 6}, {63, 1}, {64, 1}};
  for (const auto &c : cases) failures += check(c[0], c[1]);
  failures += check_masks(10, false, 0);
  failures += check_masks(11, true, 1);
  failures += check_masks(12, true, 0);
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
