// The index arithmetic of the site-permutation pass (dynamite_amd/csrc/perm_rank.h, on pm_rank.h: the headers the kernels
// and dnm_perm_partner_indices include) as a plain C++ program for AddressSanitizer and UndefinedBehaviorSanitizer: no
// HIP runtime, no library, nothing loaded into Python (tests/test_perm_rank_host.py builds and runs it).  For every row
// of SpinConserve(16, 8) and (34, 2), of the edge sectors of 12 spins and of one set bit at 63 and 64 spins, and for every
// permutation of a fixed set -- identity, a transposition with site L - 1, the reversal, the shifts by 1 and by L - 1, a
// three-cycle through L - 1, two seeded random ones -- the source configuration is compared with a loop over all sites
// written here (bit i of the source = bit pi(i) of the row) and its index with a ranking loop written here: next
// configuration by Gosper's step with the division, rank as the sum of C(position, ordinal) computed by multiplication.
// Where L = 2 k the rows of the XParity half are walked once more in both sectors against the complement written out.
// The Full / Parity form is walked on every index of 10, 11 and 12 spins.  The binomial table has exactly the size the
// kernel is handed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dynamite_amd/csrc/perm_rank.h"

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

// bit i of the source = bit pi(i) of the row's configuration
static uint64_t plain_source(uint64_t cfg, const int32_t *pi, int L) {
  uint64_t src = 0;
  for (int i = 0; i < L; ++i) src |= ((cfg >> pi[i]) & 1) << i;
  return src;
}

static uint64_t lcg(uint64_t *s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return *s >> 33;
}

// the permutations of the check, L ints each
static std::vector<int32_t> perm_set(int L) {
  std::vector<int32_t> out;
  auto add = [&](auto f) {
    for (int i = 0; i < L; ++i) out.push_back((int32_t)f(i));
  };
  const int h = L / 2;
  add([&](int i) { return i; });
  add([&](int i) { return i == h ? L - 1 : i == L - 1 ? h : i; });
  add([&](int i) { return L - 1 - i; });
  add([&](int i) { return (i + 1) % L; });
  add([&](int i) { return (i + L - 1) % L; });
  add([&](int i) { return i == 1 ? L - 1 : i == L - 1 ? h + 1 : i == h + 1 ? 1 : i; });      // 1 -> L - 1 -> h + 1 -> 1
  for (uint64_t seed : {11ull, 12ull}) {
    std::vector<int32_t> p(L);
    for (int i = 0; i < L; ++i) p[i] = i;
    uint64_t s = seed * 1000003ull + (uint64_t)L;
    for (int i = L - 1; i > 0; --i) {
      const int j = (int)(lcg(&s) % (uint64_t)(i + 1));
      const int32_t t = p[i];
      p[i] = p[j];
      p[j] = t;
    }
    out.insert(out.end(), p.begin(), p.end());
  }
  return out;
}

static int check_invert() {
  int failures = 0;
  uint8_t inv[64];
  const int32_t twice[] = {0, 1, 1, 3}, outside[] = {0, 1, 2, 4}, negative[] = {0, -1, 2, 3}, fine[] = {2, 0, 3, 1};
  failures += dnm::perm_invert(twice, 4, inv) || dnm::perm_invert(outside, 4, inv) || dnm::perm_invert(negative, 4, inv);
  failures += !dnm::perm_invert(fine, 4, inv) || inv[2] != 0 || inv[0] != 1 || inv[3] != 2 || inv[1] != 3;
  return failures;
}

static int check(int L, int k) {
  const int ld = L + 1;
  int failures = 0;
  std::vector<int64_t> t((size_t)(k + 1) * ld);      // exactly the table the kernel gets: every look-up must stay inside
  dnm::pm_binomials(L, k, ld, t.data());
  const int64_t dim = choose(L, k);
  const std::vector<int32_t> perms = perm_set(L);
  const int nperm = (int)(perms.size() / L);
  std::vector<uint8_t> inv((size_t)nperm * L);       // (exactly L bytes each)
  for (int g = 0; g < nperm; ++g)
    if (!dnm::perm_invert(perms.data() + (size_t)g * L, L, inv.data() + (size_t)g * L)) ++failures;
  const uint64_t all = L == 64 ? ~(uint64_t)0 : (((uint64_t)1 << L) - 1);
  int64_t moved = 0, flips = 0;
  for (int xsec : {0, +1, -1}) {
    if (xsec != 0 && L != 2 * k) continue;
    const int64_t nrows = xsec ? dim / 2 : dim;
    uint64_t st = k == 64 ? ~(uint64_t)0 : (((uint64_t)1 << k) - 1);
    uint64_t stepped = st;
    for (int64_t row = 0; row < nrows; ++row) {
      if (dnm::pm_unrank(row, L, k, t.data(), ld) != st || plain_rank(st) != row || stepped != st) {
        if (++failures < 5) printf("  row %lld: unranked or stepped configuration differs\n", (long long)row);
      }
      for (int g = 0; g < nperm; ++g) {
        const int32_t *pi = perms.data() + (size_t)g * L;
        const uint64_t src = dnm::perm_source(st, inv.data() + (size_t)g * L);
        const uint64_t want_src = plain_source(st, pi, L);
        int fl = -1;
        const int64_t got = dnm::perm_sc_index(src, L, dim, xsec, t.data(), ld, &fl);
        const bool top = xsec != 0 && ((want_src >> (L - 1)) & 1);
        const int64_t want = plain_rank(top ? want_src ^ all : want_src);
        if (src != want_src || got != want || fl != (top ? 1 : 0) || got < 0 || got >= nrows) {
          if (++failures < 5)
            printf("  row %lld permutation %d sector %d: source %llx (want %llx), index %lld, flag %d (want %lld, %d)\n",
                   (long long)row, g, xsec, (unsigned long long)src, (unsigned long long)want_src, (long long)got, fl,
                   (long long)want, top ? 1 : 0);
        }
        moved += want_src != st;
        flips += top;
      }
      if (row + 1 < nrows && k > 0) {          // Gosper: the next configuration with k set bits is the next in colex order
        const uint64_t c = st & (~st + 1), r = st + c;
        stepped = dnm::perm_next_config(st);
        st = (((r ^ st) >> 2) / c) | r;
      }
    }
  }
  printf("SpinConserve(%d, %d): %lld rows, %d permutations, %lld sources that differ, %lld complements: %s\n", L, k,
         (long long)dim, nperm, (long long)moved, (long long)flips, failures ? "FAILED" : "ok");
  return failures;
}

// Full (parity = false) and Parity of L spins: every index
static int check_index(int L, bool parity, int space) {
  int failures = 0;
  const std::vector<int32_t> perms = perm_set(L);
  const int nperm = (int)(perms.size() / L);
  std::vector<uint8_t> inv((size_t)nperm * L);
  for (int g = 0; g < nperm; ++g)
    if (!dnm::perm_invert(perms.data() + (size_t)g * L, L, inv.data() + (size_t)g * L)) ++failures;
  const uint64_t all = ((uint64_t)1 << L) - 1;
  const int64_t dim = (int64_t)1 << (L - parity);
  int64_t flips = 0;
  for (int xsec : {0, +1, -1}) {
    if (xsec != 0 && parity && L % 2) continue;
    const int64_t nrows = xsec ? dim / 2 : dim;
    for (int64_t row = 0; row < nrows; ++row) {
      const uint64_t st = parity ? ((uint64_t)row << 1) | (uint64_t)((__builtin_popcountll((uint64_t)row) & 1) ^ space)
                                 : (uint64_t)row;
      if (dnm::perm_index_config(parity, space, (uint64_t)row) != st) ++failures;
      for (int g = 0; g < nperm; ++g) {
        const uint64_t src = dnm::perm_source(st, inv.data() + (size_t)g * L);
        uint64_t want_src = plain_source(st, perms.data() + (size_t)g * L, L);
        int fl = -1;
        const int64_t got = dnm::perm_xor_index(src, parity, L, xsec, &fl);
        const bool same = src == want_src;
        const bool top = xsec != 0 && ((want_src >> (L - 1)) & 1);
        if (top) want_src ^= all;
        const int64_t want = (int64_t)(parity ? want_src >> 1 : want_src);
        const bool in_space = !parity || (__builtin_popcountll(want_src) & 1) == space;
        if (!same || got != want || !in_space || fl != (top ? 1 : 0) || got < 0 || got >= nrows) {
          if (++failures < 5)
            printf("  index %lld permutation %d sector %d: index %lld, flag %d (want %lld, %d)\n", (long long)row, g, xsec,
                   (long long)got, fl, (long long)want, top ? 1 : 0);
        }
        flips += top;
      }
    }
  }
  printf("%s(%d): %lld rows, %d permutations, %lld complements: %s\n",
         parity ? (space ? "Parity odd" : "Parity even") : "Full", L, (long long)dim, nperm, (long long)flips,
         failures ? "FAILED" : "ok");
  return failures;
}

int main() {
  int failures = check_invert();
  const int cases[][2] = {{16, 8}, {34, 2}, {12, 0}, {12, 1}, {12, 11}, {12, 12}, {12, 6}, {63, 1}, {64, 1}};
  for (const auto &c : cases) failures += check(c[0], c[1]);
  failures += check_index(10, false, 0);
  failures += check_index(11, true, 1);
  failures += check_index(12, true, 0);
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
