// The column arithmetic of the two-spin Pauli pass (dynamite_amd/csrc/pauli_cols.h) against a plain loop, as a program
// of its own for the sanitizers (tests/test_pauli_cols_host.py builds and runs it): the partner mask, the configuration
// a column reads and its sign, for every row and every column of Full(6) and of both sectors of Parity(7), and for a
// handful of rows at 63 and 64 spins, sites 0 and L - 1 among them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dynamite_amd/csrc/pauli_cols.h"

using namespace dnm;

static int failures = 0;

static int parity_of(uint64_t v) {
  int p = 0;
  for (int b = 0; b < 64; ++b) p ^= (int)((v >> b) & 1);
  return p;
}

// One subspace: rows are indices into the vector; type 0 Full, 1 Parity
static void check(const char *name, bool parity, int space, int L, const std::vector<uint64_t> &rows) {
  long long checked = 0, flipped = 0, negative = 0;
  const int before = failures;
  for (uint64_t q : rows) {
    for (int site = 0; site < L; ++site) {
      for (int kind = 1; kind <= 3; ++kind) {
        // the plain loop: the configuration of the row of A bit by bit, the Pauli matrix applied to it
        const bool f = kind != 3, g = kind != 1;
        uint64_t cfg = 0;          // the configuration r of the row of column c
        if (!parity) {
          for (int b = 0; b < L; ++b) cfg |= ((q >> b) & 1) << b;
        } else {
          for (int b = 1; b < L; ++b) cfg |= ((q >> (b - 1)) & 1) << b;
          // the rows of a flipping column are those of the other sector
          const int want_parity = f ? space ^ 1 : space;
          if (parity_of(cfg) != want_parity) cfg |= 1;
        }
        uint64_t src = cfg;        // the configuration whose amplitude the column takes
        if (f) src ^= (uint64_t)1 << site;
        if (parity && parity_of(src) != space) {
          if (++failures < 5) printf("  %s: the source of row %llu leaves the sector\n", name, (unsigned long long)q);
          continue;
        }
        const uint64_t want_idx = parity ? src >> 1 : src;
        const bool want_neg = g && ((cfg >> site) & 1);

        const uint64_t mask = pauli_index_mask(parity, site, kind);
        const uint64_t got_cfg = pauli_row_config(parity, space, q, parity_of(q), pauli_flips(kind));
        const bool got_neg = pauli_negative(got_cfg, site, kind);
        ++checked;
        flipped += mask != 0;
        negative += got_neg;
        if (pauli_flips(kind) != f || pauli_signs(kind) != g || (q ^ mask) != want_idx || got_cfg != cfg ||
            got_neg != want_neg) {
          if (++failures < 5)
            printf("  %s row %llu site %d kind %d: index %llu, configuration %llx, negative %d (want %llu, %llx, %d)\n",
                   name, (unsigned long long)q, site, kind, (unsigned long long)(q ^ mask), (unsigned long long)got_cfg,
                   (int)got_neg, (unsigned long long)want_idx, (unsigned long long)cfg, (int)want_neg);
        }
      }
    }
  }
  printf("%s: %lld columns checked, %lld partners elsewhere, %lld signs -1: %s\n", name, checked, flipped, negative,
         failures == before ? "ok" : "FAILED");
}

static std::vector<uint64_t> all_rows(int bits) {
  std::vector<uint64_t> r((size_t)1 << bits);
  for (size_t i = 0; i < r.size(); ++i) r[i] = i;
  return r;
}

int main() {
  check("Full(6)", false, 0, 6, all_rows(6));
  check("Parity(even, 7)", true, 0, 7, all_rows(6));
  check("Parity(odd, 7)", true, 1, 7, all_rows(6));
  // a handful of rows at the widest configurations: all clear, all set, the top bit alone, patterns
  const uint64_t top63 = (uint64_t)1 << 62;
  check("Full(63)", false, 0, 63, {0, 1, top63, top63 - 1, top63 | 1, 0x5555555555555555ull & (2 * top63 - 1),
                                   0x2aaaaaaaaaaaaaaaull, 2 * top63 - 1});
  check("Full(64)", false, 0, 64, {0, 1, ~(uint64_t)0, (uint64_t)1 << 63, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull,
                                   ((uint64_t)1 << 63) | 1});
  check("Parity(even, 63)", true, 0, 63, {0, 1, top63 - 1, top63 >> 1, 0x1555555555555555ull, 0x2aaaaaaaaaaaaaaaull});
  check("Parity(odd, 63)", true, 1, 63, {0, 1, top63 - 1, top63 >> 1, 0x1555555555555555ull, 0x2aaaaaaaaaaaaaaaull});
  check("Parity(even, 64)", true, 0, 64, {0, 1, 2 * top63 - 1, top63, 0x5555555555555555ull & (2 * top63 - 1),
                                          0x2aaaaaaaaaaaaaaaull});
  check("Parity(odd, 64)", true, 1, 64, {0, 1, 2 * top63 - 1, top63, 0x5555555555555555ull & (2 * top63 - 1),
                                         0x2aaaaaaaaaaaaaaaull});
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
