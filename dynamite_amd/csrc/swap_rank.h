// Partner arithmetic of the bond-swap pass (swap_kernels.hip, dnm_swap_partner_indices), for host and device alike --
// tests/swap_rank_check.cpp runs these very functions under the sanitizers.
//
// P_ab exchanges bits a and b of a configuration c.  Where the two bits are equal the partner of a row is the row
// itself; where they differ it is c ^ e_a ^ e_b, which stays inside Full, Parity and SpinConserve.
//
// SpinConserve, colex rank = sum_i C(p_i, i + 1) over the set bits p_0 < p_1 < ...: with lo < hi the two sites and j0
// the number of set bits below lo, the swap moves one set bit between lo and hi and only the set bits strictly between
// the two change their ordinal, by one:
//   bit hi set:  rank' - rank = C(lo, j0 + 1) - C(hi, j0 + nb + 1) + sum_between [C(p, i + 2) - C(p, i + 1)]
//   bit lo set:  rank' - rank = C(hi, j0 + nb + 1) - C(lo, j0 + 1) + sum_between [C(p, i) - C(p, i + 1)]
// (i: the old 0-based ordinal of p, nb: the set bits between).  Binomials come from pm_rank.h's table t[m * ld + n] =
// C(n, m) with rows 0 <= m <= k: the largest row read is k, the number of set bits.
//
// XParity sector s = +-1: the vector holds the representatives (bit L - 1 clear), y(c) = x[index(c)] there and
// s x[index(~c)] where bit L - 1 of c is set.  A swap sets bit L - 1 only for a bond that touches site L - 1, on the
// rows whose other bit is set.  Full / Parity: ~c is c ^ (all ones), one more XOR mask in index space.
// SpinConserve(L, L / 2): the complement reverses the colex order, index(~c) = dim - 1 - index(c).
#pragma once

#include <cstdint>

#include "pm_rank.h"

namespace dnm {

// rank(c ^ e_a ^ e_b) - rank(c) for a configuration c whose bits a and b differ
DNM_PM_HD int64_t swap_rank_delta(uint64_t c, int a, int b, const int64_t *t, int ld) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const uint64_t below = c & (((uint64_t)1 << lo) - 1);
  uint64_t mid = (c >> (lo + 1)) & (((uint64_t)1 << (hi - lo - 1)) - 1);      // (hi - lo - 1 <= 62)
  const bool down = (c >> hi) & 1;               // the set bit moves from hi down to lo
  int i = __builtin_popcountll(below) + (down ? 0 : 1);                       // old ordinal of the first bit between
  int64_t d = 0;
  for (; mid; mid &= mid - 1, ++i) {
    const int p = lo + 1 + __builtin_ctzll(mid);
    d += t[(down ? i + 2 : i) * ld + p] - t[(i + 1) * ld + p];
  }
  // i is now the old ordinal of hi (down) or one more than the new ordinal of hi (up): j0 + nb (+ 1)
  const int j0 = __builtin_popcountll(below);
  const int64_t at_lo = t[(j0 + 1) * ld + lo], at_hi = t[(down ? i + 1 : i) * ld + hi];
  return down ? d + at_lo - at_hi : d + at_hi - at_lo;
}

// Index into the vector of the partner of row `row` (configuration c, colex rank row) of SpinConserve for bond (a, b);
// xsec != 0: the vector holds the first dim / 2 rows of SpinConserve(L, L / 2).  *flipped: the partner is the complement's
// amplitude and carries the sector's sign.
DNM_PM_HD int64_t swap_sc_partner(uint64_t c, int64_t row, int a, int b, int L, int64_t dim, int xsec, const int64_t *t,
                                  int ld, int *flipped) {
  *flipped = 0;
  if ((((c >> a) ^ (c >> b)) & 1) == 0) return row;
  const int64_t r = row + swap_rank_delta(c, a, b, t, ld);
  if (xsec != 0 && (a == L - 1 || b == L - 1)) {
    *flipped = 1;
    return dim - 1 - r;
  }
  return r;
}

// Full / Parity: the XOR mask in index space that takes a row whose bits a and b differ to its partner (Parity: the
// index is the configuration without site 0).  xsec != 0 and a bond at site L - 1: the mask of the complement, *flipped
// set.
DNM_PM_HD uint64_t swap_index_mask(bool parity, int L, int a, int b, int xsec, int *flipped) {
  uint64_t m = ((uint64_t)1 << a) ^ ((uint64_t)1 << b);
  *flipped = xsec != 0 && (a == L - 1 || b == L - 1);
  if (*flipped) m ^= L >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << L) - 1);
  return parity ? m >> 1 : m;
}

}  // namespace dnm
