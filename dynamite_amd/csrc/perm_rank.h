// Index arithmetic of the site-permutation pass (perm_kernels.hip, dnm_perm_partner_indices), for host and device alike
// -- tests/perm_rank_check.cpp runs these very functions under the sanitizers.
//
// A site permutation is an int array pi of length L, a bijection of [0, L).  P_pi moves the spin at site i to site pi(i):
// P_pi |c> = |c'> with c'_{pi(i)} = c_i, so (P_pi psi)(c') = psi(c) where the SOURCE configuration c has bit i equal to
// bit pi(i) of c'.  Consequence: P_pi sigma^a_i P_pi^H = sigma^a_{pi(i)}.  The three-site rotation of cyc_rank.h for the
// triple (a, b, c) is pi(a) = b, pi(b) = c, pi(c) = a, all else fixed.
//
// The source is built from the set bits of the row's configuration c': set bit p of c' is set bit inv(p) of c, inv =
// pi^-1 -- popcount(c') short steps where a loop over the sites takes L.  A permutation keeps the number of set bits
// and the parity and commutes with the global flip, so the source of a row of Full, Parity or SpinConserve is a row of
// the same subspace.  Its index into the vector:
//   Full          the configuration itself (the caller takes it through vec_pos for a swizzled vector);
//   Parity        the configuration without site 0;
//   SpinConserve  the colex rank sum_j C(p_j, j + 1) over its set bits p_0 < p_1 < ..., on pm_rank.h's table t[m * ld + n]
//                 = C(n, m) with rows 0 <= m <= k: k more steps, the largest row read is k.
// XParity sector s = +-1: the vector holds the representatives (bit L - 1 clear).  A source whose bit L - 1 is set is s
// times the amplitude of its complement: one more XOR with the mask of all sites for Full / Parity, index dim - 1 - rank
// for SpinConserve(L, L / 2), where the complement reverses the colex order.  L <= 64.
#pragma once

#include <cstdint>

#include "pm_rank.h"

namespace dnm {

// inv[pi[i]] = i; false unless pi is a bijection of [0, L)
inline bool perm_invert(const int32_t *pi, int L, uint8_t *inv) {
  uint64_t seen = 0;
  for (int i = 0; i < L; ++i) {
    if (pi[i] < 0 || pi[i] >= L || ((seen >> pi[i]) & 1)) return false;
    seen |= (uint64_t)1 << pi[i];
    inv[pi[i]] = (uint8_t)i;
  }
  return true;
}

// the source configuration of the row's configuration cfg: bit i = bit pi(i) of cfg
DNM_PM_HD uint64_t perm_source(uint64_t cfg, const uint8_t *inv) {
  uint64_t src = 0;
  for (uint64_t v = cfg; v; v &= v - 1) src |= (uint64_t)1 << inv[__builtin_ctzll(v)];
  return src;
}

// Full / Parity: the configuration of the row of index idx, and the index of a configuration
DNM_PM_HD uint64_t perm_index_config(bool parity, int space, uint64_t idx) {
  return parity ? (idx << 1) | (uint64_t)((__builtin_popcountll(idx) & 1) ^ space) : idx;
}

// Full / Parity: the index of the amplitude of the source configuration src; xsec != 0 and bit L - 1 of src set: that
// of its complement, *flipped set
DNM_PM_HD int64_t perm_xor_index(uint64_t src, bool parity, int L, int xsec, int *flipped) {
  *flipped = xsec != 0 && ((src >> (L - 1)) & 1);
  if (*flipped) src ^= L >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << L) - 1);
  return (int64_t)(parity ? src >> 1 : src);
}

// SpinConserve: the colex rank of a configuration with at most k set bits, k the last row of the table
DNM_PM_HD int64_t perm_sc_rank(uint64_t src, const int64_t *t, int ld) {
  int64_t r = 0;
  int j = 1;
  for (uint64_t v = src; v; v &= v - 1, ++j) r += t[j * ld + __builtin_ctzll(v)];
  return r;
}

// SpinConserve: the index of the amplitude of the source configuration src in a vector of SpinConserve (xsec == 0: dim
// rows) or of the representatives of an XParity sector over SpinConserve(L, L / 2) (dim / 2 rows; *flipped: the
// complement's amplitude)
DNM_PM_HD int64_t perm_sc_index(uint64_t src, int L, int64_t dim, int xsec, const int64_t *t, int ld, int *flipped) {
  const int64_t r = perm_sc_rank(src, t, ld);
  *flipped = xsec != 0 && ((src >> (L - 1)) & 1);
  return *flipped ? dim - 1 - r : r;
}

// SpinConserve: the configuration after cfg in colex order (Gosper's step, the division by the lowest set bit as a
// shift); cfg != 0 and not the last of its sector
DNM_PM_HD uint64_t perm_next_config(uint64_t cfg) {
  const uint64_t c = cfg & (~cfg + 1), r = cfg + c;
  return r | (((cfg ^ r) >> 2) >> __builtin_ctzll(cfg));
}

}  // namespace dnm
