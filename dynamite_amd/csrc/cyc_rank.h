// Partner arithmetic of the three-site rotation pass (cyc_kernels.hip, dnm_cyc_partner_indices), for host and device
// alike -- tests/cyc_rank_check.cpp runs these very functions under the sanitizers.
//
// C = P_ab P_bc rotates the spins of the oriented triple (a, b, c): the partner r' of a configuration r has bit a = bit
// b of r, bit b = bit c of r, bit c = bit a of r.  Site a changes where x_a != x_b, site b where x_b != x_c, site c
// where x_c != x_a: none where the three bits are equal, otherwise exactly two, and those two differ -- the rotation
// is then the exchange of those two sites and everything of swap_rank.h serves as it stands: the colex difference
// form for SpinConserve and, for a state on an XParity sector, the complement's amplitude times the sector's sign
// where site L - 1 is one of the two (the rows are the representatives, bit L - 1 clear, so a change sets it).
//
// Full / Parity: the partner of index i is i ^ (M_a & -d_a) ^ (M_b & -d_b) ^ (M_c & -d_c) with one mask per site
// (Parity: the index is the configuration without site 0, whose mask is 0) and, where the change sets bit L - 1 under
// XParity, one more XOR with the complement's mask.  The XOR swizzle of the vector is linear, so the same form holds
// in position space with every mask taken through vec_pos.
#pragma once

#include <cstdint>

#include "swap_rank.h"

namespace dnm {

// Which sites the rotation of (a, b, c) changes in configuration cfg: bit 0 of the result for a, bit 1 for b, bit 2 for
// c -- 0 (the three bits are equal: the partner is the row itself) or exactly two bits, and then *p, *q are those two
// sites, whose bits differ.
DNM_PM_HD int cyc_changed(uint64_t cfg, int a, int b, int c, int *p, int *q) {
  const int xa = (int)((cfg >> a) & 1), xb = (int)((cfg >> b) & 1), xc = (int)((cfg >> c) & 1);
  const int da = xa ^ xb, db = xb ^ xc, dc = xc ^ xa;
  *p = da ? a : b;
  *q = dc ? c : b;
  return da | (db << 1) | (dc << 2);
}

// the changed sites `d` of (a, b, c) hold site L - 1 on a state of an XParity sector: the partner is the complement's
// amplitude and carries the sector's sign
DNM_PM_HD int cyc_flipped(int d, int a, int b, int c, int L, int xsec) {
  if (xsec == 0) return 0;
  return ((d & 1) && a == L - 1) || ((d & 2) && b == L - 1) || ((d & 4) && c == L - 1);
}

// Full / Parity: the index-space mask of a change of site s, and of the complement of all L sites
DNM_PM_HD uint64_t cyc_site_mask(bool parity, int s) {
  const uint64_t m = (uint64_t)1 << s;
  return parity ? m >> 1 : m;
}
DNM_PM_HD uint64_t cyc_all_mask(bool parity, int L) {
  const uint64_t m = L >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << L) - 1);
  return parity ? m >> 1 : m;
}

// Full / Parity: the partner of index (or position) i for the changed sites d, with the masks of a, b, c and -- where
// the partner is the complement's (fl) -- of all sites, each in the space of i
DNM_PM_HD int64_t cyc_xor_partner(int64_t i, int d, int fl, uint64_t ma, uint64_t mb, uint64_t mc, uint64_t mall) {
  const uint64_t m = (ma & (uint64_t)-(int64_t)(d & 1)) ^ (mb & (uint64_t)-(int64_t)((d >> 1) & 1)) ^
                     (mc & (uint64_t)-(int64_t)((d >> 2) & 1)) ^ (mall & (uint64_t)-(int64_t)(fl != 0));
  return i ^ (int64_t)m;
}

// SpinConserve: index into the vector of the partner of row `row` (configuration cfg, colex rank row) for the triple
// (a, b, c); xsec, dim, *flipped as swap_sc_partner
DNM_PM_HD int64_t cyc_sc_partner(uint64_t cfg, int64_t row, int a, int b, int c, int L, int64_t dim, int xsec,
                                 const int64_t *t, int ld, int *flipped) {
  int p, q;
  *flipped = 0;
  if (cyc_changed(cfg, a, b, c, &p, &q) == 0) return row;
  return swap_sc_partner(cfg, row, p, q, L, dim, xsec, t, ld, flipped);
}

}  // namespace dnm
