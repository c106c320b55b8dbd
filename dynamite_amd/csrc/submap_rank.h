// Index arithmetic of the subspace maps (submap_kernels.hip, dnm_subspace_map_indices), for host and device alike --
// tests/submap_rank_check.cpp runs these very functions under the sanitizers.
//
// A map takes a state from one subspace to another of the same L spins: the result is the orthogonal projection, onto
// the span of the target subspace, of the source state seen as a vector of the whole 2^L space -- an embedding when the
// source's configurations lie in the target's, a restriction the other way round; nothing is normalised.  With psi(c)
// the amplitude of configuration c in the source,
//   source without XParity        psi(c) = x[i_src(c)], 0 when c is not in the source;
//   source on XParity sector s    psi(c) = kappa x[i(c)] for c in the parent with bit L - 1 clear, kappa s x[i(cbar)] with
//                                 it set, cbar = c with all L spins flipped, kappa = SUBMAP_KAPPA;
// and for the target row r of configuration c (the representative, bit L - 1 clear, under an XParity sector t)
//   plain     -> plain      y[r] = x[i_src(c)] or 0                    (SUBMAP_COPY: the bits of x)
//   XParity s -> plain      y[r] = (+-kappa) x[.] or 0                 (SUBMAP_FROM_SECTOR: one multiply per component)
//   plain     -> XParity t  y[r] = (psi(c) + t psi(cbar)) kappa        (SUBMAP_TO_SECTOR: one add, one multiply)
//   XParity s -> XParity t  y[r] = x[i(c)] if s == t and c lies in the source's parent, else 0   (SUBMAP_COPY)
// In every case y[r] = scale * sum_{m < 2} sign[m] x[idx[m]] with at most two terms (submap_terms), scale 1 or kappa.
//
// Positions.  A Full / Parity vector is read and written as it lies: the element of index i sits at vec_pos(i, swz) of
// its own descriptor, and vec_pos is an involution, so the index of the row at position p is vec_pos(p, swz) too.  An
// XParity vector holds the first half of its parent's rows (the representatives) and keeps the parent's swizzle, which
// leaves the top index bit alone.  SpinConserve is in reference order, Explicit in list order.  The complement of the
// row of index i is the row dim - 1 - i wherever the subspace carries the flip in closed form (Full, Parity with even
// L, SpinConserve(L, L / 2): SubmapSide::closed); anywhere else it is looked up like any configuration.  L <= 63.
#pragma once

#include <cstdint>

#include "../../include/dynamite_amd.h"
#include "subspace.h"
#include "pm_rank.h"
#include "perm_rank.h"

namespace dnm {

constexpr double SUBMAP_KAPPA = 0.70710678118654752440;      // M_SQRT1_2

enum { SUBMAP_COPY = 0, SUBMAP_FROM_SECTOR = 1, SUBMAP_TO_SECTOR = 2 };

// One side of a map.  v: the (parent) subspace -- its tables are host pointers on the host and device or LDS pointers
// in a kernel; xsec: 0, or the XParity sector +-1 whose representatives the vector holds
struct SubmapSide {
  SubView v;
  int32_t xsec;
  int32_t closed;      // the complement of row i is row dim - 1 - i
  int64_t dim;         // rows of the (parent) subspace
  int64_t rows;        // elements of the vector: dim, or dim / 2 under XParity
};

// at most two amplitudes of the source enter a row of the target: positions in the source vector as it lies (-1: none)
// and their signs (0: none)
struct SubmapTerms {
  int64_t idx[2];
  int32_t sign[2];
};

DNM_HD int submap_mode(int src_xsec, int dst_xsec) {
  if (src_xsec) return dst_xsec ? SUBMAP_COPY : SUBMAP_FROM_SECTOR;
  return dst_xsec ? SUBMAP_TO_SECTOR : SUBMAP_COPY;
}
DNM_HD double submap_scale(int mode) { return mode == SUBMAP_COPY ? 1.0 : SUBMAP_KAPPA; }

DNM_HD uint64_t submap_all_sites(int L) { return L >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << L) - 1); }

// position <-> index of an element of a vector of subspace type T (an involution)
template <int T>
DNM_HD int64_t submap_pos(int64_t i, const SubView &v) {
  return (T == DNM_FULL || T == DNM_PARITY) ? vec_pos(i, v.swz) : i;
}

// the configuration of the row at position p of a vector of subspace type T
template <int T>
DNM_HD uint64_t submap_row_config(int64_t p, const SubView &v) {
  return (uint64_t)Sub<T>::i2s(submap_pos<T>(p, v), v);
}

// the terms of the target row of configuration c (the representative under a target sector dst_xsec != 0) from a
// source of subspace type ST
template <int ST>
DNM_HD void submap_terms(uint64_t c, const SubmapSide &s, int dst_xsec, SubmapTerms *out) {
  out->idx[0] = out->idx[1] = -1;
  out->sign[0] = out->sign[1] = 0;
  const int L = s.v.L;
  const uint64_t all = submap_all_sites(L);
  if (c & ~all) return;                    // (a listed state of more than L bits: in no subspace of L spins)
  if (s.xsec) {
    if (dst_xsec && dst_xsec != s.xsec) return;               // the two sectors are orthogonal
    const int fl = (int)((c >> (L - 1)) & 1);                  // (never set for a representative)
    const int64_t i = Sub<ST>::s2i((int64_t)(fl ? c ^ all : c), s.v);
    if (i < 0 || i >= s.rows) return;
    out->idx[0] = submap_pos<ST>(i, s.v);
    out->sign[0] = fl ? s.xsec : 1;
    return;
  }
  const int64_t i = Sub<ST>::s2i((int64_t)c, s.v);
  if (i >= 0) {
    out->idx[0] = submap_pos<ST>(i, s.v);
    out->sign[0] = 1;
  }
  if (dst_xsec) {
    int64_t j;
    if (ST != DNM_EXPLICIT && s.closed) j = i >= 0 ? s.dim - 1 - i : -1;
    else j = Sub<ST>::s2i((int64_t)(c ^ all), s.v);
    if (j >= 0) {
      out->idx[1] = submap_pos<ST>(j, s.v);
      out->sign[1] = dst_xsec;
    }
  }
}

// ---- sector weights ------------------------------------------------------------------------------------------------
// the number of set bits of the row of index i of subspace type T (spins beyond L in a listed state are ignored)
template <int T>
DNM_HD int submap_row_popcount(int64_t i, const SubView &v) {
  if (T == DNM_SPIN_CONSERVE) return v.k;
  return hd_popc((uint64_t)Sub<T>::i2s(i, v) & submap_all_sites(v.L));
}

}  // namespace dnm
