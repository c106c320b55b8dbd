// Ranking for the sigma+ sigma- pass on SpinConserve(L, k) (pm_kernels.hip, dnm_pm_partner_indices), for host and
// device alike -- tests/pm_rank_check.cpp runs these very functions under the sanitizers.
//
// sigma_minus(j) sets bit j, so the rows r of the operand matrix A[r, j] = psi(r ^ e_j) are the configurations with
// K = k + 1 set bits and the partner of row r for site j, a set bit of r, is r without that bit.  With the set bits
// p_0 < p_1 < ... < p_k of r and j = p_c, the colex rank of r ^ e_j in sector k is
//   sum_{m < c} C(p_m, m + 1) + sum_{m > c} C(p_m, m)
// (the bits below j keep their place in the order, the bits above move down by one): two running sums per row, no
// second ranking.  Binomials come from a table t[m * ld + n] = C(n, m), 0 <= m <= K, 0 <= n <= L, ld >= L + 1, with
// zeros where m > n (pm_binomials).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define DNM_PM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DNM_PM_HD inline
#endif

namespace dnm {

// t[(kmax + 1) * ld], ld >= L + 1; L <= 64: every entry is at most C(64, 32) < 2^63
inline void pm_binomials(int L, int kmax, int ld, int64_t *t) {
  for (int m = 0; m <= kmax; ++m)
    for (int n = 0; n <= L; ++n) {
      int64_t v;
      if (m == 0) v = 1;
      else if (n == 0) v = 0;
      else v = t[(m - 1) * ld + (n - 1)] + t[m * ld + (n - 1)];
      t[m * ld + n] = v;
    }
}

// the configuration with K set bits of colex rank idx: Sub<DNM_SPIN_CONSERVE>::i2s step for step, on this table
DNM_PM_HD uint64_t pm_unrank(int64_t idx, int L, int K, const int64_t *t, int ld) {
  uint64_t st = 0;
  int k = K;
  for (int n = L; n > 0; --n) {
    const int64_t here = t[k * ld + (n - 1)];       // (0 where k > n - 1: the bit is then set)
    st <<= 1;
    if (k > 0 && idx >= here) {
      idx -= here;
      --k;
      st |= 1;
    }
  }
  return st;
}

// f(j, index in sector K - 1 of r ^ e_j) for every set bit j of r, in ascending order of j
template <class F>
DNM_PM_HD void pm_partners(uint64_t r, const int64_t *t, int ld, F f) {
  int64_t hi = 0, lo = 0;
  int m = 0;
  for (uint64_t v = r; v; v &= v - 1, ++m)
    if (m) hi += t[m * ld + __builtin_ctzll(v)];
  int c = 0;
  for (uint64_t v = r; v; v &= v - 1, ++c) {
    const int p = __builtin_ctzll(v);
    if (c) hi -= t[c * ld + p];
    f(p, lo + hi);
    lo += t[(c + 1) * ld + p];
  }
}

}  // namespace dnm
