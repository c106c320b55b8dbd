// The site-permutation pass (perm_kernels.hip): y = sum_g c_g P_g x and <phi|P_g|psi> for up to 64 permutations of the
// L sites in one pass over the state.  Definitions and index arithmetic: perm_rank.h.
#pragma once
#include <cstring>

#include "kernels.h"
#include "perm_rank.h"

namespace dnm {

constexpr int PERM_NT = 256;                // threads of a workgroup
constexpr int PERM_MAX = 64;                // permutations of one launch
constexpr int PERM_LD = 68;                 // bytes between the inverse permutations in LDS: 17 dwords, odd, so that
                                            // lanes on different permutations and one site read different banks
constexpr int PERM_RUN = 4;                 // SpinConserve: adjacent rows a thread unranks once and then steps through
constexpr int PERM_ROWS_PER_WG_LOG2 = 10;   // workgroups = ceil(rows / 2^10), at most PERM_MAX_WG, at least one
constexpr int64_t PERM_MAX_WG = 4096;

// What a launch is made with: host arithmetic from the subspace, the sector and the number of permutations alone.
struct PermPlan {
  int32_t nwg, K, ntab;            // workgroups; set bits of a row and entries of the binomial table (SpinConserve)
  int64_t nrows, dim;              // rows of the vector; dimension of the (parent) subspace
  size_t lds_bytes;                // the tables of a launch, in LDS and on the device: binomials, inverse permutations
  size_t partial_bytes;            // perm_dots: nwg * 2 nperm doubles
};

// type: DNM_FULL / DNM_PARITY / DNM_SPIN_CONSERVE, L <= 64; xsec = +-1: the rows are the representatives of the sector
int perm_plan(int type, int L, int k, int nperm, int xsec, PermPlan *p);

// the tables of a launch (host, p.lds_bytes): pm_binomials(L, K, L + 1) for SpinConserve, then the inverse of
// permutation g at byte p.ntab * 8 + g * PERM_LD; false: row g = *bad of perms is no bijection of [0, L)
inline bool perm_fill_tables(const PermPlan &p, int L, int nperm, const int32_t *perms, unsigned char *buf, int *bad) {
  memset(buf, 0, p.lds_bytes);
  if (p.ntab) pm_binomials(L, p.K, L + 1, reinterpret_cast<int64_t *>(buf));
  for (int g = 0; g < nperm; ++g)
    if (!perm_invert(perms + (size_t)g * L, L, buf + (size_t)p.ntab * 8 + (size_t)g * PERM_LD)) {
      *bad = g;
      return false;
    }
  return true;
}

// y[r] = (accumulate ? y[r] : 0) + sum_g coef_g s_g(r) x[p_g(r)] over the rows of the vector.  x, y: device, distinct,
// Full / Parity as they lie in the swizzled layout swz, SpinConserve in reference order; coef: 2 nperm doubles (host);
// tables: perm_fill_tables on the device
int launch_perm_apply(const void *x, void *y, int type, int L, int space, int swz, int xsec, int nperm,
                      const double *coef, int accumulate, const PermPlan &p, const void *tables, hipStream_t st);
// out[g] = sum_r conj(phi[r]) s_g(r) psi[p_g(r)] (device, 2 nperm doubles); partial: p.partial_bytes
int launch_perm_dots(const void *phi, const void *psi, int type, int L, int space, int swz, int xsec, int nperm,
                     const PermPlan &p, const void *tables, void *partial, void *out, hipStream_t st);

}  // namespace dnm
