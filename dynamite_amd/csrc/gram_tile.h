// The panel scheme of the Gram-matrix sweeps: G = A^H A for an operand matrix A of 16 NB columns whose panels of 2^B
// rows a workgroup stages in LDS -- the plan of a sweep, the Hermitian rank-4 steps on v_mfma_f64_16x16x4_f64, the sum
// of the four wavefronts through LDS in a fixed order, the sum of the workgroups' partial tiles and the choice of a
// kernel instance by subspace type and tile rows.  A sweep adds the panel fill: pm_kernels.hip (sigma+ sigma-),
// swap_kernels.hip (bond swaps), cyc_kernels.hip (three-site rotations, on the bond swaps' plan) and pauli_kernels.hip
// (single-site Paulis, on that plan too).  zz_kernels.hip
// (sigma-z: real symmetric, no panel) takes the wave sum and the choice of the instance.
//   Re G = Ar^T Ar + Ai^T Ai   (symmetric: lower-triangle tiles, both products into one accumulator)
//   Q    = Ar^T Ai             (all tiles),   Im G = Q - Q^T
// partial: [workgroup][Re tile (ti, tj), tj <= ti, at ti (ti + 1) / 2 + tj; then Q tile (ti, tj) at NT + ti NB + tj]
// [16 x 16 row-major] doubles, NT = NB (NB + 1) / 2.
#pragma once
#include <type_traits>

#include "rdm_tile.h"

namespace dnm {

constexpr int PM_NT = 256;                      // threads of a workgroup: four wavefronts, one per SIMD
constexpr int64_t PM_MAX_WG = 1024;
constexpr size_t PM_LDS_BUDGET = 152 * 1024;    // of the 160 KB of a CU

static inline int pm_nacc(int nb) { return nb * (nb + 1) / 2 + nb * nb; }

// What a sweep is launched with: host arithmetic from the subspace alone.  K, dim: the sweep's own (dim: the (parent)
// subspace of the bond swaps).
struct GramPlan {
  int32_t nb, B, nwg, K;          // tile rows, log2 of the panel's rows, workgroups, set bits of a row (SpinConserve)
  int64_t nrows, dim, npanels, per_wg;      // rows of the sweep; panels in all and per workgroup
  size_t lds_bytes, table_bytes;  // dynamic LDS of a launch; of it the binomial table (SpinConserve)
  size_t partial_bytes;           // nwg * (NT + nb^2) * 256 doubles, NT = nb (nb + 1) / 2
};

// The panel and the shares of a sweep of nrows rows of ncols columns: 2^b_max rows at one tile row, 2^b_max_wide from two
// on (b_forced in [b_min, b_max]: that one instead), lowered down to 2^b_min while panel and table exceed the budget;
// `nwg` workgroups as the sweep decides, never more than panels or PM_MAX_WG, at least one.  False: the panel does not
// fit, or the reduction buffer of the wavefronts' sum, which takes the panel's place after the sweep, does not fit in
// it (q->lds_bytes is set for the caller's message).
static inline bool gram_plan(int ncols, int64_t nrows, size_t table_bytes, int b_max, int b_max_wide, int b_min,
                             int b_forced, int64_t nwg, GramPlan *q) {
  q->nb = (ncols + 15) / 16;
  q->nrows = nrows;
  q->table_bytes = table_bytes;
  const size_t row_bytes = (size_t)(16 * q->nb + 1) * 16;
  q->B = q->nb == 1 ? b_max : b_max_wide;
  if (b_forced >= b_min && b_forced <= b_max) q->B = b_forced;
  while (q->B > b_min && (row_bytes << q->B) + table_bytes > PM_LDS_BUDGET) --q->B;
  q->lds_bytes = (row_bytes << q->B) + table_bytes;
  if (q->lds_bytes > PM_LDS_BUDGET || (size_t)pm_nacc(q->nb) * 256 * sizeof(double) > (row_bytes << q->B)) return false;
  q->npanels = (nrows + ((int64_t)1 << q->B) - 1) >> q->B;
  if (nwg > q->npanels) nwg = q->npanels;
  if (nwg > PM_MAX_WG) nwg = PM_MAX_WG;
  if (nwg < 1) nwg = 1;
  q->nwg = (int)nwg;
  q->per_wg = (q->npanels + nwg - 1) / nwg;
  q->partial_bytes = (size_t)nwg * (size_t)pm_nacc(q->nb) * 256 * sizeof(double);
  return true;
}

// f(std::integral_constant<int, TYPE>, std::integral_constant<int, NB>) for the subspace type and the 1 to 4 tile rows of
// a launch: Full, Parity, SpinConserve and, where the sweep has them, Explicit subspaces.  `what`: the sweep, for the
// message about the tile rows; bad_type: the message about the type, a format that is handed it.
template <bool WITH_EXPLICIT, class F>
static int gram_dispatch(int type, int nb, const char *what, const char *bad_type, F f) {
  auto by_nb = [&](auto t) {
    switch (nb) {
      case 1: return f(t, std::integral_constant<int, 1>{});
      case 2: return f(t, std::integral_constant<int, 2>{});
      case 3: return f(t, std::integral_constant<int, 3>{});
      case 4: return f(t, std::integral_constant<int, 4>{});
    }
    set_error("internal: %d tile rows of %s", nb, what);
    return 1;
  };
  switch (type) {
    case DNM_FULL: return by_nb(std::integral_constant<int, DNM_FULL>{});
    case DNM_PARITY: return by_nb(std::integral_constant<int, DNM_PARITY>{});
    case DNM_SPIN_CONSERVE: return by_nb(std::integral_constant<int, DNM_SPIN_CONSERVE>{});
    case DNM_EXPLICIT:
      if constexpr (WITH_EXPLICIT) return by_nb(std::integral_constant<int, DNM_EXPLICIT>{});
      break;
  }
  set_error(bad_type, type);
  return 1;
}

// the panel's steps of four rows, shared among the four wavefronts: 2 NT + NB^2 MFMAs per step; panel rows have
// 16 NB + 1 amplitudes (an odd stride spreads a column's stores)
template <int NB>
__device__ __forceinline__ void pm_tile_multiply(const c128 *panel, int rows, int wave, int slot, int r,
                                                 mfma_acc (&acc)[NB * (NB + 1) / 2 + NB * NB]) {
  constexpr int NTILE = NB * (NB + 1) / 2, LDP = 16 * NB + 1;
  for (int q = wave; q < rows / 4; q += PM_NT / 64) {
    const c128 *pr = panel + (4 * q + slot) * LDP + r;
    c128 v[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) v[t] = pr[16 * t];
#pragma unroll
    for (int ti = 0; ti < NB; ++ti)
#pragma unroll
      for (int tj = 0; tj <= ti; ++tj) {
        const int i = ti * (ti + 1) / 2 + tj;
        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti].x, v[tj].x, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti].y, v[tj].y, acc[i], 0, 0, 0);
      }
#pragma unroll
    for (int ti = 0; ti < NB; ++ti)
#pragma unroll
      for (int tj = 0; tj < NB; ++tj) {
        const int i = NTILE + ti * NB + tj;
        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti].x, v[tj].y, acc[i], 0, 0, 0);
      }
  }
}

// the four wavefronts, summed in the order ((0 + 1) + 2) + 3 through `red` (LDS, NACC * 256 doubles: the panel's once
// the sweep is done), and the workgroup's partial tiles written by wavefront 0; C/D layout: col = lane & 15,
// row = (lane >> 4) + 4 * reg
template <int NACC>
__device__ __forceinline__ void pm_tile_reduce_store(double *red, int wave, int slot, int r, mfma_acc (&acc)[NACC],
                                                     double *__restrict__ out) {
  for (int wv = 1; wv < PM_NT / 64; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) red[i * 256 + (slot + 4 * gq) * 16 + r] = acc[i][gq];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) acc[i][gq] += red[i * 256 + (slot + 4 * gq) * 16 + r];
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) out[i * 256 + (slot + 4 * gq) * 16 + r] = acc[i][gq];
  }
}

// G (D x D complex128, row-major) from the workgroups' partial tiles, summed in their order: entry (a, b), b <= a, is
// (Re[a][b], Q[a][b] - Q[b][a]); the upper triangle is its conjugate and the diagonal real.  One workgroup of PM_NT
// threads per lower-triangle tile.
__device__ __forceinline__ void pm_tile_finalize(const double *__restrict__ partial, int nwg, int nb, int D,
                                                 c128 *__restrict__ out) {
  int ti, tj;
  rdm_tile_coords(blockIdx.x, &ti, &tj);
  const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
  const int a = ti * 16 + row, b = tj * 16 + col;
  if (a >= D || b >= D || b > a) return;
  const int ntile = nb * (nb + 1) / 2, nacc = ntile + nb * nb;
  const int64_t e_re = (int64_t)blockIdx.x * 256 + row * 16 + col;
  const int64_t e_ab = (int64_t)(ntile + ti * nb + tj) * 256 + row * 16 + col;
  const int64_t e_ba = (int64_t)(ntile + tj * nb + ti) * 256 + col * 16 + row;
  double re = 0.0, qab = 0.0, qba = 0.0;
  for (int g = 0; g < nwg; ++g) {
    const double *p = partial + (int64_t)g * nacc * 256;
    re += p[e_re];
    qab += p[e_ab];
    qba += p[e_ba];
  }
  const double im = a == b ? 0.0 : qab - qba;
  out[a * D + b] = make_double2(re, im);
  if (a != b) out[b * D + a] = make_double2(re, -im);
}

// The plan of the bond-swap sweep (swap_kernels.hip) with the pass named for its messages: ncols - 1 partner columns
// beside the state's own.
int swap_plan(int type, int L, int k, int nbonds, int xsec, GramPlan *p, const char *what);

// All three-site rotations of a state (cyc_kernels.hip): G = A^H A, A[r, 0] = x(r), A[r, 1 + m] = x(r with the bits of
// the triple m rotated: bit a <- bit b <- bit c <- bit a) over the rows r of the subspace (xsec = +-1: the
// representatives of the XParity sector, type / L the parent's); (n + 1) x (n + 1) result.  p: swap_plan(..., ncycles,
// ...).  x: the whole state (device; Full / Parity as it lies in the swizzled layout swz, SpinConserve in reference
// order); cycles: 3 ncycles sites (host); nck: pm_binomials(L, k, L + 1) on the device (SpinConserve); partial:
// p.partial_bytes; out: (ncycles + 1)^2 complex128 (device)
int launch_cyc_moments(const void *x, int type, int L, int space, int swz, int xsec, int ncycles, const int32_t *cycles,
                       const GramPlan &p, const int64_t *nck, void *partial, void *out, hipStream_t st);

// All single-site Pauli columns of a state (pauli_kernels.hip): G = A^H A, A[q, 0] = x(q), A[q, 1 + c] = +-x(q ^ m_c) for
// the columns c = (site, kind: 1 flip, 2 flip and sign, 3 sign) of pauli_cols.h over the rows q of a Full or Parity
// vector; (ncols + 1) x (ncols + 1) result, on Parity with the entries between a flipping and a non-flipping column
// still to be zeroed by the caller.  p: swap_plan(type, L, 0, ncols, 0, ...).  x: the whole state (device, as it lies in
// the swizzled layout swz); cols: 2 ncols ints (host); partial: p.partial_bytes; out: (ncols + 1)^2 complex128 (device)
int launch_pauli_moments(const void *x, int type, int L, int space, int swz, int ncols, const int32_t *cols,
                         const GramPlan &p, void *partial, void *out, hipStream_t st);

}  // namespace dnm
