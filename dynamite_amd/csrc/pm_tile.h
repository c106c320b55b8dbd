// The panel scheme of the Gram-matrix sweeps as functions: G = A^H A for an operand matrix A of 16 NB columns whose
// panels of 2^B rows a workgroup stages in LDS -- the Hermitian rank-4 steps on v_mfma_f64_16x16x4_f64, the sum of the
// four wavefronts through LDS in a fixed order and the sum of the workgroups' partial tiles.  A sweep adds the panel
// fill.  swap_kernels.hip (bond swaps) is built on them.  pm_kernels.hip (sigma+ sigma-), where the scheme comes from,
// keeps its own text of the same steps: taken through these functions, pm_moments_kernel<Full / Parity, 1..3> came out
// of the compiler with 2 to 4 vector registers fewer (40 -> 36, 76 -> 74, 140 -> 138; AGPRs, scratch and LDS
// unchanged), and its measured times (docs/lab/sigma_pm_correlations.md) belong to the code as it stands.
//   Re G = Ar^T Ar + Ai^T Ai   (symmetric: lower-triangle tiles, both products into one accumulator)
//   Q    = Ar^T Ai             (all tiles),   Im G = Q - Q^T
// partial: [workgroup][Re tile (ti, tj), tj <= ti, at ti (ti + 1) / 2 + tj; then Q tile (ti, tj) at NT + ti NB + tj]
// [16 x 16 row-major] doubles, NT = NB (NB + 1) / 2.
#pragma once
#include "rdm_tile.h"

namespace dnm {

constexpr int PM_NT = 256;                      // threads of a workgroup: four wavefronts, one per SIMD
constexpr int64_t PM_MAX_WG = 1024;
constexpr size_t PM_LDS_BUDGET = 152 * 1024;    // of the 160 KB of a CU

static inline int pm_nacc(int nb) { return nb * (nb + 1) / 2 + nb * nb; }

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

// the four wavefronts, summed in the order ((0 + 1) + 2) + 3 through `red` (the panel's LDS, NACC * 256 doubles), and
// the workgroup's partial tiles written by wavefront 0; C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
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

}  // namespace dnm
