// All two-spin Pauli correlators of a state in one pass over it, for states without a U(1) symmetry.  Each single-site
// Pauli applied to psi is one partner amplitude times a sign (pauli_cols.h), so with the operand matrix over the rows q
// of the vector
//   A[q, 0] = psi(q),   A[q, 1 + c] = (-1)^(g_c bit j_c of r_c(q)) psi(q ^ m_c)
// for the columns c = (site j_c, kind: 1 flip, 2 flip and sign, 3 sign) the Gram matrix G = A^H A ((n + 1) x (n + 1)
// complex128, Hermitian) holds every <sigma^a_i sigma^b_j> up to the phase -i of a sigma-y column, which the caller
// applies: the Hermitian rank-N update of gram_tile.h on v_mfma_f64_16x16x4_f64, NB = ceil((n + 1) / 16) <= 4 tile rows.
// Full and Parity only: a flip leaves a SpinConserve sector.  On Parity a flipping column holds the rows of the
// opposite sector; the entries of G between a flipping and a non-flipping column would pair rows of two different
// sectors, vanish by symmetry and are written as zeros by the caller (observables.cpp).
//
// Panel fill: a thread owns a row of the panel -- adjacent threads adjacent rows -- loads its own amplitude once and
// walks the columns in the host's order: the flipping columns sorted by site, then the others.  The first flipping
// column of a site loads the partner, one load per (row, site); the columns that follow at the same site (the other
// kind, a repeat) take it from the register, and a column that only signs takes the row's own amplitude.  The vector
// is read as it lies: the XOR swizzle is linear, so in position space the partner of position p is p ^ mask with one
// mask per column from the host, and a wavefront reads an aligned 1 KB run of the vector, permuted inside the run by
// the low bits of the mask.  A flip of site 0 on Parity has mask 0: the partner is the row's own amplitude.
//
// The plan is that of the bond-swap sweep (swap_plan: SWAP_B_* for the panel, one workgroup per 2^9 rows): the rule is
// inherited, not measured for this fill.
//
// No atomics: wavefronts and workgroups are summed in a fixed order (gram_tile.h).  The number of workgroups follows from
// the number of rows alone: two calls return the same bits on any device.
#include "gram_tile.h"
#include "pauli_cols.h"

#include <algorithm>

namespace dnm {

struct PauliArgs {
  int64_t nrows, npanels, per_wg;
  int32_t B, space, swz, n;
  // the columns in the order of the fill
  uint64_t mask[63];          // partner of position p = p ^ mask (read where load is set)
  int8_t dst[63];             // the column of A, less one
  int8_t site[63], kind[63];
  int8_t load[63];            // the first flipping column of a site whose mask is not 0: fetch the partner
};

template <int TYPE, int NB>
__global__ void __launch_bounds__(PM_NT)
pauli_moments_kernel(const c128 *__restrict__ x, const PauliArgs a, double *__restrict__ partial) {
  constexpr int NACC = NB * (NB + 1) / 2 + NB * NB;
  constexpr int LDP = 16 * NB + 1;
  constexpr bool PARITY = TYPE == DNM_PARITY;
  extern __shared__ __align__(16) unsigned char pauli_lds[];
  c128 *panel = reinterpret_cast<c128 *>(pauli_lds);
  const int tid = threadIdx.x;
  const int rows = 1 << a.B;
  // (the padding column and the columns at or beyond n + 1 stay zero for the whole sweep)
  for (int e = tid; e < LDP * rows; e += PM_NT) panel[e] = make_double2(0.0, 0.0);
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, slot = lane >> 4;
  mfma_acc acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = mfma_acc{0.0, 0.0, 0.0, 0.0};

  const int64_t g0 = (int64_t)blockIdx.x * a.per_wg;
  int64_t g1 = g0 + a.per_wg;
  if (g1 > a.npanels) g1 = a.npanels;
  for (int64_t g = g0; g < g1; ++g) {
    const int64_t base = g << a.B;
    for (int t = tid; t < rows; t += PM_NT) {
      c128 *prow = panel + t * LDP;
      const int64_t p = base + t;
      if (p >= a.nrows) {
        for (int m = 0; m <= a.n; ++m) prow[m] = make_double2(0.0, 0.0);
        continue;
      }
      const c128 self = x[p];
      prow[0] = self;
      const uint64_t idx = (uint64_t)vec_pos(p, a.swz);
      const int par = PARITY ? hd_par(idx) : 0;
      c128 v = self;           // the partner in hand: the row's own until a column fetches one
#pragma unroll 4
      for (int k = 0; k < a.n; ++k) {
        const int kind = a.kind[k];
        const bool fl = pauli_flips(kind);
        if (a.load[k]) v = x[p ^ (int64_t)a.mask[k]];
        c128 w = fl ? v : self;
        if (pauli_negative(pauli_row_config(PARITY, a.space, idx, par, fl), a.site[k], kind))
          w = make_double2(-w.x, -w.y);
        prow[1 + a.dst[k]] = w;
      }
    }
    __syncthreads();
    pm_tile_multiply<NB>(panel, rows, wave, slot, r, acc);
    __syncthreads();
  }
  pm_tile_reduce_store<NACC>(reinterpret_cast<double *>(pauli_lds), wave, slot, r, acc,
                             partial + (int64_t)blockIdx.x * (NACC * 256));
}

__global__ void __launch_bounds__(PM_NT)
pauli_finalize_kernel(const double *__restrict__ partial, int nwg, int nb, int D, c128 *__restrict__ out) {
  pm_tile_finalize(partial, nwg, nb, D, out);
}

int launch_pauli_moments(const void *x, int type, int L, int space, int swz, int ncols, const int32_t *cols,
                         const GramPlan &p, void *partial, void *out, hipStream_t st) {
  if (type != DNM_FULL && type != DNM_PARITY) {
    set_error("Pauli moments: subspace type %d", type);
    return 1;
  }
  PauliArgs a{};
  a.nrows = p.nrows;
  a.npanels = p.npanels;
  a.per_wg = p.per_wg;
  a.B = p.B;
  a.space = space;
  a.swz = swz;
  a.n = ncols;
  // the order of the fill: flipping columns by site, then the columns that only sign (a stable sort: the same order
  // for the same list, whatever the host)
  int order[63];
  for (int c = 0; c < ncols; ++c) order[c] = c;
  auto key = [&](int c) { return pauli_flips(cols[2 * c + 1]) ? cols[2 * c] : L; };
  std::stable_sort(order, order + ncols, [&](int c, int d) { return key(c) < key(d); });
  for (int k = 0; k < ncols; ++k) {
    const int c = order[k], site = cols[2 * c], kind = cols[2 * c + 1];
    a.dst[k] = (int8_t)c;
    a.site[k] = (int8_t)site;
    a.kind[k] = (int8_t)kind;
    // the index-space partner mask of the column, taken through the swizzle
    a.mask[k] = (uint64_t)vec_pos((int64_t)pauli_index_mask(type == DNM_PARITY, site, kind), swz);
    const bool first = k == 0 || key(order[k - 1]) != key(c);
    a.load[k] = (int8_t)(pauli_flips(kind) && first && a.mask[k] != 0);
  }
  const c128 *xp = (const c128 *)x;
  double *pp = (double *)partial;
  DNM_TRY(gram_dispatch<false>(type, p.nb, "Pauli moments", "Pauli moments: subspace type %d", [&](auto T, auto NB) {
    constexpr int TYPE = decltype(T)::value;
    if constexpr (TYPE == DNM_FULL || TYPE == DNM_PARITY) {
      auto k = pauli_moments_kernel<TYPE, decltype(NB)::value>;
      DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
      hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(PM_NT), p.lds_bytes, st, xp, a, pp);
      DNM_HIP(hipGetLastError());
      return 0;
    } else {
      set_error("Pauli moments: subspace type %d", TYPE);
      return 1;
    }
  }));
  hipLaunchKernelGGL(pauli_finalize_kernel, dim3((unsigned)(p.nb * (p.nb + 1) / 2)), dim3(PM_NT), 0, st,
                     (const double *)pp, p.nwg, p.nb, ncols + 1, (c128 *)out);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
