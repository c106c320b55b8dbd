// All scalar-chirality correlators of a list of triangles in one pass over the state.  For spin 1/2
//   sigma_a . (sigma_b x sigma_c) = 2i (C - C^H),   C = P_ab P_bc
// the rotation of the three spins, so with the operand matrix over the rows r of the subspace
//   A[r, 0] = psi(r),   A[r, 1 + m] = psi(r with bit a_m <- bit b_m <- bit c_m <- bit a_m)
// the Gram matrix G = A^H A ((n + 1) x (n + 1) complex128, Hermitian) holds G[0][0] = <psi|psi>, G[0][1 + m] = <C_m> and
// G[1 + m][1 + m'] = <C_m^H C_m'>: the Hermitian rank-N update of gram_tile.h on v_mfma_f64_16x16x4_f64, NB = ceil((n + 1)
// / 16) <= 4 tile rows, with the plan of the bond-swap sweep (swap_plan: panel, workgroups, binomials).  The opposite
// rotation of (a, b, c) is the rotation of (a, c, b): one triple, one column.  A rotation permutes sites, so it keeps a
// row inside Full, Parity and SpinConserve and commutes with the global flip: for a state on an XParity sector s the
// rows are the representatives (bit L - 1 clear) and a partner whose bit L - 1 is set is s times the amplitude of its
// complement.
//
// Panel fill: a thread owns a row of the panel -- adjacent threads adjacent rows -- loads its own amplitude once and
// walks the triples.  Where the three bits are equal the partner is the row itself; otherwise exactly two sites change
// (cyc_rank.h: cyc_changed) and the rotation is their exchange.
// Full / Parity: the vector is read as it lies.  One position-space mask per site from the host (the index-space mask
// taken through the linear XOR swizzle; Parity's index does not hold site 0), the partner of position p is
// p ^ (M[a] & -d_a) ^ (M[b] & -d_b) ^ (M[c] & -d_c), and one more XOR with the complement's mask where the change sets
// bit L - 1 under XParity.
// SpinConserve: reference order.  A thread unranks its row (binomials in LDS) and ranks the exchange of the two changed
// sites by swap_rank.h's difference form; under XParity a partner with bit L - 1 set is fetched at dim - 1 - rank.
//
// No atomics: wavefronts and workgroups are summed in a fixed order (gram_tile.h).  The number of workgroups follows from
// the number of rows alone: two calls return the same bits on any device.
#include "gram_tile.h"
#include "cyc_rank.h"

namespace dnm {

struct CycArgs {
  int64_t nrows, npanels, per_wg, dim;
  int32_t L, B, K, ld, space, swz, n, xsec;
  double sign;                // the XParity sector, +-1 (1 without one)
  uint64_t mall;              // Full / Parity: the complement's mask in position space
  uint64_t site[64];          // Full / Parity: the mask of a change of site s in position space
  int8_t a[63], b[63], c[63];         // the triple's sites
};

// the configuration of the row at position p of the (swizzled) order
template <int TYPE>
__device__ __forceinline__ uint64_t cyc_row_config(int64_t p, const CycArgs &a) {
  const uint64_t idx = (uint64_t)vec_pos(p, a.swz);
  if (TYPE == DNM_PARITY) return (idx << 1) | (uint64_t)(hd_par(idx) ^ a.space);
  return idx;
}

template <int TYPE, int NB>
__global__ void __launch_bounds__(PM_NT)
cyc_moments_kernel(const c128 *__restrict__ x, const CycArgs a, const int64_t *__restrict__ nck,
                   double *__restrict__ partial) {
  constexpr int NACC = NB * (NB + 1) / 2 + NB * NB;
  constexpr int LDP = 16 * NB + 1;
  extern __shared__ __align__(16) unsigned char cyc_lds[];
  c128 *panel = reinterpret_cast<c128 *>(cyc_lds);
  int64_t *tab = reinterpret_cast<int64_t *>(cyc_lds + (((size_t)LDP * 16) << a.B));
  const int tid = threadIdx.x;
  const int rows = 1 << a.B;
  if (TYPE == DNM_SPIN_CONSERVE)
    for (int i = tid; i < (a.K + 1) * a.ld; i += PM_NT) tab[i] = nck[i];
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
      if (TYPE == DNM_SPIN_CONSERVE) {
        const uint64_t cfg = pm_unrank(p, a.L, a.K, tab, a.ld);
        for (int m = 0; m < a.n; ++m) {
          int fl;
          const int64_t idx = cyc_sc_partner(cfg, p, a.a[m], a.b[m], a.c[m], a.L, a.dim, a.xsec, tab, a.ld, &fl);
          c128 v = self;
          if (idx != p) v = x[idx];
          if (fl) v = make_double2(a.sign * v.x, a.sign * v.y);
          prow[1 + m] = v;
        }
      } else {
        const uint64_t cfg = cyc_row_config<TYPE>(p, a);
#pragma unroll 4
        for (int m = 0; m < a.n; ++m) {
          const int sa = a.a[m], sb = a.b[m], sc = a.c[m];
          int pp, qq;
          const int d = cyc_changed(cfg, sa, sb, sc, &pp, &qq);
          c128 v = self;
          if (d) {
            const int fl = cyc_flipped(d, sa, sb, sc, a.L, a.xsec);
            v = x[cyc_xor_partner(p, d, fl, a.site[sa], a.site[sb], a.site[sc], a.mall)];
            if (fl) v = make_double2(a.sign * v.x, a.sign * v.y);
          }
          prow[1 + m] = v;
        }
      }
    }
    __syncthreads();
    pm_tile_multiply<NB>(panel, rows, wave, slot, r, acc);
    __syncthreads();
  }
  pm_tile_reduce_store<NACC>(reinterpret_cast<double *>(cyc_lds), wave, slot, r, acc,
                             partial + (int64_t)blockIdx.x * (NACC * 256));
}

__global__ void __launch_bounds__(PM_NT)
cyc_finalize_kernel(const double *__restrict__ partial, int nwg, int nb, int D, c128 *__restrict__ out) {
  pm_tile_finalize(partial, nwg, nb, D, out);
}

int launch_cyc_moments(const void *x, int type, int L, int space, int swz, int xsec, int ncycles, const int32_t *cycles,
                       const GramPlan &p, const int64_t *nck, void *partial, void *out, hipStream_t st) {
  CycArgs a{};
  a.nrows = p.nrows;
  a.npanels = p.npanels;
  a.per_wg = p.per_wg;
  a.dim = p.dim;
  a.L = L;
  a.B = p.B;
  a.K = p.K;
  a.ld = L + 1;
  a.space = space;
  a.swz = swz;
  a.n = ncycles;
  a.xsec = xsec;
  a.sign = xsec < 0 ? -1.0 : 1.0;
  for (int m = 0; m < ncycles; ++m) {
    a.a[m] = (int8_t)cycles[3 * m];
    a.b[m] = (int8_t)cycles[3 * m + 1];
    a.c[m] = (int8_t)cycles[3 * m + 2];
  }
  if (type != DNM_SPIN_CONSERVE) {
    // the index-space masks, taken through the swizzle
    const bool parity = type == DNM_PARITY;
    for (int s = 0; s < L; ++s) a.site[s] = (uint64_t)vec_pos((int64_t)cyc_site_mask(parity, s), swz);
    a.mall = (uint64_t)vec_pos((int64_t)cyc_all_mask(parity, L), swz);
  }
  const c128 *xp = (const c128 *)x;
  double *pp = (double *)partial;
  DNM_TRY(gram_dispatch<false>(type, p.nb, "chirality moments", "chirality moments: subspace type %d",
                               [&](auto T, auto NB) {
    auto k = cyc_moments_kernel<decltype(T)::value, decltype(NB)::value>;
    DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(PM_NT), p.lds_bytes, st, xp, a, nck, pp);
    DNM_HIP(hipGetLastError());
    return 0;
  }));
  hipLaunchKernelGGL(cyc_finalize_kernel, dim3((unsigned)(p.nb * (p.nb + 1) / 2)), dim3(PM_NT), 0, st,
                     (const double *)pp, p.nwg, p.nb, ncycles + 1, (c128 *)out);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
