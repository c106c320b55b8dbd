// All bond-swap correlators of a state in one pass over it.  sigma_a . sigma_b = 2 P_ab - 1 with P_ab the exchange of
// the spins a and b, so with the operand matrix over the rows r of the subspace
//   A[r, 0] = psi(r),   A[r, 1 + m] = psi(r with bits a_m and b_m exchanged)
// the Gram matrix G = A^H A ((n + 1) x (n + 1) complex128, Hermitian) holds G[0][0] = <psi|psi>, G[0][1 + m] = <P_m> and
// G[1 + m][1 + m'] = <P_m P_m'>: the Hermitian rank-N update of gram_tile.h on v_mfma_f64_16x16x4_f64, NB = ceil((n + 1)
// / 16) <= 4 tile rows.  A swap keeps a row inside Full, Parity and SpinConserve -- the rows are the subspace's own --
// and commutes with the global flip: for a state on an XParity sector s the rows are the representatives (the parent's
// first dim / 2 rows, bit L - 1 clear) and a partner whose bit L - 1 is set is s times the amplitude of its complement;
// the sum over the representatives is then the expectation value in the sector.
//
// Panel fill: a thread owns a row of the panel -- adjacent threads adjacent rows -- and walks the bonds; where the two
// bits of its configuration are equal the partner is the row's own amplitude, loaded once.
// Full / Parity: the vector is read as it lies.  The XOR swizzle is linear, so in position space the partner of position
// p for bond m is p ^ mask[m] with one mask per bond from the host (swap_rank.h: Parity's index does not hold site 0;
// a bond at site L - 1 under XParity has the complement's mask and the sector's sign): a wavefront reads an aligned 1 KB
// run of the vector, permuted inside the run by the low bits of the mask.
// SpinConserve: reference order.  A thread unranks its row (binomials in LDS) and ranks each swapped configuration by
// swap_rank.h's difference form; under XParity a partner with bit L - 1 set is fetched at dim - 1 - rank.
//
// No atomics: wavefronts and workgroups are summed in a fixed order (gram_tile.h).  The number of workgroups follows from
// the number of rows alone: two calls return the same bits on any device.
#include "gram_tile.h"
#include "swap_rank.h"

namespace dnm {

// log2 of the panel's rows: the rule of the sigma+ sigma- sweep (pm_kernels.hip) -- the largest panel at one tile row,
// 2^7 rows from two tile rows on so that two workgroups share a compute unit.  Not measured again for this fill.
constexpr int SWAP_B_MAX = 9, SWAP_B_MAX_WIDE = 7, SWAP_B_MIN = 6;
constexpr int SWAP_ROWS_PER_WG_LOG2 = 9;        // workgroups = ceil(rows / 2^9), at most PM_MAX_WG

static_assert(SWAP_B_MAX <= SWAP_ROWS_PER_WG_LOG2, "a workgroup has at least one panel");

// rows: the subspace's own (the representatives of an XParity sector), with the binomials of sector K = k; `what`: the
// pass, for the messages (gram_tile.h: the rotation pass plans through this too)
int swap_plan(int type, int L, int k, int nbonds, int xsec, GramPlan *p, const char *what) {
  GramPlan q{};
  q.K = type == DNM_SPIN_CONSERVE ? k : 0;
  size_t table_bytes = 0;
  if (type == DNM_SPIN_CONSERVE) {
    std::vector<int64_t> t((size_t)(k + 1) * (size_t)(L + 1));
    pm_binomials(L, k, L + 1, t.data());
    q.dim = t[(size_t)k * (L + 1) + L];
    table_bytes = t.size() * sizeof(int64_t);
  } else {
    if (L - (type == DNM_PARITY) > 62) {
      set_error("%s moments: 2^%d rows", what, L - (type == DNM_PARITY));
      return 1;
    }
    q.dim = (int64_t)1 << (L - (type == DNM_PARITY));
  }
  const int64_t nrows = xsec ? q.dim / 2 : q.dim;
  const int64_t nwg = (nrows + ((int64_t)1 << SWAP_ROWS_PER_WG_LOG2) - 1) >> SWAP_ROWS_PER_WG_LOG2;
  if (!gram_plan(nbonds + 1, nrows, table_bytes, SWAP_B_MAX, SWAP_B_MAX_WIDE, SWAP_B_MIN, 0, nwg, &q)) {
    set_error("internal: %s panel of %zu bytes", what, q.lds_bytes);
    return 1;
  }
  *p = q;
  return 0;
}

int swap_plan(int type, int L, int k, int nbonds, int xsec, GramPlan *p) {
  return swap_plan(type, L, k, nbonds, xsec, p, "bond-swap");
}

struct SwapArgs {
  int64_t nrows, npanels, per_wg, dim;
  int32_t L, B, K, ld, space, swz, n;
  double sign;                // the XParity sector, +-1 (1 without one)
  int32_t xsec;
  uint64_t mask[63];          // Full / Parity: partner of position p for bond m = p ^ mask[m]
  int8_t a[63], b[63], flip[63];      // the bond's sites; flip: the partner is the complement's amplitude times sign
};

// the configuration of the row at position p of the (swizzled) order
template <int TYPE>
__device__ __forceinline__ uint64_t swap_row_config(int64_t p, const SwapArgs &a) {
  const uint64_t idx = (uint64_t)vec_pos(p, a.swz);
  if (TYPE == DNM_PARITY) return (idx << 1) | (uint64_t)(hd_par(idx) ^ a.space);
  return idx;
}

template <int TYPE, int NB>
__global__ void __launch_bounds__(PM_NT)
swap_moments_kernel(const c128 *__restrict__ x, const SwapArgs a, const int64_t *__restrict__ nck,
                    double *__restrict__ partial) {
  constexpr int NACC = NB * (NB + 1) / 2 + NB * NB;
  constexpr int LDP = 16 * NB + 1;
  extern __shared__ __align__(16) unsigned char swap_lds[];
  c128 *panel = reinterpret_cast<c128 *>(swap_lds);
  int64_t *tab = reinterpret_cast<int64_t *>(swap_lds + (((size_t)LDP * 16) << a.B));
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
          const int64_t idx = swap_sc_partner(cfg, p, a.a[m], a.b[m], a.L, a.dim, a.xsec, tab, a.ld, &fl);
          c128 v = self;
          if (idx != p) v = x[idx];
          if (fl) v = make_double2(a.sign * v.x, a.sign * v.y);
          prow[1 + m] = v;
        }
      } else {
        const uint64_t cfg = swap_row_config<TYPE>(p, a);
#pragma unroll 4
        for (int m = 0; m < a.n; ++m) {
          c128 v = self;
          if (((cfg >> a.a[m]) ^ (cfg >> a.b[m])) & 1) {
            v = x[p ^ (int64_t)a.mask[m]];
            if (a.flip[m]) v = make_double2(a.sign * v.x, a.sign * v.y);
          }
          prow[1 + m] = v;
        }
      }
    }
    __syncthreads();
    pm_tile_multiply<NB>(panel, rows, wave, slot, r, acc);
    __syncthreads();
  }
  pm_tile_reduce_store<NACC>(reinterpret_cast<double *>(swap_lds), wave, slot, r, acc,
                             partial + (int64_t)blockIdx.x * (NACC * 256));
}

__global__ void __launch_bounds__(PM_NT)
swap_finalize_kernel(const double *__restrict__ partial, int nwg, int nb, int D, c128 *__restrict__ out) {
  pm_tile_finalize(partial, nwg, nb, D, out);
}

int launch_swap_moments(const void *x, int type, int L, int space, int swz, int xsec, int nbonds, const int32_t *bonds,
                        const GramPlan &p, const int64_t *nck, void *partial, void *out, hipStream_t st) {
  SwapArgs a{};
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
  a.n = nbonds;
  a.xsec = xsec;
  a.sign = xsec < 0 ? -1.0 : 1.0;
  for (int m = 0; m < nbonds; ++m) {
    a.a[m] = (int8_t)bonds[2 * m];
    a.b[m] = (int8_t)bonds[2 * m + 1];
    if (type == DNM_SPIN_CONSERVE) continue;
    // the index-space partner mask of the bond, taken through the swizzle
    int fl;
    a.mask[m] = (uint64_t)vec_pos((int64_t)swap_index_mask(type == DNM_PARITY, L, a.a[m], a.b[m], xsec, &fl), swz);
    a.flip[m] = (int8_t)fl;
  }
  const c128 *xp = (const c128 *)x;
  double *pp = (double *)partial;
  DNM_TRY(gram_dispatch<false>(type, p.nb, "bond-swap moments", "bond-swap moments: subspace type %d",
                               [&](auto T, auto NB) {
    auto k = swap_moments_kernel<decltype(T)::value, decltype(NB)::value>;
    DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(PM_NT), p.lds_bytes, st, xp, a, nck, pp);
    DNM_HIP(hipGetLastError());
    return 0;
  }));
  hipLaunchKernelGGL(swap_finalize_kernel, dim3((unsigned)(p.nb * (p.nb + 1) / 2)), dim3(PM_NT), 0, st,
                     (const double *)pp, p.nwg, p.nb, nbonds + 1, (c128 *)out);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
