// All <sigma+_i sigma-_j> of a state in one pass over it.  sigma_minus(j) = sigmax - i sigmay sets bit j (matrix
// element 2), so with the operand matrix
//   A[r, j] = psi(r ^ e_j) where bit j of the configuration r is set, 0 elsewhere
// the raw result is the Gram matrix
//   P[i][j] = sum_r conj(A[r, i]) A[r, j]        (L x L complex128, Hermitian),   <sigma+_i sigma-_j> = 4 P[i][j]:
// a Hermitian rank-N update on v_mfma_f64_16x16x4_f64 (operand and result layouts: rdm_tile.h).  The rows r are every
// configuration (Full), the configurations of the opposite parity (Parity, enumerated by the same index bits) or those
// with k + 1 set bits (SpinConserve(L, k), in colex order).
//
// A workgroup stages a panel of A in LDS -- 2^B rows x 16 NB sites of complex128, one amplitude of padding per row --
// and its four wavefronts share the panel's k-steps of four rows: per step a lane reads NB amplitudes (ds_read_b128:
// site 16 t + (lane & 15) of row 4 q + (lane >> 4)) and issues 2 NT + NB^2 MFMAs, NT = NB (NB + 1) / 2:
//   Re P = Ar^T Ar + Ai^T Ai   (symmetric: lower-triangle tiles, both products into one accumulator)
//   Q    = Ar^T Ai             (all tiles),   Im P = Q - Q^T
// The NT + NB^2 accumulators stay in registers for the whole sweep.
//
// Panel fill, Full / Parity: the vector is read as it lies.  The XOR swizzle is linear, so in position space the
// partner of position p for site j is p ^ m_j with a mask per site from the host; a column of the panel is one run of
// 2^B positions -- the panel's base ^ the high part of m_j -- loaded whole with coalesced 16-byte loads and permuted
// inside the run by the low part of m_j on its way into LDS.  Rows whose bit j is clear load nothing: for the sites
// above the panel that is the whole column of every other panel.  Parity: the spin the index does not hold (bit 0 of
// the configuration) has m = 0, its partner is the amplitude of the same index.
// SpinConserve: reference order.  A thread unranks its row of sector k + 1 (binomials in LDS) and gathers the partners
// from global memory by pm_rank.h's running sums.
//
// No atomics: the wavefronts are summed through LDS in a fixed order, the workgroups by pm_finalize_kernel in a fixed
// order, which forms Q - Q^T, mirrors the lower triangle as the conjugate and writes real diagonals.  The number of
// workgroups follows from the number of rows alone: two calls return the same bits on any device.
#include "gram_tile.h"
#include "pm_rank.h"

namespace dnm {

// log2 of the panel's rows: the largest that fits, but 2^7 from two tile rows on -- two workgroups then share a compute
// unit and one fills its panel while the other multiplies.  Measured at NB = 2 on MI355X, Full L=30 / SpinConserve(32,
// 16): 2^8 rows 302.9 / 174.7 ms, 2^7 273.9 / 155.1 ms, 2^6 437.9 / 260.3 ms.  One tile row (L <= 16) is not measured
// and keeps the largest panel.
constexpr int PM_B_MAX = 9, PM_B_MAX_WIDE = 7, PM_B_MIN = 6;

// rows: every configuration (the opposite parity), or sector K = k + 1 with its binomials -- none where it is empty; a
// workgroup per panel
int pm_plan(int type, int L, int k, GramPlan *p) {
  GramPlan q{};
  q.K = k + 1;
  int64_t nrows;
  size_t table_bytes = 0;
  if (type == DNM_SPIN_CONSERVE) {
    std::vector<int64_t> t((size_t)(L + 1) * (size_t)(L + 1));
    pm_binomials(L, L, L + 1, t.data());
    nrows = q.K <= L ? t[(size_t)q.K * (L + 1) + L] : 0;
    if (nrows) table_bytes = (size_t)(q.K + 1) * (size_t)(L + 1) * sizeof(int64_t);
  } else {
    if (L - (type == DNM_PARITY) > 62) {
      set_error("sigma+ sigma- moments: 2^%d rows", L - (type == DNM_PARITY));
      return 1;
    }
    nrows = (int64_t)1 << (L - (type == DNM_PARITY));
  }
  const char *e = knob("DNM_PM_B");             // experiments: other panels
  if (!gram_plan(L, nrows, table_bytes, PM_B_MAX, PM_B_MAX_WIDE, PM_B_MIN, e ? atoi(e) : 0, PM_MAX_WG, &q)) {
    set_error("internal: sigma+ sigma- panel of %zu bytes", q.lds_bytes);
    return 1;
  }
  *p = q;
  return 0;
}

struct PmArgs {
  int64_t nrows, npanels, per_wg;
  int32_t L, B, K, ld, space, swz;
  uint64_t mask[64];          // Full / Parity: partner of position p for site j = p ^ mask[j]
};

// the configuration of the row at position p of the (swizzled) order
template <int TYPE>
__device__ __forceinline__ uint64_t pm_row_config(int64_t p, const PmArgs &a) {
  const uint64_t idx = (uint64_t)vec_pos(p, a.swz);
  if (TYPE == DNM_PARITY) return (idx << 1) | (uint64_t)(hd_par(idx) ^ a.space ^ 1);     // the opposite sector
  return idx;
}

// partial: [workgroup][Re tile (ti, tj), tj <= ti, at ti (ti + 1) / 2 + tj; then Q tile (ti, tj) at NT + ti NB + tj]
// [16 x 16 row-major] doubles
template <int TYPE, int NB>
__global__ void __launch_bounds__(PM_NT)
pm_moments_kernel(const c128 *__restrict__ x, const PmArgs a, const int64_t *__restrict__ nck,
                  double *__restrict__ partial) {
  constexpr int NTILE = NB * (NB + 1) / 2, NACC = NTILE + NB * NB;
  constexpr int LDP = 16 * NB + 1;             // amplitudes of a panel row: an odd stride spreads a column's stores
  extern __shared__ __align__(16) unsigned char pm_lds[];
  c128 *panel = reinterpret_cast<c128 *>(pm_lds);
  int64_t *tab = reinterpret_cast<int64_t *>(pm_lds + (((size_t)LDP * 16) << a.B));
  const int tid = threadIdx.x;
  const int rows = 1 << a.B;
  if (TYPE == DNM_SPIN_CONSERVE)
    for (int i = tid; i < (a.K + 1) * a.ld; i += PM_NT) tab[i] = nck[i];
  // (the padding columns and the sites at or above L stay zero for the whole sweep)
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
    if (TYPE == DNM_SPIN_CONSERVE) {
      for (int t = tid; t < rows; t += PM_NT) {
        c128 *prow = panel + t * LDP;
        for (int j = 0; j < a.L; ++j) prow[j] = make_double2(0.0, 0.0);
        if (base + t < a.nrows) {
          const uint64_t cfg = pm_unrank(base + t, a.L, a.K, tab, a.ld);
          pm_partners(cfg, tab, a.ld, [&](int j, int64_t idx) { prow[j] = x[idx]; });
        }
      }
    } else {
      for (int j = 0; j < a.L; ++j) {
        const uint64_t m = a.mask[j];
        const int ml = (int)(m & (uint64_t)(rows - 1));
        const int64_t src0 = base ^ (int64_t)(m - (uint64_t)ml);
        for (int t = tid; t < rows; t += PM_NT) {
          const int row = t ^ ml;
          c128 v = make_double2(0.0, 0.0);
          if (src0 + t < a.nrows && ((pm_row_config<TYPE>(base + row, a) >> j) & 1)) v = x[src0 + t];
          panel[row * LDP + j] = v;
        }
      }
    }
    __syncthreads();
    pm_tile_multiply<NB>(panel, rows, wave, slot, r, acc);
    __syncthreads();
  }

  pm_tile_reduce_store<NACC>(reinterpret_cast<double *>(pm_lds), wave, slot, r, acc,
                             partial + (int64_t)blockIdx.x * (NACC * 256));
}

__global__ void __launch_bounds__(PM_NT)
pm_finalize_kernel(const double *__restrict__ partial, int nwg, int nb, int L, c128 *__restrict__ out) {
  pm_tile_finalize(partial, nwg, nb, L, out);
}

int launch_pm_moments(const void *x, int type, int L, int k, int space, int swz, const GramPlan &p, const int64_t *nck,
                      void *partial, void *out, hipStream_t st) {
  PmArgs a{};
  a.nrows = p.nrows;
  a.npanels = p.npanels;
  a.per_wg = p.per_wg;
  a.L = L;
  a.B = p.B;
  a.K = p.K;
  a.ld = L + 1;
  a.space = space;
  a.swz = swz;
  for (int j = 0; j < L; ++j) {
    // index-space partner mask of site j (Parity: index bit j - 1, none for site 0), taken through the swizzle
    const int bit = type == DNM_PARITY ? j - 1 : j;
    a.mask[j] = type == DNM_SPIN_CONSERVE || bit < 0 ? 0 : (uint64_t)vec_pos((int64_t)1 << bit, swz);
  }
  const c128 *xp = (const c128 *)x;
  double *pp = (double *)partial;
  DNM_TRY(gram_dispatch<false>(type, p.nb, "sigma+ sigma- moments", "sigma+ sigma- moments: subspace type %d",
                               [&](auto T, auto NB) {
    auto k = pm_moments_kernel<decltype(T)::value, decltype(NB)::value>;
    DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(PM_NT), p.lds_bytes, st, xp, a, nck, pp);
    DNM_HIP(hipGetLastError());
    return 0;
  }));
  hipLaunchKernelGGL(pm_finalize_kernel, dim3((unsigned)(p.nb * (p.nb + 1) / 2)), dim3(PM_NT), 0, st,
                     (const double *)pp, p.nwg, p.nb, L, (c128 *)out);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
