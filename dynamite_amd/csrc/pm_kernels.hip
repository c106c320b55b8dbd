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
#include "rdm_tile.h"
#include "pm_rank.h"

namespace dnm {

constexpr int PM_NT = 256;                      // threads of a workgroup: four wavefronts, one per SIMD
constexpr int64_t PM_MAX_WG = 1024;
constexpr size_t PM_LDS_BUDGET = 152 * 1024;    // of the 160 KB of a CU
// log2 of the panel's rows: the largest that fits, but 2^7 from two tile rows on -- two workgroups then share a compute
// unit and one fills its panel while the other multiplies.  Measured at NB = 2 on MI355X, Full L=30 / SpinConserve(32,
// 16): 2^8 rows 302.9 / 174.7 ms, 2^7 273.9 / 155.1 ms, 2^6 437.9 / 260.3 ms.  One tile row (L <= 16) is not measured
// and keeps the largest panel.
constexpr int PM_B_MAX = 9, PM_B_MAX_WIDE = 7, PM_B_MIN = 6;

static inline int pm_nacc(int nb) { return nb * (nb + 1) / 2 + nb * nb; }

int pm_plan(int type, int L, int k, PmPlan *p) {
  PmPlan q{};
  q.nb = (L + 15) / 16;
  q.K = k + 1;
  if (type == DNM_SPIN_CONSERVE) {
    std::vector<int64_t> t((size_t)(L + 1) * (size_t)(L + 1));
    pm_binomials(L, L, L + 1, t.data());
    q.nrows = q.K <= L ? t[(size_t)q.K * (L + 1) + L] : 0;
    q.table_bytes = q.nrows ? (size_t)(q.K + 1) * (size_t)(L + 1) * sizeof(int64_t) : 0;
  } else {
    if (L - (type == DNM_PARITY) > 62) {
      set_error("sigma+ sigma- moments: 2^%d rows", L - (type == DNM_PARITY));
      return 1;
    }
    q.nrows = (int64_t)1 << (L - (type == DNM_PARITY));
  }
  const size_t row_bytes = (size_t)(16 * q.nb + 1) * 16;
  q.B = q.nb == 1 ? PM_B_MAX : PM_B_MAX_WIDE;
  if (const char *e = knob("DNM_PM_B")) {       // experiments: other panels
    const int b = atoi(e);
    if (b >= PM_B_MIN && b <= PM_B_MAX) q.B = b;
  }
  while (q.B > PM_B_MIN && (row_bytes << q.B) + q.table_bytes > PM_LDS_BUDGET) --q.B;
  q.lds_bytes = (row_bytes << q.B) + q.table_bytes;
  // (the reduction buffer of the wavefronts' sum takes the panel's place after the sweep)
  if (q.lds_bytes > PM_LDS_BUDGET || (size_t)pm_nacc(q.nb) * 256 * sizeof(double) > (row_bytes << q.B)) {
    set_error("internal: sigma+ sigma- panel of %zu bytes", q.lds_bytes);
    return 1;
  }
  q.npanels = (q.nrows + ((int64_t)1 << q.B) - 1) >> q.B;
  int64_t nwg = q.npanels < PM_MAX_WG ? q.npanels : PM_MAX_WG;
  if (nwg < 1) nwg = 1;
  q.nwg = (int)nwg;
  q.per_wg = (q.npanels + nwg - 1) / nwg;
  q.partial_bytes = (size_t)nwg * (size_t)pm_nacc(q.nb) * 256 * sizeof(double);
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
    __syncthreads();
  }

  // the four wavefronts, summed in the order ((0 + 1) + 2) + 3 through the panel's LDS; C/D layout: col = lane & 15,
  // row = (lane >> 4) + 4 * reg
  double *red = reinterpret_cast<double *>(pm_lds);
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
    double *out = partial + (int64_t)blockIdx.x * (NACC * 256);
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) out[i * 256 + (slot + 4 * gq) * 16 + r] = acc[i][gq];
  }
}

// P (L x L complex128, row-major) from the workgroups' partial tiles, summed in their order: entry (a, b), b <= a, is
// (Re[a][b], Q[a][b] - Q[b][a]); the upper triangle is its conjugate and the diagonal real.  One workgroup per
// lower-triangle tile.
__global__ void __launch_bounds__(PM_NT)
pm_finalize_kernel(const double *__restrict__ partial, int nwg, int nb, int L, c128 *__restrict__ out) {
  int ti, tj;
  rdm_tile_coords(blockIdx.x, &ti, &tj);
  const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
  const int a = ti * 16 + row, b = tj * 16 + col;
  if (a >= L || b >= L || b > a) return;
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
  out[a * L + b] = make_double2(re, im);
  if (a != b) out[b * L + a] = make_double2(re, -im);
}

template <int TYPE>
static int pm_launch_nb(const PmPlan &p, const c128 *x, const PmArgs &a, const int64_t *nck, double *partial,
                        hipStream_t st) {
  void (*k)(const c128 *, const PmArgs, const int64_t *, double *) = nullptr;
  switch (p.nb) {
    case 1: k = pm_moments_kernel<TYPE, 1>; break;
    case 2: k = pm_moments_kernel<TYPE, 2>; break;
    case 3: k = pm_moments_kernel<TYPE, 3>; break;
    case 4: k = pm_moments_kernel<TYPE, 4>; break;
    default: set_error("internal: %d tile rows of sigma+ sigma- moments", p.nb); return 1;
  }
  DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(PM_NT), p.lds_bytes, st, x, a, nck, partial);
  DNM_HIP(hipGetLastError());
  return 0;
}

int launch_pm_moments(const void *x, int type, int L, int k, int space, int swz, const PmPlan &p, const int64_t *nck,
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
  switch (type) {
    case DNM_FULL: DNM_TRY(pm_launch_nb<DNM_FULL>(p, xp, a, nck, pp, st)); break;
    case DNM_PARITY: DNM_TRY(pm_launch_nb<DNM_PARITY>(p, xp, a, nck, pp, st)); break;
    case DNM_SPIN_CONSERVE: DNM_TRY(pm_launch_nb<DNM_SPIN_CONSERVE>(p, xp, a, nck, pp, st)); break;
    default: set_error("sigma+ sigma- moments: subspace type %d", type); return 1;
  }
  hipLaunchKernelGGL(pm_finalize_kernel, dim3((unsigned)(p.nb * (p.nb + 1) / 2)), dim3(PM_NT), 0, st,
                     (const double *)pp, p.nwg, p.nb, L, (c128 *)out);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
