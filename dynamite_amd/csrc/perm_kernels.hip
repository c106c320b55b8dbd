// Site permutations of a state: lattice translations, rotations and mirrors, in one pass over it.  A site permutation
// is an int array pi of length L, a bijection of [0, L); P_pi moves the spin at site i to site pi(i), P_pi |c> = |c'>
// with c'_{pi(i)} = c_i, so (P_pi x)(c') = x(c) where the source configuration c has bit i equal to bit pi(i) of c'
// (perm_rank.h).  For n <= 64 permutations P_g and the rows r of the vector, with p_g(r) the index of the source of row
// r and s_g(r) its factor (1, or the sector's sign where the source is the complement's amplitude under XParity):
//   perm_apply   y[r] = (accumulate ? y[r] : 0) + sum_g c_g s_g(r) x[p_g(r)]      the plain permutation at n = 1, c = 1;
//                                                                                  a projector onto an irrep otherwise
//   perm_dots    out[g] = sum_r conj(phi[r]) s_g(r) psi[p_g(r)] = <phi|P_g|psi>
// Both are gathers: x and y must not alias.  A permutation keeps a row inside Full, Parity and SpinConserve and commutes
// with the global flip: for a state on an XParity sector the rows are the representatives (bit L - 1 clear), sums run
// over them alone, and P_g x lies in the same sector, so that its representatives define it.
//
// Rows.  Full / Parity: the vector is read as it lies; a thread takes the row at its position (adjacent lanes adjacent
// 16-byte amplitudes: loads of phi and stores of y are 1 KB per wave instruction), whose index is vec_pos of the
// position and whose configuration follows from the index.  SpinConserve: reference order; a thread owns a run of
// PERM_RUN adjacent rows, unranks the first (L steps on the binomials) and steps to the next configuration by Gosper's
// rule -- a lane then covers 64 contiguous bytes of y and a wave instruction a quarter of each of 64 such segments,
// which the four stores of a run complete; the gathers of x, whose sectors are scattered anyway, carry the traffic.
// Source index: perm_rank.h -- popcount steps through the inverse permutation (LDS, one byte per site, PERM_LD bytes
// apart so that lanes on different permutations read different banks) and, for SpinConserve, as many through the
// binomial rows (LDS; lanes read one row at lane-dependent columns of 8 bytes: columns 32 apart share a bank, two ways at
// the worst).
//
// perm_dots: the lanes of a wave are (run, permutation) pairs -- GP = the power of two >= n permutations side by side,
// 64 / GP runs of rows per wave -- so that a lane holds one complex sum however many permutations there are and phi[r]
// is loaded once per row (one address per group of GP lanes).  No atomics: the lanes of one permutation are summed by
// XOR shuffles in a fixed order, the four waves through LDS in their order, the workgroups by vk_reduce_partials.  The
// number of workgroups follows from the number of rows alone: two calls return the same bits.
#include <type_traits>

#include "perm.h"

namespace dnm {

typedef double2 c128;

int perm_plan(int type, int L, int k, int nperm, int xsec, PermPlan *p) {
  PermPlan q{};
  if (type == DNM_SPIN_CONSERVE) {
    q.K = k;
    q.ntab = (k + 1) * (L + 1);
    std::vector<int64_t> t((size_t)q.ntab);
    pm_binomials(L, k, L + 1, t.data());
    q.dim = t[(size_t)k * (L + 1) + L];
  } else {
    const int bits = L - (type == DNM_PARITY);
    if (bits > 62) {
      set_error("site permutations: 2^%d rows", bits);
      return 1;
    }
    q.dim = (int64_t)1 << bits;
  }
  q.nrows = xsec ? q.dim / 2 : q.dim;
  int64_t nwg = (q.nrows + ((int64_t)1 << PERM_ROWS_PER_WG_LOG2) - 1) >> PERM_ROWS_PER_WG_LOG2;
  if (nwg > PERM_MAX_WG) nwg = PERM_MAX_WG;
  if (nwg < 1) nwg = 1;
  q.nwg = (int)nwg;
  q.lds_bytes = ((size_t)q.ntab * 8 + (size_t)nperm * PERM_LD + 15) & ~(size_t)15;
  q.partial_bytes = (size_t)nwg * 2 * (size_t)nperm * sizeof(double);
  *p = q;
  return 0;
}

struct PermArgs {
  int64_t nrows, dim;
  int32_t L, K, ld, ntab, space, swz, xsec, n, accumulate, gp_log2;
  double sign;                 // the XParity sector, +-1 (1 without one)
  double coef[2 * PERM_MAX];   // perm_apply: (re, im) per permutation
};

// the tables of the launch into LDS: whole dwords (the binomials are 8 bytes each, PERM_LD is a multiple of 4)
__device__ __forceinline__ void perm_stage(unsigned char *lds, const unsigned char *__restrict__ tables,
                                           const PermArgs &a) {
  const int nwords = (a.ntab * 8 + a.n * PERM_LD) / 4;
  for (int i = threadIdx.x; i < nwords; i += PERM_NT)
    reinterpret_cast<uint32_t *>(lds)[i] = reinterpret_cast<const uint32_t *>(tables)[i];
  __syncthreads();
}

// s_g(r) x[p_g(r)] for the row of configuration cfg
template <int TYPE>
__device__ __forceinline__ c128 perm_gather(const c128 *__restrict__ x, uint64_t cfg, const uint8_t *inv,
                                            const int64_t *tab, const PermArgs &a) {
  const uint64_t src = perm_source(cfg, inv);
  int fl;
  int64_t at;
  if (TYPE == DNM_SPIN_CONSERVE) at = perm_sc_index(src, a.L, a.dim, a.xsec, tab, a.ld, &fl);
  else at = vec_pos(perm_xor_index(src, TYPE == DNM_PARITY, a.L, a.xsec, &fl), a.swz);
  c128 v = x[at];
  if (fl) v = make_double2(a.sign * v.x, a.sign * v.y);
  return v;
}

// the configuration of the row at position p: unranked for SpinConserve, from the index otherwise
template <int TYPE>
__device__ __forceinline__ uint64_t perm_row_config(int64_t p, const int64_t *tab, const PermArgs &a) {
  if (TYPE == DNM_SPIN_CONSERVE) return pm_unrank(p, a.L, a.K, tab, a.ld);
  return perm_index_config(TYPE == DNM_PARITY, a.space, (uint64_t)vec_pos(p, a.swz));
}

template <int TYPE>
__global__ void __launch_bounds__(PERM_NT)
perm_apply_kernel(const c128 *__restrict__ x, c128 *__restrict__ y, const PermArgs a,
                  const unsigned char *__restrict__ tables) {
  constexpr int RUN = TYPE == DNM_SPIN_CONSERVE ? PERM_RUN : 1;
  extern __shared__ __align__(16) unsigned char perm_lds[];
  perm_stage(perm_lds, tables, a);
  const int64_t *tab = reinterpret_cast<const int64_t *>(perm_lds);
  const uint8_t *inv = perm_lds + (size_t)a.ntab * 8;
  const int64_t nruns = (a.nrows + RUN - 1) / RUN;
  for (int64_t q = (int64_t)blockIdx.x * PERM_NT + threadIdx.x; q < nruns; q += (int64_t)gridDim.x * PERM_NT) {
    int64_t row = q * RUN;
    uint64_t cfg = perm_row_config<TYPE>(row, tab, a);
    for (int j = 0; j < RUN && row < a.nrows; ++j, ++row) {
      c128 acc = a.accumulate ? y[row] : make_double2(0.0, 0.0);
      for (int g = 0; g < a.n; ++g) {
        const c128 v = perm_gather<TYPE>(x, cfg, inv + g * PERM_LD, tab, a);
        const double cr = a.coef[2 * g], ci = a.coef[2 * g + 1];
        acc.x += cr * v.x - ci * v.y;
        acc.y += cr * v.y + ci * v.x;
      }
      y[row] = acc;
      if (RUN > 1 && j + 1 < RUN && row + 1 < a.nrows) cfg = perm_next_config(cfg);
    }
  }
}

template <int TYPE>
__global__ void __launch_bounds__(PERM_NT)
perm_dots_kernel(const c128 *__restrict__ phi, const c128 *__restrict__ psi, const PermArgs a,
                 const unsigned char *__restrict__ tables, double *__restrict__ partial) {
  constexpr int RUN = TYPE == DNM_SPIN_CONSERVE ? PERM_RUN : 1;
  extern __shared__ __align__(16) unsigned char perm_lds[];
  __shared__ double red[PERM_NT / 64][2 * PERM_MAX];
  perm_stage(perm_lds, tables, a);
  const int64_t *tab = reinterpret_cast<const int64_t *>(perm_lds);
  const int tid = threadIdx.x;
  const int gp = 1 << a.gp_log2, g = tid & (gp - 1);
  const bool active = g < a.n;
  const uint8_t *inv = perm_lds + (size_t)a.ntab * 8 + (active ? g : 0) * PERM_LD;
  const int64_t nruns = (a.nrows + RUN - 1) / RUN;
  const int64_t nslots = ((int64_t)gridDim.x * PERM_NT) >> a.gp_log2;
  double sr = 0.0, si = 0.0;
  for (int64_t q = ((int64_t)blockIdx.x * PERM_NT + tid) >> a.gp_log2; q < nruns; q += nslots) {
    int64_t row = q * RUN;
    uint64_t cfg = perm_row_config<TYPE>(row, tab, a);
    for (int j = 0; j < RUN && row < a.nrows; ++j, ++row) {
      if (active) {
        const c128 f = phi[row];
        const c128 v = perm_gather<TYPE>(psi, cfg, inv, tab, a);
        sr += f.x * v.x + f.y * v.y;
        si += f.x * v.y - f.y * v.x;
      }
      if (RUN > 1 && j + 1 < RUN && row + 1 < a.nrows) cfg = perm_next_config(cfg);
    }
  }
  // the lanes of one permutation: gp apart
  for (int off = gp; off < 64; off <<= 1) {
    sr += __shfl_xor(sr, off, 64);
    si += __shfl_xor(si, off, 64);
  }
  const int lane = tid & 63, wave = tid >> 6;
  if (lane < gp) {
    red[wave][2 * lane] = sr;
    red[wave][2 * lane + 1] = si;
  }
  __syncthreads();
  if (tid < a.n) {
    double tr = 0.0, ti = 0.0;
    for (int wv = 0; wv < PERM_NT / 64; ++wv) {
      tr += red[wv][2 * tid];
      ti += red[wv][2 * tid + 1];
    }
    partial[((int64_t)blockIdx.x * a.n + tid) * 2] = tr;
    partial[((int64_t)blockIdx.x * a.n + tid) * 2 + 1] = ti;
  }
}

static PermArgs perm_args(int type, int L, int space, int swz, int xsec, int nperm, const PermPlan &p) {
  PermArgs a{};
  a.nrows = p.nrows;
  a.dim = p.dim;
  a.L = L;
  a.K = p.K;
  a.ld = L + 1;
  a.ntab = p.ntab;
  a.space = space;
  a.swz = type == DNM_SPIN_CONSERVE ? 0 : swz;
  a.xsec = xsec;
  a.n = nperm;
  a.sign = xsec < 0 ? -1.0 : 1.0;
  while ((1 << a.gp_log2) < nperm) ++a.gp_log2;
  return a;
}

template <class F>
static int perm_dispatch(int type, F f) {
  switch (type) {
    case DNM_FULL: return f(std::integral_constant<int, DNM_FULL>{});
    case DNM_PARITY: return f(std::integral_constant<int, DNM_PARITY>{});
    case DNM_SPIN_CONSERVE: return f(std::integral_constant<int, DNM_SPIN_CONSERVE>{});
  }
  set_error("site permutations: subspace type %d", type);
  return 1;
}

int launch_perm_apply(const void *x, void *y, int type, int L, int space, int swz, int xsec, int nperm,
                      const double *coef, int accumulate, const PermPlan &p, const void *tables, hipStream_t st) {
  PermArgs a = perm_args(type, L, space, swz, xsec, nperm, p);
  a.accumulate = accumulate;
  for (int i = 0; i < 2 * nperm; ++i) a.coef[i] = coef[i];
  return perm_dispatch(type, [&](auto T) {
    hipLaunchKernelGGL(perm_apply_kernel<decltype(T)::value>, dim3((unsigned)p.nwg), dim3(PERM_NT), p.lds_bytes, st,
                       (const c128 *)x, (c128 *)y, a, (const unsigned char *)tables);
    DNM_HIP(hipGetLastError());
    return 0;
  });
}

int launch_perm_dots(const void *phi, const void *psi, int type, int L, int space, int swz, int xsec, int nperm,
                     const PermPlan &p, const void *tables, void *partial, void *out, hipStream_t st) {
  const PermArgs a = perm_args(type, L, space, swz, xsec, nperm, p);
  DNM_TRY(perm_dispatch(type, [&](auto T) {
    hipLaunchKernelGGL(perm_dots_kernel<decltype(T)::value>, dim3((unsigned)p.nwg), dim3(PERM_NT), p.lds_bytes, st,
                       (const c128 *)phi, (const c128 *)psi, a, (const unsigned char *)tables, (double *)partial);
    DNM_HIP(hipGetLastError());
    return 0;
  }));
  return vk_reduce_partials((const double *)partial, p.nwg, 2 * nperm, (double *)out, st);
}

}  // namespace dnm
