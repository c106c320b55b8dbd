// All first and second sigma-z moments of a state in one pass over it:
//   M = sum_c |psi_c|^2 s~(c) s~(c)^T,   s~(c) = (1, s_0(c), ..., s_{L-1}(c)),   s_i(c) = +1 / -1 for bit i of c clear / set
// so that M[0,0] = <psi|psi>, M[0,1+i] = <sigmaz_i> and M[1+i,1+j] = <sigmaz_i sigmaz_j> (D = L + 1 <= 64 rows).
// sigma-z strings are diagonal in the product basis: no partner amplitude, no operator, no second vector -- a real
// symmetric rank-N update of a D x D matrix whose operand rows are signs, on v_mfma_f64_16x16x4_f64 (operand and
// result layouts: rdm_tile.h).  A wavefront takes 64 amplitudes per step, one per lane (weight w = re^2 + im^2 and the
// configuration shifted up by one bit, so that bit d of it is entry d of s~ and bit 0 the constant +1), and hands them
// round by cross-lane reads: in k-step q the lane (r = lane & 15, slot = lane >> 4) uses amplitude 4 q + slot, its A
// fragment of tile row t is +-w by bit 16 t + r, its B fragment the same sign as +-1.0.  One operand of every product
// is +-1: products are exact, only the accumulation rounds.  The lower-triangle tiles stay in registers for the whole
// sweep; the four wavefronts of a workgroup are summed in a fixed order through LDS, the workgroups by a second kernel
// in a fixed order (no atomics: two calls agree to the last bit).  The number of workgroups depends on the number of
// rows alone, never on the device.  The wave sum and the choice of the kernel instance are gram_tile.h's.
#include "gram_tile.h"

namespace dnm {

constexpr int ZZ_NT = PM_NT;              // threads of a workgroup: four wavefronts
constexpr int64_t ZZ_MIN_PER_WG = 2048;   // positions a workgroup sweeps at least (8 steps per wavefront)
constexpr int64_t ZZ_MAX_WG = 1024;       // one resident wavefront per SIMD and workgroup: 4 per SIMD on 256 CUs

typedef double zz_d2v __attribute__((ext_vector_type(2)));

void zz_plan(int L, int64_t nrows, int *tile_rows, int *nworkgroups, int64_t *per_wg, size_t *scratch_bytes) {
  const int nb = (L + 1 + 15) / 16;
  int64_t nwg = (nrows + ZZ_MIN_PER_WG - 1) / ZZ_MIN_PER_WG;
  if (nwg > ZZ_MAX_WG) nwg = ZZ_MAX_WG;
  if (nwg < 1) nwg = 1;
  // (a share is a whole number of workgroup steps; the last workgroups of a ragged split may find nothing to do and
  // write zeros -- the count stays a monotone function of nrows)
  int64_t per = (nrows + nwg - 1) / nwg;
  per = (per + ZZ_NT - 1) / ZZ_NT * ZZ_NT;
  *tile_rows = nb;
  *nworkgroups = (int)nwg;
  *per_wg = per;
  *scratch_bytes = (size_t)nwg * (size_t)(nb * (nb + 1) / 2) * 256 * sizeof(double);
}

// The configuration of basis index idx.  SpinConserve: Sub<DNM_SPIN_CONSERVE>::i2s step for step, with the binomials
// read from the workgroup's LDS copy of the table: L dependent look-ups per amplitude (SpinConserve(32, 16) on MI355X:
// the sweep takes 39.3 ms this way and 51.2 ms with the table read from global memory).
template <int TYPE>
__device__ __forceinline__ int64_t zz_config(int64_t idx, const SubView &sub, const int64_t *) {
  return Sub<TYPE>::i2s(idx, sub);
}
template <>
__device__ __forceinline__ int64_t zz_config<DNM_SPIN_CONSERVE>(int64_t idx, const SubView &sub, const int64_t *nck) {
  int64_t st = 0;
  int k = sub.k;
  for (int n = sub.L; n > 0; --n) {
    const int64_t here = (k > n - 1) ? 0 : nck[k * sub.ld + (n - 1)];
    st <<= 1;
    if (idx >= here) {
      idx -= here;
      --k;
      st |= 1;
    }
  }
  return st;
}
// bytes of that copy (dynamic LDS of a launch): at most 64 x 64 binomials
static size_t zz_table_bytes(const SubView &sub) {
  return sub.type == DNM_SPIN_CONSERVE ? (size_t)(sub.k + 1) * (size_t)sub.ld * sizeof(int64_t) : 0;
}

// partial: [workgroup][tile (ti, tj), tj <= ti, at ti (ti + 1) / 2 + tj][16 x 16 row-major] doubles
template <int TYPE, int NB>
__global__ void __launch_bounds__(ZZ_NT)
zz_moments_kernel(const c128 *__restrict__ x, const SubView sub, int64_t row0, int64_t nrows, int64_t per_wg,
                  double *__restrict__ partial) {
  constexpr int NTILE = NB * (NB + 1) / 2;
  __shared__ double red[NTILE * 256];
  extern __shared__ int64_t zz_nck[];       // SpinConserve: (k + 1) x (L + 1) binomials
  const int tid = threadIdx.x;
  if (TYPE == DNM_SPIN_CONSERVE) {
    for (int i = tid; i < (sub.k + 1) * sub.ld; i += ZZ_NT) zz_nck[i] = sub.nchoosek[i];
    __syncthreads();
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, slot = lane >> 4;
  mfma_acc acc[NTILE];
#pragma unroll
  for (int i = 0; i < NTILE; ++i) acc[i] = mfma_acc{0.0, 0.0, 0.0, 0.0};

  const int64_t begin = (int64_t)blockIdx.x * per_wg;
  int64_t end = begin + per_wg;
  if (end > nrows) end = nrows;

  // positions at or beyond the end weigh nothing and are not read
  auto fetch = [&](int64_t p, double &w, uint64_t &cfg) {
    w = 0.0;
    cfg = 0;
    if (p < end) {
      const zz_d2v a = __builtin_nontemporal_load(reinterpret_cast<const zz_d2v *>(x + p));
      w = __dadd_rn(__dmul_rn(a.x, a.x), __dmul_rn(a.y, a.y));
      cfg = (uint64_t)zz_config<TYPE>(row0 + vec_pos(p, sub.swz), sub, zz_nck) << 1;
    }
  };

  // (p0 is the same in every lane of a wavefront: the cross-lane reads below see all 64 lanes)
  int64_t p0 = begin + wave * 64;
  double w, wn = 0.0;
  uint64_t cfg, cfgn = 0;
  if (p0 < end) fetch(p0 + lane, wn, cfgn);
  for (; p0 < end; p0 += ZZ_NT) {
    w = wn;
    cfg = cfgn;
    if (p0 + ZZ_NT < end) fetch(p0 + ZZ_NT + lane, wn, cfgn);      // in flight under the MFMAs below
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int src = 4 * q + slot;
      const double wq = __shfl(w, src, 64);
      const uint64_t cq = (uint64_t)__shfl((unsigned long long)cfg, src, 64) >> r;
      double a[NB], b[NB];
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        const bool set = (cq >> (16 * t)) & 1;
        a[t] = set ? -wq : wq;
        b[t] = set ? -1.0 : 1.0;
      }
#pragma unroll
      for (int ti = 0; ti < NB; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) {
          const int i = ti * (ti + 1) / 2 + tj;
          acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[i], 0, 0, 0);
        }
    }
  }

  pm_tile_reduce_store<NTILE>(red, wave, slot, r, acc, partial + (int64_t)blockIdx.x * (NTILE * 256));
}

// M (D x D doubles, row-major) = the workgroups' partial tiles summed in their order; the lower triangle is mirrored
// into the upper one and every diagonal entry is M[0,0] (sigmaz^2 = 1 identically).  One workgroup per tile.
__global__ void __launch_bounds__(ZZ_NT)
zz_finalize_kernel(const double *__restrict__ partial, int nwg, int ntiles, int D, double *__restrict__ out) {
  int ti, tj;
  rdm_tile_coords(blockIdx.x, &ti, &tj);
  const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
  const int a = ti * 16 + row, b = tj * 16 + col;
  if (a >= D || b >= D || b > a) return;
  const int tile = a == b ? 0 : (int)blockIdx.x, e = a == b ? 0 : (int)threadIdx.x;
  double s = 0.0;
  for (int g = 0; g < nwg; ++g) s += partial[((int64_t)g * ntiles + tile) * 256 + e];
  out[a * D + b] = s;
  out[b * D + a] = s;
}

int launch_zz_moments(const void *x, const SubView &sub, int64_t row0, int64_t nrows, void *partial, double *out,
                      hipStream_t st) {
  int nb, nwg;
  int64_t per_wg;
  size_t bytes;
  zz_plan(sub.L, nrows, &nb, &nwg, &per_wg, &bytes);
  const c128 *xp = (const c128 *)x;
  double *pp = (double *)partial;
  DNM_TRY(gram_dispatch<true>(sub.type, nb, "sigma-z moments", "bad subspace type", [&](auto T, auto NB) {
    hipLaunchKernelGGL((zz_moments_kernel<decltype(T)::value, decltype(NB)::value>), dim3((unsigned)nwg), dim3(ZZ_NT),
                       zz_table_bytes(sub), st, xp, sub, row0, nrows, per_wg, pp);
    return 0;
  }));
  const int ntiles = nb * (nb + 1) / 2;
  hipLaunchKernelGGL(zz_finalize_kernel, dim3((unsigned)ntiles), dim3(ZZ_NT), 0, st, (const double *)pp, nwg, ntiles,
                     sub.L + 1, out);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
