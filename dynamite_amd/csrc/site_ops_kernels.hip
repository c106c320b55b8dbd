// Products of single-site operators on a Full-space state and the exponential of a diagonal operator: the two kernels.
// Definitions, the classes of the sites and the plan of a pass: site_ops.h.
//
// site_ops_kernel.  A workgroup takes tiles of 2^tbe amplitudes (stride gridDim.x): the 4 low index bits -- a 256-byte
// run of the vector, which the XOR swizzle leaves whole -- times tbe - 4 free index bits.  It loads the tile (16 lanes per
// run, every thread 16 loads in flight), multiplies by the factor of the diagonal sites outside the tile (one per tile:
// uniform arithmetic), stores it to LDS and then runs the stages of the pass: in a stage a thread holds the 16 amplitudes
// that differ in 4 tile-local bits [g, g + 4) in registers, applies the butterflies of those bits and puts them back where
// it took them -- no other thread touches them in that stage, so one barrier per stage suffices and 12 butterfly levels
// cost three LDS round trips, not twelve.  The tile is written to y from LDS in the order it was loaded.  x == y is safe:
// a tile is in LDS whole before its first store, and tiles are disjoint.
// LDS image: amplitude t of the tile at slot t ^ ((t >> 4) & 15) ^ ((t >> 8) & 15), 16 bytes each.  ds_read_b128 is
// served in groups of 16 lanes that must hit 16 different 16-byte slots mod 16, ds_write_b128 in groups of 8: in the load
// and store phases lanes hold consecutive t; in a stage with g >= 4 the low lane bits are the low bits of t; in a stage
// with g < 4 they are tile-local bits of the fields that the XOR folds onto the low four.  No conflicts in either.
// No atomics; the grid follows from L and the plan alone; every index is 64-bit.
#include "site_ops.h"

namespace dnm {

typedef double2 c128;

__device__ __forceinline__ int site_slot(int t) { return t ^ ((t >> 4) & 15) ^ ((t >> 8) & 15); }

// Products and sums are rounded one by one (no fused multiply-add): M[1][0] x0 + M[1][1] x1 with M[1][1] = -M[1][0] and
// x0 = x1 is then exactly zero, which the sampler of a rotated state relies on (a row of weight zero is never drawn).
__device__ __forceinline__ c128 site_cmul(double mr, double mi, c128 v) {
#pragma clang fp contract(off)
  return make_double2(mr * v.x - mi * v.y, mr * v.y + mi * v.x);
}

// index offset of the tile-local number t: bits 0..3 stay, bit 4 + i goes to index bit pos[i]
__device__ __forceinline__ int64_t site_spread(int t, const SiteOpsPass &a) {
  int64_t o = t & 15;
  for (int i = 0; i < a.nfree; ++i) o |= (int64_t)((t >> (4 + i)) & 1) << a.pos[i];
  return o;
}

template <int NT>
__global__ void __launch_bounds__(NT) site_ops_kernel(const c128 *x, c128 *y, const SiteOpsPass a) {
#pragma clang fp contract(off)
  constexpr int PER = 1 << SITE_OPS_RADIX;      // amplitudes of a thread: in a stage, and in the load and store phases
  extern __shared__ __align__(16) unsigned char site_lds[];
  c128 *tile = reinterpret_cast<c128 *>(site_lds);
  const int tid = threadIdx.x;
  const int nelem = 1 << a.tbe;
  const int R = a.tbe < SITE_OPS_RADIX ? a.tbe : SITE_OPS_RADIX;
  const int ngroups = nelem >> R;
  const int64_t off_tid = site_spread(tid, a);
  for (int64_t u = blockIdx.x; u < a.ntiles; u += gridDim.x) {
    // the tile's first index: zeros inserted into its number at the tile's bits
    uint64_t base = (uint64_t)u << 4;
    for (int i = 0; i < a.nfree; ++i) {
      const int p = a.asc[i];
      base = ((base >> p) << (p + 1)) | (base & (((uint64_t)1 << p) - 1));
    }
    double fr = 1.0, fi = 0.0;
    for (int i = 0; i < a.nout; ++i) {
      const int up = (int)((base >> a.out_site[i]) & 1);
      const double dr = a.out_d[i][2 * up], di = a.out_d[i][2 * up + 1];
      const double nr = fr * dr - fi * di;
      fi = fr * di + fi * dr;
      fr = nr;
    }
    c128 r[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int e = k * NT + tid;
      r[k] = make_double2(0.0, 0.0);
      if (e < nelem) r[k] = x[vec_pos((int64_t)base | off_tid | a.koff[k], a.swz)];
    }
    if (a.nout) {
#pragma unroll
      for (int k = 0; k < PER; ++k) r[k] = site_cmul(fr, fi, r[k]);
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int e = k * NT + tid;
      if (e < nelem) tile[site_slot(e)] = r[k];
    }
    __syncthreads();
    for (int s = 0; s < a.nstages; ++s) {
      const int g = a.stage_g[s];
      if (tid < ngroups) {
        const int t0 = ((tid >> g) << (g + R)) | (tid & ((1 << g) - 1));
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          r[k] = make_double2(0.0, 0.0);
          if (k < (1 << R)) r[k] = tile[site_slot(t0 | (k << g))];
        }
#pragma unroll
        for (int j = 0; j < SITE_OPS_RADIX; ++j) {
          const int kind = a.kind[s][j];
          if (kind == LEVEL_NONE) continue;
          const double *m = a.m[s][j];
          if (kind == LEVEL_GENERAL) {
#pragma unroll
            for (int k = 0; k < PER; ++k) {
              if (k & (1 << j)) continue;
              const c128 v0 = r[k], v1 = r[k | (1 << j)];
              const c128 a00 = site_cmul(m[0], m[1], v0), a01 = site_cmul(m[2], m[3], v1);
              const c128 a10 = site_cmul(m[4], m[5], v0), a11 = site_cmul(m[6], m[7], v1);
              r[k] = make_double2(a00.x + a01.x, a00.y + a01.y);
              r[k | (1 << j)] = make_double2(a10.x + a11.x, a10.y + a11.y);
            }
          } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) r[k] = (k & (1 << j)) ? site_cmul(m[6], m[7], r[k]) : site_cmul(m[0], m[1], r[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < PER; ++k)
          if (k < (1 << R)) tile[site_slot(t0 | (k << g))] = r[k];
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int e = k * NT + tid;
      if (e < nelem) y[vec_pos((int64_t)base | off_tid | a.koff[k], a.swz)] = tile[site_slot(e)];
    }
    __syncthreads();      // the next tile's stores to LDS
  }
}

int launch_site_ops_pass(const void *x, void *y, const SiteOpsPass &a, int tile_bits, int nwg, hipStream_t st) {
  const size_t lds = (size_t)16 << a.tbe;
  if (tile_bits == 13) {
    auto k = site_ops_kernel<512>;
    DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(512), lds, st, (const c128 *)x, (c128 *)y, a);
  } else {
    auto k = site_ops_kernel<256>;
    DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(256), lds, st, (const c128 *)x, (c128 *)y, a);
  }
  DNM_HIP(hipGetLastError());
  return 0;
}

// ---- exp of a diagonal operator --------------------------------------------------------------------------------------
constexpr int EXPD_NT = 256;
constexpr int64_t EXPD_MAX_WG = 1 << 16;

__global__ void __launch_bounds__(EXPD_NT)
expm_diagonal_kernel(const c128 *x, c128 *y, const double *__restrict__ d, int64_t n, int swz, double sr, double si) {
  for (int64_t p = (int64_t)blockIdx.x * EXPD_NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * EXPD_NT) {
    const c128 v = x[p];
    c128 o = make_double2(0.0, 0.0);
    // an amplitude that is exactly zero stays zero, whatever exp does with its row (padding, empty rows)
    if (v.x != 0.0 || v.y != 0.0) {
      const double dd = d[vec_pos(p, swz)];
      double sn, cs;
      sincos(si * dd, &sn, &cs);
      const double e = exp(sr * dd);
      o = site_cmul(e * cs, e * sn, v);
    }
    y[p] = o;
  }
}

int launch_expm_diagonal(const void *x, void *y, const double *d, int64_t n, int swz, double s_re, double s_im,
                         hipStream_t st) {
  if (n <= 0) return 0;
  int64_t nwg = (n + EXPD_NT - 1) / EXPD_NT;
  if (nwg > EXPD_MAX_WG) nwg = EXPD_MAX_WG;
  hipLaunchKernelGGL(expm_diagonal_kernel, dim3((unsigned)nwg), dim3(EXPD_NT), 0, st, (const c128 *)x, (c128 *)y, d, n,
                     swz, s_re, s_im);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
