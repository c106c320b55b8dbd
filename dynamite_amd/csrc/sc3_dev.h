// Device-side helpers shared by the SpinConserve internal-layout kernels (sc3_kernels.hip: chain operators and the
// layout's vector utilities; sc3g_kernels.hip: operators on any bond graph).
#pragma once

#include "sc3.h"
#include "sc3_shape.h"

namespace dnm {

typedef double2 c128;
typedef double d2v __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ int64_t rl_i64(int64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(v & 0xffffffff), l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double rl_f64(double v, int l) { return __longlong_as_double(rl_i64(__double_as_longlong(v), l)); }
__device__ __forceinline__ int rl_i32(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ void store_nt(c128 *p, double re, double im) {
  d2v v = {re, im};
  __builtin_nontemporal_store(v, reinterpret_cast<d2v *>(p));
}
__device__ __forceinline__ c128 load_nt(const c128 *p) {
  d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(p));
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double flip(double c, uint32_t parity_bit) {
  int hi = __double2hiint(c) ^ (int)(parity_bit << 31);
  return __hiloint2double(hi, __double2loint(c));
}

// wave priority by phase (round 4, as in tile_pass_kernel): raised while a workgroup is in a memory phase, lowered for
// its LDS bond loops, so that of the two workgroups of a CU the one asking for memory wins the issue slots
// (SpinConserve(32,16): window pass 5.38 -> 5.25 ms, lo pass level; a rank of config 5 25.7 -> 24.8 ms;
// profiles/r04_sc3_spans.txt; -DDNM_SC3_PRIO=0 builds without)
// the layout's and the operator's tables are read-only: through the constant address space their wave-uniform reads
// stay scalar loads whatever else the kernel contains (see CQuad in matvec_kernels.hip)
#define SC3_CP(T, p) ((const __attribute__((address_space(4))) T *)(p))
#ifndef DNM_SC3_PRIO
#define DNM_SC3_PRIO 1
#endif
#if DNM_SC3_PRIO == 1
#define SC3_PRIO_MEM() asm volatile("s_setprio 3")
#define SC3_PRIO_LDS() asm volatile("s_setprio 0")
#else
#define SC3_PRIO_MEM()
#define SC3_PRIO_LDS()
#endif

constexpr int ilog2c(int v) { return v <= 1 ? 0 : 1 + ilog2c(v >> 1); }

// row (T, W) of a workgroup: everything the kernels derive from the perm entry
struct RowId {
  uint32_t T, W;
  int cw, kr, kl, nrows, pitch;
  int64_t tb, base;        // internal offset of the T block / of the row
};
__device__ __forceinline__ RowId decode_row(uint32_t e, const Sc3Tab &S) {
  RowId r;
  r.T = e >> S.w;
  r.W = e & ((1u << S.w) - 1u);
  r.cw = __popc(r.W);
  r.kr = S.k - __popc(r.T);
  r.kl = r.kr - r.cw;
  r.nrows = S.nl[r.kl];
  r.pitch = S.pitch[r.kl];
  r.tb = SC3_CP(int64_t, S.ibase)[r.T];
  r.base = r.tb + SC3_CP(int64_t, S.icoff)[r.kr * (S.w + 1) + r.cw] + (int64_t)SC3_CP(uint16_t, S.w_rank)[r.W] * r.pitch;
  return r;
}

// waves per SIMD a tiled pass can have: what its LDS tile lets be resident (two workgroups per CU for the 64 KB
// tiles), at most 8 -- the register budget follows from it (128 registers at 512 threads, 64 at 1024)
constexpr int sc3_win_waves(int nt, int tile_kb) {
  int wgs = 160 / (tile_kb > 0 ? tile_kb : 1);
  if (wgs > 2048 / nt) wgs = 2048 / nt;
  if (wgs < 1) wgs = 1;
  const int w = wgs * nt / 256;
  return w > 8 ? 8 : (w < 1 ? 1 : w);
}

}  // namespace
}  // namespace dnm
