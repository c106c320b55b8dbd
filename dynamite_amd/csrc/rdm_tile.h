// What the reduced-density-matrix kernels share (rdm_kernels.hip: the dense form, rdm_sector_kernels.hip: block by
// block for fixed-magnetisation states): the bit deposit, the lower-triangle tile index, the 64 x 64 tile on the matrix
// cores and the last step of the slice sum.  The two forms differ in how they gather psi(a, t), in nothing else.
#pragma once
#include "kernels.h"

namespace dnm {

typedef double2 c128;
typedef double mfma_acc __attribute__((ext_vector_type(4)));

constexpr int RDM_NT = 256;       // threads of a workgroup, every kernel of the two files
constexpr int RDM_TM = 64;        // side of a matrix-core tile

// waves per SIMD the matrix-core kernels are compiled for / chunk size: 4 waves (128 registers, a few B/lane of
// scratch) run 2.4 % faster than 3; chunks of 32 traced configurations (64 KB of LDS, two workgroups per CU) 2.7 %
// slower (GPU session 39)
#ifndef DNM_RDM_WAVES
#define DNM_RDM_WAVES 4
#endif
#ifndef DNM_RDM_MSTAGE
#define DNM_RDM_MSTAGE 1024
#endif

__device__ __forceinline__ uint64_t rdm_deposit(uint64_t v, const int8_t *len, const int8_t *pos, int nseg) {
  uint64_t out = 0;
  for (int i = 0; i < nseg; ++i) {
    out |= (v & (((uint64_t)1 << len[i]) - 1)) << pos[i];
    v >>= len[i];
  }
  return out;
}

// tile (ti, tj), tj <= ti, from the linear lower-triangle index
__device__ __forceinline__ void rdm_tile_coords(int tile, int *ti_out, int *tj_out) {
  int ti = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
  while ((int64_t)(ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  while ((int64_t)ti * (ti + 1) / 2 > tile) --ti;
  *ti_out = ti;
  *tj_out = tile - (int)((int64_t)ti * (ti + 1) / 2);
}

// ---- a 64 x 64 tile on the matrix cores ---------------------------------------------------------------------
// out (64 x 64, row-major) = A B^H over nchunks chunks of TK = MST / 64 traced configurations, the rank-T update done
// by v_mfma_f64_16x16x4_f64: a wavefront owns a 32 x 32 block of the tile (2 x 2 MFMA blocks, real and imaginary
// accumulators: 64 VGPRs) and per four traced configurations reads two A and two B fragments from LDS -- each lane one
// complex amplitude (ds_read_b128: row / column = lane & 15, traced slot = lane >> 4) -- where the VALU form reads
// eight amplitudes per 16 complex products: an eighth of the LDS traffic per flop, and the FMAs leave the vector unit.
//   rho = A B^H:  Re += Ar Br^T + Ai Bi^T,   Im += Ai Br^T + (-Ar) Bi^T      (four real MFMAs per complex block)
// C/D layout of the f64 MFMA (not the f32 one): col = lane & 15, row = (lane >> 4) + 4 * reg.
// The next chunk's amplitudes are gathered into registers while the matrix cores work on the staged one.
//   As, Bs         the LDS operand buffers, MST amplitudes each (element e: row e % 64, traced slot e / 64); a diagonal
//                  tile (diag_tile) is A A^H, Bs stays untouched
//   prepare(c)     leaves in LDS whatever gather needs per traced configuration of chunk c, in a slot of parity c & 1
//                  (one lane per configuration); called for c up to nchunks + 1
//   gather(c, va, vb)   a thread's MST / RDM_NT amplitudes of chunk c per operand: element i is amplitude
//                  threadIdx.x + i * RDM_NT of the buffers (vb is not read for a diagonal tile)
template <int MST, class Prepare, class Gather>
__device__ __forceinline__ void rdm_mfma_tile(c128 *As, c128 *Bs, bool diag_tile, int64_t nchunks,
                                              c128 *__restrict__ out, Prepare prepare, Gather gather) {
  constexpr int TM = RDM_TM;
  constexpr int TK = MST / TM;            // traced configurations per chunk (16: four MFMA steps)
  constexpr int EPT = MST / RDM_NT;       // amplitudes per thread and operand in a chunk
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wy = wave >> 1, wx = wave & 1;
  mfma_acc re[2][2], im[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) re[i][j] = im[i][j] = mfma_acc{0.0, 0.0, 0.0, 0.0};
  const c128 *Bp = diag_tile ? As : Bs;

  c128 va[EPT], vb[EPT];
  prepare(0);
  prepare(1);
  __syncthreads();
  if (0 < nchunks) gather(0, va, vb);
  __syncthreads();                              // every wave has read its slots before prepare(2)
  for (int64_t c = 0; c < nchunks; ++c) {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      As[tid + i * RDM_NT] = va[i];
      if (!diag_tile) Bs[tid + i * RDM_NT] = vb[i];
    }
    prepare(c + 2);                             // (its slot was last read by gather(c), before this barrier)
    __syncthreads();
    if (c + 1 < nchunks) gather(c + 1, va, vb); // in flight under the MFMAs below
#pragma unroll
    for (int kk = 0; kk < TK; kk += 4) {
      const int slot = (kk + (lane >> 4)) * TM + (lane & 15);
      c128 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = As[slot + wy * 32 + i * 16];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = Bp[slot + wx * 32 + j * 16];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].x, b[j].x, re[i][j], 0, 0, 0);
          re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].y, b[j].y, re[i][j], 0, 0, 0);
          im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].y, b[j].x, im[i][j], 0, 0, 0);
          im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[i].x, b[j].y, im[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wy * 32 + i * 16 + (lane >> 4) + 4 * r, col = wx * 32 + j * 16 + (lane & 15);
        out[row * TM + col] = make_double2(re[i][j][r], im[i][j][r]);
      }
}

// ---- the last step of the slice sum -------------------------------------------------------------------------
// Tile `tile` = (ti, tj) of rho (D x D, row-major) = scale * the sum of the nsplit <= 32 slices rdm_sum_slices left;
// the upper triangle is the conjugate transpose.  One workgroup per tile.
template <int TM>
__device__ __forceinline__ void rdm_finalize_tile(const c128 *__restrict__ partial, int ntiles, int nsplit, int tile,
                                                  int ti, int tj, int64_t D, double scale, c128 *__restrict__ rho) {
  for (int e = threadIdx.x; e < TM * TM; e += RDM_NT) {
    const int r = e / TM, cidx = e % TM;
    const int64_t a = (int64_t)ti * TM + r, b = (int64_t)tj * TM + cidx;
    if (a >= D || b >= D) continue;
    // a diagonal tile holds both triangles, accumulated in different orders (MFMA: the imaginary part of (a, b) and
    // of (b, a) add the same products in different sequence): the lower one is taken and mirrored like every other
    // tile, so that rho is Hermitian to the last bit, as the reference's element-by-element sum is
    if (ti == tj && cidx > r) continue;
    double sr = 0.0, si = 0.0;
    for (int s = 0; s < nsplit; ++s) {
      const c128 v = partial[((int64_t)s * ntiles + tile) * (TM * TM) + e];
      sr += v.x;
      si += v.y;
    }
    sr *= scale;
    si *= scale;
    if (a == b) si = 0.0;     // |psi|^2 sums: the reference's a * conj(a) has no imaginary part either
    rho[a * D + b] = make_double2(sr, si);
    if (a != b) rho[b * D + a] = make_double2(sr, -si);
  }
}

}  // namespace dnm
