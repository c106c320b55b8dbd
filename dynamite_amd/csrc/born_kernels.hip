// Born sampling and the power sums of the participation entropies: streaming passes over w_i = |x_i|^2 (born.h has
// the scheme and the host arithmetic).
//   born_block_sums_kernel   B_b = the sum of w over block b (1024 rows in index order): one wavefront per block, 16
//                            coalesced loads a lane, a fixed butterfly over the lanes
//   born_search_kernel       one wavefront per shot: bisection of the scanned block sums, then the block's 1024 rows
//                            again, lane l the 16 consecutive rows [16 l, 16 l + 16): their serial sums q_j, the lane
//                            totals scanned serially into offsets O_l, in-block prefix P = O_l + q_j -- non-decreasing
//                            (fl(O + q) is monotone in q, and O_{l+1} = O_l + q_15 is lane l's last prefix), equal on
//                            both sides of a row of weight zero
//   born_power_sums_kernel   sum w^q for up to 8 exponents, sum w, sum w ln w, max w and the count of w > 0
// No atomics and fixed reduction shapes: two calls return the same bits.  Workgroup counts are functions of the number
// of rows alone.  A swizzled vector is read as it lies: index i sits at position vec_pos(i); the swizzle keeps runs of
// 16 elements together, so both access patterns stay whole 256-byte runs.
#include "born.h"
#include "dnm_common.h"
#include "subspace.h"

namespace dnm {

typedef double born_d2v __attribute__((ext_vector_type(2)));

// (separate roundings, no contraction: every kernel sees the same weight of a row)
__device__ __forceinline__ double born_weight(const born_d2v a) {
  return __dadd_rn(__dmul_rn(a.x, a.x), __dmul_rn(a.y, a.y));
}

__device__ __forceinline__ double born_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ void __launch_bounds__(BORN_NT)
born_block_sums_kernel(const born_d2v *__restrict__ x, int swz, int64_t nrows, int64_t nblocks,
                       double *__restrict__ sums) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < nblocks; b += (int64_t)gridDim.x * 4) {
    const int64_t i0 = (b << BORN_BLOCK_LOG2) + lane;
    double w[16];
    if (((b + 1) << BORN_BLOCK_LOG2) <= nrows) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        w[j] = born_weight(__builtin_nontemporal_load(x + vec_pos(i0 + 64 * j, swz)));
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int64_t i = i0 + 64 * j;
        w[j] = i < nrows ? born_weight(__builtin_nontemporal_load(x + vec_pos(i, swz))) : 0.0;
      }
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += w[j];
    s = born_wave_sum(s);
    if (lane == 0) sums[b] = s;
  }
}

__global__ void __launch_bounds__(BORN_NT)
born_search_kernel(const born_d2v *__restrict__ x, int swz, const double *__restrict__ scan, const BornSearch p,
                   int64_t *__restrict__ rows, uint8_t *__restrict__ flips) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // (the same in every lane of a wavefront)
  if (s >= p.nshots) return;
  double t;
  if (p.targets_dev) {
    t = p.targets_dev[s];
  } else {
    uint8_t flip;
    t = __dmul_rn(born_uniform((uint64_t)(p.shot0 + s), p.seed, &flip), p.total);
    if (flips && lane == 0) flips[s] = flip;
  }
  // the smallest block b with scan[b] > t
  int64_t lo = 0, hi = p.nblocks;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (scan[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  int64_t b = lo;
  double r;
  if (!(t >= p.before) || (b == p.nblocks && p.clamp_block < 0)) {
    if (lane == 0) rows[s] = -1;
    return;
  }
  if (b == p.nblocks) {            // at or beyond the total: the last row of weight takes it
    b = p.clamp_block;
    r = __builtin_inf();
  } else {
    r = t - (b ? scan[b - 1] : p.before);
  }
  const int64_t i0 = (b << BORN_BLOCK_LOG2) + 16 * lane;
  const born_d2v *xl = x + vec_pos(i0 < p.nrows ? i0 : 0, swz);       // (a run of 16 stays together under the swizzle)
  double q[16];
  int lastnz = -1;
  double run = 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double w = i0 + j < p.nrows ? born_weight(xl[j]) : 0.0;
    if (w > 0.0) lastnz = 16 * lane + j;
    run += w;
    q[j] = run;
  }
  // offsets: the lane totals summed serially, the same sum in every lane
  double off = 0.0, tot = 0.0;
  for (int l = 0; l < 64; ++l) {
    const double tl = __shfl(run, l, 64);
    if (lane == l) off = tot;
    tot += tl;
  }
  int first = BORN_BLOCK_ROWS;
#pragma unroll
  for (int j = 15; j >= 0; --j)
    if (off + q[j] > r) first = 16 * lane + j;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int f = __shfl_xor(first, m, 64), z = __shfl_xor(lastnz, m, 64);
    first = f < first ? f : first;
    lastnz = z > lastnz ? z : lastnz;
  }
  // (rounding may leave no row beyond the residual: the block's last row of weight)
  const int local = first < BORN_BLOCK_ROWS ? first : lastnz;
  if (lane == 0) rows[s] = local < 0 ? -1 : p.row0 + (b << BORN_BLOCK_LOG2) + local;
}

struct BornPowers {
  int nq;
  int kind[BORN_MAX_Q];         // 2, 3, 4: by multiplication; 0: pow
  double q[BORN_MAX_Q];
};

// acc[K] += w^q_K for the exponents K, K + 1, ... of the pass (static indices: the sums stay in registers; the branches
// are the same in every lane)
template <int K>
__device__ __forceinline__ void born_add_powers(double (&acc)[BORN_NSUMS], const BornPowers &pw, double w, double w2) {
  if constexpr (K < BORN_MAX_Q) {
    if (K < pw.nq) {
      const int kind = pw.kind[K];
      double v;
      if (kind == 2) v = w2;
      else if (kind == 3) v = w2 * w;
      else if (kind == 4) v = w2 * w2;
      else v = pow(w, pw.q[K]);
      acc[K] += v;
      born_add_powers<K + 1>(acc, pw, w, w2);
    }
  }
}

__global__ void __launch_bounds__(BORN_NT)
born_power_sums_kernel(const born_d2v *__restrict__ x, int64_t n, const BornPowers pw, double *__restrict__ partials) {
  __shared__ double red[4][BORN_NSUMS];
  double acc[BORN_NSUMS];
#pragma unroll
  for (int c = 0; c < BORN_NSUMS; ++c) acc[c] = 0.0;
  // four loads a thread in flight, then the arithmetic in a loop that is kept rolled: one copy of log and of each
  // exponent's pow in the kernel.  An element beyond the end counts as weight zero, which adds nothing to any sum.
  const int64_t T = (int64_t)gridDim.x * BORN_NT;
  for (int64_t i = (int64_t)blockIdx.x * BORN_NT + threadIdx.x; i < n; i += 4 * T) {
    double w4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w4[j] = i + j * T < n ? born_weight(__builtin_nontemporal_load(x + i + j * T)) : 0.0;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const double w = j == 0 ? w4[0] : j == 1 ? w4[1] : j == 2 ? w4[2] : w4[3];
      acc[BORN_MAX_Q] += w;
      acc[BORN_MAX_Q + 1] += w > 0.0 ? w * log(w) : 0.0;
      acc[BORN_MAX_Q + 2] = fmax(acc[BORN_MAX_Q + 2], w);
      acc[BORN_MAX_Q + 3] += w > 0.0 ? 1.0 : 0.0;
      born_add_powers<0>(acc, pw, w, w * w);
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < BORN_NSUMS; ++c) {
    double v = acc[c];
    if (c == BORN_MAX_Q + 2) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    } else {
      v = born_wave_sum(v);
    }
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < BORN_NSUMS) {
    const int c = threadIdx.x;
    double v = red[0][c];
    for (int wv = 1; wv < 4; ++wv) v = c == BORN_MAX_Q + 2 ? fmax(v, red[wv][c]) : v + red[wv][c];
    partials[(int64_t)blockIdx.x * BORN_NSUMS + c] = v;
  }
}

int launch_born_block_sums(const void *x, int swz, int64_t nrows, double *sums_dev, hipStream_t st) {
  int64_t nblocks, nwg;
  size_t bytes;
  born_plan(nrows, &nblocks, &nwg, &bytes);
  if (nblocks == 0) return 0;
  hipLaunchKernelGGL(born_block_sums_kernel, dim3((unsigned)nwg), dim3(BORN_NT), 0, st, (const born_d2v *)x, swz, nrows,
                     nblocks, sums_dev);
  DNM_HIP(hipGetLastError());
  return 0;
}

int launch_born_search(const void *x, int swz, const double *scan_dev, const BornSearch &s, int64_t *rows_dev,
                       uint8_t *flips_dev, hipStream_t st) {
  if (s.nshots == 0) return 0;
  DNM_CHECK(s.nshots <= ((int64_t)1 << 32), "%lld shots in one call: at most 2^32", (long long)s.nshots);
  hipLaunchKernelGGL(born_search_kernel, dim3((unsigned)((s.nshots + 3) / 4)), dim3(BORN_NT), 0, st,
                     (const born_d2v *)x, swz, scan_dev, s, rows_dev, flips_dev);
  DNM_HIP(hipGetLastError());
  return 0;
}

int launch_born_power_sums(const void *x, int64_t n, int nq, const double *q, double *partials_dev, hipStream_t st) {
  BornPowers pw{};
  pw.nq = nq;
  for (int k = 0; k < nq; ++k) {
    pw.q[k] = q[k];
    pw.kind[k] = q[k] == 2.0 ? 2 : q[k] == 3.0 ? 3 : q[k] == 4.0 ? 4 : 0;
  }
  hipLaunchKernelGGL(born_power_sums_kernel, dim3((unsigned)born_power_workgroups(n)), dim3(BORN_NT), 0, st,
                     (const born_d2v *)x, n, pw, partials_dev);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
