// Born sampling and participation entropies: the host arithmetic (plan, scan of the block sums, the uniform stream,
// the sum of the workgroups' partial power sums) and the launchers of born_kernels.hip.  Nothing here needs a device;
// the generator is shared with the kernels.
//
// The weights w_i = |x_i|^2 of the rows of a block are cut into blocks of BORN_BLOCK_ROWS rows in index order.  One
// pass gives the block sums B_b; their inclusive prefix S_b is a serial sum on the host -- fl(S + B) >= S for B >= 0, so
// S is non-decreasing, which a tree scan does not promise and the bisection of the search needs.  A target t belongs to
// the smallest b with S_b > t and, inside it, to the smallest row whose in-block prefix exceeds t - S_{b-1}; that
// prefix is again one by serial chunks (born_kernels.hip), non-decreasing and flat across rows of weight zero, so that
// such a row is never the smallest.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BORN_HD __host__ __device__ __forceinline__
#else
#define BORN_HD inline
#endif

namespace dnm {

constexpr int BORN_BLOCK_LOG2 = 10;
constexpr int64_t BORN_BLOCK_ROWS = (int64_t)1 << BORN_BLOCK_LOG2;   // rows of a block: one wavefront, 16 rows a lane
constexpr int BORN_NT = 256;                                         // threads of a workgroup: four wavefronts
constexpr int64_t BORN_MAX_WG = 2048;     // workgroups of a streaming pass at most (they stride over the blocks)
constexpr int BORN_MAX_Q = 8;             // exponents of one power-sum pass
constexpr int BORN_NSUMS = BORN_MAX_Q + 4;      // a workgroup's partial: P_0..P_7, W, H, wmax, nnz
constexpr int64_t BORN_POW_PER_WG = 4096;       // elements a workgroup of the power-sum pass sweeps at least

// blocks of `nrows` rows, the workgroups of the block-sum pass (four blocks each per step) and the scratch: the block
// sums, which their scan overwrites -- functions of nrows alone
inline void born_plan(int64_t nrows, int64_t *nblocks, int64_t *nworkgroups, size_t *scratch_bytes) {
  const int64_t nb = (nrows + BORN_BLOCK_ROWS - 1) >> BORN_BLOCK_LOG2;
  int64_t nwg = (nb + 3) / 4;
  if (nwg > BORN_MAX_WG) nwg = BORN_MAX_WG;
  if (nwg < 1) nwg = 1;
  *nblocks = nb;
  *nworkgroups = nwg;
  *scratch_bytes = (size_t)nb * sizeof(double);
}

// workgroups of the power-sum pass over n elements
inline int64_t born_power_workgroups(int64_t n) {
  int64_t nwg = (n + BORN_POW_PER_WG - 1) / BORN_POW_PER_WG;
  if (nwg > BORN_MAX_WG) nwg = BORN_MAX_WG;
  return nwg < 1 ? 1 : nwg;
}

// scan[b] = before + sums[0] + ... + sums[b], summed serially in that order (in place allowed); returns the last value
// (`before` when n = 0).  Non-decreasing for sums >= 0.
inline double born_scan(const double *sums, int64_t n, double before, double *scan) {
  double s = before;
  for (int64_t b = 0; b < n; ++b) {
    s += sums[b];
    scan[b] = s;
  }
  return s;
}

// the last b with sums[b] > 0, -1 when there is none
inline int64_t born_last_weight(const double *sums, int64_t n) {
  for (int64_t b = n - 1; b >= 0; --b)
    if (sums[b] > 0.0) return b;
  return -1;
}

// out[0..11] = the workgroups' partials (nwg x BORN_NSUMS) combined in their order: sums, and the maximum of column 10
inline void born_power_reduce(const double *partials, int64_t nwg, double *out) {
  for (int c = 0; c < BORN_NSUMS; ++c) out[c] = 0.0;
  for (int64_t g = 0; g < nwg; ++g)
    for (int c = 0; c < BORN_NSUMS; ++c) {
      const double v = partials[g * BORN_NSUMS + c];
      if (c == BORN_MAX_Q + 2) out[c] = v > out[c] ? v : out[c];
      else out[c] += v;
    }
}

// ---- the uniform stream of the shots ------------------------------------------------------------------------------
// Philox-4x32-10 (philox.h has the device twin that makes the normal deviates of set_random) with the counter
// (lo32(shot), hi32(shot), BORN_C2, BORN_C3) under the key `seed`.  The constant words differ from philox_normal's: with
// the same ones shot i would reuse the bits that set |x_i| in set_random(seed).
constexpr uint32_t BORN_C2 = 0x13198A2Eu, BORN_C3 = 0x03707344u;

BORN_HD void born_philox(uint64_t shot, uint64_t seed, uint32_t c[4]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t c0 = (uint32_t)shot, c1 = (uint32_t)(shot >> 32), c2 = BORN_C2, c3 = BORN_C3;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1,
                   n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
}

// u in [0, 1) from 53 bits (exact) and the flip bit of a shot
BORN_HD double born_uniform(uint64_t shot, uint64_t seed, uint8_t *flip) {
  uint32_t c[4];
  born_philox(shot, seed, c);
  *flip = (uint8_t)(c[2] & 1u);
  return (double)((((uint64_t)c[0] << 32) | c[1]) >> 11) * (1.0 / 9007199254740992.0);
}

#if defined(__HIPCC__)
// ---- launchers (born_kernels.hip) ---------------------------------------------------------------------------------
// x: the nrows amplitudes of a block of a state (device); swz: the XOR-swizzle shift of its layout (0: index order),
// which acts on the block's own positions.  sums_dev: born_plan's nblocks doubles.
int launch_born_block_sums(const void *x, int swz, int64_t nrows, double *sums_dev, hipStream_t st);
// What a search is told.  Targets are read from targets_dev, or made on the device when it is null: t = u W with the
// uniform of shot shot0 + s under seed (flips_dev, may be null, gets the flip bits).  rows_dev[s] = row0 + the local
// row, or -1 for a target outside [before, scan[nblocks - 1]) -- unless clamp_block >= 0, the last block that carries
// weight of the final block of a state, whose last row of weight takes every target at or beyond the total.
struct BornSearch {
  int64_t row0, nrows, nblocks, nshots;
  double before;
  int64_t clamp_block;
  const double *targets_dev;
  uint64_t seed;
  int64_t shot0;
  double total;
};
int launch_born_search(const void *x, int swz, const double *scan_dev, const BornSearch &s, int64_t *rows_dev,
                       uint8_t *flips_dev, hipStream_t st);
// partials_dev: born_power_workgroups(n) x BORN_NSUMS doubles; q: the nq <= BORN_MAX_Q exponents
int launch_born_power_sums(const void *x, int64_t n, int nq, const double *q, double *partials_dev, hipStream_t st);
#endif

}  // namespace dnm
