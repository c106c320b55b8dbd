// Products of single-site operators on a Full-space state, U = (x)_j M_j with M_j any 2 x 2 matrix on spin j (= index
// bit j), y(c') = sum_c prod_j M_j[c'_j][c_j] x(c), and the exponential of a diagonal operator (site_ops_kernels.hip,
// site_ops.cpp).  Here: the host plan of the product and the launchers.  The plan needs no device.
//
// A pass stages tiles of tile_bits index bits in LDS -- the 4 low bits, one 256-byte run of the vector, and tile_bits - 4
// further index bits chosen freely -- applies the 2 x 2 butterflies of the sites it holds and writes the tile back: each
// amplitude is read once and written once per pass.  Sites are classed by bitwise comparison of their matrices:
// identity sites are skipped, diagonal sites are a factor per row in the first pass (those the tile holds as a scaling
// of the butterfly levels, the others as one factor per tile: they need no tile bit of their own), general sites below
// bit 4 belong to the first pass and the other general sites fill the passes in ascending order.
#pragma once
#include <cmath>
#include <cstring>

#include "dnm_common.h"
#include "subspace.h"

namespace dnm {

constexpr int SITE_OPS_MAX_L = 62;
// index bits of a tile: 12 (64 KB of LDS, two workgroups per CU, 4 passes at L = 30) or 13 (128 KB, one workgroup, 3
// passes); the choice and both timings: docs/lab/site_operators.md.  DNM_SITE_OPS_TILE_BITS=12|13 under
// DNM_EXPERIMENTAL=1 overrides it for that measurement.
constexpr int SITE_OPS_TILE_BITS = 12;
constexpr int SITE_OPS_MAX_TILE_BITS = 13;
constexpr int SITE_OPS_RADIX = 4;             // tile bits a thread holds in registers in one stage: 16 amplitudes
constexpr int SITE_OPS_MAX_STAGES = 4;
constexpr int64_t SITE_OPS_MAX_WG = 1 << 16;  // workgroups of a pass at most (they stride over the tiles)

enum { SITE_IDENTITY = -1, SITE_DIAGONAL = -2 };
enum { LEVEL_NONE = 0, LEVEL_GENERAL = 1, LEVEL_DIAGONAL = 2 };

// One pass, as the kernel gets it (by value: about 3.4 KB of kernel arguments, no table on the device).  Tile-local bit
// t < 4 is index bit t; tile-local bit 4 + i is index bit pos[i].  Stage s holds the tile-local bits [g, g + 4) of a
// tile in a thread's registers, g = stage_g[s], and applies m[s][j] to bit g + j where kind[s][j] says so.
struct SiteOpsPass {
  int64_t ntiles;
  int64_t koff[1 << SITE_OPS_RADIX];             // index offset of the tile-local number k * threads: the k-th load of a thread
  int32_t L, tbe, swz, nstages, nfree, nout;     // tbe = min(tile_bits, L); nfree = max(tbe - 4, 0)
  // (32-bit entries: a uniform index into them is a scalar load; bytes would be vector loads that wait on the vector's)
  int32_t pos[10];         // index bit of tile-local bit 4 + i
  int32_t asc[10];         // the same bits in ascending order (where zeros are inserted into a tile's number)
  int32_t stage_g[SITE_OPS_MAX_STAGES];
  int32_t kind[SITE_OPS_MAX_STAGES][SITE_OPS_RADIX];
  double m[SITE_OPS_MAX_STAGES][SITE_OPS_RADIX][8];      // row-major, (re, im)
  int32_t out_site[SITE_OPS_MAX_L - 4];                  // first pass: the diagonal sites outside the tile ...
  double out_d[SITE_OPS_MAX_L - 4][4];                   // ... and their M[0][0], M[1][1]
};

struct SiteOpsPlan {
  int tile_bits, tbe, npasses, nwg;
  size_t lds_bytes;
  bool identity;                       // every site is the identity: nothing to launch
  int8_t site_pass[SITE_OPS_MAX_L];
  std::vector<SiteOpsPass> passes;
};

inline int site_ops_tile_bits() {
  if (const char *v = knob("DNM_SITE_OPS_TILE_BITS")) {
    const int tb = atoi(v);
    if (tb == 12 || tb == 13) return tb;
  }
  return SITE_OPS_TILE_BITS;
}

// the class of a matrix, by the bits of its eight doubles (-0.0 is not 0.0: such a site is general, which is correct)
inline int site_ops_class(const double *m) {
  static const double id[8] = {1, 0, 0, 0, 0, 0, 1, 0};
  if (memcmp(m, id, sizeof id) == 0) return SITE_IDENTITY;
  static const double z[4] = {0, 0, 0, 0};
  if (memcmp(m + 2, z, sizeof z) == 0) return SITE_DIAGONAL;
  return 0;
}

// mats: L matrices of 8 doubles, all finite (the caller has checked); 1 <= L <= SITE_OPS_MAX_L
inline void site_ops_plan(int L, int swz, const double *mats, int tile_bits, SiteOpsPlan *out) {
  SiteOpsPlan &P = *out;
  P.tile_bits = tile_bits;
  P.tbe = L < tile_bits ? L : tile_bits;
  P.lds_bytes = (size_t)16 << P.tbe;
  const int F = tile_bits - 4;
  int cls[SITE_OPS_MAX_L];
  std::vector<int> hi;                  // the general sites >= 4, ascending
  P.identity = true;
  for (int j = 0; j < L; ++j) {
    cls[j] = site_ops_class(mats + 8 * j);
    if (cls[j] != SITE_IDENTITY) P.identity = false;
    if (cls[j] == 0 && j >= 4) hi.push_back(j);
  }
  const int nhi = (int)hi.size();
  P.npasses = nhi ? (nhi + F - 1) / F : 1;
  for (int j = 0; j < L; ++j) P.site_pass[j] = (int8_t)(cls[j] ? cls[j] : 0);
  for (int i = 0; i < nhi; ++i) P.site_pass[hi[i]] = (int8_t)(i / F);
  const int64_t ntiles = (int64_t)1 << (L - P.tbe);
  P.nwg = (int)(ntiles < SITE_OPS_MAX_WG ? ntiles : SITE_OPS_MAX_WG);
  P.passes.clear();
  if (P.identity) return;
  const int nfree = P.tbe > 4 ? P.tbe - 4 : 0;
  for (int p = 0; p < P.npasses; ++p) {
    SiteOpsPass a;
    memset(&a, 0, sizeof a);
    a.ntiles = ntiles;
    a.L = L;
    a.tbe = P.tbe;
    a.swz = swz;
    a.nfree = nfree;
    // the tile's free bits: this pass's general sites, then (first pass) diagonal sites, then any other bit
    bool in_tile[SITE_OPS_MAX_L] = {};
    int n = 0;
    for (int i = p * F; i < nhi && i < (p + 1) * F; ++i) a.pos[n++] = hi[i];
    auto pad = [&](int want) {          // want = 0: any bit (general sites of other passes are identity levels here)
      for (int j = 4; j < L && n < nfree; ++j) {
        bool taken = false;
        for (int i = 0; i < n; ++i) taken |= a.pos[i] == j;
        if (!taken && (want == 0 || cls[j] == want)) a.pos[n++] = j;
      }
    };
    if (p == 0) pad(SITE_DIAGONAL);
    pad(SITE_IDENTITY);
    pad(0);
    for (int i = 0; i < nfree; ++i) {
      in_tile[a.pos[i]] = true;
      a.asc[i] = a.pos[i];
    }
    for (int i = 1; i < nfree; ++i)
      for (int k = i; k > 0 && a.asc[k - 1] > a.asc[k]; --k) std::swap(a.asc[k - 1], a.asc[k]);
    // the offsets of a thread's loads: thread t of 2^(tile_bits - 4) takes the tile-local numbers k * threads + t
    for (int k = 0; k < (1 << SITE_OPS_RADIX); ++k) {
      const int t = k << (tile_bits - 4);
      for (int i = 0; i < nfree; ++i) a.koff[k] |= (int64_t)((t >> (4 + i)) & 1) << a.pos[i];
    }
    // the levels: what this pass applies at each tile-local bit
    int lvl_site[SITE_OPS_MAX_TILE_BITS], lvl_kind[SITE_OPS_MAX_TILE_BITS];
    for (int t = 0; t < P.tbe; ++t) {
      const int site = t < 4 ? t : a.pos[t - 4];
      int kind = LEVEL_NONE;
      if (cls[site] == SITE_DIAGONAL && p == 0) kind = LEVEL_DIAGONAL;
      if (cls[site] == 0 && P.site_pass[site] == p) kind = LEVEL_GENERAL;
      lvl_site[t] = site;
      lvl_kind[t] = kind;
    }
    // stages: the lowest level not yet held starts a group of 4 tile-local bits (the last group is shifted down to end
    // at the tile's top bit)
    const int R = P.tbe < SITE_OPS_RADIX ? P.tbe : SITE_OPS_RADIX;
    bool done[SITE_OPS_MAX_TILE_BITS] = {};
    for (int t = 0; t < P.tbe; ++t) {
      if (lvl_kind[t] == LEVEL_NONE || done[t]) continue;
      const int g = t < P.tbe - R ? t : P.tbe - R, s = a.nstages++;
      a.stage_g[s] = g;
      for (int j = 0; j < R; ++j) {
        if (done[g + j]) continue;
        done[g + j] = true;
        a.kind[s][j] = lvl_kind[g + j];
        memcpy(a.m[s][j], mats + 8 * lvl_site[g + j], 8 * sizeof(double));
      }
    }
    if (p == 0)
      for (int j = 4; j < L; ++j)
        if (cls[j] == SITE_DIAGONAL && !in_tile[j]) {
          a.out_site[a.nout] = j;
          a.out_d[a.nout][0] = mats[8 * j];
          a.out_d[a.nout][1] = mats[8 * j + 1];
          a.out_d[a.nout][2] = mats[8 * j + 6];
          a.out_d[a.nout][3] = mats[8 * j + 7];
          ++a.nout;
        }
    P.passes.push_back(a);
  }
}

#if defined(__HIPCC__)
// one pass over the vector (x == y allowed: a tile is read whole before it is written, and tiles are disjoint)
int launch_site_ops_pass(const void *x, void *y, const SiteOpsPass &a, int tile_bits, int nwg, hipStream_t st);
// y[p] = exp((s_re + i s_im) d[row(p)]) x[p], row(p) = vec_pos(p, swz); y[p] = 0 where x[p] is 0.  d: device, n doubles
int launch_expm_diagonal(const void *x, void *y, const double *d, int64_t n, int swz, double s_re, double s_im,
                         hipStream_t st);
#endif

}  // namespace dnm
