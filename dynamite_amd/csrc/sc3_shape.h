// Launch shapes of the SpinConserve tiled passes, stated once for both sides: the kernels' template arguments and LDS
// sizes (sc3_dev.h, the launchers) and the host tables that must agree with them (sc3_tables.cpp: the rows a workgroup of
// the lo pass takes, the partner table's zero entry).  No device code: plain C++ compiles this file.
#pragma once

#include <cstdint>

namespace dnm {

constexpr uint32_t SC3_NOROW = 1u << 29;       // lo pass: a sub-group slot without a row

constexpr int cbinom(int n, int k) {
  long long r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return (int)r;
}

// threads of the two passes by field split: the instances (a, w) = (14, 10) and (6, 4) (sc3_instance).  256 threads for
// rows of at most 20 states: the small instance runs four rows per workgroup, so that the tests at L = 11...24 cover the
// sub-group form of the lo pass.  (512 x 7 entries for the lo pass at a = 14: 7.4 ms against 6.4.)
constexpr int sc3_lo_threads(int a) { return a == 14 ? 1024 : 256; }
constexpr int sc3_win_threads(int a) { return a == 14 ? 512 : 64; }

// entries of the lo pass's LDS tile: what the workgroup's threads hold (RPT entries each), at least the longest row
constexpr int sc3_lo_cap(int a, int nt) { return ((cbinom(a, a / 2) + nt - 1) / nt) * nt; }

// shape of the real lo pass: NTR threads with PPT pairs each (DNM_SC3R_SHAPE 0: as many threads as the complex pass and
// twice its entries per thread -- 1024 x 8 entries, a 64 KB tile, two workgroups per CU; 1: half the threads, 512 x 8, a
// 32 KB tile, four workgroups per CU; 2: 1024 x 4, 32 KB, two per CU)
#ifndef DNM_SC3R_SHAPE
#define DNM_SC3R_SHAPE 0
#endif
constexpr int sc3r_threads(int nt) { return (DNM_SC3R_SHAPE == 1 && nt >= 512) ? nt / 2 : nt; }
constexpr int sc3r_pairs(int a, int nt) {
  return (DNM_SC3R_SHAPE == 2 && nt >= 512) ? (cbinom(a, a / 2) / 2 + nt - 1) / nt : (cbinom(a, a / 2) + nt - 1) / nt;
}
constexpr int sc3_lo_cap_r(int a, int nt) { return 2 * sc3r_pairs(a, nt) * sc3r_threads(nt); }

// Rows of the lo pass: a workgroup takes 2^m rows where 2^m rows of their length fit the `cap` entries its threads hold,
// each row a sub-group of whole wavefronts (m <= maxm <= 3); a row's slice of the tile has cap >> m entries.
constexpr int sc3_rows_log2(int nl, int cap, int maxm) {
  int m = 0;
  while (m < maxm && nl <= (cap >> (m + 1))) ++m;
  return m;
}
struct Sc3LoShape {
  int cap;        // entries of the tile
  int threads;    // of a workgroup
  int maxm;       // log2 of the most sub-groups of 64 threads or more
  constexpr int rows_log2(int nl) const { return sc3_rows_log2(nl, cap, maxm); }
};
constexpr Sc3LoShape sc3_lo_shape(int a, bool real) {
  const int nt = sc3_lo_threads(a), threads = real ? sc3r_threads(nt) : nt;
  int maxm = 0;
  while (maxm < 3 && (threads >> (maxm + 1)) >= 64) ++maxm;
  return Sc3LoShape{real ? sc3_lo_cap_r(a, nt) : sc3_lo_cap(a, nt), threads, maxm};
}

}  // namespace dnm
