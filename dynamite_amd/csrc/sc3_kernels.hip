// SpinConserve(L,k) x SpinConserve(L,k) multiply in the three-field internal layout (sc3.h): two tiled passes for
// nearest-neighbour chains, a row kernel for any other operator, and the layout's vector utilities.
// Semantics: MatMult_CPU_General (src/dynamite/_backend/bpetsc_template_2.c:371-412) with the index maps of
// bsubspace_impl.h:187-245; the cached-diagonal variant follows bpetsc_template_1.c:186-199.
#include "sc3.h"

#include <algorithm>

#include "dnm_common.h"
#include "kernels.h"
#include "philox.h"
#include "sc3_dev.h"
#include "sc3_launch.h"

namespace dnm {

namespace {

// ---------------------------------------------------------------------------------------------------------
// lo pass (the second, accumulating pass): y += (bonds inside Lo, the Lo/W boundary, whatever else bondsA names
// and the diagonal) x.  A workgroup takes 2^m rows (T, W), m = 0..3 (round 4): a row has C(a, kl) states -- 3432 at
// kl = 7, 2002 at kl = 5, 364 at kl = 3 -- and one row per 1024-thread workgroup left 44 % of the lanes idle at
// SpinConserve(32,16).  The workgroup splits into 2^m sub-groups of NT >> m threads (whole wavefronts), each with its
// own row and its own slice of the LDS tile; everything that is uniform per row is uniform per wavefront, as before.
// perm holds 8 entries per workgroup: entry j = row of sub-group j | m << 30, bit 29 set = no row (SC3_NOROW).
//   DIAGM 0: no diagonal; 1: cached (internal order, 8 B/row); 2: on the fly -- terms that see Lo only from a table
//   over (kl, lr) (L2-resident), terms that see (T, W) only as one number per row, terms that see both as at most
//   four (Lo sign mask, per-row coefficient) pairs.
//   SYM: every bond coefficient is real and the same in both directions (Heisenberg, XXZ, XX chains).
//   ACC: true = the second pass (y += ...); false = it runs first and writes y, starting from the solver's start
//   vectors -- the order of a partitioned multiply, where this pass needs nothing from other ranks (a rank owns whole
//   T blocks) and runs while the window of x is still on the links.
template <int A, int NT, int DIAGM, bool SYM, bool ACC>
__global__ void __launch_bounds__(NT, sc3_win_waves(NT, (sc3_lo_cap(A, NT) * 16 + 1023) / 1024 + 1))
sc3_lo_pass(const Sc3Tab S, const Sc3Op O, const uint32_t *__restrict__ perm, const Sc3Call C,
            const c128 *__restrict__ xw, c128 *__restrict__ y) {
  constexpr int MAXROWS = cbinom(A, A / 2);
  constexpr int RPT = (MAXROWS + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int32_t cl[A * (A + 1)];
  __shared__ double red[3 * (NT / 64)];
  __shared__ double dsh[5 * 8];
  const uint32_t e0 = SC3_CP(uint32_t, perm)[8 * (size_t)blockIdx.x];
  if (e0 == 0xffffffffu) return;                        // padding of the dispatch order: a workgroup without rows
  const int lane = threadIdx.x & 63;
  const int w = S.w;
  // sub-group of this wavefront: NTS threads, RPT entries each, its own slice of the tile
  const int logm = (int)(e0 >> 30);
  const int NTS = NT >> logm;
  const int sub = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) >> (ilog2c(NT) - 6 - logm);
  const int tsub = (int)threadIdx.x & (NTS - 1);
  const uint32_t e = SC3_CP(uint32_t, perm)[8 * (size_t)blockIdx.x + sub];
  const bool has_row = !(e & SC3_NOROW);
  c128 *xs = reinterpret_cast<c128 *>(smem) + (size_t)sub * ((NT * RPT) >> logm);
  const RowId R = decode_row(has_row ? (e & (SC3_NOROW - 1u)) : (e0 & (SC3_NOROW - 1u)), S);
  const uint32_t T = R.T, W = R.W;
  const int cw = R.cw, kr = R.kr, kl = R.kl, nrows = has_row ? R.nrows : 0, p = has_row ? R.pitch : 0;
  const int64_t tb = R.tb, base = R.base;
  const c128 *__restrict__ x = xw - C.win_start;
  const int64_t lbase = base - C.row0;                 // position of the row in this rank's vectors

  SC3_PRIO_MEM();
  uint32_t lowb[RPT];
  c128 xv[RPT];
  const auto pat = SC3_CP(uint16_t, S.lo_pat) + S.lo_off[kl];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int r = tsub + i * NTS;
    lowb[i] = 0;
    xv[i] = make_double2(0.0, 0.0);
    if (r < nrows) {
      lowb[i] = pat[r];
      xv[i] = x[base + r];
    }
  }
  // bonds outside Lo, one per lane: l = 0 the Lo/W boundary, 1..w-1 inside W, w the W/T boundary, above inside T.
  // Each couples this row to one other row at a uniform offset (the boundary bond: a contiguous part of it).
  int act = 0, r0 = 0, r1 = nrows;
  int64_t delta = 0;
  double c0 = 0.0, c1 = 0.0;
  {
    const int b = A - 1 + lane;
    if (b < S.L - 1 && ((O.bondsA >> b) & 1ull)) {
      bool up = false;
      if (lane == 0) {
        const int cut = SC3_CP(int32_t, S.cbin)[(A - 1) * 17 + kl];                   // rows below: top bit of Lo clear
        if (W & 1u) {                                                // the one comes down into Lo
          if (cut > 0) {
            act = 1; r0 = 0; r1 = cut; up = false;
            delta = tb + SC3_CP(int64_t, S.icoff)[kr * (w + 1) + cw - 1] + (int64_t)SC3_CP(uint16_t, S.w_rank)[W & ~1u] * S.pitch[kl + 1] +
                    SC3_CP(int32_t, S.cbin)[(A - 1) * 17 + kl + 1] - base;
          }
        } else if (cut < nrows) {                                    // the one goes up into W
          act = 1; r0 = cut; r1 = nrows; up = true;
          delta = tb + SC3_CP(int64_t, S.icoff)[kr * (w + 1) + cw + 1] + (int64_t)SC3_CP(uint16_t, S.w_rank)[W | 1u] * S.pitch[kl - 1] - cut - base;
        }
      } else if (lane < w) {
        const int bw = lane - 1;
        const uint32_t pair = (W >> bw) & 3u;
        if (pair == 1u || pair == 2u) {
          act = 1; up = pair == 1u;
          delta = ((int64_t)SC3_CP(uint16_t, S.w_rank)[W ^ (3u << bw)] - (int64_t)SC3_CP(uint16_t, S.w_rank)[W]) * p;
        }
      } else if (lane == w) {
        const uint32_t pair = ((W >> (w - 1)) & 1u) | ((T & 1u) << 1);
        if (pair == 1u) {
          act = 1; up = true;
          delta = SC3_CP(int64_t, S.ibase)[T | 1u] + SC3_CP(int64_t, S.icoff)[(kr - 1) * (w + 1) + cw - 1] +
                  (int64_t)SC3_CP(uint16_t, S.w_rank)[W & ~(1u << (w - 1))] * p - base;
        } else if (pair == 2u) {
          act = 1; up = false;
          delta = SC3_CP(int64_t, S.ibase)[T & ~1u] + SC3_CP(int64_t, S.icoff)[(kr + 1) * (w + 1) + cw + 1] +
                  (int64_t)SC3_CP(uint16_t, S.w_rank)[W | (1u << (w - 1))] * p - base;
        }
      } else {
        const int bt = lane - w - 1;
        const uint32_t pair = (T >> bt) & 3u;
        if (pair == 1u || pair == 2u) {
          act = 1; up = pair == 1u;
          delta = SC3_CP(int64_t, S.ibase)[T ^ (3u << bt)] - tb;
        }
      }
      if (act) {
        c0 = SC3_CP(double, O.bond)[4 * b + (up ? 0 : 2)];
        c1 = SC3_CP(double, O.bond)[4 * b + (up ? 1 : 3)];
      }
    }
  }
  uint64_t hb = has_row ? __ballot(act) : 0ull;

  for (int tt = threadIdx.x; tt < A * (A + 1); tt += NT) {
    const int lo = tt / (A + 1), o = tt % (A + 1);
    cl[tt] = SC3_CP(int32_t, S.cbin)[lo * 17 + o];
  }
  // on-the-fly diagonal: what the row (T, W) contributes -- group 0 to every state of the row, groups 1..4 with the
  // sign of a Lo pattern.  The first wavefront evaluates the terms, one per lane, and leaves the sums in LDS; they
  // are applied after the barrier the tile needs anyway.
  if (DIAGM == 2 && tsub < 64) {
    const uint64_t hi = ((uint64_t)T << w) | W;
    double v0 = 0.0, vm[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < O.ndt; t0 += 64) {
      const int t = t0 + lane;
      if (t < O.ndt) {
        const uint64_t sg = SC3_CP(uint64_t, O.dt_sign)[t];                       // bits 61..63: the group
        const double c = flip(SC3_CP(double, O.dt_coef)[t], (uint32_t)__popcll(hi & sg & 0x1fffffffffffffffull) & 1u);
        const int g = (int)(sg >> 61);
        if (g == 0) v0 += c;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (g == j + 1) vm[j] += c;
      }
    }
    v0 = wave_sum(v0);
    if (lane == 0) dsh[5 * sub] = v0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < O.ngroups) {
        const double s = wave_sum(vm[j]);
        if (lane == 0) dsh[5 * sub + j + 1] = s;
      }
  }
  double accr[RPT], acci[RPT];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int r = tsub + i * NTS;
    accr[i] = 0.0;
    acci[i] = 0.0;
    if (r < nrows) {
      xs[r] = xv[i];
      if (DIAGM == 1) {
        const double dg = __builtin_nontemporal_load(O.diag + lbase + r);
        accr[i] = dg * xv[i].x;
        acci[i] = dg * xv[i].y;
      }
    }
  }
  while (hb) {
    const int m = __ffsll((long long)hb) - 1;
    hb &= hb - 1;
    const c128 *__restrict__ pp = x + (base + rl_i64(delta, m));
    const double cr = rl_f64(c0, m), ci = rl_f64(c1, m);
    const int q0 = rl_i32(r0, m), q1 = rl_i32(r1, m);
    c128 v[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int r = tsub + i * NTS;
      v[i] = make_double2(0.0, 0.0);
      if (r >= q0 && r < q1) v[i] = pp[r];
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      accr[i] = fma(cr, v[i].x, accr[i]);
      acci[i] = fma(cr, v[i].y, acci[i]);
      if (!SYM) {
        accr[i] = fma(-ci, v[i].y, accr[i]);
        acci[i] = fma(ci, v[i].x, acci[i]);
      }
    }
  }
  // the accumulating pass asks for its y now: it arrives while the bonds are served from LDS (the x values of the
  // entries are read back from the tile below, so their registers are free for it)
  c128 yv[RPT];
  if (ACC) {
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int r = tsub + i * NTS;
      yv[i] = make_double2(0.0, 0.0);
      if (r < nrows) yv[i] = load_nt(y + lbase + r);
    }
  }
  double dlv[RPT];
  if (DIAGM == 2) {          // the Lo-only part of the diagonal (L2-resident table), asked for before the barrier as well
    const auto dl = SC3_CP(double, O.dlo) + S.lo_off[kl];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int r = tsub + i * NTS;
      dlv[i] = r < nrows ? dl[r] : 0.0;
    }
  }
  __syncthreads();
  SC3_PRIO_LDS();
  if (DIAGM == 2) {
    const double dg0 = dsh[5 * sub];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int r = tsub + i * NTS;
      if (r < nrows) {
        double dg = dlv[i] + dg0;
        for (int j = 0; j < O.ngroups; ++j) dg += flip(dsh[5 * sub + j + 1], (uint32_t)__popc(lowb[i] & O.glo[j]) & 1u);
        const c128 xo = xs[r];
        accr[i] = fma(dg, xo.x, accr[i]);
        acci[i] = fma(dg, xo.y, acci[i]);
      }
    }
  }
  // bonds inside Lo.  (A partner table per (entry, bond) -- what the window pass uses, Sc3Tab::w_nb -- was measured here
  // too: 32 % fewer vector instructions and 0.3-0.9 ms MORE time, its 24 B per entry come from the L2 and every bond
  // then reads LDS, profiles/r03_exp11_sc3_tables.txt: this pass is not bound by its instructions.)
  for (int lo = 0; lo < A - 1; ++lo) {
    if (!((O.present >> lo) & 1ull)) continue;
    const double ure = SC3_CP(double, O.bond)[4 * lo], uim = SC3_CP(double, O.bond)[4 * lo + 1], dre = SC3_CP(double, O.bond)[4 * lo + 2], dim_ = SC3_CP(double, O.bond)[4 * lo + 3];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int r = tsub + i * NTS;
      const uint32_t pair = (lowb[i] >> lo) & 3u;
      if (r < nrows && (pair == 1u || pair == 2u)) {
        const bool up = pair == 1u;
        const int ord0 = __popc(lowb[i] & ((1u << lo) - 1u));
        const int d = cl[lo * (A + 1) + ord0];
        const c128 xp = xs[up ? r + d : r - d];
        if (SYM) {
          accr[i] = fma(ure, xp.x, accr[i]);
          acci[i] = fma(ure, xp.y, acci[i]);
        } else {
          const double cre = up ? ure : dre, cim = up ? uim : dim_;
          accr[i] = fma(cre, xp.x, accr[i]);
          acci[i] = fma(cre, xp.y, acci[i]);
          accr[i] = fma(-cim, xp.y, accr[i]);
          acci[i] = fma(cim, xp.x, acci[i]);
        }
      }
    }
  }
  double dr = 0.0, di = 0.0, dn = 0.0;
  SC3_PRIO_MEM();
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int r = tsub + i * NTS;
    if (r < p) {                                  // the padding of a row is written too (zeros)
      double ar = accr[i], ai = acci[i];
      if (r < nrows) {
        if (ACC) {
          ar += yv[i].x;
          ai += yv[i].y;
        } else if (C.zinit) {                     // y = A x - b z (+ c z2): the first pass carries the start vectors
          const c128 zv = C.zinit[lbase + r];
          ar = fma(-C.zscale, zv.x, ar);
          ai = fma(-C.zscale, zv.y, ai);
          if (C.zinit2) {
            const c128 z2 = C.zinit2[lbase + r];
            ar = fma(C.z2re, z2.x, ar);
            ar = fma(-C.z2im, z2.y, ar);
            ai = fma(C.z2re, z2.y, ai);
            ai = fma(C.z2im, z2.x, ai);
          }
        }
        if (ACC && C.dot_out) {                   // <x, y> and |y|^2 of the finished rows (the row of x is in LDS)
          const c128 xo = xs[r];
          dr = fma(xo.x, ar, dr);
          dr = fma(xo.y, ai, dr);
          di = fma(xo.x, ai, di);
          di = fma(-xo.y, ar, di);
          dn = fma(ar, ar, dn);
          dn = fma(ai, ai, dn);
        }
      }
      store_nt(y + lbase + r, ar, ai);
    }
  }
  if (ACC && C.dot_out) {
    dr = wave_sum(dr); di = wave_sum(di); dn = wave_sum(dn);
    if (lane == 0) {
      red[3 * (threadIdx.x >> 6)] = dr;
      red[3 * (threadIdx.x >> 6) + 1] = di;
      red[3 * (threadIdx.x >> 6) + 2] = dn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double sr = 0.0, si = 0.0, sn = 0.0;
      for (int wv = 0; wv < NT / 64; ++wv) { sr += red[3 * wv]; si += red[3 * wv + 1]; sn += red[3 * wv + 2]; }
      C.dot_out[3 * (size_t)blockIdx.x] = sr;
      C.dot_out[3 * (size_t)blockIdx.x + 1] = si;
      C.dot_out[3 * (size_t)blockIdx.x + 2] = sn;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// lo pass on REAL vectors (DNM_MAT_REAL_PACKED on a SpinConserve pair, round 4): x and y are arrays of doubles in the
// same positions of the layout.  A thread owns PAIRS of adjacent row entries (2q, 2q + 1) -- rows start at multiples of
// 8 entries, so a pair is one aligned 16-byte access -- and twice as many entries as the complex pass (the same 64 KB
// tile holds 8192 doubles: two rows of 3432 states per workgroup, four of 2002 ...); the tile in LDS is an array of
// doubles, so the bonds inside Lo (partner r +- d, d of either parity) read 8 bytes.  Real operators have equal `up`
// and `dn` elements (Hermitian and real), so there is only the SYM form.  Everything per row -- sub-groups, the bond
// table in the lanes, the on-the-fly diagonal -- is as in sc3_lo_pass.
template <int A, int NT, int PPT, int DIAGM, bool ACC>
__global__ void __launch_bounds__(NT, sc3_win_waves(NT, (NT * 2 * PPT * 8 + 1023) / 1024 + 1))
sc3_lo_pass_r(const Sc3Tab S, const Sc3Op O, const uint32_t *__restrict__ perm, const Sc3Call C,
              const double *__restrict__ xw, double *__restrict__ y) {
  constexpr int MAXROWS = cbinom(A, A / 2);
  constexpr int EPT = 2 * PPT;                          // entries per thread (PPT pairs)
  static_assert(NT * EPT >= MAXROWS, "the longest row does not fit the workgroup");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int32_t cl[A * (A + 1)];
  __shared__ double red[3 * (NT / 64)];
  __shared__ double dsh[5 * 8];
  const uint32_t e0 = SC3_CP(uint32_t, perm)[8 * (size_t)blockIdx.x];
  if (e0 == 0xffffffffu) return;
  const int lane = threadIdx.x & 63;
  const int w = S.w;
  const int logm = (int)(e0 >> 30);
  const int NTS = NT >> logm;
  const int sub = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) >> (ilog2c(NT) - 6 - logm);
  const int tsub = (int)threadIdx.x & (NTS - 1);
  const uint32_t e = SC3_CP(uint32_t, perm)[8 * (size_t)blockIdx.x + sub];
  const bool has_row = !(e & SC3_NOROW);
  double *xs = reinterpret_cast<double *>(smem) + (size_t)sub * ((NT * EPT) >> logm);
  const RowId R = decode_row(has_row ? (e & (SC3_NOROW - 1u)) : (e0 & (SC3_NOROW - 1u)), S);
  const uint32_t T = R.T, W = R.W;
  const int cw = R.cw, kr = R.kr, kl = R.kl, nrows = has_row ? R.nrows : 0, p = has_row ? R.pitch : 0;
  const int64_t tb = R.tb, base = R.base;
  const double *__restrict__ x = xw - C.win_start;
  const int64_t lbase = base - C.row0;
  // entry i of this thread: pair i >> 1, lane i & 1
#define SC3R_ENT(i) (2 * (tsub + ((i) >> 1) * NTS) + ((i) & 1))
  // where entry r of the row sits in the LDS slice.  The lanes of a wavefront read entries two apart (their own lane
  // of consecutive pairs, shifted by the bond's offset): two lanes per bank.  -DDNM_SC3R_DEINT=1 stores even entries
  // in the first half of the slice and odd ones in the second, which removes the conflicts -- and measured SLOWER
  // (5.11 against 4.45 ms at SpinConserve(32,16): the index arithmetic and 12-16 B/lane of spills cost more than the
  // conflicts; gpurun_out/r04_s16) -- so the interleaved form is the default
#ifndef DNM_SC3R_DEINT
#define DNM_SC3R_DEINT 0
#endif
#if DNM_SC3R_DEINT
  const int half = (NT * EPT >> logm) >> 1;
#define SC3R_LDS(r) (((r) >> 1) + (((r) & 1) ? half : 0))
#else
#define SC3R_LDS(r) (r)
#endif

  SC3_PRIO_MEM();
  uint32_t lowp[PPT];                                   // the Lo patterns of a pair's entries, 16 bits each
#define SC3R_PAT(i) ((lowp[(i) >> 1] >> (((i) & 1) * 16)) & 0xffffu)
  double xv[EPT];
  const auto pat = SC3_CP(uint16_t, S.lo_pat) + S.lo_off[kl];
#pragma unroll
  for (int i = 0; i < EPT; i += 2) {
    const int r = SC3R_ENT(i);
    lowp[i >> 1] = 0;
    xv[i] = xv[i + 1] = 0.0;
    if (r < p) {                                        // (the padding of a row holds zeros)
      const d2v v = *reinterpret_cast<const d2v *>(x + base + r);
      xv[i] = v.x;
      xv[i + 1] = v.y;
      if (r < nrows) lowp[i >> 1] = pat[r];
      if (r + 1 < nrows) lowp[i >> 1] |= (uint32_t)pat[r + 1] << 16;
    }
  }
  int act = 0, r0 = 0, r1 = nrows;
  int64_t delta = 0;
  double c0 = 0.0;
  {
    const int b = A - 1 + lane;
    if (b < S.L - 1 && ((O.bondsA >> b) & 1ull)) {
      bool up = false;
      if (lane == 0) {
        const int cut = SC3_CP(int32_t, S.cbin)[(A - 1) * 17 + kl];
        if (W & 1u) {
          if (cut > 0) {
            act = 1; r0 = 0; r1 = cut; up = false;
            delta = tb + SC3_CP(int64_t, S.icoff)[kr * (w + 1) + cw - 1] + (int64_t)SC3_CP(uint16_t, S.w_rank)[W & ~1u] * S.pitch[kl + 1] +
                    SC3_CP(int32_t, S.cbin)[(A - 1) * 17 + kl + 1] - base;
          }
        } else if (cut < nrows) {
          act = 1; r0 = cut; r1 = nrows; up = true;
          delta = tb + SC3_CP(int64_t, S.icoff)[kr * (w + 1) + cw + 1] + (int64_t)SC3_CP(uint16_t, S.w_rank)[W | 1u] * S.pitch[kl - 1] - cut - base;
        }
      } else if (lane < w) {
        const int bw = lane - 1;
        const uint32_t pair = (W >> bw) & 3u;
        if (pair == 1u || pair == 2u) {
          act = 1; up = pair == 1u;
          delta = ((int64_t)SC3_CP(uint16_t, S.w_rank)[W ^ (3u << bw)] - (int64_t)SC3_CP(uint16_t, S.w_rank)[W]) * p;
        }
      } else if (lane == w) {
        const uint32_t pair = ((W >> (w - 1)) & 1u) | ((T & 1u) << 1);
        if (pair == 1u) {
          act = 1; up = true;
          delta = SC3_CP(int64_t, S.ibase)[T | 1u] + SC3_CP(int64_t, S.icoff)[(kr - 1) * (w + 1) + cw - 1] +
                  (int64_t)SC3_CP(uint16_t, S.w_rank)[W & ~(1u << (w - 1))] * p - base;
        } else if (pair == 2u) {
          act = 1; up = false;
          delta = SC3_CP(int64_t, S.ibase)[T & ~1u] + SC3_CP(int64_t, S.icoff)[(kr + 1) * (w + 1) + cw + 1] +
                  (int64_t)SC3_CP(uint16_t, S.w_rank)[W | (1u << (w - 1))] * p - base;
        }
      } else {
        const int bt = lane - w - 1;
        const uint32_t pair = (T >> bt) & 3u;
        if (pair == 1u || pair == 2u) {
          act = 1; up = pair == 1u;
          delta = SC3_CP(int64_t, S.ibase)[T ^ (3u << bt)] - tb;
        }
      }
      if (act) c0 = SC3_CP(double, O.bond)[4 * b + (up ? 0 : 2)];
    }
  }
  uint64_t hb = has_row ? __ballot(act) : 0ull;

  for (int tt = threadIdx.x; tt < A * (A + 1); tt += NT) {
    const int lo = tt / (A + 1), o = tt % (A + 1);
    cl[tt] = SC3_CP(int32_t, S.cbin)[lo * 17 + o];
  }
  if (DIAGM == 2 && tsub < 64) {
    const uint64_t hi = ((uint64_t)T << w) | W;
    double v0 = 0.0, vm[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < O.ndt; t0 += 64) {
      const int t = t0 + lane;
      if (t < O.ndt) {
        const uint64_t sg = SC3_CP(uint64_t, O.dt_sign)[t];
        const double c = flip(SC3_CP(double, O.dt_coef)[t], (uint32_t)__popcll(hi & sg & 0x1fffffffffffffffull) & 1u);
        const int g = (int)(sg >> 61);
        if (g == 0) v0 += c;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (g == j + 1) vm[j] += c;
      }
    }
    v0 = wave_sum(v0);
    if (lane == 0) dsh[5 * sub] = v0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < O.ngroups) {
        const double s = wave_sum(vm[j]);
        if (lane == 0) dsh[5 * sub + j + 1] = s;
      }
  }
  double acc[EPT];
#pragma unroll
  for (int i = 0; i < EPT; i += 2) {
    const int r = SC3R_ENT(i);
    acc[i] = acc[i + 1] = 0.0;
    if (r < p) {
#if DNM_SC3R_DEINT
      xs[r >> 1] = xv[i];
      xs[half + (r >> 1)] = xv[i + 1];
#else
      *reinterpret_cast<d2v *>(xs + r) = d2v{xv[i], xv[i + 1]};
#endif
      if (DIAGM == 1) {
        const d2v dg = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(O.diag + lbase + r));
        acc[i] = dg.x * xv[i];
        acc[i + 1] = dg.y * xv[i + 1];
      }
    }
  }
  while (hb) {
    const int m = __ffsll((long long)hb) - 1;
    hb &= hb - 1;
    const int64_t dl_ = rl_i64(delta, m);
    const double *__restrict__ pp = x + (base + dl_);
    const double cr = rl_f64(c0, m);
    const int q0 = rl_i32(r0, m), q1 = rl_i32(r1, m);
    double v[EPT];
    if (!(dl_ & 1)) {                 // whole elements line up (every bond but, mostly, the Lo/W boundary)
#pragma unroll
      for (int i = 0; i < EPT; i += 2) {
        const int r = SC3R_ENT(i);
        v[i] = v[i + 1] = 0.0;
        if (r >= q0 && r + 1 < q1) {                // the whole pair lies in [q0, q1): one 16-byte load
          const d2v t = *reinterpret_cast<const d2v *>(pp + r);
          v[i] = t.x;
          v[i + 1] = t.y;
        } else {                                    // a pair that straddles an end of the range
          if (r >= q0 && r < q1) v[i] = pp[r];
          if (r + 1 >= q0 && r + 1 < q1) v[i + 1] = pp[r + 1];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const int r = SC3R_ENT(i);
        v[i] = 0.0;
        if (r >= q0 && r < q1) v[i] = pp[r];
      }
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i) acc[i] = fma(cr, v[i], acc[i]);
  }
  d2v yv[PPT];
  if (ACC) {
#pragma unroll
    for (int i = 0; i < EPT; i += 2) {
      const int r = SC3R_ENT(i);
      yv[i >> 1] = d2v{0.0, 0.0};
      if (r < p) yv[i >> 1] = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(y + lbase + r));
    }
  }
  __syncthreads();
  SC3_PRIO_LDS();
  if (DIAGM == 2) {
    // (the Lo-only part of the diagonal comes from its L2-resident table here, not before the barrier as in the
    // complex pass: eight entries per thread leave no registers to carry it across)
    const auto dl = SC3_CP(double, O.dlo) + S.lo_off[kl];
    const double dg0 = dsh[5 * sub];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int r = SC3R_ENT(i);
      if (r < nrows) {
        double dg = dl[r] + dg0;
        for (int j = 0; j < O.ngroups; ++j) dg += flip(dsh[5 * sub + j + 1], (uint32_t)__popc(SC3R_PAT(i) & O.glo[j]) & 1u);
        acc[i] = fma(dg, xs[SC3R_LDS(r)], acc[i]);
      }
    }
  }
  for (int lo = 0; lo < A - 1; ++lo) {
    if (!((O.present >> lo) & 1ull)) continue;
    const double ure = SC3_CP(double, O.bond)[4 * lo];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int r = SC3R_ENT(i);
      const uint32_t pt = SC3R_PAT(i);
      const uint32_t pair = (pt >> lo) & 3u;
      if (r < nrows && (pair == 1u || pair == 2u)) {
        const int ord0 = __popc(pt & ((1u << lo) - 1u));
        const int d = cl[lo * (A + 1) + ord0];
        const int rp = pair == 1u ? r + d : r - d;
        acc[i] = fma(ure, xs[SC3R_LDS(rp)], acc[i]);
      }
    }
  }
  double dr = 0.0, dn = 0.0;
  SC3_PRIO_MEM();
#pragma unroll
  for (int i = 0; i < EPT; i += 2) {
    const int r = SC3R_ENT(i);
    if (r < p) {                                  // the padding of a row is written too (zeros)
      double a2[2] = {acc[i], acc[i + 1]};
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (r + b < nrows) {
          if (ACC) a2[b] += b ? yv[i >> 1].y : yv[i >> 1].x;
          else if (C.zinit) {
            a2[b] = fma(-C.zscale, reinterpret_cast<const double *>(C.zinit)[lbase + r + b], a2[b]);
            if (C.zinit2) a2[b] = fma(C.z2re, reinterpret_cast<const double *>(C.zinit2)[lbase + r + b], a2[b]);
          }
          if (ACC && C.dot_out) {
            dr = fma(xs[SC3R_LDS(r + b)], a2[b], dr);
            dn = fma(a2[b], a2[b], dn);
          }
        } else {
          a2[b] = 0.0;
        }
      }
      __builtin_nontemporal_store(d2v{a2[0], a2[1]}, reinterpret_cast<d2v *>(y + lbase + r));
    }
  }
#undef SC3R_ENT
#undef SC3R_PAT
#undef SC3R_LDS
  if (ACC && C.dot_out) {
    dr = wave_sum(dr); dn = wave_sum(dn);
    if (lane == 0) {
      red[3 * (threadIdx.x >> 6)] = dr;
      red[3 * (threadIdx.x >> 6) + 1] = 0.0;
      red[3 * (threadIdx.x >> 6) + 2] = dn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double sr = 0.0, sn = 0.0;
      for (int wv = 0; wv < NT / 64; ++wv) { sr += red[3 * wv]; sn += red[3 * wv + 2]; }
      C.dot_out[3 * (size_t)blockIdx.x] = sr;
      C.dot_out[3 * (size_t)blockIdx.x + 1] = 0.0;
      C.dot_out[3 * (size_t)blockIdx.x + 2] = sn;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// window pass (the first pass: writes y): one workgroup per (T, cw, run of R = 16 << s columns): all window
// patterns of the class x R columns in LDS; the accumulators start from -zscale * zinit + z2 * zinit2 if given.
// (512 threads x 8 entries against 1024 x 4: 5.40 against 5.75 ms at SpinConserve(32,16), level on a rank of config 5,
// profiles/r03_exp12_sc3_win512.txt.  Two gathered bonds in flight at a time -- half the round trips of a workgroup's
// life, 12 of them on a rank of config 5 -- do not fit: the compiler needs 12-13 registers per entry where 8 are live,
// and the spills cost more than the round trips: 22 ms.)
template <int WB, int NT, bool SYM, bool ACC>
__global__ void __launch_bounds__(NT, sc3_win_waves(NT, (cbinom(WB, WB / 2) * 16 * 16 + 1023) / 1024 + 1))
sc3_win_pass(const Sc3Tab S, const Sc3Op O, const uint32_t *__restrict__ perm, const Sc3Call C,
             const c128 *__restrict__ xw, c128 *__restrict__ y) {
  constexpr int MAXE = cbinom(WB, WB / 2) * 16;
  constexpr int RPT = (MAXE + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  c128 *xs = reinterpret_cast<c128 *>(smem);       // the tile [wr][column], then one zero row (wr = nwp)
  const uint32_t e = SC3_CP(uint32_t, perm)[blockIdx.x];
  if (e == 0xffffffffu) return;
  const int lane = threadIdx.x & 63;
  const uint32_t T = e >> 16;
  const int cw = (e >> 12) & 15, run = e & 0xfff;
  const int kr = S.k - __popc(T), kl = kr - cw;
  const int nwp = S.nw[cw], p = S.pitch[kl];
  const int sh = 4 + S.rs[cw];
  const int lr0 = run << sh;
  const int ncols = min(1 << sh, p - lr0);
  const int64_t tb = SC3_CP(int64_t, S.ibase)[T];
  const int64_t own = tb + SC3_CP(int64_t, S.icoff)[kr * (WB + 1) + cw];
  const int64_t cbase = own + lr0;
  const int64_t lcb = cbase - C.row0;
  const int nent = nwp << sh;
  const c128 *__restrict__ x = xw - C.win_start;

  SC3_PRIO_MEM();
  uint32_t wpat[RPT];
  int32_t off[RPT];          // offset of the entry from cbase, -1: not an entry
  c128 xv[RPT];
  const auto pat = SC3_CP(uint16_t, S.w_pat) + S.w_off[cw];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int en = threadIdx.x + i * NT;
    wpat[i] = 0;
    off[i] = -1;
    xv[i] = make_double2(0.0, 0.0);
    if (en < nent) {
      const int wrr = en >> sh, j = en & ((1 << sh) - 1);
      wpat[i] = pat[wrr] | ((uint32_t)wrr << 16);
      if (j < ncols) {
        off[i] = wrr * p + j;
        xv[i] = x[cbase + off[i]];
      }
    }
  }
  // gathered bonds, one per lane: l = 0 the W/T boundary, above inside T
  int act = 0, r0 = 0, r1 = nwp;
  int64_t delta = 0;
  double c0 = 0.0, c1 = 0.0;
  {
    const int b = S.a + WB - 1 + lane;
    if (b < S.L - 1 && ((O.bondsB >> b) & 1ull)) {
      bool up = false;
      if (lane == 0) {
        const int cut = SC3_CP(int32_t, S.cbin)[(WB - 1) * 17 + cw];                // rows below: top bit of W clear
        if (T & 1u) {                                              // the one comes down into W
          if (cut > 0) {
            act = 1; r0 = 0; r1 = cut; up = false;
            delta = SC3_CP(int64_t, S.ibase)[T & ~1u] + SC3_CP(int64_t, S.icoff)[(kr + 1) * (WB + 1) + cw + 1] +
                    (int64_t)SC3_CP(int32_t, S.cbin)[(WB - 1) * 17 + cw + 1] * p - own;
          }
        } else if (cut < nwp) {                                    // the one goes up into T
          act = 1; r0 = cut; r1 = nwp; up = true;
          delta = SC3_CP(int64_t, S.ibase)[T | 1u] + SC3_CP(int64_t, S.icoff)[(kr - 1) * (WB + 1) + cw - 1] - (int64_t)cut * p - own;
        }
      } else {
        const int bt = lane - 1;
        const uint32_t pair = (T >> bt) & 3u;
        if (pair == 1u || pair == 2u) {
          act = 1; up = pair == 1u;
          delta = SC3_CP(int64_t, S.ibase)[T ^ (3u << bt)] - tb;
        }
      }
      if (act) {
        c0 = SC3_CP(double, O.bond)[4 * b + (up ? 0 : 2)];
        c1 = SC3_CP(double, O.bond)[4 * b + (up ? 1 : 3)];
      }
    }
  }
  uint64_t hb = __ballot(act);
  for (int j = threadIdx.x; j < (1 << sh); j += NT) xs[nent + j] = make_double2(0.0, 0.0);       // the zero row
  // the class's partner table (Sc3Tab::w_nb, 16 bytes per row) behind it: read back from LDS after the barrier
  ulonglong2 *wtab = reinterpret_cast<ulonglong2 *>(xs + nent + (1 << sh));
  for (int j = threadIdx.x; j < nwp; j += NT)
    wtab[j] = reinterpret_cast<const ulonglong2 *>(S.w_nb + (size_t)2 * S.w_off[cw])[j];
  double accr[RPT], acci[RPT];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int en = threadIdx.x + i * NT;
    accr[i] = 0.0;
    acci[i] = 0.0;
    if (en < nent) {
      xs[en] = xv[i];
      if (!ACC && C.zinit && off[i] >= 0) {        // y = A x - b z (+ c z2): the start vectors open the accumulators
        const c128 zv = C.zinit[lcb + off[i]];
        accr[i] = -C.zscale * zv.x;
        acci[i] = -C.zscale * zv.y;
        if (C.zinit2) {
          const c128 z2 = C.zinit2[lcb + off[i]];
          accr[i] = fma(C.z2re, z2.x, accr[i]);
          accr[i] = fma(-C.z2im, z2.y, accr[i]);
          acci[i] = fma(C.z2re, z2.y, acci[i]);
          acci[i] = fma(C.z2im, z2.x, acci[i]);
        }
      }
    }
  }
  while (hb) {
    const int m = __ffsll((long long)hb) - 1;
    hb &= hb - 1;
    const c128 *__restrict__ pp = x + (cbase + rl_i64(delta, m));
    const double cr = rl_f64(c0, m), ci = rl_f64(c1, m);
    const int q0 = rl_i32(r0, m), q1 = rl_i32(r1, m);
    c128 v[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int wrr = (int)(wpat[i] >> 16);
      v[i] = make_double2(0.0, 0.0);
      if (off[i] >= 0 && wrr >= q0 && wrr < q1) v[i] = pp[off[i]];
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      accr[i] = fma(cr, v[i].x, accr[i]);
      acci[i] = fma(cr, v[i].y, acci[i]);
      if (!SYM) {
        accr[i] = fma(-ci, v[i].y, accr[i]);
        acci[i] = fma(ci, v[i].x, acci[i]);
      }
    }
  }
  __syncthreads();
  SC3_PRIO_LDS();
  // bonds inside W: the partner row of (row, bond) from the layout's table (Sc3Tab::w_nb) -- a row whose two spins are
  // equal points at the zero row behind the tile, so the loop has no branches
  {
    uint64_t t0[RPT], t1[RPT];
    uint32_t col[RPT];
    const uint64_t zr = (uint64_t)nwp * 0x0101010101010101ull;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int en = threadIdx.x + i * NT;
      const int wrr = (int)(wpat[i] >> 16);
      col[i] = (uint32_t)en & ((1u << sh) - 1u);
      t0[i] = zr;
      t1[i] = zr;
      if (en < nent) {
        const ulonglong2 tw = wtab[wrr];
        t0[i] = tw.x;
        if (WB - 1 > 8) t1[i] = tw.y;
      }
    }
#pragma unroll
    for (int lo = 0; lo < WB - 1; ++lo) {
      const int b = S.a + lo;
      if (!((O.present >> b) & 1ull)) continue;
      const double ure = SC3_CP(double, O.bond)[4 * b], uim = SC3_CP(double, O.bond)[4 * b + 1], dre = SC3_CP(double, O.bond)[4 * b + 2], dim_ = SC3_CP(double, O.bond)[4 * b + 3];
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const uint32_t pr = (uint32_t)((lo < 8 ? t0[i] : t1[i]) >> (8 * (lo & 7))) & 0xffu;
        const c128 xp = xs[(pr << sh) + col[i]];
        if (SYM) {
          accr[i] = fma(ure, xp.x, accr[i]);
          acci[i] = fma(ure, xp.y, acci[i]);
        } else {
          const bool up = (wpat[i] >> lo) & 1u;
          const double cre = up ? ure : dre, cim = up ? uim : dim_;
          accr[i] = fma(cre, xp.x, accr[i]);
          acci[i] = fma(cre, xp.y, acci[i]);
          accr[i] = fma(-cim, xp.y, accr[i]);
          acci[i] = fma(cim, xp.x, acci[i]);
        }
      }
    }
  }
  SC3_PRIO_MEM();
#pragma unroll
  for (int i = 0; i < RPT; ++i)
    if (off[i] >= 0) {
      double ar = accr[i], ai = acci[i];
      if (ACC) {
        const c128 yo = load_nt(y + lcb + off[i]);
        ar += yo.x;
        ai += yo.y;
      }
      store_nt(y + lcb + off[i], ar, ai);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Row kernel: any operator between SpinConserve(L,k) and itself in the internal layout.  One workgroup per row
// (T, W); a state's position is three table lookups (sc3_pos), so a column costs no unranking.  The matrix element
// follows bpetsc_template_2.c:396-405 (sign on the column state, TERM_REAL decides real / imaginary).
constexpr int SC3_ROW_NT = 256;
__global__ void __launch_bounds__(SC3_ROW_NT)
sc3_row_kernel(const Sc3Tab S, const DevMsc msc, const uint32_t *__restrict__ rows, const Sc3Call C,
               const double *__restrict__ diag, const c128 *__restrict__ xw, c128 *__restrict__ y) {
  const uint32_t e = rows[blockIdx.x];
  if (e == 0xffffffffu) return;
  const RowId R = decode_row(e, S);
  const c128 *__restrict__ x = xw - C.win_start;
  const int64_t lbase = R.base - C.row0;
  const uint64_t hi = (((uint64_t)R.T << S.w) | R.W) << S.a;
  const uint16_t *__restrict__ pat = S.lo_pat + S.lo_off[R.kl];
  for (int r = threadIdx.x; r < R.pitch; r += SC3_ROW_NT) {
    double accr = 0.0, acci = 0.0;
    if (r < R.nrows) {
      const uint64_t ket = hi | pat[r];
      if (C.zinit) {
        const c128 zv = C.zinit[lbase + r];
        accr = -C.zscale * zv.x;
        acci = -C.zscale * zv.y;
        if (C.zinit2) {
          const c128 z2 = C.zinit2[lbase + r];
          accr = fma(C.z2re, z2.x, accr);
          accr = fma(-C.z2im, z2.y, accr);
          acci = fma(C.z2re, z2.y, acci);
          acci = fma(C.z2im, z2.x, acci);
        }
      }
      int m0 = 0;
      if (diag) {
        const c128 xo = x[R.base + r];
        const double dg = diag[lbase + r];
        accr = fma(dg, xo.x, accr);
        acci = fma(dg, xo.y, acci);
        m0 = 1;
      }
      for (int m = m0; m < msc.nmasks; ++m) {
        const uint64_t mask = (uint64_t)msc.masks[m];
        const uint64_t bra = ket ^ mask;
        if (__popcll(bra) != S.k) continue;               // leaves the subspace: no such column
        double cre = 0.0, cim = 0.0;
        for (int64_t t = msc.mask_offsets[m]; t < msc.mask_offsets[m + 1]; ++t) {
          const uint64_t sg = (uint64_t)msc.signs[t];
          const double c = flip(msc.real_coeffs[t], (uint32_t)__popcll(bra & sg) & 1u);
          if (__popcll(mask & sg) & 1) cim += c; else cre += c;   // TERM_REAL (bpetsc_impl.h:34)
        }
        const c128 xv = x[sc3_pos(bra, S)];
        accr = fma(cre, xv.x, accr);
        acci = fma(cre, xv.y, acci);
        accr = fma(-cim, xv.y, accr);
        acci = fma(cim, xv.x, acci);
      }
    }
    store_nt(y + lbase + r, accr, acci);
  }
}

// ---------------------------------------------------------------------------------------------------------
// layout utilities: one workgroup per row (T, W)
template <typename V>
__global__ void __launch_bounds__(256)
sc3_copy_kernel(const Sc3Tab S, const uint32_t *__restrict__ rows, V *__restrict__ dst, const V *__restrict__ src,
                int to_internal, int64_t ioff, int64_t noff) {
  // ioff / noff: where the (partitioned) vectors start in the internal layout / the reference order
  const uint32_t e = rows[blockIdx.x];
  const RowId R = decode_row(e, S);
  const int64_t nat = S.nbase[R.T] + S.ncoff[(int64_t)R.kr * ((int64_t)1 << S.w) + R.W] - noff;
  const int64_t base = R.base - ioff;
  V zero{};
  for (int r = threadIdx.x; r < R.pitch; r += 256) {
    if (to_internal) dst[base + r] = r < R.nrows ? src[nat + r] : zero;
    else if (r < R.nrows) dst[nat + r] = src[base + r];
  }
}
__global__ void __launch_bounds__(64)
sc3_zero_pad_kernel(const Sc3Tab S, const uint32_t *__restrict__ rows, c128 *__restrict__ x, int64_t ioff) {
  const RowId R = decode_row(rows[blockIdx.x], S);
  for (int r = R.nrows + threadIdx.x; r < R.pitch; r += 64) x[R.base - ioff + r] = make_double2(0.0, 0.0);
}
__global__ void __launch_bounds__(256)
sc3_random_kernel(const Sc3Tab S, const uint32_t *__restrict__ rows, c128 *__restrict__ x, uint64_t seed, int64_t ioff) {
  const RowId R = decode_row(rows[blockIdx.x], S);
  const int64_t nat = S.nbase[R.T] + S.ncoff[(int64_t)R.kr * ((int64_t)1 << S.w) + R.W];
  for (int r = threadIdx.x; r < R.pitch; r += 256)
    x[R.base - ioff + r] = r < R.nrows ? philox_normal((uint64_t)(nat + r), seed) : make_double2(0.0, 0.0);
}
__global__ void __launch_bounds__(256)
sc3_random_real_kernel(const Sc3Tab S, const uint32_t *__restrict__ rows, double *__restrict__ x, uint64_t seed, int64_t ioff) {
  const RowId R = decode_row(rows[blockIdx.x], S);
  const int64_t nat = S.nbase[R.T] + S.ncoff[(int64_t)R.kr * ((int64_t)1 << S.w) + R.W];
  for (int r = threadIdx.x; r < R.pitch; r += 256)
    x[R.base - ioff + r] = r < R.nrows ? philox_normal((uint64_t)(nat + r), seed).x : 0.0;
}
__global__ void __launch_bounds__(256) sc3_unpack_real_kernel(c128 *__restrict__ dst, const double *__restrict__ src, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dst[i] = make_double2(src[i], 0.0);
}
// reference index -> internal position: unrank (bsubspace_impl.h:210-228), then the tables
__global__ void __launch_bounds__(256)
sc3_positions_kernel(const Sc3Tab S, int64_t n, const int64_t *__restrict__ idx, int64_t *__restrict__ pos, int64_t ioff,
                     int64_t noff) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t *__restrict__ nck = S.nck;
  const int ld = S.L + 1;
  int64_t id = idx[i] + noff;
  uint64_t st = 0;
  int k = S.k;
  for (int b = S.L; b > 0; --b) {
    const int64_t here = (k > b - 1) ? 0 : nck[(int64_t)k * ld + (b - 1)];
    st <<= 1;
    if (id >= here) { id -= here; --k; st |= 1; }
  }
  pos[i] = sc3_pos(st, S) - ioff;
}

// ---- the same utilities under a site relabelling (Sc3Perm; one rank, whole vectors) -----------------------
// reference index of a state given in the layout's labelling: back to the reference's spins, then the colex rank
// (bsubspace_impl.h:191-208)
__device__ __forceinline__ int64_t ref_index_of(uint64_t s_ref, const Sc3Tab &S) {
  int64_t idx = 0;
  int j = 0;
  const int ld = S.L + 1;
  while (s_ref) {
    const int n = __ffsll((long long)s_ref) - 1;
    ++j;
    if (j <= n) idx += S.nck[(int64_t)j * ld + n];
    s_ref &= s_ref - 1;
  }
  return idx;
}
template <typename V>
__global__ void __launch_bounds__(256)
sc3_copy_perm_kernel(const Sc3Tab S, const Sc3Perm P, const uint32_t *__restrict__ rows, V *__restrict__ dst,
                     const V *__restrict__ src, int to_internal) {
  const RowId R = decode_row(rows[blockIdx.x], S);
  const uint64_t hi = sc3_permute((((uint64_t)R.T << S.w) | R.W) << S.a, P.to_ref, S.L);
  const uint16_t *__restrict__ pat = S.lo_pat + S.lo_off[R.kl];
  V zero{};
  for (int r = threadIdx.x; r < R.pitch; r += 256) {
    if (r < R.nrows) {
      const int64_t nat = ref_index_of(hi | sc3_permute(pat[r], P.to_ref, S.a), S);
      if (to_internal) dst[R.base + r] = src[nat];
      else dst[nat] = src[R.base + r];
    } else if (to_internal) {
      dst[R.base + r] = zero;
    }
  }
}
template <bool REAL>
__global__ void __launch_bounds__(256)
sc3_random_perm_kernel(const Sc3Tab S, const Sc3Perm P, const uint32_t *__restrict__ rows, void *__restrict__ xv, uint64_t seed) {
  const RowId R = decode_row(rows[blockIdx.x], S);
  const uint64_t hi = sc3_permute((((uint64_t)R.T << S.w) | R.W) << S.a, P.to_ref, S.L);
  const uint16_t *__restrict__ pat = S.lo_pat + S.lo_off[R.kl];
  for (int r = threadIdx.x; r < R.pitch; r += 256) {
    c128 v = make_double2(0.0, 0.0);
    if (r < R.nrows) v = philox_normal((uint64_t)ref_index_of(hi | sc3_permute(pat[r], P.to_ref, S.a), S), seed);
    if (REAL) reinterpret_cast<double *>(xv)[R.base + r] = v.x;
    else reinterpret_cast<c128 *>(xv)[R.base + r] = v;
  }
}
__global__ void __launch_bounds__(256)
sc3_positions_perm_kernel(const Sc3Tab S, const Sc3Perm P, int64_t n, const int64_t *__restrict__ idx, int64_t *__restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t *__restrict__ nck = S.nck;
  const int ld = S.L + 1;
  int64_t id = idx[i];
  uint64_t st = 0;
  int k = S.k;
  for (int b = S.L; b > 0; --b) {
    const int64_t here = (k > b - 1) ? 0 : nck[(int64_t)k * ld + (b - 1)];
    st <<= 1;
    if (id >= here) { id -= here; --k; st |= 1; }
  }
  pos[i] = sc3_pos(sc3_permute(st, P.to_int, S.L), S);
}

}  // namespace

// ===========================================================================================================
// host side: what launches (every table these launches read is built in sc3_tables.cpp)
// ===========================================================================================================
// ---- the layout's vector utilities --------------------------------------------------------------------------
int sc3_layout_copy(const Sc3Layout &Ly, void *dst, const void *src, bool to_internal, hipStream_t st, uint32_t T0, uint32_t T1,
                    const Sc3Perm *perm) {
  DNM_CHECK(Ly.on_device, "layout tables are not on the device");
  const RowRange r = row_range(Ly, T0, T1);
  if (!r.count) return 0;
  DNM_TRY(perm_whole(Ly, perm, r));
  DNM_TRY(ref_side(Ly, r));
  if (perm && perm->on) {
    hipLaunchKernelGGL(sc3_copy_perm_kernel<c128>, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev, *perm,
                       Ly.d_rows.as<uint32_t>(), (c128 *)dst, (const c128 *)src, to_internal ? 1 : 0);
    DNM_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(sc3_copy_kernel<c128>, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev,
                     Ly.d_rows.as<uint32_t>() + r.first, (c128 *)dst, (const c128 *)src, to_internal ? 1 : 0, r.ioff, r.noff);
  DNM_HIP(hipGetLastError());
  return 0;
}
int sc3_layout_copy_f64(const Sc3Layout &Ly, double *dst, const double *src, bool to_internal, hipStream_t st, uint32_t T0,
                        uint32_t T1, const Sc3Perm *perm) {
  DNM_CHECK(Ly.on_device, "layout tables are not on the device");
  const RowRange r = row_range(Ly, T0, T1);
  if (!r.count) return 0;
  DNM_TRY(perm_whole(Ly, perm, r));
  DNM_TRY(ref_side(Ly, r));
  if (perm && perm->on) {
    hipLaunchKernelGGL(sc3_copy_perm_kernel<double>, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev, *perm,
                       Ly.d_rows.as<uint32_t>(), dst, src, to_internal ? 1 : 0);
    DNM_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(sc3_copy_kernel<double>, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev,
                     Ly.d_rows.as<uint32_t>() + r.first, dst, src, to_internal ? 1 : 0, r.ioff, r.noff);
  DNM_HIP(hipGetLastError());
  return 0;
}
int sc3_zero_padding(const Sc3Layout &Ly, void *x, hipStream_t st, uint32_t T0, uint32_t T1) {
  DNM_CHECK(Ly.on_device, "layout tables are not on the device");
  const RowRange r = row_range(Ly, T0, T1);
  if (!r.count) return 0;
  hipLaunchKernelGGL(sc3_zero_pad_kernel, dim3((unsigned)r.count), dim3(64), 0, st, Ly.dev,
                     Ly.d_rows.as<uint32_t>() + r.first, (c128 *)x, r.ioff);
  DNM_HIP(hipGetLastError());
  return 0;
}
int sc3_random(const Sc3Layout &Ly, void *x, uint64_t seed, hipStream_t st, uint32_t T0, uint32_t T1, const Sc3Perm *perm) {
  DNM_CHECK(Ly.on_device, "layout tables are not on the device");
  const RowRange r = row_range(Ly, T0, T1);
  if (!r.count) return 0;
  DNM_TRY(perm_whole(Ly, perm, r));
  if (perm && perm->on) {
    hipLaunchKernelGGL(sc3_random_perm_kernel<false>, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev, *perm,
                       Ly.d_rows.as<uint32_t>(), x, seed);
    DNM_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(sc3_random_kernel, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev,
                     Ly.d_rows.as<uint32_t>() + r.first, (c128 *)x, seed, r.ioff);
  DNM_HIP(hipGetLastError());
  return 0;
}
int sc3_random_real(const Sc3Layout &Ly, double *x, uint64_t seed, hipStream_t st, uint32_t T0, uint32_t T1,
                    const Sc3Perm *perm) {
  DNM_CHECK(Ly.on_device, "layout tables are not on the device");
  const RowRange r = row_range(Ly, T0, T1);
  if (!r.count) return 0;
  DNM_TRY(perm_whole(Ly, perm, r));
  if (perm && perm->on) {
    hipLaunchKernelGGL(sc3_random_perm_kernel<true>, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev, *perm,
                       Ly.d_rows.as<uint32_t>(), (void *)x, seed);
    DNM_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(sc3_random_real_kernel, dim3((unsigned)r.count), dim3(256), 0, st, Ly.dev,
                     Ly.d_rows.as<uint32_t>() + r.first, x, seed, r.ioff);
  DNM_HIP(hipGetLastError());
  return 0;
}
int sc3_unpack_real(const Sc3Layout &Ly, void *dst, const double *src, hipStream_t st, uint32_t T0, uint32_t T1) {
  int64_t is, n, ns, nl;
  sc3_range(Ly, T0, T1, &is, &n, &ns, &nl);
  if (n <= 0) return 0;
  const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)1 << 22);
  hipLaunchKernelGGL(sc3_unpack_real_kernel, dim3(nb), dim3(256), 0, st, (c128 *)dst, src, n);
  DNM_HIP(hipGetLastError());
  return 0;
}
int sc3_positions(const Sc3Layout &Ly, int64_t n, const int64_t *idx, int64_t *pos, hipStream_t st, uint32_t T0, uint32_t T1,
                  const Sc3Perm *perm) {
  DNM_CHECK(Ly.on_device, "layout tables are not on the device");
  if (n <= 0) return 0;
  DNM_CHECK(n < ((int64_t)1 << 32), "more than 2^32 indices in one call (one thread each: a launch holds fewer)");
  const RowRange r = row_range(Ly, T0, T1);
  DNM_TRY(perm_whole(Ly, perm, r));
  DNM_TRY(ref_side(Ly, r));
  if (perm && perm->on) {
    hipLaunchKernelGGL(sc3_positions_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Ly.dev, *perm, n, idx, pos);
    DNM_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(sc3_positions_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Ly.dev, n, idx, pos, r.ioff,
                     r.noff);
  DNM_HIP(hipGetLastError());
  return 0;
}

// the chain family's instances and shapes for the launcher (sc3_launch.h)
template <int A, int W, int NTW>
static int launch_two_pass(const Sc3Mat &M, const Sc3Call &call, const double *cached_diag, const void *xw, void *y,
                           hipStream_t st, int phase) {
  constexpr int NT = sc3_lo_threads(A), NTR = sc3r_threads(NT), PPR = sc3r_pairs(A, NT);
  Sc3LaunchShape L;
  L.nt_lo = NT; L.nt_win = NTW; L.nt_lo_real = NTR;
  L.lds_lo = (size_t)sc3_lo_cap(A, NT) * 16;
  L.lds_lo_real = (size_t)sc3_lo_cap_r(A, NT) * 8;
  for (int cw = 0; cw <= W; ++cw)      // the window pass's tile and the class's partner table
    L.lds_win = std::max(L.lds_win, sc3_win_tile_bytes(M.ly->host, cw) + (size_t)M.ly->host.nw[cw] * 16);
  const bool lo_first = phase != 0;
  Sc3Kernels K;
  if (lo_first) K.win = M.sym ? sc3_win_pass<W, NTW, true, true> : sc3_win_pass<W, NTW, false, true>;
  else K.win = M.sym ? sc3_win_pass<W, NTW, true, false> : sc3_win_pass<W, NTW, false, false>;
  K.win_real = K.win;
  K.lo = DNM_SC3_PICK_LO(sc3_lo_pass, A, NT, M.diag_mode, M.sym, lo_first);
  K.lo_real = DNM_SC3_PICK_LO_REAL(sc3_lo_pass_r, A, NTR, PPR, M.diag_mode, lo_first);
  return sc3_launch_passes(M, K, L, call, cached_diag, xw, y, st, phase);
}

int launch_sc3(const Sc3Mat &M, const DevMsc &msc, const Sc3Call &call, const double *cached_diag, const void *xw,
               void *y, hipStream_t st, int phase) {
  DNM_CHECK(M.ly && M.ly->on_device, "layout tables are not on the device");
  DNM_CHECK(phase == 0 || (M.tiled && !call.dot_out), "internal: only the tiled passes split into a local and a remote part");
  if (M.tiled) {
    if (call.dot_out) DNM_HIP(hipMemsetAsync(call.dot_out, 0, sc3_dot_partials(M) * 3 * sizeof(double), st));
    if (M.graph) return launch_sc3g(M, call, cached_diag, xw, y, st, phase);
    if (M.ly->host.a == 14) {
      static const bool w1024 = [] { const char *e = knob("DNM_SC3_WIN_THREADS"); return e && atoi(e) == 1024; }();   // experiments
      if (w1024) return launch_two_pass<14, 10, 1024>(M, call, cached_diag, xw, y, st, phase);
      return launch_two_pass<14, 10, sc3_win_threads(14)>(M, call, cached_diag, xw, y, st, phase);
    }
    return launch_two_pass<6, 4, sc3_win_threads(6)>(M, call, cached_diag, xw, y, st, phase);
  }
  DNM_CHECK(!call.dot_out, "internal: the row kernel has no fused sums");
  if (M.rowsel.empty()) return 0;      // a rank that owns no rows
  hipLaunchKernelGGL(sc3_row_kernel, dim3((unsigned)M.rowsel.size()), dim3(SC3_ROW_NT), 0, st, M.ly->dev, msc,
                     M.d_rowsel.as<uint32_t>(), call, cached_diag, (const c128 *)xw, (c128 *)y);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
