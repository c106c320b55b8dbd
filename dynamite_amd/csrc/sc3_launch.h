// The launcher of the two tiled passes, shared by the chain kernels (sc3_kernels.hip) and the bond-graph kernels
// (sc3g_kernels.hip).  A family picks its kernel instances (Sc3Kernels) and states its LDS sizes and thread counts
// (Sc3LaunchShape); the order of the passes, what each is told per call and the real-vector form are the same for both.
#pragma once

#include <map>

#include "dnm_common.h"
#include "sc3_dev.h"

namespace dnm {

using sc3_kern_t = void (*)(const Sc3Tab, const Sc3Op, const uint32_t *, const Sc3Call, const c128 *, c128 *);
using sc3_kern_r = void (*)(const Sc3Tab, const Sc3Op, const uint32_t *, const Sc3Call, const double *, double *);

// the instances for one (diag_mode, sym, pass order): lo / win on complex vectors; on real vectors the lo pass has its
// own kernel on doubles and the window pass is a complex kernel run on the halved tables (pairs of entries as elements:
// every offset it forms is even) -- the chain family's ordinary one, the graph family's REALV instance
struct Sc3Kernels {
  sc3_kern_t lo = nullptr, win = nullptr, win_real = nullptr;
  sc3_kern_r lo_real = nullptr;
};
struct Sc3LaunchShape {
  size_t lds_lo = 0, lds_win = 0, lds_lo_real = 0;     // dynamic LDS of the three kernels
  int nt_lo = 0, nt_win = 0, nt_lo_real = 0;           // their threads
};

// the instances of a lo-pass kernel template over diag_mode x sym x pass order (ACC false: it runs first)
#define DNM_SC3_PICK_LO(KERNEL, A, NT, dm, sym, lo_first)                                                         \
  [&]() -> sc3_kern_t {                                                                                           \
    switch ((dm) * 2 + ((sym) ? 1 : 0)) {                                                                         \
      case 0: return (lo_first) ? (sc3_kern_t)KERNEL<A, NT, 0, false, false> : (sc3_kern_t)KERNEL<A, NT, 0, false, true>; \
      case 1: return (lo_first) ? (sc3_kern_t)KERNEL<A, NT, 0, true, false> : (sc3_kern_t)KERNEL<A, NT, 0, true, true>;   \
      case 2: return (lo_first) ? (sc3_kern_t)KERNEL<A, NT, 1, false, false> : (sc3_kern_t)KERNEL<A, NT, 1, false, true>; \
      case 3: return (lo_first) ? (sc3_kern_t)KERNEL<A, NT, 1, true, false> : (sc3_kern_t)KERNEL<A, NT, 1, true, true>;   \
      case 4: return (lo_first) ? (sc3_kern_t)KERNEL<A, NT, 2, false, false> : (sc3_kern_t)KERNEL<A, NT, 2, false, true>; \
      default: return (lo_first) ? (sc3_kern_t)KERNEL<A, NT, 2, true, false> : (sc3_kern_t)KERNEL<A, NT, 2, true, true>;  \
    }                                                                                                             \
  }()
#define DNM_SC3_PICK_LO_REAL(KERNEL, A, NTR, PPR, dm, lo_first)                                                   \
  ((dm) == 0 ? ((lo_first) ? (sc3_kern_r)KERNEL<A, NTR, PPR, 0, false> : (sc3_kern_r)KERNEL<A, NTR, PPR, 0, true>)  \
   : (dm) == 1 ? ((lo_first) ? (sc3_kern_r)KERNEL<A, NTR, PPR, 1, false> : (sc3_kern_r)KERNEL<A, NTR, PPR, 1, true>) \
               : ((lo_first) ? (sc3_kern_r)KERNEL<A, NTR, PPR, 2, false> : (sc3_kern_r)KERNEL<A, NTR, PPR, 2, true>))

// LDS of the window pass without the family's partner table: the class's tile plus its zero row
static inline size_t sc3_win_tile_bytes(const Sc3Tab &S, int cw) { return ((size_t)S.nw[cw] + 1) << (4 + S.rs[cw] + 4); }

// phase 0: the whole multiply (window pass writes y, lo pass adds: one rank); phase 1: the part that needs nothing
// from other ranks (lo pass, writes y); phase 2: the rest (window pass, adds).  K: the instances for this phase's order.
static int sc3_launch_passes(const Sc3Mat &M, const Sc3Kernels &K, const Sc3LaunchShape &L, const Sc3Call &call,
                             const double *cached_diag, const void *xw, void *y, hipStream_t st, int phase) {
  Sc3Op op = M.op;
  const int dm = M.diag_mode;       // 2: on the fly whether or not a cached copy exists (8 B/row less to read)
  if (dm == 1) op.diag = cached_diag;
  DNM_CHECK(dm != 1 || op.diag, "this operator needs its diagonal precomputed (dnm_mat_precompute_diagonal)");
  DNM_CHECK(!M.real || M.sym, "internal: real vectors need a real operator");
  const void *klo = M.real ? (const void *)K.lo_real : (const void *)K.lo;
  const sc3_kern_t kwin = M.real ? K.win_real : K.win;
  const size_t lds_lo = M.real ? L.lds_lo_real : L.lds_lo;
  // the largest dynamic LDS each kernel has been allowed so far (the window pass's depends on the operator)
  static std::map<const void *, size_t> attr_done;
  for (auto kp : {std::make_pair(klo, lds_lo), std::make_pair((const void *)kwin, L.lds_win)})
    if (attr_done[kp.first] < kp.second) {
      DNM_HIP(hipFuncSetAttribute(kp.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kp.second));
      attr_done[kp.first] = kp.second;
    }
  // the pass that runs first starts y from the solver's start vectors, the one that runs last takes the fused sums
  Sc3Call first = call, second = call;
  first.dot_out = nullptr;
  second.zinit = nullptr;
  second.zinit2 = nullptr;
  const dim3 grid_win((unsigned)M.permB.size()), grid_lo((unsigned)(M.permA.size() / 8));
  const uint32_t *permA = M.d_permA.as<uint32_t>(), *permB = M.d_permB.as<uint32_t>();
  if (phase == 0 || phase == 2) {
    Sc3Call cw = phase == 0 ? first : second;
    if (M.real) {
      cw.row0 /= 2;
      cw.win_start /= 2;
    }
    hipLaunchKernelGGL(kwin, grid_win, dim3(L.nt_win), L.lds_win, st, M.real ? M.ly->dev_h : M.ly->dev, op, permB, cw,
                       (const c128 *)xw, (c128 *)y);
  }
  if (phase == 0 || phase == 1) {
    const Sc3Call &cl = phase == 0 ? second : first;
    if (M.real)
      hipLaunchKernelGGL(K.lo_real, grid_lo, dim3(L.nt_lo_real), lds_lo, st, M.ly->dev, op, permA, cl, (const double *)xw,
                         (double *)y);
    else
      hipLaunchKernelGGL(K.lo, grid_lo, dim3(L.nt_lo), lds_lo, st, M.ly->dev, op, permA, cl, (const c128 *)xw, (c128 *)y);
  }
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
