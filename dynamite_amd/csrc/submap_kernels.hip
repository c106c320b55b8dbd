// Subspace maps: a state moved between two subspaces of the same L spins in one pass over the target, and the weight of
// a state per magnetisation sector and per sector of the global flip in one pass over it.  Definitions, the table of
// the four (source, target) cases and the index arithmetic: submap_rank.h.
//
// submap_kernel<ST, DT>: target-driven, one instance per (source type, target type), no atomics, every index 64-bit;
// the grid follows from the target's rows alone.  Full / Parity / Explicit targets: a thread takes the row at its
// position (adjacent lanes store adjacent 16-byte amplitudes: 1 KB per wave instruction); its configuration follows
// from the index (Explicit: one coalesced load of the list).  SpinConserve targets: reference order; a thread owns a
// run of SUBMAP_RUN adjacent rows, unranks the first and steps by perm_next_config, so that a lane covers 64 contiguous
// bytes of y which the four stores of a run complete.  The binomials of a SpinConserve side are staged in LDS.  In the
// closed-form subspaces index order is ascending configuration order, so that the gathers of x climb with the rows;
// an Explicit source is searched (bucket table first where the descriptor has one).  A row whose configuration is not
// in the source is written as zero by the same store: there is no memset pass.
//
// sector_weights_kernel<T>: a workgroup takes SW_ROWS_PER_WG adjacent rows at a time -- or as many pairs (i, dim - 1 - i)
// where the subspace carries the flip in closed form, the partner read as a second, descending stream -- and every
// thread adds |x|^2 into a column of its own in LDS, bins[popcount][thread]: 2 KB between the bins, so that the lanes
// of a wave never share a bank whatever their popcounts.  At the end the columns of a bin are summed in a fixed order
// (four per lane, then XOR shuffles), the workgroups by vk_reduce_partials in their order: no floating-point atomics,
// and the number of workgroups follows from the rows alone, so two calls return the same bits.
#include "submap.h"

namespace dnm {

typedef double2 c128;

static void submap_side(const SubView &v, int xsec, SubmapSide *s) {
  s->v = v;
  s->xsec = xsec;
  s->dim = sub_dim(v);
  s->closed = v.type == DNM_FULL || (v.type == DNM_PARITY && v.L % 2 == 0) ||
              (v.type == DNM_SPIN_CONSERVE && v.L == 2 * v.k);
  s->rows = xsec ? s->dim / 2 : s->dim;
}

int submap_plan(const SubView &src, int src_xsec, const SubView &dst, int dst_xsec, SubmapPlan *p) {
  SubmapPlan q{};
  submap_side(src, src_xsec, &q.src);
  submap_side(dst, dst_xsec, &q.dst);
  q.mode = submap_mode(src_xsec, dst_xsec);
  q.run = dst.type == DNM_SPIN_CONSERVE ? SUBMAP_RUN : 1;
  int64_t nwg = (q.dst.rows + ((int64_t)1 << SUBMAP_ROWS_PER_WG_LOG2) - 1) >> SUBMAP_ROWS_PER_WG_LOG2;
  if (nwg > SUBMAP_MAX_WG) nwg = SUBMAP_MAX_WG;
  if (nwg < 1) nwg = 1;
  q.nwg = (int)nwg;
  q.ntab_src = src.type == DNM_SPIN_CONSERVE ? (src.k + 1) * src.ld : 0;
  q.ntab_dst = dst.type == DNM_SPIN_CONSERVE ? (dst.k + 1) * dst.ld : 0;
  q.lds_bytes = ((size_t)(q.ntab_src + q.ntab_dst) * 8 + 15) & ~(size_t)15;
  *p = q;
  return 0;
}

struct SubmapArgs {
  SubmapSide src, dst;
  int32_t mode, ntab_src, ntab_dst;
};

template <int ST, int DT>
__global__ void __launch_bounds__(SUBMAP_NT)
submap_kernel(const c128 *__restrict__ x, c128 *__restrict__ y, const SubmapArgs a) {
  constexpr int RUN = DT == DNM_SPIN_CONSERVE ? SUBMAP_RUN : 1;
  extern __shared__ __align__(16) unsigned char submap_lds[];
  int64_t *tab = reinterpret_cast<int64_t *>(submap_lds);
  SubmapSide src = a.src;
  SubView dv = a.dst.v;
  if (ST == DNM_SPIN_CONSERVE) {
    for (int i = threadIdx.x; i < a.ntab_src; i += SUBMAP_NT) tab[i] = a.src.v.nchoosek[i];
    src.v.nchoosek = tab;
  }
  if (DT == DNM_SPIN_CONSERVE) {
    for (int i = threadIdx.x; i < a.ntab_dst; i += SUBMAP_NT) tab[a.ntab_src + i] = a.dst.v.nchoosek[i];
    dv.nchoosek = tab + a.ntab_src;
  }
  if (ST == DNM_SPIN_CONSERVE || DT == DNM_SPIN_CONSERVE) __syncthreads();
  const int64_t nrows = a.dst.rows;
  const int dxsec = a.dst.xsec;
  const int64_t nruns = (nrows + RUN - 1) / RUN;
  for (int64_t q = (int64_t)blockIdx.x * SUBMAP_NT + threadIdx.x; q < nruns; q += (int64_t)gridDim.x * SUBMAP_NT) {
    int64_t row = q * RUN;
    uint64_t cfg = submap_row_config<DT>(row, dv);
    for (int j = 0; j < RUN && row < nrows; ++j, ++row) {
      SubmapTerms t;
      submap_terms<ST>(cfg, src, dxsec, &t);
      c128 v = make_double2(0.0, 0.0);
      if (a.mode == SUBMAP_TO_SECTOR) {
        c128 p = v, m = v;
        if (t.idx[0] >= 0) p = x[t.idx[0]];
        if (t.idx[1] >= 0) m = x[t.idx[1]];
        if (dxsec > 0) v = make_double2(p.x + m.x, p.y + m.y);
        else v = make_double2(p.x - m.x, p.y - m.y);
        v = make_double2(v.x * SUBMAP_KAPPA, v.y * SUBMAP_KAPPA);
      } else if (t.idx[0] >= 0) {
        v = x[t.idx[0]];
        if (a.mode == SUBMAP_FROM_SECTOR) {
          const double f = t.sign[0] < 0 ? -SUBMAP_KAPPA : SUBMAP_KAPPA;
          v = make_double2(v.x * f, v.y * f);
        }
      }
      y[row] = v;
      if (RUN > 1 && j + 1 < RUN && row + 1 < nrows) cfg = perm_next_config(cfg);
    }
  }
}

int launch_submap(const void *x, void *y, const SubmapPlan &p, hipStream_t st) {
  SubmapArgs a{};
  a.src = p.src;
  a.dst = p.dst;
  a.mode = p.mode;
  a.ntab_src = p.ntab_src;
  a.ntab_dst = p.ntab_dst;
  const int rc = submap_dispatch(p.src.v.type, p.dst.v.type, [&](auto S, auto D) {
    auto k = submap_kernel<decltype(S)::value, decltype(D)::value>;
    if (p.lds_bytes)
      DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(SUBMAP_NT), p.lds_bytes, st, (const c128 *)x, (c128 *)y, a);
    DNM_HIP(hipGetLastError());
    return 0;
  });
  if (rc < 0) {
    set_error("subspace map: subspace types %d, %d", p.src.v.type, p.dst.v.type);
    return 1;
  }
  return rc;
}

// ---- sector weights ------------------------------------------------------------------------------------------------
int sector_weights_plan(const SubView &v, int xsec, SectorWeightsPlan *p) {
  SectorWeightsPlan q{};
  submap_side(v, xsec, &q.side);
  q.pairs = xsec == 0 && q.side.closed && v.type != DNM_EXPLICIT && q.side.dim % 2 == 0;
  q.items = q.pairs ? q.side.dim / 2 : q.side.rows;
  q.ncols = v.L + 3;
  int64_t nwg = (q.items + SW_ROWS_PER_WG - 1) / SW_ROWS_PER_WG;
  if (nwg > SW_MAX_WG) nwg = SW_MAX_WG;
  if (nwg < 1) nwg = 1;
  q.nwg = (int)nwg;
  q.lds_bytes = (size_t)q.ncols * SUBMAP_NT * sizeof(double);
  q.partial_bytes = (size_t)q.nwg * (size_t)q.ncols * sizeof(double);
  *p = q;
  return 0;
}

struct SwArgs {
  SubmapSide side;
  int64_t items;
  int32_t pairs, ncols;
};

__device__ __forceinline__ double sw_norm2(c128 v) { return v.x * v.x + v.y * v.y; }

template <int T>
__global__ void __launch_bounds__(SUBMAP_NT)
sector_weights_kernel(const c128 *__restrict__ x, const SwArgs a, double *__restrict__ partial) {
  constexpr int PER = SW_ROWS_PER_WG / SUBMAP_NT;
  extern __shared__ __align__(16) unsigned char submap_lds[];
  double *bins = reinterpret_cast<double *>(submap_lds);       // [ncols][SUBMAP_NT]: a thread's column is its own
  const int tid = threadIdx.x;
  const int L = a.side.v.L;
  for (int c = 0; c < a.ncols; ++c) bins[c * SUBMAP_NT + tid] = 0.0;
  double fp = 0.0, fm = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * SW_ROWS_PER_WG; base < a.items; base += (int64_t)gridDim.x * SW_ROWS_PER_WG) {
    c128 va[PER], vb[PER];
    int64_t idx[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int64_t p = base + j * SUBMAP_NT + tid;
      va[j] = vb[j] = make_double2(0.0, 0.0);
      idx[j] = -1;
      if (p < a.items) {
        idx[j] = submap_pos<T>(p, a.side.v);
        va[j] = x[p];
        if (a.pairs) vb[j] = x[submap_pos<T>(a.side.dim - 1 - idx[j], a.side.v)];
      }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (idx[j] < 0) continue;
      const int k = submap_row_popcount<T>(idx[j], a.side.v);
      const double w = sw_norm2(va[j]);
      if (a.pairs) {
        bins[k * SUBMAP_NT + tid] += w;
        bins[(L - k) * SUBMAP_NT + tid] += sw_norm2(vb[j]);
        fp += 0.5 * sw_norm2(make_double2(va[j].x + vb[j].x, va[j].y + vb[j].y));
        fm += 0.5 * sw_norm2(make_double2(va[j].x - vb[j].x, va[j].y - vb[j].y));
      } else if (a.side.xsec) {
        bins[k * SUBMAP_NT + tid] += 0.5 * w;
        bins[(L - k) * SUBMAP_NT + tid] += 0.5 * w;
        if (a.side.xsec > 0) fp += w;
        else fm += w;
      } else {
        bins[k * SUBMAP_NT + tid] += w;
      }
    }
  }
  bins[(L + 1) * SUBMAP_NT + tid] = fp;
  bins[(L + 2) * SUBMAP_NT + tid] = fm;
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int c = wave; c < a.ncols; c += SUBMAP_NT / 64) {
    const double *col = bins + c * SUBMAP_NT;
    double s = ((col[lane] + col[lane + 64]) + col[lane + 128]) + col[lane + 192];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) partial[(int64_t)blockIdx.x * a.ncols + c] = s;
  }
}

int launch_sector_weights(const void *x, const SectorWeightsPlan &p, void *partial, void *out, hipStream_t st) {
  SwArgs a{};
  a.side = p.side;
  a.items = p.items;
  a.pairs = p.pairs;
  a.ncols = p.ncols;
  const int rc = submap_dispatch1(p.side.v.type, [&](auto T) {
    auto k = sector_weights_kernel<decltype(T)::value>;
    DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(SUBMAP_NT), p.lds_bytes, st, (const c128 *)x, a, (double *)partial);
    DNM_HIP(hipGetLastError());
    return 0;
  });
  if (rc < 0) {
    set_error("sector weights: subspace type %d", p.side.v.type);
    return 1;
  }
  DNM_TRY(rc);
  return vk_reduce_partials((const double *)partial, p.nwg, p.ncols, (double *)out, st);
}

}  // namespace dnm
