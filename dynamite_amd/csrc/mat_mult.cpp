// C ABI: every entry point that launches a multiply of a shell matrix.  A handle runs on one kernel family, its route
// (mat.h: Route, decided by dnm_mat_create): the one-rank multiply y = A x - b z + c z2 [, sums] is mult_fused -- one
// switch over the route, what the route does not fuse (mat.h: route_fuses) done by sweeps afterwards -- and the window
// multiplies of the partitions and the column-range sweeps share launch_rows / sweep_column_ranges.
#include "mat.h"
#include "vec_api.h"
#include "row_fused.h"

#include <algorithm>

using namespace dnm;

static hipStream_t S(void *stream) { return (hipStream_t)stream; }

// What one call adds to the description of a pass: the extra terms of the product (DevPass::zinit ... dot_out) and, for
// nparts > 1, the 1 / nparts of the pass's workgroups that starts at block_offset
struct PassCall {
  RowFuse fuse;
  uint32_t block_offset = 0;
  unsigned nparts = 1;
};

static int launch_pass(const dnm_mat *A, const PassOnDevice &p, const PassCall &c, const void *x, void *y,
                       const void *xr, hipStream_t st) {
  DevPass d = p.runs().desc;
  d.zinit = c.fuse.zinit; d.zscale = c.fuse.zscale;
  d.zinit2 = c.fuse.zinit2; d.z2re = c.fuse.z2re; d.z2im = c.fuse.z2im;
  d.dot_out = c.fuse.dot_out;
  d.block_offset = c.block_offset;
  return launch_tile_pass(d, d.tile_bits, d.log_rows, (A->flags & DNM_MAT_USE_GLDS) != 0, p.n_eff, x, y, xr, st, c.nparts,
                          p.reduced ? &p.reduced->flip : nullptr);
}

// partial sums a pass writes to dot_out: one per tile
static size_t pass_dot_partials(const dnm_mat *, const PassOnDevice &p) {
  return (size_t)1 << (p.n_eff - p.whole.desc.tile_bits);
}

// The internal-layout kernels (Route::Sc3Tiled / Sc3Rows) with the extra terms of `f`; win_start < 0: one rank, x is the
// whole vector; phase: sc3_launch.h
static int sc3_mult(dnm_mat *A, const void *x, void *y, const RowFuse &f, void *stream, int64_t win_start = -1,
                    int phase = 0) {
  Sc3Call call;
  call.row0 = A->sc3->row0;
  call.win_start = win_start >= 0 ? win_start : A->sc3->row0;
  call.zinit = (const double2 *)f.zinit;
  call.zscale = f.zscale;
  call.zinit2 = (const double2 *)f.zinit2;
  call.z2re = f.z2re;
  call.z2im = f.z2im;
  call.dot_out = f.dot_out;
  return launch_sc3(*A->sc3, A->dmsc_sc3, call, A->cached_diag(), x, y, S(stream), phase);
}

// workgroups of the one-thread-per-row kernel of a row route (the block kernel's handles sweep columns with it too)
static int row_blocks(const dnm_mat *A) {
  return A->route == Route::Gather ? gather_num_blocks(A->m_local) : sc_num_blocks(A->m_local);
}

// One launch of a row route's kernel (mat.h: row_route) over the rows [first_row, first_row + nrows): y and diag start
// at the first of them, x holds the columns [win_start, win_start + win_len) -- xswz -1: the whole right vector in its
// own layout (one rank), 0: a window in index order.  blk: the handle's ScBlock, or one narrowed to the rows.
// f: extra terms, for all rows of a handle on one rank only -- the block kernel takes them itself, the one-thread-per-row
// kernels have fused twins for them (row_fused.h) and run plain when there is none.
static int launch_rows(dnm_mat *A, const ScBlock &blk, int64_t nrows, int64_t first_row, int64_t win_start,
                       int64_t win_len, int xswz, const double *diag, const void *x, void *y, void *stream,
                       const RowFuse &f = RowFuse()) {
  const ScMask *scm = (const ScMask *)A->d_scmasks.p;
  const bool twin = f.zinit || f.dot_out;
  switch (A->route) {
    case Route::ScBlock:
      return launch_sc_block(A->dmsc, scm, blk, A->right.dev, nrows, first_row, win_start, win_len, diag, x, y, S(stream),
                             f.zinit, f.zscale, f.dot_out, f.zinit2, f.z2re, f.z2im);
    case Route::ScRows:
      if (twin) return launch_sc_matvec_fused(A->dmsc, scm, A->sclow, A->right.dev, nrows, diag, x, y, f, S(stream));
      return launch_sc_matvec(A->dmsc, scm, A->sclow, A->right.dev, nrows, first_row, win_start, diag, x, y, nullptr,
                              S(stream));
    case Route::Gather:
      if (twin) return launch_gather_matvec_fused(A->dmsc, A->left.dev, A->right.dev, nrows, diag, x, y, f, S(stream));
      return launch_gather_matvec(A->dmsc, A->left.dev, A->right.dev, nrows, diag, x, y, S(stream), first_row, win_start,
                                  xswz, nullptr);
    default: DNM_CHECK(false, "internal: not a row kernel's handle");
  }
  return 0;
}

// The sums a kernel leaves as workgroup partials part[nwg][3]: scratch before the launch; afterwards their reduction on
// the device, the copy of the three doubles and the synchronisation.  two_level: beyond 8192 partials
// vk_reduce_partials sums slices first.  The block kernel has always summed in ONE level, and its grid passes 8192
// (sc_block_grid: one workgroup per high part, 2^19 of them at L = 32): the second level would change its order of
// summation, i.e. results -- that is no refactoring, so the choice stays a parameter.
namespace {
struct SumPartials {
  double *part = nullptr;
  size_t nwg = 0;
  bool two_level = true;
  int scratch(size_t nwg_, bool two_level_ = true) {
    nwg = nwg_;
    two_level = two_level_;
    return vec_scratch(((nwg + 1) * 3 + (two_level ? vk_reduce_scratch(3) : 0)) * sizeof(double), &part);
  }
  int to_host(double *sums3_host, hipStream_t st) const {
    DNM_TRY(vk_reduce_partials(part, (int)nwg, 3, part + 3 * nwg, st, two_level ? part + 3 * nwg + 3 : nullptr));
    DNM_HIP(hipMemcpyAsync(sums3_host, part + 3 * nwg, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    DNM_HIP(hipStreamSynchronize(st));
    return 0;
  }
};
}  // namespace

// y = A x - b z + c z2 on one rank (t: z, b, z2, c as RowFuse states them; its dot_out is not read); sums3_host != null:
// also <x, y> = sum conj(x_i) y_i (re, im) and |y|^2 (no z2 then), and the stream is synchronised.  The kernels of the
// route take what route_fuses says they fuse; the rest follows in sweeps.
static int mult_fused(dnm_mat *A, const void *x, void *y, const RowFuse &t, double *sums3_host, void *stream) {
  DNM_CHECK(!A->host_only, "host-only handle cannot multiply");
  const RouteFuses can = route_fuses(*A);
  const bool sums_fused = sums3_host && can.sums;
  bool start_fused = can.start;
  if (row_route(A->route)) {
    DNM_CHECK(A->nranks == 1, "this subspace pair cannot run partitioned (use dnm_mat_mult_window)");
    if (sums3_host && !can.sums) start_fused = false;      // sums in a sweep of their own: it carries -b z as well
  }
  RowFuse k;                    // what the kernels are handed
  if (start_fused) k = t;
  k.dot_out = nullptr;
  SumPartials sp;
  switch (A->route) {
    case Route::Tiled: {        // the first pass starts from the vectors, the last one takes the sums
      const size_t np = A->local_passes.size();
      if (sums_fused) DNM_TRY(sp.scratch(pass_dot_partials(A, *A->local_passes.back())));
      for (size_t i = 0; i < np; ++i) {
        PassCall c;
        if (i == 0 && k.zinit) {
          DNM_CHECK(!A->local_passes[i]->whole.desc.accumulate, "internal: first pass accumulates");
          c.fuse = k;
        }
        if (i + 1 == np) c.fuse.dot_out = sp.part;
        DNM_TRY(launch_pass(A, *A->local_passes[i], c, x, y, nullptr, S(stream)));
      }
      break;
    }
    case Route::Sc3Tiled:
    case Route::Sc3Rows:
      if (sums_fused) DNM_TRY(sp.scratch(sc3_dot_partials(*A->sc3)));
      k.dot_out = sp.part;
      DNM_TRY(sc3_mult(A, x, y, k, stream));
      break;
    case Route::ScBlock:
    case Route::ScRows:
    case Route::Gather:
      if (sums_fused && A->route == Route::ScBlock) DNM_TRY(sp.scratch((size_t)sc_block_grid(A->scblock), false));
      else if (sums_fused) DNM_TRY(sp.scratch((size_t)row_blocks(A)));
      k.dot_out = sp.part;
      DNM_TRY(launch_rows(A, A->scblock, A->m_local, A->row0, 0, A->N, -1, A->cached_diag(), x, y, stream, k));
      break;
  }
  if (sums_fused) return sp.to_host(sums3_host, S(stream));
  if (sums3_host)
    return vec_lanczos_dot_host(y, start_fused ? nullptr : t.zinit, x, A->m_local, t.zscale, sums3_host, S(stream));
  if (!start_fused && t.zinit) DNM_TRY(vk_axpby(y, t.zinit, A->m_local, -t.zscale, 0.0, 1.0, 0.0, S(stream)));
  if (!start_fused && t.zinit2) DNM_TRY(vk_axpby(y, t.zinit2, A->m_local, t.z2re, t.z2im, 1.0, 0.0, S(stream)));
  return 0;
}

// Column ranges per workgroup of the row kernels: one sweep without vectors writes (min, max) of the columns each of
// the row_blocks(A) workgroups reads into buf, and marks the chunks of columns read if `mark` has a map.
static int sweep_column_ranges(dnm_mat *A, DevBuf *buf, ColMark mark, void *stream) {
  DNM_TRY(buf->alloc((size_t)row_blocks(A) * 2 * sizeof(int64_t)));
  if (A->route == Route::Gather)
    return launch_gather_matvec(A->dmsc, A->left.dev, A->right.dev, A->m_local, nullptr, nullptr, nullptr, S(stream),
                                A->row0, 0, 0, (int64_t *)buf->p, mark);
  return launch_sc_matvec(A->dmsc, (const ScMask *)A->d_scmasks.p, A->sclow, A->right.dev, A->m_local, A->row0, 0,
                          nullptr, nullptr, nullptr, (int64_t *)buf->p, S(stream), mark);
}

// A later pass adds to what the passes before it wrote of the SAME call of dnm_mat_mult_local_part: range `part` has to
// be the same amplitudes in every pass, i.e. the top log2(nparts) block-id bits of every pass are the same index bits in
// the same order.  (Two tile-only passes that agree on their highest free bit need not agree on the next one: the window
// tile of the second holds it, and its workgroups split along a lower bit -- four ranges then gave another y than the
// whole launch.)  Returns the first pass whose ranges differ from those of pass 0, -1 if none does.
static int part_ranges_agree(const dnm_mat *A, int nparts) {
  if (A->local_passes.size() < 2 || nparts < 2) return -1;
  int logp = 0;
  while ((1 << logp) < nparts) ++logp;
  std::vector<int> first;
  for (size_t i = 0; i < A->local_passes.size(); ++i) {
    const DevPass &d = A->local_passes[i]->whole.desc;
    const int nbb = A->local_passes[i]->n_eff - d.tile_bits;
    std::vector<int> pos;
    for (int b = std::max(0, nbb - logp); b < nbb; ++b)
      for (int j = 0; j < d.nbseg; ++j)
        if (b >= d.bseg_off[j] && b < d.bseg_off[j] + d.bseg_len[j]) pos.push_back(d.bseg_pos[j] + b - d.bseg_off[j]);
    if (i == 0) first = pos;
    else if (pos != first) return (int)i;
  }
  return -1;
}

extern "C" {

int dnm_mat_mult_local(dnm_mat *A, const void *x, void *y, void *stream) {
  DNM_CHECK(A && x && y, "null argument");
  DNM_CHECK(!A->host_only, "host-only handle cannot multiply");
  DNM_CHECK(x != y, "x and y must be different vectors");
  // (the tiled passes of a partitioned handle are its rank-local part)
  DNM_CHECK(A->route == Route::Tiled || A->nranks == 1, "this subspace pair cannot run partitioned (use dnm_mat_mult_window)");
  return mult_fused(A, x, y, RowFuse(), nullptr, stream);
}

// The rank-local passes over ONE of nparts equal ranges of their workgroups (block ids [part, part + 1) * grid / nparts):
// with an LDS-only plan whose tile holds the top index bits, range `part` reads and writes exactly the amplitudes whose
// highest non-tile index bits equal `part` -- the transposed exchange runs its layout-B pass sub-piece by sub-piece.
int dnm_mat_mult_local_part(dnm_mat *A, const void *x, void *y, int part, int nparts, void *stream) {
  DNM_CHECK(A && x && y && x != y && !A->host_only, "bad argument");
  DNM_CHECK(A->route == Route::Tiled, "only the tiled hypercube passes run over a range of their workgroups");
  DNM_CHECK(nparts >= 1 && (nparts & (nparts - 1)) == 0 && part >= 0 && part < nparts, "bad range %d of %d", part, nparts);
  DNM_CHECK(part_ranges_agree(A, nparts) < 0,
            "the %d ranges of pass %d of this plan are not the amplitudes of the ranges of its first pass", nparts,
            part_ranges_agree(A, nparts));
  for (auto &p : A->local_passes) {
    const unsigned grid = 1u << (p->n_eff - p->whole.desc.tile_bits);
    DNM_CHECK((unsigned)nparts <= grid, "more ranges than workgroups");
    PassCall c;
    c.block_offset = (uint32_t)part * (grid / (unsigned)nparts);
    c.nparts = (unsigned)nparts;
    DNM_TRY(launch_pass(A, *p, c, x, y, nullptr, S(stream)));
  }
  return 0;
}

// 1 if range `part` of nparts is the same amplitudes in every rank-local pass (always on a plan of one pass): what
// dnm_mat_mult_local_part needs, for callers that decide beforehand whether to run by ranges
int dnm_mat_local_part_agree(const dnm_mat *A, int nparts, int *agree) {
  DNM_CHECK(A && agree && nparts >= 1 && (nparts & (nparts - 1)) == 0, "bad argument");
  *agree = part_ranges_agree(A, nparts) < 0 ? 1 : 0;
  return 0;
}

// what the top non-tile index bits of the rank-local passes are: *top_free_bit = the highest index bit that is in no
// pass's tile (the ranges of dnm_mat_mult_local_part split along it and the ones below it), -1 if passes disagree
int dnm_mat_local_part_bits(const dnm_mat *A, int *top_free_bit, int *gathers) {
  DNM_CHECK(A && top_free_bit && gathers, "null argument");
  *top_free_bit = -1;
  *gathers = 0;
  if (A->route != Route::Tiled) return 0;
  int top = -2;
  for (auto &p : A->local_passes) {
    uint64_t tb = 0;
    const DevPass &d = p->whole.desc;
    for (int j = 0; j < d.nseg; ++j) tb |= ((((uint64_t)1 << d.seg_len[j]) - 1) << d.seg_pos[j]);
    int hi = p->n_eff - 1;
    while (hi >= 0 && ((tb >> hi) & 1)) --hi;
    if (top == -2) top = hi; else if (top != hi) top = -1;
    *gathers += (int)(d.loop[LP_COUNT] - d.loop[LP_GATHER_REAL]);     // gathered records
    *gathers += (int)(d.tab_loop[2] - d.tab_loop[1]);
  }
  *top_free_bit = top < 0 ? -1 : top;
  return 0;
}

// y = A x - b z, <x, y> = sum conj(x_i) y_i and |y|^2 (z may be null): the Lanczos step
int dnm_mat_mult_lanczos(dnm_mat *A, const void *x, void *y, const void *z, double b, double *dot, void *stream) {
  DNM_CHECK(A && x && y && dot, "null argument");
  DNM_CHECK(A->remote_passes.empty(), "operator couples different ranks: no fused Lanczos step");
  DNM_CHECK(z != y && x != y, "y must not alias x or z");
  // <x, y> pairs element i of x with element i of y: on a handle between two subspaces that is no inner product, and
  // with M > N the sweep of the sums (a route that does not fuse them) would read past the end of x; the sweep pairs
  // by position in memory, so one subspace in two vector layouts is no inner product either (dnm_mat_create turns a
  // Full / Parity pair of two layouts away already: this is the statement of what the sums need, at their entry)
  DNM_CHECK(A->one_subspace,
            "the sums of a Lanczos step need the same subspace on both sides (this handle projects between two)");
  DNM_CHECK(A->left.host.swz == A->right.host.swz,
            "the sums of a Lanczos step need x and y in one vector layout (left vec_swizzle %d, right %d)",
            A->left.host.swz, A->right.host.swz);
  return mult_fused(A, x, y, RowFuse{z, b}, dot, stream);
}

// true when the multiply can start its accumulators from other vectors (dnm_mat_mult_sub2 costs no extra sweep)
int dnm_mat_fuses_init(const dnm_mat *A) { return A && route_fuses(*A).start ? 1 : 0; }

// y = A x - b z + c z2 without the sums (Chebyshev / Clenshaw recurrences; z2 may be null): the extra terms ride
// on the multiply where a kernel can start its accumulators from them, otherwise one more sweep each.
int dnm_mat_mult_sub2(dnm_mat *A, const void *x, void *y, const void *z, double b, const void *z2, double c_re,
                      double c_im, void *stream) {
  DNM_CHECK(A && x && y && z, "null argument");
  DNM_CHECK(A->remote_passes.empty(), "operator couples different ranks: use the partitioned multiply");
  DNM_CHECK(z != y && x != y && z2 != y, "y must not alias x, z or z2");
  return mult_fused(A, x, y, RowFuse{z, b, z2, c_re, c_im}, nullptr, stream);
}

int dnm_mat_mult_sub(dnm_mat *A, const void *x, void *y, const void *z, double b, void *stream) {
  return dnm_mat_mult_sub2(A, x, y, z, b, nullptr, 0.0, 0.0, stream);
}

int dnm_mat_mult_dot(dnm_mat *A, const void *x, void *y, double *dot, void *stream) {
  DNM_CHECK(dot, "null argument");
  double d3[3];
  DNM_TRY(dnm_mat_mult_lanczos(A, x, y, nullptr, 0.0, d3, stream));
  dot[0] = d3[0];
  dot[1] = d3[1];
  return 0;
}

int dnm_mat_mult(dnm_mat *A, const void *x, void *y, void *stream) {
  DNM_CHECK(A, "null matrix");
  DNM_CHECK(A->remote_passes.empty(),
            "operator couples different ranks: use dnm_mat_mult_local + dnm_mat_mult_remote");
  return dnm_mat_mult_local(A, x, y, stream);
}

int dnm_mat_column_window(dnm_mat *A, int64_t *cmin, int64_t *cmax, void *stream) {
  DNM_CHECK(A && cmin && cmax, "bad argument");
  if (A->use_sc3) {          // positions of the internal layout, from the T blocks the rank's rows reach (host tables)
    A->sc3->window(cmin, cmax);
    if (A->real_packed) {     // whole blocks: [cmin, cmax + 1) is a range of pairs
      *cmin /= 2;
      *cmax = (*cmax + 1) / 2 - 1;
    }
    return 0;
  }
  DNM_CHECK(!A->host_only, "bad argument");
  DNM_CHECK(A->route != Route::Tiled, "Full/Parity partitions on 2^p ranks exchange partner blocks, not windows");
  if (A->win_max < A->win_min) {
    const int nb = row_blocks(A);
    DevBuf buf;
    DNM_TRY(sweep_column_ranges(A, &buf, ColMark(), stream));
    std::vector<int64_t> h((size_t)nb * 2);
    DNM_TRY(dnm_memcpy_d2h(h.data(), buf.p, h.size() * sizeof(int64_t), stream));
    // (a SpinConserve pair always reads its own rows' columns; a general pair reads what its masks reach)
    int64_t lo = A->sc_pair ? A->row0 : INT64_MAX, hi = A->sc_pair ? A->row0 + A->m_local - 1 : INT64_MIN;
    for (int b = 0; b < nb; ++b) { lo = std::min(lo, h[2 * b]); hi = std::max(hi, h[2 * b + 1]); }
    if (hi < lo) lo = hi = 0;          // no matrix element at all in these rows
    A->win_min = lo;
    A->win_max = hi;
  }
  *cmin = A->win_min;
  *cmax = A->win_max;
  return 0;
}

int dnm_mat_column_chunks(dnm_mat *A, int chunk_shift, uint8_t *map, int64_t nchunks, void *stream) {
  DNM_CHECK(A && map && chunk_shift >= 0 && chunk_shift < 62, "bad argument");
  int64_t lo, hi;
  DNM_TRY(dnm_mat_column_window(A, &lo, &hi, stream));
  const int64_t first = lo >> chunk_shift;
  DNM_CHECK(nchunks == (hi >> chunk_shift) - first + 1, "the window [%lld, %lld] has %lld chunks of 2^%d columns",
            (long long)lo, (long long)hi, (long long)((hi >> chunk_shift) - first + 1), chunk_shift);
  if (A->use_sc3) {
    A->sc3->chunks(chunk_shift + (A->real_packed ? 1 : 0), first, nchunks, map);      // (chunks of 2^shift elements)
    return 0;
  }
  DevBuf range, dmap;
  DNM_TRY(dmap.alloc((size_t)nchunks));
  DNM_HIP(hipMemsetAsync(dmap.p, 0, (size_t)nchunks, S(stream)));
  ColMark mark;
  mark.map = (uint8_t *)dmap.p;
  mark.shift = chunk_shift;
  mark.first = first;
  DNM_TRY(sweep_column_ranges(A, &range, mark, stream));
  DNM_TRY(dnm_memcpy_d2h(map, dmap.p, (size_t)nchunks, stream));
  return 0;
}

int dnm_mat_mult_window(dnm_mat *A, const void *x_window, int64_t win_start, int64_t win_len, void *y_local,
                        void *stream) {
  DNM_CHECK(A && x_window && y_local && !A->host_only, "bad argument");
  int64_t lo, hi;
  DNM_TRY(dnm_mat_column_window(A, &lo, &hi, stream));
  DNM_CHECK(win_start <= lo && win_start + win_len > hi,
            "window [%lld, %lld) does not cover the columns [%lld, %lld] this rank reads", (long long)win_start,
            (long long)(win_start + win_len), (long long)lo, (long long)hi);
  if (A->use_sc3) return sc3_mult(A, x_window, y_local, RowFuse(), stream, A->real_packed ? 2 * win_start : win_start);
  // the rank's rows, columns read from the window (index order)
  return launch_rows(A, A->scblock, A->m_local, A->row0, win_start, win_len, 0, A->cached_diag(), x_window, y_local,
                     stream);
}

// Rows of a window partition whose columns all lie in [col_lo, col_hi) -- the rank's own block of x: they can be
// multiplied while the rest of the window is on the links.  From the per-workgroup column ranges of the row kernels
// (one sweep): runs of consecutive workgroups that read nothing else, the largest `max_ranges` of them, none
// shorter than min_blocks workgroups (of 256 rows).  ranges: pairs [r0, r1) of local row numbers, ascending.
int dnm_mat_window_local_rows(dnm_mat *A, int64_t col_lo, int64_t col_hi, int max_ranges, int min_blocks,
                              int64_t *ranges, int *nranges, void *stream) {
  DNM_CHECK(A && ranges && nranges && max_ranges >= 1, "bad argument");
  *nranges = 0;
  if (A->host_only || !row_route(A->route) || A->m_local <= 0) return 0;
  if (A->left.host.swz != 0) return 0;       // a swizzled result block is not a sequence of row ranges
  DNM_CHECK(A->row0 >= 0, "internal: no first row in reference order");      // (the sweep below walks reference rows)
  const int64_t per = A->route == Route::Gather ? gather_rows_per_block() : sc_rows_per_block();
  const int nb = row_blocks(A);
  DevBuf buf;
  DNM_TRY(sweep_column_ranges(A, &buf, ColMark(), stream));
  std::vector<int64_t> h((size_t)nb * 2);
  DNM_TRY(dnm_memcpy_d2h(h.data(), buf.p, h.size() * sizeof(int64_t), stream));
  // (a SpinConserve pair reads its own rows' columns as well: the diagonal and the row's own amplitude)
  struct Run { int64_t b0, b1; };
  std::vector<Run> runs;
  for (int b = 0; b < nb;) {
    auto local = [&](int i) {
      int64_t lo = h[2 * (size_t)i], hi = h[2 * (size_t)i + 1];
      if (A->sc_pair) {
        lo = std::min(lo, A->row0 + (int64_t)i * per);
        hi = std::max(hi, std::min(A->row0 + A->m_local, A->row0 + (int64_t)(i + 1) * per) - 1);
      }
      return hi < lo || (lo >= col_lo && hi < col_hi);
    };
    if (!local(b)) { ++b; continue; }
    int e = b;
    while (e < nb && local(e)) ++e;
    if (e - b >= std::max(1, min_blocks)) runs.push_back({b, e});
    b = e;
  }
  std::sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) { return a.b1 - a.b0 > b.b1 - b.b0; });
  if ((int)runs.size() > max_ranges) runs.resize((size_t)max_ranges);
  std::sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) { return a.b0 < b.b0; });
  for (const Run &r : runs) {
    ranges[2 * *nranges] = r.b0 * per;
    ranges[2 * *nranges + 1] = std::min(A->m_local, r.b1 * per);
    ++*nranges;
  }
  return 0;
}

// dnm_mat_mult_window for the local rows [r0, r1) only (y_local is still the rank's whole result block)
int dnm_mat_mult_window_rows(dnm_mat *A, const void *x_window, int64_t win_start, int64_t win_len, void *y_local,
                             int64_t r0, int64_t r1, void *stream) {
  DNM_CHECK(A && x_window && y_local && !A->host_only, "bad argument");
  DNM_CHECK(row_route(A->route), "this operator does not multiply by row ranges");
  DNM_CHECK(r0 >= 0 && r0 < r1 && r1 <= A->m_local, "row range [%lld, %lld) outside the %lld local rows", (long long)r0,
            (long long)r1, (long long)A->m_local);
  ScBlock blk = A->scblock;
  if (A->route == Route::ScBlock) {        // the high parts of these rows, in ascending order
    blk.h_first = sub_i2s(A->row0 + r0, A->left.host) >> blk.lb;
    blk.h_last = sub_i2s(A->row0 + r1 - 1, A->left.host) >> blk.lb;
    blk.swizzle = 0;
    blk.perm = nullptr;
    blk.nperm = 0;
  }
  return launch_rows(A, blk, r1 - r0, A->row0 + r0, win_start, win_len, 0, A->have_diag ? A->cached_diag() + r0 : nullptr,
                     x_window, (char *)y_local + (size_t)r0 * 16, stream);
}

int dnm_mat_window_split(const dnm_mat *A, int *supported) {
  DNM_CHECK(A && supported, "null argument");
  *supported = (A->route == Route::Sc3Tiled && !A->sc3->graph && A->nranks > 1) ? 1 : 0;    // (a bond graph's lo pass reads other blocks)
  return 0;
}

int dnm_mat_mult_window_local(dnm_mat *A, const void *x_local, void *y_local, void *stream) {
  DNM_CHECK(A && x_local && y_local && !A->host_only, "bad argument");
  DNM_CHECK(A->route == Route::Sc3Tiled, "this operator's window multiply does not split (dnm_mat_window_split)");
  // the lo pass reads the rank's own rows and, for the Lo/W boundary bond, other rows of the same T block: all local
  return sc3_mult(A, x_local, y_local, RowFuse(), stream, A->sc3->row0, 1);
}

int dnm_mat_mult_window_remote(dnm_mat *A, const void *x_window, int64_t win_start, int64_t win_len, void *y_local,
                               void *stream) {
  DNM_CHECK(A && x_window && y_local && !A->host_only, "bad argument");
  DNM_CHECK(A->route == Route::Sc3Tiled, "this operator's window multiply does not split (dnm_mat_window_split)");
  int64_t lo, hi;
  DNM_TRY(dnm_mat_column_window(A, &lo, &hi, stream));
  DNM_CHECK(win_start <= lo && win_start + win_len > hi,
            "window [%lld, %lld) does not cover the positions [%lld, %lld] this rank reads", (long long)win_start,
            (long long)(win_start + win_len), (long long)lo, (long long)hi);
  return sc3_mult(A, x_window, y_local, RowFuse(), stream, A->real_packed ? 2 * win_start : win_start, 2);
}

int dnm_mat_mult_remote(dnm_mat *A, int32_t recv_index, const void *x_recv, void *y, void *stream) {
  DNM_CHECK(A && x_recv && y, "null argument");
  DNM_CHECK(!A->host_only, "host-only handle cannot multiply");
  DNM_CHECK(recv_index >= 0 && recv_index < (int)A->remote_passes.size(), "rank %d has no receive %d", A->rank,
            recv_index);
  const auto &p = A->remote_passes[recv_index];
  return launch_pass(A, *p, PassCall(), x_recv, (char *)y + (size_t)p->y_off * 16, x_recv, S(stream));
}

}  // extern "C"
