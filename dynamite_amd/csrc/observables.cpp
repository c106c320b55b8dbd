// C ABI: the observables of a state that are computed in one pass over it and never touch a shell matrix -- reduced
// density matrices (dense and sector by sector) and the sigma-z, sigma+ sigma-, bond-swap, three-site rotation
// (chirality) and two-spin Pauli moments -- the Gram matrix of many vectors, which runs on the same panel scheme, the
// site permutations of a state (two plain gather kernels, no panel), the maps of a state between subspaces with its
// weights per sector (a gather and a streaming kernel, no panel), and Born sampling with the power sums of the
// participation entropies (streaming passes over |x_i|^2, no panel).  They share the cached scratch of the partial
// tiles.
#include "born.h"
#include "gram_tile.h"
#include "mat.h"
#include "pm_rank.h"
#include "cyc_rank.h"
#include "pauli_cols.h"
#include "perm.h"
#include "submap.h"
#include "vgram.h"

#include <algorithm>
#include <cstring>

namespace dnm {

static DevBuf g_rdm_scratch;     // released by dnm_release_workspace()

int rdm_release_scratch() {
  g_rdm_scratch.release();
  return 0;
}

}  // namespace dnm

using namespace dnm;
static hipStream_t S(void *s) { return (hipStream_t)s; }

// Scratch for the partial tiles: up to 1 GiB it is kept between calls (hipMalloc costs more than the kernel), a larger
// one lives in `big`, which the caller releases after the stream has drained.  `what`, tiles, tm, slices: for the
// message when the device has no room.
static int rdm_scratch(size_t bytes, DevBuf *big, void **scratch, const char *what, long long tiles, int tm,
                       int slices) {
  DevBuf &cached = g_rdm_scratch;
  const bool keep_it = bytes <= ((size_t)1 << 30);
  if (!keep_it || cached.bytes < bytes) {
    if (keep_it) cached.release();
    size_t free_b = 0, total_b = 0;
    DNM_HIP(hipMemGetInfo(&free_b, &total_b));
    DNM_CHECK(bytes <= free_b, "%s: %zu bytes of scratch asked for (%lld tiles of %d x %d in %d slices), %zu bytes of "
              "device memory free", what, bytes, tiles, tm, tm, slices, free_b);
    DNM_TRY((keep_it ? cached : *big).alloc(bytes));
  }
  *scratch = keep_it ? cached.p : big->p;
  return 0;
}

// ---- what the moment passes share ----------------------------------------------------------------------------------
// the out-parameters of a *_moments_plan entry point, each optional
static void plan_out(int nb, int B, int nwg, size_t lds, size_t scratch, int *tile_rows, int *panel_rows_log2,
                     int *nworkgroups, size_t *lds_bytes, size_t *scratch_bytes) {
  if (tile_rows) *tile_rows = nb;
  if (panel_rows_log2) *panel_rows_log2 = B;
  if (nworkgroups) *nworkgroups = nwg;
  if (lds_bytes) *lds_bytes = lds;
  if (scratch_bytes) *scratch_bytes = scratch;
}

// A Gram-matrix sweep (gram_tile.h) from its plan to the result on the host: scratch for the partial tiles, the D x D
// complex128 matrix and the binomials pm_binomials(L, p.K, L + 1) of a SpinConserve sweep, their upload,
// launch(table, partial, matrix) and the copy into `out`.  `what`: the pass, for the message about the scratch.
template <class Launch>
static int gram_moments(const GramPlan &p, int L, size_t D, const char *what, double *out, void *stream, Launch launch) {
  const size_t obytes = D * D * 2 * sizeof(double);
  std::vector<int64_t> nck(p.table_bytes / sizeof(int64_t));
  if (!nck.empty()) pm_binomials(L, p.K, L + 1, nck.data());
  DevBuf big;
  void *scratch = nullptr;       // the partial tiles, the matrix, the binomials
  DNM_TRY(rdm_scratch(p.partial_bytes + obytes + p.table_bytes, &big, &scratch, what,
                      (long long)(p.partial_bytes / 2048 / (size_t)p.nwg), 16, p.nwg));
  void *g_dev = (char *)scratch + p.partial_bytes;
  int64_t *t_dev = (int64_t *)((char *)g_dev + obytes);
  if (!nck.empty())
    DNM_HIP(hipMemcpyAsync(t_dev, nck.data(), nck.size() * sizeof(int64_t), hipMemcpyHostToDevice, S(stream)));
  DNM_TRY(launch(t_dev, scratch, g_dev));
  // (synchronises: `big` and the host table are released on return)
  return dnm_memcpy_d2h(out, g_dev, obytes, stream);
}

extern "C" {

// ---- reduced density matrix -----------------------------------------------------------
// runs of kept / traced spin positions (kernels.h: RdmGeom)
static void rdm_geom(int L, int keep_size, const int64_t *keep, RdmGeom *out) {
  RdmGeom &geo = *out;
  memset(&geo, 0, sizeof(geo));
  geo.k = keep_size;
  geo.L = L;
  uint64_t keepmask = 0;
  for (int i = 0; i < keep_size; ++i) keepmask |= (uint64_t)1 << keep[i];
  for (int pos = 0; pos < L;) {
    const bool kept = (keepmask >> pos) & 1;
    int end = pos;
    while (end < L && (((keepmask >> end) & 1) != 0) == kept) ++end;
    if (kept) {
      geo.klen[geo.nseg_keep] = (int8_t)(end - pos);
      geo.kpos[geo.nseg_keep++] = (int8_t)pos;
    } else {
      geo.tlen[geo.nseg_tr] = (int8_t)(end - pos);
      geo.tpos[geo.nseg_tr++] = (int8_t)pos;
    }
    pos = end;
  }
}

// the kept spins of a call: at most `cap` of them (over_cap: the caller's message, a format that is handed keep_size
// twice and may use it once), inside [0, L), strictly increasing (bpetsc_template_1.c:117-121)
static int rdm_check_keep(int L, int keep_size, const int64_t *keep, int cap, const char *over_cap) {
  DNM_CHECK(keep_size <= L, "more kept spins than spins");
  DNM_CHECK(keep_size <= cap, over_cap, keep_size, keep_size);
  for (int i = 0; i < keep_size; ++i) {
    DNM_CHECK(keep[i] >= 0 && keep[i] < L, "kept spin index %lld out of range [0, %d)", (long long)keep[i], L);
    DNM_CHECK(i == 0 || keep[i] > keep[i - 1], "keep array must be strictly increasing");
  }
  return 0;
}

// widest subspace of a dense reduced density matrix: a condition, not a measurement -- 16 times the 2^36 fetches of the
// widest subspaces a device holds
constexpr int RDM_MAX_SPINS = 40;

int dnm_reduced_density_matrix(const void *x, const dnm_subspace *sub, int keep_size, const int64_t *keep,
                               void *rho, void *stream) {
  DNM_CHECK(x && sub && rho && keep_size >= 0 && (keep_size == 0 || keep), "null argument");
  // every entry of rho sums over the 2^(L - keep_size) traced configurations, whatever the dimension of the subspace
  // (rdm_plan): on a wide subspace of few states (SpinConserve(63, 2): 1953 of them) the call would not end.  The widest
  // subspaces a device holds have 36 spins; refused before anything touches the device
  DNM_CHECK(sub->L <= RDM_MAX_SPINS, "reduced density matrix on L=%lld spins: the kernel fetches 2^L = 2^%lld amplitudes "
            "(2^(L - %d) traced configurations for each of the 2^%d kept ones) whatever the dimension of the subspace; "
            "at most L=%d", (long long)sub->L, (long long)sub->L, keep_size, keep_size, RDM_MAX_SPINS);
  SubOwned s;
  DNM_TRY(s.init(sub, true));
  const int L = s.host.L;
  DNM_TRY(rdm_check_keep(L, keep_size, keep, 15, "reduced density matrix of %d spins (4^%d entries) is too large"));
  RdmGeom geo;
  rdm_geom(L, keep_size, keep, &geo);
  int logtm, ntiles, nsplit;
  int64_t cps;
  size_t pbytes;
  rdm_plan(geo, &logtm, &ntiles, &nsplit, &cps, &pbytes);
  DevBuf big;
  void *scratch = nullptr;
  DNM_TRY(rdm_scratch(pbytes, &big, &scratch, "reduced density matrix", ntiles, 1 << logtm, nsplit));
  DNM_TRY(launch_rdm(x, s.dev, geo, scratch, rho, S(stream)));
  DNM_HIP(hipStreamSynchronize(S(stream)));     // `big` is released on return
  return 0;
}

// ---- sector-resolved reduced density matrix (SpinConserve, XParity over SpinConserve) ------------------------------
// argument checks and the list of feasible blocks, on the host
static int rdm_sector_blocks_of(const dnm_subspace *sub, int keep_size, const int64_t *keep, int xparity_sector,
                                SubView *view, RdmGeom *geo, bool *contig, std::vector<RdmSectorBlock> *blocks) {
  DNM_CHECK(sub && keep_size >= 0 && (keep_size == 0 || keep), "null argument");
  SubView v{};
  DNM_TRY(view_from_c(sub, &v));
  DNM_CHECK(v.type == DNM_SPIN_CONSERVE, "sector-resolved reduced density matrices need a SpinConserve subspace "
            "(type %d given)", v.type);
  const int L = v.L, k = v.k;
  DNM_CHECK(xparity_sector == 0 || xparity_sector == 1 || xparity_sector == -1, "xparity_sector must be 0, +1 or -1");
  DNM_CHECK(xparity_sector == 0 || L == 2 * k, "XParity needs SpinConserve(L, L/2): L=%d, k=%d", L, k);
  DNM_TRY(rdm_check_keep(L, keep_size, keep, 40, "reduced density matrix blocks of %d kept spins: at most 40"));
  rdm_geom(L, keep_size, keep, geo);
  // the kept spins are [0, keep_size): increasing from 0 and ending at keep_size - 1
  *contig = keep_size < L && (keep_size == 0 || keep[keep_size - 1] == keep_size - 1);
  *view = v;
  blocks->clear();
  const int nlo = std::max(0, k - (L - keep_size)), nhi = std::min(k, keep_size);
  for (int n = nlo; n <= nhi; ++n) {
    RdmSectorBlock b{};
    b.n = n;
    b.m = k - n;
    b.dim = v.nchoosek[(int64_t)n * v.ld + keep_size];
    b.traced = v.nchoosek[(int64_t)(k - n) * v.ld + (L - keep_size)];
    DNM_CHECK(b.dim >= 1 && b.dim < ((int64_t)1 << 31), "block n=%d of the reduced density matrix has %lld rows: "
              "2^31 or more", n, (long long)b.dim);
    blocks->push_back(b);
  }
  return 0;
}

int dnm_rdm_sector_plan(const dnm_subspace *sub, int keep_size, const int64_t *keep, int xparity_sector, int *nblocks,
                        int32_t *n_of_block, int64_t *dim_of_block, int64_t *traced_of_block,
                        size_t *scratch_bytes_max) {
  DNM_CHECK(nblocks, "null argument");
  SubView v{};
  RdmGeom geo;
  bool contig;
  std::vector<RdmSectorBlock> blocks;
  DNM_TRY(rdm_sector_blocks_of(sub, keep_size, keep, xparity_sector, &v, &geo, &contig, &blocks));
  *nblocks = (int)blocks.size();
  for (size_t i = 0; i < blocks.size(); ++i) {
    if (n_of_block) n_of_block[i] = blocks[i].n;
    if (dim_of_block) dim_of_block[i] = blocks[i].dim;
    if (traced_of_block) traced_of_block[i] = blocks[i].traced;
  }
  if (scratch_bytes_max) {
    int64_t nt;
    int ns;
    size_t tb, pb;
    DNM_TRY(rdm_sector_plan((int)blocks.size(), blocks.data(), &nt, &ns, &tb, &pb));
    *scratch_bytes_max = tb + pb;
  }
  return 0;
}

int dnm_rdm_sector_blocks(const void *x, const dnm_subspace *sub, int keep_size, const int64_t *keep,
                          int xparity_sector, int nsel, const int32_t *sel_n, void *const *out_ptrs, void *stream) {
  DNM_CHECK(x && nsel >= 1 && sel_n && out_ptrs, "null argument");
  SubView v{};
  RdmGeom geo;
  bool contig;
  std::vector<RdmSectorBlock> all, blocks;
  DNM_TRY(rdm_sector_blocks_of(sub, keep_size, keep, xparity_sector, &v, &geo, &contig, &all));
  DNM_CHECK(v.sc3 == 0, "the sector kernels read the state in reference order (vec_swizzle %d given)", v.sc3);
  for (int i = 0; i < nsel; ++i) {
    const int n = sel_n[i] - all.front().n;
    DNM_CHECK(n >= 0 && n < (int)all.size(), "no block with %d set bits among the kept spins (feasible: %d..%d)",
              (int)sel_n[i], all.front().n, all.back().n);
    DNM_CHECK(out_ptrs[i], "null output for block n=%d", (int)sel_n[i]);
    blocks.push_back(all[(size_t)n]);
    blocks.back().out = out_ptrs[i];
  }
  int64_t ntiles;
  int nsplit;
  size_t tbytes, pbytes;
  DNM_TRY(rdm_sector_plan((int)blocks.size(), blocks.data(), &ntiles, &nsplit, &tbytes, &pbytes));
  const size_t bytes = tbytes + pbytes;
  SubOwned s;
  DNM_TRY(s.init(sub, true));
  DevBuf big;
  void *scratch = nullptr;
  DNM_TRY(rdm_scratch(bytes, &big, &scratch, "reduced density matrix blocks", (long long)ntiles, 64, nsplit));
  DNM_TRY(launch_rdm_sector(x, s.dev, geo, contig, xparity_sector, (int)blocks.size(), blocks.data(), ntiles, nsplit,
                            tbytes, scratch, S(stream)));
  DNM_HIP(hipStreamSynchronize(S(stream)));     // `big` and the subspace tables are released on return
  return 0;
}

// ---- first and second sigma-z moments -----------------------------------------------------------------------------
// what the plans and the calls of the passes over a block of rows (`what`: sigma-z moments, Born sampling) check alike:
// the descriptor, the layout and the rows
static int rows_check(const char *what, const dnm_subspace *sub, int64_t row0, int64_t nrows, SubView *v) {
  DNM_CHECK(sub, "null argument");
  DNM_TRY(view_from_c(sub, v));
  DNM_CHECK(v->sc3 == 0, "%s read a SpinConserve state in reference order (vec_swizzle %d given: "
            "dnm_vec_layout_copy converts)", what, v->sc3);
  DNM_CHECK(sub->site_perm == nullptr, "%s take no relabelled subspace (site_perm given): hand over the "
            "state in reference order with a descriptor without it", what);
  const int64_t dim = sub_dim(*v);
  DNM_CHECK(nrows >= 0 && row0 >= 0 && nrows <= dim && row0 <= dim - nrows,
            "rows [%lld, %lld + %lld) of a subspace of dimension %lld", (long long)row0, (long long)row0,
            (long long)nrows, (long long)dim);
  const int64_t run = (int64_t)1 << v->swz;
  DNM_CHECK(v->swz == 0 || nrows <= run || nrows % run == 0, "a block of %lld rows has no layout of swizzle shift %d: "
            "beyond 2^%d rows the size must be a multiple of 2^%d", (long long)nrows, v->swz, v->swz, v->swz);
  return 0;
}

int dnm_zz_moments_plan(const dnm_subspace *sub, int64_t nrows, int *tile_rows, int *nworkgroups,
                        size_t *scratch_bytes) {
  SubView v{};
  DNM_TRY(rows_check("sigma-z moments", sub, 0, nrows, &v));
  int nb, nwg;
  int64_t per_wg;
  size_t bytes;
  zz_plan(v.L, nrows, &nb, &nwg, &per_wg, &bytes);
  plan_out(nb, 0, nwg, 0, bytes, tile_rows, nullptr, nworkgroups, nullptr, scratch_bytes);
  return 0;
}

int dnm_zz_moments(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, double *out, void *stream) {
  DNM_CHECK(out && (x || nrows == 0), "null argument");
  SubView v{};
  DNM_TRY(rows_check("sigma-z moments", sub, row0, nrows, &v));
  int nb, nwg;
  int64_t per_wg;
  size_t pbytes;
  zz_plan(v.L, nrows, &nb, &nwg, &per_wg, &pbytes);
  const size_t D = (size_t)v.L + 1;
  SubOwned s;
  DNM_TRY(s.init(sub, true));
  DevBuf big;
  void *scratch = nullptr;       // the partial tiles, then the matrix
  DNM_TRY(rdm_scratch(pbytes + D * D * sizeof(double), &big, &scratch, "sigma-z moments", (long long)(nb * (nb + 1) / 2),
                      16, nwg));
  double *m_dev = (double *)((char *)scratch + pbytes);
  DNM_TRY(launch_zz_moments(x, s.dev, row0, nrows, scratch, m_dev, S(stream)));
  // (synchronises: the subspace tables are released on return)
  return dnm_memcpy_d2h(out, m_dev, D * D * sizeof(double), stream);
}

// ---- Born sampling and the power sums of the participation entropies (born.h, born_kernels.hip) -------------------
int dnm_born_plan(const dnm_subspace *sub, int64_t nrows, int64_t *block_rows, int64_t *nblocks, size_t *scratch_bytes) {
  SubView v{};
  DNM_TRY(rows_check("Born sampling passes", sub, 0, nrows, &v));
  int64_t nb, nwg;
  size_t bytes;
  born_plan(nrows, &nb, &nwg, &bytes);
  if (block_rows) *block_rows = BORN_BLOCK_ROWS;
  if (nblocks) *nblocks = nb;
  if (scratch_bytes) *scratch_bytes = bytes;
  return 0;
}

int dnm_born_scan(const double *sums_host, int64_t n, double before, double *scan_host) {
  DNM_CHECK(n >= 0 && (n == 0 || (sums_host && scan_host)), "null argument");
  born_scan(sums_host, n, before, scan_host);
  return 0;
}

int dnm_born_uniforms(uint64_t seed, int64_t shot0, int64_t nshots, double *u_host, uint8_t *flip_host) {
  DNM_CHECK(nshots >= 0 && (u_host || nshots == 0), "null argument");
  for (int64_t s = 0; s < nshots; ++s) {
    uint8_t flip;
    u_host[s] = born_uniform((uint64_t)(shot0 + s), seed, &flip);
    if (flip_host) flip_host[s] = flip;
  }
  return 0;
}

namespace {
// the scanned block sums of a block of rows on the device, with `extra` bytes of scratch behind them for the shots
struct BornScan {
  std::vector<double> host;      // the block sums, then their scan
  DevBuf big;
  double *scan_dev = nullptr;
  char *extra_dev = nullptr;
  int64_t nblocks = 0, last = -1;      // last: the last block that carries weight
  double total = 0.0;                  // the last scan value: `before` + the weight of the rows
};
}  // namespace

// sums_out (host, may be null) gets the block sums.  Synchronises the stream.  for_search: the scan goes back to the
// device; bs->host backs that upload, which is still in flight on return, and lives until the caller's own
// synchronisation.
static int born_scan_rows(const void *x, const SubView &v, int64_t nrows, double before, size_t extra, double *sums_out,
                          bool for_search, BornScan *bs, void *stream) {
  int64_t nwg;
  size_t bytes;
  born_plan(nrows, &bs->nblocks, &nwg, &bytes);
  void *scratch = nullptr;
  DNM_TRY(rdm_scratch(bytes + extra + 8, &bs->big, &scratch, "Born sampling", (long long)bs->nblocks, 32, 1));
  bs->scan_dev = (double *)scratch;
  bs->extra_dev = (char *)scratch + bytes;
  bs->host.resize((size_t)bs->nblocks);
  bs->total = before;
  if (bs->nblocks == 0) return 0;
  DNM_TRY(launch_born_block_sums(x, v.swz, nrows, bs->scan_dev, S(stream)));
  DNM_TRY(dnm_memcpy_d2h(bs->host.data(), bs->scan_dev, bytes, stream));
  if (sums_out) memcpy(sums_out, bs->host.data(), bytes);
  bs->last = born_last_weight(bs->host.data(), bs->nblocks);
  bs->total = born_scan(bs->host.data(), bs->nblocks, before, bs->host.data());
  if (for_search) DNM_HIP(hipMemcpyAsync(bs->scan_dev, bs->host.data(), bytes, hipMemcpyHostToDevice, S(stream)));
  return 0;
}

int dnm_born_block_sums(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, double before,
                        double *sums_host, double *scan_host, void *stream) {
  DNM_CHECK(x || nrows == 0, "null argument");
  DNM_CHECK(before >= 0.0, "the weight in front of a block cannot be negative");
  SubView v{};
  DNM_TRY(rows_check("Born sampling passes", sub, row0, nrows, &v));
  BornScan bs;
  DNM_TRY(born_scan_rows(x, v, nrows, before, 0, sums_host, false, &bs, stream));
  if (scan_host && bs.nblocks) memcpy(scan_host, bs.host.data(), (size_t)bs.nblocks * sizeof(double));
  return 0;
}

int dnm_born_search(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, double before, int final_block,
                    int64_t nshots, const double *targets_host, int64_t *rows_host, void *stream) {
  DNM_CHECK((x || nrows == 0) && nshots >= 0 && (nshots == 0 || (targets_host && rows_host)), "null argument");
  DNM_CHECK(before >= 0.0, "the weight in front of a block cannot be negative");
  SubView v{};
  DNM_TRY(rows_check("Born sampling passes", sub, row0, nrows, &v));
  const size_t sbytes = (size_t)nshots * 8;
  BornScan bs;
  DNM_TRY(born_scan_rows(x, v, nrows, before, 2 * sbytes, nullptr, true, &bs, stream));
  double *t_dev = (double *)bs.extra_dev;
  int64_t *r_dev = (int64_t *)(bs.extra_dev + sbytes);
  if (nshots) DNM_HIP(hipMemcpyAsync(t_dev, targets_host, sbytes, hipMemcpyHostToDevice, S(stream)));
  BornSearch p{};
  p.row0 = row0;
  p.nrows = nrows;
  p.nblocks = bs.nblocks;
  p.nshots = nshots;
  p.before = before;
  p.clamp_block = final_block ? bs.last : -1;
  p.targets_dev = t_dev;
  DNM_TRY(launch_born_search(x, v.swz, bs.scan_dev, p, r_dev, nullptr, S(stream)));
  // (synchronises: the host scan and `big` are released on return)
  return dnm_memcpy_d2h(rows_host, r_dev, sbytes, stream);
}

int dnm_born_sample(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, uint64_t seed, int64_t shot0,
                    int64_t nshots, int64_t *rows_host, uint8_t *flip_host, void *stream) {
  DNM_CHECK((x || nrows == 0) && nshots >= 0 && shot0 >= 0 && (nshots == 0 || rows_host), "null argument");
  SubView v{};
  DNM_TRY(rows_check("Born sampling passes", sub, row0, nrows, &v));
  const size_t sbytes = (size_t)nshots * 8;
  BornScan bs;
  DNM_TRY(born_scan_rows(x, v, nrows, 0.0, sbytes + (size_t)nshots, nullptr, true, &bs, stream));
  int64_t *r_dev = (int64_t *)bs.extra_dev;
  uint8_t *f_dev = (uint8_t *)(bs.extra_dev + sbytes);
  BornSearch p{};
  p.row0 = row0;
  p.nrows = nrows;
  p.nblocks = bs.nblocks;
  p.nshots = nshots;
  p.clamp_block = bs.last;
  p.seed = seed;
  p.shot0 = shot0;
  p.total = bs.total;
  DNM_TRY(launch_born_search(x, v.swz, bs.scan_dev, p, r_dev, f_dev, S(stream)));
  if (flip_host && nshots) DNM_HIP(hipMemcpyAsync(flip_host, f_dev, (size_t)nshots, hipMemcpyDeviceToHost, S(stream)));
  // (synchronises: the host scan and `big` are released on return)
  return dnm_memcpy_d2h(rows_host, r_dev, sbytes, stream);
}

int dnm_vec_power_sums(const void *x, int64_t n, int nq, const double *q_host, double *out_host, void *stream) {
  DNM_CHECK((x || n == 0) && n >= 0 && out_host && nq >= 0 && (nq == 0 || q_host), "null argument");
  DNM_CHECK(nq <= BORN_MAX_Q, "%d exponents in one pass: at most %d", nq, BORN_MAX_Q);
  for (int k = 0; k < nq; ++k)
    DNM_CHECK(q_host[k] > 0.0 && q_host[k] < 1e300, "exponent %g: the power sums take finite q > 0", q_host[k]);
  const int64_t nwg = born_power_workgroups(n);
  const size_t bytes = (size_t)nwg * BORN_NSUMS * sizeof(double);
  DevBuf big;
  void *scratch = nullptr;
  DNM_TRY(rdm_scratch(bytes, &big, &scratch, "power sums", (long long)nwg, 1, 1));
  DNM_TRY(launch_born_power_sums(x, n, nq, q_host, (double *)scratch, S(stream)));
  std::vector<double> part((size_t)nwg * BORN_NSUMS);
  DNM_TRY(dnm_memcpy_d2h(part.data(), scratch, bytes, stream));
  double all[BORN_NSUMS];
  born_power_reduce(part.data(), nwg, all);
  for (int k = 0; k < nq; ++k) out_host[k] = all[k];
  for (int c = 0; c < 4; ++c) out_host[nq + c] = all[BORN_MAX_Q + c];
  return 0;
}

// ---- sigma+ sigma- moments ----------------------------------------------------------------------------------------
// what the plan, the call and the partner table check alike, before any device call.  The pass brings its own
// binomials (sector k + 1), so that the descriptor's fields are read here and nothing else of it is used.
static int pm_check(const dnm_subspace *sub, const char *what) {
  DNM_CHECK(sub, "%s: null subspace descriptor", what);
  DNM_CHECK(sub->type != DNM_EXPLICIT, "%s: Explicit subspaces are not supported (the partners of a row have no "
            "closed-form index there)", what);
  DNM_CHECK(sub->type == DNM_FULL || sub->type == DNM_PARITY || sub->type == DNM_SPIN_CONSERVE,
            "%s: unknown subspace type %d", what, sub->type);
  DNM_CHECK(sub->L >= 1 && sub->L <= 64, "%s: L=%lld out of range (at most 64 spins)", what, (long long)sub->L);
  if (sub->type == DNM_SPIN_CONSERVE) {
    DNM_CHECK(sub->k >= 0 && sub->k <= sub->L, "%s: bad SpinConserve descriptor (k=%lld)", what, (long long)sub->k);
    DNM_CHECK(sub->vec_swizzle == 0, "%s: a SpinConserve state is read in reference order (vec_swizzle %d given: "
              "dnm_vec_layout_copy converts)", what, sub->vec_swizzle);
    DNM_CHECK(sub->site_perm == nullptr, "%s: no relabelled subspace (site_perm given): hand over the state in "
              "reference order with a descriptor without it", what);
  } else {
    DNM_CHECK(sub->site_perm == nullptr, "%s: site_perm given for a subspace that is not SpinConserve", what);
    DNM_CHECK(sub->vec_swizzle == 0 || (sub->vec_swizzle >= 5 && sub->vec_swizzle <= 24),
              "%s: vec_swizzle %d: the shift of a swizzled vector lies in [5, 24]", what, sub->vec_swizzle);
    if (sub->type == DNM_PARITY) DNM_CHECK(sub->space == 0 || sub->space == 1, "%s: parity space must be 0 or 1", what);
  }
  return 0;
}

int dnm_pm_moments_plan(const dnm_subspace *sub, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                        size_t *lds_bytes, size_t *scratch_bytes) {
  DNM_TRY(pm_check(sub, "sigma+ sigma- moments"));
  GramPlan p;
  DNM_TRY(pm_plan(sub->type, (int)sub->L, (int)sub->k, &p));
  plan_out(p.nb, p.B, p.nwg, p.lds_bytes, p.partial_bytes, tile_rows, panel_rows_log2, nworkgroups, lds_bytes,
           scratch_bytes);
  return 0;
}

int dnm_pm_moments(const void *x, const dnm_subspace *sub, double *out, void *stream) {
  DNM_CHECK(x && out, "sigma+ sigma- moments: null argument");
  DNM_TRY(pm_check(sub, "sigma+ sigma- moments"));
  const int L = (int)sub->L;
  GramPlan p;
  DNM_TRY(pm_plan(sub->type, L, (int)sub->k, &p));
  if (p.nrows == 0) {       // SpinConserve(L, L): no configuration has a spin left to lower
    memset(out, 0, (size_t)L * (size_t)L * 2 * sizeof(double));
    return 0;
  }
  return gram_moments(p, L, (size_t)L, "sigma+ sigma- moments", out, stream,
                      [&](int64_t *table, void *partial, void *P) {
    return launch_pm_moments(x, sub->type, L, (int)sub->k, (int)sub->space, sub->vec_swizzle, p, table, partial, P,
                             S(stream));
  });
}

int dnm_pm_partner_indices(const dnm_subspace *sub, int64_t n, const int64_t *rows, int64_t *out) {
  DNM_TRY(pm_check(sub, "sigma+ sigma- partner indices"));
  DNM_CHECK(sub->type == DNM_SPIN_CONSERVE, "sigma+ sigma- partner indices: SpinConserve only (Full and Parity "
            "partners are index ^ mask)");
  DNM_CHECK(n >= 0 && (n == 0 || (rows && out)), "sigma+ sigma- partner indices: null argument");
  const int L = (int)sub->L;
  GramPlan p;
  DNM_TRY(pm_plan(sub->type, L, (int)sub->k, &p));
  std::vector<int64_t> nck((size_t)(p.K + 1) * (size_t)(L + 1));
  if (p.nrows) pm_binomials(L, p.K, L + 1, nck.data());
  for (int64_t i = 0; i < n; ++i) {
    DNM_CHECK(rows[i] >= 0 && rows[i] < p.nrows, "sigma+ sigma- partner indices: row %lld of a sector of %lld rows "
              "(%d set bits)", (long long)rows[i], (long long)p.nrows, p.K);
    int64_t *o = out + i * L;
    for (int j = 0; j < L; ++j) o[j] = -1;
    pm_partners(pm_unrank(rows[i], L, p.K, nck.data(), L + 1), nck.data(), L + 1,
                [&](int j, int64_t idx) { o[j] = idx; });
  }
  return 0;
}

// ---- bond-swap moments --------------------------------------------------------------------------------------------
// what the bond-swap and the rotation pass check alike of the subspace and the sector, before any device call
static int swap_check_subspace(const dnm_subspace *sub, int xsec, const char *what) {
  DNM_TRY(pm_check(sub, what));
  DNM_CHECK(xsec == 0 || xsec == 1 || xsec == -1, "%s: xparity_sector %d (0, +1 or -1)", what, xsec);
  if (xsec != 0) {
    DNM_CHECK(sub->L >= 2, "%s: an XParity sector of L=%lld", what, (long long)sub->L);
    if (sub->type == DNM_PARITY)
      DNM_CHECK(sub->L % 2 == 0, "%s: Parity carries the global flip of XParity only when L is even (L=%lld)", what,
                (long long)sub->L);
    if (sub->type == DNM_SPIN_CONSERVE)
      DNM_CHECK(sub->L == 2 * sub->k, "%s: SpinConserve carries the global flip of XParity only when k = L / 2 "
                "(L=%lld, k=%lld)", what, (long long)sub->L, (long long)sub->k);
  }
  return 0;
}

// what the plan, the call and the partner table check alike, before any device call (bonds: null for the plan)
static int swap_check(const dnm_subspace *sub, int xsec, int nbonds, const int32_t *bonds) {
  const char *what = "bond-swap moments";
  DNM_TRY(swap_check_subspace(sub, xsec, what));
  DNM_CHECK(nbonds >= 1 && nbonds <= 63, "%s: %d bonds (1 to 63 in one call)", what, nbonds);
  for (int m = 0; bonds && m < nbonds; ++m) {
    const int a = bonds[2 * m], b = bonds[2 * m + 1];
    DNM_CHECK(a >= 0 && a < sub->L && b >= 0 && b < sub->L, "%s: bond %d = (%d, %d) has a site outside [0, %lld)", what,
              m, a, b, (long long)sub->L);
    DNM_CHECK(a != b, "%s: bond %d joins site %d to itself", what, m, a);
  }
  return 0;
}

int dnm_swap_moments_plan(const dnm_subspace *sub, int nbonds, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                          size_t *lds_bytes, size_t *scratch_bytes) {
  DNM_TRY(swap_check(sub, 0, nbonds, nullptr));
  GramPlan p;
  DNM_TRY(swap_plan(sub->type, (int)sub->L, (int)sub->k, nbonds, 0, &p));
  plan_out(p.nb, p.B, p.nwg, p.lds_bytes, p.partial_bytes, tile_rows, panel_rows_log2, nworkgroups, lds_bytes,
           scratch_bytes);
  return 0;
}

int dnm_swap_moments(const void *x, const dnm_subspace *sub, int xparity_sector, int nbonds, const int32_t *bonds,
                     double *out, void *stream) {
  DNM_CHECK(x && out && bonds, "bond-swap moments: null argument");
  DNM_TRY(swap_check(sub, xparity_sector, nbonds, bonds));
  const int L = (int)sub->L;
  GramPlan p;
  DNM_TRY(swap_plan(sub->type, L, (int)sub->k, nbonds, xparity_sector, &p));
  return gram_moments(p, L, (size_t)nbonds + 1, "bond-swap moments", out, stream,
                      [&](int64_t *table, void *partial, void *G) {
    return launch_swap_moments(x, sub->type, L, (int)sub->space, sub->vec_swizzle, xparity_sector, nbonds, bonds, p,
                               table, partial, G, S(stream));
  });
}

int dnm_swap_partner_indices(const dnm_subspace *sub, int xparity_sector, int nbonds, const int32_t *bonds, int64_t n,
                             const int64_t *rows, int64_t *idx, int8_t *sign) {
  DNM_CHECK(bonds, "bond-swap partner indices: null argument");
  DNM_TRY(swap_check(sub, xparity_sector, nbonds, bonds));
  DNM_CHECK(n >= 0 && (n == 0 || (rows && idx && sign)), "bond-swap partner indices: null argument");
  const int L = (int)sub->L;
  GramPlan p;
  DNM_TRY(swap_plan(sub->type, L, (int)sub->k, nbonds, xparity_sector, &p));
  const bool sc = sub->type == DNM_SPIN_CONSERVE, parity = sub->type == DNM_PARITY;
  std::vector<int64_t> nck;
  if (sc) {
    nck.resize((size_t)(p.K + 1) * (size_t)(L + 1));
    pm_binomials(L, p.K, L + 1, nck.data());
  }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t row = rows[i];
    DNM_CHECK(row >= 0 && row < p.nrows, "bond-swap partner indices: row %lld of %lld rows", (long long)row,
              (long long)p.nrows);
    const uint64_t cfg = sc ? pm_unrank(row, L, p.K, nck.data(), L + 1)
                         : parity ? ((uint64_t)row << 1) | (uint64_t)(hd_par((uint64_t)row) ^ (int)sub->space)
                                  : (uint64_t)row;
    for (int m = 0; m < nbonds; ++m) {
      const int a = bonds[2 * m], b = bonds[2 * m + 1];
      int fl = 0;
      int64_t at = row;
      if (sc) {
        at = swap_sc_partner(cfg, row, a, b, L, p.dim, xparity_sector, nck.data(), L + 1, &fl);
      } else if (((cfg >> a) ^ (cfg >> b)) & 1) {
        at = row ^ (int64_t)swap_index_mask(parity, L, a, b, xparity_sector, &fl);
      }
      idx[i * nbonds + m] = at;
      sign[i * nbonds + m] = (int8_t)(fl ? xparity_sector : 1);
    }
  }
  return 0;
}

// ---- three-site rotation (scalar chirality) moments ------------------------------------------------------------------
// what the plan, the call and the partner table check alike, before any device call (cycles: null for the plan)
static int cyc_check(const dnm_subspace *sub, int xsec, int ncycles, const int32_t *cycles) {
  const char *what = "chirality moments";
  DNM_TRY(swap_check_subspace(sub, xsec, what));
  DNM_CHECK(ncycles >= 1 && ncycles <= 63, "%s: %d cycles (1 to 63 in one call)", what, ncycles);
  for (int m = 0; cycles && m < ncycles; ++m) {
    const int a = cycles[3 * m], b = cycles[3 * m + 1], c = cycles[3 * m + 2];
    DNM_CHECK(a >= 0 && a < sub->L && b >= 0 && b < sub->L && c >= 0 && c < sub->L,
              "%s: cycle %d = (%d, %d, %d) has a site outside [0, %lld)", what, m, a, b, c, (long long)sub->L);
    DNM_CHECK(a != b && b != c && c != a, "%s: the sites of cycle %d = (%d, %d, %d) are not pairwise distinct", what, m,
              a, b, c);
  }
  return 0;
}

int dnm_cyc_moments_plan(const dnm_subspace *sub, int ncycles, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                         size_t *lds_bytes, size_t *scratch_bytes) {
  DNM_TRY(cyc_check(sub, 0, ncycles, nullptr));
  GramPlan p;
  DNM_TRY(swap_plan(sub->type, (int)sub->L, (int)sub->k, ncycles, 0, &p, "chirality"));
  plan_out(p.nb, p.B, p.nwg, p.lds_bytes, p.partial_bytes, tile_rows, panel_rows_log2, nworkgroups, lds_bytes,
           scratch_bytes);
  return 0;
}

int dnm_cyc_moments(const void *x, const dnm_subspace *sub, int xparity_sector, int ncycles, const int32_t *cycles,
                    double *out, void *stream) {
  DNM_CHECK(x && out && cycles, "chirality moments: null argument");
  DNM_TRY(cyc_check(sub, xparity_sector, ncycles, cycles));
  const int L = (int)sub->L;
  GramPlan p;
  DNM_TRY(swap_plan(sub->type, L, (int)sub->k, ncycles, xparity_sector, &p, "chirality"));
  return gram_moments(p, L, (size_t)ncycles + 1, "chirality moments", out, stream,
                      [&](int64_t *table, void *partial, void *G) {
    return launch_cyc_moments(x, sub->type, L, (int)sub->space, sub->vec_swizzle, xparity_sector, ncycles, cycles, p,
                              table, partial, G, S(stream));
  });
}

int dnm_cyc_partner_indices(const dnm_subspace *sub, int xparity_sector, int ncycles, const int32_t *cycles, int64_t n,
                            const int64_t *rows, int64_t *idx, int8_t *sign) {
  DNM_CHECK(cycles, "chirality partner indices: null argument");
  DNM_TRY(cyc_check(sub, xparity_sector, ncycles, cycles));
  DNM_CHECK(n >= 0 && (n == 0 || (rows && idx && sign)), "chirality partner indices: null argument");
  const int L = (int)sub->L;
  GramPlan p;
  DNM_TRY(swap_plan(sub->type, L, (int)sub->k, ncycles, xparity_sector, &p, "chirality"));
  const bool sc = sub->type == DNM_SPIN_CONSERVE, parity = sub->type == DNM_PARITY;
  std::vector<int64_t> nck;
  if (sc) {
    nck.resize((size_t)(p.K + 1) * (size_t)(L + 1));
    pm_binomials(L, p.K, L + 1, nck.data());
  }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t row = rows[i];
    DNM_CHECK(row >= 0 && row < p.nrows, "chirality partner indices: row %lld of %lld rows", (long long)row,
              (long long)p.nrows);
    const uint64_t cfg = sc ? pm_unrank(row, L, p.K, nck.data(), L + 1)
                         : parity ? ((uint64_t)row << 1) | (uint64_t)(hd_par((uint64_t)row) ^ (int)sub->space)
                                  : (uint64_t)row;
    for (int m = 0; m < ncycles; ++m) {
      const int a = cycles[3 * m], b = cycles[3 * m + 1], c = cycles[3 * m + 2];
      int fl = 0;
      int64_t at;
      if (sc) {
        at = cyc_sc_partner(cfg, row, a, b, c, L, p.dim, xparity_sector, nck.data(), L + 1, &fl);
      } else {
        int pp, qq;
        const int d = cyc_changed(cfg, a, b, c, &pp, &qq);
        fl = cyc_flipped(d, a, b, c, L, xparity_sector);
        at = cyc_xor_partner(row, d, fl, cyc_site_mask(parity, a), cyc_site_mask(parity, b), cyc_site_mask(parity, c),
                             cyc_all_mask(parity, L));
      }
      idx[i * ncycles + m] = at;
      sign[i * ncycles + m] = (int8_t)(fl ? xparity_sector : 1);
    }
  }
  return 0;
}

// ---- two-spin Pauli moments ---------------------------------------------------------------------------------------
// what the plan, the call and the partner table check alike, before any device call (cols: null for the plan)
static int pauli_check(const dnm_subspace *sub, int ncols, const int32_t *cols) {
  const char *what = "Pauli moments";
  DNM_CHECK(sub, "%s: null subspace descriptor", what);
  DNM_CHECK(sub->type != DNM_EXPLICIT, "%s: Explicit subspaces are not supported (a flipped row may lie outside the "
            "subspace)", what);
  DNM_CHECK(sub->type != DNM_SPIN_CONSERVE, "%s: SpinConserve subspaces are not supported: a flip leaves the sector "
            "(dnm_zz_moments and dnm_pm_moments hold every correlator that does not vanish there)", what);
  DNM_CHECK(sub->type == DNM_FULL || sub->type == DNM_PARITY, "%s: unknown subspace type %d", what, sub->type);
  DNM_CHECK(sub->L >= 1 && sub->L <= 64, "%s: L=%lld out of range (at most 64 spins)", what, (long long)sub->L);
  const int bits = (int)sub->L - (sub->type == DNM_PARITY);
  DNM_CHECK(bits <= 62, "%s: %d index bits (2^%d rows): at most 62", what, bits, bits);
  DNM_CHECK(sub->site_perm == nullptr, "%s: site_perm given for a subspace that is not SpinConserve", what);
  DNM_CHECK(sub->vec_swizzle == 0 || (sub->vec_swizzle >= 5 && sub->vec_swizzle <= 24),
            "%s: vec_swizzle %d: the shift of a swizzled vector lies in [5, 24]", what, sub->vec_swizzle);
  if (sub->type == DNM_PARITY) DNM_CHECK(sub->space == 0 || sub->space == 1, "%s: parity space must be 0 or 1", what);
  DNM_CHECK(ncols >= 1 && ncols <= 63, "%s: %d columns (1 to 63 in one call)", what, ncols);
  for (int c = 0; cols && c < ncols; ++c) {
    const int site = cols[2 * c], kind = cols[2 * c + 1];
    DNM_CHECK(site >= 0 && site < sub->L, "%s: column %d has site %d outside [0, %lld)", what, c, site,
              (long long)sub->L);
    DNM_CHECK(kind >= PAULI_X && kind <= PAULI_Z, "%s: column %d has kind %d (1 flip, 2 flip and sign, 3 sign)", what, c,
              kind);
  }
  return 0;
}

int dnm_pauli_moments_plan(const dnm_subspace *sub, int ncols, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                           size_t *lds_bytes, size_t *scratch_bytes) {
  DNM_TRY(pauli_check(sub, ncols, nullptr));
  GramPlan p;
  // (the bond-swap sweep's panel rule and workgroup count: inherited, not measured for this fill)
  DNM_TRY(swap_plan(sub->type, (int)sub->L, 0, ncols, 0, &p, "Pauli"));
  plan_out(p.nb, p.B, p.nwg, p.lds_bytes, p.partial_bytes, tile_rows, panel_rows_log2, nworkgroups, lds_bytes,
           scratch_bytes);
  return 0;
}

int dnm_pauli_moments(const void *x, const dnm_subspace *sub, int ncols, const int32_t *cols, double *out,
                      void *stream) {
  DNM_CHECK(x && out && cols, "Pauli moments: null argument");
  DNM_TRY(pauli_check(sub, ncols, cols));
  const int L = (int)sub->L;
  GramPlan p;
  DNM_TRY(swap_plan(sub->type, L, 0, ncols, 0, &p, "Pauli"));
  DNM_TRY(gram_moments(p, L, (size_t)ncols + 1, "Pauli moments", out, stream,
                       [&](int64_t *, void *partial, void *G) {
    return launch_pauli_moments(x, sub->type, L, (int)sub->space, sub->vec_swizzle, ncols, cols, p, partial, G,
                                S(stream));
  }));
  if (sub->type == DNM_PARITY) {
    // a flipping column holds the rows of the opposite sector: its products with the columns that do not flip (the
    // state's own among them) vanish by symmetry
    const size_t D = (size_t)ncols + 1;
    auto flips = [&](size_t col) { return col > 0 && pauli_flips(cols[2 * (col - 1) + 1]); };
    for (size_t i = 0; i < D; ++i)
      for (size_t j = 0; j < D; ++j)
        if (flips(i) != flips(j)) out[2 * (i * D + j)] = out[2 * (i * D + j) + 1] = 0.0;
  }
  return 0;
}

int dnm_pauli_partner_indices(const dnm_subspace *sub, int ncols, const int32_t *cols, int64_t n, const int64_t *rows,
                              int64_t *idx, int8_t *sign) {
  DNM_CHECK(cols, "Pauli partner indices: null argument");
  DNM_TRY(pauli_check(sub, ncols, cols));
  DNM_CHECK(n >= 0 && (n == 0 || (rows && idx && sign)), "Pauli partner indices: null argument");
  const bool parity = sub->type == DNM_PARITY;
  const int64_t nrows = (int64_t)1 << ((int)sub->L - (parity ? 1 : 0));
  for (int64_t i = 0; i < n; ++i) {
    const int64_t row = rows[i];
    DNM_CHECK(row >= 0 && row < nrows, "Pauli partner indices: row %lld of %lld rows", (long long)row,
              (long long)nrows);
    const int par = hd_par((uint64_t)row);
    for (int c = 0; c < ncols; ++c) {
      const int site = cols[2 * c], kind = cols[2 * c + 1];
      const uint64_t cfg = pauli_row_config(parity, (int)sub->space, (uint64_t)row, par, pauli_flips(kind));
      idx[i * ncols + c] = row ^ (int64_t)pauli_index_mask(parity, site, kind);
      sign[i * ncols + c] = (int8_t)(pauli_negative(cfg, site, kind) ? -1 : 1);
    }
  }
  return 0;
}

// ---- site permutations ----------------------------------------------------------------------------------------------
// what the plan, the calls and the partner table check alike, before any device call (perms: null for the plan)
static int perm_check(const dnm_subspace *sub, int xsec, int nperm, const int32_t *perms, PermPlan *p,
                      std::vector<unsigned char> *tables) {
  const char *what = "site permutations";
  DNM_TRY(swap_check_subspace(sub, xsec, what));
  DNM_CHECK(nperm >= 1 && nperm <= PERM_MAX, "%s: %d permutations (1 to %d in one call)", what, nperm, PERM_MAX);
  DNM_TRY(perm_plan(sub->type, (int)sub->L, (int)sub->k, nperm, xsec, p));
  if (perms) {
    tables->resize(p->lds_bytes);
    int bad = 0;
    DNM_CHECK(perm_fill_tables(*p, (int)sub->L, nperm, perms, tables->data(), &bad),
              "%s: permutation %d is not a bijection of [0, %lld)", what, bad, (long long)sub->L);
  }
  return 0;
}

int dnm_perm_plan(const dnm_subspace *sub, int nperm, int *nworkgroups, size_t *lds_bytes, size_t *scratch_bytes) {
  PermPlan p;
  DNM_TRY(perm_check(sub, 0, nperm, nullptr, &p, nullptr));
  plan_out(0, 0, p.nwg, p.lds_bytes, p.lds_bytes + p.partial_bytes + 2 * (size_t)nperm * sizeof(double), nullptr,
           nullptr, nworkgroups, lds_bytes, scratch_bytes);
  return 0;
}

int dnm_perm_partner_indices(const dnm_subspace *sub, int xparity_sector, int nperm, const int32_t *perms, int64_t n,
                             const int64_t *rows, int64_t *idx, int8_t *sign) {
  DNM_CHECK(perms, "site permutation partner indices: null argument");
  PermPlan p;
  std::vector<unsigned char> tables;
  DNM_TRY(perm_check(sub, xparity_sector, nperm, perms, &p, &tables));
  DNM_CHECK(n >= 0 && (n == 0 || (rows && idx && sign)), "site permutation partner indices: null argument");
  const int L = (int)sub->L, swz = sub->vec_swizzle;
  const bool sc = sub->type == DNM_SPIN_CONSERVE, parity = sub->type == DNM_PARITY;
  const int64_t *tab = reinterpret_cast<const int64_t *>(tables.data());
  for (int64_t i = 0; i < n; ++i) {
    const int64_t row = rows[i];
    DNM_CHECK(row >= 0 && row < p.nrows, "site permutation partner indices: row %lld of %lld rows", (long long)row,
              (long long)p.nrows);
    const uint64_t cfg = sc ? pm_unrank(row, L, p.K, tab, L + 1)
                            : perm_index_config(parity, (int)sub->space, (uint64_t)vec_pos(row, swz));
    for (int g = 0; g < nperm; ++g) {
      const uint64_t src = perm_source(cfg, tables.data() + (size_t)p.ntab * 8 + (size_t)g * PERM_LD);
      int fl = 0;
      idx[i * nperm + g] = sc ? perm_sc_index(src, L, p.dim, xparity_sector, tab, L + 1, &fl)
                              : vec_pos(perm_xor_index(src, parity, L, xparity_sector, &fl), swz);
      sign[i * nperm + g] = (int8_t)(fl ? xparity_sector : 1);
    }
  }
  return 0;
}

// scratch of a call ([tables | partial sums | result]) with the tables uploaded
static int perm_scratch(const PermPlan &p, const std::vector<unsigned char> &tables, size_t more, DevBuf *big,
                        void **scratch, void *stream) {
  DNM_TRY(rdm_scratch(p.lds_bytes + more, big, scratch, "site permutations", 0, 0, p.nwg));
  DNM_HIP(hipMemcpyAsync(*scratch, tables.data(), p.lds_bytes, hipMemcpyHostToDevice, S(stream)));
  return 0;
}

int dnm_perm_apply(const void *x, void *y, const dnm_subspace *sub, int xparity_sector, int nperm, const int32_t *perms,
                   const double *coef, int accumulate, void *stream) {
  DNM_CHECK(x && y && perms && coef, "site permutations: null argument");
  DNM_CHECK(x != y, "site permutations: x and y are the same vector (the pass gathers: the result needs its own)");
  PermPlan p;
  std::vector<unsigned char> tables;
  DNM_TRY(perm_check(sub, xparity_sector, nperm, perms, &p, &tables));
  DevBuf big;
  void *scratch = nullptr;
  DNM_TRY(perm_scratch(p, tables, 0, &big, &scratch, stream));
  DNM_TRY(launch_perm_apply(x, y, sub->type, (int)sub->L, (int)sub->space, sub->vec_swizzle, xparity_sector, nperm, coef,
                            accumulate != 0, p, scratch, S(stream)));
  DNM_HIP(hipStreamSynchronize(S(stream)));     // the host tables and `big` are released on return
  return 0;
}

int dnm_perm_dots(const void *phi, const void *psi, const dnm_subspace *sub, int xparity_sector, int nperm,
                  const int32_t *perms, double *out, void *stream) {
  DNM_CHECK(phi && psi && perms && out, "site permutations: null argument");
  PermPlan p;
  std::vector<unsigned char> tables;
  DNM_TRY(perm_check(sub, xparity_sector, nperm, perms, &p, &tables));
  const size_t obytes = 2 * (size_t)nperm * sizeof(double);
  DevBuf big;
  void *scratch = nullptr;
  DNM_TRY(perm_scratch(p, tables, p.partial_bytes + obytes, &big, &scratch, stream));
  void *partial = (char *)scratch + p.lds_bytes, *o_dev = (char *)partial + p.partial_bytes;
  DNM_TRY(launch_perm_dots(phi, psi, sub->type, (int)sub->L, (int)sub->space, sub->vec_swizzle, xparity_sector, nperm, p,
                           scratch, partial, o_dev, S(stream)));
  // (synchronises: the host tables and `big` are released on return)
  return dnm_memcpy_d2h(out, o_dev, obytes, stream);
}

// ---- subspace maps and sector weights (submap.h, submap_kernels.hip) -----------------------------------------------
// one side of a map, or the subspace of the sector weights: what every entry point checks, before any device call
static int submap_check_side(const dnm_subspace *sub, int xsec, const char *what, const char *side, SubView *v) {
  DNM_CHECK(sub->type == DNM_FULL || sub->type == DNM_PARITY || sub->type == DNM_EXPLICIT ||
            sub->type == DNM_SPIN_CONSERVE, "%s: unknown subspace type %d%s", what, sub->type, side);
  DNM_CHECK(sub->L >= 1 && sub->L <= 63, "%s: L=%lld out of range%s (1 to 63 spins)", what, (long long)sub->L, side);
  DNM_CHECK(sub->type != DNM_FULL || sub->L <= 62, "%s: 2^%lld rows%s (at most 62 index bits)", what, (long long)sub->L,
            side);
  DNM_CHECK(sub->site_perm == nullptr, "%s: no relabelled subspace%s (site_perm given): hand over the state in "
            "reference order with a descriptor without it", what, side);
  if (sub->type == DNM_SPIN_CONSERVE)
    DNM_CHECK(sub->vec_swizzle == 0, "%s: a SpinConserve state is read and written in reference order%s (vec_swizzle %d "
              "given: dnm_vec_layout_copy converts)", what, side, sub->vec_swizzle);
  else if (sub->type == DNM_EXPLICIT)
    DNM_CHECK(sub->vec_swizzle == 0, "%s: vec_swizzle %d on an Explicit subspace%s", what, sub->vec_swizzle, side);
  else
    DNM_CHECK(sub->vec_swizzle == 0 || (sub->vec_swizzle >= 5 && sub->vec_swizzle <= 24),
              "%s: vec_swizzle %d%s: the shift of a swizzled vector lies in [5, 24]", what, sub->vec_swizzle, side);
  DNM_CHECK(xsec == 0 || xsec == 1 || xsec == -1, "%s: xparity sector %d%s (0, +1 or -1)", what, xsec, side);
  DNM_TRY(view_from_c(sub, v));
  if (xsec != 0) {
    if (sub->type == DNM_PARITY)
      DNM_CHECK(sub->L % 2 == 0, "%s: Parity carries the global flip of XParity only when L is even (L=%lld)%s", what,
                (long long)sub->L, side);
    if (sub->type == DNM_SPIN_CONSERVE)
      DNM_CHECK(sub->L == 2 * sub->k, "%s: SpinConserve carries the global flip of XParity only when k = L / 2 "
                "(L=%lld, k=%lld)%s", what, (long long)sub->L, (long long)sub->k, side);
    if (sub->type == DNM_EXPLICIT) {
      DNM_CHECK(sub->dim % 2 == 0, "%s: an Explicit subspace of odd dimension %lld carries no XParity sector%s", what,
                (long long)sub->dim, side);
      // (the whole closure check is XParity's constructor's; here: the halves meet where they should)
      const int64_t h = sub->dim / 2;
      DNM_CHECK(((sub->state_map[h - 1] >> (sub->L - 1)) & 1) == 0 && ((sub->state_map[h] >> (sub->L - 1)) & 1) == 1,
                "%s: an XParity sector over an Explicit subspace needs the representatives (spin L-1 up) in the first "
                "half of the list and their complements in the second%s", what, side);
    }
  }
  return 0;
}

static int submap_check(const dnm_subspace *src, int src_sector, const dnm_subspace *dst, int dst_sector, SubView *sv,
                        SubView *dv) {
  const char *what = "subspace map";
  DNM_CHECK(src && dst, "%s: null subspace descriptor", what);
  DNM_TRY(submap_check_side(src, src_sector, what, " (source)", sv));
  DNM_TRY(submap_check_side(dst, dst_sector, what, " (target)", dv));
  DNM_CHECK(src->L == dst->L, "%s: the source has L=%lld spins, the target L=%lld", what, (long long)src->L,
            (long long)dst->L);
  return 0;
}

int dnm_subspace_map_plan(const dnm_subspace *src, int src_sector, const dnm_subspace *dst, int dst_sector,
                          int64_t *src_rows, int64_t *dst_rows, int *run, int *nworkgroups, size_t *lds_bytes) {
  SubView sv{}, dv{};
  DNM_TRY(submap_check(src, src_sector, dst, dst_sector, &sv, &dv));
  SubmapPlan p;
  DNM_TRY(submap_plan(sv, src_sector, dv, dst_sector, &p));
  if (src_rows) *src_rows = p.src.rows;
  if (dst_rows) *dst_rows = p.dst.rows;
  if (run) *run = p.run;
  if (nworkgroups) *nworkgroups = p.nwg;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

int dnm_subspace_map_indices(const dnm_subspace *src, int src_sector, const dnm_subspace *dst, int dst_sector,
                             int64_t n, const int64_t *rows, int64_t *idx, int8_t *sign, double *scale) {
  SubView sv{}, dv{};
  DNM_TRY(submap_check(src, src_sector, dst, dst_sector, &sv, &dv));
  DNM_CHECK(n >= 0 && (n == 0 || (rows && idx && sign)), "subspace map indices: null argument");
  SubOwned s, d;           // (host only: the bucket table of an Explicit side as the kernel has it)
  DNM_TRY(s.init(src, false));
  DNM_TRY(d.init(dst, false));
  SubmapPlan p;
  DNM_TRY(submap_plan(s.host, src_sector, d.host, dst_sector, &p));
  if (scale) *scale = submap_scale(p.mode);
  for (int64_t i = 0; i < n; ++i)
    DNM_CHECK(rows[i] >= 0 && rows[i] < p.dst.rows, "subspace map indices: row %lld of %lld rows", (long long)rows[i],
              (long long)p.dst.rows);
  return submap_dispatch(sv.type, dv.type, [&](auto S, auto D) {
    for (int64_t i = 0; i < n; ++i) {
      SubmapTerms t;
      submap_terms<decltype(S)::value>(submap_row_config<decltype(D)::value>(rows[i], p.dst.v), p.src, dst_sector, &t);
      for (int m = 0; m < 2; ++m) {
        idx[2 * i + m] = t.idx[m];
        sign[2 * i + m] = (int8_t)t.sign[m];
      }
    }
    return 0;
  });
}

int dnm_subspace_map_apply(const void *x, const dnm_subspace *src, int src_sector, void *y, const dnm_subspace *dst,
                           int dst_sector, void *stream) {
  DNM_CHECK(x && y, "subspace map: null argument");
  DNM_CHECK(x != y, "subspace map: x and y are the same vector (the pass gathers: the result needs its own)");
  SubView sv{}, dv{};
  DNM_TRY(submap_check(src, src_sector, dst, dst_sector, &sv, &dv));
  SubOwned s, d;
  DNM_TRY(s.init(src, true));
  DNM_TRY(d.init(dst, true));
  SubmapPlan p;
  DNM_TRY(submap_plan(s.host, src_sector, d.host, dst_sector, &p));
  p.src.v = s.dev;
  p.dst.v = d.dev;
  DNM_TRY(launch_submap(x, y, p, S(stream)));
  DNM_HIP(hipStreamSynchronize(S(stream)));     // the subspace tables are released on return
  return 0;
}

int dnm_sector_weights_plan(const dnm_subspace *sub, int xparity_sector, int *nworkgroups, size_t *scratch_bytes) {
  DNM_CHECK(sub, "sector weights: null subspace descriptor");
  SubView v{};
  DNM_TRY(submap_check_side(sub, xparity_sector, "sector weights", "", &v));
  SectorWeightsPlan p;
  DNM_TRY(sector_weights_plan(v, xparity_sector, &p));
  if (nworkgroups) *nworkgroups = p.nwg;
  if (scratch_bytes) *scratch_bytes = p.partial_bytes + (size_t)p.ncols * sizeof(double);
  return 0;
}

int dnm_sector_weights(const void *x, const dnm_subspace *sub, int xparity_sector, double *popcount_out,
                       double *flip_out, void *stream) {
  const char *what = "sector weights";
  DNM_CHECK(x && sub && popcount_out, "%s: null argument", what);
  SubView v{};
  DNM_TRY(submap_check_side(sub, xparity_sector, what, "", &v));
  SectorWeightsPlan p;
  DNM_TRY(sector_weights_plan(v, xparity_sector, &p));
  DNM_CHECK(!flip_out || xparity_sector != 0 || p.pairs, "%s: the sectors of the global flip are defined on Full, on "
            "Parity with even L, on SpinConserve(L, L/2) and on XParity states, not on this subspace (type %d, L=%d): "
            "pass a null flip_out", what, v.type, v.L);
  SubOwned s;
  DNM_TRY(s.init(sub, true));
  p.side.v = s.dev;
  const size_t obytes = (size_t)p.ncols * sizeof(double);
  DevBuf big;
  void *scratch = nullptr;       // the workgroups' partial sums, then the sums
  DNM_TRY(rdm_scratch(p.partial_bytes + obytes, &big, &scratch, what, 0, 0, p.nwg));
  void *o_dev = (char *)scratch + p.partial_bytes;
  DNM_TRY(launch_sector_weights(x, p, scratch, o_dev, S(stream)));
  std::vector<double> sums((size_t)p.ncols);
  // (synchronises: the subspace tables and `big` are released on return)
  DNM_TRY(dnm_memcpy_d2h(sums.data(), o_dev, obytes, stream));
  memcpy(popcount_out, sums.data(), ((size_t)v.L + 1) * sizeof(double));
  if (flip_out) memcpy(flip_out, sums.data() + v.L + 1, 2 * sizeof(double));
  return 0;
}

// ---- Gram matrix of many vectors ----------------------------------------------------------------------------------
// what the plan and the call check alike, before any device call
static int vgram_check(int nvec, int64_t n) {
  const char *what = "state Gram matrix";
  DNM_CHECK(nvec >= 1 && nvec <= 64, "%s: %d vectors (1 to 64 in one call)", what, nvec);
  DNM_CHECK(n >= 0, "%s: vectors of %lld elements", what, (long long)n);
  return 0;
}

int dnm_vec_gram_plan(int nvec, int64_t n, int *tile_rows, int *panel_rows_log2, int *nworkgroups, size_t *lds_bytes,
                      size_t *scratch_bytes) {
  DNM_TRY(vgram_check(nvec, n));
  GramPlan p;
  DNM_TRY(vgram_plan(nvec, n, &p));
  plan_out(p.nb, p.B, p.nwg, p.lds_bytes, p.partial_bytes, tile_rows, panel_rows_log2, nworkgroups, lds_bytes,
           scratch_bytes);
  return 0;
}

int dnm_vec_gram(const void *const *xs, int nvec, int64_t n, double *out, void *stream) {
  const char *what = "state Gram matrix";
  DNM_TRY(vgram_check(nvec, n));
  DNM_CHECK(xs && out, "%s: null argument", what);
  for (int c = 0; c < nvec; ++c) {
    DNM_CHECK(xs[c] || n == 0, "%s: vector %d is a null pointer", what, c);
    DNM_CHECK((uintptr_t)xs[c] % 16 == 0, "%s: vector %d at %p is not 16-byte aligned", what, c, xs[c]);
  }
  if (n == 0) {
    memset(out, 0, (size_t)nvec * (size_t)nvec * 2 * sizeof(double));
    return 0;
  }
  GramPlan p;
  DNM_TRY(vgram_plan(nvec, n, &p));
  return gram_moments(p, 0, (size_t)nvec, what, out, stream, [&](int64_t *, void *partial, void *G) {
    return launch_vec_gram(xs, nvec, p, partial, G, S(stream));
  });
}

}  // extern "C"
