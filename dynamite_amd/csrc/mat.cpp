// C ABI: device helpers, subspace maps, and the shell matrix (create / norm / diagonal / exports / destroy); its
// multiplies are in mat_mult.cpp, the observables of a state in observables.cpp.
// See include/dynamite_amd.h for the reference interfaces each entry point replaces.
#include "passes.h"

#include <algorithm>
#include <cstring>

namespace dnm {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

int DevBuf::alloc(size_t nbytes) {
  release();
  if (nbytes == 0) nbytes = 16;
  DNM_HIP(hipMalloc(&p, nbytes));
  bytes = nbytes;
  return 0;
}
int DevBuf::upload(const void *host, size_t nbytes) {
  DNM_TRY(alloc(nbytes));
  if (nbytes) DNM_HIP(hipMemcpy(p, host, nbytes, hipMemcpyHostToDevice));
  return 0;
}
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
}

int view_from_c(const dnm_subspace *s, SubView *v) {
  DNM_CHECK(s != nullptr, "null subspace descriptor");
  DNM_CHECK(s->type >= DNM_FULL && s->type <= DNM_SPIN_CONSERVE, "unknown subspace type %d", s->type);
  DNM_CHECK(s->L >= 1 && s->L <= 63, "L=%lld out of range", (long long)s->L);
  v->type = s->type;
  v->L = (int32_t)s->L;
  v->space = (int32_t)s->space;
  v->k = (int32_t)s->k;
  v->ld = (int32_t)s->ld_nchoosek;
  v->dim = s->dim;
  v->nchoosek = s->nchoosek;
  v->state_map = s->state_map;
  v->rmap_indices = s->rmap_indices;
  v->rmap_states = s->rmap_states;
  v->swz = s->vec_swizzle;
  v->sc3 = 0;
  if (s->type == DNM_SPIN_CONSERVE && v->swz != 0) {       // the internal layout of sc3.h: a | w << 8
    v->sc3 = v->swz;
    v->swz = 0;
    DNM_CHECK(sc3_valid((int)s->L, (int)s->k, sc3_code_a(v->sc3), sc3_code_w(v->sc3)),
              "vec_swizzle %d: no such SpinConserve layout for L=%d k=%d", v->sc3, (int)s->L, (int)s->k);
  }
  DNM_CHECK(v->swz == 0 || ((s->type == DNM_FULL || s->type == DNM_PARITY) && v->swz >= 5 && v->swz <= 24),
            "vec_swizzle %d: swizzled vectors need a Full or Parity subspace and a shift in [5, 24]", v->swz);
  if (s->type == DNM_PARITY) DNM_CHECK(s->space == 0 || s->space == 1, "parity space must be 0 or 1");
  if (s->type == DNM_SPIN_CONSERVE) {
    DNM_CHECK(s->nchoosek != nullptr && s->ld_nchoosek == s->L + 1 && s->k >= 0 && s->k <= s->L,
              "bad SpinConserve descriptor");
  }
  if (s->type == DNM_EXPLICIT)
    DNM_CHECK(s->state_map && s->rmap_states && s->dim >= 1, "bad Explicit descriptor");
  return 0;
}

int SubOwned::init(const dnm_subspace *s, bool want_device) {
  SubView v{};
  DNM_TRY(view_from_c(s, &v));
  host = v;
  if (v.type == DNM_SPIN_CONSERVE) {
    nck.assign(v.nchoosek, v.nchoosek + (size_t)(v.k + 1) * v.ld);
    host.nchoosek = nck.data();
  }
  if (v.type == DNM_EXPLICIT) {
    smap.assign(v.state_map, v.state_map + v.dim);
    rstates.assign(v.rmap_states, v.rmap_states + v.dim);
    host.state_map = smap.data();
    host.rmap_states = rstates.data();
    if (v.rmap_indices) {
      rind.assign(v.rmap_indices, v.rmap_indices + v.dim);
      host.rmap_indices = rind.data();
    }
    // bucket table: about two buckets per state (at most 2^26: 512 MB), so a search touches one or two entries
    int tb = 1;
    int tb_max = 26;         // measured at 40 M states: 8.2 ms (2^20 buckets), 6.5 (2^22), 4.9 (2^24), 4.2 (2^26); binary search: 22.9
    if (const char *e = knob("DNM_BUCKET_BITS")) tb_max = atoi(e);
    while (tb < v.L && tb < tb_max && ((int64_t)1 << tb) < 2 * v.dim) ++tb;
    host.bucket_shift = v.L - tb;
    const int64_t nb = (int64_t)1 << tb;
    bucket.assign((size_t)nb + 1, 0);
    bool sorted = true;
    for (int64_t i = 0; i < v.dim; ++i) {
      const int64_t st = rstates[(size_t)i];
      if (st < 0 || (st >> host.bucket_shift) >= nb || (i > 0 && st <= rstates[(size_t)i - 1])) { sorted = false; break; }
      ++bucket[(size_t)(st >> host.bucket_shift) + 1];
    }
    if (sorted) {
      for (int64_t b = 0; b < nb; ++b) bucket[(size_t)b + 1] += bucket[(size_t)b];
      host.bucket = bucket.data();
    } else {          // not a sorted list of L-bit states: plain binary search over everything
      bucket.clear();
      host.bucket = nullptr;
    }
  }
  host.dim = sub_dim(host);
  dev = host;
  dev.nchoosek = nullptr;
  dev.state_map = dev.rmap_indices = dev.rmap_states = nullptr;
  dev.bucket = nullptr;
  if (want_device) {
    if (!nck.empty()) {
      DNM_TRY(d_nck.upload(nck.data(), nck.size() * 8));
      dev.nchoosek = (const int64_t *)d_nck.p;
    }
    if (!smap.empty()) {
      DNM_TRY(d_smap.upload(smap.data(), smap.size() * 8));
      DNM_TRY(d_rstates.upload(rstates.data(), rstates.size() * 8));
      dev.state_map = (const int64_t *)d_smap.p;
      dev.rmap_states = (const int64_t *)d_rstates.p;
      if (!rind.empty()) {
        DNM_TRY(d_rind.upload(rind.data(), rind.size() * 8));
        dev.rmap_indices = (const int64_t *)d_rind.p;
      }
      if (!bucket.empty()) {
        DNM_TRY(d_bucket.upload(bucket.data(), bucket.size() * 8));
        dev.bucket = (const int64_t *)d_bucket.p;
      }
    }
  }
  return 0;
}

// (the pass builder -- build_opform ... build_flip_pass -- lives in passes.cpp)
template <class T>
static int upload_to(DevBuf &buf, const std::vector<T> &v, const T **dev) {
  DNM_TRY(buf.upload(v.data(), v.size() * sizeof(T)));
  *dev = (const T *)buf.p;
  return 0;
}
int PassRecords::upload() {
  DNM_TRY(upload_to(d_quads, quads, &desc.quads));
  if (!dtile.empty()) DNM_TRY(upload_to(d_dtile, dblock.empty() ? dtile : dtile_sections(), &desc.dtile));
  if (!dblock.empty()) DNM_TRY(upload_to(d_dblock, dblock, &desc.dblock));
  if (!tabs.empty()) DNM_TRY(upload_to(d_tabs, tabs, &desc.tabs));
  if (!tabs.empty()) DNM_TRY(upload_to(d_tabvals, tabvals, &desc.tabvals));
  // (a pass that only carries the reduced diagonal has no flip-flop record: the kernel still takes a non-null pointer)
  if (is_reduced) DNM_TRY(upload_to(d_flips, flips.empty() ? std::vector<DevFlip>(1) : flips, &flip.recs));
  return 0;
}

static hipStream_t S(void *stream) { return (hipStream_t)stream; }

// the exports: pass lookup, and the checked copy-out of a host vector (item: the caller's size of one element; an empty
// vector copies nothing and, unless `strict`, checks nothing)
static int export_lookup(const dnm_mat *A, int remote, int idx, const PassOnDevice **p) {
  DNM_CHECK(A, "null argument");
  const auto &v = remote ? A->remote_passes : A->local_passes;
  DNM_CHECK(idx >= 0 && idx < (int)v.size(), "pass index out of range");
  *p = v[idx].get();
  return 0;
}
template <class T>
static int export_copy(const std::vector<T> &v, void *out, size_t item, int64_t room, const char *type, const char *full,
                       bool strict = false) {
  if (!out || (v.empty() && !strict)) return 0;
  DNM_CHECK(item == sizeof(T), "%s size mismatch (%zu vs %zu)", type, item, sizeof(T));
  DNM_CHECK(room >= (int64_t)v.size(), "%s buffer too small", full);
  if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(T));   // (an empty pass: no null source)
  return 0;
}
// a description and its records (dnm_mat_export_pass, dnm_mat_export_flip_pass)
static int export_records(const PassRecords &r, void *desc_out, size_t desc_bytes, void *quads_out, size_t quad_bytes,
                          int max_quads, int *nquads, bool strict) {
  *nquads = (int)r.quads.size();
  if (desc_out) {
    DNM_CHECK(desc_bytes == sizeof(DevPass), "DevPass size mismatch (%zu vs %zu)", desc_bytes, sizeof(DevPass));
    // (the fields of the diagonal's tables are derived data with an export of their own, dnm_mat_export_diag_tables:
    // the description handed out here is the same with and without them)
    DevPass d = r.desc;
    d.dblock = nullptr;
    d.dsel_n = 0;
    memset(d.dsel_mask, 0, sizeof(d.dsel_mask));
    memcpy(desc_out, &d, sizeof(DevPass));
  }
  return export_copy(r.quads, quads_out, quad_bytes, max_quads, "DevQuad", "record", strict);
}

}  // namespace dnm

using namespace dnm;

extern "C" {

const char *dnm_last_error(void) { return g_err.c_str(); }
int dnm_version(void) { return 100; }

int dnm_device_count(int *count) {
  DNM_CHECK(count, "null pointer");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); }
  return 0;
}
int dnm_set_device(int device) { DNM_HIP(hipSetDevice(device)); return 0; }
int dnm_malloc(void **dptr, size_t bytes) { DNM_HIP(hipMalloc(dptr, bytes ? bytes : 16)); return 0; }
int dnm_free(void *dptr) { DNM_HIP(hipFree(dptr)); return 0; }
int dnm_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream) {
  DNM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream)));
  DNM_HIP(hipStreamSynchronize(S(stream)));
  return 0;
}
int dnm_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream) {
  DNM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)));
  DNM_HIP(hipStreamSynchronize(S(stream)));
  return 0;
}
int dnm_stream_synchronize(void *stream) { DNM_HIP(hipStreamSynchronize(S(stream))); return 0; }

// ---- subspaces --------------------------------------------------------------
int dnm_subspace_dim(const dnm_subspace *s, int64_t *dim) {
  SubView v{};
  DNM_TRY(view_from_c(s, &v));
  *dim = sub_dim(v);
  return 0;
}

int dnm_idx_to_state(const dnm_subspace *s, int64_t n, const int64_t *idxs, int64_t *states) {
  SubView v{};
  DNM_TRY(view_from_c(s, &v));
  const int64_t dim = sub_dim(v);
  for (int64_t i = 0; i < n; ++i) {
    // the reference raises for out-of-range indices (bsubspace.pyx:170-173)
    DNM_CHECK(idxs[i] >= 0 && idxs[i] < dim, "index %lld out of bounds for subspace of dimension %lld",
              (long long)idxs[i], (long long)dim);
    states[i] = sub_i2s(idxs[i], v);
  }
  return 0;
}

int dnm_state_to_idx(const dnm_subspace *s, int64_t n, const int64_t *states, int64_t *idxs) {
  SubView v{};
  DNM_TRY(view_from_c(s, &v));
  for (int64_t i = 0; i < n; ++i) idxs[i] = sub_s2i(states[i], v);
  return 0;
}

// ---- CheckConserves ---------------------------------------------------------------
int dnm_check_conserves(int64_t nmasks, const int64_t *masks, const int64_t *mask_offsets,
                        const int64_t *signs, const double *coeffs, const dnm_subspace *left,
                        const dnm_subspace *right, int xparity, int *result, void *stream) {
  DNM_CHECK(result && (nmasks == 0 || (masks && mask_offsets && signs && coeffs)), "null argument");
  SubOwned l, r;
  DNM_TRY(l.init(left, true));
  DNM_TRY(r.init(right, true));
  const int64_t nterms = nmasks ? mask_offsets[nmasks] : 0;
  std::vector<double> re(nterms), im(nterms);
  for (int64_t t = 0; t < nterms; ++t) { re[t] = coeffs[2 * t]; im[t] = coeffs[2 * t + 1]; }
  DevBuf dm, doff, ds, dre, dim_, dbad;
  DNM_TRY(dm.upload(masks, (size_t)nmasks * 8));
  DNM_TRY(doff.upload(mask_offsets, (size_t)(nmasks + 1) * 8));
  DNM_TRY(ds.upload(signs, (size_t)nterms * 8));
  DNM_TRY(dre.upload(re.data(), (size_t)nterms * 8));
  DNM_TRY(dim_.upload(im.data(), (size_t)nterms * 8));
  int zero = 0;
  DNM_TRY(dbad.upload(&zero, sizeof(int)));
  DevMsc msc{(int32_t)nmasks, (const int64_t *)dm.p, (const int64_t *)doff.p, (const int64_t *)ds.p,
             (const double *)dre.p};
  // XParity: the columns are the first half of the parent's (bpetsc_template_2.c:1005-1008)
  const int64_t ncols = xparity ? r.host.dim / 2 : r.host.dim;
  DNM_TRY(launch_conserves(msc, (const double *)dim_.p, l.dev, r.dev, ncols, (int *)dbad.p, S(stream)));
  int bad = 0;
  DNM_TRY(dnm_memcpy_d2h(&bad, dbad.p, sizeof(int), stream));
  *result = bad ? 0 : 1;
  return 0;
}

// ---- shell matrix -------------------------------------------------------------
// The patterns of `bits` <= 16 bits grouped by popcount, ascending inside a group (colex order = numeric order): group j
// starts at table[off[j]]
static void popcount_groups(int bits, std::vector<uint16_t> *table, int32_t off[18]) {
  const int n = 1 << bits;
  table->resize((size_t)n);
  int cnt[18] = {0};
  for (int v = 0; v < n; ++v) ++cnt[__builtin_popcount(v) + 1];
  for (int j = 0; j < 17; ++j) { cnt[j + 1] += cnt[j]; off[j] = cnt[j]; }
  off[17] = n;
  int fill[17];
  for (int j = 0; j < 17; ++j) fill[j] = off[j];
  for (int v = 0; v < n; ++v) (*table)[fill[__builtin_popcount(v)]++] = (uint16_t)v;
}

// Decide whether the SpinConserve block kernel runs and build its table.  DNM_SC_BLOCK = 0 (row kernel),
// 10 / 13 (low bits per block); default: 13 when the blocks are large enough to fill a workgroup.
static int setup_sc_block(dnm_mat *A) {
  A->scblock.lb = 0;
  if (!A->sc_pair || A->m_local <= 0) return 0;
  const SubView &h = A->left.host;
  const int L = h.L, k = h.k;
  int lb = -1;
  if (const char *e = knob("DNM_SC_BLOCK")) lb = atoi(e);
  if (lb == 0) return 0;
  const bool forced = lb > 0;
  if (!forced) lb = 13;
  if ((int64_t)A->masks.size() > sc_block_max_masks()) return 0;     // one lane per mask in the block kernel
  DNM_CHECK(sc_block_supported(lb), "DNM_SC_BLOCK=%d: no such kernel instance (0, 10, 13)", lb);
  if (L <= lb || L - lb > 48) return 0;
  if (!forced && (A->M >> (L - lb)) < 256) return 0;     // blocks too small on average: one row per thread instead
  if (!forced && 2 * A->sc_nfast < (int)A->masks.size()) return 0;   // mostly non-chain masks: they take the per-row path anyway
  std::vector<uint16_t> tab;
  popcount_groups(lb, &tab, A->scblock.off);
  DNM_TRY(A->d_scblock.upload(tab.data(), tab.size() * sizeof(uint16_t)));
  A->scblock.lowtab = (const uint16_t *)A->d_scblock.p;
  int64_t hf = sub_i2s(A->row0, h) >> lb, hl = sub_i2s(A->row0 + A->m_local - 1, h) >> lb;
  A->scblock.swizzle = 0;
  if (hl - (hf & ~(int64_t)511) + 1 >= 1024) {
    A->scblock.swizzle = 1;
    hf &= ~(int64_t)511;
  }
  A->scblock.h_first = hf;
  A->scblock.h_last = hl;
  A->scblock.lb = lb;
  A->scblock.perm = nullptr;
  A->scblock.nperm = 0;
  // Block order (DNM_SC_ORDER=g, 0 = ascending H): blocks of equal size run together -- ordered by the popcount
  // of H, then by the bits of H above the lowest g -- so that the workgroups resident at one time do equal work
  // and stay in step, and the blocks an XCD holds are siblings under the g-1 lowest high bonds; groups go
  // round-robin to the XCDs.  Measured on MI355X, L=32 k=16: 17.6 ms ascending, 15.3 (g=1), 14.4 (g=6), 15.9 (g=8).
  int g = (hl - hf + 1 >= 1024) ? 6 : 0;
  if (const char *e = knob("DNM_SC_ORDER")) g = atoi(e);
  // DNM_SC_CHUNK=c (experiment): the order above inside chunks of 2^c consecutive high parts, chunk after chunk --
  // partners under the c-1 lowest high bonds then lie in the same chunk, i.e. within what the Infinity Cache holds
  int chunk = 0;
  if (const char *e = knob("DNM_SC_CHUNK")) chunk = atoi(e);
  if (chunk <= 0 || chunk > 40) chunk = 62;
  if (g > 0 && hl - hf + 1 < ((int64_t)1 << 31)) {
    const int64_t span = hl - hf + 1;
    std::vector<uint32_t> ord;
    ord.reserve((size_t)span);
    for (int64_t e = 0; e < span; ++e) {
      const int kl = k - __builtin_popcountll((uint64_t)(hf + e));
      if (kl >= 0 && kl <= lb) ord.push_back((uint32_t)e);
    }
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
      const uint64_t ha = (uint64_t)(hf + a), hb = (uint64_t)(hf + b);
      const int pa = __builtin_popcountll(ha), pb = __builtin_popcountll(hb);
      if ((ha >> chunk) != (hb >> chunk)) return (ha >> chunk) < (hb >> chunk);
      if (pa != pb) return pa < pb;
      if ((ha >> g) != (hb >> g)) return (ha >> g) < (hb >> g);
      return ha < hb;
    });
    std::vector<std::vector<uint32_t>> lists(8);
    size_t i = 0;
    int64_t q = 0;
    while (i < ord.size()) {
      size_t j = i;
      const uint64_t h0 = (uint64_t)(hf + ord[i]);
      while (j < ord.size() && ((uint64_t)(hf + ord[j]) >> g) == (h0 >> g) &&
             __builtin_popcountll((uint64_t)(hf + ord[j])) == __builtin_popcountll(h0)) ++j;
      auto &dst = lists[(size_t)(q++ & 7)];
      dst.insert(dst.end(), ord.begin() + i, ord.begin() + j);
      i = j;
    }
    size_t longest = 0;
    for (auto &l : lists) longest = std::max(longest, l.size());
    std::vector<uint32_t> perm(longest * 8, 0xffffffffu);
    for (size_t x = 0; x < 8; ++x)
      for (size_t t = 0; t < lists[x].size(); ++t) perm[t * 8 + x] = lists[x][t];
    DNM_TRY(A->d_scperm.upload(perm.data(), perm.size() * sizeof(uint32_t)));
    A->scblock.perm = (const uint32_t *)A->d_scperm.p;
    A->scblock.nperm = (int64_t)perm.size();
  }
  return 0;
}

// the passes of one list of the plan, in their generic form
static int build_passes(const dnm_mat &A, const std::vector<PassSpec> &specs, std::vector<std::unique_ptr<PassOnDevice>> *out) {
  for (const PassSpec &ps : specs) {
    out->emplace_back(new PassOnDevice());
    DNM_TRY(build_pass(A, ps, out->back().get()));
  }
  return 0;
}

// dnm_mat_create, step 1: the device tables of the row kernels.  The generic ones always (norm and diagonal use them);
// for two SpinConserve subspaces the per-mask table `scm`, the 16-bit unranking table and, in reference order, the
// block kernel's.  A host-only handle has none of them.
static int setup_row_tables(dnm_mat *A, const std::vector<ScMask> &scm) {
  if (A->host_only) return 0;
  DNM_TRY(A->d_masks.upload(A->masks.data(), A->masks.size() * 8));
  DNM_TRY(A->d_offsets.upload(A->mask_offsets.data(), A->mask_offsets.size() * 8));
  DNM_TRY(A->d_signs.upload(A->signs.data(), A->signs.size() * 8));
  DNM_TRY(A->d_rcoeffs.upload(A->real_coeffs.data(), A->real_coeffs.size() * 8));
  A->dmsc.nmasks = (int32_t)A->masks.size();
  A->dmsc.masks = (const int64_t *)A->d_masks.p;
  A->dmsc.mask_offsets = (const int64_t *)A->d_offsets.p;
  A->dmsc.signs = (const int64_t *)A->d_signs.p;
  A->dmsc.real_coeffs = (const double *)A->d_rcoeffs.p;
  if (A->left.host.type == DNM_SPIN_CONSERVE && A->right.host.type == DNM_SPIN_CONSERVE) {
    A->sc_nfast = 0;
    for (const ScMask &e : scm) A->sc_nfast += e.fast ? 1 : 0;
    DNM_TRY(A->d_scmasks.upload(scm.data(), scm.size() * sizeof(ScMask)));
    std::vector<uint16_t> low;
    popcount_groups(16, &low, A->sclow.off);
    DNM_TRY(A->d_sclow.upload(low.data(), low.size() * sizeof(uint16_t)));
    A->sclow.tab = (const uint16_t *)A->d_sclow.p;
    if (!A->use_sc3) DNM_TRY(setup_sc_block(A));
  }
  return 0;
}

// the operator arrays of a handle (dnm_mat::masks ... real_coeffs) in another labelling of the sites
namespace {
struct OpArrays {
  std::vector<int64_t> masks, offsets, signs;
  std::vector<double> coeffs;
};
}  // namespace

// The operator as the kernels of a relabelled layout see it: masks and signs bit by bit into the layout's labelling, the
// mask groups sorted again (terms keep their order inside a group; a coefficient is unchanged: it multiplies the same
// product of Pauli matrices).  No relabelling: the arrays as they are.
static OpArrays relabelled_operator(const dnm_mat &A, const Sc3Perm &P) {
  OpArrays o{A.masks, A.mask_offsets, A.signs, A.real_coeffs};
  if (!P.on) return o;
  const int L = A.left.host.L;
  const int64_t nmasks = (int64_t)A.masks.size();
  std::vector<int64_t> order((size_t)nmasks);
  std::vector<uint64_t> nm((size_t)nmasks);
  for (int64_t i = 0; i < nmasks; ++i) {
    order[(size_t)i] = i;
    nm[(size_t)i] = sc3_permute((uint64_t)A.masks[(size_t)i], P.to_int, L);
  }
  std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return nm[(size_t)x] < nm[(size_t)y]; });
  o.masks.clear(); o.signs.clear(); o.coeffs.clear();
  o.offsets.assign(1, 0);
  for (int64_t q = 0; q < nmasks; ++q) {
    const int64_t i = order[(size_t)q];
    o.masks.push_back((int64_t)nm[(size_t)i]);
    for (int64_t t = A.mask_offsets[(size_t)i]; t < A.mask_offsets[(size_t)i + 1]; ++t) {
      o.signs.push_back((int64_t)sc3_permute((uint64_t)A.signs[(size_t)t], P.to_int, L));
      o.coeffs.push_back(A.real_coeffs[(size_t)t]);
    }
    o.offsets.push_back((int64_t)o.signs.size());
  }
  return o;
}

// dnm_mat_create, step 2: a SpinConserve pair whose vectors are in the internal layout (sc3.h) -- the layout, the
// rank's share of it, the operator in the layout's site labelling (left / right: the caller's descriptors, for their
// site_perm) and the tables of its kernels (sc3_tables.cpp); m_local / n_local / rows_local / row0 then describe the share.
// scm: the per-mask table in reference labelling.
static int setup_sc3(dnm_mat *A, const dnm_subspace *left, const dnm_subspace *right, std::vector<ScMask> scm) {
  const SubView &h = A->left.host;
  const Sc3Layout *ly = sc3_get(h.L, h.k, sc3_code_a(h.sc3), sc3_code_w(h.sc3), !A->host_only, sc3_code_order(h.sc3));
  DNM_CHECK(ly, "could not build the SpinConserve vector layout");
  A->sc3.reset(new Sc3Mat());
  // partitioned: whole T blocks per rank (a contiguous range of both the internal layout and the reference order)
  std::vector<uint32_t> Tb = sc3_partition(*ly, A->nranks);
  if (A->xparity) {
    // the half whose top bit is clear, as a PLACE in the block sequence (a layout with empty blocks -- k > a + w or
    // t > k -- has fewer than 2^(t-1) blocks below it); only block order 0 keeps that half together
    DNM_CHECK(ly->order == 0, "XParity on a SpinConserve layout in block order %d: the half whose top bit is clear is "
              "no range of that layout", ly->order);
    Tb = {0u, sc3_top_clear_blocks(*ly)};
  }
  const bool want_real = (A->flags & DNM_MAT_REAL_PACKED) != 0;
  // site relabelling of the vectors (dnm_subspace.site_perm): the kernels of the layout see the operator in it
  Sc3Perm P, Pr;
  DNM_CHECK(sc3_perm_make(left->site_perm, h.L, &P) && sc3_perm_make(right->site_perm, h.L, &Pr),
            "site_perm is not a permutation of the %d spins", h.L);
  DNM_CHECK(memcmp(P.to_int, Pr.to_int, sizeof P.to_int) == 0, "left and right vectors must share their site relabelling");
  DNM_CHECK(!P.on || A->nranks == 1, "a relabelled SpinConserve layout is not partitioned over ranks");
  DNM_CHECK(!A->xparity || P.to_int[h.L - 1] == h.L - 1, "XParity: the site relabelling must keep spin L-1 in place");
  A->sc3->perm = P;
  const OpArrays o = relabelled_operator(*A, P);
  if (P.on) scm = sc_masks(o.masks, o.offsets, o.signs, o.coeffs, h.L, A->xparity);
  A->dmsc_sc3 = A->dmsc;
  if (P.on && !A->host_only) {           // the row kernel's tables in the layout's labelling
    DNM_TRY(A->d_pmasks.upload(o.masks.data(), o.masks.size() * 8));
    DNM_TRY(A->d_poffsets.upload(o.offsets.data(), o.offsets.size() * 8));
    DNM_TRY(A->d_psigns.upload(o.signs.data(), o.signs.size() * 8));
    DNM_TRY(A->d_prcoeffs.upload(o.coeffs.data(), o.coeffs.size() * 8));
    A->dmsc_sc3.masks = (const int64_t *)A->d_pmasks.p;
    A->dmsc_sc3.mask_offsets = (const int64_t *)A->d_poffsets.p;
    A->dmsc_sc3.signs = (const int64_t *)A->d_psigns.p;
    A->dmsc_sc3.real_coeffs = (const double *)A->d_prcoeffs.p;
  }
  DNM_TRY(A->sc3->init(ly, o.masks, o.offsets, o.signs, o.coeffs, scm, !A->host_only, Tb[A->rank], Tb[A->rank + 1],
                       want_real));
  if (const char *e = knob("DNM_SC3_TILED")) if (e[0] == '0') A->sc3->tiled = false;     // tests: the row kernel
  if (const char *e = knob("DNM_SC3_DIAG")) if (e[0] == 'c' && A->sc3->diag_mode == 2) A->sc3->diag_mode = 1;
  // (timing probe, WRONG results: the passes without any diagonal -- what dropping the cached diagonal's 8 B/row could save)
  if (const char *e = knob("DNM_SC3_DIAG")) if (e[0] == 'n') A->sc3->diag_mode = 0;
  int64_t is, il, ns, nl;
  sc3_range(*ly, Tb[A->rank], Tb[A->rank + 1], &is, &il, &ns, &nl);
  A->m_local = A->n_local = il;          // what the vector kernels sweep: rows + padding
  A->rows_local = nl;
  // first row in reference order (norm / diagonal kernels).  Block order 0: the share is the reference rows
  // [row0, row0 + rows_local).  Any other order: rows_local still counts the share's rows, but they are no range of
  // the reference order and row0 is -1 on every share that does not start the sequence -- whatever walks reference
  // rows asks ref_side first or walks sc3_ref_runs (dnm_mat_norm_inf)
  A->row0 = ns;
  if (want_real) {
    // real vectors in the same positions of the layout, one double each: a vector is il / 2 complex128 elements for
    // everything that sweeps it (the Krylov kernels); the two tiled passes only (chain operators, real symmetric)
    // Partitions: every position the C ABI speaks of for such a handle -- ownership, column windows, chunk maps,
    // window starts -- counts complex128 ELEMENTS (pairs of entries; blocks of equal top bits start at multiples of 8
    // entries), so the caller's exchange code is the one it runs for complex vectors, on half the bytes
    DNM_CHECK(A->sc3->tiled && A->sc3->sym,
              "operator has an imaginary matrix element or is not a sum of pair hops: no real-packed form in this layout");
    A->real_packed = true;
    A->m_local = A->n_local = il / 2;
  }
  return 0;
}

// dnm_mat_create, step 3: a Full / Parity pair -- the operator in index-space form, the plan with the defaults of its
// configuration and, when the plan is tiled, the passes' records (passes.cpp) and their upload
static int setup_hypercube(dnm_mat *A) {
  const int flags = A->flags;
  DNM_TRY(build_opform(*A, &A->op));
  if (flags & DNM_MAT_REAL_PACKED) {
    // (partitions: the rank bits are the top index bits, the packed bit is bit 0 -- the partner exchange of the packed
    // operator is that of an operator on one bit less; the transposed exchange is not built for it)
    // (XParity on top: the reduced operator is packed like any other -- its flip-composed masks reach index bit 0, the
    // lane, like every odd mask -- and loses its top index bit below)
    DNM_CHECK(A->M == A->N, "real-packed operators: square");
    DNM_TRY(pack_opform(&A->op));
    A->real_packed = true;
    A->M /= 2; A->N /= 2; A->m_local /= 2; A->n_local /= 2;         // complex128 elements, two amplitudes each
  }
  if (A->xparity) {
    // rows and columns have the top index bit clear: the hypercube loses one dimension
    const uint64_t topbit = (uint64_t)1 << (A->op.n - 1);
    for (RowMask &rm : A->op.masks) {
      DNM_CHECK(!(rm.mask & topbit), "internal: XParity mask reaches the top index bit");
      for (RowTerm &t : rm.terms) t.sign &= ~topbit;
    }
    A->op.n -= 1;
  }
  PlanConfig cfg = plan_config_from_env();
  if (const int fa = (flags >> DNM_MAT_AMIN_SHIFT) & 0xff) cfg.amin = fa;      // caller-chosen run length of window tiles
  DNM_CHECK(A->left.host.swz == A->right.host.swz, "left and right vectors of a Full/Parity pair must share a layout");
  cfg.swz = A->left.host.swz;
  int nl = A->op.n;            // index bits of a rank's block: what the measured defaults below go by
  for (int r = A->nranks; r > 1; r >>= 1) --nl;
  if (cfg.logR < 0) {
    // measured: in index order 16 rows per thread pay from 2^26 local amplitudes on (profiles/r01_sweep6.txt);
    // with swizzled vectors 8 rows beat 16 at every size (profiles/r02_exp3_v2.txt), and once the window pass
    // runs first and the accumulating pass carries the diagonal, 4 rows per thread (two 1024-thread workgroups,
    // 32 waves per CU) beat 8: L=30 16.9 -> 16.5 ms, 2-3 % from 2^26 amplitudes on
    // (profiles/r02_exp46_rows4_series.txt, r02_exp47_rows4_sizes.txt)
    cfg.logR = cfg.swz ? 2 : (nl >= 26 ? 4 : 3);
  }
  if (cfg.diag_last < 0) cfg.diag_last = cfg.swz ? 1 : 0;
  if (cfg.window_first < 0) {
    // which pass writes y and which adds to it: the window pass is bound by its bytes (48 B/amp when it
    // accumulates, at the streaming rate), the contiguous pass by its records (8.0 ms for 32.9 B/amp) -- so the y
    // read belongs to the latter.  With swizzled vectors (in index order the window pass's gathers do not merge
    // and it is the slow one either way, profiles/r01_prof_multi18.txt): L=30 17.5 -> 17.0 ms, L=28 4.43 -> 4.22,
    // L=26 1.09 -> 1.07; level or worse while both vectors fit in the Infinity Cache
    // (profiles/r02_exp41_pass_order.txt, r02_exp42_window_first_wide.txt)
    cfg.window_first = (cfg.swz && nl >= 25) ? 1 : 0;
  }
  if (!tile_config_supported(cfg.B, cfg.logR)) {
    set_error("unsupported tile configuration B=%d logR=%d", cfg.B, cfg.logR);
    return 1;
  }
  DNM_TRY(make_plan(A->op, A->rank, A->nranks, cfg, &A->plan));
  if (flags & DNM_MAT_FORCE_GATHER) A->plan.use_tiled = false;
  DNM_CHECK(!A->real_packed || A->plan.use_tiled, "real-packed operators run on the tiled kernel only (vector too small)");
  if (A->nranks > 1 && !A->plan.use_tiled) {
    // blocks smaller than one tile (or DNM_MAT_FORCE_GATHER): the window partition of the row kernel
    A->plan.remote.clear();
    A->plan.sends.clear();
  }
  if (A->plan.use_tiled) {
    DNM_TRY(build_passes(*A, A->plan.local, &A->local_passes));
    DNM_TRY(build_passes(*A, A->plan.remote, &A->remote_passes));
    // flip-flop records (plan.h: DevFlip): decided for the operator as a whole, from its passes as they stand
    decide_flip_bonds(A);
    for (size_t i = 0; i < A->plan.local.size(); ++i)
      DNM_TRY(build_flip_pass(*A, A->plan.local[i], A->local_passes[i].get()));
    // the diagonal of what the kernel runs on as tables (DevPass::dblock), where it qualifies
    for (auto *v : {&A->local_passes, &A->remote_passes})
      for (auto &p : *v) DNM_TRY(build_diag_tables(*A, p.get()));
    if (!A->host_only)
      for (auto *v : {&A->local_passes, &A->remote_passes})
        for (auto &p : *v) DNM_TRY(p->runs().upload());
  }
  return 0;
}

int dnm_mat_create(int64_t nmasks, const int64_t *masks, const int64_t *mask_offsets,
                   const int64_t *signs, const double *coeffs, const dnm_subspace *left,
                   const dnm_subspace *right, int xparity, int flags, const dnm_partition *part,
                   dnm_mat **out) {
  DNM_CHECK(out, "null output handle");
  *out = nullptr;
  DNM_CHECK(nmasks >= 0 && (nmasks == 0 || (masks && mask_offsets && signs && coeffs)),
            "null operator arrays");
  std::unique_ptr<dnm_mat> A(new dnm_mat());
  A->xparity = xparity != 0;
  if (const char *e = knob("DNM_ROW_FUSE")) A->row_fuse = e[0] != '0';
  A->flags = flags;
  A->host_only = (flags & DNM_MAT_HOST_ONLY) != 0;
  const int64_t nterms = nmasks ? mask_offsets[nmasks] : 0;
  A->masks.assign(masks, masks + nmasks);
  if (nmasks) A->mask_offsets.assign(mask_offsets, mask_offsets + nmasks + 1);
  else A->mask_offsets.assign(1, 0);
  A->signs.assign(signs, signs + nterms);
  A->real_coeffs.resize(nterms);
  for (int64_t i = 1; i < nmasks; ++i)
    DNM_CHECK(masks[i] > masks[i - 1], "masks must be sorted and unique");
  for (int64_t t = 0; t < nterms; ++t) {
    // one double per term: the real part if non-zero, else the imaginary part
    const double re = coeffs[2 * t], im = coeffs[2 * t + 1];
    A->real_coeffs[t] = (re != 0.0) ? re : im;
  }
  DNM_TRY(A->left.init(left, !A->host_only));
  DNM_TRY(A->right.init(right, !A->host_only));
  DNM_CHECK(A->left.host.L == A->right.host.L, "left and right subspaces have different L");
  A->M = A->left.host.dim;
  A->N = A->right.host.dim;
  A->one_subspace = same_subspace(A->left, A->right);
  if (A->xparity) {
    // The operator has been rewritten by XParity.reduce_msc (subspaces.py:632-674) and the basis is
    // the first half of the parent's: halving the dimensions is all the backend does
    // (bpetsc_template_2.c:78-85,223-230).  No mask may flip spin L-1 any more.
    DNM_CHECK(A->M % 2 == 0 && A->N % 2 == 0, "XParity needs parent subspaces of even dimension");
    const int64_t top = (int64_t)1 << (A->left.host.L - 1);
    for (int64_t i = 0; i < nmasks; ++i)
      DNM_CHECK(!(masks[i] & top), "XParity: mask %lld flips spin L-1 (operator not reduced by XParity.reduce_msc)",
                (long long)masks[i]);
    A->M /= 2;
    A->N /= 2;
  }
  A->rank = part ? part->rank : 0;
  A->nranks = part ? part->nranks : 1;
  DNM_CHECK(A->nranks >= 1 && A->rank >= 0 && A->rank < A->nranks, "bad partition (rank %d of %d)", A->rank,
            A->nranks);

  const int lt = A->left.host.type, rt = A->right.host.type;
  A->hypercube = (lt == rt) && (lt == DNM_FULL || lt == DNM_PARITY);
  A->sc_pair = lt == DNM_SPIN_CONSERVE && rt == DNM_SPIN_CONSERVE && A->left.host.k == A->right.host.k &&
               !(flags & DNM_MAT_FORCE_GATHER);
  if (A->nranks > 1 && A->hypercube && ((A->nranks & (A->nranks - 1)) != 0 || A->M % A->nranks != 0)) {
    // Full / Parity on a rank count that is not a power of two: blocks are not subcubes, so the XOR-partner
    // exchange does not apply -- rows are split as PetscSplitOwnership does and the generic row kernel reads
    // its columns through a window (MatMult_CPU_General's MPI branch, bpetsc_template_2.c:413-504)
    A->hypercube = false;
  }
  if (A->nranks > 1 && !A->hypercube) {
    // rows of a window partition are index-ordered blocks of any size: swizzled blocks need power-of-two sizes
    DNM_CHECK(A->left.host.swz == 0 || (A->M % A->nranks == 0 && ((A->M / A->nranks) & (A->M / A->nranks - 1)) == 0),
              "swizzled left vectors need power-of-two blocks (use vec_swizzle = 0 for this partition)");
  }
  // PetscSplitOwnership: M / P rows each, the first M % P ranks one more
  {
    const int64_t q = A->M / A->nranks, rem = A->M % A->nranks;
    A->m_local = q + (A->rank < rem ? 1 : 0);
    A->row0 = (int64_t)A->rank * q + std::min<int64_t>(A->rank, rem);
    const int64_t qn = A->N / A->nranks, remn = A->N % A->nranks;
    A->n_local = qn + (A->rank < remn ? 1 : 0);
    A->rows_local = A->m_local;
  }
  // SpinConserve pair whose vectors are in the internal layout: the two-pass / row kernels of sc3_kernels.hip.  Any
  // other use of such a subspace (another partner, XParity, several ranks) works in reference order: the caller
  // converts (dnm_mat_layouts tells).
  // (XParity on top: one rank, half filling -- the vectors are the blocks whose top bit is clear, the first half of the
  // layout as of the reference order)
  A->use_sc3 = A->sc_pair && A->left.host.sc3 != 0 && A->left.host.sc3 == A->right.host.sc3 &&
               A->left.host.L == A->right.host.L &&
               (!A->xparity || (A->nranks == 1 && 2 * A->left.host.k == A->left.host.L &&
                                sc3_instance(sc3_code_a(A->left.host.sc3), sc3_code_w(A->left.host.sc3))));

  std::vector<ScMask> scm;
  if (lt == DNM_SPIN_CONSERVE && rt == DNM_SPIN_CONSERVE)
    scm = sc_masks(A->masks, A->mask_offsets, A->signs, A->real_coeffs, A->left.host.L, A->xparity);
  DNM_TRY(setup_row_tables(A.get(), scm));
  if (A->use_sc3) DNM_TRY(setup_sc3(A.get(), left, right, scm));
  else DNM_CHECK(!(flags & DNM_MAT_REAL_PACKED) || A->hypercube,
                 "real-packed operators: Full / Parity pairs, or a SpinConserve pair in the internal layout");
  if (A->hypercube) DNM_TRY(setup_hypercube(A.get()));
  // the kernel family the handle multiplies on (mat.h: Route), now that the knobs have had their say; a host-only
  // handle has built no block-kernel table, so its SpinConserve pair in reference order reads as the row kernel
  if (A->hypercube && A->plan.use_tiled) A->route = Route::Tiled;
  else if (A->use_sc3) A->route = A->sc3->tiled ? Route::Sc3Tiled : Route::Sc3Rows;
  else if (A->sc_pair) A->route = A->scblock.lb ? Route::ScBlock : Route::ScRows;
  else A->route = Route::Gather;
  *out = A.release();
  return 0;
}

int dnm_mat_destroy(dnm_mat *A) {
  delete A;
  return 0;
}

// Exchange scheme of a partitioned Full / Parity operator.  The transposed exchange (backend.transpose_split is the
// host-side statement of the same split, tests/test_transpose_exchange.py compares the two): a rank's block holds the
// n = L - p low index bits, the rank number is the p top ones.  A term that flips a top bit couples blocks of different
// ranks; instead of shipping a partner block per such mask (bpetsc_template_2.c:787-879 scatters the needed entries) the
// state is redistributed ONCE so that the top bits become local: layout B swaps bits [n, n + p) with the local field
// F = [f, f + p), f = n - 1 - p (right below the top local bit, which the boundary bond touches).  In layout B every
// term that flips a top bit is rank-local provided it leaves F alone -- the same MSC term with the two fields swapped.
int dnm_mat_set_exchange(dnm_mat *A, int scheme, int *chosen) {
  DNM_CHECK(A && chosen, "null argument");
  DNM_CHECK(scheme == DNM_EXCHANGE_AUTO || scheme == DNM_EXCHANGE_PARTNER || scheme == DNM_EXCHANGE_TRANSPOSE,
            "unknown exchange scheme %d", scheme);
  delete A->tr_lo; delete A->tr_hi;
  A->tr_lo = A->tr_hi = nullptr;
  A->tr_f = -1;
  *chosen = DNM_EXCHANGE_PARTNER;
  const int P = A->nranks;
  if (scheme == DNM_EXCHANGE_PARTNER || P < 2 || (scheme == DNM_EXCHANGE_AUTO && P < 4)) return 0;
  const SubView &lh = A->left.host, &rh = A->right.host;
  if (!(A->route == Route::Tiled && !A->xparity && lh.type == rh.type && lh.L == rh.L &&
        (lh.type == DNM_FULL || lh.space == rh.space) && lh.swz == rh.swz))
    return 0;
  int p = 0;
  while ((1 << p) < P) ++p;
  const int shift = lh.type == DNM_PARITY ? 1 : 0;      // Parity: index = configuration >> 1, index bit j is spin j + 1
  const int packed = A->real_packed ? 1 : 0;            // index bit 0 is the lane of an element: F must leave it alone
  const int n = (int)lh.L - shift - p, f = n - 1 - p;
  if ((1 << p) != P || f < packed) return 0;
  if (lh.swz && f - packed < 2 * lh.swz - 4) return 0;  // pieces of 2^f amplitudes keep their internal order in both layouts
  const int fs = f + shift, ns = n + shift;             // the two fields as spins
  const int64_t fld = P - 1;
  struct Term { int64_t m, s; double c; };
  std::vector<Term> lo, hi;
  for (size_t i = 0; i < A->masks.size(); ++i)
    for (int64_t t = A->mask_offsets[i]; t < A->mask_offsets[i + 1]; ++t) {
      const int64_t m = A->masks[i], s = A->signs[(size_t)t];
      if ((m >> ns) == 0) { lo.push_back({m, s, A->real_coeffs[(size_t)t]}); continue; }
      if ((m >> fs) & fld) return 0;                    // a term that flips a rank bit AND the field it would move to
      auto swap = [&](int64_t v) {
        const int64_t d = ((v >> fs) ^ (v >> ns)) & fld;
        return v ^ (d << fs) ^ (d << ns);
      };
      hi.push_back({swap(m), swap(s), A->real_coeffs[(size_t)t]});
    }
  if (lo.empty() || hi.empty()) return 0;
  // the pieces of the packed operator sit one bit lower
  const int np = n - packed, fp = f - packed;
  dnm_subspace ld{}, rd{};
  ld.type = lh.type; ld.L = lh.L; ld.space = lh.space; ld.vec_swizzle = lh.swz;
  rd.type = rh.type; rd.L = rh.L; rd.space = rh.space; rd.vec_swizzle = rh.swz;
  const dnm_partition part{A->rank, A->nranks};
  dnm_mat *made[2] = {nullptr, nullptr};
  for (int which = 0; which < 2; ++which) {
    std::vector<Term> &T = which ? hi : lo;
    std::stable_sort(T.begin(), T.end(), [](const Term &a, const Term &b) { return a.m < b.m; });
    std::vector<int64_t> masks, offs, signs;
    std::vector<double> coeffs;
    for (size_t i = 0; i < T.size(); ++i) {
      if (i == 0 || T[i].m != T[i - 1].m) { masks.push_back(T[i].m); offs.push_back((int64_t)i); }
      signs.push_back(T[i].s);
      coeffs.push_back(T[i].c); coeffs.push_back(0.0);  // (one double per term is all a handle keeps: see dnm_mat_create)
    }
    offs.push_back((int64_t)T.size());
    int fl = A->flags & ~(0xff << DNM_MAT_AMIN_SHIFT);
    if (which == 1 && np - fp <= 8) {
      // layout B's masks live on the p exchanged bits and the top bit: a tile [0, a) + [f, n) holds them all and
      // leaves the bits right below f -- the top bits INSIDE a piece -- to the workgroup index, so that ranges of
      // workgroups are contiguous sub-pieces (dnm_mat_mult_local_part)
      const char *tb = knob("DNM_TILE_BITS");
      const int a = (tb ? atoi(tb) : 12) - (np - fp);
      if (a >= 2 && a <= 9) fl |= a << DNM_MAT_AMIN_SHIFT;
    } else {
      fl |= A->flags & (0xff << DNM_MAT_AMIN_SHIFT);
    }
    int rc = dnm_mat_create((int64_t)masks.size(), masks.data(), offs.data(), signs.data(), coeffs.data(), &ld, &rd, 0, fl,
                            &part, &made[which]);
    int ns_ = 0, nr_ = 0;
    if (rc == 0) rc = dnm_mat_exchange_plan(made[which], &ns_, nullptr, &nr_, nullptr);
    if (rc == 0 && (ns_ || nr_)) { set_error("transposed exchange: a pass is not rank-local"); rc = 1; }
    if (rc == 0 && made[which]->route != Route::Tiled) {
      set_error("transposed exchange: a part of the operator has no tiled plan"); rc = 1;
    }
    if (rc != 0) { delete made[0]; delete made[1]; return rc; }
  }
  A->tr_lo = made[0];
  A->tr_hi = made[1];
  A->tr_f = fp;
  *chosen = DNM_EXCHANGE_TRANSPOSE;
  return 0;
}

int dnm_mat_operator(const dnm_mat *A, int64_t *nmasks, int64_t *nterms, int64_t *masks, int64_t *mask_offsets,
                     int64_t *signs, double *coeffs) {
  DNM_CHECK(A && nmasks && nterms, "null argument");
  *nmasks = (int64_t)A->masks.size();
  *nterms = (int64_t)A->signs.size();
  if (masks) std::copy(A->masks.begin(), A->masks.end(), masks);
  if (mask_offsets) std::copy(A->mask_offsets.begin(), A->mask_offsets.end(), mask_offsets);
  if (signs) std::copy(A->signs.begin(), A->signs.end(), signs);
  if (coeffs) std::copy(A->real_coeffs.begin(), A->real_coeffs.end(), coeffs);
  return 0;
}

int dnm_mat_exchange_parts(const dnm_mat *A, dnm_mat **lo, dnm_mat **hi, int *f) {
  DNM_CHECK(A && lo && hi && f, "null argument");
  *lo = A->tr_lo; *hi = A->tr_hi; *f = A->tr_f;
  return 0;
}

int dnm_mat_sizes(const dnm_mat *A, int64_t *M, int64_t *N, int64_t *m_local, int64_t *n_local) {
  DNM_CHECK(A, "null matrix");
  if (M) *M = A->M;
  if (N) *N = A->N;
  if (m_local) *m_local = A->m_local;
  if (n_local) *n_local = A->n_local;
  return 0;
}

int dnm_mat_layouts(const dnm_mat *A, int *left, int *right) {
  DNM_CHECK(A, "null matrix");
  if (left) *left = A->use_sc3 ? A->left.host.sc3 : A->left.host.swz;
  if (right) *right = A->use_sc3 ? A->right.host.sc3 : A->right.host.swz;
  return 0;
}

int dnm_mat_is_real_packed(const dnm_mat *A, int *packed) {
  DNM_CHECK(A && packed, "null argument");
  *packed = A->real_packed ? 1 : 0;
  return 0;
}

int dnm_mat_precompute_diagonal(dnm_mat *A, void *stream) {
  DNM_CHECK(A && !A->host_only, "null or host-only matrix");
  DNM_CHECK(!A->real_packed || (A->use_sc3 && A->sc3->diag_mode == 1),
            "this real-packed operator evaluates its diagonal on the fly: nothing to precompute");
  // only when the first mask is the identity (bpetsc_template_1.c:177-180) and
  // left == right (operators.py:627-629)
  if (A->masks.empty() || A->masks[0] != 0) return 0;
  DNM_CHECK(A->nranks == 1 || A->route != Route::Tiled,
            "precomputed diagonal is not used by the partitioned tiled multiply");
  DNM_CHECK(A->M == A->N, "precompute_diagonal needs a square matrix");
  // (equal dimensions are not enough: the row kernels add diag[row] x[row], and between two different subspaces the
  // identity mask pairs row i with the column of the SAME state, if the right subspace holds it at all)
  DNM_CHECK(A->one_subspace,
            "precompute_diagonal needs the same subspace on both sides (this handle projects between two)");
  if (A->use_sc3) {
    // computed row by row in reference order, kept in the vectors' layout: the share needs a reference side (every share
    // of block order 0, whole vectors of the others) -- asked before anything is launched
    DNM_TRY(ref_side(*A->sc3->ly, row_range(*A->sc3->ly, A->sc3->T0, A->sc3->T1)));
    DNM_CHECK(A->row0 >= 0, "internal: a share with a reference side has no first reference row");
    DevBuf nat;
    DNM_TRY(nat.alloc((size_t)A->rows_local * sizeof(double)));
    DNM_TRY(launch_diag(A->dmsc, A->right.dev, A->rows_local, A->row0, (double *)nat.p, S(stream)));
    // (one double per position of the layout; a real-packed handle counts its vectors in pairs of positions)
    DNM_TRY(A->diag.alloc((size_t)A->m_local * (A->real_packed ? 2 : 1) * sizeof(double)));
    DNM_TRY(sc3_layout_copy_f64(*A->sc3->ly, (double *)A->diag.p, (const double *)nat.p, true, S(stream), A->sc3->T0,
                                A->sc3->T1, &A->sc3->perm));
    DNM_HIP(hipStreamSynchronize(S(stream)));      // `nat` is released on return
    A->have_diag = true;
    return 0;
  }
  DNM_TRY(A->diag.alloc((size_t)A->m_local * sizeof(double)));
  DNM_TRY(launch_diag(A->dmsc, A->right.dev, A->m_local, A->row0, (double *)A->diag.p, S(stream)));
  A->have_diag = true;
  return 0;
}

int dnm_mat_get_diagonal(dnm_mat *A, double *diag_host, void *stream) {
  DNM_CHECK(A && A->have_diag, "no precomputed diagonal");
  if (A->use_sc3) {       // handed out in reference order (row r of the matrix)
    DevBuf nat;
    DNM_TRY(nat.alloc((size_t)A->rows_local * sizeof(double)));
    DNM_TRY(sc3_layout_copy_f64(*A->sc3->ly, (double *)nat.p, (const double *)A->diag.p, false, S(stream), A->sc3->T0,
                                A->sc3->T1, &A->sc3->perm));
    return dnm_memcpy_d2h(diag_host, nat.p, (size_t)A->rows_local * sizeof(double), stream);
  }
  return dnm_memcpy_d2h(diag_host, A->diag.p, (size_t)A->m_local * sizeof(double), stream);
}

int dnm_mat_ownership(const dnm_mat *A, int64_t *row0, int64_t *m_local) {
  DNM_CHECK(A, "null matrix");
  // (internal SpinConserve layout: the rank's range of the layout -- the index space its windows are expressed in)
  if (row0) *row0 = A->use_sc3 ? (A->real_packed ? A->sc3->row0 / 2 : A->sc3->row0) : A->row0;
  if (m_local) *m_local = A->m_local;
  return 0;
}

int dnm_mat_column_ranges(dnm_mat *A, int64_t max_ranges, int64_t *ranges, int64_t *nranges) {
  DNM_CHECK(A && nranges && max_ranges >= 0 && (ranges || max_ranges == 0), "bad argument");
  *nranges = 0;
  if (!A->use_sc3) return 0;             // (other partitions: dnm_mat_column_chunks)
  const auto rg = A->sc3->ranges();
  *nranges = (int64_t)rg.size();
  const int64_t unit = A->real_packed ? 2 : 1;       // a real-packed handle counts pairs of positions (whole blocks: even)
  for (int64_t i = 0; i < *nranges && i < max_ranges; ++i) {
    ranges[2 * i] = rg[(size_t)i].first / unit;
    ranges[2 * i + 1] = rg[(size_t)i].second / unit;
  }
  return 0;
}

int dnm_mat_exchange_plan(const dnm_mat *A, int *nsend, dnm_xfer *sends, int *nrecv, dnm_xfer *recvs) {
  DNM_CHECK(A && nsend && nrecv, "null argument");
  *nsend = (int)A->plan.sends.size();
  *nrecv = (int)A->remote_passes.size();
  if (sends)
    for (size_t i = 0; i < A->plan.sends.size(); ++i)
      sends[i] = {A->plan.sends[i].partner, -1, A->plan.sends[i].offset, A->plan.sends[i].count};
  if (recvs)
    for (size_t i = 0; i < A->remote_passes.size(); ++i) {
      const auto &p = A->remote_passes[i];
      recvs[i] = {p->partner, (int32_t)i, p->src_off, (int64_t)1 << p->n_eff};
    }
  return 0;
}

int dnm_mat_norm_inf(dnm_mat *A, double *nrm, void *stream) {
  DNM_CHECK(A && nrm, "null argument");
  DNM_CHECK(!A->host_only, "host-only handle has no device tables");
  if (A->nrm != -1.0) {
    *nrm = A->nrm;
    return 0;
  }
  // The rows this handle sweeps, as runs of the reference order: [row0, row0 + rows_local) -- except a SpinConserve
  // share in a block order other than 0 (the solver's partition), which is no range of that order: its blocks, merged
  // where they follow each other in the reference order (one launch per run, once per handle: SpinConserve(36,18) on 8
  // ranks has a few hundred blocks per rank)
  std::vector<std::pair<int64_t, int64_t>> runs;
  if (A->use_sc3 && A->sc3->ly->order != 0) runs = sc3_ref_runs(*A->sc3->ly, A->sc3->T0, A->sc3->T1);
  else {
    DNM_CHECK(A->row0 >= 0, "internal: no first row in reference order");
    runs.push_back({A->row0, A->rows_local});
  }
  size_t nb = 0;
  for (const auto &r : runs) {
    DNM_CHECK(r.first >= 0 && r.second >= 0 && r.first + r.second <= A->left.host.dim,
              "internal: rows [%lld, %lld + %lld) outside the subspace", (long long)r.first, (long long)r.first,
              (long long)r.second);
    nb += (size_t)norm_num_blocks(r.second);
  }
  DNM_TRY(A->scratch.alloc(std::max<size_t>(nb, 1) * sizeof(double)));
  size_t at = 0;
  for (const auto &r : runs) {
    if (r.second == 0) continue;
    DNM_TRY(launch_norm(A->dmsc, A->left.dev, A->right.dev, r.second, r.first, (double *)A->scratch.p + at, S(stream)));
    at += (size_t)norm_num_blocks(r.second);
  }
  std::vector<double> h(nb);
  if (nb) DNM_TRY(dnm_memcpy_d2h(h.data(), A->scratch.p, nb * sizeof(double), stream));
  double best = 0.0;
  for (double v : h) best = std::max(best, v);
  if (A->nranks == 1) A->nrm = best;   // partitioned: caller reduces, then dnm_mat_set_norm
  *nrm = best;
  return 0;
}

int dnm_mat_set_norm(dnm_mat *A, double nrm) {
  DNM_CHECK(A, "null matrix");
  A->nrm = nrm;
  return 0;
}

int dnm_mat_plan_describe(const dnm_mat *A, char *buf, size_t buflen) {
  DNM_CHECK(A && buf && buflen, "null argument");
  std::string s;
  if (A->hypercube) {
    // a pass whose diagonal the kernel reads from tables (DevPass::dblock) says so at the end of its own line; the
    // others keep their text
    std::vector<std::string> notes[2];
    const std::vector<std::unique_ptr<PassOnDevice>> *lists[2] = {&A->local_passes, &A->remote_passes};
    for (int k = 0; k < 2; ++k)
      for (const auto &p : *lists[k]) notes[k].push_back(p->runs().dblock.empty() ? "" : " diag_tables=1");
    s = A->plan.describe(A->op, &notes[0], &notes[1]);
  }
  else if (A->use_sc3) {
    const Sc3Tab &T = A->sc3->ly->host;
    char tmp[512];
    if (A->sc3->tiled && A->sc3->graph)
      snprintf(tmp, sizeof tmp, "SpinConserve two-pass kernels on a bond graph, internal layout [T %d | W %d | Lo %d]: "
               "window pass (%zu workgroups, %d hops in LDS, %d gathered) then lo pass (%zu workgroups, %d hops in LDS, "
               "%d gathered), diagonal %s, coefficients %s\n", T.t, T.w, T.a, A->sc3->permB.size(), A->sc3->op.nldsB,
               A->sc3->op.ngatB, A->sc3->permA.size() / 8, A->sc3->op.nldsA, A->sc3->op.ngatA,
               A->sc3->diag_mode == 2 ? "on the fly" : (A->sc3->diag_mode == 1 ? "cached" : "none"),
               A->sc3->sym ? "real symmetric" : "complex");
    else if (A->sc3->tiled)
      snprintf(tmp, sizeof tmp, "SpinConserve two-pass kernels, internal layout [T %d | W %d | Lo %d]: window pass (%zu "
               "workgroups, %d bonds in LDS, %d gathered) then lo pass (%zu workgroups, %d bonds in LDS, %d gathered), "
               "diagonal %s, coefficients %s\n", T.t, T.w, T.a, A->sc3->permB.size(), T.w - 1,
               __builtin_popcountll(A->sc3->op.bondsB), A->sc3->permA.size() / 8, T.a - 1,
               __builtin_popcountll(A->sc3->op.bondsA),
               A->sc3->diag_mode == 2 ? "on the fly" : (A->sc3->diag_mode == 1 ? "cached" : "none"),
               A->sc3->sym ? "real symmetric" : "complex");
    else
      snprintf(tmp, sizeof tmp, "SpinConserve row kernel, internal layout [T %d | W %d | Lo %d] (positions by table)\n",
               T.t, T.w, T.a);
    s = tmp;
  } else if (A->sc_pair)
    s = A->scblock.lb ? "SpinConserve kernel, block form (" + std::to_string(A->scblock.lb) +
                            " low bits per workgroup in LDS, high bonds as block runs)\n"
                      : std::string("SpinConserve kernel (one row per thread, incremental colex rank)\n");
  else s = A->nranks > 1 ? "generic row-gather kernel (rows split in index order, columns through a window)\n"
                         : "generic row-gather kernel (non-hypercube subspace pair)\n";
  if (A->hypercube && !A->plan.use_tiled) s += "generic row-gather kernel in use\n";
  if (A->route == Route::Tiled) {
    // masks of many terms run as table records (plan.h: DevTab); said only when there are any: the plans without keep their text
    size_t ntab = 0, nquad = 0;
    for (const auto &p : A->local_passes) { ntab += p->whole.tabs.size(); nquad += p->whole.desc.loop[LP_COUNT] - p->whole.desc.loop[0]; }
    for (const auto &p : A->remote_passes) { ntab += p->whole.tabs.size(); nquad += p->whole.desc.loop[LP_COUNT] - p->whole.desc.loop[0]; }
    if (ntab) s += "table records: " + std::to_string(ntab) + " (beside " + std::to_string(nquad) + " records of four terms)\n";
    // (flip-flop records -- plan.h: DevFlip -- add no line: tests pin the line count of the chain plans; dnm_mat_export_flip)
  }
  snprintf(buf, buflen, "%s", s.c_str());
  return 0;
}

int dnm_mat_export_pass(const dnm_mat *A, int remote, int idx, void *desc_out, size_t desc_bytes,
                        void *quads_out, size_t quad_bytes, int max_quads, int *nquads) {
  const PassOnDevice *p;
  DNM_CHECK(nquads, "null argument");
  DNM_TRY(export_lookup(A, remote, idx, &p));
  return export_records(p->whole, desc_out, desc_bytes, quads_out, quad_bytes, max_quads, nquads, true);
}

int dnm_mat_export_tabs(const dnm_mat *A, int remote, int idx, void *tabs_out, size_t tab_bytes, int max_tabs, int *ntabs,
                        double *vals_out, int64_t max_vals, int64_t *nvals) {
  const PassOnDevice *p;
  DNM_CHECK(ntabs && nvals, "null argument");
  DNM_TRY(export_lookup(A, remote, idx, &p));
  *ntabs = (int)p->whole.tabs.size();
  *nvals = (int64_t)p->whole.tabvals.size();
  DNM_TRY(export_copy(p->whole.tabs, tabs_out, tab_bytes, max_tabs, "DevTab", "record"));
  return export_copy(p->whole.tabvals, vals_out, sizeof(double), max_vals, "double", "table");
}

int dnm_mat_export_dtile(const dnm_mat *A, int remote, int idx, double *out, int64_t n) {
  const PassOnDevice *p;
  DNM_CHECK(out, "null argument");
  DNM_TRY(export_lookup(A, remote, idx, &p));
  DNM_CHECK((int64_t)p->whole.dtile.size() == n, "the pass has %zu tabulated diagonal entries, not %lld",
            p->whole.dtile.size(), (long long)n);
  return export_copy(p->whole.dtile, out, sizeof(double), n, "double", "table");
}

int dnm_mat_export_flip(const dnm_mat *A, int remote, int idx, void *flips_out, size_t flip_bytes, int max_flips,
                        int *nflips, uint32_t *loops_out, double *dconst) {
  const PassOnDevice *p;
  DNM_CHECK(nflips, "null argument");
  DNM_TRY(export_lookup(A, remote, idx, &p));
  *nflips = p->reduced ? (int)p->reduced->flips.size() : -1;      // -1: the pass runs on its generic records
  if (!p->reduced) return 0;
  if (loops_out) memcpy(loops_out, p->reduced->flip.loop, sizeof(p->reduced->flip.loop));
  if (dconst) *dconst = p->reduced->flip.dconst;
  return export_copy(p->reduced->flips, flips_out, flip_bytes, max_flips, "DevFlip", "record");
}

int dnm_mat_export_flip_pass(const dnm_mat *A, int remote, int idx, void *desc_out, size_t desc_bytes, void *quads_out,
                             size_t quad_bytes, int max_quads, int *nquads, double *dtile_out, int64_t max_dtile,
                             int64_t *ndtile) {
  const PassOnDevice *p;
  DNM_CHECK(nquads && ndtile, "null argument");
  DNM_TRY(export_lookup(A, remote, idx, &p));
  DNM_CHECK(p->reduced, "the pass has no flip-flop form");
  *ndtile = (int64_t)p->reduced->dtile.size();
  DNM_TRY(export_records(*p->reduced, desc_out, desc_bytes, quads_out, quad_bytes, max_quads, nquads, false));
  return export_copy(p->reduced->dtile, dtile_out, sizeof(double), max_dtile, "double", "table");
}

int dnm_mat_export_diag_tables(const dnm_mat *A, int remote, int idx, double *dblock_out, int64_t max_dblock,
                               int64_t *ndblock, double *dtile_out, int64_t max_dtile, int64_t *ndtile,
                               uint64_t *masks_out, int *nmasks) {
  const PassOnDevice *p;
  DNM_CHECK(ndblock && ndtile && nmasks, "null argument");
  DNM_TRY(export_lookup(A, remote, idx, &p));
  const PassRecords &r = p->runs();
  const bool have = !r.dblock.empty();
  *ndblock = (int64_t)r.dblock.size();
  *ndtile = have ? (int64_t)r.dtile_sections().size() : 0;
  *nmasks = have ? (int)r.desc.dsel_n : 0;
  if (!have) return 0;
  if (masks_out) memcpy(masks_out, r.desc.dsel_mask, sizeof(r.desc.dsel_mask));
  DNM_TRY(export_copy(r.dblock, dblock_out, sizeof(double), max_dblock, "double", "table"));
  return export_copy(r.dtile_sections(), dtile_out, sizeof(double), max_dtile, "double", "table");
}

// One table of the SpinConserve passes as its builder left it on the host (sc3_tables.cpp), by name: rowsel needT hops
// wnb ptab pcoef permA permB bond dlo dt_sign dt_coef dt_group, the bytes the device gets; "op": what the kernels are
// handed beside the tables (include/dynamite_amd.h has the order).  Null out: the size alone.
int dnm_mat_export_sc3(const dnm_mat *A, const char *name, void *out, size_t max_bytes, size_t *nbytes) {
  DNM_CHECK(A && name && nbytes, "null argument");
  DNM_CHECK(A->use_sc3 && A->sc3, "the operator does not run on the SpinConserve layout's passes");
  const Sc3Mat &M = *A->sc3;
  const std::string n = name;
  const void *src = nullptr;
  size_t len = 0;
  std::vector<unsigned char> packed;
#define DNM_SC3_TABLE(NAME_)                                        \
  if (n == #NAME_) {                                                \
    src = M.NAME_.data();                                           \
    len = M.NAME_.size() * sizeof(M.NAME_[0]);                      \
  } else
  DNM_SC3_TABLE(rowsel) DNM_SC3_TABLE(needT) DNM_SC3_TABLE(hops) DNM_SC3_TABLE(wnb) DNM_SC3_TABLE(ptab)
  DNM_SC3_TABLE(pcoef) DNM_SC3_TABLE(permA) DNM_SC3_TABLE(permB) DNM_SC3_TABLE(bond) DNM_SC3_TABLE(dlo)
  DNM_SC3_TABLE(dt_sign) DNM_SC3_TABLE(dt_coef) DNM_SC3_TABLE(dt_group)
#undef DNM_SC3_TABLE
  if (n == "op") {
    const Sc3Op &O = M.op;
    const uint64_t u[3] = {O.present, O.bondsA, O.bondsB};
    std::vector<int32_t> v = {O.ndt, O.ngroups, (int32_t)O.glo[0], (int32_t)O.glo[1], (int32_t)O.glo[2], (int32_t)O.glo[3],
                              O.nldsA, O.ngatA, O.nldsB, O.ngatB, O.nhp};
    v.insert(v.end(), O.ptab_row, O.ptab_row + SC3_MAXA + 2);
    for (int f : {(int)M.tiled, (int)M.graph, (int)M.sym, (int)M.real, M.diag_mode}) v.push_back(f);
    packed.resize(sizeof u + v.size() * sizeof(int32_t));
    memcpy(packed.data(), u, sizeof u);
    memcpy(packed.data() + sizeof u, v.data(), v.size() * sizeof(int32_t));
    src = packed.data();
    len = packed.size();
  } else {
    DNM_CHECK(false, "no table '%s' of the SpinConserve passes", name);
  }
  *nbytes = len;
  if (!out) return 0;
  DNM_CHECK(max_bytes >= len, "table '%s' has %zu bytes, the buffer %zu", name, len, max_bytes);
  if (len) memcpy(out, src, len);
  return 0;
}

// What the block form of a SpinConserve pair in reference order launches (setup_sc_block): fields[0..5] = low bits per
// block (0: the handle does not run the block form, everything else is 0 then), first and last high part, swizzle,
// entries of the block order, workgroups of a launch (sc_block_grid); perm_out != null: the block order itself
// (0xffffffff: a workgroup without a block), copied from the device.  Reads only.
int dnm_mat_export_sc_block(const dnm_mat *A, int64_t *fields, uint32_t *perm_out, int64_t max_perm) {
  DNM_CHECK(A && fields, "null argument");
  for (int i = 0; i < 6; ++i) fields[i] = 0;
  if (A->host_only || A->route != Route::ScBlock) return 0;
  const ScBlock &b = A->scblock;
  fields[0] = b.lb;
  fields[1] = b.h_first;
  fields[2] = b.h_last;
  fields[3] = b.swizzle;
  fields[4] = b.perm ? b.nperm : 0;
  fields[5] = sc_block_grid(b);
  if (!perm_out || !b.perm) return 0;
  DNM_CHECK(max_perm >= b.nperm, "the block order has %lld entries, the buffer %lld", (long long)b.nperm,
            (long long)max_perm);
  return dnm_memcpy_d2h(perm_out, b.perm, (size_t)b.nperm * sizeof(uint32_t), nullptr);
}

int dnm_mat_plan_counts(const dnm_mat *A, int *n_local_passes, int *n_remote_passes, int *tiled,
                        int *B, int *logR, int *n_loc) {
  DNM_CHECK(A, "null matrix");
  if (n_local_passes) *n_local_passes = (int)A->local_passes.size();
  if (n_remote_passes) *n_remote_passes = (int)A->remote_passes.size();
  if (tiled) *tiled = A->route == Route::Tiled ? 1 : 0;
  if (B) *B = A->plan.cfg.B;
  if (logR) *logR = A->plan.cfg.logR;
  if (n_loc) *n_loc = A->plan.n_loc;
  return 0;
}

int dnm_mat_plan_launches(const dnm_mat *A, int *n) {
  DNM_CHECK(A && n, "null argument");
  *n = A->route == Route::Tiled ? (int)A->local_passes.size() : 1;
  return 0;
}

}  // extern "C"

dnm_mat::~dnm_mat() {
  delete tr_lo;
  delete tr_hi;
}
