// C ABI: products of single-site operators on a Full-space state (dnm_site_ops_plan, dnm_site_ops_apply) and the
// exponential of a diagonal operator (dnm_mat_expm_diagonal).  Plan and kernels: site_ops.h, site_ops_kernels.hip.
#include "site_ops.h"

#include "mat.h"

using namespace dnm;
static hipStream_t S(void *s) { return (hipStream_t)s; }

// what the plan and the call check alike, before any device call
static int site_ops_check(const dnm_subspace *sub, const double *mats) {
  const char *what = "site operators";
  DNM_CHECK(sub && mats, "%s: null argument", what);
  DNM_CHECK(sub->type == DNM_FULL, "%s: subspace type %d: the product of single-site operators acts on the Full space "
            "(expand the state first)", what, sub->type);
  DNM_CHECK(sub->site_perm == nullptr, "%s: site_perm given for a subspace that is not SpinConserve", what);
  DNM_CHECK(sub->L >= 1 && sub->L <= SITE_OPS_MAX_L, "%s: L=%lld outside [1, %d]", what, (long long)sub->L,
            SITE_OPS_MAX_L);
  DNM_CHECK(sub->vec_swizzle == 0 || (sub->vec_swizzle >= 5 && sub->vec_swizzle <= 24),
            "%s: vec_swizzle %d: the shift of a swizzled vector lies in [5, 24]", what, sub->vec_swizzle);
  for (int64_t i = 0; i < 8 * sub->L; ++i)
    DNM_CHECK(std::isfinite(mats[i]), "%s: the matrix of site %lld has an entry that is not finite", what,
              (long long)(i / 8));
  return 0;
}

extern "C" {

int dnm_site_ops_plan(const dnm_subspace *sub, const double *mats_host, int *tile_bits, int *npasses, int8_t *site_pass,
                      int *nworkgroups, size_t *lds_bytes) {
  DNM_TRY(site_ops_check(sub, mats_host));
  SiteOpsPlan p;
  site_ops_plan((int)sub->L, sub->vec_swizzle, mats_host, site_ops_tile_bits(), &p);
  if (tile_bits) *tile_bits = p.tile_bits;
  if (npasses) *npasses = p.npasses;
  if (site_pass) memcpy(site_pass, p.site_pass, (size_t)sub->L);
  if (nworkgroups) *nworkgroups = p.nwg;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

int dnm_site_ops_apply(const void *x, void *y, const dnm_subspace *sub, const double *mats_host, void *stream) {
  DNM_CHECK(x && y, "site operators: null argument");
  DNM_TRY(site_ops_check(sub, mats_host));
  SiteOpsPlan p;
  site_ops_plan((int)sub->L, sub->vec_swizzle, mats_host, site_ops_tile_bits(), &p);
  if (p.identity) {
    if (x != y) DNM_TRY(vk_copy(y, x, (int64_t)1 << sub->L, S(stream)));
    return 0;
  }
  // (the first pass reads x, every later one works on y in place)
  for (size_t i = 0; i < p.passes.size(); ++i)
    DNM_TRY(launch_site_ops_pass(i ? y : x, y, p.passes[i], p.tile_bits, p.nwg, S(stream)));
  return 0;
}

int dnm_mat_expm_diagonal(dnm_mat *A, const void *x, void *y, double s_re, double s_im, void *stream) {
  const char *what = "exponential of a diagonal operator";
  DNM_CHECK(A && x && y, "%s: null argument", what);
  DNM_CHECK(std::isfinite(s_re) && std::isfinite(s_im), "%s: the factor is not finite", what);
  for (int64_t m : A->masks) DNM_CHECK(m == 0, "%s: operator is not diagonal (it has the mask %lld)", what, (long long)m);
  DNM_CHECK(!A->real_packed, "%s: a real-packed handle multiplies packed real vectors (build the complex handle)", what);
  DNM_CHECK(!A->host_only, "%s: a host-only handle", what);
  DNM_CHECK(A->nranks == 1, "%s: a handle on %d ranks", what, A->nranks);
  DNM_CHECK(A->M == A->N && A->one_subspace, "%s: needs one subspace on both sides", what);
  const int64_t n = A->m_local;
  // the zero operator and s = 0: y = x, bit for bit
  if (A->masks.empty() || (s_re == 0.0 && s_im == 0.0)) {
    if (x != y) DNM_TRY(vk_copy(y, x, n, S(stream)));
    return 0;
  }
  if (!A->have_diag) DNM_TRY(dnm_mat_precompute_diagonal(A, stream));
  DNM_CHECK(A->have_diag, "%s: the handle has no diagonal", what);
  // the cache is indexed by row; a swizzled Full / Parity vector by position.  In the SpinConserve internal layout
  // the cache lies as the vectors do.
  const int swz = A->use_sc3 ? 0 : A->right.host.swz;
  return launch_expm_diagonal(x, y, A->cached_diag(), n, swz, s_re, s_im, S(stream));
}

}  // extern "C"
