// The host builder of the tiled kernel's records (csrc/passes.cpp, csrc/plan.cpp) on its own, for a run under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_diag_tables_host.py): a plain program that builds the
// passes of three chains as dnm_mat_create does -- generic form, flip-flop form, then the diagonal as tables
// (DevPass::dblock) -- and checks every row of the tables against the diagonal evaluated term by term.  Nothing here
// touches a device: the few symbols of the library that the two sources reach for (error text, the device buffer's
// release, the list of kernel instances, the handle's destructor) are defined below.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../dynamite_amd/csrc/passes.h"

namespace dnm {
static char g_err[1024];
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
void DevBuf::release() {}
bool tile_config_supported(int B, int logR) { return (B == 8 && logR == 2) || (B == 10 && (logR == 2 || logR == 3)); }
}  // namespace dnm
dnm_mat::~dnm_mat() {}

using namespace dnm;

static int failures = 0;
#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      ++failures;                          \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                 \
      printf("\n");                        \
    }                                      \
  } while (0)

// a chain in MSC form: bonds a (XX + YY) + d ZZ, fields h_i Z_i, all coefficients dyadic
static void chain(dnm_mat &A, int L, double a, double d, bool fields) {
  // mask 0: the diagonal
  A.masks.push_back(0);
  A.mask_offsets.push_back(0);
  for (int i = 0; i + 1 < L; ++i)
    if (d != 0.0) {
      A.signs.push_back((int64_t)3 << i);
      A.real_coeffs.push_back(d);
    }
  for (int i = 0; fields && i < L; ++i) {
    const double h = ((7 * i + 3) % 17 - 8) / 8.0;
    if (h == 0.0) continue;
    A.signs.push_back((int64_t)1 << i);
    A.real_coeffs.push_back(h);
  }
  // XX + YY on (i, i + 1): mask 3 << i, terms (sign 0, a) and (sign 3 << i, -a) evaluated on the column
  for (int i = 0; i + 1 < L; ++i) {
    A.mask_offsets.push_back((int64_t)A.signs.size());
    A.masks.push_back((int64_t)3 << i);
    A.signs.push_back(0);
    A.real_coeffs.push_back(a);
    A.signs.push_back((int64_t)3 << i);
    A.real_coeffs.push_back(-a);
  }
  A.mask_offsets.push_back((int64_t)A.signs.size());
}

static int run(const char *name, int L, double a, double d, bool fields, int B, int logR, int rank, int nranks,
               bool expect_flip) {
  dnm_mat A;
  chain(A, L, a, d, fields);
  A.left.host.type = A.right.host.type = DNM_FULL;
  A.left.host.L = A.right.host.L = L;
  A.host_only = true;
  A.hypercube = true;
  A.rank = rank;
  A.nranks = nranks;
  DNM_TRY(build_opform(A, &A.op));
  PlanConfig cfg;
  cfg.B = B;
  cfg.logR = logR;
  cfg.mode = 2;
  cfg.amin = 3;
  cfg.gbits = 3;
  DNM_TRY(make_plan(A.op, rank, nranks, cfg, &A.plan));
  EXPECT(A.plan.use_tiled, "%s: not tiled", name);
  if (!A.plan.use_tiled) return 0;
  for (auto *lst : {&A.plan.local, &A.plan.remote})
    for (const PassSpec &ps : *lst) {
      auto &out = lst == &A.plan.local ? A.local_passes : A.remote_passes;
      out.emplace_back(new PassOnDevice());
      DNM_TRY(build_pass(A, ps, out.back().get()));
    }
  decide_flip_bonds(&A);
  EXPECT(expect_flip == !A.flip_bonds.empty(), "%s: flip-flop form %d", name, (int)!A.flip_bonds.empty());
  for (size_t i = 0; i < A.plan.local.size(); ++i) DNM_TRY(build_flip_pass(A, A.plan.local[i], A.local_passes[i].get()));
  for (auto *v : {&A.local_passes, &A.remote_passes})
    for (auto &p : *v) DNM_TRY(build_diag_tables(A, p.get()));
  // what the exchanges take back from the diagonal: c on the rows whose two bits agree
  std::vector<std::pair<uint64_t, double>> exch;
  for (size_t i = 0; i < A.flip_bonds.size(); ++i)
    if (A.flip_bonds[i].exch) exch.push_back({A.op.masks[i].mask, A.flip_bonds[i].c});
  int checked = 0;
  for (auto &pp : A.local_passes) {
    const PassRecords &r = pp->runs();
    const DevPass &P = r.desc;
    if (!P.has_diag) {
      EXPECT(r.dblock.empty(), "%s: tables without a diagonal", name);
      continue;
    }
    EXPECT(!r.dblock.empty(), "%s: the diagonal pass has no tables", name);
    if (r.dblock.empty()) continue;
    const int Bp = P.tile_bits, n = P.n_eff;
    EXPECT(r.dblock.size() == (size_t)1 << (n - Bp), "%s: %zu workgroup entries", name, r.dblock.size());
    EXPECT(r.dtile_sections().size() == ((size_t)1 << Bp) << P.dsel_n, "%s: %zu table entries", name,
           r.dtile_sections().size());
    uint64_t tb = 0;
    for (int j = 0; j < P.nseg; ++j) tb |= (((uint64_t)1 << P.seg_len[j]) - 1) << P.seg_pos[j];
    for (uint64_t row = 0; row < ((uint64_t)1 << n); ++row) {
      uint64_t t = 0, b = 0, sec = 0;
      for (int j = 0; j < P.nseg; ++j) t |= ((row >> P.seg_pos[j]) & (((uint64_t)1 << P.seg_len[j]) - 1)) << P.seg_off[j];
      for (int j = 0; j < P.nbseg; ++j) b |= ((row >> P.bseg_pos[j]) & (((uint64_t)1 << P.bseg_len[j]) - 1)) << P.bseg_off[j];
      const uint64_t sbase = P.sign_base | (row & ~tb);
      for (uint32_t i = 0; i < P.dsel_n; ++i) sec |= (uint64_t)parity64(sbase & P.dsel_mask[i]) << i;
      const double got = r.dblock[b] + r.dtile_sections()[(sec << Bp) + t];
      const uint64_t g = ((uint64_t)rank << A.plan.n_loc) | row;
      double want = 0.0;
      for (int64_t k = A.mask_offsets[0]; k < A.mask_offsets[1]; ++k)
        want += parity64(g & (uint64_t)A.signs[k]) ? -A.real_coeffs[k] : A.real_coeffs[k];
      for (const auto &e : exch)
        if (!parity64(g & e.first)) want -= e.second;
      if (got != want) {
        EXPECT(false, "%s: row %llu: tables %.17g, terms %.17g", name, (unsigned long long)row, got, want);
        return 0;
      }
    }
    ++checked;
  }
  EXPECT(checked == 1, "%s: %d passes checked", name, checked);
  printf("%-28s L=%d B=%d logR=%d rank %d/%d: ok\n", name, L, B, logR, rank, nranks);
  return 0;
}

int main() {
  setenv("DNM_EXPERIMENTAL", "1", 1);
  int rc = 0;
  rc |= run("isotropic chain, fields", 14, 0.25, 0.25, true, 10, 2, 0, 1, true);
  rc |= run("anisotropic chain, fields", 14, 0.25, 0.125, true, 8, 2, 1, 2, true);
  rc |= run("xxz chain", 14, 0.25, 0.125, false, 10, 3, 3, 4, true);
  setenv("DNM_FLIPFLOP", "0", 1);
  rc |= run("anisotropic, generic records", 14, 0.25, 0.125, true, 10, 2, 3, 4, false);
  if (rc) {
    ++failures;
    printf("FAILED: %s\n", g_err);
  }
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
