// The host builder of the SpinConserve passes' tables (csrc/sc3_tables.cpp) on its own, for a run under AddressSanitizer
// and UndefinedBehaviorSanitizer (tests/test_sc3_tables_host.py): a plain program that builds the (6,4) layout and the
// tables of a few dyadic operators as dnm_mat_create does, and checks every table against its definition by brute force
// over the states of the subspace.  Nothing here touches a device: the few symbols of the library that the source
// reaches for (error text, the device buffer) are defined below; the buffer "uploads" into host memory, so that the two
// upload() functions run too.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

#include "../dynamite_amd/csrc/dnm_common.h"
#include "../dynamite_amd/csrc/sc3.h"
#include "../dynamite_amd/csrc/sc3_shape.h"

namespace dnm {
static char g_err[1024];
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
int DevBuf::alloc(size_t nbytes) {
  release();
  p = malloc(nbytes ? nbytes : 16);
  bytes = nbytes;
  return p ? 0 : 1;
}
int DevBuf::upload(const void *host, size_t nbytes) {
  if (alloc(nbytes)) return 1;
  if (nbytes) memcpy(p, host, nbytes);
  return 0;
}
void DevBuf::release() {
  free(p);
  p = nullptr;
  bytes = 0;
}
}  // namespace dnm

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

static int pc(uint64_t v) { return __builtin_popcountll(v); }
// rank of a pattern among the patterns with as many ones, ascending: counted, not computed
static int rank_of(uint32_t v) {
  int r = 0;
  for (uint32_t u = 0; u < v; ++u) r += pc(u) == pc(v);
  return r;
}

// an operator in MSC form (masks ascending, the diagonal first), all coefficients dyadic
struct Msc {
  struct Term { uint64_t mask, sign; double c; };
  std::vector<Term> terms;
  std::vector<int64_t> masks, offs, signs;
  std::vector<double> coef;
  void zz(int i, int j, double d) { terms.push_back({0, (1ull << i) | (1ull << j), d}); }
  void z(int i, double h) { terms.push_back({0, 1ull << i, h}); }
  void hop(int i, int j, double a) {      // a (XX + YY): element 2a both ways
    const uint64_t m = (1ull << i) | (1ull << j);
    terms.push_back({m, 0, a});
    terms.push_back({m, m, -a});
  }
  void hop_imag(int i, int j, double c) { terms.push_back({(1ull << i) | (1ull << j), 1ull << std::max(i, j), c}); }
  // XParity's composed hop between spin i and spin L-1: every spin but those two flips
  void xhop(int L, int i, double a) { terms.push_back({((1ull << (L - 1)) - 1) & ~(1ull << i), 0, a}); }
  void finish() {
    std::stable_sort(terms.begin(), terms.end(), [](const Term &x, const Term &y) { return x.mask < y.mask; });
    for (size_t i = 0; i < terms.size(); ++i) {
      if (i == 0 || terms[i].mask != terms[i - 1].mask) {
        masks.push_back((int64_t)terms[i].mask);
        offs.push_back((int64_t)i);
      }
      signs.push_back((int64_t)terms[i].sign);
      coef.push_back(terms[i].c);
    }
    offs.push_back((int64_t)terms.size());
  }
};

static Msc chain12() {
  Msc o;
  for (int i = 0; i + 1 < 12; ++i) { o.hop(i, i + 1, 0.25); o.zz(i, i + 1, 0.125); }
  for (int i = 0; i < 12; ++i) if ((7 * i + 3) % 17 != 8) o.z(i, ((7 * i + 3) % 17 - 8) / 8.0);
  o.finish();
  return o;
}
static std::vector<std::pair<int, int>> graph13_pairs() {
  std::vector<std::pair<int, int>> p;
  for (int i = 0; i < 13; ++i) p.push_back({std::min(i, (i + 1) % 13), std::max(i, (i + 1) % 13)});
  for (auto e : {std::make_pair(0, 5), std::make_pair(2, 8), std::make_pair(1, 11), std::make_pair(7, 12), std::make_pair(10, 12)})
    p.push_back(e);
  return p;
}
static Msc graph13(bool complex_pair) {
  Msc o;
  for (auto e : graph13_pairs()) { o.hop(e.first, e.second, 0.25); o.zz(e.first, e.second, 0.125); }
  if (complex_pair) o.hop_imag(2, 8, 0.5);
  o.finish();
  return o;
}
static Msc xparity12() {
  Msc o;
  for (int i = 0; i + 1 < 11; ++i) { o.hop(i, i + 1, 0.25); o.zz(i, i + 1, 0.5); }
  o.hop(1, 7, 0.125);
  o.xhop(12, 10, 0.25);
  o.xhop(12, 3, 0.5);
  o.finish();
  return o;
}
// ZZ between five different spins of Lo and spins outside it: five Lo sign patterns, one more than the passes take
static Msc manygroups12() {
  Msc o;
  for (int i = 0; i + 1 < 12; ++i) o.hop(i, i + 1, 0.25);
  for (int i = 0; i < 5; ++i) o.zz(i, i + 6, 0.25 * (i + 1));
  o.finish();
  return o;
}

// ---- the layout ---------------------------------------------------------------------------------------------
static void check_layout(const char *name, const Sc3Layout &ly) {
  const Sc3Tab &S = ly.host;
  const int a = S.a, w = S.w, L = S.L, k = S.k;
  // the non-padding positions, walked as the head of sc3.h describes the layout
  std::set<int64_t> want;
  int64_t pos = 0;
  for (uint32_t T : ly.tseq) {
    EXPECT(ly.ibase[T] == pos, "%s: block %u starts at %lld, not %lld", name, T, (long long)ly.ibase[T], (long long)pos);
    for (int cw = 0; cw <= w; ++cw) {
      const int kl = k - pc(T) - cw;
      if (kl < 0 || kl > a) continue;
      for (int wr = 0; wr < S.nw[cw]; ++wr, pos += S.pitch[kl])
        for (int c = 0; c < S.nl[kl]; ++c) want.insert(pos + c);
    }
  }
  EXPECT(pos == S.nint, "%s: the layout has %lld positions, its rows %lld", name, (long long)S.nint, (long long)pos);
  std::set<int64_t> got;
  for (uint64_t s = 0; s < (1ull << L); ++s)
    if (pc(s) == k) got.insert(sc3_pos(s, S));
  EXPECT((int64_t)got.size() == ly.dim, "%s: sc3_pos hits %zu positions for %lld states", name, got.size(), (long long)ly.dim);
  EXPECT(got == want, "%s: sc3_pos is no bijection onto the non-padding positions", name);
  // w_nb: byte b of a pattern's 16 = the rank of its partner under the bond (b, b+1) inside W, or the zero row
  bool ok = ly.w_nb.size() == 2 * ly.w_pat.size();
  for (int cw = 0; ok && cw <= w; ++cw)
    for (int wr = 0; wr < S.nw[cw]; ++wr) {
      const uint32_t v = ly.w_pat[S.w_off[cw] + wr];
      ok = ok && pc(v) == cw && rank_of(v) == wr;
      for (int b = 0; b < 16; ++b) {
        const int byte = (int)((ly.w_nb[2 * (size_t)(S.w_off[cw] + wr) + b / 8] >> (8 * (b % 8))) & 0xff);
        const bool acts = b < w - 1 && ((v >> b) & 1u) != ((v >> (b + 1)) & 1u);
        ok = ok && byte == (acts ? rank_of(v ^ (3u << b)) : S.nw[cw]);
      }
    }
  EXPECT(ok, "%s: w_nb", name);
  // host_h: host with every position halved
  const Sc3Tab &H = ly.host_h;
  ok = H.nint * 2 == S.nint && H.L == S.L && H.k == S.k && H.a == a && H.w == w && H.t == S.t && H.nbase == S.nbase &&
       H.ncoff == S.ncoff && H.lo_pat == S.lo_pat && H.w_pat == S.w_pat && H.lo_rank == S.lo_rank && H.w_rank == S.w_rank &&
       H.w_nb == S.w_nb && H.cbin == S.cbin && H.lo_rlo == S.lo_rlo && H.lo_rhi == S.lo_rhi && H.nck == S.nck;
  for (size_t i = 0; i < ly.ibase.size(); ++i) ok = ok && (ly.ibase[i] < 0 ? H.ibase[i] == -1 : H.ibase[i] * 2 == ly.ibase[i]);
  for (size_t i = 0; i < ly.icoff.size(); ++i) ok = ok && H.icoff[i] * 2 == ly.icoff[i];
  for (int j = 0; j <= a; ++j) ok = ok && H.pitch[j] * 2 == S.pitch[j] && H.nl[j] == S.nl[j] && H.lo_off[j] == S.lo_off[j];
  for (int j = 0; j <= w; ++j) ok = ok && H.nw[j] == S.nw[j] && H.w_off[j] == S.w_off[j] && H.rs[j] == S.rs[j];
  EXPECT(ok, "%s: host_h is not host halved", name);
}

// ---- the hops ------------------------------------------------------------------------------------------------
static void check_hops(const char *name, const Sc3Mat &M, const Msc &o, bool xparity, bool expect_all_kinds) {
  const Sc3Tab &S = M.ly->host;
  const int a = S.a, w = S.w, L = S.L;
  const int n[4] = {M.op.nldsA, M.op.ngatA, M.op.nldsB, M.op.ngatB};
  EXPECT((int)M.hops.size() == std::max(1, n[0] + n[1] + n[2] + n[3]), "%s: %zu hop records", name, M.hops.size());
  if (expect_all_kinds) EXPECT(n[0] && n[1] && n[2] && n[3], "%s: hop kinds %d %d %d %d", name, n[0], n[1], n[2], n[3]);
  auto field = [&](int b) { return b < a ? 0 : (b < a + w ? 1 : 2); };
  int live = 0;
  for (size_t m = 0; m < o.masks.size(); ++m) {
    const uint64_t mk = (uint64_t)o.masks[m];
    if (mk == 0 || (pc(mk) & 1)) continue;
    ++live;
    // the two spins: a pair hop's own, or (XParity's composed hops) the one spin below L-1 the mask leaves out and L-1
    int i, j;
    if (pc(mk) == 2) { i = __builtin_ctzll(mk); j = 63 - __builtin_clzll(mk); }
    else { EXPECT(xparity && pc(mk) == L - 2, "%s: mask %llx", name, (unsigned long long)mk); i = __builtin_ctzll(~mk); j = L - 1; }
    const int fi = field(i), fj = field(j);
    const int want = fi == 0 ? (fj == 0 ? 0 : 1) : (fi == 1 && fj == 1 ? 2 : 3);
    int found = 0, part = -1;
    for (int q = 0, base = 0; q < 4; base += n[q], ++q)
      for (int h = base; h < base + n[q]; ++h) {
        const Sc3Hop &H = M.hops[h];
        if ((((uint64_t)H.mT << (a + w)) | ((uint64_t)H.mW << a) | H.mLo) != mk) continue;
        ++found;
        part = q;
        EXPECT(H.half == pc(mk) / 2, "%s: mask %llx: half %d", name, (unsigned long long)mk, H.half);
        EXPECT(H.dfield == (pc(mk) == 2 ? fi : 3) && H.dbit == i - (fi == 0 ? 0 : (fi == 1 ? a : a + w)),
               "%s: mask %llx: direction bit (%d, %d)", name, (unsigned long long)mk, H.dfield, H.dbit);
        // the elements: the sum of the mask's terms on a column that carries the moved spin at j (up) or at i (down)
        double up[2] = {0, 0}, dn[2] = {0, 0};
        for (int64_t t = o.offs[m]; t < o.offs[m + 1]; ++t) {
          const uint64_t sg = (uint64_t)o.signs[t];
          const int im = pc(mk & sg) & 1;
          // (a composed hop moves both ways on a column with spin i down and spin L-1 up)
          up[im] += ((sg >> (pc(mk) == 2 ? j : i)) & 1) ? -o.coef[t] : o.coef[t];
          dn[im] += ((sg >> i) & 1) ? -o.coef[t] : o.coef[t];
        }
        EXPECT(H.up_re == up[0] && H.up_im == up[1] && H.dn_re == dn[0] && H.dn_im == dn[1],
               "%s: mask %llx: elements (%g %g %g %g)", name, (unsigned long long)mk, H.up_re, H.up_im, H.dn_re, H.dn_im);
      }
    EXPECT(found == 1 && part == want, "%s: mask %llx in %d records, part %d (spins %d %d want %d)", name,
           (unsigned long long)mk, found, part, i, j, want);
  }
  EXPECT(live == n[0] + n[1] + n[2] + n[3], "%s: %d live masks, %d hops", name, live, n[0] + n[1] + n[2] + n[3]);
}

// wnb, ptab: the rank of pattern ^ mask where the hop acts (the flip keeps the pattern's ones), the zero row / entry elsewhere
static void check_partner_tables(const char *name, const Sc3Mat &M) {
  const Sc3Tab &S = M.ly->host;
  const int a = S.a, w = S.w, nb = M.op.nldsB, nlds = M.op.nldsA;
  bool ok = M.wnb.size() == std::max<size_t>(1, M.ly->w_pat.size() * (size_t)nb);
  for (int cw = 0; ok && cw <= w; ++cw)
    for (int wr = 0; wr < S.nw[cw]; ++wr)
      for (int q = 0; q < nb; ++q) {
        const uint32_t v = M.ly->w_pat[S.w_off[cw] + wr], u = v ^ M.hops[nlds + M.op.ngatA + q].mW;
        ok = ok && M.wnb[(size_t)(S.w_off[cw] + wr) * nb + q] == (pc(u) == pc(v) ? rank_of(u) : S.nw[cw]);
      }
  EXPECT(ok, "%s: wnb", name);
  EXPECT(!M.ptab.empty() && M.op.nhp == ((nlds + 7) & ~7), "%s: no partner table of the lo pass (nhp %d)", name, M.op.nhp);
  if (M.ptab.empty()) return;
  const int esz = M.real ? 8 : 16, nhp = M.op.nhp;
  int row = 0;
  ok = true;
  for (int kl = 0; kl <= a; ++kl) {
    ok = ok && M.op.ptab_row[kl] == row;
    const int nrow = (S.nl[kl] + 2) & ~1;
    for (int r = 0; r < nrow; ++r)
      for (int q = 0; q < nhp; ++q) {
        int want = S.nl[kl] * esz;
        if (r < S.nl[kl] && q < nlds) {
          const uint32_t v = M.ly->lo_pat[S.lo_off[kl] + r], u = v ^ M.hops[q].mLo;
          if (pc(u) == pc(v)) want = rank_of(u) * esz;
        }
        ok = ok && M.ptab[(size_t)(row + r) * nhp + q] == want;
      }
    row += nrow;
  }
  ok = ok && M.ptab.size() == (size_t)row * nhp && (int)M.pcoef.size() == nhp;
  for (int q = 0; ok && q < nhp; ++q) ok = M.pcoef[q] == (q < nlds ? M.hops[q].up_re : 0.0);
  EXPECT(ok, "%s: ptab / pcoef", name);
}

// ---- the diagonal --------------------------------------------------------------------------------------------
static void check_diagonal(const char *name, const Sc3Mat &M, const Msc &o) {
  const Sc3Tab &S = M.ly->host;
  const int a = S.a, L = S.L, k = S.k;
  const uint64_t lom = (1ull << a) - 1;
  const bool has = !o.masks.empty() && o.masks[0] == 0;
  std::set<uint64_t> groups;
  for (int64_t t = 0; has && t < o.offs[1]; ++t)
    if (((uint64_t)o.signs[t] & ~lom) && ((uint64_t)o.signs[t] & lom)) groups.insert((uint64_t)o.signs[t] & lom);
  const int want_mode = !has ? 0 : (groups.size() > 4 ? 1 : 2);
  EXPECT(M.diag_mode == want_mode, "%s: diag_mode %d with %zu groups", name, M.diag_mode, groups.size());
  EXPECT(M.op.ndt == (M.diag_mode == 2 ? (int)M.dt_sign.size() : 0), "%s: ndt %d", name, M.op.ndt);
  if (M.diag_mode != 2) return;
  EXPECT(M.op.ngroups == (int)groups.size() && M.dlo.size() == M.ly->lo_pat.size() && M.dt_coef.size() == M.dt_sign.size() &&
             M.dt_group.size() == M.dt_sign.size(), "%s: sizes of the diagonal's tables", name);
  bool ok = true;
  for (uint64_t s = 0; s < (1ull << L); ++s) {
    if (pc(s) != k) continue;
    const uint32_t Lo = (uint32_t)(s & lom);
    double got = M.dlo[S.lo_off[pc(Lo)] + rank_of(Lo)], want = 0.0;
    for (size_t i = 0; i < M.dt_sign.size(); ++i) {
      const int g = M.dt_group[i];
      ok = ok && (int)(M.dt_sign[i] >> 61) == g && g <= M.op.ngroups;
      int par = pc((s >> a) & (M.dt_sign[i] & ((1ull << 61) - 1)));
      if (g) par += pc(Lo & M.op.glo[g - 1]);
      got += (par & 1) ? -M.dt_coef[i] : M.dt_coef[i];
    }
    for (int64_t t = 0; t < o.offs[1]; ++t) want += (pc(s & (uint64_t)o.signs[t]) & 1) ? -o.coef[t] : o.coef[t];
    ok = ok && got == want;
  }
  EXPECT(ok, "%s: dlo + dt terms against the diagonal term by term", name);
}

// ---- the dispatch orders -------------------------------------------------------------------------------------
static void check_dispatch(const char *name, const Sc3Mat &M) {
  const Sc3Tab &S = M.ly->host;
  const int a = S.a, w = S.w, k = S.k;
  const int nt = sc3_lo_threads(a), cap = M.real ? sc3_lo_cap_r(a, nt) : sc3_lo_cap(a, nt);
  const int threads = M.real ? sc3r_threads(nt) : nt, esz = M.real ? 8 : 16;
  std::map<uint32_t, int> seen;
  bool ok = M.permA.size() % 64 == 0;
  for (size_t g = 0; ok && g < M.permA.size() / 8; ++g) {
    const uint32_t *e = &M.permA[8 * g];
    if (e[0] == 0xffffffffu) {
      for (int j = 0; j < 8; ++j) ok = ok && e[j] == 0xffffffffu;
      continue;
    }
    const int m = (int)(e[0] >> 30);
    ok = ok && (threads >> m) >= 64;
    for (int j = 0; j < 8; ++j) {
      ok = ok && (int)(e[j] >> 30) == m;
      if (e[j] & SC3_NOROW) { ok = ok && (e[j] & ~(3u << 30)) == SC3_NOROW; continue; }
      const uint32_t id = e[j] & (SC3_NOROW - 1u);
      const int kl = k - pc(id >> w) - pc(id & ((1u << w) - 1u));
      ++seen[id];
      ok = ok && j < (1 << m) && kl >= 0 && kl <= a && S.nl[kl] <= (cap >> m);
      // the partner table's zero entry, right behind the row's entries, lies inside the row's slice of the tile
      if (!M.ptab.empty()) ok = ok && S.nl[kl] < (cap >> m) && M.ptab[(size_t)(M.op.ptab_row[kl] + S.nl[kl]) * M.op.nhp] == S.nl[kl] * esz;
    }
  }
  std::vector<uint32_t> rows;
  for (uint32_t b = M.T0; b < M.T1 && b < (uint32_t)M.ly->tseq.size(); ++b)
    for (uint32_t W = 0; W < (1u << w); ++W) {
      const int kl = k - pc(M.ly->tseq[b]) - pc(W);
      if (kl >= 0 && kl <= a) rows.push_back((M.ly->tseq[b] << w) | W);
    }
  ok = ok && seen.size() == rows.size();
  for (uint32_t r : rows) ok = ok && seen.count(r) && seen[r] == 1;
  EXPECT(ok, "%s: permA", name);
  EXPECT(M.rowsel == (rows.empty() ? std::vector<uint32_t>{0xffffffffu} : rows), "%s: rowsel", name);
  // window pass: every (T, cw, run) once
  std::map<uint32_t, int> runs;
  for (uint32_t e : M.permB) if (e != 0xffffffffu) ++runs[e];
  size_t want = 0;
  ok = M.permB.size() % 8 == 0;
  for (uint32_t b = M.T0; b < M.T1 && b < (uint32_t)M.ly->tseq.size(); ++b)
    for (int cw = 0; cw <= w; ++cw) {
      const uint32_t T = M.ly->tseq[b];
      const int kl = k - pc(T) - cw;
      if (kl < 0 || kl > a) continue;
      const int R = 16 << S.rs[cw], len = M.real ? S.pitch[kl] / 2 : S.pitch[kl];
      for (int run = 0; run * R < len; ++run, ++want) ok = ok && runs.count((T << 16) | (cw << 12) | run) && runs[(T << 16) | (cw << 12) | run] == 1;
    }
  EXPECT(ok && runs.size() == want, "%s: permB (%zu runs, %zu wanted)", name, runs.size(), want);
}

// ---- the blocks a rank reads ---------------------------------------------------------------------------------
static void check_window(const char *name, const Sc3Mat &M, const Msc &o) {
  const Sc3Layout &ly = *M.ly;
  const Sc3Tab &S = ly.host;
  const int a = S.a, w = S.w, L = S.L, k = S.k;
  bool ok = M.needT.size() == (size_t)1 << S.t;
  for (uint64_t s = 0; ok && s < (1ull << L); ++s) {
    if (pc(s) != k || !ly.in_range((uint32_t)(s >> (a + w)), M.T0, M.T1)) continue;
    for (int64_t m : o.masks)
      if (pc(s ^ (uint64_t)m) == k) ok = ok && M.needT[(s ^ (uint64_t)m) >> (a + w)];
  }
  EXPECT(ok, "%s: needT misses a block that a mask reaches", name);
  // the needed blocks as [start, end), their lengths summed from the rows
  std::vector<std::pair<int64_t, int64_t>> blk, merged;
  for (uint32_t T = 0; T < (uint32_t)M.needT.size(); ++T) {
    if (!M.needT[T] || ly.ibase[T] < 0) continue;
    int64_t len = 0;
    for (uint32_t W = 0; W < (1u << w); ++W) {
      const int kl = k - pc(T) - pc(W);
      if (kl >= 0 && kl <= a) len += S.pitch[kl];
    }
    blk.push_back({ly.ibase[T], ly.ibase[T] + len});
  }
  std::sort(blk.begin(), blk.end());
  for (auto &b : blk) {
    if (!merged.empty() && merged.back().second == b.first) merged.back().second = b.second;
    else merged.push_back(b);
  }
  EXPECT(M.ranges() == merged, "%s: ranges()", name);
  int64_t lo, hi;
  M.window(&lo, &hi);
  EXPECT(!merged.empty() && lo == merged.front().first && hi == merged.back().second - 1, "%s: window() [%lld, %lld]", name,
         (long long)lo, (long long)hi);
  const int shift = 5;
  const int64_t first = 1, n = (S.nint >> shift) + 1;      // (a map that starts one chunk in and ends past the layout)
  std::vector<uint8_t> map((size_t)n, 7);
  M.chunks(shift, first, n, map.data());
  ok = true;
  for (int64_t c = 0; c < n; ++c) {
    bool hit = false;
    for (auto &r : merged) hit = hit || (r.first < ((c + first + 1) << shift) && r.second > ((c + first) << shift));
    ok = ok && map[(size_t)c] == (hit ? 1 : 0);
  }
  EXPECT(ok, "%s: chunks()", name);
}

struct Case {
  const char *name;
  Msc op;
  int L, rank, nranks;
  bool xparity, real, graph, sym, tables;     // what the builder must decide; tables: the lo pass has its partner table
};

static int run(const Case &c) {
  const int k = 6, a = 6, w = 4, failed_before = failures;
  const Sc3Layout *ly = sc3_get(c.L, k, a, w, true, 0);
  DNM_CHECK(ly, "no layout");
  check_layout(c.name, *ly);
  std::vector<uint32_t> Tb = sc3_partition(*ly, c.nranks);
  EXPECT(Tb.size() == (size_t)c.nranks + 1 && Tb.front() == 0 && Tb.back() == ly->tseq.size() &&
             std::is_sorted(Tb.begin(), Tb.end()), "%s: sc3_partition", c.name);
  if (c.xparity) Tb = {0u, sc3_top_clear_blocks(*ly)};    // the blocks whose top bit is clear (dnm_mat_create)
  const std::vector<ScMask> scm = sc_masks(c.op.masks, c.op.offs, c.op.signs, c.op.coef, c.L, c.xparity);
  int npair2 = 0;
  for (const ScMask &e : scm) npair2 += e.pair == 2;
  EXPECT(npair2 == (c.xparity ? 2 : 0), "%s: %d composed hops", c.name, npair2);
  Sc3Mat M;
  DNM_TRY(M.init(ly, c.op.masks, c.op.offs, c.op.signs, c.op.coef, scm, true, Tb[c.rank], Tb[c.rank + 1], c.real));
  EXPECT(M.tiled && M.graph == c.graph && M.sym == c.sym && M.real == c.real, "%s: tiled %d graph %d sym %d", c.name,
         (int)M.tiled, (int)M.graph, (int)M.sym);
  if (!M.tiled) return 0;
  if (M.graph) {
    check_hops(c.name, M, c.op, c.xparity, !c.xparity);
    if (c.tables) check_partner_tables(c.name, M);
    else EXPECT(M.ptab.empty() && M.op.nhp == 0, "%s: a partner table without LDS hops of the lo pass", c.name);
  } else {
    bool ok = M.op.present == (1ull << (c.L - 1)) - 1 && M.op.bondsA == 1ull << (a - 1) && M.hops.empty() &&
              M.op.bondsB == (M.op.present & ~((1ull << (a + w - 1)) - 1)) && M.bond.size() == 4 * (size_t)(c.L - 1);
    for (int b = 0; ok && b < c.L - 1; ++b)
      ok = M.bond[4 * b] == 0.5 && M.bond[4 * b + 1] == 0.0 && M.bond[4 * b + 2] == 0.5 && M.bond[4 * b + 3] == 0.0;
    EXPECT(ok, "%s: the chain's bonds", c.name);
  }
  check_diagonal(c.name, M, c.op);
  check_dispatch(c.name, M);
  check_window(c.name, M, c.op);
  // upload(): every pointer the kernels are handed points at a copy of its table
  EXPECT(M.op.bond && !memcmp(M.op.bond, M.bond.data(), M.bond.size() * 8), "%s: op.bond", c.name);
  if (M.graph) EXPECT(M.op.gatB == M.op.ldsA + M.op.nldsA + M.op.ngatA + M.op.nldsB && M.op.wnb, "%s: op's hop pointers", c.name);
  EXPECT((M.diag_mode == 2) == (M.op.dlo != nullptr) && (M.op.ptab != nullptr) == !M.ptab.empty(), "%s: op.dlo / op.ptab", c.name);
  if (failures == failed_before) printf("%-24s L=%d rank %d/%d%s: ok\n", c.name, c.L, c.rank, c.nranks, c.real ? " real" : "");
  return 0;
}

// ---- block ranges as PLACES of the block sequence: layouts with empty blocks -----------------------------------
// SpinConserve(L, L/2) in the (6, 4) layout from L = 22 on: k > a + w, so the blocks T = 0 and T = all ones are empty and
// a place of the sequence is no value of T.  The half whose top bit is clear (XParity's vectors) ends at the place
// sc3_top_clear_blocks names, and it is half of both index spaces; in block order 1 a share's reference side is the runs
// of sc3_ref_runs: whole blocks, disjoint, all of the subspace over the ranks.
static int check_places(int L, int a, int w) {
  const int k = L / 2, failed_before = failures;
  char name[32];
  snprintf(name, sizeof name, "places(%d,%d)", L, k);
  const Sc3Layout *ly = sc3_get(L, k, a, w, false, 0);
  DNM_CHECK(ly, "no layout");
  const uint32_t t = (uint32_t)ly->host.t, top = 1u << (t - 1), nb = (uint32_t)ly->tseq.size();
  uint32_t full = 0, below = 0;            // the non-empty blocks (0 <= k - |T| <= a + w), counted
  for (uint32_t T = 0; T < (1u << t); ++T)
    if (k - pc(T) >= 0 && k - pc(T) <= a + w) { ++full; below += T < top; }
  EXPECT(nb == full && full < (1u << t) && below < top && ly->ibase[0] < 0 && ly->ibase[(1u << t) - 1] < 0, "%s: %u blocks",
         name, nb);
  const uint32_t b = sc3_top_clear_blocks(*ly);
  EXPECT(b == below && b == sc3_partition(*ly, 2)[1], "%s: the first half ends at place %u", name, b);
  bool ok = std::is_sorted(ly->tseq.begin(), ly->tseq.end());
  for (uint32_t j = 0; j < nb; ++j) ok = ok && (ly->tseq[j] < top) == (j < b) && ly->tidx[ly->tseq[j]] == j;
  EXPECT(ok, "%s: the blocks below place %u are not those whose top bit is clear", name, b);
  int64_t is, il, ns, nl;
  sc3_range(*ly, 0, b, &is, &il, &ns, &nl);
  EXPECT(is == 0 && ns == 0 && 2 * il == ly->host.nint && 2 * nl == ly->dim, "%s: first half [%lld + %lld), rows [%lld + %lld)",
         name, (long long)is, (long long)il, (long long)ns, (long long)nl);
  EXPECT(b < nb && ly->nbase[ly->tseq[b]] == ly->dim / 2 && 2 * ly->ibase[ly->tseq[b]] == ly->host.nint,
         "%s: the block at place %u starts at row %lld", name, b, (long long)ly->nbase[ly->tseq[b]]);
  const auto half = sc3_ref_runs(*ly, 0, b);
  EXPECT(half.size() == 1 && half[0].first == 0 && half[0].second == ly->dim / 2, "%s: sc3_ref_runs of the first half", name);
  // (what a value of T in place of the place would have taken: one block too many)
  sc3_range(*ly, 0, top, &is, &il, &ns, &nl);
  EXPECT(2 * nl > ly->dim && 2 * il > ly->host.nint, "%s: places [0, 2^(t-1)) hold %lld rows", name, (long long)nl);
  // block order 1, three ranks
  const Sc3Layout *l1 = sc3_get(L, k, a, w, false, 1);
  DNM_CHECK(l1, "no layout in block order 1");
  EXPECT(sc3_top_clear_blocks(*l1) == 0xffffffffu, "%s: a first half in block order 1", name);
  const std::vector<uint32_t> Tb = sc3_partition(*l1, 3);
  std::vector<std::pair<int64_t, int64_t>> all;
  for (int r = 0; r < 3; ++r) {
    const auto runs = sc3_ref_runs(*l1, Tb[r], Tb[r + 1]);
    sc3_range(*l1, Tb[r], Tb[r + 1], &is, &il, &ns, &nl);
    int64_t n = 0;
    ok = !runs.empty() && ns == (r == 0 ? 0 : -1);
    for (size_t i = 0; i < runs.size(); ++i) {
      n += runs[i].second;
      ok = ok && runs[i].first >= 0 && runs[i].second > 0 && runs[i].first + runs[i].second <= l1->dim;
      ok = ok && (i == 0 || runs[i - 1].first + runs[i - 1].second != runs[i].first);       // maximal
    }
    EXPECT(ok && n == nl, "%s: rank %d of 3: %zu runs of %lld rows, the share has %lld", name, r, runs.size(), (long long)n,
           (long long)nl);
    EXPECT(runs.size() > 1, "%s: rank %d of 3 is a range of the reference order in block order 1", name, r);
    all.insert(all.end(), runs.begin(), runs.end());
  }
  std::sort(all.begin(), all.end());
  int64_t end = 0;
  ok = true;
  for (const auto &r : all) { ok = ok && r.first == end; end = r.first + r.second; }
  EXPECT(ok && end == l1->dim, "%s: the shares' runs do not tile the reference order", name);
  const auto whole = sc3_ref_runs(*l1, 0, 0xffffffffu);
  int64_t n = 0;
  for (const auto &r : whole) n += r.second;
  EXPECT(n == l1->dim, "%s: the whole sequence has %lld rows", name, (long long)n);
  if (failures == failed_before) printf("%-24s blocks as places: ok\n", name);
  return 0;
}

int main() {
  for (int L : {22, 24})
    if (check_places(L, 6, 4)) {
      ++failures;
      printf("FAILED places(%d): %s\n", L, g_err);
    }
  const std::vector<Case> cases = {
      {"chain12", chain12(), 12, 0, 1, false, false, false, true, false},
      {"graph13", graph13(false), 13, 0, 1, false, false, true, true, true},
      {"graph13", graph13(false), 13, 0, 3, false, false, true, true, true},
      {"graph13", graph13(false), 13, 1, 3, false, false, true, true, true},
      {"graph13", graph13(false), 13, 2, 3, false, false, true, true, true},
      {"xparity12", xparity12(), 12, 0, 1, true, false, true, true, true},
      {"complex13", graph13(true), 13, 0, 1, false, false, true, false, true},
      {"manygroups12", manygroups12(), 12, 0, 1, false, false, false, true, false},
      {"chain12", chain12(), 12, 0, 1, false, true, false, true, false},
      {"graph13", graph13(false), 13, 0, 1, false, true, true, true, true},
      {"xparity12", xparity12(), 12, 0, 1, true, true, true, true, true},
  };
  for (const Case &c : cases)
    if (run(c)) {
      ++failures;
      printf("FAILED %s: %s\n", c.name, g_err);
    }
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
