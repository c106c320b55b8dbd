// Host tables of the SpinConserve internal layout (sc3.h) and of an operator's two tiled passes: everything that
// sc3_kernels.hip / sc3g_kernels.hip read and that calls no HIP function.  Sc3Layout::init and Sc3Mat::init fill host
// members step by step; their upload() (the end of this file) is the only code that touches DevBuf.  Plain C++:
// tests/sc3_tables_check.cpp links this file alone and checks every table against its definition.
#include "sc3.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

#include "dnm_common.h"
#include "sc3_shape.h"

namespace dnm {

// ---- the operator as pair hops ----
std::vector<ScMask> sc_masks(const std::vector<int64_t> &masks, const std::vector<int64_t> &mask_offsets,
                             const std::vector<int64_t> &signs, const std::vector<double> &rcoef, int L, bool xparity) {
  std::vector<ScMask> scm(masks.size());
  for (size_t mi = 0; mi < masks.size(); ++mi) {
    ScMask &e = scm[mi];
    memset(&e, 0, sizeof(e));
    const uint64_t mask = (uint64_t)masks[mi];
    e.dead = __builtin_popcountll(mask) & 1;
    if (xparity && L >= 3 && __builtin_popcountll(mask) == L - 2 && !((mask >> (L - 1)) & 1ull)) {
      // a hop between spin i and spin L-1 times the global flip (XParity.reduce_msc): every spin but those two
      const uint64_t miss = ~mask & ((((uint64_t)1 << (L - 1)) - 1));
      const int i = __builtin_ctzll(miss);
      const uint64_t pairbits = ((uint64_t)1 << i) | ((uint64_t)1 << (L - 1));
      bool local = true;
      for (int64_t t = mask_offsets[mi]; t < mask_offsets[mi + 1]; ++t)
        if ((uint64_t)signs[t] & ~pairbits) local = false;
      if (!local) continue;
      e.pair = 2;
      e.lo = i;
      e.hi = L - 1;
      for (int64_t t = mask_offsets[mi]; t < mask_offsets[mi + 1]; ++t) {
        // the column state keeps spin i down and spin L-1 up; the sign masks do not meet the mask: a real element
        const double c = (((uint64_t)signs[t] >> i) & 1) ? -rcoef[t] : rcoef[t];
        e.up_re += c;
        e.dn_re += c;
      }
      continue;
    }
    if (__builtin_popcountll(mask) != 2) continue;
    const int lo = __builtin_ctzll(mask), hi = 63 - __builtin_clzll(mask);
    bool local = true;
    for (int64_t t = mask_offsets[mi]; t < mask_offsets[mi + 1]; ++t)
      if ((uint64_t)signs[t] & ~mask) local = false;
    if (!local) continue;
    e.pair = 1;
    e.fast = hi == lo + 1;
    e.lo = lo;
    e.hi = hi;
    for (int64_t t = mask_offsets[mi]; t < mask_offsets[mi + 1]; ++t) {
      const uint64_t sg = (uint64_t)signs[t];
      const double rc = rcoef[t];
      const bool imag = parity64(mask & sg);
      // column state (bra) carries the moved spin: bit hi for an up hop, bit lo for a down hop
      const double up = ((sg >> hi) & 1) ? -rc : rc;
      const double dn = ((sg >> lo) & 1) ? -rc : rc;
      (imag ? e.up_im : e.up_re) += up;
      (imag ? e.dn_im : e.dn_re) += dn;
    }
  }
  return scm;
}

static int64_t hbinom(int n, int k) {
  if (k < 0 || k > n) return 0;
  long double r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return (int64_t)llroundl(r);
}

bool sc3_valid(int L, int k, int a, int w) {
  const int t = L - a - w;
  return a >= 2 && a <= SC3_MAXA && w >= 2 && w <= SC3_MAXW && t >= 1 && t <= 15 && k >= 0 && k <= L;
}

int Sc3Layout::init(int L, int k, int a, int w, bool want_device, int order_) {
  DNM_CHECK(sc3_valid(L, k, a, w), "no such vector layout: L=%d k=%d a=%d w=%d", L, k, a, w);
  DNM_CHECK(order_ == 0 || order_ == 1, "unknown block order %d of a SpinConserve layout", order_);
  order = order_;
  host = Sc3Tab{};
  host.L = L; host.k = k; host.a = a; host.w = w; host.t = L - a - w;
  build_patterns();
  build_window_partners();
  DNM_TRY(build_split_rank());
  DNM_TRY(build_offsets());
  point_tables();
  return want_device ? upload() : 0;
}

void Sc3Layout::build_patterns() {
  Sc3Tab &S = host;
  const int L = S.L, k = S.k, a = S.a, w = S.w;
  cbin.assign(17 * 17, 0);
  for (int n = 0; n < 17; ++n) for (int j = 0; j < 17; ++j) cbin[n * 17 + j] = (int32_t)hbinom(n, j);
  nck.assign((size_t)(k + 1) * (L + 1), 0);
  for (int kk = 0; kk <= k; ++kk) for (int LL = 0; LL <= L; ++LL) nck[(size_t)kk * (L + 1) + LL] = hbinom(LL, kk);
  lo_rank.assign((size_t)1 << a, 0);
  w_rank.assign((size_t)1 << w, 0);
  lo_pat.clear();
  w_pat.clear();
  for (int j = 0; j <= a; ++j) {
    S.lo_off[j] = (int32_t)lo_pat.size();
    S.nl[j] = (int32_t)hbinom(a, j);
    S.pitch[j] = (S.nl[j] + 7) / 8 * 8;
    int r = 0;
    for (uint32_t v = 0; v < (1u << a); ++v)
      if (__builtin_popcount(v) == j) { lo_rank[v] = (uint16_t)r++; lo_pat.push_back((uint16_t)v); }
  }
  S.lo_off[a + 1] = (int32_t)lo_pat.size();
  const int wmax = (int)hbinom(w, w / 2);
  for (int j = 0; j <= w; ++j) {
    S.w_off[j] = (int32_t)w_pat.size();
    S.nw[j] = (int32_t)hbinom(w, j);
    int r = 0;
    for (uint32_t v = 0; v < (1u << w); ++v)
      if (__builtin_popcount(v) == j) { w_rank[v] = (uint16_t)r++; w_pat.push_back((uint16_t)v); }
    int s = 0;
    while ((S.nw[j] << (s + 1)) <= wmax && s < 8) ++s;      // R = 16 << s keeps nw * R within the largest tile
    S.rs[j] = s;
  }
  S.w_off[w + 1] = (int32_t)w_pat.size();
}

// partner table of the window pass's LDS bonds (Sc3Tab::w_nb)
void Sc3Layout::build_window_partners() {
  const Sc3Tab &S = host;
  const int w = S.w;
  // (only the field splits that have kernel instances need them; wider ones keep the tables empty)
  const bool nbfit = w - 1 <= 16 && hbinom(w, w / 2) < 255;
  w_nb.assign(nbfit ? (size_t)2 * w_pat.size() : 0, 0);
  for (int j = 0; nbfit && j <= w; ++j)
    for (int r = 0; r < S.nw[j]; ++r) {
      const uint32_t v = w_pat[S.w_off[j] + r];
      for (int b = 0; b < 16; ++b) {
        uint64_t f = (uint64_t)S.nw[j];                        // the zero row
        if (b < w - 1) {
          const uint32_t pair = (v >> b) & 3u;
          if (pair == 1u || pair == 2u) f = w_rank[v ^ (3u << b)];
        }
        w_nb[(size_t)2 * (S.w_off[j] + r) + (size_t)(b / 8)] |= f << (8 * (b % 8));
      }
    }
}

// lo_rank in two halves (Sc3Tab::lo_rlo / lo_rhi): colex rank = sum over the ones, m-th one at position q: C(q, m)
int Sc3Layout::build_split_rank() {
  const int a = host.a;
  const int h = a / 2, hb = a - h;
  lo_rlo.assign((size_t)1 << h, 0);
  lo_rhi.assign(((size_t)1 << hb) * (h + 1), 0);
  for (uint32_t v = 0; v < (1u << h); ++v) {
    int64_t r = 0;
    int m = 0;
    for (int q = 0; q < h; ++q) if ((v >> q) & 1u) r += hbinom(q, ++m);
    lo_rlo[v] = (uint16_t)r;
  }
  for (uint32_t v = 0; v < (1u << hb); ++v)
    for (int cl = 0; cl <= h; ++cl) {
      int64_t r = 0;
      int m = cl;
      for (int q = 0; q < hb; ++q) if ((v >> q) & 1u) r += hbinom(h + q, ++m);
      lo_rhi[(size_t)v * (h + 1) + cl] = (uint16_t)r;
    }
  for (uint32_t v = 0; v < (1u << a); ++v) {
    const uint32_t lo = v & ((1u << h) - 1u);
    DNM_CHECK(lo_rank[v] == lo_rlo[lo] + lo_rhi[(size_t)(v >> h) * (h + 1) + __builtin_popcount(lo)],
              "internal: split rank table of pattern %u", v);
  }
  return 0;
}

// offsets inside a block by the ones it has left, then the blocks in the order they lie in with their rows
int Sc3Layout::build_offsets() {
  Sc3Tab &S = host;
  const int L = S.L, k = S.k, a = S.a, w = S.w, t = S.t;
  icoff.assign((size_t)(a + w + 1) * (w + 1), 0);
  ncoff.assign((size_t)(a + w + 1) << w, 0);
  std::vector<int64_t> isize(a + w + 1, 0);
  for (int kr = 0; kr <= a + w; ++kr) {
    int64_t o = 0;
    for (int cw = 0; cw <= w; ++cw) {
      icoff[(size_t)kr * (w + 1) + cw] = o;
      const int kl = kr - cw;
      if (kl >= 0 && kl <= a) o += hbinom(w, cw) * S.pitch[kl];
    }
    isize[kr] = o;
    int64_t no = 0;
    for (uint32_t W = 0; W < (1u << w); ++W) {
      ncoff[((size_t)kr << w) + W] = no;
      const int kl = kr - __builtin_popcount(W);
      if (kl >= 0 && kl <= a) no += hbinom(a, kl);
    }
  }
  ibase.assign((size_t)1 << t, -1);
  nbase.assign((size_t)1 << t, -1);
  rows.clear();
  int64_t ni = 0, nn = 0;
  // reference indices: ascending T
  tseq.clear();
  for (uint32_t T = 0; T < (1u << t); ++T) {
    const int kr = k - __builtin_popcount(T);
    if (kr < 0 || kr > a + w) continue;
    nbase[T] = nn;
    nn += hbinom(a + w, kr);
    tseq.push_back(T);
  }
  // the order the blocks lie in (sc3_code_order)
  if (order == 1) {
    // by (ones of T above its lowest bit, ones of T's upper half, T >> 1, T & 1): the two blocks that differ in T's lowest
    // bit -- partners under the W/T boundary bond -- lie side by side, the bonds inside T >> 1 keep the first key, and of
    // a chain's bonds only the one between T's two lowest bits changes it (sc3.h: sc3_code_order)
    const int th = t / 2;
    std::stable_sort(tseq.begin(), tseq.end(), [th](uint32_t x, uint32_t y) {
      const int px = __builtin_popcount(x >> 1), py = __builtin_popcount(y >> 1);
      if (px != py) return px < py;
      const int hx = __builtin_popcount(x >> th), hy = __builtin_popcount(y >> th);
      if (hx != hy) return hx < hy;
      return x < y;                    // (T >> 1, then T & 1)
    });
  }
  tidx.assign((size_t)1 << t, 0xffffffffu);
  rowstart.assign(tseq.size() + 1, 0);
  for (size_t b = 0; b < tseq.size(); ++b) {
    const uint32_t T = tseq[b];
    const int kr = k - __builtin_popcount(T);
    tidx[T] = (uint32_t)b;
    ibase[T] = ni;
    ni += isize[kr];
    rowstart[b] = rows.size();
    for (uint32_t W = 0; W < (1u << w); ++W) {
      const int kl = kr - __builtin_popcount(W);
      if (kl >= 0 && kl <= a) rows.push_back((T << w) | W);
    }
  }
  rowstart[tseq.size()] = rows.size();
  S.nint = ni;
  dim = nn;
  DNM_CHECK(nn == hbinom(L, k), "internal: layout does not cover the subspace");
  return 0;
}

void Sc3Layout::point_tables() {
  Sc3Tab &S = host;
  const int a = S.a;
  S.ibase = ibase.data(); S.nbase = nbase.data(); S.icoff = icoff.data(); S.ncoff = ncoff.data();
  S.lo_pat = lo_pat.data(); S.w_pat = w_pat.data(); S.lo_rank = lo_rank.data(); S.w_rank = w_rank.data();
  S.cbin = cbin.data();
  S.nck = nck.data();
  S.w_nb = w_nb.data();
  S.lo_rlo = lo_rlo.data();
  S.lo_rhi = lo_rhi.data();
  dev = S;
  // halved positions (real vectors read as pairs of entries): everything is a multiple of 8 entries
  ibase_h.assign(ibase.size(), -1);
  for (size_t i = 0; i < ibase.size(); ++i) if (ibase[i] >= 0) ibase_h[i] = ibase[i] / 2;
  icoff_h.assign(icoff.size(), 0);
  for (size_t i = 0; i < icoff.size(); ++i) icoff_h[i] = icoff[i] / 2;
  host_h = S;
  host_h.ibase = ibase_h.data();
  host_h.icoff = icoff_h.data();
  host_h.nint = S.nint / 2;
  for (int j = 0; j <= a; ++j) host_h.pitch[j] = S.pitch[j] / 2;
}

const Sc3Layout *sc3_get(int L, int k, int a, int w, bool want_device, int order) {
  static std::mutex mu;
  static std::map<std::array<int, 6>, std::unique_ptr<Sc3Layout>> cache;
  std::lock_guard<std::mutex> g(mu);
  const std::array<int, 6> key{L, k, a, w, want_device ? 1 : 0, order};
  auto it = cache.find(key);
  if (it != cache.end()) return it->second.get();
  std::unique_ptr<Sc3Layout> lay(new Sc3Layout());
  if (lay->init(L, k, a, w, want_device, order)) return nullptr;
  return (cache[key] = std::move(lay)).get();
}

bool sc3_perm_make(const int8_t *site_perm, int L, Sc3Perm *out) {
  *out = Sc3Perm{};
  out->L = L;
  for (int i = 0; i < 64; ++i) out->to_int[i] = out->to_ref[i] = (uint8_t)i;
  if (!site_perm) return true;
  uint64_t seen = 0;
  for (int i = 0; i < L; ++i) {
    const int b = site_perm[i];
    if (b < 0 || b >= L || ((seen >> b) & 1ull)) return false;
    seen |= 1ull << b;
    out->to_int[i] = (uint8_t)b;
    out->to_ref[b] = (uint8_t)i;
    if (b != i) out->on = 1;
  }
  return true;
}

// ---- the operator ---------------------------------------------------------------------------------------
// deal groups of workgroups to the 8 XCDs (workgroup b runs on XCD b % 8): the next group goes to the shortest stream
static std::vector<uint32_t> deal(const std::vector<std::vector<uint32_t>> &groups) {
  std::vector<std::vector<uint32_t>> st(8);
  for (auto &g : groups) {
    int best = 0;
    for (int s = 1; s < 8; ++s) if (st[s].size() < st[best].size()) best = s;
    st[best].insert(st[best].end(), g.begin(), g.end());
  }
  size_t n = 0;
  for (auto &s : st) n = std::max(n, s.size());
  std::vector<uint32_t> out(8 * n, 0xffffffffu);
  for (int s = 0; s < 8; ++s)
    for (size_t i = 0; i < st[s].size(); ++i) out[8 * i + s] = st[s][i];
  return out;
}

// lo pass: rows -> workgroups.  `order` is the dispatch order of the rows (8 interleaved XCD streams, 0xffffffff =
// padding); inside a stream rows are packed, in that order, 2^m to a workgroup where 2^m rows of their length fit the
// entries a workgroup's threads hold (sc3_shape.h: Sc3LoShape; sub-groups of whole wavefronts, m <= 3).  Rows that follow each other in
// a stream are the same (cw, wr) over the T's of a popcount class, so a workgroup's rows have equal lengths and its
// place in the stream stays next to the boundary-bond partners of its rows.  Returns 8 entries per workgroup, the
// workgroups of the streams interleaved again.
static std::vector<uint32_t> pack_lo_rows(const std::vector<uint32_t> &order, const Sc3Layout &ly, const Sc3LoShape &shape) {
  const Sc3Tab &S = ly.host;
  auto logm_of = [&](uint32_t e) {
    const uint32_t T = e >> S.w, W = e & ((1u << S.w) - 1u);
    return shape.rows_log2(S.nl[S.k - __builtin_popcount(T) - __builtin_popcount(W)]);
  };
  std::vector<std::vector<uint32_t>> wgs(8);        // per stream: 8 entries per workgroup
  for (int s = 0; s < 8; ++s) {
    std::vector<uint32_t> open[4];                  // rows waiting for their workgroup to fill, by m
    auto flush = [&](int m) {
      if (open[m].empty()) return;
      for (int j = 0; j < 8; ++j)
        wgs[s].push_back(j < (int)open[m].size() ? (open[m][j] | ((uint32_t)m << 30)) : (SC3_NOROW | ((uint32_t)m << 30)));
      open[m].clear();
    };
    for (size_t i = s; i < order.size(); i += 8) {
      const uint32_t e = order[i];
      if (e == 0xffffffffu) continue;
      const int m = logm_of(e);
      open[m].push_back(e);
      if ((int)open[m].size() == (1 << m)) flush(m);
    }
    for (int m = 0; m < 4; ++m) flush(m);
  }
  size_t n = 0;
  for (auto &v : wgs) n = std::max(n, v.size() / 8);
  std::vector<uint32_t> out(8 * 8 * n, 0xffffffffu);
  for (int s = 0; s < 8; ++s)
    for (size_t i = 0; i < wgs[s].size() / 8; ++i)
      for (int j = 0; j < 8; ++j) out[8 * (8 * i + s) + j] = wgs[s][8 * i + j];
  return out;
}

bool sc3_instance(int a, int w) { return (a == 14 && w == 10) || (a == 6 && w == 4); }

static int64_t block_len(const Sc3Layout &ly, uint32_t T) {        // internal length of the T block
  if (ly.ibase[T] < 0) return 0;
  const uint32_t b = ly.tidx[T];                                     // (the next block of the layout's sequence, whatever its order)
  return (b + 1 < (uint32_t)ly.tseq.size() ? ly.ibase[ly.tseq[b + 1]] : ly.host.nint) - ly.ibase[T];
}

std::vector<uint32_t> sc3_partition(const Sc3Layout &ly, int nranks) {
  const uint32_t nb = (uint32_t)ly.tseq.size();
  std::vector<uint32_t> Tb((size_t)nranks + 1, nb);
  Tb[0] = 0;
  uint32_t b = 0;
  for (int r = 1; r < nranks; ++r) {
    const int64_t target = (int64_t)((__int128)ly.host.nint * r / nranks);
    while (b < nb && ly.ibase[ly.tseq[b]] < target) ++b;
    Tb[r] = b;
  }
  return Tb;
}

void sc3_range(const Sc3Layout &ly, uint32_t T0, uint32_t T1, int64_t *istart, int64_t *ilen, int64_t *nstart, int64_t *nlen) {
  const uint32_t nb = (uint32_t)ly.tseq.size();
  const uint32_t b0 = std::min(T0, nb), b1 = std::max(b0, std::min(T1, nb));
  const int64_t i0 = b0 < nb ? ly.ibase[ly.tseq[b0]] : ly.host.nint, i1 = b1 < nb ? ly.ibase[ly.tseq[b1]] : ly.host.nint;
  *istart = i0;
  *ilen = i1 - i0;
  if (ly.order == 0) {
    const int64_t n0 = b0 < nb ? ly.nbase[ly.tseq[b0]] : ly.dim, n1 = b1 < nb ? ly.nbase[ly.tseq[b1]] : ly.dim;
    *nstart = n0;
    *nlen = n1 - n0;
    return;
  }
  // any other block order: the states of the range (its reference side is a range only for the whole sequence)
  int64_t n = 0;
  const int aw = ly.host.a + ly.host.w;
  for (uint32_t b = b0; b < b1; ++b) n += hbinom(aw, ly.host.k - __builtin_popcount(ly.tseq[b]));
  *nstart = b0 == 0 ? 0 : -1;
  *nlen = n;
}

std::vector<std::pair<int64_t, int64_t>> sc3_ref_runs(const Sc3Layout &ly, uint32_t T0, uint32_t T1) {
  const uint32_t nb = (uint32_t)ly.tseq.size();
  const uint32_t b0 = std::min(T0, nb), b1 = std::max(b0, std::min(T1, nb));
  const int aw = ly.host.a + ly.host.w;
  std::vector<std::pair<int64_t, int64_t>> out;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t T = ly.tseq[b];
    const int64_t n0 = ly.nbase[T], cnt = hbinom(aw, ly.host.k - __builtin_popcount(T));
    if (!out.empty() && out.back().first + out.back().second == n0) out.back().second += cnt;
    else out.push_back({n0, cnt});
  }
  return out;
}

uint32_t sc3_top_clear_blocks(const Sc3Layout &ly) {
  if (ly.order != 0) return 0xffffffffu;
  const uint32_t top = 1u << (ly.host.t - 1);
  return (uint32_t)(std::lower_bound(ly.tseq.begin(), ly.tseq.end(), top) - ly.tseq.begin());
}

void Sc3Mat::window(int64_t *lo, int64_t *hi) const {
  int64_t a = INT64_MAX, b = INT64_MIN;
  for (uint32_t T = 0; T < (uint32_t)needT.size(); ++T)
    if (needT[T] && ly->ibase[T] >= 0) {
      a = std::min(a, ly->ibase[T]);
      b = std::max(b, ly->ibase[T] + block_len(*ly, T) - 1);
    }
  if (b < a) a = b = row0;
  *lo = a;
  *hi = b;
}

// the needed blocks as maximal runs of positions [lo, hi), ascending
std::vector<std::pair<int64_t, int64_t>> Sc3Mat::ranges() const {
  std::vector<std::pair<int64_t, int64_t>> blk;
  for (uint32_t T = 0; T < (uint32_t)needT.size(); ++T)
    if (needT[T] && ly->ibase[T] >= 0) blk.push_back({ly->ibase[T], ly->ibase[T] + block_len(*ly, T)});
  std::sort(blk.begin(), blk.end());
  std::vector<std::pair<int64_t, int64_t>> out;
  for (const auto &b : blk) {
    if (!out.empty() && out.back().second == b.first) out.back().second = b.second;
    else out.push_back(b);
  }
  return out;
}

void Sc3Mat::chunks(int shift, int64_t first_chunk, int64_t nchunks, uint8_t *map) const {
  for (int64_t c = 0; c < nchunks; ++c) map[c] = 0;
  for (uint32_t T = 0; T < (uint32_t)needT.size(); ++T)
    if (needT[T] && ly->ibase[T] >= 0) {
      const int64_t c0 = (ly->ibase[T] >> shift) - first_chunk, c1 = ((ly->ibase[T] + block_len(*ly, T) - 1) >> shift) - first_chunk;
      for (int64_t c = std::max<int64_t>(c0, 0); c <= c1 && c < nchunks; ++c) map[c] = 1;
    }
}

int Sc3Mat::init(const Sc3Layout *layout, const std::vector<int64_t> &masks, const std::vector<int64_t> &mask_offsets,
                 const std::vector<int64_t> &signs, const std::vector<double> &rcoef, const std::vector<ScMask> &scm,
                 bool want_device, uint32_t T0_, uint32_t T1_, bool real_vectors) {
  ly = layout;
  real = real_vectors;
  T0 = T0_;
  T1 = T1_;
  {
    int64_t il, ns, nl;
    sc3_range(*ly, T0, T1, &row0, &il, &ns, &nl);
  }
  need_blocks(masks);
  classify(masks, scm);
  if (tiled) chain_bonds(masks, scm);
  if (graph && !graph_hops(masks, scm)) tiled = graph = false;     // more hops than a pass has room for: the row kernel
  if (tiled) {
    lo_partner_table();
    split_diagonal(masks, mask_offsets, signs, rcoef);
    lo_dispatch();
    DNM_TRY(window_dispatch());
  }
  return want_device ? upload() : 0;
}

// the rank's rows and the T blocks they read: their own and, for every mask that flips bits of T, the partner's
void Sc3Mat::need_blocks(const std::vector<int64_t> &masks) {
  const Sc3Tab &S = ly->host;
  const int a = S.a, w = S.w, t = S.t;
  const int64_t nmasks = (int64_t)masks.size();
  rowsel.clear();
  {
    const uint32_t nb = (uint32_t)ly->tseq.size();
    const uint32_t b0 = std::min(T0, nb), b1 = std::max(b0, std::min(T1, nb));
    rowsel.assign(ly->rows.begin() + (ptrdiff_t)ly->rowstart[b0], ly->rows.begin() + (ptrdiff_t)ly->rowstart[b1]);
  }
  if (rowsel.empty()) rowsel.push_back(0xffffffffu);
  needT.assign((size_t)1 << t, 0);
  for (uint32_t bq = T0; bq < T1 && bq < (uint32_t)ly->tseq.size(); ++bq) {
    const uint32_t T = ly->tseq[bq];
    needT[T] = 1;
    for (int64_t m = 0; m < nmasks; ++m) {
      const uint64_t hm = (uint64_t)masks[m] >> (a + w);
      const uint32_t U = T ^ (uint32_t)hm;
      if (!hm || U >= (1u << t) || ly->ibase[U] < 0) continue;     // (a mask that leaves T alone reads T itself)
      // a mask that flips bits of T only keeps the state in the subspace only if it keeps T's popcount
      const bool inside_T = ((uint64_t)masks[m] & (((uint64_t)1 << (a + w)) - 1)) == 0;
      if (inside_T && __builtin_popcount(U) != __builtin_popcount(T)) continue;
      needT[U] = 1;
    }
  }
}

void Sc3Mat::classify(const std::vector<int64_t> &masks, const std::vector<ScMask> &scm) {
  const int a = ly->host.a, w = ly->host.w;
  const int64_t nmasks = (int64_t)masks.size();
  // Two tiled passes need every off-diagonal mask to be a pair hop with signs inside the pair (ScMask::pair); masks
  // that never keep a state in the subspace (an odd number of flips: the fields of the harness's long-range model)
  // are skipped.  Chains of adjacent spins take the kernels of sc3_kernels.hip, any other bond graph those of
  // sc3g_kernels.hip (DNM_SC3_GRAPH=1: chains as well, for A/B runs).
  bool chain = sc3_instance(a, w), pairs = sc3_instance(a, w);
  for (int64_t m = 0; m < nmasks; ++m) {
    if (masks[m] == 0 || scm[m].dead) continue;
    if (!scm[m].fast) chain = false;
    if (!scm[m].pair) pairs = false;
  }
  if (const char *e = knob("DNM_SC3_GRAPH")) if (e[0] == '1') chain = false;
  tiled = chain || pairs;
  graph = tiled && !chain;
}

// the chain's bond elements (a bond graph: only whether every element is real and direction-independent)
void Sc3Mat::chain_bonds(const std::vector<int64_t> &masks, const std::vector<ScMask> &scm) {
  const int L = ly->host.L, a = ly->host.a, w = ly->host.w;
  const int64_t nmasks = (int64_t)masks.size();
  bond.assign(4 * (size_t)std::max(1, L - 1), 0.0);
  op.present = 0;
  sym = true;
  for (int64_t m = 0; m < nmasks; ++m) {
    if (masks[m] == 0 || scm[m].dead) continue;
    if (scm[m].up_im != 0.0 || scm[m].dn_im != 0.0 || scm[m].up_re != scm[m].dn_re) sym = false;
    if (graph) continue;
    const int b = scm[m].lo;
    bond[4 * b] = scm[m].up_re; bond[4 * b + 1] = scm[m].up_im;
    bond[4 * b + 2] = scm[m].dn_re; bond[4 * b + 3] = scm[m].dn_im;
    op.present |= 1ull << b;
  }
  // which pass gathers which bond outside its LDS tile: the Lo/W boundary in the lo pass, the W/T boundary and the
  // bonds inside T in the window pass (measured, profiles/r03_exp3_sc3_v2.txt)
  op.bondsA = op.present & (1ull << (a - 1));
  op.bondsB = 0;
  for (int b = a + w - 1; b < L - 1; ++b) op.bondsB |= op.present & (1ull << b);
}

// any bond graph: the hops by pass and by the way they are applied, and the partner rows of the window pass's LDS hops
bool Sc3Mat::graph_hops(const std::vector<int64_t> &masks, const std::vector<ScMask> &scm) {
  const Sc3Tab &S = ly->host;
  const int a = S.a, w = S.w;
  const int64_t nmasks = (int64_t)masks.size();
  hops.clear();
  wnb.clear();
  size_t nh[4] = {0, 0, 0, 0};
  {
    std::vector<Sc3Hop> part[4];       // lds A, gathered A, lds B, gathered B
    auto field = [&](int b) { return b < a ? 0 : (b < a + w ? 1 : 2); };
    auto fstart = [&](int f) { return f == 0 ? 0 : (f == 1 ? a : a + w); };
    for (int64_t m = 0; m < nmasks; ++m) {
      if (masks[m] == 0 || scm[m].dead) continue;
      const uint64_t mk = (uint64_t)masks[m];
      Sc3Hop h{};
      h.mLo = (uint32_t)(mk & (((uint64_t)1 << a) - 1));
      h.mW = (uint32_t)((mk >> a) & (((uint64_t)1 << w) - 1));
      h.mT = (uint32_t)(mk >> (a + w));
      h.half = __builtin_popcountll(mk) / 2;
      const int fi = field(scm[m].lo), fj = field(scm[m].hi);
      h.dfield = scm[m].pair == 2 ? 3 : fi;      // (the flip-composed hops of XParity act one way only)
      h.dbit = scm[m].lo - fstart(fi);
      h.up_re = scm[m].up_re; h.up_im = scm[m].up_im; h.dn_re = scm[m].dn_re; h.dn_im = scm[m].dn_im;
      part[fi == 0 ? (fj == 0 ? 0 : 1) : (fi == 1 && fj == 1 ? 2 : 3)].push_back(h);
    }
    // probes (timing only, WRONG results): keep the first n hops of a kind -- what a pass would take without the others
    // bounds what any reworking of them can gain (tools/probes/sc3g_drop_hops.sh)
    for (int q = 0; q < 4; ++q) {
      static const char *names[4] = {"DNM_SC3G_KEEP_LDSA", "DNM_SC3G_KEEP_GATA", "DNM_SC3G_KEEP_LDSB", "DNM_SC3G_KEEP_GATB"};
      if (const char *e = knob(names[q]))
        if ((size_t)atoi(e) < part[q].size()) part[q].resize((size_t)atoi(e));
    }
    if ((int)part[1].size() > SC3G_MAX_GATHER || (int)part[3].size() > SC3G_MAX_GATHER ||
        (int)part[2].size() > SC3G_MAX_WLDS)        // more hops than a pass has lanes / table columns for
      return false;
    for (int q = 0; q < 4; ++q) {
      nh[q] = part[q].size();
      hops.insert(hops.end(), part[q].begin(), part[q].end());
    }
    if (hops.empty()) hops.push_back(Sc3Hop{});
    // partner rows of the window pass's LDS hops
    const size_t nb = nh[2];
    wnb.assign(std::max<size_t>(1, ly->w_pat.size() * nb), 0);
    for (int cw = 0; cw <= w; ++cw)
      for (int wr = 0; wr < S.nw[cw]; ++wr) {
        const uint32_t v = ly->w_pat[S.w_off[cw] + wr];
        for (size_t q = 0; q < nb; ++q) {
          const uint32_t mw = part[2][q].mW;
          wnb[(size_t)(S.w_off[cw] + wr) * nb + q] =
              (uint8_t)(__builtin_popcount(v & mw) == part[2][q].half ? ly->w_rank[v ^ mw] : S.nw[cw]);
        }
      }
  }
  op.nldsA = (int32_t)nh[0]; op.ngatA = (int32_t)nh[1]; op.nldsB = (int32_t)nh[2]; op.ngatB = (int32_t)nh[3];
  return true;
}

// partner table of the lo pass's LDS hops (Sc3Op::ptab).  Needs the zero entry behind a row's entries inside the
// row's share of the tile under the rows-per-workgroup rule that lo_dispatch packs by (sc3_shape.h): true for every
// class of the instances (C(a, kl) is no power of two above 1).
void Sc3Mat::lo_partner_table() {
  const Sc3Tab &S = ly->host;
  const int a = S.a;
  const size_t nlds = (size_t)op.nldsA;               // (the LDS hops of the lo pass come first in hops)
  ptab.clear();
  op.ptab = nullptr;
  op.nhp = 0;
  {
    const char *pe = knob("DNM_SC3G_PTAB");
    const Sc3LoShape shape = sc3_lo_shape(a, real);
    bool ok = graph && nlds > 0 && (int)nlds <= SC3G_MAX_PTAB && !(pe && pe[0] == '0');
    for (int kl = 0; kl <= a && ok; ++kl)
      if (S.nl[kl] >= (shape.cap >> shape.rows_log2(S.nl[kl])) || (S.nl[kl] + 1) * (real ? 8 : 16) > 0xffff) ok = false;
    if (ok) {
      const int nhp = ((int)nlds + 7) & ~7, esz = real ? 8 : 16;
      int row = 0;
      for (int kl = 0; kl <= a; ++kl) {
        op.ptab_row[kl] = row;
        row += (S.nl[kl] + 2) & ~1;
      }
      ptab.assign((size_t)row * nhp, 0);
      for (int kl = 0; kl <= a; ++kl) {
        const uint16_t zero = (uint16_t)(S.nl[kl] * esz);
        const int nrow = (S.nl[kl] + 2) & ~1;
        for (int r = 0; r < nrow; ++r) {
          uint16_t *t = ptab.data() + (size_t)(op.ptab_row[kl] + r) * nhp;
          for (int q = 0; q < nhp; ++q) t[q] = zero;
          if (r >= S.nl[kl]) continue;
          const uint32_t v = ly->lo_pat[S.lo_off[kl] + r];
          for (size_t q = 0; q < nlds; ++q) {
            const Sc3Hop &h = hops[q];               // (the LDS hops of the lo pass come first)
            if (__builtin_popcount(v & h.mLo) == h.half) t[q] = (uint16_t)(ly->lo_rank[v ^ h.mLo] * esz);
          }
        }
      }
      op.nhp = nhp;
      pcoef.assign((size_t)nhp, 0.0);
      for (size_t q = 0; q < nlds; ++q) pcoef[q] = hops[q].up_re;
    }
  }
}

// diagonal on the fly: split the mask-0 terms by what their sign masks see
void Sc3Mat::split_diagonal(const std::vector<int64_t> &masks, const std::vector<int64_t> &mask_offsets,
                            const std::vector<int64_t> &signs, const std::vector<double> &rcoef) {
  const int a = ly->host.a;
  const int64_t nmasks = (int64_t)masks.size();
  diag_mode = 0;
  dlo.clear();
  dt_sign.clear();
  dt_coef.clear();
  dt_group.clear();
  op.ngroups = 0;
  if (nmasks > 0 && masks[0] == 0) {
    diag_mode = 2;
    const uint64_t lom = ((uint64_t)1 << a) - 1;
    dlo.assign(ly->lo_pat.size(), 0.0);
    std::vector<uint64_t> groups;
    for (int64_t tt = mask_offsets[0]; tt < mask_offsets[1]; ++tt) {
      const uint64_t sg = (uint64_t)signs[tt];
      const double c = rcoef[tt];
      if ((sg & ~lom) == 0) {
        for (size_t i = 0; i < ly->lo_pat.size(); ++i)
          dlo[i] += (__builtin_popcountll(ly->lo_pat[i] & sg) & 1) ? -c : c;
        continue;
      }
      int g = 0;
      if (sg & lom) {
        size_t j = 0;
        while (j < groups.size() && groups[j] != (sg & lom)) ++j;
        if (j == groups.size()) groups.push_back(sg & lom);
        g = (int)j + 1;
      }
      dt_sign.push_back((sg >> a) | ((uint64_t)g << 61));
      dt_coef.push_back(c);
      dt_group.push_back(g);
    }
    if (groups.size() > 4) diag_mode = 1;      // too many mixed patterns: the cached diagonal instead
    else {
      op.ngroups = (int32_t)groups.size();
      for (size_t j = 0; j < groups.size(); ++j) op.glo[j] = (uint32_t)groups[j];
    }
  }
  op.ndt = diag_mode == 2 ? (int32_t)dt_sign.size() : 0;
}

// Dispatch orders: workgroups that gather from each other run on one XCD at one time (their requests meet in that
// XCD's L2).  Both passes start from the rank's T blocks by popcount class, ascending inside a class.
std::vector<std::vector<uint32_t>> Sc3Mat::own_blocks_by_popcount() const {
  std::vector<std::vector<uint32_t>> Tby(ly->host.t + 1);
  for (uint32_t bq = T0; bq < T1 && bq < (uint32_t)ly->tseq.size(); ++bq) Tby[__builtin_popcount(ly->tseq[bq])].push_back(ly->tseq[bq]);
  for (auto &v : Tby) std::sort(v.begin(), v.end());
  return Tby;
}

// lo pass of a chain: the groups of rows that go to one XCD back to back
std::vector<std::vector<uint32_t>> Sc3Mat::lo_groups_pairs() const {
  const Sc3Tab &S = ly->host;
  const int a = S.a, w = S.w, t = S.t, k = S.k;
  const std::vector<std::vector<uint32_t>> Tby = own_blocks_by_popcount();
  std::vector<std::vector<uint32_t>> gA;
  for (int kt = 0; kt <= t; ++kt) {
    if (Tby[kt].empty()) continue;
    const int kr = k - kt;
    for (int cw = 0; cw <= w; ++cw) {
      const int kl = kr - cw;
      if (kl < 0 || kl > a) continue;
      // it gathers the Lo/W boundary bond only, which couples the rows (T, W) and (T, W ^ 1): each pair goes to
      // one XCD back to back, so that what one row gathers is what the other stages (their requests meet in the L2);
      // pairs of one (cw, wr) over the T's of the class follow each other -- equal lengths side by side
      for (int wr = 0; wr < S.nw[cw]; ++wr) {
        const uint32_t W = ly->w_pat[S.w_off[cw] + wr];
        const int klp = (W & 1u) ? kl + 1 : kl - 1;                 // Lo ones of the partner row (T, W ^ 1)
        const bool partner = klp >= 0 && klp <= a;
        if ((W & 1u) && partner) continue;                          // listed with its even partner
        for (uint32_t T : Tby[kt]) {
          std::vector<uint32_t> g{(T << w) | W};
          if (partner) g.push_back((T << w) | (W ^ 1u));
          gA.push_back(g);
        }
      }
    }
  }
  return gA;
}

// Bond graphs: the lo pass gathers, for every hop between Lo and W, from the row (T, W ^ bit) -- rows that differ
// in the window bits such hops touch go to one XCD back to back (what one of them gathers is what another stages:
// the requests meet in that XCD's L2), and the groups of one window pattern over all T's follow each other, so that
// the partner blocks of the hops between Lo and T are at least in the Infinity Cache.  DNM_SC3G_ORDER=0: the chain's
// order (pairs under window bit 0).
std::vector<std::vector<uint32_t>> Sc3Mat::lo_groups_graph() const {
  const Sc3Tab &S = ly->host;
  const int a = S.a, w = S.w, t = S.t, k = S.k;
  std::vector<std::vector<uint32_t>> gA;
  // the bits of a row's id (T << w | W) its gathered hops flip, by the number of hops that flip them; the six most
  // used ones span a group (DNM_SC3G_ORDER=w: window bits only, the first form of this order)
  const bool wonly = knob("DNM_SC3G_ORDER") && knob("DNM_SC3G_ORDER")[0] == 'w';
  std::vector<std::pair<int, int>> use;                        // (-count, bit)
  for (int b = 0; b < t + w; ++b) {
    int cnt = 0;
    for (size_t q = (size_t)op.nldsA; q < (size_t)(op.nldsA + op.ngatA); ++q) {      // the lo pass's gathered hops
      const uint64_t fl = ((uint64_t)hops[q].mT << w) | hops[q].mW;
      if (__builtin_popcountll(fl) == 1 && ((fl >> b) & 1ull) && !(wonly && b >= w)) ++cnt;
    }
    if (cnt) use.push_back({-cnt, b});
  }
  std::sort(use.begin(), use.end());
  uint32_t jm = 0;
  for (size_t q = 0; q < use.size() && q < 6; ++q) jm |= 1u << use[q].second;     // at most 64 rows to a group (what an XCD holds)
  std::vector<uint32_t> subs;
  for (uint32_t sset = jm;; sset = (sset - 1) & jm) {           // the subsets of jm, descending
    subs.push_back(sset);
    if (!sset) break;
  }
  std::reverse(subs.begin(), subs.end());
  const uint32_t wm = (1u << w) - 1u;
  for (uint32_t W0 = 0; W0 < (1u << w); ++W0) {
    if (W0 & jm & wm) continue;
    for (uint32_t Tb = 0; Tb < (1u << t); ++Tb) {
      if ((Tb << w) & jm) continue;
      std::vector<uint32_t> g;
      for (uint32_t sset : subs) {
        const uint32_t id = ((Tb << w) | W0) | sset, T = id >> w, W = id & wm;
        if (!ly->in_range(T, T0, T1)) continue;
        const int kl = k - __builtin_popcount(T) - __builtin_popcount(W);
        if (kl >= 0 && kl <= a) g.push_back(id);
      }
      if (!g.empty()) gA.push_back(g);
    }
  }
  return gA;
}

void Sc3Mat::lo_dispatch() {
  const bool chain_order = !graph || (knob("DNM_SC3G_ORDER") && knob("DNM_SC3G_ORDER")[0] == '0');
  permA = pack_lo_rows(deal(chain_order ? lo_groups_pairs() : lo_groups_graph()), *ly, sc3_lo_shape(ly->host.a, real));
  if (permA.empty()) permA.assign(8, 0xffffffffu);
}

// Window pass: groups (kt, cw, run) over the T's of a popcount class -- siblings under the T bonds -- then (unless
// DNM_SC3G_WORDER=0) regrouped by Lo population and column block
int Sc3Mat::window_dispatch() {
  const Sc3Tab &S = ly->host;
  const int a = S.a, w = S.w, t = S.t, k = S.k;
  const std::vector<std::vector<uint32_t>> Tby = own_blocks_by_popcount();
  std::vector<std::vector<uint32_t>> gB;
  for (int kt = 0; kt <= t; ++kt) {
    if (Tby[kt].empty()) continue;
    const int kr = k - kt;
    for (int cw = 0; cw <= w; ++cw) {
      const int kl = kr - cw;
      if (kl < 0 || kl > a) continue;
      // (real vectors: the window pass runs on pairs of entries, rows of pitch / 2 elements)
      const int Rr = 16 << S.rs[cw], nrun = ((real ? S.pitch[kl] / 2 : S.pitch[kl]) + Rr - 1) / Rr;
      DNM_CHECK(nrun < 4096, "internal: too many runs");
      for (int run = 0; run < nrun; ++run) {
        std::vector<uint32_t> g;
        for (uint32_t T : Tby[kt]) g.push_back((T << 16) | (cw << 12) | run);
        gB.push_back(g);
      }
    }
  }
  // Window pass: a hop between W and T (the chain's W/T boundary bond; any such pair of a bond graph) couples the class
  // (T, cw) to (T ^ bit, cw -+ 1) at the same columns -- the same number of ones in Lo.  Workgroups of one Lo population
  // and one block of 64 columns form a group, ordered by their first column inside it, so that such partners run on one
  // XCD at about the same time (the first order grouped the T's of one popcount class at fixed (cw, run): partners under
  // the hops inside T only, which this order keeps together as well).  kagome-30: the pass's fetch 59.6 -> 28.6 B/row, L2
  // hits 49 -> 70 %, 2.40 -> 2.22 ms (profiles/r05_kagome_window_order.txt); chains: SpinConserve(32,16) 35.8 -> 30.5
  // B/row, 5.30 -> 5.07 ms, a rank of config 5 24.6 -> 24.2 ms (profiles/r05_chain_window_order.txt).
  // DNM_SC3G_WORDER=0: the first order.
  const char *worder = knob("DNM_SC3G_WORDER");
  if (!(worder && worder[0] == '0')) {
    struct Wg { uint32_t e; int kl, col; };
    std::vector<Wg> all;
    for (auto &g : gB)
      for (uint32_t e : g) {
        const uint32_t T = e >> 16;
        const int cw = (e >> 12) & 15, run = e & 0xfff;
        all.push_back({e, k - __builtin_popcount(T) - cw, run * (16 << S.rs[cw])});
      }
    int bs = 6;                                        // log2 of the column block (2^5 ... 2^7 level, 2^8: +1.5 %, 2^10: +6 %)
    if (const char *e = knob("DNM_SC3G_WBLOCK")) bs = atoi(e);
    std::stable_sort(all.begin(), all.end(), [bs](const Wg &x, const Wg &y) {
      if (x.kl != y.kl) return x.kl < y.kl;
      if ((x.col >> bs) != (y.col >> bs)) return (x.col >> bs) < (y.col >> bs);
      return x.col < y.col;
    });
    gB.clear();
    for (size_t i = 0; i < all.size();) {
      size_t j = i;
      std::vector<uint32_t> g;
      while (j < all.size() && all[j].kl == all[i].kl && (all[j].col >> bs) == (all[i].col >> bs)) g.push_back(all[j++].e);
      gB.push_back(g);
      i = j;
    }
  }
  permB = deal(gB);
  if (permB.empty()) permB.assign(8, 0xffffffffu);
  return 0;
}

// per-workgroup partial sums of the fused dot products: one set per workgroup of the lo pass
size_t sc3_dot_partials(const Sc3Mat &M) { return M.permA.size() / 8; }

// ---- what the vector-level launch wrappers check before they launch ---------------------------------------
// the rows of the T blocks [T0, T1) inside Ly.rows (sorted by T, then W) and the offsets of that range
RowRange row_range(const Sc3Layout &Ly, uint32_t T0, uint32_t T1) {
  const uint32_t nb = (uint32_t)Ly.tseq.size();
  const uint32_t b0 = std::min(T0, nb), b1 = std::max(b0, std::min(T1, nb));
  RowRange r;
  r.first = Ly.rowstart[b0];
  r.count = Ly.rowstart[b1] - Ly.rowstart[b0];
  int64_t il, nl;
  sc3_range(Ly, T0, T1, &r.ioff, &il, &r.noff, &nl);
  return r;
}
// the maps between a layout and the reference order need the range's reference side to be a range too: every range of
// block order 0, whole vectors of the others
int ref_side(const Sc3Layout &Ly, const RowRange &r) {
  DNM_CHECK(Ly.order == 0 || (r.first == 0 && r.count == Ly.rows.size()),
            "a rank's share of a SpinConserve layout in block order %d is no range of the reference order", Ly.order);
  return 0;
}

// a relabelled layout covers whole vectors on one rank
int perm_whole(const Sc3Layout &Ly, const Sc3Perm *perm, const RowRange &r) {
  // (whole vectors, or the blocks below a bound -- the half whose top bit is clear, an XParity vector: both start at
  // position 0 of the layout and at index 0 of the reference order)
  DNM_CHECK(!perm || !perm->on || (r.first == 0 && r.ioff == 0 && r.noff == 0),
            "a relabelled SpinConserve layout is not partitioned over ranks");
  return 0;
}

// ---- the device side -------------------------------------------------------------------------------------
int Sc3Layout::upload() {
  DNM_TRY(d_ibase.upload(ibase)); DNM_TRY(d_nbase.upload(nbase)); DNM_TRY(d_icoff.upload(icoff));
  DNM_TRY(d_ncoff.upload(ncoff)); DNM_TRY(d_lo_pat.upload(lo_pat)); DNM_TRY(d_w_pat.upload(w_pat));
  DNM_TRY(d_lo_rank.upload(lo_rank)); DNM_TRY(d_w_rank.upload(w_rank)); DNM_TRY(d_cbin.upload(cbin));
  DNM_TRY(d_rows.upload(rows)); DNM_TRY(d_nck.upload(nck)); DNM_TRY(d_w_nb.upload(w_nb));
  DNM_TRY(d_lo_rlo.upload(lo_rlo)); DNM_TRY(d_lo_rhi.upload(lo_rhi));
  DNM_TRY(d_ibase_h.upload(ibase_h)); DNM_TRY(d_icoff_h.upload(icoff_h));
  dev = host;
  dev.ibase = d_ibase.as<int64_t>(); dev.nbase = d_nbase.as<int64_t>();
  dev.icoff = d_icoff.as<int64_t>(); dev.ncoff = d_ncoff.as<int64_t>();
  dev.lo_pat = d_lo_pat.as<uint16_t>(); dev.w_pat = d_w_pat.as<uint16_t>();
  dev.lo_rank = d_lo_rank.as<uint16_t>(); dev.w_rank = d_w_rank.as<uint16_t>();
  dev.cbin = d_cbin.as<int32_t>();
  dev.nck = d_nck.as<int64_t>();
  dev.w_nb = d_w_nb.as<uint64_t>();
  dev.lo_rlo = d_lo_rlo.as<uint16_t>(); dev.lo_rhi = d_lo_rhi.as<uint16_t>();
  // the halved tables differ from the whole ones in what host_h does
  dev_h = dev;
  dev_h.ibase = d_ibase_h.as<int64_t>();
  dev_h.icoff = d_icoff_h.as<int64_t>();
  dev_h.nint = host_h.nint;
  for (int j = 0; j <= host.a; ++j) dev_h.pitch[j] = host_h.pitch[j];
  on_device = true;
  return 0;
}

int Sc3Mat::upload() {
  DNM_TRY(d_rowsel.upload(rowsel));
  if (!tiled) return 0;
  DNM_TRY(d_permA.upload(permA)); DNM_TRY(d_permB.upload(permB)); DNM_TRY(d_bond.upload(bond));
  op.bond = d_bond.as<double>();
  if (graph) {
    DNM_TRY(d_hops.upload(hops)); DNM_TRY(d_wnb.upload(wnb));
    op.ldsA = d_hops.as<Sc3Hop>();
    op.gatA = op.ldsA + op.nldsA;
    op.ldsB = op.gatA + op.ngatA;
    op.gatB = op.ldsB + op.nldsB;
    op.wnb = d_wnb.as<uint8_t>();
    if (!ptab.empty()) {
      DNM_TRY(d_ptab.upload(ptab)); DNM_TRY(d_pcoef.upload(pcoef));
      op.ptab = d_ptab.as<uint16_t>();
      op.pcoef = d_pcoef.as<double>();
    }
  }
  if (diag_mode == 2) {
    DNM_TRY(d_dlo.upload(dlo)); DNM_TRY(d_dt_sign.upload(dt_sign)); DNM_TRY(d_dt_coef.upload(dt_coef));
    DNM_TRY(d_dt_group.upload(dt_group));
    op.dlo = d_dlo.as<double>(); op.dt_sign = d_dt_sign.as<uint64_t>();
    op.dt_coef = d_dt_coef.as<double>(); op.dt_group = d_dt_group.as<int32_t>();
  }
  return 0;
}

}  // namespace dnm
