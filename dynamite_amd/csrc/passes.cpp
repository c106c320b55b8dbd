// The records the tiled kernel reads (plan.h: DevPass, DevQuad, DevTab, DevFlip), built on the host from the operator
// and its plan.  Nothing here touches the device: PassRecords::upload (mat.cpp) does, for handles that have one.
#include "passes.h"

#include <algorithm>
#include <cstring>

namespace dnm {

// ---------------------------------------------------------------------------
// MSC -> row-evaluated index-space form (see plan.h).  Full: identity map.
// Parity: index = state >> 1; the dropped bit parity(idx)^space is folded
// into the sign masks (cf. the check_parity branch of sum_term,
// bpetsc_template_2.c:659-662, 848-854).
// ---------------------------------------------------------------------------
int build_opform(const dnm_mat &A, OpForm *op) {
  const SubView &l = A.left.host, &r = A.right.host;
  const bool par = l.type == DNM_PARITY;
  const int n = par ? l.L - 1 : l.L;
  op->n = n;
  op->masks.clear();
  const uint64_t ones = n >= 64 ? ~0ull : (((uint64_t)1 << n) - 1);
  for (size_t mi = 0; mi < A.masks.size(); ++mi) {
    const uint64_t mask = (uint64_t)A.masks[mi];
    if (par && (parity64(mask) != (l.space ^ r.space))) continue;   // maps outside the right space
    RowMask rm;
    rm.mask = par ? (mask >> 1) : mask;
    for (int64_t t = A.mask_offsets[mi]; t < A.mask_offsets[mi + 1]; ++t) {
      const uint64_t sg = (uint64_t)A.signs[t];
      RowTerm rt;
      rt.is_imag = parity64(mask & sg);           // !TERM_REAL
      double c = A.real_coeffs[t];
      uint64_t s2 = sg;
      if (par) {
        s2 = sg >> 1;
        if (sg & 1) {
          s2 ^= ones;
          if (r.space) c = -c;
        }
      }
      // column-evaluated -> row-evaluated: col = row ^ mask
      if (parity64(rm.mask & s2)) c = -c;
      rt.sign = s2;
      rt.coeff = c;
      rm.terms.push_back(rt);
    }
    if (rm.mask == 0) {
      RowMask im;
      im.mask = 0;
      im.zero_mask_offdiag = true;
      std::vector<RowTerm> re;
      for (const RowTerm &t : rm.terms) (t.is_imag ? im.terms : re).push_back(t);
      rm.terms.swap(re);
      if (!im.terms.empty()) op->masks.push_back(std::move(im));
      if (rm.terms.empty()) continue;
    }
    op->masks.push_back(std::move(rm));
  }
  std::stable_sort(op->masks.begin(), op->masks.end(),
            [](const RowMask &a, const RowMask &b) { return a.mask < b.mask; });
  return 0;
}

static uint32_t compress_to_tile(uint64_t bits, const PassSpec &ps) {
  uint32_t out = 0;
  int off = 0;
  for (int j = 0; j < ps.nseg; ++j) {
    uint64_t seg = (bits >> ps.seg_pos[j]) & (((uint64_t)1 << ps.seg_len[j]) - 1);
    out |= (uint32_t)seg << off;
    off += ps.seg_len[j];
  }
  return out;
}

// Real-packed form of a real operator (DNM_MAT_REAL_PACKED): index r = 2 j + b, element j of a vector holds the
// amplitudes b = 0 (real part) and b = 1 (imaginary part).  A term (mask m, sign s, coefficient c) contributes
// c (-1)^popcount(r & s) x[r ^ m] to y[r]; with m' = m >> 1, s' = s >> 1, f = m & 1:
//   y[j].lane(b) += c (-1)^popcount(j & s') (-1)^(b (s & 1)) x[j ^ m'].lane(b ^ f)
// -- one coefficient per lane.  The form keeps the record layout: a term's is_imag names its lane, the records of a
// mask carry both lanes (slots 0, 1: lane 0; slots 2, 3: lane 1) and RowMask::pack_flip = f.  Diagonal terms whose
// sign reaches bit 0 differ between the lanes: they become a mask-0 off-diagonal entry (partner = the element itself).
int pack_opform(OpForm *op) {
  DNM_CHECK(op->n >= 2, "real-packed form needs at least two index bits");
  std::vector<RowMask> out;
  for (const RowMask &rm : op->masks) {
    for (const RowTerm &t : rm.terms) DNM_CHECK(!t.is_imag, "operator has an imaginary matrix element: no real-packed form");
    DNM_CHECK(!rm.zero_mask_offdiag, "operator has an imaginary matrix element: no real-packed form");
    RowMask lanes;
    lanes.mask = rm.mask >> 1;
    lanes.pack_flip = (rm.mask & 1) != 0;
    if (rm.mask == 0) {
      RowMask diag;                       // what both lanes share stays the diagonal
      diag.mask = 0;
      lanes.zero_mask_offdiag = true;
      for (const RowTerm &t : rm.terms) {
        if (!(t.sign & 1)) { diag.terms.push_back({t.sign >> 1, t.coeff, 0}); continue; }
        lanes.terms.push_back({t.sign >> 1, t.coeff, 0});
        lanes.terms.push_back({t.sign >> 1, -t.coeff, 1});
      }
      if (!diag.terms.empty()) out.push_back(std::move(diag));
      if (!lanes.terms.empty()) out.push_back(std::move(lanes));
      continue;
    }
    lanes.zero_mask_offdiag = lanes.mask == 0;       // the mask flipped bit 0 only: the element's own other lane
    bool same = !lanes.pack_flip;                    // bit 0 neither flipped nor seen by a sign: both lanes get the same
    for (const RowTerm &t : rm.terms) same = same && !(t.sign & 1);      // real coefficient -- an ordinary real record
    for (const RowTerm &t : rm.terms) {
      lanes.terms.push_back({t.sign >> 1, t.coeff, 0});
      if (!same) lanes.terms.push_back({t.sign >> 1, (t.sign & 1) ? -t.coeff : t.coeff, 1});
    }
    out.push_back(std::move(lanes));
  }
  std::stable_sort(out.begin(), out.end(), [](const RowMask &a, const RowMask &b) {
    if (a.mask != b.mask) return a.mask < b.mask;
    return (int)a.zero_mask_offdiag < (int)b.zero_mask_offdiag;        // the diagonal first
  });
  op->masks.swap(out);
  op->n -= 1;
  op->packed = true;
  return 0;
}

// A mask of many terms as table records (plan.h: DevTab)?  Its terms grouped by their sign mask outside the flipped bits
// (`zs`: one record and one table per group) -- taken where that is cheaper than records of four terms (about 45 against
// 76 vector instructions each for four rows; DNM_TAB_RECORDS=0: never).
static bool table_form(const OpForm &op, const RowMask &m, std::vector<uint64_t> *zs) {
  const char *tabs_env = knob("DNM_TAB_RECORDS");
  if (tabs_env && tabs_env[0] == '0') return false;
  const int nb = __builtin_popcountll(m.mask);
  if (op.packed || m.pack_flip || nb < 1 || nb > MAXTABBITS || m.terms.size() < 5) return false;
  size_t nre = 0, nim = 0;
  zs->clear();
  for (const RowTerm &t : m.terms) {
    (t.is_imag ? nim : nre)++;
    const uint64_t z = t.sign & ~m.mask;
    if (std::find(zs->begin(), zs->end(), z) == zs->end()) zs->push_back(z);
  }
  // (masks of one record stay records: a single flip's X + iY -- the harness's long_range -- as a table of two entries made
  // that operator SLOWER, 7.11 -> 7.59 ms at L=28: a table record has its own fixed costs, the staging of the tables and the
  // kernel instance of 8 rows per thread among them)
  const size_t nq = std::max((nre + 1) / 2, (nim + 1) / 2);
  return nq >= 2 && zs->size() * 45 < nq * 76;
}

// the operator's diagonal (its mask-0 entry of real terms), or null
static const RowMask *diagonal_mask(const OpForm &op) {
  const RowMask *dm = nullptr;
  for (const RowMask &m : op.masks) if (m.mask == 0 && !m.zero_mask_offdiag) dm = &m;
  return dm;
}

// A mask as a flip-flop record (plan.h: DevFlip)?  It flips exactly two bits, its terms are real and see no other bit,
// and their sum is c on the rows whose two bits differ and nothing on the others: a bond a (XX + YY), c = 2a.  (A Parity
// mask whose folded bit spreads a sign mask over the index does not qualify, nor does XX alone or a DM term.)
static FlipBond flip_classify(const RowMask &m) {
  FlipBond fb;
  if (__builtin_popcountll(m.mask) != 2 || m.zero_mask_offdiag || m.pack_flip) return fb;
  fb.b0 = __builtin_ctzll(m.mask);
  fb.b1 = 63 - __builtin_clzll(m.mask);
  double f[4] = {0.0, 0.0, 0.0, 0.0};      // the coefficient by (bit b0, bit b1) of the row
  for (const RowTerm &t : m.terms) {
    if (t.is_imag || (t.sign & ~m.mask)) return fb;
    for (int v = 0; v < 4; ++v) {
      const int par = ((v & 1) && ((t.sign >> fb.b0) & 1)) ^ ((v & 2) && ((t.sign >> fb.b1) & 1));
      f[v] += par ? -t.coeff : t.coeff;
    }
  }
  if (f[0] != 0.0 || f[3] != 0.0 || f[1] != f[2] || f[1] == 0.0) return fb;
  fb.c = f[1];
  fb.ok = true;
  return fb;
}

// The records of a pass from a list of diagonal terms (null: none) and the masks that `skip` does not name (empty: all):
// once for the generic description of the pass (the operator's own diagonal, every mask), once more for the kernel when
// some of the operator's masks run as flip-flop records (plan.h: DevFlip; build_flip_pass below).  Fills the records and
// their ranges in out.desc (the table records merged: tile, then gathered); the geometry in out.desc, log_rows
// included, is the caller's.
static int emit_records(const dnm_mat &A, const PassSpec &ps, PassRecords &out, const std::vector<RowTerm> *dterms,
                        const std::vector<char> &skip) {
  const OpForm &op = A.op;
  DevPass &d = out.desc;
  const int B = ps.B, logR = d.log_rows, lognt = B - logR, R = 1 << logR;
  const int n_eff = ps.n_eff ? ps.n_eff : A.plan.n_loc;
  const uint64_t tb = ps.tile_bits();
  std::vector<DevQuad> &quads = out.quads;
  std::vector<double> &dtile = out.dtile, &tabvals = out.tabvals;
  std::vector<DevTab> &tabs_tile = out.tabs, tabs_gather;
  auto empty_quad = [&]() {
    DevQuad q;
    memset(&q, 0, sizeof(q));
    return q;
  };
  auto set_slot = [&](DevQuad &q, int slot, const RowTerm &t) {
    q.sign_ext[slot] = t.sign & ~tb;
    q.sign_tile[slot] = compress_to_tile(t.sign & tb, ps);
    q.coeff[slot] = t.coeff;
  };
  // pack a list of (real) diagonal terms four to a record
  auto push_diag_list = [&](const std::vector<RowTerm> &lst) {
    for (size_t i = 0; i < lst.size(); i += 4) {
      DevQuad q = empty_quad();
      for (size_t j = i; j < lst.size() && j < i + 4; ++j) {
        set_slot(q, (int)(j - i), lst[j]);
        q.nslots = (uint32_t)(j - i + 1);
      }
      quads.push_back(q);
    }
  };

  if (ps.has_diag && dterms) {
    d.has_diag = 1;
    std::vector<RowTerm> lst;
    for (const RowTerm &t : *dterms)
      if (compress_to_tile(t.sign & tb, ps) == 0) lst.push_back(t);
    d.dext_begin = (uint32_t)quads.size();
    push_diag_list(lst);
    d.dext_end = (uint32_t)quads.size();
    // terms inside the tile only: tabulated per tile coordinate (DNM_DIAG_TABLE=0: bucket lists as before)
    const char *dte = knob("DNM_DIAG_TABLE");
    const bool use_table = !(dte && dte[0] == '0') && B <= 13;
    if (use_table) dtile.assign((size_t)1 << B, 0.0);
    // terms that see the tile AND bits outside it, grouped by their sign mask inside the tile (DevPass::gbucket): groups of
    // three terms or more are summed over the outside bits once per workgroup (DNM_DIAG_GROUPS=0: every term per thread)
    std::vector<std::pair<uint32_t, std::vector<RowTerm>>> groups;
    {
      const char *dge = knob("DNM_DIAG_GROUPS");
      const bool grouping = !(dge && dge[0] == '0') && !op.packed && !(A.flags & DNM_MAT_USE_GLDS);
      std::vector<std::pair<uint32_t, std::vector<RowTerm>>> all;
      if (grouping)
        for (const RowTerm &t : *dterms) {
          const uint32_t st = compress_to_tile(t.sign & tb, ps);
          if (st == 0 || (t.sign & ~tb) == 0) continue;
          auto it = std::find_if(all.begin(), all.end(), [&](const auto &g) { return g.first == st; });
          if (it == all.end()) { all.push_back({st, {}}); it = all.end() - 1; }
          it->second.push_back(t);
        }
      std::stable_sort(all.begin(), all.end(), [](const auto &a, const auto &b) { return a.second.size() > b.second.size(); });
      for (auto &g : all)
        if (g.second.size() >= 3 && groups.size() < MAXDGROUPS) groups.push_back(std::move(g));
    }
    auto grouped = [&](uint32_t st) {
      return std::any_of(groups.begin(), groups.end(), [&](const auto &g) { return g.first == st; });
    };
    for (int j = 0; j < R; ++j) {
      lst.clear();
      for (const RowTerm &t : *dterms) {
        uint32_t st = compress_to_tile(t.sign & tb, ps);
        if (st == 0 || (int)(st >> lognt) != j) continue;
        if (use_table && (t.sign & ~tb) == 0) {
          for (uint32_t tc = 0; tc < (1u << B); ++tc)
            dtile[tc] += (__builtin_popcount(tc & st) & 1) ? -t.coeff : t.coeff;
        } else if ((t.sign & ~tb) != 0 && grouped(st)) {
          continue;
        } else {
          lst.push_back(t);
        }
      }
      d.dbucket[j] = (uint32_t)quads.size();
      push_diag_list(lst);
    }
    for (int j = R; j <= MAXR; ++j) d.dbucket[j] = (uint32_t)quads.size();
    // the groups: their term records (the outside part of every sign mask), then one record per group, by k bucket
    std::vector<std::pair<uint32_t, uint32_t>> where(groups.size());
    for (size_t g = 0; g < groups.size(); ++g) {
      std::vector<RowTerm> outside = groups[g].second;
      for (RowTerm &t : outside) t.sign &= ~tb;
      where[g].first = (uint32_t)quads.size();
      push_diag_list(outside);
      where[g].second = (uint32_t)quads.size() - where[g].first;
    }
    for (int j = 0; j < R; ++j) {
      d.gbucket[j] = (uint32_t)quads.size();
      for (size_t g = 0; g < groups.size(); ++g) {
        if ((int)(groups[g].first >> lognt) != j) continue;
        DevQuad q = empty_quad();
        q.sign_tile[0] = groups[g].first;
        q.mask_loc = where[g].first;
        q.src = where[g].second;
        q.nslots = 1;
        quads.push_back(q);
      }
    }
    for (int j = R; j <= MAXR; ++j) d.gbucket[j] = (uint32_t)quads.size();
  }

  // off-diagonal masks: records of <= 2 real + <= 2 imaginary terms, sorted into
  // the kernel's loops (tile/gather x k-variant x real/complex)
  struct Rec { int loop; DevQuad q; };
  std::vector<Rec> recs;
  // masks of many terms as table records (table_form above)
  auto push_tabs = [&](const RowMask &m, uint64_t mloc, bool gather, int src) -> bool {
    std::vector<uint64_t> zs;
    if (!table_form(op, m, &zs)) return false;
    const int nb = __builtin_popcountll(m.mask);
    int pb[MAXTABBITS];
    for (int q = 0, pos = 0; pos < 64; ++pos)
      if ((m.mask >> pos) & 1ull) pb[q++] = pos;
    for (uint64_t z : zs) {
      DevTab T;
      memset(&T, 0, sizeof(T));
      T.mask_tile = compress_to_tile(mloc & tb, ps);
      T.mask_loc = (uint32_t)mloc;
      T.src = (uint32_t)src;
      T.nbits = (uint32_t)nb;
      const uint32_t zt = compress_to_tile(z & tb, ps);
      T.z_tile = zt & ((1u << lognt) - 1u);
      T.z_ext = z & ~tb;
      T.first = (uint32_t)(tabvals.size() / 2);
      for (int k = 0; k < R; ++k)
        if (__builtin_popcount((uint32_t)k & (zt >> lognt)) & 1) T.ksign |= 1u << k;
      for (int q = 0; q < nb; ++q) {
        if ((tb >> pb[q]) & 1ull) {
          const int tpos = __builtin_ctz(compress_to_tile((uint64_t)1 << pb[q], ps));
          if (tpos < lognt) {
            T.tpos |= (uint32_t)tpos << (8 * q);
            T.twid |= 1u << (8 * q);
          } else {
            T.flags |= 1u;
            for (int k = 0; k < R; ++k)
              if ((k >> (tpos - lognt)) & 1) T.ik |= (uint64_t)1 << (4 * k + q);
          }
        } else {
          T.epos |= (uint32_t)pb[q] << (8 * q);
          T.ewid |= 1u << (8 * q);
        }
      }
      for (int j = 0; j < (1 << nb); ++j) {
        uint64_t rowbits = 0;
        for (int q = 0; q < nb; ++q)
          if ((j >> q) & 1) rowbits |= (uint64_t)1 << pb[q];
        double re = 0.0, im = 0.0;
        for (const RowTerm &t : m.terms) {
          if ((t.sign & ~m.mask) != z) continue;
          const double c = (__builtin_popcountll(rowbits & t.sign & m.mask) & 1) ? -t.coeff : t.coeff;
          (t.is_imag ? im : re) += c;
        }
        tabvals.push_back(re);
        tabvals.push_back(im);
      }
      if (z == zs.back()) T.flags |= 2u;        // (the groups of a mask: consecutive records, one fetch of the partners)
      (gather ? tabs_gather : tabs_tile).push_back(T);
    }
    return true;
  };
  auto push_mask = [&](int idx, bool gather, int src) {
    const RowMask &m = op.masks[idx];
    const uint64_t mloc = m.mask & (((uint64_t)1 << n_eff) - 1);
    if (!gather) DNM_CHECK((mloc & ~tb) == 0, "internal: tile mask leaves the tile");
    if (push_tabs(m, mloc, gather, src)) return 0;
    std::vector<const RowTerm *> re, im;
    for (const RowTerm &t : m.terms) (t.is_imag ? im : re).push_back(&t);
    size_t ir = 0, ii = 0;
    while (ir < re.size() || ii < im.size()) {
      DevQuad q = empty_quad();
      q.mask_tile = compress_to_tile(mloc & tb, ps);
      q.mask_loc = (uint32_t)mloc;
      q.src = (uint32_t)src;
      q.nslots = m.pack_flip ? 1u : 0u;       // real-packed operators: a lane reads the partner's other lane
      bool kvar = false, cplx = false;
      for (int s = 0; s < 2 && ir < re.size(); ++s, ++ir) {
        set_slot(q, s, *re[ir]);
        kvar |= (q.sign_tile[s] >> lognt) != 0;
      }
      for (int s = 2; s < 4 && ii < im.size(); ++s, ++ii) {
        set_slot(q, s, *im[ii]);
        kvar |= (q.sign_tile[s] >> lognt) != 0;
        cplx = true;
      }
      int loop;
      if (gather) loop = kvar ? (cplx ? LP_GATHER_KVAR_CPLX : LP_GATHER_KVAR_REAL) : (cplx ? LP_GATHER_CPLX : LP_GATHER_REAL);
      else if (kvar) loop = cplx ? LP_TILE_KVAR_CPLX : LP_TILE_KVAR_REAL;
      else if (cplx) loop = LP_TILE_CPLX;
      else loop = (q.mask_tile >> lognt) == 0 ? LP_TILE_REAL_K0 : LP_TILE_REAL;
      recs.push_back({loop, q});
    }
    return 0;
  };
  for (int idx : ps.tile_masks)
    if (skip.empty() || !skip[idx]) DNM_TRY(push_mask(idx, false, 0));
  for (size_t i = 0; i < ps.gather_masks.size(); ++i)
    if (skip.empty() || !skip[ps.gather_masks[i]]) DNM_TRY(push_mask(ps.gather_masks[i], true, ps.gather_src[i]));
  for (int lp = 0; lp < LP_COUNT; ++lp) {
    d.loop[lp] = (uint32_t)quads.size();
    for (const Rec &r : recs) if (r.loop == lp) quads.push_back(r.q);
  }
  d.loop[LP_COUNT] = (uint32_t)quads.size();
  d.nquads = (int32_t)quads.size();
  d.tab_loop[0] = 0;
  d.tab_loop[1] = (uint32_t)tabs_tile.size();
  tabs_tile.insert(tabs_tile.end(), tabs_gather.begin(), tabs_gather.end());
  d.tab_loop[2] = (uint32_t)tabs_tile.size();
  return 0;
}

// The geometry of a pass: rows per thread, tile segments, the order of the block bits, the constants of the vector
// layout and pos_tmask -- everything in d but the record ranges (emit_records) and need_tile (build_pass)
static int pass_geometry(const dnm_mat &A, const PassSpec &ps, DevPass &d) {
  const OpForm &op = A.op;
  const Plan &pl = A.plan;
  const int B = ps.B;
  int logR = ps.logR ? ps.logR : pl.cfg.logR;
  {
    // passes with table records: rows per thread of their own (DNM_TAB_LOG_ROWS; the per-record work of a thread -- table
    // index, parity -- is shared by its rows)
    std::vector<uint64_t> zs;
    bool any = false;
    for (int idx : ps.tile_masks) any = any || table_form(op, op.masks[idx], &zs);
    for (int idx : ps.gather_masks) any = any || table_form(op, op.masks[idx], &zs);
    int want = 3;
    if (const char *e = knob("DNM_TAB_LOG_ROWS")) want = atoi(e);
    if (any && want > logR && tile_config_supported(B, want)) logR = want;
  }
  {
    // the thread part of a position has to fit a 32-bit byte offset (DevPass::pos_tmask): a tile that reaches above
    // bit 27 gives its top bits to the rows of a thread
    auto top_thread_pos = [&](int lr) {
      int c = 0, top = -1;
      for (int j = 0; j < ps.nseg; ++j)
        for (int i = 0; i < ps.seg_len[j]; ++i, ++c)
          if (c < B - lr) top = std::max(top, ps.seg_pos[j] + i);
      return top;
    };
    while (top_thread_pos(logR) >= 28 && tile_config_supported(B, logR + 1)) ++logR;
  }
  const int lognt = B - logR, R = 1 << logR;
  const int n_eff = ps.n_eff ? ps.n_eff : pl.n_loc;     // index bits this pass sweeps
  const uint64_t tb = ps.tile_bits();
  memset(&d, 0, sizeof(d));
  d.nseg = ps.nseg;
  int off = 0;
  for (int j = 0; j < ps.nseg; ++j) {
    d.seg_off[j] = off;
    d.seg_len[j] = ps.seg_len[j];
    d.seg_pos[j] = ps.seg_pos[j];
    off += ps.seg_len[j];
  }
  DNM_CHECK(off == B, "internal: tile segments do not add up to B");
  // block-id bits -> local index bits outside the tile.  Order (low to high):
  // three selector bits (workgroup b runs on XCD b % 8), the XCD-group bits, the rest.
  {
    std::vector<int> order;
    uint64_t gb = ps.glen ? ((((uint64_t)1 << ps.glen) - 1) << ps.gpos) : 0;
    std::vector<int> rest;
    for (int pos = 0; pos < n_eff; ++pos)
      if (!((tb >> pos) & 1) && !((gb >> pos) & 1)) rest.push_back(pos);
    size_t nsel = ps.glen ? std::min<size_t>(3, rest.size()) : 0;
    for (size_t i = 0; i < nsel; ++i) order.push_back(rest[i]);
    for (int pos = ps.gpos; pos < ps.gpos + ps.glen; ++pos) order.push_back(pos);
    for (size_t i = nsel; i < rest.size(); ++i) order.push_back(rest[i]);
    if (const char *e = knob("DNM_ORDER_WINDOW")) {     // experiments: explicit block-id bit order (low to high)
      if (ps.nseg > 1 && ps.partner < 0) {
        std::vector<int> o;
        for (const char *q = e; *q;) {
          o.push_back(atoi(q));
          while (*q && *q != ',') ++q;
          if (*q == ',') ++q;
        }
        std::vector<int> a = o, b2 = order;
        std::sort(a.begin(), a.end());
        std::sort(b2.begin(), b2.end());
        DNM_CHECK(a == b2, "DNM_ORDER_WINDOW is not a permutation of the block bits");
        order = o;
      }
    }
    DNM_CHECK((int)order.size() == n_eff - B, "internal: block bits do not add up");
    int nb = 0;
    for (size_t i = 0; i < order.size();) {
      size_t j = i + 1;
      while (j < order.size() && order[j] == order[j - 1] + 1) ++j;
      DNM_CHECK(nb < MAXBSEG, "internal: too many block segments");
      d.bseg_off[nb] = (int32_t)i;
      d.bseg_len[nb] = (int32_t)(j - i);
      d.bseg_pos[nb] = order[i];
      ++nb;
      i = j;
    }
    d.nbseg = nb;
  }
  d.sign_base = ((uint64_t)pl.rank << pl.n_loc) | ps.sign_extra;
  d.n_eff = n_eff;
  d.tile_bits = B;
  d.log_rows = logR;
  DNM_CHECK(tile_config_supported(B, logR), "unsupported tile configuration B=%d logR=%d", B, logR);
  d.accumulate = ps.accumulate ? 1 : 0;
  d.has_diag = 0;
  d.cache_policy = pl.cfg.cache_policy | (op.packed ? 256 : 0);      // bit 8: real-packed records (kernel instance)
  {
    const int S = pl.cfg.swz;
    DNM_CHECK(S == 0 || (S >= 5 && S <= 24), "swizzle shift %d out of range", S);
    d.swz_shift = S;
    auto sw = [S](uint64_t v) -> uint32_t {
      return S ? (uint32_t)(((v >> S) & (((uint64_t)1 << (S - 4)) - 1)) << 4) : 0u;
    };
    d.swz_xor_y = sw((uint64_t)ps.y_off);
    d.swz_xor_src = sw((uint64_t)ps.src_off);
    // position bits the thread part of the tile coordinate reaches (the kernel keeps them in a 32-bit byte offset)
    uint64_t tm = 0;
    int c = 0;
    for (int j = 0; j < ps.nseg; ++j)
      for (int i = 0; i < ps.seg_len[j]; ++i, ++c)
        if (c < lognt) tm |= ((uint64_t)1 << (ps.seg_pos[j] + i)) | sw((uint64_t)1 << (ps.seg_pos[j] + i));
    DNM_CHECK((tm >> 28) == 0, "internal: thread bits of the tile above bit 27 (tile %llx, %d rows per thread)",
              (unsigned long long)tb, R);
    d.pos_tmask = (uint32_t)tm;
  }
  return 0;
}

int build_pass(const dnm_mat &A, const PassSpec &ps, PassOnDevice *out) {
  DevPass &d = out->whole.desc;
  DNM_TRY(pass_geometry(A, ps, d));
  const RowMask *dm = diagonal_mask(A.op);
  DNM_TRY(emit_records(A, ps, out->whole, dm ? &dm->terms : nullptr, std::vector<char>()));
  d.need_tile = (d.has_diag || !ps.tile_masks.empty()) ? 1 : 0;
  out->partner = ps.partner;
  out->n_eff = d.n_eff;
  out->y_off = ps.y_off;
  out->src_off = ps.src_off;
  return 0;
}

// The masks of an operator that run as flip-flop records (plan.h: DevFlip), decided ONCE per operator, after its passes
// have been built generically: A->flip_bonds[i] for op.masks[i].  None (DNM_FLIPFLOP=0, or an operator that needs another
// kernel instance: real-packed, late gathers, or any local pass whose generic form has table records or grouped diagonal
// terms -- read off the passes as emit_records built them) leaves the vector empty.
//   gathered masks: no condition beyond flip_classify (nothing changes but the record);
//   tile masks run as exchanges, which take a = c / 2 off the ZZ term on the bond's pair: taken only where the diagonal HAS
//   that term.  The reduced diagonal then has no sign mask that the operator's own lacks, so whatever emit_records groups
//   of it is a subset of what it grouped before -- a pass without grouped terms stays without.  (An XY bond would ADD a
//   term per bond, across the tile boundary of the diagonal pass one that every thread evaluates, three of them on one
//   spin a group: such bonds keep their generic tile records.)
void decide_flip_bonds(dnm_mat *A) {
  const OpForm &op = A->op;
  const Plan &pl = A->plan;
  A->flip_bonds.clear();
  const char *e = knob("DNM_FLIPFLOP");
  if ((e && e[0] == '0') || op.packed || !(pl.cfg.cache_policy & 32)) return;
  const RowMask *dm = diagonal_mask(op);
  bool diag_pass = false;
  for (size_t i = 0; i < pl.local.size(); ++i) {
    const DevPass &d = A->local_passes[i]->whole.desc;
    if (d.tab_loop[2] > 0 || d.gbucket[MAXR] > d.gbucket[0]) return;
    diag_pass = diag_pass || d.has_diag;
  }
  std::vector<FlipBond> bonds(op.masks.size());
  bool any = false;
  for (const PassSpec &ps : pl.local) {
    for (int idx : ps.tile_masks) {
      FlipBond fb = flip_classify(op.masks[idx]);
      const uint64_t pair = op.masks[idx].mask;
      fb.exch = fb.ok && diag_pass && dm &&
                std::any_of(dm->terms.begin(), dm->terms.end(), [&](const RowTerm &t) { return t.sign == pair; });
      fb.ok = fb.exch;
      bonds[idx] = fb;
      any = any || fb.ok;
    }
    for (size_t i = 0; i < ps.gather_masks.size(); ++i) {
      if (ps.gather_src[i] != 0) continue;
      bonds[ps.gather_masks[i]] = flip_classify(op.masks[ps.gather_masks[i]]);
      any = any || bonds[ps.gather_masks[i]].ok;
    }
  }
  if (any) A->flip_bonds.swap(bonds);
}

// What the kernel runs on when the operator has flip-flop records: the records of this local pass, the generic records
// that remain and the diagonal as the exchanges leave it (out->reduced, built by the same emit_records)
int build_flip_pass(const dnm_mat &A, const PassSpec &ps, PassOnDevice *out) {
  const OpForm &op = A.op;
  const Plan &pl = A.plan;
  const std::vector<FlipBond> &bonds = A.flip_bonds;
  if (bonds.empty()) return 0;
  const DevPass &d = out->whole.desc;
  const int lognt = d.tile_bits - d.log_rows;
  const uint64_t tb = ps.tile_bits();
  std::vector<char> skip(op.masks.size(), 0);
  std::vector<DevFlip> fl[FL_COUNT];
  const int S = pl.cfg.swz;
  auto add_flip = [&](int idx, bool gather) {
    const FlipBond &fb = bonds[idx];
    if (!fb.ok) return;
    DevFlip f;
    memset(&f, 0, sizeof(f));
    f.c = fb.c;
    const uint64_t b0 = (uint64_t)1 << fb.b0, b1 = (uint64_t)1 << fb.b1;
    int cls;
    if (!gather) {
      f.mask_tile = compress_to_tile(b0 | b1, ps);
      f.p0 = (uint32_t)__builtin_ctz(f.mask_tile);
      f.p1 = 31u - (uint32_t)__builtin_clz(f.mask_tile);
      cls = (int)f.p1 < lognt ? FL_TILE_T : FL_TILE_K;
    } else {
      const uint64_t mloc = b0 | b1;
      f.mask_pos = (uint32_t)(S ? (mloc ^ (((mloc >> S) & (((uint64_t)1 << (S - 4)) - 1)) << 4)) : mloc);
      if (!(tb & mloc)) {
        f.p0 = (uint32_t)fb.b0;
        f.p1 = (uint32_t)fb.b1;
        cls = FL_GATHER_U;
      } else {
        const bool low_in = (tb & b0) != 0;        // (a gather mask has a bit outside the tile)
        f.p0 = (uint32_t)__builtin_ctz(compress_to_tile(low_in ? b0 : b1, ps));
        f.p1 = (uint32_t)(low_in ? fb.b1 : fb.b0);
        cls = FL_GATHER_B;
      }
    }
    fl[cls].push_back(f);
    skip[idx] = 1;
  };
  for (int idx : ps.tile_masks) add_flip(idx, false);
  for (int idx : ps.gather_masks) add_flip(idx, true);
  // the diagonal as the exchanges leave it: per bond that runs as an exchange (in whichever local pass) the ZZ term on
  // its pair loses a = c / 2 (an isotropic bond's is gone), and -a joins the constant
  const RowMask *dm = diagonal_mask(op);
  std::vector<RowTerm> dterms;
  if (dm) dterms = dm->terms;
  double dconst = 0.0;
  bool diag_changed = false;
  if (ps.has_diag)
    for (size_t idx = 0; idx < bonds.size(); ++idx) {
      if (!bonds[idx].exch) continue;
      const double a = 0.5 * bonds[idx].c;
      const uint64_t pair = op.masks[idx].mask;
      auto it = std::find_if(dterms.begin(), dterms.end(), [&](const RowTerm &t) { return t.sign == pair; });
      DNM_CHECK(it != dterms.end(), "internal: an exchange without a ZZ term on its pair");
      if (it->coeff == a) dterms.erase(it);
      else it->coeff -= a;
      dconst -= a;
      diag_changed = true;
    }
  if (!diag_changed && std::find(skip.begin(), skip.end(), 1) == skip.end()) return 0;      // the pass stays as it is
  std::unique_ptr<PassRecords> r(new PassRecords());
  r->is_reduced = true;
  r->desc = d;            // the geometry (and need_tile) of the whole pass
  DNM_TRY(emit_records(A, ps, *r, dm ? &dterms : nullptr, skip));
  // (what decide_flip_bonds relies on: the reduced pass needs no other kernel instance than the flip-flop one)
  DNM_CHECK(r->tabs.empty() && r->desc.gbucket[MAXR] == r->desc.gbucket[0],
            "internal: the flip-flop form of a pass has table records or grouped diagonal terms");
  for (int c = 0; c < FL_COUNT; ++c) {
    r->flip.loop[c] = (uint32_t)r->flips.size();
    r->flips.insert(r->flips.end(), fl[c].begin(), fl[c].end());
  }
  r->flip.loop[FL_COUNT] = (uint32_t)r->flips.size();
  r->flip.dconst = dconst;
  out->reduced = std::move(r);
  return 0;
}

// The diagonal of a pass as tables (plan.h: DevPass::dblock), derived from the records the kernel would read otherwise --
// the dext list, the bucket lists, the in-tile table and the constant of the flip-flop form -- once the pass has its final
// form (after build_flip_pass).  Built where the in-tile table is, the pass has neither grouped diagonal terms nor table
// records (those run on the kernel instance that keeps the lists), its gathers are early, the terms of the bucket lists have at most MAXDSEL
// distinct outside parts and the pass no more than 2^MAXDBLOCK_BITS workgroups; DNM_DIAG_BLOCK_TABLE=0: never.  Changes
// nothing that dnm_mat_export_pass / _dtile / _flip_pass hand out.
int build_diag_tables(const dnm_mat &A, PassOnDevice *out) {
  PassRecords &r = out->runs();
  DevPass &d = r.desc;
  const char *e = knob("DNM_DIAG_BLOCK_TABLE");
  // (the kernel instances that read the tables: early gathers, not real-packed)
  if (!d.has_diag || (e && e[0] == '0') || r.dtile.empty() || A.op.packed || !(d.cache_policy & 32)) return 0;
  if (!r.tabs.empty() || d.gbucket[MAXR] > d.gbucket[0]) return 0;
  const int B = d.tile_bits, R = 1 << d.log_rows, nbb = d.n_eff - B;
  if (nbb < 0 || nbb > MAXDBLOCK_BITS) return 0;
  // the distinct outside parts of the terms that see the tile and bits outside it
  std::vector<uint64_t> sel;
  for (uint32_t q = d.dbucket[0]; q < d.dbucket[R]; ++q)
    for (uint32_t j = 0; j < r.quads[q].nslots; ++j) {
      const uint64_t m = r.quads[q].sign_ext[j];
      if (m && std::find(sel.begin(), sel.end(), m) == sel.end()) sel.push_back(m);
    }
  if ((int)sel.size() > MAXDSEL) return 0;
  // per workgroup: the terms outside the tile at sign_base | deposit(b), as the kernel forms the block part of a row
  r.dblock.resize((size_t)1 << nbb);
  for (uint32_t b = 0; b < ((uint32_t)1 << nbb); ++b) {
    uint64_t base = 0;
    for (int j = 0; j < d.nbseg; ++j)
      base |= (uint64_t)((b >> d.bseg_off[j]) & ((1u << d.bseg_len[j]) - 1u)) << d.bseg_pos[j];
    const uint64_t sbase = d.sign_base | base;
    double v = r.is_reduced ? r.flip.dconst : 0.0;
    for (uint32_t q = d.dext_begin; q < d.dext_end; ++q)
      for (uint32_t j = 0; j < r.quads[q].nslots; ++j)
        v += parity64(sbase & r.quads[q].sign_ext[j]) ? -r.quads[q].coeff[j] : r.quads[q].coeff[j];
    r.dblock[b] = v;
  }
  // per tile coordinate: one section per combination of the outside parities
  d.dsel_n = (uint32_t)sel.size();
  for (size_t i = 0; i < sel.size(); ++i) d.dsel_mask[i] = sel[i];
  if (!sel.empty()) {
    const size_t T = (size_t)1 << B;
    r.dsect.resize(T << sel.size());
    for (size_t s = 0; s < ((size_t)1 << sel.size()); ++s) {
      double *sec = r.dsect.data() + s * T;
      std::copy(r.dtile.begin(), r.dtile.end(), sec);
      for (uint32_t q = d.dbucket[0]; q < d.dbucket[R]; ++q)
        for (uint32_t j = 0; j < r.quads[q].nslots; ++j) {
          const DevQuad &Q = r.quads[q];
          uint32_t po = 0;      // the parity of the term's outside part in this section
          for (size_t i = 0; i < sel.size(); ++i)
            if (sel[i] == Q.sign_ext[j]) po = (uint32_t)(s >> i) & 1u;
          for (uint32_t tc = 0; tc < (uint32_t)T; ++tc)
            sec[tc] += ((__builtin_popcount(tc & Q.sign_tile[j]) ^ po) & 1) ? -Q.coeff[j] : Q.coeff[j];
        }
    }
  }
  return 0;
}

}  // namespace dnm
