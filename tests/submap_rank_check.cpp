// The index arithmetic of the subspace maps (dynamite_amd/csrc/submap_rank.h, on subspace.h, pm_rank.h and perm_rank.h:
// the header the kernel and dnm_subspace_map_indices include) as a plain C++ program for AddressSanitizer and
// UndefinedBehaviorSanitizer: no HIP runtime, no library, nothing loaded into Python (tests/test_submap_rank_host.py
// builds and runs it).  A subspace is written out here as the list of its configurations in index order, found by a
// loop over all 2^L of them, and a configuration is looked up in a std::map; every target row of every case is then
// compared with the table of the four (source, target) cases spelled out in expected() below.  The binomial tables,
// the Explicit tables and the bucket table have exactly the sizes the kernel is handed.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../dynamite_amd/csrc/submap_rank.h"

using dnm::SubView;

// a subspace spelled out, with the tables a descriptor of it carries
struct Space {
  int type = 0, L = 0, space = 0, k = 0, swz = 0;
  std::vector<int64_t> configs;                 // index -> configuration
  std::map<int64_t, int64_t> index;             // configuration -> index
  std::vector<int64_t> nck, rstates, rind, bucket;
  int bucket_shift = 0;
  std::string name;

  void finish() {
    for (size_t i = 0; i < configs.size(); ++i) index[configs[i]] = (int64_t)i;
  }
  SubView view() const {
    SubView v{};
    v.type = type;
    v.L = L;
    v.space = space;
    v.k = k;
    v.ld = L + 1;
    v.dim = (int64_t)configs.size();
    v.nchoosek = nck.empty() ? nullptr : nck.data();
    if (type == DNM_EXPLICIT) {
      v.state_map = configs.data();
      v.rmap_states = rstates.data();
      v.rmap_indices = rind.empty() ? nullptr : rind.data();
      v.bucket = bucket.empty() ? nullptr : bucket.data();
      v.bucket_shift = bucket_shift;
    }
    v.swz = swz;
    return v;
  }
};

static Space closed_form(int type, int L, int par_or_k, int swz = 0) {
  Space s;
  s.type = type;
  s.L = L;
  s.swz = swz;
  if (type == DNM_PARITY) s.space = par_or_k;
  if (type == DNM_SPIN_CONSERVE) {
    s.k = par_or_k;
    s.nck.resize((size_t)(s.k + 1) * (L + 1));           // exactly the table of the descriptor
    dnm::pm_binomials(L, s.k, L + 1, s.nck.data());
  }
  for (int64_t c = 0; c < ((int64_t)1 << L); ++c) {
    const int pc = __builtin_popcountll((uint64_t)c);
    if (type == DNM_PARITY && (pc & 1) != par_or_k) continue;
    if (type == DNM_SPIN_CONSERVE && pc != par_or_k) continue;
    s.configs.push_back(c);
  }
  char buf[64];
  snprintf(buf, sizeof buf, "%s(%d%s%d)%s", type == DNM_FULL ? "Full" : type == DNM_PARITY ? "Parity" : "SpinConserve",
           L, type == DNM_FULL ? "; " : ", ", par_or_k, swz ? " swizzled" : "");
  s.name = buf;
  s.finish();
  return s;
}

static uint64_t lcg(uint64_t *s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return *s >> 33;
}

// n distinct states of L spins in a seeded, unsorted order; with_bucket: the bucket table over the sorted list
static Space listed(int L, int n, bool with_bucket) {
  Space s;
  s.type = DNM_EXPLICIT;
  s.L = L;
  uint64_t seed = 12345;
  std::map<int64_t, int> seen;
  while ((int)s.configs.size() < n) {
    const int64_t c = (int64_t)(lcg(&seed) % ((uint64_t)1 << L));
    if (seen.count(c)) continue;
    seen[c] = 1;
    s.configs.push_back(c);
  }
  s.finish();
  for (const auto &kv : s.index) {            // (a std::map walks its keys in ascending order)
    s.rstates.push_back(kv.first);
    s.rind.push_back(kv.second);
  }
  if (with_bucket) {
    const int tb = 6;
    s.bucket_shift = L - tb;
    s.bucket.assign(((size_t)1 << tb) + 1, 0);
    for (int64_t st : s.rstates) ++s.bucket[(size_t)(st >> s.bucket_shift) + 1];
    for (size_t b = 0; b + 1 < s.bucket.size(); ++b) s.bucket[b + 1] += s.bucket[b];
  }
  s.name = with_bucket ? "Explicit(40 of 10, buckets)" : "Explicit(40 of 10)";
  return s;
}

static int64_t pos_of(const Space &s, int64_t i) {
  return (s.type == DNM_FULL || s.type == DNM_PARITY) ? dnm::vec_pos(i, s.swz) : i;
}

// psi(c) of the source in units of its scale: the position of the amplitude and its sign, or (-1, 0)
static void amplitude(const Space &s, int sec, int64_t c, int64_t *at, int *sign) {
  *at = -1;
  *sign = 0;
  int sg = 1;
  if (sec && ((c >> (s.L - 1)) & 1)) {
    c ^= ((int64_t)1 << s.L) - 1;
    sg = sec;
  }
  const auto it = s.index.find(c);
  if (it == s.index.end()) return;
  if (sec && it->second >= (int64_t)s.configs.size() / 2) return;
  *at = pos_of(s, it->second);
  *sign = sg;
}

// the table of the four cases for the target row of configuration c
static void expected(const Space &src, int ssec, int dsec, int64_t c, int64_t at[2], int sign[2]) {
  at[0] = at[1] = -1;
  sign[0] = sign[1] = 0;
  if (ssec && dsec) {
    if (ssec == dsec) amplitude(src, ssec, c, &at[0], &sign[0]);
    if (sign[0]) sign[0] = 1;
  } else if (ssec) {
    amplitude(src, ssec, c, &at[0], &sign[0]);
  } else if (dsec) {
    amplitude(src, 0, c, &at[0], &sign[0]);
    amplitude(src, 0, c ^ (((int64_t)1 << src.L) - 1), &at[1], &sign[1]);
    sign[1] *= dsec;
  } else {
    amplitude(src, 0, c, &at[0], &sign[0]);
  }
}

static dnm::SubmapSide side_of(const Space &s, int sec) {
  dnm::SubmapSide d{};
  d.v = s.view();
  d.xsec = sec;
  d.dim = (int64_t)s.configs.size();
  d.closed = s.type == DNM_FULL || (s.type == DNM_PARITY && s.L % 2 == 0) ||
             (s.type == DNM_SPIN_CONSERVE && s.L == 2 * s.k);
  d.rows = sec ? d.dim / 2 : d.dim;
  return d;
}

template <int ST, int DT>
static int walk(const Space &src, int ssec, const Space &dst, int dsec, int64_t *found) {
  int failures = 0;
  const dnm::SubmapSide s = side_of(src, ssec), d = side_of(dst, dsec);
  for (int64_t row = 0; row < d.rows; ++row) {
    const int64_t want_c = dst.configs[(size_t)pos_of(dst, row)];
    const uint64_t c = dnm::submap_row_config<DT>(row, d.v);
    int64_t at[2];
    int sign[2];
    expected(src, ssec, dsec, want_c, at, sign);
    dnm::SubmapTerms t;
    dnm::submap_terms<ST>(c, s, dsec, &t);
    bool bad = (int64_t)c != want_c;
    for (int m = 0; m < 2; ++m) {
      bad = bad || t.idx[m] != at[m] || t.sign[m] != sign[m] || t.idx[m] < -1 || t.idx[m] >= s.rows;
      *found += t.idx[m] >= 0;
    }
    if (bad && ++failures < 5)
      printf("  row %lld: configuration %llx (want %llx), terms (%lld, %d) (%lld, %d), want (%lld, %d) (%lld, %d)\n",
             (long long)row, (unsigned long long)c, (unsigned long long)want_c, (long long)t.idx[0], t.sign[0],
             (long long)t.idx[1], t.sign[1], (long long)at[0], sign[0], (long long)at[1], sign[1]);
  }
  return failures;
}

static int check(const Space &src, int ssec, const Space &dst, int dsec, int64_t want_found = -2) {
  int64_t found = 0;
  const int failures = [&] {
    auto with_dst = [&](auto S) {
      constexpr int ST = decltype(S)::value;
      switch (dst.type) {
        case DNM_FULL: return walk<ST, DNM_FULL>(src, ssec, dst, dsec, &found);
        case DNM_PARITY: return walk<ST, DNM_PARITY>(src, ssec, dst, dsec, &found);
        case DNM_EXPLICIT: return walk<ST, DNM_EXPLICIT>(src, ssec, dst, dsec, &found);
        default: return walk<ST, DNM_SPIN_CONSERVE>(src, ssec, dst, dsec, &found);
      }
    };
    switch (src.type) {
      case DNM_FULL: return with_dst(std::integral_constant<int, DNM_FULL>{});
      case DNM_PARITY: return with_dst(std::integral_constant<int, DNM_PARITY>{});
      case DNM_EXPLICIT: return with_dst(std::integral_constant<int, DNM_EXPLICIT>{});
      default: return with_dst(std::integral_constant<int, DNM_SPIN_CONSERVE>{});
    }
  }();
  const bool count_bad = want_found != -2 && found != want_found;
  printf("%s sector %d -> %s sector %d: %lld terms: %s\n", src.name.c_str(), ssec, dst.name.c_str(), dsec,
         (long long)found, failures || count_bad ? "FAILED" : "ok");
  return failures + count_bad;
}

// one set bit at 63 spins: SpinConserve(63, 1) and Parity(63, odd), whose rows cannot all be walked
static int check_63() {
  const int L = 63;
  int failures = 0;
  std::vector<int64_t> nck((size_t)2 * (L + 1));
  dnm::pm_binomials(L, 1, L + 1, nck.data());
  dnm::SubmapSide sc{}, par{};
  sc.v.type = DNM_SPIN_CONSERVE;
  sc.v.L = L;
  sc.v.k = 1;
  sc.v.ld = L + 1;
  sc.v.nchoosek = nck.data();
  sc.dim = sc.rows = L;
  par.v.type = DNM_PARITY;
  par.v.L = L;
  par.v.space = 1;
  par.dim = par.rows = (int64_t)1 << (L - 1);
  for (int j = 0; j < L; ++j) {
    const uint64_t c = (uint64_t)1 << j;
    dnm::SubmapTerms t;
    // target SpinConserve row j from the Parity source, and from itself
    failures += dnm::submap_row_config<DNM_SPIN_CONSERVE>(j, sc.v) != c;
    dnm::submap_terms<DNM_PARITY>(c, par, 0, &t);
    failures += t.idx[0] != (int64_t)(c >> 1) || t.sign[0] != 1 || t.idx[1] != -1 || t.sign[1] != 0;
    dnm::submap_terms<DNM_SPIN_CONSERVE>(c, sc, 0, &t);
    failures += t.idx[0] != j || t.sign[0] != 1;
    // target Parity row of that configuration from the SpinConserve source
    failures += dnm::submap_row_config<DNM_PARITY>((int64_t)(c >> 1), par.v) != c;
  }
  for (int64_t row : {(int64_t)3, (int64_t)5, ((int64_t)1 << 61) + 1, ((int64_t)1 << 62) - 1}) {      // more than one set bit
    dnm::SubmapTerms t;
    dnm::submap_terms<DNM_SPIN_CONSERVE>(dnm::submap_row_config<DNM_PARITY>(row, par.v), sc, 0, &t);
    failures += t.idx[0] != -1 || t.sign[0] != 0 || t.idx[1] != -1;
  }
  printf("SpinConserve(63, 1) <-> Parity(63, odd): %s\n", failures ? "FAILED" : "ok");
  return failures;
}

int main() {
  int failures = 0;
  const Space sc126 = closed_form(DNM_SPIN_CONSERVE, 12, 6), sc125 = closed_form(DNM_SPIN_CONSERVE, 12, 5);
  const Space full12 = closed_form(DNM_FULL, 12, 0), full12s = closed_form(DNM_FULL, 12, 0, 5);
  const Space full11 = closed_form(DNM_FULL, 11, 0), full11s = closed_form(DNM_FULL, 11, 0, 5);
  const Space par11 = closed_form(DNM_PARITY, 11, 1), par11s = closed_form(DNM_PARITY, 11, 1, 5);
  const Space par12 = closed_form(DNM_PARITY, 12, 0);
  const Space full10 = closed_form(DNM_FULL, 10, 0), sc103 = closed_form(DNM_SPIN_CONSERVE, 10, 3);
  const Space sc104 = closed_form(DNM_SPIN_CONSERVE, 10, 4);
  const Space ex = listed(10, 40, false), exb = listed(10, 40, true);
  // SpinConserve(12, 6) -> Full(12), and both XParity sectors of the source
  failures += check(sc126, 0, full12, 0, 924);
  failures += check(sc126, +1, full12, 0, 924);
  failures += check(sc126, -1, full12, 0, 924);
  failures += check(sc126, 0, full12s, 0, 924);
  // Full(12) -> SpinConserve(12, 6), and both XParity sectors of the target
  failures += check(full12, 0, sc126, 0, 924);
  failures += check(full12, 0, sc126, +1, 924);
  failures += check(full12, 0, sc126, -1, 924);
  failures += check(full12s, 0, sc126, -1, 924);
  // sector to sector, equal and different
  failures += check(sc126, +1, full12, +1, 462);
  failures += check(sc126, +1, full12, -1, 0);
  failures += check(full12, -1, sc126, -1, 462);
  // a sector that is not closed under the flip: the complement is looked up, not mirrored
  failures += check(sc125, 0, full12, 0, 792);
  failures += check(sc125, 0, full12, +1, 792);
  // Parity(11 odd) <-> Full(11), swizzled on either side
  failures += check(par11, 0, full11, 0, 1024);
  failures += check(full11, 0, par11, 0, 1024);
  failures += check(par11s, 0, full11s, 0, 1024);
  failures += check(full11s, 0, par11s, 0, 1024);
  failures += check(par11, 0, full11, -1, 1024);
  // Parity(12 even) <-> SpinConserve(12, 6)
  failures += check(par12, 0, sc126, 0, 924);
  failures += check(sc126, 0, par12, 0, 924);
  failures += check(par12, +1, sc126, 0, 924);
  failures += check(sc126, 0, par12, -1, 924);
  // an unsorted Explicit list of 40 states of 10 spins <-> Full(10), with and without the bucket table
  failures += check(ex, 0, full10, 0, 40);
  failures += check(full10, 0, ex, 0, 40);
  failures += check(exb, 0, full10, 0, 40);
  failures += check(exb, 0, full10, +1, 40);
  failures += check(exb, 0, ex, 0, 40);
  failures += check(sc104, 0, exb, 0);
  failures += check(exb, 0, sc104, 0);
  // disjoint sectors: all -1
  failures += check(sc103, 0, sc104, 0, 0);
  failures += check_63();
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
