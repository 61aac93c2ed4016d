// layout_roundtrip.cc -- the host-side layout planner (csrc/gmg_layout.hpp) without a GPU: every plan is decoded back to
// (row, column, value) triples by the addressing rules of the kernels, restated here, and must give back the CSR it was
// planned from, entry for entry in stored order, values compared as bit patterns.  Explicit +0.0 entries carry no
// information in a product (x is finite) and are what the layouts pad with: they are dropped on both sides where a layout
// may have inserted them.  Every case also asserts the layout it was written for: a fall-back to CSR is a failure.
// Cases: the SELL variants, the other SELL cases, the hybrid layout, operators cut into the row chunks of 2 - 4 ranks, invalid
// input, host threads, and -- limit_cases() -- a pair of operators on either side of every integer limit of the planner.
// Driven by tests/test_operator_layout_cpu.py; exit status 0 = every requirement held.
#include "gmg_layout.hpp"

#include <cmath>
#include <cstdlib>
#include <string>
#include <utility>

using namespace gmg;

namespace {

int g_failures = 0;
std::string g_case;
#define REQUIRE(cond)                                                                                    \
  do {                                                                                                   \
    if (!(cond) && ++g_failures <= 20) std::fprintf(stderr, "FAIL [%s] line %d: %s\n", g_case.c_str(), __LINE__, #cond); \
  } while (0)

uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
  double real() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }  // all distinct in practice
};

struct Csr {
  int64_t n_rows = 0, n_cols = 0;
  std::vector<int64_t> rp = {0};
  std::vector<int32_t> col;
  std::vector<double> val;
  void add_row(const std::vector<int32_t> &c, const std::vector<double> &v) {
    col.insert(col.end(), c.begin(), c.end());
    val.insert(val.end(), v.begin(), v.end());
    rp.push_back((int64_t)col.size());
    ++n_rows;
  }
  CsrView view() const { return CsrView{n_rows, n_cols, rp.data(), col.data(), val.data()}; }
};

using Entry = std::pair<int32_t, uint64_t>;  // column, value bits

std::vector<Entry> without_zeros(const std::vector<Entry> &e) {
  std::vector<Entry> out;
  for (const Entry &x : e)
    if (x.second != 0) out.push_back(x);
  return out;
}
std::vector<Entry> csr_row(const CsrView &A, int64_t r) {
  std::vector<Entry> e;
  for (int64_t k = A.rowptr[r]; k < A.rowptr[r + 1]; ++k) e.emplace_back(A.col[k], bits_of(A.val[k]));
  return e;
}

// ---- spmv_sell_kernel / spmv_hybrid_kernel: slice sl holds quads [qptr[sl], qptr[sl + 1]); entry j of lane `lane` sits in
// quad q = qptr[sl] + j / 4 at e = j % 4: its 8-bit code at (q * 64 + lane) * 4 + e, its double at
// ((2 q + e / 2) * 64 + lane) * 2 + e % 2; its column is row + pat[pid * 32 + j] in a pattern slice, otherwise the 32-bit
// column or base[sl] + the 16-bit offset at (q * 64 + lane) * 4 + e.
struct StreamsView {
  const std::vector<int32_t> &qptr, &spat, &pat;
  const std::vector<double> &dict;
  const SellStreams &s;
  const int32_t *base;  // per slice (16-bit columns only)
};
std::vector<Entry> decode_lane(const StreamsView &V, int64_t sl, int lane) {
  std::vector<Entry> e;
  const int64_t q0 = V.qptr[(size_t)sl], nq = V.qptr[(size_t)sl + 1] - q0, row = sl * 64 + lane;
  const int pid = V.spat[(size_t)sl];
  for (int64_t j = 0; j < 4 * nq; ++j) {
    const int64_t q = q0 + j / 4, en = j % 4;
    const size_t oc = (size_t)((q * 64 + lane) * 4 + en), ov = (size_t)(((2 * q + en / 2) * 64 + lane) * 2 + en % 2);
    const double v = V.s.val8 ? V.dict[V.s.v1[oc]] : V.s.v2[ov];
    int32_t c;
    if (pid >= 0) c = (int32_t)(row + V.pat[(size_t)pid * 32 + (size_t)j]);
    else c = V.s.col16 ? V.base[sl] + (int32_t)V.s.c2[oc] : V.s.c4[oc];
    e.emplace_back(c, bits_of(v));
  }
  return e;
}
// a decoded slice against the CSR: a plain slice holds the row's entries as they are, then +0.0 padding; a pattern slice the
// row's entries with +0.0 in between.  Every column, padding included, is gathered: it must be a valid one.
void check_slice(const CsrView &A, const StreamsView &V, int64_t sl) {
  REQUIRE(V.spat[(size_t)sl] < 0 || sl * 64 + 64 <= A.n_rows);
  for (int lane = 0; lane < 64; ++lane) {
    const int64_t r = sl * 64 + lane;
    const std::vector<Entry> got = decode_lane(V, sl, lane), want = r < A.n_rows ? csr_row(A, r) : std::vector<Entry>();
    bool ok = got.size() >= want.size();
    for (const Entry &x : got) ok = ok && x.first >= 0 && x.first < A.n_cols;
    if (V.spat[(size_t)sl] >= 0) ok = ok && without_zeros(got) == without_zeros(want);
    else {
      for (size_t j = 0; ok && j < got.size(); ++j) ok = j < want.size() ? got[j] == want[j] : got[j].second == 0;
    }
    REQUIRE(ok);
    if (!ok) return;
  }
}

void check_tiles(const std::vector<int32_t> &t, int64_t n_rows, const int64_t *rp) {
  REQUIRE(!t.empty() && t.front() == 0 && t.back() == n_rows);
  for (size_t i = 0; i + 1 < t.size(); ++i) {
    REQUIRE(t[i] < t[i + 1]);
    // more than one row: the window from the start rounded down to 4 holds them all
    REQUIRE(t[i + 1] - t[i] == 1 || (rp[t[i + 1]] - (rp[t[i]] & ~(int64_t)3) <= kTileNnz && t[i + 1] - t[i] <= kTileMaxRowsEarly));
  }
}

void check_sell(const CsrView &A, const SellPlan &s) {
  REQUIRE((int64_t)s.slice_ptr.size() == A.n_slices() + 1 && s.slice_ptr.back() == s.quads);
  const StreamsView V{s.slice_ptr, s.pat.spat, s.pat.table, s.vd.dict, s.s, s.slice_base.data()};
  for (int64_t sl = 0; sl < A.n_slices(); ++sl) check_slice(A, V, sl);
}

// ---- spmv_sellp_kernel: wave w serves slices [wave_ptr[w], wave_ptr[w + 1]) (flags masked off); a strided fast wave serves
// the pairs of slices first + k stride, k < pairs, and `extra` if >= 0.  In a fast wave, entry j < 27 of a row is
// ctab[rowcls[row] * 27 + j] at column row + pattern[j].
void check_sellp(const CsrView &A, const SellPlan &s, const SellpPlan &w) {
  const int n_waves = (int)w.wave_ptr.size() - 1;
  REQUIRE(n_waves == s.sell_grid * 4);
  std::vector<int> served((size_t)s.n_slices, 0);
  const auto &pattern = s.pat.list[(size_t)s.sellp_pid];
  auto fast_slice = [&](int64_t sl) {
    REQUIRE(sl >= 0 && sl < s.n_slices && s.pat.spat[(size_t)sl] == s.sellp_pid);
    for (int lane = 0; lane < 64; ++lane) {
      std::vector<Entry> got;
      const int64_t r = sl * 64 + lane;
      for (int j = 0; j < 27; ++j) got.emplace_back((int32_t)(r + pattern[(size_t)j]), bits_of(w.ctab[(size_t)w.rowcls[(size_t)r] * 27 + (size_t)j]));
      REQUIRE(w.rowcls[(size_t)r] < w.n_classes && without_zeros(got) == without_zeros(csr_row(A, r)));
    }
  };
  for (int wv = 0; wv < n_waves; ++wv) {
    const int32_t e0 = w.wave_ptr[(size_t)wv], s0 = e0 & (kSellpStrided - 1), s1 = w.wave_ptr[(size_t)wv + 1] & (kSellpStrided - 1);
    REQUIRE(s0 <= s1 && s1 - s0 <= 64);
    if (!(e0 & kSellpFastWave)) {
      REQUIRE(!(e0 & kSellpStrided));
      for (int32_t sl = s0; sl < s1; ++sl) ++served[(size_t)sl];  // (served from the streams: check_sell)
      continue;
    }
    REQUIRE(w.rowclass);
    WaveRR d{s0, 2, (s1 - s0) / 2, ((s1 - s0) & 1) ? s1 - 1 : -1};
    if (e0 & kSellpStrided) { REQUIRE(!w.wave_rr.empty()); d = w.wave_rr[(size_t)wv]; }
    for (int k = 0; k < d.pairs; ++k)
      for (int h = 0; h < 2; ++h) { fast_slice(d.first + k * d.stride + h); ++served[(size_t)(d.first + k * d.stride + h)]; }
    if (d.extra >= 0) { fast_slice(d.extra); ++served[(size_t)d.extra]; }
  }
  REQUIRE(w.wave_ptr.front() == 0 && (w.wave_ptr.back() & (kSellpStrided - 1)) == s.n_slices);
  for (int64_t sl = 0; sl < s.n_slices; ++sl) REQUIRE(served[(size_t)sl] == 1);
}

// ---- spmv_lattice_kernel: rows R0 + k nxy + [0, W), k < K, below R1, take entry pos = (dz + 1) * 9 + (dy + 1) * 3 + dx + 1
// from ctab[rowcls[row] * 27 + pos] at column row + dz nxy + dy nx + dx; every slice with another row is in `gen` and is
// served from the SELL streams.
void check_lattice(const CsrView &A, const SellPlan &s, const LatticePlan &L) {
  const int64_t reach = L.nxy + L.nx + 1;
  REQUIRE(L.R0 - 2 - reach >= 0 && L.R1 + reach <= A.n_rows);  // the marching waves' reads, two rows beyond either end
  REQUIRE(L.C == (L.W + kLatRowsPerUnit - 1) / kLatRowsPerUnit && L.classes <= kLatMaxClasses && L.grid <= kMaxPartials);
  int64_t n_fast = 0;
  std::vector<char> in_gen((size_t)s.n_slices, 0);
  for (int32_t sl : L.gen) in_gen[(size_t)sl] = 1;
  for (int64_t r = 0; r < A.n_rows; ++r) {
    const bool fast = r >= L.R0 && r < L.R1 && (r - L.R0) % L.nxy < L.W && (r - L.R0) / L.nxy < L.K;
    REQUIRE(fast || in_gen[(size_t)(r / 64)]);  // every row is served by one of the two
    if (!fast) continue;
    ++n_fast;
    std::vector<Entry> got;
    bool inside = true;
    for (int pos = 0; pos < 27; ++pos) {
      const int64_t c = r + (pos / 9 - 1) * L.nxy + (pos / 3 % 3 - 1) * L.nx + (pos % 3 - 1);
      inside = inside && c >= 0 && c < A.n_rows;
      got.emplace_back((int32_t)c, bits_of(L.ctab[(size_t)L.rowcls[(size_t)r] * 27 + (size_t)pos]));
    }
    REQUIRE(inside && L.rowcls[(size_t)r] < L.classes && without_zeros(got) == without_zeros(csr_row(A, r)));
  }
  REQUIRE(n_fast == L.fast_rows);
}

// ---- spmv_hybrid_kernel: the regular slices from streams of their own (32-bit columns), the rows of the other slices from
// the CSR copy, tile by tile
void check_hybrid(const CsrView &A, const HybridPlan &H) {
  const StreamsView V{H.qptr, H.pat.spat, H.pat.table, H.vd.dict, H.s, nullptr};
  REQUIRE(!H.s.col16 && (int64_t)H.qptr.size() == A.n_slices() + 1 && H.n_tiles * 2 == (int)H.tiles.size());
  std::vector<int> served((size_t)A.n_rows, 0);
  for (int32_t sl : H.reg) {
    check_slice(A, V, sl);
    for (int64_t r = (int64_t)sl * 64; r < A.slice_end(sl); ++r) ++served[(size_t)r];
  }
  int32_t last_end = 0;
  for (size_t t = 0; t < H.tiles.size(); t += 2) {
    const int32_t b = H.tiles[t], e = H.tiles[t + 1];
    REQUIRE(b >= last_end && b < e && e <= A.n_rows);
    REQUIRE(e - b == 1 || A.rowptr[e] - (A.rowptr[b] & ~(int64_t)3) <= kTileNnz);
    for (int32_t r = b; r < e; ++r) ++served[(size_t)r];
    last_end = e;
  }
  for (int64_t r = 0; r < A.n_rows; ++r) REQUIRE(served[(size_t)r] == 1);
  for (int64_t sl = 0; sl < A.n_slices(); ++sl)  // a slice outside the regular ones has no quads
    REQUIRE(std::binary_search(H.reg.begin(), H.reg.end(), (int32_t)sl) || H.qptr[(size_t)sl + 1] == H.qptr[(size_t)sl]);
}

// plan an operator and check whatever was built; the caller asserts the flags it expects
StreamPlan plan_and_check(const Csr &m, const LayoutOptions &opt, bool allow_hybrid = false) {
  const CsrView A = m.view();
  REQUIRE(check_csr(A) == nullptr);
  const TilePlan T = plan_tiles(A.rowptr, A.n_rows);
  check_tiles(T.tile_row, A.n_rows, A.rowptr);
  REQUIRE(T.n_tiles == (int)T.tile_row.size() - 1 && T.grid % 8 == 0 && T.grid >= 8 && T.grid <= kMaxPartials);
  PhaseLog quiet;
  StreamPlan P = plan_streams(A, opt, allow_hybrid, quiet);
  REQUIRE(!(P.sell.built && P.hyb.built));
  if (P.sell.built) check_sell(A, P.sell);
  if (P.sell.built && P.sell.use_sellp) check_sellp(A, P.sell, P.sellp);
  if (P.lat.built) check_lattice(A, P.sell, P.lat);
  if (P.hyb.built) check_hybrid(A, P.hyb);
  return P;
}

// ---------------------------------------------------------------- operators (the rules of the GPU tests' generators)

const double kFive[5] = {-1.0 / 6, -1.0 / 12, 8.0 / 3, 0.0, 1.25};

// tests/test_gpu_layouts.py banded(): `width` columns `spread` apart around the diagonal, clipped to [0, n) (rows at the ends
// are shorter); values from kFive (few) or all distinct; n_classes > 0: full rows take one of that many coefficient vectors.
// ghost > 0: the operator is the first n rows of one with n + ghost rows (columns >= n are ghost columns).
Csr banded(int64_t n, int width, uint64_t seed, bool few, int64_t spread = 1, int n_classes = 0, int64_t ghost = 0) {
  Rng rng{seed};
  Csr m;
  m.n_cols = n + ghost;
  std::vector<std::vector<double>> vectors((size_t)n_classes, std::vector<double>((size_t)width));
  for (auto &v : vectors)
    for (double &x : v) x = kFive[rng.below(5)];
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> c;
    for (int k = 0; k < width; ++k) c.push_back((int32_t)std::min(n + ghost - 1, std::max<int64_t>(0, i + spread * (k - width / 2))));
    c.push_back((int32_t)i);
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    std::vector<double> v(c.size());
    if (n_classes && (int)c.size() == width) v = vectors[(size_t)((i * 7 + i / 64) % n_classes)];
    else for (double &x : v) x = few ? kFive[rng.below(5)] : rng.real();
    double &diag = v[(size_t)(std::lower_bound(c.begin(), c.end(), (int32_t)i) - c.begin())];
    diag = 4.0 + std::fabs(diag);
    m.add_row(c, v);
  }
  return m;
}

// 11 full-width rows whose columns wrap around: every slice spans more than 65535 columns without the short rows of a
// clipped band (which would cost the SELL layout its 12 % padding bound at this size)
Csr wide_columns(int64_t n, uint64_t seed) {
  Rng rng{seed};
  Csr m;
  m.n_cols = n;
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> c;
    for (int k = 0; k < 11; ++k) c.push_back((int32_t)(((i + 6600 * (k - 5)) % n + n) % n));
    std::sort(c.begin(), c.end());
    std::vector<double> v(c.size());
    for (double &x : v) x = kFive[rng.below(5)];
    m.add_row(c, v);
  }
  return m;
}

// tests/cg_reference.py lattice_operator(): 27-point operator on an nx x ny x nz lattice, lexicographic numbering; rows at
// the boundary store only the neighbours that exist (shorter rows) and are Dirichlet rows (stored zeros off the diagonal)
Csr lattice(int nx, int ny, int nz) {
  const double h = 0.25, by_m[4] = {8.0 / 3.0, 0.0, -1.0 / 6.0, -1.0 / 12.0};
  Csr m;
  m.n_cols = (int64_t)nx * ny * nz;
  auto kind = [&](int x, int y, int z) { return (x == 0) + (x == nx - 1) + (y == 0) + (y == ny - 1) + (z == 0) + (z == nz - 1); };
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        std::vector<int32_t> c;
        std::vector<double> v;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int X = x + dx, Y = y + dy, Z = z + dz;
              if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
              const bool bnd = kind(x, y, z) > 0;
              double w = (bnd || kind(X, Y, Z) > 0) ? 0.0 : h * by_m[std::abs(dz) + std::abs(dy) + std::abs(dx)];
              if (!dx && !dy && !dz) w = bnd ? h * (4.0 / 3.0) / kind(x, y, z) : h * by_m[0];
              c.push_back((int32_t)(((int64_t)Z * ny + Y) * nx + X));
              v.push_back(w);
            }
        m.add_row(c, v);
      }
  return m;
}

// tests/test_gpu_hybrid_spmv.py banded(): 27 entries per row at row + dz * 100 + dy * 10 + dx (clipped at the ends); wide
// rows get 84 entries; odd rows of shifted slices take their last nine columns 200 further out (36 offsets in the slice: no
// column pattern); values from 20 given ones (-0.0 among them) or all distinct
Csr hybrid_band(int64_t n, std::vector<int64_t> wide_rows, std::vector<int64_t> empty_rows, std::vector<int64_t> shifted_slices, bool few_regular, bool few_wide,
                uint64_t seed) {
  const double few[20] = {-0.75, -0.5, -0.25, -0.125, 0.0625, 0.125, 0.25, 0.5, 1.0, 1.5, 2.0, 2.6666666666666665, 1.0 / 3.0, -1.0 / 3.0,
                          1.0 / 6.0, -1.0 / 6.0, 1.0 / 12.0, -1.0 / 12.0, 4.0 / 3.0, -0.0};
  auto has = [](const std::vector<int64_t> &v, int64_t x) { return std::find(v.begin(), v.end(), x) != v.end(); };
  Rng rng{seed};
  Csr m;
  m.n_cols = n;
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> c;
    if (!has(empty_rows, i)) {
      int j = 0;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx, ++j) {
            const int64_t cc = i + dz * 100 + dy * 10 + dx + ((has(shifted_slices, i / 64) && i % 2 && j >= 18) ? 200 : 0);
            if (cc >= 0 && cc < n) c.push_back((int32_t)cc);
          }
      while (has(wide_rows, i) && c.size() < 84) {
        const int32_t extra = (int32_t)rng.below((int)n);
        if (std::find(c.begin(), c.end(), extra) == c.end()) c.push_back(extra);
      }
      std::sort(c.begin(), c.end());
    }
    std::vector<double> v(c.size());
    for (double &x : v) x = (has(wide_rows, i) ? few_wide : few_regular) ? few[rng.below(20)] : rng.real();
    m.add_row(c, v);
  }
  return m;
}

// every host array and scalar of a plan, for the comparison across thread counts
template <class T>
void put(std::vector<uint8_t> &out, const std::vector<T> &v) {
  const uint64_t n = v.size();
  out.insert(out.end(), (const uint8_t *)&n, (const uint8_t *)&n + 8);
  if (n) out.insert(out.end(), (const uint8_t *)v.data(), (const uint8_t *)(v.data() + n));
}
std::vector<uint8_t> plan_bytes(const StreamPlan &P) {
  std::vector<uint8_t> b;
  const SellPlan &s = P.sell;
  put(b, s.slice_ptr); put(b, s.slice_base); put(b, s.pat.spat); put(b, s.pat.table); put(b, s.vd.dict);
  put(b, s.s.v1); put(b, s.s.v2); put(b, s.s.c2); put(b, s.s.c4);
  put(b, P.sellp.wave_ptr); put(b, P.sellp.rowcls); put(b, P.sellp.ctab);
  std::vector<int32_t> rr;
  for (const WaveRR &d : P.sellp.wave_rr) rr.insert(rr.end(), {d.first, d.stride, d.pairs, d.extra});
  put(b, rr);
  put(b, P.lat.rowcls); put(b, P.lat.ctab); put(b, P.lat.gen);
  put(b, std::vector<int64_t>{s.built, s.s.val8, s.s.col16, s.quads, s.sellp_pid, s.use_sellp, s.sell_grid, P.sellp.rowclass, P.sellp.n_classes, P.lat.built,
                              P.lat.nx, P.lat.nxy, P.lat.R0, P.lat.R1, P.lat.W, P.lat.K, P.lat.C, P.lat.S, P.lat.fast_blocks, P.lat.grid, P.lat.classes,
                              P.lat.fast_rows, P.lat.gen_bytes});
  return b;
}

// ---------------------------------------------------------------- cases

void sell_variants() {
  const Csr m = banded(5037, 27, 11, true, 1, 7);  // 27 consecutive columns = nine runs of three = a 3 x 3 x n lattice
  struct Variant { const char *name; void (*set)(LayoutOptions &); bool sellp, rowclass, lattice, strided; };
  const Variant variants[] = {
      {"sell: default", [](LayoutOptions &) {}, true, true, true, false},
      {"sell: disable_sellp", [](LayoutOptions &o) { o.disable_sellp = true; }, false, false, true, false},
      {"sell: disable_rowclass", [](LayoutOptions &o) { o.disable_rowclass = true; }, true, false, true, false},
      {"sell: disable_lattice", [](LayoutOptions &o) { o.disable_lattice = true; }, true, true, false, false},
      {"sell: sellp_rr", [](LayoutOptions &o) { o.sellp_rr = 1; }, true, true, true, false},
      // 32 waves for 79 slices: the fast waves of an XCD own several pairs of slices and are dealt them round-robin
      {"sell: sellp_rr, sell_grid 8", [](LayoutOptions &o) { o.sellp_rr = 1; o.sell_grid = 8; }, true, true, true, true},
  };
  for (const Variant &v : variants) {
    g_case = v.name;
    LayoutOptions opt;
    opt.sellp_cost = 4.0;
    v.set(opt);
    const StreamPlan P = plan_and_check(m, opt);
    REQUIRE(P.sell.built && P.sell.s.val8 && P.sell.s.col16 && P.sell.pat.n_pattern_slices > 0 && P.sell.sellp_pid >= 0);
    REQUIRE(P.sell.use_sellp == v.sellp && P.sellp.rowclass == v.rowclass && P.lat.built == v.lattice);
    REQUIRE((opt.sellp_rr == 1 && v.rowclass) == !P.sellp.wave_rr.empty());
    bool strided = false;
    for (int32_t e : P.sellp.wave_ptr) strided = strided || (e & kSellpStrided);
    REQUIRE(strided == v.strided);
  }
}

void other_sell_cases() {
  LayoutOptions opt;
  opt.sellp_cost = 4.0;
  g_case = "values: more than 256 distinct";
  StreamPlan P = plan_and_check(banded(3000, 27, 12, false), opt);
  REQUIRE(P.sell.built && !P.sell.s.val8 && P.sell.s.col16 && !P.sell.use_sellp && !P.lat.built);
  g_case = "columns: more than 65535 apart in a slice";
  P = plan_and_check(wide_columns(66037, 13), opt);
  REQUIRE(P.sell.built && P.sell.s.val8 && !P.sell.s.col16);
  g_case = "csr: 9 of 12 padded entries";
  P = plan_and_check(banded(3000, 9, 14, false), opt);
  REQUIRE(!P.sell.built && !P.hyb.built);
  g_case = "lattice 37 x 23 x 19";
  P = plan_and_check(lattice(37, 23, 19), opt);
  REQUIRE(P.sell.built && P.sell.s.val8 && P.lat.built && P.lat.nx == 37 && P.lat.nxy == 37 * 23 && P.lat.W == P.lat.nxy && !P.lat.gen.empty());
  g_case = "ghost columns behind the owned ones";
  P = plan_and_check(banded(5037, 27, 15, true, 1, 7, 40), opt);
  REQUIRE(P.sell.built && P.sell.pat.n_pattern_slices > 0 && P.sell.use_sellp && P.lat.built);
}

void hybrid_cases() {
  LayoutOptions opt;
  opt.sellp_cost = 4.0;
  std::vector<int64_t> some_empty = {400, 401, 402, 403}, six_wide;
  for (int64_t r = 640; r < 704; ++r) some_empty.push_back(r);
  for (int64_t r = 3 * 64 + 30; r < 3 * 64 + 36; ++r) six_wide.push_back(r);
  struct Case { const char *name; Csr m; bool val8, streamed; };
  const Case cases[] = {
      {"hybrid: wide row in the middle of slice 3", hybrid_band(1088, {3 * 64 + 32}, {}, {}, true, true, 0), true, false},
      {"hybrid: wide rows in the first and the last slice", hybrid_band(1088, {5, 1088 - 7}, {}, {}, true, true, 0), true, false},
      {"hybrid: partial last slice", hybrid_band(1100, {3 * 64 + 32}, {}, {}, true, true, 0), true, false},
      {"hybrid: empty rows, an empty slice, streamed columns", hybrid_band(1088, {3 * 64 + 32, 9 * 64}, some_empty, {5, 6, 7}, true, true, 0), true, true},
      {"hybrid: > 256 values overall, <= 256 in the regular slices", hybrid_band(1088, six_wide, {}, {}, true, false, 0), true, false},
      {"hybrid: > 256 values in the regular slices", hybrid_band(1088, {3 * 64 + 32}, {}, {6}, false, true, 0), false, true},
  };
  for (const Case &c : cases) {
    g_case = c.name;
    const StreamPlan P = plan_and_check(c.m, opt, true);
    REQUIRE(P.hyb.built && !P.sell.built && P.hyb.vd.val8 == c.val8 && P.hyb.n_tiles > 0 && P.hyb.pat.n_pattern_slices > 0);
    bool streamed = false;
    for (int32_t sl : P.hyb.reg) streamed = streamed || P.hyb.pat.spat[(size_t)sl] < 0;
    REQUIRE(streamed == c.streamed);
    REQUIRE(!plan_and_check(c.m, opt, false).hyb.built);  // only where the caller allows it
  }
}

// tests/partition_reference.py localize(): the rows [begin, end) of a square operator with the columns renumbered [owned |
// ghosts], the ghosts in ascending global order behind the owned ones.  A row keeps its stored order, so a row that refers
// to a lower rank has local columns that are not ascending.
Csr localize(const Csr &g, int64_t begin, int64_t end) {
  std::vector<int32_t> ghosts;
  for (int64_t k = g.rp[(size_t)begin]; k < g.rp[(size_t)end]; ++k)
    if (g.col[(size_t)k] < begin || g.col[(size_t)k] >= end) ghosts.push_back(g.col[(size_t)k]);
  std::sort(ghosts.begin(), ghosts.end());
  ghosts.erase(std::unique(ghosts.begin(), ghosts.end()), ghosts.end());
  Csr m;
  m.n_cols = end - begin + (int64_t)ghosts.size();
  for (int64_t r = begin; r < end; ++r) {
    std::vector<int32_t> c;
    std::vector<double> v;
    for (int64_t k = g.rp[(size_t)r]; k < g.rp[(size_t)r + 1]; ++k) {
      const int32_t gc = g.col[(size_t)k];
      const bool owned = gc >= begin && gc < end;
      c.push_back(owned ? (int32_t)(gc - begin) : (int32_t)(end - begin + (std::lower_bound(ghosts.begin(), ghosts.end(), gc) - ghosts.begin())));
      v.push_back(g.val[(size_t)k]);
    }
    m.add_row(c, v);
  }
  return m;
}

// The operators of tests/rank_cases.py LAYOUT_OPERATORS cut into the row chunks of 2, 3 and 4 ranks (chunk = ceil(n / N)):
// what every rank's planner makes of its owned rows.  The expectations are the planner's output when the cases were
// written; a rank that falls back to a simpler layout than listed fails.
struct RankWant { bool sell, val8, col16, sellp, rowclass, lat, hyb; int K, C; int64_t W; };
const RankWant kCsr = {false, false, false, false, false, false, false, 0, 0, 0};
const RankWant kHyb = {false, false, false, false, false, false, true, 0, 0, 0};
RankWant lat_run(int K, int C, int64_t W) { return {true, true, true, true, true, true, false, K, C, W}; }   // lattice window + pattern-run + row classes
RankWant lat_only(int K, int C, int64_t W) { return {true, true, true, false, false, true, false, K, C, W}; }  // lattice window on plain SELL streams
const RankWant kSellDistinct = {true, false, true, false, false, false, false, 0, 0, 0};

void localized_case(const char *name, const Csr &g, int n_ranks, const std::vector<RankWant> &want, bool allow_hybrid = false) {
  LayoutOptions opt;
  opt.sellp_cost = 4.0;
  const int64_t n = g.n_rows, chunk = (n + n_ranks - 1) / n_ranks;
  REQUIRE((int)want.size() == n_ranks);
  for (int rank = 0; rank < n_ranks; ++rank) {
    g_case = std::string("localized ") + name + ": rank " + std::to_string(rank) + " of " + std::to_string(n_ranks);
    const int64_t begin = std::min(n, rank * chunk), end = std::min(n, (rank + 1) * chunk);
    const Csr m = localize(g, begin, end);
    const StreamPlan P = plan_and_check(m, opt, allow_hybrid);
    const RankWant &w = want[(size_t)rank];
    std::printf("%s: sell %d val8 %d col16 %d pattern-run %d rowclass %d lattice %d (K %d C %d W %lld R0 %lld, %zu generic slices) hybrid %d; %lld rows, %lld ghosts, %d pattern slices\n",
                g_case.c_str(), (int)P.sell.built, (int)P.sell.s.val8, (int)P.sell.s.col16, (int)P.sell.use_sellp, (int)P.sellp.rowclass, (int)P.lat.built, P.lat.K, P.lat.C,
                (long long)P.lat.W, (long long)P.lat.R0, P.lat.gen.size(), (int)P.hyb.built, (long long)m.n_rows, (long long)(m.n_cols - m.n_rows),
                P.sell.built ? P.sell.pat.n_pattern_slices : P.hyb.built ? P.hyb.pat.n_pattern_slices : 0);
    REQUIRE(P.sell.built == w.sell && P.hyb.built == w.hyb && P.lat.built == w.lat);
    if (P.sell.built) REQUIRE(P.sell.s.val8 == w.val8 && P.sell.s.col16 == w.col16 && P.sell.use_sellp == w.sellp && P.sellp.rowclass == w.rowclass);
    if (P.hyb.built) REQUIRE(P.hyb.n_tiles > 0 && P.hyb.pat.n_pattern_slices > 0);
    if (!P.lat.built) continue;
    REQUIRE(P.lat.K == w.K && P.lat.C == w.C && P.lat.W == w.W);
    // an interior row is served without a look at its stored columns: none of them may be a ghost
    bool owned_only = true;
    for (int64_t r = P.lat.R0; r < P.lat.R1; ++r) {
      if (!((r - P.lat.R0) % P.lat.nxy < P.lat.W && (r - P.lat.R0) / P.lat.nxy < P.lat.K)) continue;
      for (int64_t k = m.rp[(size_t)r]; k < m.rp[(size_t)r + 1]; ++k) owned_only = owned_only && m.col[(size_t)k] < m.n_rows;
    }
    REQUIRE(owned_only);
  }
}

void localized_operators() {
  const Csr big = lattice(37, 23, 19), mixed = lattice(21, 17, 40), thin = lattice(13, 11, 9);
  const Csr hyb = hybrid_band(4400, {224, 1500, 2900, 4300}, {}, {}, true, true, 0);
  const Csr few = banded(5037, 27, 11, true, 1, 7), distinct = banded(5037, 27, 12, false);
  for (int n_ranks = 2; n_ranks <= 4; ++n_ranks) {
    localized_case("hybrid band 4400", hyb, n_ranks, std::vector<RankWant>((size_t)n_ranks, kHyb), true);
    localized_case("lattice 13 x 11 x 9", thin, n_ranks, std::vector<RankWant>((size_t)n_ranks, kCsr));
    localized_case("band 5037 distinct values", distinct, n_ranks, std::vector<RankWant>((size_t)n_ranks, kSellDistinct));
  }
  localized_case("lattice 37 x 23 x 19", big, 2, {lat_run(8, 7, 851), lat_run(8, 7, 851)});
  localized_case("lattice 37 x 23 x 19", big, 3, {lat_run(5, 7, 851), lat_only(5, 7, 851), lat_only(5, 7, 851)});
  localized_case("lattice 37 x 23 x 19", big, 4, {lat_run(3, 7, 851), lat_only(3, 7, 851), lat_only(3, 7, 851), lat_only(3, 7, 851)});
  localized_case("lattice 21 x 17 x 40", mixed, 2, {kCsr, kCsr});
  localized_case("lattice 21 x 17 x 40", mixed, 3, {kCsr, kCsr, kCsr});
  localized_case("lattice 21 x 17 x 40", mixed, 4, {kCsr, lat_run(8, 3, 357), lat_run(8, 3, 357), kCsr});
  localized_case("band 5037 few values", few, 2, {lat_run(277, 1, 9), lat_run(277, 1, 9)});
  localized_case("band 5037 few values", few, 3, {lat_run(184, 1, 9), lat_run(184, 1, 9), lat_run(184, 1, 9)});
  localized_case("band 5037 few values", few, 4, {lat_run(137, 1, 9), lat_run(137, 1, 9), lat_run(137, 1, 9), lat_run(137, 1, 9)});
}

void invalid_input() {
  g_case = "invalid input";
  Csr m = banded(100, 3, 16, true);
  REQUIRE(check_csr(m.view()) == nullptr);
  std::swap(m.rp[40], m.rp[41]);
  const char *msg = check_csr(m.view());
  REQUIRE(msg && std::string(msg) == "rowptr not monotone");
  std::swap(m.rp[40], m.rp[41]);
  m.col[17] = 100;
  msg = check_csr(m.view());
  REQUIRE(msg && std::string(msg) == "column index out of range");
  m.col[17] = -1;
  REQUIRE(check_csr(m.view()) != nullptr);
}

void threading() {
  g_case = "threading: 1 and 7 host threads";
  const Csr m = banded(2100 * 64 + 37, 27, 17, true, 1, 7);  // more than 2048 slices: every parallel loop splits
  LayoutOptions opt;
  opt.sellp_cost = 4.0;
  opt.sellp_rr = 1;
  PhaseLog quiet;
  g_host_threads = 1;
  const StreamPlan one = plan_streams(m.view(), opt, false, quiet);
  g_host_threads = 7;
  const StreamPlan seven = plan_and_check(m, opt);
  g_host_threads = 0;
  REQUIRE(one.sell.built && one.sellp.rowclass && one.lat.built && !one.sellp.wave_rr.empty());
  REQUIRE(plan_bytes(one) == plan_bytes(seven));
}

// ---------------------------------------------------------------- operators on the planner's limits
// The generators of tests/layout_limit_cases.py, restated (no random numbers on either side), and for every limit one operator
// on either side of it with the flags it must get.  The limits appear here as plain numbers: a planner
// whose limit moves by one fails the pair of that limit.

// A[i, i + d] = A[i + d, i] = upper(i, d), d = 1 .. 13; the rows of the empty slices store nothing and no row refers to them
template <class U, class D>
Csr symmetric_band(int64_t n, U upper, D diag, const std::vector<int64_t> &empty_slices = {}) {
  auto empty = [&](int64_t r) { return std::find(empty_slices.begin(), empty_slices.end(), r / 64) != empty_slices.end(); };
  Csr m;
  m.n_cols = n;
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> c;
    std::vector<double> v;
    for (int d = -13; d <= 13 && !empty(i); ++d) {
      const int64_t j = i + d;
      if (j < 0 || j >= n || empty(j)) continue;
      c.push_back((int32_t)j);
      v.push_back(d < 0 ? upper(j, -d) : d == 0 ? diag(i) : upper(i, d));
    }
    m.add_row(c, v);
  }
  return m;
}

Csr dictionary_operator(int n_nonzero, int64_t n = 5037) {
  std::vector<double> pool = {-0.0, 5e-324};
  for (int k = 1; k < 128; ++k) { pool.push_back(k / 128.0); pool.push_back(-k / 128.0); }
  const int64_t len = n_nonzero - 2;
  return symmetric_band(n, [&](int64_t i, int d) { return (d == 1 && (i == 40 * 64 + 10 || i == 5000)) ? 255.0 / 256.0 : pool[(size_t)((13 * i + d - 1) % len)]; },
                        [](int64_t) { return 64.0; });
}

Csr class_operator(int K, int64_t n, const std::vector<int64_t> &empty_slices = {}) {
  auto g = [K](int64_t i, int d) {
    const int64_t c = i % K;
    if (d == 13) return -(double)(c + 1) / 256.0;
    const int64_t t = (c * (2 * d + 1) + (c / 16) * d) % 16;
    return (t % 2 ? -1.0 : 1.0) * (double)(t / 2 + 1) / 64.0;
  };
  return symmetric_band(n, g, [K](int64_t i) { return 64.0 + (double)((i % K) % 3); }, empty_slices);
}

const double kFiveNonzero[5] = {-1.0 / 6, -1.0 / 12, 8.0 / 3, 0.5, 1.25};

Csr spread_operator(int64_t dmax, bool few, int64_t n = 5037, const std::vector<int64_t> &empty_slices = {}) {
  Csr m;
  m.n_cols = n + dmax;
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> c;
    std::vector<double> v;
    const int64_t lane = i % 64;
    const bool empty = std::find(empty_slices.begin(), empty_slices.end(), i / 64) != empty_slices.end();
    for (int64_t k = 0; k < 11 && !empty; ++k) {
      int64_t off = k * 6000 + 3 * (lane % 7);
      if (k == 0) off = lane == 0 ? 0 : lane % 7 + 1;
      if (k == 10) off = lane == 63 ? dmax : dmax - 1 - lane % 7;
      const int64_t e = 11 * i + k;
      c.push_back((int32_t)(i + off));
      v.push_back(few ? kFiveNonzero[(e * 7 + e / 5) % 5] : 1.0 + (double)e / 65536.0);
    }
    m.add_row(c, v);
  }
  return m;
}

Csr padding_operator(int64_t slices, int64_t wide_rows = 0) {
  Csr m;
  const int64_t n = 64 * slices;
  m.n_cols = n + 3 * 29;
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> c;
    std::vector<double> v;
    for (int64_t k = 0; k < ((i >= 64 && i < 64 + wide_rows) ? 29 : 25); ++k) {
      const int64_t e = 29 * i + k;
      c.push_back((int32_t)(i + 3 * k));
      v.push_back(kFiveNonzero[(e * 3 + e / 5) % 5]);
    }
    m.add_row(c, v);
  }
  return m;
}

Csr few_valued_band(int64_t n) {
  Csr m;
  m.n_cols = n;
  for (int64_t i = 0; i < n; ++i) {
    std::vector<int32_t> c;
    std::vector<double> v;
    for (int64_t k = 0; k < 27; ++k) {
      const int64_t j = i + k - 13, e = 27 * i + k;
      if (j < 0 || j >= n) continue;
      c.push_back((int32_t)j);
      v.push_back(k == 13 ? 64.0 : kFiveNonzero[(e * 3 + e / 5) % 5]);
    }
    m.add_row(c, v);
  }
  return m;
}

std::vector<int64_t> window_rows(int64_t first_len, int64_t last_len, int last_align) {
  std::vector<int64_t> lens = {first_len, 2};
  int64_t nnz = first_len + 2;
  auto align = [&](int a) {
    const int64_t pad = (((int64_t)a - nnz) % 4 + 4) % 4;
    if (pad) { lens.push_back(pad); nnz += pad; }
  };
  const std::vector<std::vector<int64_t>> follows = {{5}, {1, 0, 2}};
  for (const auto &follow : follows)
    for (int64_t L = 4092; L <= 4097; ++L)
      for (int a = 0; a < 4; ++a) {
        align(a);
        lens.push_back(L); nnz += L;
        for (int64_t f : follow) { lens.push_back(f); nnz += f; }
      }
  for (int64_t run : {1023, 1024, 1025}) {
    lens.insert(lens.end(), (size_t)run, 0);
    lens.push_back(3); nnz += 3;
  }
  align(last_align);
  lens.push_back(last_len);
  return lens;
}

Csr window_operator(int64_t first_len, int64_t last_len, int last_align) {
  Csr m;
  m.n_cols = 6000;
  int64_t k = 0, r = 0;
  for (int64_t len : window_rows(first_len, last_len, last_align)) {
    std::vector<int32_t> c;
    std::vector<double> v;
    for (int64_t j = 0; j < len; ++j, ++k) {
      c.push_back((int32_t)((17 * r) % 1200 + j + j / 7));
      v.push_back((k % 2 == 0 ? 1.0 : -1.0) * (0.5 + (double)(k % 8191) / 8192.0));
    }
    m.add_row(c, v);
    ++r;
  }
  return m;
}

// the tile boundaries the planner must give, with the limits as plain numbers
std::vector<int32_t> window_tiles_restated(const std::vector<int64_t> &rp) {
  const int64_t n = (int64_t)rp.size() - 1;
  std::vector<int32_t> tiles(1, 0);
  for (int64_t r = 0; r < n;) {
    const int64_t ka = rp[(size_t)r] & ~(int64_t)3;
    int64_t e = r + 1;
    while (e < n && rp[(size_t)e + 1] - ka <= 4096 && e - r < 1024) ++e;
    if (rp[(size_t)e] - ka > 4096) e = r + 1;
    tiles.push_back((int32_t)e);
    r = e;
  }
  return tiles;
}

struct LimitWant { bool sell, val8, col16, sellp, rowclass, lat; int sellp_classes, lat_classes; };  // lat_classes < 0: the count at which the planner gave up

StreamPlan limit_case(const char *name, const Csr &m, LayoutOptions opt, const LimitWant &w) {
  g_case = std::string("limit ") + name;
  opt.sellp_cost = opt.sellp_cost > 0.0 ? opt.sellp_cost : 4.0;
  const StreamPlan P = plan_and_check(m, opt);
  int fullest = 0;
  for (size_t wv = 0; wv + 1 < P.sellp.wave_ptr.size(); ++wv)
    fullest = std::max(fullest, (P.sellp.wave_ptr[wv + 1] & (kSellpStrided - 1)) - (P.sellp.wave_ptr[wv] & (kSellpStrided - 1)));
  std::printf("%s: sell %d val8 %d (%zu values) col16 %d pattern-run %d rowclass %d (%d classes) lattice %d (%d classes); %lld rows, %d pattern slices, %lld of %lld padded entries, fullest wave %d slices\n",
              g_case.c_str(), (int)P.sell.built, (int)P.sell.s.val8, P.sell.vd.n_values, (int)P.sell.s.col16, (int)P.sell.use_sellp, (int)P.sellp.rowclass, P.sellp.n_classes,
              (int)P.lat.built, P.lat.classes, (long long)m.n_rows, P.sell.pat.n_pattern_slices, (long long)(P.sell.quads * 256), (long long)m.rp.back(), fullest);
  REQUIRE(P.sell.built == w.sell && !P.hyb.built);
  if (!P.sell.built) return P;
  REQUIRE(P.sell.s.val8 == w.val8 && P.sell.s.col16 == w.col16 && P.sell.use_sellp == w.sellp && P.sellp.rowclass == w.rowclass && P.lat.built == w.lat);
  REQUIRE(P.sellp.n_classes == w.sellp_classes && P.lat.classes == w.lat_classes);
  return P;
}

LayoutOptions with(std::initializer_list<const char *> keys, int sell_grid = 0, double sellp_cost = 0.0) {
  LayoutOptions o;
  for (const char *k : keys) {
    const std::string s = k;
    if (s == "disable_sellp") o.disable_sellp = true;
    else if (s == "disable_rowclass") o.disable_rowclass = true;
    else if (s == "disable_lattice") o.disable_lattice = true;
    else REQUIRE(!"known option");
  }
  o.sell_grid = sell_grid; o.sellp_cost = sellp_cost;
  return o;
}

void limit_cases() {
  const std::vector<int64_t> empty_slices = {0, 20, 38, 39, 77};
  // ---- 1. value dictionary: 255 nonzero bit patterns + the padding zero = 256 codes | 257 values
  {
    const Csr at = dictionary_operator(255), beyond = dictionary_operator(256);
    StreamPlan P = limit_case("values-255", at, with({}), {true, true, true, true, false, false, 0, -129});
    REQUIRE(P.sell.vd.n_values == 256);
    // code 255 belongs to the value placed by hand, in slice 40 and in the last, partial slice: read back from the packed codes
    if (P.sell.vd.val8) {
      const uint8_t last = P.sell.vd.lookup(255.0 / 256.0);
      REQUIRE(last == 255 && P.sell.vd.lookup(-0.0) != 0 && P.sell.vd.lookup(5e-324) != 0 && P.sell.vd.lookup(-0.0) != P.sell.vd.lookup(5e-324));
      for (int64_t sl : {(int64_t)40, (int64_t)78}) {
        bool found = false;
        for (size_t o = (size_t)P.sell.slice_ptr[(size_t)sl] * 256; o < (size_t)P.sell.slice_ptr[(size_t)sl + 1] * 256; ++o) found = found || P.sell.s.v1[o] == 255;
        REQUIRE(found);
      }
    }
    limit_case("values-255-per-entry-kernel", at, with({"disable_sellp"}), {true, true, true, false, false, false, 0, -129});
    limit_case("values-255-grid8", at, with({"disable_sellp"}, 8), {true, true, true, false, false, false, 0, -129});
    P = limit_case("values-256", beyond, with({}), {true, false, true, false, false, false, 0, 0});
    REQUIRE(P.sell.vd.n_values > 256 || !P.sell.vd.val8);
    limit_case("values-256-grid8", beyond, with({}, 8), {true, false, true, false, false, false, 0, 0});
  }
  // ---- 2. slice span 65535 | 65536 columns, no column patterns
  for (int grid : {0, 8})
    for (int few = 1; few >= 0; --few) {
      const std::string tail = std::string(few ? "-codes" : "-doubles") + (grid ? "-grid8" : "");
      const Csr at = spread_operator(65472, few), beyond = spread_operator(65473, few);
      StreamPlan P = limit_case(("span-65535" + tail).c_str(), at, with({}, grid), {true, (bool)few, true, false, false, false, 0, 0});
      int64_t span = 0;
      for (int64_t k = at.rp[0]; k < at.rp[64]; ++k) span = std::max<int64_t>(span, at.col[(size_t)k] - P.sell.slice_base[0]);
      REQUIRE(span == 65535 && P.sell.pat.n_pattern_slices == 0);
      if (P.sell.s.col16) REQUIRE(*std::max_element(P.sell.s.c2.begin(), P.sell.s.c2.end()) == 65535);
      P = limit_case(("span-65536" + tail).c_str(), beyond, with({}, grid), {true, (bool)few, false, false, false, false, 0, 0});
      REQUIRE(P.sell.pat.n_pattern_slices == 0);
    }
  // ---- 3. row classes: 96 | 97 for the pattern-run kernel, 128 | 129 for the lattice kernel
  {
    const int64_t n = 20037;
    limit_case("classes-96", class_operator(96, n), with({}), {true, true, true, true, true, true, 96, 96});
    limit_case("classes-96-no-lattice", class_operator(96, n), with({"disable_lattice"}), {true, true, true, true, true, false, 96, 0});
    limit_case("classes-97", class_operator(97, n), with({}), {true, true, true, true, false, true, 0, 97});
    limit_case("classes-97-no-lattice", class_operator(97, n), with({"disable_lattice"}), {true, true, true, true, false, false, 0, 0});
    limit_case("classes-128", class_operator(128, n), with({}), {true, true, true, true, false, true, 0, 128});
    limit_case("classes-129", class_operator(129, n), with({}), {true, true, true, true, false, false, 0, -129});
  }
  // ---- 4. slices per wave: sell_grid 8 = 32 waves; 64 | 65 slices in the fullest
  {
    const Csr keeps = class_operator(7, 2043 * 64), withdrawn = class_operator(7, 2044 * 64);
    auto fullest = [](const StreamPlan &P) {
      int f = 0;
      for (size_t wv = 0; wv + 1 < P.sellp.wave_ptr.size(); ++wv)
        f = std::max(f, (P.sellp.wave_ptr[wv + 1] & (kSellpStrided - 1)) - (P.sellp.wave_ptr[wv] & (kSellpStrided - 1)));
      return f;
    };
    StreamPlan P = limit_case("wave-64-slices", keeps, with({"disable_lattice"}, 8), {true, true, true, true, true, false, 7, 0});
    REQUIRE(P.sellp.wave_ptr.size() == 33 && fullest(P) == 64);
    P = limit_case("wave-64-slices-codes", keeps, with({"disable_lattice", "disable_rowclass"}, 8), {true, true, true, true, false, false, 0, 0});
    REQUIRE(P.sellp.wave_ptr.size() == 33 && fullest(P) == 64);
    for (size_t wv = 0; wv + 1 < P.sellp.wave_ptr.size(); ++wv) REQUIRE(!(P.sellp.wave_ptr[wv] & kSellpFastWave));  // every wave needs its metadata lanes
    P = limit_case("wave-65-slices", withdrawn, with({"disable_lattice"}, 8), {true, true, true, false, false, false, 0, 0});
    REQUIRE(P.sellp.wave_ptr.empty() && P.sell.sellp_pid >= 0);
  }
  // ---- 5. slices without quads: first, where an XCD's eighth begins, two neighbours, the last full slice
  {
    const Csr pat = class_operator(7, 5037, empty_slices);
    auto no_quads = [&](const StreamPlan &P) {
      bool ok = P.sell.n_slices == 79;
      for (int64_t sl : empty_slices) ok = ok && P.sell.slice_ptr[(size_t)sl + 1] == P.sell.slice_ptr[(size_t)sl] && P.sell.pat.spat[(size_t)sl] < 0;
      return ok;
    };
    REQUIRE(20 == 2 * ((79 + 7) / 8));  // slice 20 is the first of XCD 2's eighth
    StreamPlan P = limit_case("empty-slices-lattice", pat, with({}), {true, true, true, true, true, true, 85, 86});
    REQUIRE(no_quads(P));
    limit_case("empty-slices-rowclass", pat, with({"disable_lattice"}), {true, true, true, true, true, false, 85, 0});
    limit_case("empty-slices-codes", pat, with({"disable_lattice", "disable_rowclass"}), {true, true, true, true, false, false, 0, 0});
    limit_case("empty-slices-per-entry-kernel", pat, with({"disable_lattice", "disable_sellp"}), {true, true, true, false, false, false, 0, 0});
    const StreamPlan c4 = limit_case("empty-slices-rowclass-grid8", pat, with({"disable_lattice"}, 8), {true, true, true, true, true, false, 85, 0});
    const StreamPlan c1 = limit_case("empty-slices-rowclass-grid8-cost1", pat, with({"disable_lattice"}, 8, 1.0), {true, true, true, true, true, false, 85, 0});
    const StreamPlan c16 = limit_case("empty-slices-codes-grid8-cost16", pat, with({"disable_lattice", "disable_rowclass"}, 8, 16.0), {true, true, true, true, false, false, 0, 0});
    auto bounds = [](const StreamPlan &Q) { std::vector<int32_t> b; for (int32_t e : Q.sellp.wave_ptr) b.push_back(e & (kSellpStrided - 1)); return b; };
    REQUIRE(bounds(c4) != bounds(c1) && bounds(c4) != bounds(c16) && bounds(c1) != bounds(c16));  // other wave boundaries
    limit_case("empty-slices-per-entry-kernel-grid8", pat, with({"disable_lattice", "disable_sellp"}, 8), {true, true, true, false, false, false, 0, 0});
    for (int grid : {0, 8}) {
      P = limit_case(grid ? "empty-slices-streamed-codes-grid8" : "empty-slices-streamed-codes", spread_operator(65472, true, 5037, empty_slices), with({}, grid),
                     {true, true, true, false, false, false, 0, 0});
      REQUIRE(no_quads(P) && P.sell.pat.n_pattern_slices == 0);
      P = limit_case(grid ? "empty-slices-streamed-doubles-grid8" : "empty-slices-streamed-doubles", spread_operator(65473, false, 5037, empty_slices), with({}, grid),
                     {true, false, false, false, false, false, 0, 0});
      REQUIRE(no_quads(P) && P.sell.pat.n_pattern_slices == 0);
    }
  }
  // ---- 6. the row window: 4096 entries from the row's start rounded down to 4, at most 1024 rows in a tile
  for (int64_t L = 4092; L <= 4097; ++L)
    for (int a = 0; a < 4; ++a) {
      g_case = "limit window: first and last row of " + std::to_string(L) + " entries, the last starting at " + std::to_string(a) + " mod 4";
      const Csr m = window_operator(L, L, a);
      const StreamPlan P = plan_and_check(m, with({}, 0, 4.0));
      REQUIRE(!P.sell.built && !P.hyb.built);
      const TilePlan T = plan_tiles(m.rp.data(), m.n_rows);
      REQUIRE(T.tile_row == window_tiles_restated(m.rp));
      REQUIRE(m.rp[(size_t)m.n_rows - 1] % 4 == a && m.rp[(size_t)m.n_rows] - m.rp[(size_t)m.n_rows - 1] == L);
      if (L != 4092 || a != 0) continue;
      // what the tiles of this operator must show: rows that end exactly at the window's edge, rows one entry beyond it, and
      // tiles of exactly 1024 rows
      int exact = 0, beyond = 0, capped = 0, shared = 0;
      for (size_t t = 0; t + 1 < T.tile_row.size(); ++t) {
        const int32_t b = T.tile_row[t], e = T.tile_row[t + 1];
        const int64_t used = m.rp[(size_t)e] - (m.rp[(size_t)b] & ~(int64_t)3);
        exact += used == 4096;
        beyond += used == 4097 && e - b == 1;
        capped += e - b == 1024;
        shared += e - b > 1 && m.rp[(size_t)b + 1] - m.rp[(size_t)b] >= 4092;
      }
      std::printf("%s: %d tiles, %d filled to the last entry, %d long rows one entry beyond, %d of 1024 rows, %d with a row of >= 4092 entries and others\n", g_case.c_str(),
                  T.n_tiles, exact, beyond, capped, shared);
      REQUIRE(exact >= 4 && beyond >= 4 && capped >= 3 && shared >= 4);
    }
  // ---- 7. entry conditions: 1024 | 1023 rows; padded entries = floor(1.12 nnz) | one quad more
  {
    limit_case("rows-1024", few_valued_band(1024), with({"disable_lattice"}), {true, true, true, true, true, false, 25, 0});
    limit_case("rows-1023", few_valued_band(1023), with({"disable_lattice"}), {false, false, false, false, false, false, 0, 0});
    const Csr at = padding_operator(20), beyond = padding_operator(20, 2);
    const StreamPlan P = limit_case("padding-at-the-bound", at, with({}), {true, true, true, false, false, false, 0, 0});
    REQUIRE(P.sell.quads * 256 == (int64_t)std::floor(1.12 * (double)at.rp.back()) && P.sell.quads == 20 * 7);
    limit_case("padding-one-quad-beyond", beyond, with({}), {false, false, false, false, false, false, 0, 0});
    // the operator beyond the bound is one quad wider and would pass again with the bound at 1.13
    PhaseLog quiet;
    SellPlan s;
    const CsrView B = beyond.view();
    REQUIRE(!plan_sell(B, analyse_slices(B, true), LayoutOptions(), quiet, s) && s.quads == 20 * 7 + 1 && beyond.rp.back() == at.rp.back() + 8);
  }
}

}  // namespace

int main() {
  sell_variants();
  other_sell_cases();
  hybrid_cases();
  localized_operators();
  invalid_input();
  threading();
  limit_cases();
  if (g_failures) std::fprintf(stderr, "%d requirement(s) failed\n", g_failures);
  else std::printf("layout round trip: all cases passed\n");
  return g_failures ? 1 : 0;
}
