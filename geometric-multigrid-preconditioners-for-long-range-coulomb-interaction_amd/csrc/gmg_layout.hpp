// gmg_layout.hpp -- the device layouts of a host-given CSR operator, planned on the host (DESIGN.md sections 3 and 28).
// Host-only standard C++: no HIP, no context.  plan_tiles / plan_streams turn a CSR into plain vectors and scalars, upload_csr
// (gmg_coulomb.hip) copies them to the device as they are.  The kernels that read the layouts are in gmg_device.hpp and
// gmg_lattice.hpp, which take their layout constants from here; tests/layout_roundtrip.cc restates their addressing rules
// and decodes every plan back to the CSR it came from.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <map>
#include <thread>
#include <unordered_map>
#include <vector>

namespace gmg {

constexpr int kTileNnz = 4096;     // LDS row window, doubles (32 KiB) -> 4 workgroups / CU
constexpr int64_t kTileMaxRowsEarly = 1024;
constexpr int kMaxPartials = 2048; // upper bound of any grid that emits reduction partials
constexpr int kSellpMaxClasses = 96;  // row classes (27 coefficients each) the pattern-run kernel keeps in LDS: 20 KB, 6 workgroups / CU
constexpr int kSellpWaves = 4;  // resident waves per SIMD (= workgroups per CU) the register budget of the kernel is set for
constexpr int kSellpStrided = 0x20000000;   // flag in wave_ptr[w]: the wave's pairs of slices are described by wave_rr[w]
constexpr int kSellpFastWave = 0x40000000;  // flag in wave_ptr[w]: every slice of wave w is a run-pattern slice with row classes
constexpr int kLatMaxClasses = 128;  // 27 doubles each in LDS: 27.6 KB (125 = the position types of gmg_set_level_matrix_lattice)
constexpr int kLatRowsPerUnit = 124;
constexpr int kLatWavesPerSimd = 4;  // register budget of the kernel (128 VGPRs): the window of planes lives in registers

// Host-side setup loops (layout conversion of 10^7..10^8 nonzeros) run on a few threads: f(begin, end, chunk)
inline int g_host_threads = 0;  // option "host_threads" (process-wide); 0 = hardware concurrency, at most 16
inline int host_threads() {
  const int t = g_host_threads > 0 ? g_host_threads : (int)std::thread::hardware_concurrency();
  return std::max(1, std::min(16, t));
}
template <class F>
void parallel_chunks(int64_t n, F f) {
  const int nt = host_threads();
  if (n < 2048 || nt <= 1) { f((int64_t)0, n, 0); return; }
  const int64_t per = (n + nt - 1) / nt;
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t) {
    const int64_t b = t * per, e = std::min(n, b + per);
    if (b < e) th.emplace_back(f, b, e, t);
  }
  for (auto &x : th) x.join();
}

struct LayoutOptions {  // the context's options that steer a layout
  bool disable_sell = false, disable_patterns = false, disable_compression = false, disable_sellp = false, disable_rowclass = false,
       disable_lattice = false, disable_hybrid = false;
  int sell_grid = 0;
  double sellp_cost = 0.0;
  int sellp_rr = 0, lattice_segments = 0, lattice_max_blocks = 0;
  bool debug = false;
};

struct PhaseLog {  // the "[gmg]   upload <phase> <ms>" lines of option debug_upload
  bool on = false;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void operator()(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[gmg]   upload %-14s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

struct CsrView {
  int64_t n_rows = 0, n_cols = 0;
  const int64_t *rowptr = nullptr;
  const int32_t *col = nullptr;
  const double *val = nullptr;
  int64_t nnz() const { return rowptr[n_rows]; }
  int64_t n_slices() const { return (n_rows + 63) / 64; }
  int64_t slice_end(int64_t sl) const { return std::min<int64_t>(n_rows, sl * 64 + 64); }  // one past the last row of slice sl
};

// stable transpose: row j of A^T lists the entries of column j in ascending source row,
// i.e. the order in which the sequential scatter of Tvmult / restrict_and_add adds them.
inline void transpose_host(int64_t n_rows, int64_t n_cols, const int64_t *rp, const int32_t *col, const double *val,
                    std::vector<int64_t> &trp, std::vector<int32_t> &tcol, std::vector<double> &tval) {
  const int64_t nnz = rp[n_rows];
  trp.assign((size_t)n_cols + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) trp[(size_t)col[k] + 1]++;
  for (int64_t j = 0; j < n_cols; ++j) trp[(size_t)j + 1] += trp[(size_t)j];
  tcol.resize((size_t)nnz);
  tval.resize((size_t)nnz);
  std::vector<int64_t> pos(trp.begin(), trp.end() - 1);
  for (int64_t i = 0; i < n_rows; ++i)
    for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
      const int64_t p = pos[(size_t)col[k]]++;
      tcol[(size_t)p] = (int32_t)i;
      tval[(size_t)p] = val[k];
    }
}

// what is wrong with the row pointers or columns of A (nullptr: nothing)
inline const char *check_csr(const CsrView &A) {
  for (int64_t i = 1; i <= A.n_rows; ++i)
    if (A.rowptr[i] < A.rowptr[i - 1]) return "rowptr not monotone";
  for (int64_t k = 0; k < A.nnz(); ++k)
    if (A.col[k] < 0 || A.col[k] >= A.n_cols) return "column index out of range";
  return nullptr;
}

// ---------------------------------------------------------------- CSR row-window tiles

// Tiles of the CSR row-window kernel over rows [rb, re): consecutive rows whose nonzeros fit the LDS window (window start
// rounded down to 4).  Returns the tile boundaries, rb first, re last.
template <class RP>
std::vector<int32_t> window_tiles(const RP *rowptr, int64_t rb, int64_t re) {
  std::vector<int32_t> tiles(1, (int32_t)rb);
  for (int64_t r = rb; r < re;) {
    const int64_t ka = (int64_t)rowptr[r] & ~(int64_t)3;
    int64_t e = r + 1;  // a tile always holds at least one row (possibly a "long row")
    // rows are capped too: operators with long runs of empty rows (P^T onto the level-0 lattice)
    // would otherwise put 10^5 rows into one workgroup
    while (e < re && (int64_t)rowptr[e + 1] - ka <= kTileNnz && e - r < kTileMaxRowsEarly) ++e;
    if ((int64_t)rowptr[e] - ka > kTileNnz) e = r + 1;
    tiles.push_back((int32_t)e);
    r = e;
  }
  return tiles;
}

struct TilePlan {
  std::vector<int32_t> tile_row;  // n_tiles + 1 boundaries
  int n_tiles = 0, tiles_per_xcd = 0, grid = 0;
};
template <class RP>
TilePlan plan_tiles(const RP *rowptr, int64_t n_rows) {
  TilePlan T;
  T.tile_row = window_tiles(rowptr, 0, n_rows);
  T.n_tiles = (int)T.tile_row.size() - 1;
  T.tiles_per_xcd = (T.n_tiles + 7) / 8;
  T.grid = 8 * std::min(kMaxPartials / 8, std::max(1, T.tiles_per_xcd));
  return T;
}

// ---------------------------------------------------------------- building blocks of the SELL-64 streams

struct Slices {  // a list of slices, or all of them (list == nullptr)
  const std::vector<int32_t> *list;
  int64_t n;
  int64_t size() const { return list ? (int64_t)list->size() : n; }
  int64_t operator[](int64_t i) const { return list ? (*list)[(size_t)i] : i; }
};

// Per slice: the widest row, and the sorted union of (col - row) where the slice qualifies for a column pattern: all 64
// rows exist and the union has <= 32 members that are valid columns for every row; rows lacking a member get an explicit
// +0.0 there (exact: x is finite), which keeps the CSR summation order.
// (a row-partitioned operator has its ghost columns behind the owned ones, n_cols > n_rows: the slices whose columns are all
// owned still follow the lattice's patterns -- without them the distributed coarse CG ran on per-entry gathers, 99 us per
// iteration on two ranks against 34 us on one)
struct SliceInfo {
  std::vector<int32_t> width;
  std::vector<std::vector<int32_t>> delta;
  int64_t quads(int64_t sl) const {  // of the packed slice: the width is that of its pattern where it has one
    const int64_t w = delta[(size_t)sl].empty() ? width[(size_t)sl] : (int64_t)delta[(size_t)sl].size();
    return (w + 3) / 4;
  }
};
inline SliceInfo analyse_slices(const CsrView &A, bool allow_pat) {
  SliceInfo I;
  I.width.assign((size_t)A.n_slices(), 0);
  I.delta.resize((size_t)A.n_slices());
  const int64_t *rowptr = A.rowptr;
  const int32_t *col = A.col;
  parallel_chunks(A.n_slices(), [&](int64_t sb, int64_t se, int) {
    for (int64_t sidx = sb; sidx < se; ++sidx) {
      int64_t w = 0;
      for (int64_t r2 = sidx * 64; r2 < A.slice_end(sidx); ++r2) w = std::max(w, rowptr[r2 + 1] - rowptr[r2]);
      I.width[(size_t)sidx] = (int32_t)w;
      if (!(allow_pat && sidx * 64 + 64 <= A.n_rows)) continue;
      std::vector<int32_t> delta;
      for (int64_t r2 = sidx * 64; r2 < sidx * 64 + 64 && delta.size() <= 32; ++r2)
        for (int64_t k = rowptr[r2]; k < rowptr[r2 + 1]; ++k) {
          const int32_t d = (int32_t)(col[k] - r2);
          auto it = std::lower_bound(delta.begin(), delta.end(), d);
          if (it == delta.end() || *it != d) delta.insert(it, d);
        }
      bool ok = !delta.empty() && delta.size() <= 32;
      if (ok) ok = sidx * 64 + delta.front() >= 0 && sidx * 64 + 63 + delta.back() < A.n_cols;
      // columns must be strictly ascending inside each row for the positions to be well defined
      for (int64_t r2 = sidx * 64; ok && r2 < sidx * 64 + 64; ++r2)
        for (int64_t k = rowptr[r2] + 1; k < rowptr[r2 + 1]; ++k) ok = ok && col[k] > col[k - 1];
      if (ok && (int64_t)delta.size() <= ((w + 3) / 4) * 4 + 4) I.delta[(size_t)sidx] = std::move(delta);
    }
  });
  return I;
}

struct Patterns {
  std::vector<std::vector<int32_t>> list;
  std::vector<int32_t> spat;  // per slice: its pattern, or -1
  int n_pattern_slices = 0;
  std::vector<int32_t> table;  // 32 offsets per pattern; padding: own row, value +0.0
};
// pattern ids in slice order
inline Patterns assign_patterns(const SliceInfo &I, const Slices &S) {
  Patterns P;
  P.spat.assign(I.delta.size(), -1);
  std::map<std::vector<int32_t>, int> pattern_id;
  for (int64_t i = 0; i < S.size(); ++i) {
    const auto &delta = I.delta[(size_t)S[i]];
    if (delta.empty()) continue;
    auto ins = pattern_id.emplace(delta, (int)P.list.size());
    if (ins.second) P.list.push_back(delta);
    P.spat[(size_t)S[i]] = ins.first->second;
    ++P.n_pattern_slices;
  }
  P.table.assign(std::max<size_t>(P.list.size(), 1) * 32, 0);
  for (size_t pi = 0; pi < P.list.size(); ++pi) std::copy(P.list[pi].begin(), P.list[pi].end(), P.table.begin() + (std::ptrdiff_t)pi * 32);
  return P;
}

// Value dictionary (bit patterns, so -0.0 / NaN payloads survive) over the entries of the slices S: 8-bit codes when they
// hold <= 256 distinct values including +0.0, the padding value, which is always code 0.
struct ValueDict {
  bool val8 = false;
  size_t n_values = 1;
  std::vector<double> dict;  // 256 entries: value of every code
  std::vector<uint64_t> key = std::vector<uint64_t>(1024, 0);  // read-only open-addressing table for the packing threads
  std::vector<int16_t> code = std::vector<int16_t>(1024, -1);
  static size_t slot(uint64_t bits) { return (size_t)((bits * 0x9E3779B97F4A7C15ull) >> 54); }
  uint8_t lookup(uint64_t bits) const {
    size_t h = slot(bits);
    while (key[h] != bits || code[h] < 0) h = (h + 1) & 1023;
    return (uint8_t)code[h];
  }
  uint8_t lookup(double v) const { uint64_t bits; std::memcpy(&bits, &v, 8); return lookup(bits); }
};
inline ValueDict value_dictionary(const CsrView &A, const Slices &S, bool allow) {
  ValueDict D;
  D.val8 = allow;
  D.dict.assign(1, 0.0);
  std::unordered_map<uint64_t, int> code_of;
  code_of.emplace(0ull, 0);
  // distinct bit patterns in order of first occurrence: per chunk of slices in parallel, merged in chunk order
  std::vector<std::vector<uint64_t>> firsts((size_t)host_threads());
  std::vector<char> overflow((size_t)host_threads(), 0);
  if (D.val8)
    parallel_chunks(S.size(), [&](int64_t ib, int64_t ie, int t) {
      std::unordered_map<uint64_t, int> seen;
      uint64_t last = ~0ull;
      for (int64_t i = ib; i < ie; ++i)
        for (int64_t k = A.rowptr[S[i] * 64]; k < A.rowptr[A.slice_end(S[i])]; ++k) {
          uint64_t bits;
          std::memcpy(&bits, &A.val[k], 8);
          if (bits == last) continue;
          last = bits;
          if (seen.emplace(bits, 0).second) {
            firsts[(size_t)t].push_back(bits);
            if (firsts[(size_t)t].size() > 256) { overflow[(size_t)t] = 1; return; }
          }
        }
    });
  for (size_t t = 0; t < firsts.size() && D.val8; ++t) {
    if (overflow[t]) D.val8 = false;
    for (uint64_t bits : firsts[t]) {
      if (!D.val8) break;
      if (code_of.emplace(bits, (int)D.dict.size()).second) {
        double v;
        std::memcpy(&v, &bits, 8);
        D.dict.push_back(v);
        if (D.dict.size() > 256) D.val8 = false;
      }
    }
  }
  if (D.val8)
    for (const auto &kv : code_of) {
      size_t h = ValueDict::slot(kv.first);
      while (D.code[h] >= 0) h = (h + 1) & 1023;
      D.key[h] = kv.first; D.code[h] = (int16_t)kv.second;
    }
  D.n_values = code_of.size();
  D.dict.resize(256, 0.0);
  return D;
}

// The value and column streams of spmv_sell_kernel: values in double2 pairs or one code per entry, columns four per lane
// as 32-bit indices or 16-bit offsets from the slice's base.
struct SellStreams {
  bool val8 = false, col16 = false;
  std::vector<double> v2;
  std::vector<uint8_t> v1;
  std::vector<int32_t> c4;
  std::vector<uint16_t> c2;
  const void *vals() const { return val8 ? (const void *)v1.data() : (const void *)v2.data(); }
  const void *cols() const { return col16 ? (const void *)c2.data() : (const void *)c4.data(); }
  size_t val_bytes() const { return val8 ? v1.size() : v2.size() * 8; }
  size_t col_bytes() const { return col16 ? c2.size() * 2 : c4.size() * 4; }
};
// Packs the slices S, slice sl into quads [qptr[sl], qptr[sl + 1]).  A pattern slice walks its pattern positions, any other
// slice its rows' entries.  Padding is +0.0 at the row itself; where the row is no valid column, at the slice's base
// (sbase given) or at the slice's first column (sbase == nullptr: the hybrid streams).
inline SellStreams pack_slices(const CsrView &A, const Slices &S, const std::vector<int32_t> &qptr, const Patterns &P, const ValueDict &D, bool col16,
                               const int32_t *sbase) {
  SellStreams out;
  out.val8 = D.val8; out.col16 = col16;
  const size_t n_ent = (size_t)qptr.back() * 256;
  out.v2.assign(D.val8 ? 0 : n_ent, 0.0);
  out.v1.assign(D.val8 ? n_ent : 0, 0);
  out.c4.assign(col16 ? 0 : n_ent, 0);
  out.c2.assign(col16 ? n_ent : 0, 0);
  const int64_t *rowptr = A.rowptr;
  const int32_t *col = A.col;
  const double *val = A.val;
  auto pack_lane = [&](int64_t sl, int lane, int32_t fill) {
    const int64_t q0 = qptr[(size_t)sl], nq = qptr[(size_t)sl + 1] - q0, r2 = sl * 64 + lane;
    const int64_t k0 = r2 < A.n_rows ? rowptr[r2] : 0, len = r2 < A.n_rows ? rowptr[r2 + 1] - k0 : 0;
    const int32_t padcol = r2 < std::min(A.n_rows, A.n_cols) ? (int32_t)r2 : fill;
    const std::vector<int32_t> *dl = P.spat[(size_t)sl] >= 0 ? &P.list[(size_t)P.spat[(size_t)sl]] : nullptr;
    int64_t kk = 0;  // next CSR entry of this row (pattern slices walk the pattern positions)
    for (int64_t j = 0; j < 4 * nq; ++j) {
      const int64_t qq = q0 + j / 4, e = j & 3;
      const size_t ov = (size_t)(((2 * qq + (e >> 1)) * 64 + lane) * 2 + (e & 1));  // double2-pair layout
      const size_t oc = (size_t)((qq * 64 + lane) * 4 + e);                          // 4-per-lane layout
      int32_t cj;
      double vj;
      if (dl) {
        const bool in = j < (int64_t)dl->size();
        if (in && kk < len && col[k0 + kk] - r2 == (*dl)[(size_t)j]) { cj = col[k0 + kk]; vj = val[k0 + kk]; ++kk; }
        else { cj = (int32_t)(in ? r2 + (*dl)[(size_t)j] : r2); vj = 0.0; }
      } else {
        cj = j < len ? col[k0 + j] : padcol;
        vj = j < len ? val[k0 + j] : 0.0;
      }
      if (D.val8) out.v1[oc] = D.lookup(vj);
      else out.v2[ov] = vj;
      if (col16) out.c2[oc] = (uint16_t)(cj - sbase[sl]);
      else out.c4[oc] = cj;
    }
  };
  parallel_chunks(S.size(), [&](int64_t ib, int64_t ie, int) {
    for (int64_t i = ib; i < ie; ++i) {
      const int64_t sl = S[i], rb = sl * 64;
      const int32_t fill = sbase ? sbase[sl] : rowptr[A.slice_end(sl)] > rowptr[rb] ? col[rowptr[rb]] : 0;
      for (int lane = 0; lane < 64; ++lane) pack_lane(sl, lane, fill);
    }
  });
  return out;
}

// ---------------------------------------------------------------- SELL-64, pattern-run tables, lattice window

struct SellPlan {
  bool built = false;
  int64_t n_slices = 0, quads = 0;
  std::vector<int32_t> slice_ptr, slice_base;  // in quads / smallest column per slice
  Patterns pat;
  ValueDict vd;
  SellStreams s;
  // the most frequent pattern made of nine runs of three consecutive columns, served by spmv_sellp_kernel
  int sellp_pid = -1, sellp_centre[9] = {};
  bool use_sellp = false;
  int sell_grid = 0;
};

struct WaveRR { int32_t first, stride, pairs, extra; };  // strided fast waves: {first slice, stride, pairs, one more slice or -1}

struct SellpPlan {  // tables of spmv_sellp_kernel
  std::vector<int32_t> wave_ptr;  // slice range of every wave, with the kSellp* flags
  bool rowclass = false;          // run-pattern slices take their coefficients from a per-row class table (N4)
  int n_classes = 0;
  std::vector<uint8_t> rowcls;
  std::vector<double> ctab;
  std::vector<WaveRR> wave_rr;  // empty: no wave is strided
};

struct LatticePlan {  // rows R0 + k nxy + [0, W), k < K, below R1, are walked plane by plane from a class table
  bool planned = false, built = false;  // planned: the fields below are set; built: the grid fits the reduction partials too
  int64_t nx = 0, nxy = 0, R0 = 0, R1 = 0, W = 0, fast_rows = 0, gen_bytes = 0;
  int K = 0, C = 0, S = 0, fast_blocks = 0, grid = 0, classes = 0;
  std::vector<uint8_t> rowcls;
  std::vector<double> ctab;
  std::vector<int32_t> gen;  // the slices with a row outside the window: served from the SELL streams
  bool fast(int64_t r) const { return r >= R0 && r < R1 && (r - R0) % nxy < W; }
};

// per-slice column base, 16-bit offsets if every slice spans < 65536 columns
inline bool slice_bases(const CsrView &A, std::vector<int32_t> &sbase) {
  sbase.assign((size_t)A.n_slices(), 0);
  std::vector<char> wide((size_t)host_threads(), 0);
  parallel_chunks(A.n_slices(), [&](int64_t sb, int64_t se, int t) {
    for (int64_t sidx = sb; sidx < se; ++sidx) {
      int64_t lo = INT64_MAX, hi = -1;
      for (int64_t r2 = sidx * 64; r2 < A.slice_end(sidx); ++r2) {
        lo = std::min(lo, r2 < A.n_cols ? r2 : lo);  // the padding column is the row itself
        hi = std::max(hi, r2 < A.n_cols ? r2 : hi);
        for (int64_t k = A.rowptr[r2]; k < A.rowptr[r2 + 1]; ++k) { lo = std::min<int64_t>(lo, A.col[k]); hi = std::max<int64_t>(hi, A.col[k]); }
      }
      if (hi < 0) { lo = hi = 0; }
      sbase[(size_t)sidx] = (int32_t)lo;
      if (hi - lo > 65535) wide[(size_t)t] = 1;
    }
  });
  return std::none_of(wide.begin(), wide.end(), [](char w) { return w != 0; });
}

// the most frequent pattern made of nine runs of three consecutive columns (the x-1, x, x+1 neighbours of a 27-point
// lattice row) is served by spmv_sellp_kernel
inline void pick_run_pattern(SellPlan &s, const LayoutOptions &opt) {
  std::vector<size_t> uses(s.pat.list.size(), 0);
  for (int32_t p : s.pat.spat)
    if (p >= 0) ++uses[(size_t)p];
  size_t n_run_slices = 0;
  for (size_t pi = 0; pi < s.pat.list.size(); ++pi) {
    const auto &dl = s.pat.list[pi];
    bool ok = dl.size() == 27;
    for (size_t j = 0; ok && j < dl.size(); j += 3) ok = dl[j + 1] == dl[j] + 1 && dl[j + 2] == dl[j] + 2;
    if (!ok || uses[pi] <= n_run_slices) continue;
    n_run_slices = uses[pi];
    s.sellp_pid = (int)pi;
    for (size_t u = 0; u < 9; ++u) s.sellp_centre[u] = dl[3 * u + 1];
  }
  // a streamed slice costs ~4 pattern slices here against ~2.2 in the per-entry kernel: worth it up to ~40 % streamed slices
  s.use_sellp = s.vd.val8 && !opt.disable_sellp && n_run_slices * 10 >= (size_t)s.n_slices * 7;
}

// Contiguous slice ranges per wave of spmv_sellp_kernel, balanced by cost: a streamed slice (one memory round trip per quad)
// costs about four pattern slices.  Empty when a wave would get more than 64 slices (slice metadata lives in the 64 lanes).
inline std::vector<int32_t> balance_waves(const SellPlan &s, double other_cost) {
  const size_t n_slices = (size_t)s.n_slices;
  const int n_waves = s.sell_grid * 4;
  std::vector<double> cost(n_slices + 1, 0.0);
  for (size_t sl = 0; sl < n_slices; ++sl)
    cost[sl + 1] = cost[sl] + (s.pat.spat[sl] == s.sellp_pid ? 1.0 : std::max(0.25, other_cost * (double)(s.slice_ptr[sl + 1] - s.slice_ptr[sl]) / 7.0));
  std::vector<int32_t> wp((size_t)n_waves + 1, 0);
  size_t sl = 0;
  for (int wv = 1; wv <= n_waves; ++wv) {
    const double target = cost[n_slices] * (double)wv / (double)n_waves;
    while (sl < n_slices && cost[sl + 1] <= target + 1e-9) ++sl;
    if (wv == n_waves) sl = n_slices;
    wp[(size_t)wv] = (int32_t)sl;
    if (wp[(size_t)wv] - wp[(size_t)wv - 1] > 64) return {};
  }
  return wp;
}

// Row classes of the run-pattern slices (N4): the 27-tuple of value codes of a row, read from the packed codes; a lattice
// operator has a few dozen of them.  Too many classes (> kSellpMaxClasses): the per-entry codes stay in use.
inline void sellp_row_classes(const SellPlan &s, int64_t n_rows, SellpPlan &w) {
  w.rowcls.assign((size_t)n_rows, 0);
  std::map<std::array<uint8_t, 27>, int> cls_of;
  for (size_t s2 = 0; s2 < (size_t)s.n_slices; ++s2) {
    if (s.pat.spat[s2] != s.sellp_pid) continue;
    for (int lane = 0; lane < 64; ++lane) {
      std::array<uint8_t, 27> key;
      for (int j = 0; j < 27; ++j) key[(size_t)j] = s.s.v1[(size_t)((((int64_t)s.slice_ptr[s2] + j / 4) * 64 + lane) * 4 + (j & 3))];
      auto ins = cls_of.emplace(key, (int)cls_of.size());
      if (ins.second) {
        if ((int)cls_of.size() > kSellpMaxClasses) return;
        for (int j = 0; j < 27; ++j) w.ctab.push_back(s.vd.dict[key[(size_t)j]]);
      }
      w.rowcls[s2 * 64 + (size_t)lane] = (uint8_t)ins.first->second;
    }
  }
  w.rowclass = !cls_of.empty();
  w.n_classes = (int)cls_of.size();
}

// Large operators: the slices of consecutive fast waves of one XCD are dealt round-robin in pairs, so that at any time the
// XCD's waves sit inside a window of ~2 W slices (their x working set: three lattice planes instead of the XCD's whole
// eighth of x, which is then fetched once).
inline std::vector<WaveRR> round_robin_waves(std::vector<int32_t> &wp) {
  const int n_waves = (int)wp.size() - 1, per_xcd = n_waves / 8;
  std::vector<WaveRR> desc((size_t)n_waves, WaveRR{0, 0, 0, -1});
  for (int x = 0; x < 8; ++x) {
    int a0 = x * per_xcd;
    while (a0 < (x + 1) * per_xcd) {
      if (!(wp[(size_t)a0] & kSellpFastWave)) { ++a0; continue; }
      int b0 = a0;
      while (b0 + 1 < (x + 1) * per_xcd && (wp[(size_t)b0 + 1] & kSellpFastWave)) ++b0;
      const int wn = b0 - a0 + 1;
      const int32_t S0 = wp[(size_t)a0] & (kSellpFastWave - 1), S1 = wp[(size_t)b0 + 1] & (kSellpFastWave - 1);
      const int n_pairs = (S1 - S0) / 2;
      if (wn >= 2 && n_pairs >= wn) {
        for (int r = 0; r < wn; ++r) {
          desc[(size_t)(a0 + r)] = WaveRR{S0 + 2 * r, 2 * wn, (n_pairs - r + wn - 1) / wn, -1};
          wp[(size_t)(a0 + r)] |= kSellpStrided;
        }
        if ((S1 - S0) & 1) desc[(size_t)b0].extra = S1 - 1;
      }
      a0 = b0 + 1;
    }
  }
  return desc;
}

// the tables of spmv_sellp_kernel for the SELL plan s; s.use_sellp is withdrawn where the waves cannot be balanced
inline SellpPlan plan_sellp(SellPlan &s, int64_t n_rows, const LayoutOptions &opt) {
  SellpPlan w;
  // as many workgroups as are resident at the kernel's register budget: one round
  if (opt.sell_grid <= 0) s.sell_grid = std::min(s.sell_grid, 256 * kSellpWaves);
  w.wave_ptr = balance_waves(s, opt.sellp_cost);
  if (w.wave_ptr.empty()) { s.use_sellp = false; return w; }
  if (!opt.disable_rowclass) sellp_row_classes(s, n_rows, w);
  if (!w.rowclass) { w.rowcls.clear(); w.ctab.clear(); return w; }
  // waves whose slices are all run-pattern slices need no slice metadata (flag in their wave_ptr entry)
  for (size_t wv = 0; wv + 1 < w.wave_ptr.size(); ++wv) {
    bool all = w.wave_ptr[wv] < w.wave_ptr[wv + 1];
    for (int32_t s2 = w.wave_ptr[wv]; s2 < w.wave_ptr[wv + 1] && all; ++s2) all = s.pat.spat[(size_t)s2] == s.sellp_pid;
    if (all) w.wave_ptr[wv] |= kSellpFastWave;
  }
  // The threshold is a MEASURED crossover in rows, not the L2 size: an XCD's eighth of x leaves its 4 MiB L2 at 4 Mi rows
  // (8 x 4 MiB / 8 B), and below ~3 Mi rows the contiguous order was never slower (121^3 = 1.77 M rows: x/8 = 1.8 MB per XCD
  // stays L2-resident, 17.0 us either way; 5.18 M rows: 50.7 -> 41.0 us; 201^3: PMC traffic 454 -> 197 MB).
  if (opt.sellp_rr == 1 || (opt.sellp_rr == 0 && n_rows > (int64_t)(3 << 20))) w.wave_rr = round_robin_waves(w.wave_ptr);
  return w;
}

// Grid of spmv_lattice_kernel: L.C columns x L.K plane steps are cut into S segments per XCD slab -- 2.5 - 3 marching
// waves per SIMD (measured at 121^3: 2 segments 13.0 us, 3 segments 11.8 us on a pure lattice) as long as a wave keeps >= 4
// steps; the register budget admits four waves per SIMD = 1024 workgroups: what the marching waves leave free goes to the
// rows outside the interior (per-entry gathers, ~10 x the cost of an interior row: about one chunk of 64 rows per wave).
// Sets L.S and L.fast_blocks; returns the number of workgroups for those rows.
inline int lattice_grid(const LayoutOptions &opt, LatticePlan &L, size_t n_gen) {
  const int slab = std::max(1, L.K / 8);
  int S = (int)std::max<int64_t>(1, (2816 / 8 + L.C / 2) / L.C);
  S = std::min(S, std::max(1, slab / 4));
  if (opt.lattice_segments > 0) S = std::min(opt.lattice_segments, slab);
  L.S = S;
  L.fast_blocks = 8 * ((S * L.C + 3) / 4);
  const int n_gen_blocks = n_gen == 0 ? 0 : (int)std::min<size_t>((size_t)std::max(64, 256 * kLatWavesPerSimd - L.fast_blocks), (n_gen + 3) / 4);
  // every workgroup writes one reduction partial: beyond kMaxPartials (lattices above ~360^3) the marching waves take
  // several (segment, column) pairs each
  L.fast_blocks = std::min(L.fast_blocks, (kMaxPartials - n_gen_blocks) / 8 * 8);
  if (opt.lattice_max_blocks >= 8) L.fast_blocks = std::min(L.fast_blocks, opt.lattice_max_blocks / 8 * 8);  // (tests: the multi-pass form on a small lattice)
  return n_gen_blocks;
}

// The window of rows whose stored columns are all owned lattice neighbours (27 offsets, every offset in range).  A
// lexicographic numbering gives one run over the whole interior; deal.II's cell-by-cell numbering (the host side's) breaks
// it at every plane: the first three lines of a plane (and the first three planes) are numbered in first-touch order.  So
// the interior is a WINDOW of W rows that repeats with the plane stride: rows R0 + k nxy + [0, W), k < K.
// False when the window holds less than half of the rows or the marching waves would read outside [0, n_rows).
inline bool lattice_window(const CsrView &A, bool debug, LatticePlan &L) {
  const int64_t n_rows = A.n_rows, nx = L.nx, nxy = L.nxy, reach = nxy + nx + 1;
  std::vector<char> row_ok((size_t)n_rows, 0);
  parallel_chunks(n_rows, [&](int64_t rb2, int64_t re2, int) {
    for (int64_t r2 = rb2; r2 < re2; ++r2) {
      // (lane 0 of a unit holds the two rows in front of the unit's first row: their lowest neighbour is row - 2 - reach;
      // the highest index read is n_rows + 1: every vector has two spare entries)
      bool ok = r2 >= reach + 2 && r2 + reach < n_rows;
      for (int64_t k = A.rowptr[r2]; k < A.rowptr[r2 + 1] && ok; ++k) {
        const int64_t t = (int64_t)A.col[k] - r2 + reach;
        ok = A.col[k] < n_rows && t >= 0 && t / nxy <= 2 && (t % nxy) / nx <= 2 && (t % nxy) % nx <= 2;
      }
      row_ok[(size_t)r2] = ok ? 1 : 0;
    }
  });
  int64_t best_b = 0, best_e = 0, cur_b = -1;  // longest run of good rows
  for (int64_t r2 = 0; r2 <= n_rows; ++r2) {
    const bool ok = r2 < n_rows && row_ok[(size_t)r2];
    if (ok && cur_b < 0) cur_b = r2;
    if (!ok && cur_b >= 0) {
      if (r2 - cur_b > best_e - best_b) { best_b = cur_b; best_e = r2; }
      cur_b = -1;
    }
  }
  int64_t R0 = best_b, R1 = best_e, Wd = std::min<int64_t>(best_e - best_b, nxy), Kp = 0;
  if (best_e - best_b >= nxy) {
    Kp = (best_e - best_b + nxy - 1) / nxy;  // the last plane step may be cut by R1
  } else if (Wd > 0) {
    std::vector<int32_t> bad_before((size_t)n_rows + 1, 0);  // prefix count of bad rows
    for (int64_t r2 = 0; r2 < n_rows; ++r2) bad_before[(size_t)r2 + 1] = bad_before[(size_t)r2] + (row_ok[(size_t)r2] ? 0 : 1);
    auto window_ok = [&](int64_t b2) { return b2 >= 0 && b2 + Wd <= n_rows && bad_before[(size_t)(b2 + Wd)] == bad_before[(size_t)b2]; };
    int64_t lo = best_b, hi = best_b;
    while (window_ok(lo - nxy)) lo -= nxy;
    while (window_ok(hi + nxy)) hi += nxy;
    R0 = lo; Kp = (hi - lo) / nxy + 1; R1 = hi + Wd;
  }
  const int64_t n_fast = Wd == nxy ? R1 - R0 : Kp * Wd;
  if (debug)
    std::fprintf(stderr, "[gmg]   lattice rows: longest run [%lld, %lld) -> window of %lld rows x %lld planes from row %lld: %lld of %lld rows\n", (long long)best_b, (long long)best_e,
                 (long long)Wd, (long long)Kp, (long long)R0, (long long)n_fast, (long long)n_rows);
  L.R0 = R0; L.R1 = R1; L.W = Wd; L.K = (int)Kp; L.fast_rows = n_fast;
  // what the marching waves read: rows R0 - 2 - reach .. R1 + 1 + reach - 1 of x (lane 0 / lane 63 of a unit sit two
  // rows outside it): checked here, once, instead of trusting the row test above
  const bool reads_inside = R0 - 2 - reach >= 0 && R1 + reach <= n_rows;
  return n_fast >= n_rows / 2 && Wd >= 2 && reads_inside;
}

// Classes of the window's rows: the 27 value codes of a row by offset position (0 = +0.0 where the row stores nothing), read
// from the CSR in parallel and merged in chunk order.  False (L.classes < 0) beyond kLatMaxClasses.
inline bool lattice_classes(const CsrView &A, const ValueDict &D, LatticePlan &L) {
  using Key = std::array<uint8_t, 27>;
  const int64_t R0 = L.R0, nx = L.nx, nxy = L.nxy, reach = nxy + nx + 1;
  const int nt = host_threads();
  std::vector<std::vector<Key>> local_keys((size_t)nt);
  std::vector<std::array<int64_t, 2>> local_rng((size_t)nt, {0, 0});
  std::vector<std::vector<int32_t>> local_id((size_t)nt);
  parallel_chunks(L.R1 - R0, [&](int64_t cb, int64_t ce, int t) {
    std::map<Key, int> M;
    local_rng[(size_t)t] = {R0 + cb, R0 + ce};
    local_id[(size_t)t].resize((size_t)(ce - cb));
    for (int64_t r2 = R0 + cb; r2 < R0 + ce; ++r2) {
      Key key;
      key.fill(0);
      if (!L.fast(r2)) { local_id[(size_t)t][(size_t)(r2 - R0 - cb)] = -1; continue; }
      for (int64_t k = A.rowptr[r2]; k < A.rowptr[r2 + 1]; ++k) {
        const int64_t t2 = (int64_t)A.col[k] - r2 + reach;
        key[(size_t)((t2 / nxy) * 9 + ((t2 % nxy) / nx) * 3 + (t2 % nxy) % nx)] = D.lookup(A.val[k]);
      }
      auto ins = M.emplace(key, (int)M.size());
      if (ins.second) local_keys[(size_t)t].push_back(key);
      local_id[(size_t)t][(size_t)(r2 - R0 - cb)] = ins.first->second;
    }
  });
  L.rowcls.assign((size_t)A.n_rows, 0);
  std::map<Key, int> cls_of;
  for (int t = 0; t < nt; ++t) {
    std::vector<int> remap(local_keys[(size_t)t].size(), 0);
    for (size_t q = 0; q < local_keys[(size_t)t].size(); ++q) {
      auto ins = cls_of.emplace(local_keys[(size_t)t][q], (int)cls_of.size());
      if (ins.second) {
        if ((int)cls_of.size() > kLatMaxClasses) { L.classes = -(int)cls_of.size(); return false; }
        for (int j = 0; j < 27; ++j) L.ctab.push_back(D.dict[local_keys[(size_t)t][q][(size_t)j]]);
      }
      remap[q] = ins.first->second;
    }
    for (int64_t r2 = local_rng[(size_t)t][0]; r2 < local_rng[(size_t)t][1]; ++r2) {
      const int32_t id = local_id[(size_t)t][(size_t)(r2 - local_rng[(size_t)t][0])];
      if (id >= 0) L.rowcls[(size_t)r2] = (uint8_t)remap[(size_t)id];
    }
  }
  L.classes = (int)cls_of.size();
  return !cls_of.empty();
}

// Lattice interior (gmg_lattice.hpp): the nine runs are the (dz, dy) lines of an nx x ny x nz vertex lattice numbered
// lexicographically -> the rows whose columns are all owned lattice neighbours are walked plane by plane from a class
// table; everything else stays on the SELL streams.
inline LatticePlan plan_lattice(const CsrView &A, const SellPlan &s, const LayoutOptions &opt) {
  LatticePlan L;
  const int64_t n_rows = A.n_rows;
  L.nx = s.sellp_centre[5] - s.sellp_centre[4]; L.nxy = s.sellp_centre[7] - s.sellp_centre[4];
  bool lat_ok = L.nx >= 3 && L.nxy >= 3 * L.nx;
  for (int u = 0; u < 9 && lat_ok; ++u) lat_ok = s.sellp_centre[u] == (u / 3 - 1) * L.nxy + (u % 3 - 1) * L.nx;
  const int64_t reach = L.nxy + L.nx + 1;
  if (lat_ok && n_rows > 4 * reach + 256 && lattice_window(A, opt.debug, L) && lattice_classes(A, s.vd, L)) {
    for (int64_t sl = 0; sl < s.n_slices; ++sl) {
      bool all_fast = true;  // a slice with any row outside the interior is served from the streams (its interior rows masked)
      for (int64_t r2 = sl * 64; r2 < A.slice_end(sl) && all_fast; ++r2) all_fast = L.fast(r2);
      if (all_fast) continue;
      L.gen.push_back((int32_t)sl);
      L.gen_bytes += (int64_t)(s.slice_ptr[(size_t)sl + 1] - s.slice_ptr[(size_t)sl]) * 256 * (1 + (s.pat.spat[(size_t)sl] >= 0 ? 0 : (s.s.col16 ? 2 : 4))) + 8;
    }
    L.C = (int)((L.W + kLatRowsPerUnit - 1) / kLatRowsPerUnit);
    const int gen_blocks = lattice_grid(opt, L, L.gen.size());
    L.grid = L.fast_blocks + gen_blocks;
    L.planned = true;
    L.built = L.grid <= kMaxPartials;
    if (opt.debug && L.built)
      std::fprintf(stderr, "[gmg]   lattice interior: nx %d nxy %d rows [%d, %d) of %lld, %d classes, %d columns x %d steps, %d segments per XCD slab, grid %d + %d, %d slices outside\n",
                   (int)L.nx, (int)L.nxy, (int)L.R0, (int)L.R1, (long long)n_rows, L.classes, L.C, L.K, L.S, L.fast_blocks, gen_blocks, (int)L.gen.size());
  }
  if (opt.debug && !L.built)
    std::fprintf(stderr, "[gmg]   lattice interior not used: nx %lld nxy %lld lattice-shaped %d rows %lld reach %lld classes %d\n", (long long)L.nx, (long long)L.nxy, (int)lat_ok,
                 (long long)n_rows, (long long)reach, L.classes);
  return L;
}

// ---------------------------------------------------------------- hybrid SELL / CSR

// Hybrid layout for an operator the SELL rule refuses as a whole: slice by slice, a slice is
// regular when its own padding passes the same 12 % bound (padded entries <= 1.12 x its entries; the width is that of its
// column pattern where it has one).  Regular slices go into SELL streams -- 8-bit value codes if the REGULAR slices hold
// <= 256 distinct values, no columns for pattern slices, 32-bit columns otherwise --, the rows of the other slices are
// cut into row-window tiles of the CSR copy.  Not built (the operator stays as it is) when the regular slices hold less
// than half of the entries: the product then streams more than 3/4 of the CSR bytes anyway.
struct HybridPlan {
  bool built = false;
  std::vector<int32_t> qptr, reg, tiles;  // quads of every slice / the regular slices / (first, end) rows of the CSR tiles
  Patterns pat;
  ValueDict vd;
  SellStreams s;
  int n_slices = 0, n_tiles = 0, tile_blocks = 0, sell_blocks = 0, grid = 0;
  int64_t stream_bytes = 0, csr_bytes = 0;  // bytes one product streams: SELL part, CSR part
};
inline HybridPlan plan_hybrid(const CsrView &A, const SliceInfo &I, const LayoutOptions &opt) {
  HybridPlan H;
  const int64_t n_slices = A.n_slices(), nnz = A.nnz();
  H.qptr.assign((size_t)n_slices + 1, 0);
  std::vector<int64_t> irr_runs;  // [first, end) slices of every run of irregular slices
  int64_t quads = 0, nnz_reg = 0, n_irr = 0;
  for (int64_t sl = 0; sl < n_slices; ++sl) {
    const int64_t ent = A.rowptr[A.slice_end(sl)] - A.rowptr[sl * 64];
    if ((double)(I.quads(sl) * 256) <= 1.12 * (double)ent) {
      H.reg.push_back((int32_t)sl);
      quads += I.quads(sl);
      nnz_reg += ent;
    } else {
      if (irr_runs.empty() || irr_runs.back() != sl) { irr_runs.push_back(sl); irr_runs.push_back(sl); }
      irr_runs.back() = sl + 1;
      ++n_irr;
    }
    H.qptr[(size_t)sl + 1] = (int32_t)quads;
  }
  if (H.reg.empty() || n_irr == 0 || 2 * nnz_reg < nnz || quads == 0 || quads * 256 >= ((int64_t)1 << 31)) {
    if (opt.debug)
      std::fprintf(stderr, "[gmg]   hybrid not built: %lld of %lld slices regular, %lld of %lld entries in them\n", (long long)H.reg.size(), (long long)n_slices,
                   (long long)nnz_reg, (long long)nnz);
    return H;
  }
  const Slices regular{&H.reg, n_slices};
  H.pat = assign_patterns(I, regular);
  H.vd = value_dictionary(A, regular, !opt.disable_compression);
  H.s = pack_slices(A, regular, H.qptr, H.pat, H.vd, false, nullptr);
  for (size_t i = 0; i < irr_runs.size(); i += 2) {  // row-window tiles over the runs of irregular slices
    const std::vector<int32_t> b = window_tiles(A.rowptr, irr_runs[i] * 64, std::min<int64_t>(A.n_rows, irr_runs[i + 1] * 64));
    for (size_t q = 0; q + 1 < b.size(); ++q) { H.tiles.push_back(b[q]); H.tiles.push_back(b[q + 1]); }
  }
  H.n_slices = (int)n_slices;
  H.n_tiles = (int)(H.tiles.size() / 2);
  // as many workgroups of each kind as are resident at 4 per CU (the 32 KiB row window): two rounds at the most
  H.tile_blocks = 8 * (int)std::min<int64_t>(128, std::max<int64_t>(1, (H.n_tiles + 7) / 8));
  H.sell_blocks = 8 * (int)std::min<int64_t>(128, std::max<int64_t>(1, ((int64_t)H.reg.size() + 63) / 64));
  H.grid = H.tile_blocks + H.sell_blocks;
  int64_t streamed_cols = 0;
  for (int32_t sl : H.reg)
    if (H.pat.spat[(size_t)sl] < 0) streamed_cols += (int64_t)(H.qptr[(size_t)sl + 1] - H.qptr[(size_t)sl]) * 256;
  H.stream_bytes = quads * 256 * (H.vd.val8 ? 1 : 8) + 4 * streamed_cols + 12 * (int64_t)H.reg.size();
  H.csr_bytes = 12 * (nnz - nnz_reg) + 8 * (int64_t)H.n_tiles + 4 * ((int64_t)n_irr * 64 + H.n_tiles);
  H.built = true;
  if (opt.debug)
    std::fprintf(stderr, "[gmg]   layout hybrid: %d of %d slices regular (%d pattern slices, %zu patterns), %lld of %lld entries in them padded to %lld, val8 %d (%zu values); "
                 "%d csr tiles; bytes per product: sell %lld + csr %lld (csr alone %lld); grid %d + %d\n", (int)H.reg.size(), H.n_slices, H.pat.n_pattern_slices, H.pat.list.size(),
                 (long long)nnz_reg, (long long)nnz, (long long)(quads * 256), (int)H.vd.val8, H.vd.n_values, H.n_tiles, (long long)H.stream_bytes, (long long)H.csr_bytes,
                 (long long)(12 * nnz + 4 * (A.n_rows + 1)), H.tile_blocks, H.sell_blocks);
  return H;
}

// ---------------------------------------------------------------- the whole plan

struct StreamPlan {  // at most one of sell and hyb is built; sellp and lat go with sell
  SellPlan sell;
  SellpPlan sellp;
  LatticePlan lat;
  HybridPlan hyb;
};

// SELL-64 streams when the rows are regular enough (level-0 lattice, active-mesh matrix): padded entries <= 1.12 nnz
inline bool plan_sell(const CsrView &A, const SliceInfo &I, const LayoutOptions &opt, PhaseLog &phase, SellPlan &s) {
  const Slices all{nullptr, A.n_slices()};
  s.n_slices = A.n_slices();
  s.slice_ptr.assign((size_t)s.n_slices + 1, 0);
  for (int64_t sl = 0; sl < s.n_slices; ++sl) s.slice_ptr[(size_t)sl + 1] = (int32_t)(s.quads += I.quads(sl));
  if (!(s.quads * 256 <= (int64_t)(1.12 * (double)A.nnz()) && s.quads * 256 < ((int64_t)1 << 31))) return false;
  s.pat = assign_patterns(I, all);
  phase("patterns");
  s.vd = value_dictionary(A, all, !opt.disable_compression);
  phase("dictionary");
  const bool col16 = slice_bases(A, s.slice_base) && !opt.disable_compression;
  s.s = pack_slices(A, all, s.slice_ptr, s.pat, s.vd, col16, s.slice_base.data());
  if (s.pat.n_pattern_slices > 0) pick_run_pattern(s, opt);
  phase("sell pack+copy");
  // one wave per >= 1 slice; at most kMaxPartials workgroups (one reduction partial each)
  const int per_xcd = (int)((s.n_slices + 7) / 8);
  s.sell_grid = 8 * std::min(kMaxPartials / 8, std::max(1, (per_xcd + 3) / 4));
  if (opt.sell_grid > 0) s.sell_grid = std::max(8, opt.sell_grid / 8 * 8);
  return s.built = true;
}

// The streams of a validated operator beyond its CSR copy.  The SELL kernels gather through 32-bit byte offsets (c << 3
// into a 2 GiB buffer descriptor): columns beyond 2^28 stay on the CSR row-window kernel.  allow_hybrid: the system matrix
// only (its product is the one that is HBM bound).
inline StreamPlan plan_streams(const CsrView &A, const LayoutOptions &opt, bool allow_hybrid, PhaseLog &phase) {
  StreamPlan P;
  if (!(A.n_rows >= 1024 && !opt.disable_sell && A.n_cols < ((int64_t)1 << 28))) return P;
  const SliceInfo I = analyse_slices(A, !opt.disable_patterns && A.n_cols >= A.n_rows);
  if (plan_sell(A, I, opt, phase, P.sell)) {
    if (P.sell.use_sellp) P.sellp = plan_sellp(P.sell, A.n_rows, opt);
    // the lattice interior only needs the rows whose columns are owned (< n_rows): any n_cols >= n_rows qualifies
    if (P.sell.vd.val8 && !opt.disable_lattice && P.sell.sellp_pid >= 0 && A.n_cols >= A.n_rows && A.n_rows < ((int64_t)1 << 28)) {
      P.lat = plan_lattice(A, P.sell, opt);
      phase("lattice plan");
    }
  } else if (allow_hybrid && !opt.disable_hybrid) {
    phase("patterns");
    P.hyb = plan_hybrid(A, I, opt);
    phase("hybrid pack+copy");
  }
  return P;
}

}  // namespace gmg
