// ssor_plan_replay.cc -- the host-side planner of the SSOR sweep (csrc/gmg_sgs_layout.hpp) without a GPU.  For small matrices
// the program plans with the header and then works from the plan's arrays alone, with the record layouts restated here from
// the comments in gmg_sgs.hpp and gmg_sgs_phase.hpp:
//   (a) every record is decoded (head, T1, T2; one-wave: sub-step by sub-step), slot addresses resolved to rows by following
//       which row owns a slot at that step: it must give exactly the row's pruned entries of that direction, in ascending
//       column order, value bits included; every padding entry has value +0.0 and the row's own address;
//   (b) every slot a record reads holds the intended row at that step, and that row was updated earlier in the same sweep or
//       belongs to the range's working set; what the dependent phase does not gather was updated long enough before; a slot
//       changes hands no sooner than the hold of two steps; rpos_f / rpos_b, aux, the block table and the next-block words of
//       the headers are consistent and inside the stream; check_sweep_plan accepts the plan and rejects a copy with one aux
//       word, one slot address or one backward row pushed out of range;
//   (c) one forward plus one backward sweep is replayed from the records with the y slots as an array -- including the forward
//       prefix stored through aux into the stream and read by the backward record -- and must equal, bit for bit, a plain
//       block SSOR sweep over the CSR written below with the same left-to-right summation; rows without couplings come from
//       iso_diag / iso_invd.
// What the records of a built plan carry could so far only be read back from a context on a GPU (tests/test_gpu_ssor_sliding.py:
// "the plan needs a context"); tests/test_ssor_slots_cpu.py checks the slot allocator alone.  Every case asserts the path it was
// written for.  Driven by tests/test_ssor_plan_cpu.py; exit status 0 = every requirement held.
//
// Second mode, `ssor_plan_replay FILE [mutate=KEY:stride|t1 ...]` (tests/test_ssor_shapes_cpu.py, tests/test_gpu_ssor_shapes.py): FILE
// holds one CSR matrix, a block count or the caller's block boundaries, and option sets by the library's option names (the format:
// read_case below).  Every set is planned and put through the same run(); per set the program prints
//   plan  SET phased dep reg retried ranges self-contained-ranges steps shape-switches min-rows max-rows live-forward live-backward failures
//   shape SET g l1 l2 backward self-contained steps        (from blk_tab and pranges: one line per shape key, direction and plan kind)
// Each mutate= argument is a pass of its own, announced by a line `mutation KEY KIND`; it decodes the records of ONE shape key wrongly -- a stride 32 bytes too long, or the end of T1 four slots late -- as a kernel
// body with a wrong constant would: the replay must notice it in every plan that holds the shape and in no other.
#include "gmg_sgs_layout.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>

using namespace gmg;

namespace {

int g_failures = 0;
std::string g_case;
int g_mut_key = -1;    // file mode: the shape key whose records are decoded wrongly (-1: none)
char g_mut_kind = 0;   // 's': stride + 32; 't': T1 ends four slots late
#define REQUIRE(cond)                                                                                    \
  do {                                                                                                   \
    if (!(cond) && ++g_failures <= 30) std::fprintf(stderr, "FAIL [%s] line %d: %s\n", g_case.c_str(), __LINE__, #cond); \
  } while (0)

uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double real() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }
};

struct Csr {
  int64_t n = 0;
  std::vector<int64_t> rp = {0};
  std::vector<int32_t> col;
  std::vector<double> val;
  void add_row(const std::vector<std::pair<int32_t, double>> &e) {
    for (const auto &x : e) { col.push_back(x.first); val.push_back(x.second); }
    rp.push_back((int64_t)col.size());
    ++n;
  }
};

// rows = grid points of an nx x ny x nz box, columns = the neighbours within `reach` per axis that `keep` lets through,
// ascending; diagonal 6 + noise, off-diagonals -1 + noise (all distinct: a decoded entry identifies its source)
template <class Keep>
Csr stencil(int nx, int ny, int nz, Keep keep, uint64_t seed) {
  Csr A;
  Rng rng{seed};
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        std::vector<std::pair<int32_t, double>> e;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int X = x + dx, Y = y + dy, Z = z + dz;
              if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz || !keep(dx, dy, dz)) continue;
              const bool diag = !dx && !dy && !dz;
              e.emplace_back((Z * ny + Y) * nx + X, (diag ? 6.0 : -1.0) + 0.25 * rng.real());
            }
        A.add_row(e);
      }
  return A;
}
Csr chain(int n) { return stencil(n, 1, 1, [](int, int, int) { return true; }, 11); }
Csr five_point(int nx, int ny) { return stencil(nx, ny, 1, [](int dx, int dy, int) { return !dx || !dy; }, 12); }
Csr box27(int nx) { return stencil(nx, nx, nx, [](int, int, int) { return true; }, 13); }
Csr pairs(int n_pairs) {  // independent 2 x 2 blocks: two stages of n_pairs rows each
  Csr A;
  Rng rng{14};
  for (int p = 0; p < n_pairs; ++p) {
    A.add_row({{2 * p, 4.0 + rng.real()}, {2 * p + 1, -1.0 + 0.25 * rng.real()}});
    A.add_row({{2 * p, -1.0 + 0.25 * rng.real()}, {2 * p + 1, 4.0 + rng.real()}});
  }
  return A;
}
Csr zeros_and_lone_rows() {  // 5-point 9 x 9 with stored zeros (every 5th off-diagonal), every 7th row diagonal-only, rows 38 and 40 without a stored diagonal
  Csr A, B = five_point(9, 9);
  for (int64_t i = 0; i < B.n; ++i) {
    std::vector<std::pair<int32_t, double>> e;
    for (int64_t k = B.rp[(size_t)i]; k < B.rp[(size_t)i + 1]; ++k) {
      const int32_t c = B.col[(size_t)k];
      if ((i % 7 == 3 || c % 7 == 3) && c != i) continue;
      if ((i == 40 || i == 38) && c == i) continue;  // (row 40 stays coupled, row 38 is left without any entry)
      e.emplace_back(c, c != i && k % 5 == 0 ? (k % 10 ? 0.0 : -0.0) : B.val[(size_t)k]);
    }
    A.add_row(e);
  }
  return A;
}
Csr arrow(int n, int reach) {  // tridiagonal, and the last row (and column) couples to the `reach` rows before it
  Csr A;
  Rng rng{15};
  for (int i = 0; i < n; ++i) {
    std::vector<std::pair<int32_t, double>> e;
    for (int c = 0; c < n; ++c)
      if (std::abs(c - i) <= 1 || (i == n - 1 && c >= n - 1 - reach) || (c == n - 1 && i >= n - 1 - reach)) e.emplace_back(c, (c == i ? 8.0 : -0.1) + 0.05 * rng.real());
    A.add_row(e);
  }
  return A;
}

// ---- the record layouts, restated --------------------------------------------------------------------------------------------
// Four-wave (gmg_sgs_phase.hpp): a step's block = 16-byte header {-, bytes of the block four steps on (0: none), its offset in the
// range's stream, that step's word}, then one record per row: +0 r, +8 1 / a_ii, +16 prefix, +24 u32 LDS address of the row's y,
// +28 u32 aux, +32 head values [8 G], tail values [L1 + L2], head addresses u32 [8 G], tail addresses u32 [L1 + L2]; stride
// 32 + 96 G + 12 L rounded up to an odd multiple of 16.  Word: shape key | rows << 8 | T1 slots in use << 16, key = 64 G + 8 (L1 / 4)
// + L2 / 8.  Field-major (dep, reg): unit k (16 bytes) of row u at block + 16 + (k * rows + u) * 16.
// One-wave (gmg_sgs.hpp): header {u16 rows, u16 flags (1 first, 2 last sub-step of its step), u16 next rows, u16 -, u32 advance, u32
// next raw}; record: the same first 32 bytes, +32 a[8 g], then u32 addresses [8 g]; stride 96 g + 48.
int ph_stride_restated(int g, int l) { const int s = 32 + 96 * g + 12 * l; return (s / 16) % 2 ? s : s + 16; }
int sw_stride_restated(int g) { return 96 * g + 48; }

struct Rec {
  char *blk = nullptr;
  int64_t blk_pos = 0;
  int nrows = 0, u = 0, stride = 0;
  bool fieldmajor = false, first = true, last = true;  // (one-wave: first / last sub-step of the row)
  int n_head = 0, l1 = 0, l2 = 0;
  int row = -1;
  char *at(int o) const { return fieldmajor ? blk + 16 + ((size_t)(o / 16) * nrows + u) * 16 + o % 16 : blk + 16 + (size_t)u * stride + o; }
  int64_t pos(int o) const { return blk_pos + (at(o) - blk); }
  double f64(int o) const { double v; std::memcpy(&v, at(o), 8); return v; }
  uint32_t u32(int o) const { uint32_t v; std::memcpy(&v, at(o), 4); return v; }
  int n_ent() const { return n_head + l1 + l2; }
  double value(int e) const { return f64(32 + 8 * e); }
  uint32_t addr(int e) const { return u32(32 + 8 * n_ent() + 4 * e); }
  uint32_t my() const { return u32(24); }
  uint32_t aux() const { return u32(28); }
};
struct Range {
  bool backward = false, self = false;
  int ws_off = 0, n_own = 0, n_ws = 0, late = 1;
  std::vector<std::vector<Rec>> steps;  // (one-wave: sub-steps)
};

// (a), structure: the ranges, steps and records of a plan over the stream copy S; headers, block table and sizes checked
std::vector<Range> decode(const SsorSweepPlan &P, std::vector<char> &S) {
  std::vector<Range> out;
  const bool fm = P.dep || P.reg;
  for (const PhRange &R : P.pranges) {
    Range D;
    D.backward = R.backward != 0; D.self = R.pad0[0] == 1; D.ws_off = R.ws_off; D.n_own = R.n_own; D.n_ws = R.n_ws; D.late = P.dep ? 3 : 1;
    REQUIRE(R.stream_off >= 0 && R.stream_off % 1024 == 0 && (uint64_t)R.stream_off + R.stream_bytes <= S.size());
    REQUIRE((size_t)R.blk_tab + (size_t)R.n_steps <= P.blk_tab.size());
    if (D.self) REQUIRE(R.n_own == 0 && R.n_ws == 0 && R.own_dir == 0 && R.pad0[1] <= P.y_slots);
    for (int q = 0; q < R.n_steps; ++q) {
      const PhBlkEntry e = P.blk_tab[(size_t)R.blk_tab + (size_t)q];
      const int key = (int)(e.word & 255u), rows = (int)(e.word >> 8 & 255u), t1 = (int)(e.word >> 16);
      const int g = key >> 6, l1 = 4 * (key >> 3 & 7), l2 = 8 * (key & 7), stride = ph_stride_restated(g, l1 + l2);
      REQUIRE(g <= 3 && l1 >= 4 && l1 <= 28 && l2 <= 24 && 8 * g + l1 + l2 <= 36 && t1 >= 4 && t1 <= l1 && t1 % 4 == 0);
      REQUIRE(rows >= 1 && rows <= 32 && e.bytes == 16u + (uint32_t)rows * (uint32_t)stride && e.bytes <= 16384u && e.off % 16 == 0 && e.pad == 0);
      REQUIRE((uint64_t)e.off + e.bytes + 1008 <= R.stream_bytes);  // (the copies read whole KB)
      if (q > 0) REQUIRE(e.off >= P.blk_tab[(size_t)R.blk_tab + (size_t)q - 1].off + P.blk_tab[(size_t)R.blk_tab + (size_t)q - 1].bytes);
      if (key == g_mut_key) REQUIRE(g_mut_kind == 's' || g_mut_kind == 't');
      if (g_failures) return out;
      int l1d = l1, l2d = l2, strided = stride;  // what the records are decoded with
      if (key == g_mut_key && g_mut_kind == 's') strided += 32;
      if (key == g_mut_key && g_mut_kind == 't') { l1d += 4; l2d = std::max(0, l2 - 4); }
      REQUIRE(e.bytes == 16u + (uint32_t)rows * (uint32_t)strided);
      if (g_failures) return out;
      uint32_t h[4];
      std::memcpy(h, S.data() + R.stream_off + e.off, 16);
      if (q + 4 < R.n_steps) {
        const PhBlkEntry nx = P.blk_tab[(size_t)R.blk_tab + (size_t)q + 4];
        REQUIRE(h[1] == nx.bytes && h[2] == nx.off && h[3] == nx.word);
      } else REQUIRE(h[1] == 0 && h[2] == 0 && h[3] == 0);
      D.steps.emplace_back();
      for (int u = 0; u < rows; ++u) {
        Rec r;
        r.blk = S.data() + R.stream_off + e.off; r.blk_pos = R.stream_off + e.off; r.nrows = rows; r.u = u; r.stride = strided; r.fieldmajor = fm;
        r.n_head = 8 * g; r.l1 = l1d; r.l2 = l2d;
        // T1 slots beyond those in use are padding (the dependent phase stops there)
        for (int k = 8 * g + t1; k < 8 * g + l1d; ++k) REQUIRE(bits_of(r.value(k)) == 0 && r.addr(k) == r.my());
        D.steps.back().push_back(r);
      }
    }
    out.push_back(D);
  }
  for (const SwRange &R : P.ranges) {
    Range D;
    D.backward = R.backward != 0; D.ws_off = R.ws_off; D.n_own = R.n_own; D.n_ws = R.n_ws;
    REQUIRE(R.stream_off >= 0 && R.stream_off % 4096 == 0 && R.stream_bytes % 4096 == 0 && (uint64_t)R.stream_off + (uint64_t)R.stream_bytes <= S.size());
    REQUIRE(R.groups >= 1 && R.groups <= 4);
    const int stride = sw_stride_restated(R.groups);
    int64_t pos = 0;
    uint32_t want_raw = (uint32_t)R.first_raw;
    int want_rows = R.first_nrows;
    for (int s = 0; s < R.n_steps && !g_failures; ++s) {
      REQUIRE(pos + 16 <= R.stream_bytes);
      SwStepHdr h;
      std::memcpy(&h, S.data() + R.stream_off + pos, 16);
      const uint32_t raw = 16u + (uint32_t)h.nrows * (uint32_t)stride;
      REQUIRE(h.nrows >= 1 && h.nrows <= 64 && raw == want_raw && h.nrows == want_rows && raw <= 8192u);
      REQUIRE(pos % 32768 + raw <= 32768 && pos + raw <= R.stream_bytes && h.advance >= raw);
      REQUIRE(s + 1 < R.n_steps ? h.next_raw != 0 : h.next_raw == 0);
      D.steps.emplace_back();
      for (int u = 0; u < h.nrows; ++u) {
        Rec r;
        r.blk = S.data() + R.stream_off + pos; r.blk_pos = R.stream_off + pos; r.nrows = h.nrows; r.u = u; r.stride = stride;
        r.n_head = 8 * R.groups; r.first = h.flags & 1; r.last = h.flags & 2;
        D.steps.back().push_back(r);
      }
      want_raw = h.next_raw; want_rows = h.next_nrows;
      pos += h.advance;
    }
    out.push_back(D);
  }
  return out;
}

struct Want { bool planned = true, phased = true, dep = false, reg = false; const char *generic = nullptr; bool any_kind = false; };  // any_kind: whichever sweep the planner chose

// Plans A with block boundaries (the caller's, balanced cuts or equal runs), checks the plan and replays it.  Returns the plan.
SsorSweepPlan run(const std::string &name, const Csr &A, const SsorPlanOptions &opt, const Want &want, const std::vector<int64_t> *explicit_rows = nullptr,
                  bool balanced = false, int blocks = 1, bool *retried = nullptr) {
  g_case = name;
  const int64_t n = A.n;
  const std::vector<int32_t> block_row = ssor_block_rows(n, A.rp.data(), A.col.data(), A.val.data(), explicit_rows, balanced, blocks);
  const int n_blocks = (int)block_row.size() - 1;
  REQUIRE(block_row.front() == 0 && block_row.back() == n);
  SsorSweepPlan P;
  ssor_sweep_plan(opt, n, A.rp.data(), A.col.data(), A.val.data(), block_row, true, P);
  if (retried) *retried = P.outcome == kSsorOneWave;
  if (P.outcome == kSsorOneWave) ssor_sweep_plan(opt, n, A.rp.data(), A.col.data(), A.val.data(), block_row, false, P);
  if (!want.planned) {
    REQUIRE(P.outcome == kSsorGeneric && std::string(P.message) == want.generic);
    return P;
  }
  REQUIRE(P.outcome == kSsorPlanned);
  if (P.outcome != kSsorPlanned) return P;
  if (!want.any_kind) REQUIRE(P.phased == want.phased && P.dep == want.dep && P.reg == want.reg);
  REQUIRE(check_sweep_plan(P, n) == nullptr);
  REQUIRE((int)P.block_rng.size() == n_blocks + 1 && P.block_rng.back() == P.n_ranges() && (int64_t)P.row_ci.size() == n);
  REQUIRE(P.y_slots % 2 == 0 && P.y_slots * 8 <= P.lds_bytes && P.lds_bytes <= 160 * 1024);

  // the generic plan's tables cover every row once, stage by stage (stored zeros couple there)
  const SsorGenericPlan GP = ssor_generic_plan(n, A.rp.data(), A.col.data(), block_row);
  REQUIRE((int)GP.block_stage.size() == n_blocks + 1 && (int64_t)GP.stage_ptr.size() == GP.block_stage.back() + n_blocks);
  {
    std::vector<int> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) seen[(size_t)GP.stage_rows[(size_t)i]]++;
    for (int64_t i = 0; i < n; ++i) REQUIRE(seen[(size_t)i] == 1);
  }

  // ---- reference: the pruned entries (stored value != 0, column inside the block) and a plain block SSOR sweep
  const double omega = 0.7;
  Rng rng{99};
  std::vector<double> r((size_t)n), y_ref((size_t)n, 0.0), prefix_ref((size_t)n, 0.0), invd((size_t)n, 1.0);
  std::vector<int> block_of((size_t)n, 0);
  for (double &x : r) x = rng.real();
  using Entry = std::pair<int32_t, uint64_t>;
  auto entries = [&](int64_t i, int dir) {  // the row's pruned entries of a direction: forward c < i, backward c >= i
    std::vector<Entry> e;
    const int64_t rb = block_row[(size_t)block_of[(size_t)i]], re = block_row[(size_t)block_of[(size_t)i] + 1];
    for (int64_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) {
      const int64_t c = A.col[(size_t)k];
      if (c >= rb && c < re && A.val[(size_t)k] != 0.0 && (dir == 0 ? c < i : c >= i)) e.emplace_back((int32_t)c, bits_of(A.val[(size_t)k]));
    }
    return e;
  };
  for (int b = 0; b < n_blocks; ++b) {
    const int64_t rb = block_row[(size_t)b], re = block_row[(size_t)b + 1];
    for (int64_t i = rb; i < re; ++i) {
      block_of[(size_t)i] = b;
      for (int64_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k)
        if (A.col[(size_t)k] == i) invd[(size_t)i] = 1.0 / A.val[(size_t)k];
    }
    for (int64_t i = rb; i < re; ++i) {
      double acc = 0.0;
      for (const Entry &e : entries(i, 0)) { double v; std::memcpy(&v, &e.second, 8); acc += v * y_ref[(size_t)e.first]; }
      prefix_ref[(size_t)i] = acc;
      y_ref[(size_t)i] = 0.0 + (omega * (r[(size_t)i] - acc)) * invd[(size_t)i];
    }
    for (int64_t i = re - 1; i >= rb; --i) {
      double acc = prefix_ref[(size_t)i];
      for (const Entry &e : entries(i, 1)) { double v; std::memcpy(&v, &e.second, 8); acc += v * y_ref[(size_t)e.first]; }
      y_ref[(size_t)i] = y_ref[(size_t)i] + (omega * (r[(size_t)i] - acc)) * invd[(size_t)i];
    }
  }

  // ---- the numbering of the coupled rows, rpos_*, and the pre-pass: r into the stream, rows without couplings in closed form
  std::vector<char> S = P.stream;
  const size_t nc = P.ci_row.size();
  REQUIRE(P.rpos_f.size() == nc && P.rpos_b.size() == nc);
  std::vector<double> y((size_t)n, std::nan("")), ycur(nc, 0.0);
  std::map<int64_t, int32_t> row_at[2];  // position (doubles) of an r field -> the row it belongs to
  for (int64_t i = 0; i < n; ++i) {
    const int32_t ci = P.row_ci[(size_t)i];
    bool coupled = false;
    for (int dir = 0; dir < 2; ++dir)
      for (const Entry &e : entries(i, dir)) coupled = coupled || e.first != i;
    for (int64_t j = block_row[(size_t)block_of[(size_t)i]]; j < block_row[(size_t)block_of[(size_t)i] + 1] && !coupled; ++j)
      for (const Entry &e : entries(j, j < i ? 1 : 0)) coupled = coupled || (j != i && e.first == i);
    REQUIRE((ci >= 0) == coupled);
    if (ci < 0) {
      const double y1 = 0.0 + (omega * (r[(size_t)i] - 0.0)) * P.iso_invd[(size_t)i];
      const double acc = 0.0 + P.iso_diag[(size_t)i] * y1;
      y[(size_t)i] = y1 + (omega * (r[(size_t)i] - acc)) * P.iso_invd[(size_t)i];
      continue;
    }
    REQUIRE((size_t)ci < nc && P.ci_row[(size_t)ci] == i);
    if ((size_t)ci >= nc) return P;
    for (int dir = 0; dir < 2; ++dir) {
      const int64_t p = (dir ? P.rpos_b : P.rpos_f)[(size_t)ci];
      REQUIRE(p >= 0 && (uint64_t)p * 8 + 8 <= S.size() && !row_at[dir].count(p));
      if (p < 0 || (uint64_t)p * 8 + 8 > S.size()) return P;
      row_at[dir][p] = (int32_t)i;
      std::memcpy(S.data() + p * 8, &r[(size_t)i], 8);
    }
  }
  std::vector<Range> ranges = decode(P, S);
  if (g_failures) return P;

  // ---- who a record belongs to; where the backward record of a row keeps its prefix
  std::vector<int64_t> prefix_pos((size_t)n, -1);
  for (Range &R : ranges)
    for (auto &step : R.steps)
      for (Rec &rec : step) {
        if (P.phased) {
          const auto it = row_at[R.backward].find(rec.pos(0) / 8);
          REQUIRE(it != row_at[R.backward].end());
          if (it == row_at[R.backward].end()) return P;
          rec.row = it->second;
        } else {
          const uint32_t slot = rec.my() / 8;
          REQUIRE(rec.my() % 8 == 0 && (int)slot < R.n_own);
          if ((int)slot >= R.n_own) return P;
          rec.row = P.ci_row[(size_t)P.ws_ci[(size_t)R.ws_off + slot]];
          if (rec.last) REQUIRE((R.backward ? P.rpos_b : P.rpos_f)[(size_t)P.row_ci[(size_t)rec.row]] == rec.pos(0) / 8);
        }
        if (R.backward && rec.first) prefix_pos[(size_t)rec.row] = rec.pos(16);
      }

  // ---- (a) + (b) + (c): block by block, its ranges in table order = the order the sweep takes them (forward ones first)
  int range_no = 0;
  std::vector<int> upd((size_t)n, -1), done_dir[2] = {std::vector<int>((size_t)n, 0), std::vector<int>((size_t)n, 0)};
  std::vector<double> carry((size_t)n, 0.0);
  std::vector<std::vector<Entry>> got((size_t)n);
  for (int b = 0; b < n_blocks; ++b) {
    REQUIRE(P.block_rng[(size_t)b] == range_no);
    bool seen_backward = false;
    for (; range_no < P.block_rng[(size_t)b + 1]; ++range_no) {
      Range &R = ranges[(size_t)range_no];
      REQUIRE(!(seen_backward && !R.backward));
      seen_backward = R.backward;
      const int dir = R.backward;
      std::vector<int32_t> owner((size_t)P.y_slots, -1);
      std::vector<int> last_read((size_t)P.y_slots, -1);
      std::vector<double> lds((size_t)P.y_slots, 0.0);
      std::vector<int32_t> touched;
      REQUIRE(R.n_ws <= P.y_slots && R.n_own <= R.n_ws);
      for (int k = 0; k < R.n_ws; ++k) {  // the working set comes from ycur
        const int32_t ci = P.ws_ci[(size_t)R.ws_off + (size_t)k];
        owner[(size_t)k] = P.ci_row[(size_t)ci];
        lds[(size_t)k] = ycur[(size_t)ci];
      }
      for (size_t t = 0; t < R.steps.size(); ++t) {
        auto &step = R.steps[t];
        struct Result { uint32_t slot; double ynew, acc; };
        std::vector<Result> results;
        for (Rec &rec : step) {  // the step's rows take their slots (self-contained: one phase before the dependent one)
          const uint32_t slot = rec.my() / 8;
          const int64_t i = rec.row;
          REQUIRE(rec.my() % 8 == 0 && (int)slot < P.y_slots && block_of[(size_t)i] == b);
          REQUIRE(bits_of(rec.f64(8)) == bits_of(invd[(size_t)i]));
          if ((int)slot >= P.y_slots) return P;
          if (R.self) {
            if (owner[slot] >= 0) REQUIRE(last_read[slot] <= (int)t - 2);  // the hold of two steps
            owner[slot] = (int32_t)i;
            if (dir) {
              REQUIRE(rec.aux() == (uint32_t)i);
              lds[slot] = 0.0 + (omega * (rec.f64(0) - rec.f64(16))) * rec.f64(8);  // the row's forward value, from its own fields
            }
          } else {
            REQUIRE(owner[slot] == i && (int)slot < R.n_own);
            if (dir) REQUIRE(rec.aux() == 0);
          }
          if (!dir && rec.last) REQUIRE(prefix_pos[(size_t)i] >= 0 && (int64_t)rec.aux() * 8 == prefix_pos[(size_t)i]);
          last_read[slot] = std::max(last_read[slot], (int)t);
        }
        for (Rec &rec : step) {
          const int64_t i = rec.row;
          const uint32_t my = rec.my();
          if (rec.first) { got[(size_t)i].clear(); carry[(size_t)i] = dir ? rec.f64(16) : 0.0; }
          double acc = carry[(size_t)i];
          for (int e = 0; e < rec.n_ent(); ++e) {
            const double v = rec.value(e);
            const uint32_t ad = rec.addr(e), slot = ad / 8;
            REQUIRE(ad % 8 == 0 && (int)slot < P.y_slots);
            if ((int)slot >= P.y_slots) return P;
            if (bits_of(v) == 0) REQUIRE(ad == my);  // padding: +0.0 and the row's own address
            else {
              const int32_t c = owner[slot];
              REQUIRE(c >= 0);
              if (c < 0) return P;
              got[(size_t)i].emplace_back(c, bits_of(v));
              // the value is there: updated earlier in this sweep, or loaded with the working set (the row itself: its slot)
              const bool t1 = e >= rec.n_head && e < rec.n_head + rec.l1;
              if (c != i) {
                if (upd[(size_t)c] >= 0) REQUIRE(upd[(size_t)c] < (int)t && (t1 || !P.phased || upd[(size_t)c] < (int)t - R.late));
                else REQUIRE(!R.self && done_dir[dir][(size_t)c] == 1);  // (an earlier range of this direction wrote it back to ycur)
              }
              last_read[slot] = std::max(last_read[slot], (int)t);
            }
            acc += v * lds[slot];
          }
          carry[(size_t)i] = acc;
          if (!rec.last) continue;
          REQUIRE(got[(size_t)i] == entries(i, dir));
          for (size_t k = 1; k < got[(size_t)i].size(); ++k) REQUIRE(got[(size_t)i][k - 1].first < got[(size_t)i][k].first);
          const double yold = dir ? lds[my / 8] : 0.0;
          results.push_back(Result{my / 8, yold + (omega * (rec.f64(0) - acc)) * rec.f64(8), acc});
          if (!dir) std::memcpy(S.data() + (size_t)rec.aux() * 8, &acc, 8);  // the prefix, through aux into the backward record
          else if (R.self) y[(size_t)rec.aux()] = results.back().ynew;
          REQUIRE(done_dir[dir][(size_t)i] == 0);
          done_dir[dir][(size_t)i] = 1;
        }
        for (const Rec &rec : step)
          if (rec.last) { upd[(size_t)rec.row] = (int)t; touched.push_back(rec.row); }
        for (const Result &x : results) lds[x.slot] = x.ynew;
      }
      for (int k = 0; k < R.n_own; ++k) {  // the rows updated here go back to ycur; backward: their results are final
        const int32_t ci = P.ws_ci[(size_t)R.ws_off + (size_t)k];
        ycur[(size_t)ci] = lds[(size_t)k];
        if (dir) y[(size_t)P.ci_row[(size_t)ci]] = lds[(size_t)k];
      }
      for (int32_t i : touched) upd[(size_t)i] = -1;
    }
  }
  REQUIRE(range_no == P.n_ranges());
  int64_t mismatches = 0;
  for (int64_t i = 0; i < n; ++i) mismatches += bits_of(y[(size_t)i]) != bits_of(y_ref[(size_t)i]);
  REQUIRE(mismatches == 0);
  for (int64_t i = 0; i < n; ++i)
    if (P.row_ci[(size_t)i] >= 0) REQUIRE(done_dir[0][(size_t)i] == 1 && done_dir[1][(size_t)i] == 1);

  // ---- check_sweep_plan rejects one aux word, one slot address, one backward row out of range
  const Rec *fwd = nullptr, *bwd_self = nullptr;
  for (const Range &R : ranges)
    for (const auto &step : R.steps)
      for (const Rec &rec : step) {
        if (!R.backward && !fwd) fwd = &rec;
        if (R.backward && R.self && !bwd_self) bwd_self = &rec;
      }
  if (fwd) {
    SsorSweepPlan Q = P;
    const uint32_t far = (uint32_t)(Q.stream.size() / 8);
    std::memcpy(Q.stream.data() + fwd->pos(28), &far, 4);
    REQUIRE(check_sweep_plan(Q, n) != nullptr);
    Q = P;
    const uint32_t beyond = (uint32_t)Q.y_slots * 8u;
    std::memcpy(Q.stream.data() + fwd->pos(32 + 8 * fwd->n_ent() + 4 * (fwd->n_ent() - 1)), &beyond, 4);
    REQUIRE(check_sweep_plan(Q, n) != nullptr);
    Q = P;
    std::memcpy(Q.stream.data() + fwd->pos(24), &beyond, 4);
    REQUIRE(check_sweep_plan(Q, n) != nullptr);
  }
  if (bwd_self) {
    SsorSweepPlan Q = P;
    const uint32_t far = (uint32_t)n;
    std::memcpy(Q.stream.data() + bwd_self->pos(28), &far, 4);
    REQUIRE(check_sweep_plan(Q, n) != nullptr);
    Q = P;
    REQUIRE(!Q.bwd_rows.empty());
    if (!Q.bwd_rows.empty()) Q.bwd_rows.back() = (int32_t)n;
    REQUIRE(check_sweep_plan(Q, n) != nullptr);
  }
  if (!P.ws_ci.empty()) {
    SsorSweepPlan Q = P;
    Q.ws_ci[0] = (int32_t)nc;
    REQUIRE(check_sweep_plan(Q, n) != nullptr);
  }
  if (nc) {
    SsorSweepPlan Q = P;
    Q.rpos_b[nc - 1] = (int32_t)(Q.stream.size() / 8);
    REQUIRE(check_sweep_plan(Q, n) != nullptr);
  }
  return P;
}

int steps_of(const SsorSweepPlan &P) { return (int)P.total_steps; }

// ---- file mode ---------------------------------------------------------------------------------------------------------------
// FILE (text): "ssor-shape-case" / n nnz blocks n_bounds / rowptr [n + 1] / col [nnz] / val [nnz] as 16 hex digits each (the bits) /
// bounds [n_bounds] (n_bounds > 0: the caller's block boundaries, else `blocks` equal runs) / n_sets / per set one line: its name,
// the number of options, then key value pairs with the option names of gmg_set_option.
struct OptionSet { std::string name; SsorPlanOptions opt; };

bool read_case(const char *path, Csr &A, int &blocks, std::vector<int64_t> &bounds, std::vector<OptionSet> &sets) {
  std::FILE *f = std::fopen(path, "r");
  if (!f) return false;
  char word[128];
  long long n = 0, nnz = 0, nb = 0, v = 0;
  bool ok = std::fscanf(f, "%127s", word) == 1 && std::string(word) == "ssor-shape-case" && std::fscanf(f, "%lld %lld %d %lld", &n, &nnz, &blocks, &nb) == 4 &&
            n >= 1 && n <= 100000 && nnz >= 0 && nnz <= 10000000 && nb >= 0 && nb <= n + 2;
  if (ok) {
    A.n = n; A.rp.assign((size_t)n + 1, 0); A.col.assign((size_t)nnz, 0); A.val.assign((size_t)nnz, 0.0);
    for (int64_t &x : A.rp) { ok = ok && std::fscanf(f, "%lld", &v) == 1; x = v; }
    for (int32_t &x : A.col) { ok = ok && std::fscanf(f, "%lld", &v) == 1 && v >= 0 && v < n; x = (int32_t)v; }
    for (double &x : A.val) { unsigned long long b = 0; ok = ok && std::fscanf(f, "%llx", &b) == 1; const uint64_t b64 = b; std::memcpy(&x, &b64, 8); }
    bounds.assign((size_t)nb, 0);
    for (int64_t &x : bounds) { ok = ok && std::fscanf(f, "%lld", &v) == 1; x = v; }
    ok = ok && A.rp.front() == 0 && A.rp.back() == nnz;
    for (size_t i = 0; ok && i < (size_t)n; ++i) ok = A.rp[i] <= A.rp[i + 1];
  }
  int n_sets = 0;
  ok = ok && std::fscanf(f, "%d", &n_sets) == 1 && n_sets >= 1 && n_sets <= 64;
  for (int s = 0; ok && s < n_sets; ++s) {
    OptionSet o;
    int n_opt = 0;
    ok = std::fscanf(f, "%127s %d", word, &n_opt) == 2 && n_opt >= 0 && n_opt <= 16;
    o.name = word;
    for (int k = 0; ok && k < n_opt; ++k) {
      double x = 0;
      ok = std::fscanf(f, "%127s %lf", word, &x) == 2;
      const std::string key = word;
      if (key == "sgs_sliding") o.opt.sliding = x != 0;
      else if (key == "sgs_y_slots") o.opt.y_slots = (int)x;
      else if (key == "sgs_phase_chunk") o.opt.phase_chunk = (int)x;
      else if (key == "sgs_phase_nosplit") o.opt.phase_nosplit = x != 0;
      else if (key == "sgs_phase_nocascade") o.opt.phase_nocascade = x != 0;
      else if (key == "sgs_dep") o.opt.dep = x != 0;
      else if (key == "sgs_reg") o.opt.reg = x != 0;
      else if (key == "sgs_disable_phase") o.opt.disable_phase = x != 0;
      else if (key == "sgs_groups") o.opt.groups = (int)x;
      else ok = false;
    }
    sets.push_back(o);
  }
  std::fclose(f);
  return ok;
}

int file_mode(int argc, char **argv) {
  Csr A;
  int blocks = 1;
  std::vector<int64_t> bounds;
  std::vector<OptionSet> sets;
  if (!read_case(argv[1], A, blocks, bounds, sets)) { std::fprintf(stderr, "ssor_plan_replay: cannot read %s\n", argv[1]); return 2; }
  int total = 0;
  for (int a = 2; a < argc || a == 2; ++a) {  // one pass per mutate= argument (without any: one pass, nothing mutated)
    if (a < argc) {
      int key = -1;
      char kind[16] = "";
      if (std::sscanf(argv[a], "mutate=%d:%15s", &key, kind) != 2 || key < 0 || key > 255 || (std::string(kind) != "stride" && std::string(kind) != "t1")) {
        std::fprintf(stderr, "ssor_plan_replay: unknown argument %s\n", argv[a]);
        return 2;
      }
      g_mut_key = key; g_mut_kind = kind[0];
      std::printf("mutation %d %s\n", key, kind);
    }
    for (const OptionSet &o : sets) {
      g_failures = 0;
      Want w; w.any_kind = true;
      bool retried = false;
      const SsorSweepPlan P = run(o.name, A, o.opt, w, bounds.empty() ? nullptr : &bounds, false, blocks, &retried);
      std::map<std::vector<int>, int> table;  // (g, l1, l2, backward, self-contained) -> steps
      int switches = 0, min_rows = 0, max_rows = 0, n_self = 0;
      for (const PhRange &R : P.pranges) {
        n_self += R.pad0[0] == 1;
        for (int q = 0; q < R.n_steps; ++q) {
          const uint32_t word = P.blk_tab[(size_t)R.blk_tab + (size_t)q].word;
          const int key = (int)(word & 255u), rows = (int)(word >> 8 & 255u);
          table[{key >> 6, 4 * (key >> 3 & 7), 8 * (key & 7), R.backward != 0, R.pad0[0] == 1}]++;
          if (q > 0 && (int)(P.blk_tab[(size_t)R.blk_tab + (size_t)q - 1].word & 255u) != key) ++switches;
          min_rows = min_rows ? std::min(min_rows, rows) : rows;
          max_rows = std::max(max_rows, rows);
        }
      }
      std::printf("plan %s %d %d %d %d %d %d %lld %d %d %d %d %d %d\n", o.name.c_str(), (int)P.phased, (int)P.dep, (int)P.reg, (int)retried, P.n_ranges(), n_self,
                  (long long)P.total_steps, switches, min_rows, max_rows, P.live_max[0], P.live_max[1], g_failures);
      for (const auto &kv : table) std::printf("shape %s %d %d %d %d %d %d\n", o.name.c_str(), kv.first[0], kv.first[1], kv.first[2], kv.first[3], kv.first[4], kv.second);
      total += g_failures;
    }
  }
  return total ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) return file_mode(argc, argv);
  const SsorPlanOptions def;
  const Want four;
  Want one; one.phased = false;
  {  // 1-D chain: one row per stage
    const SsorSweepPlan P = run("chain 200", chain(200), def, four);
    REQUIRE(P.total_stages == 200 && P.total_steps == 400 && P.n_self == 2 && P.ci_row.size() == 200);
  }
  {
    const SsorSweepPlan P = run("5-point 12x12", five_point(12, 12), def, four);
    REQUIRE(P.total_stages == 23 && P.n_self == 2);
  }
  const Csr A27 = box27(6), A22 = pairs(40);
  {
    const SsorSweepPlan P = run("27-point 6x6x6", A27, def, four);
    REQUIRE(P.n_self == 2 && P.ci_row.size() == 216);
    const SsorSweepPlan Q = run("40 pairs", A22, def, four);
    REQUIRE(Q.total_stages == 2 && Q.total_steps == 8);  // a stage of 40 rows = two steps, per direction
  }
  {  // stored zeros are pruned (not so in the generic schedule), diagonal-only rows and a row without a diagonal are closed-form
    const Csr A = zeros_and_lone_rows();
    const SsorSweepPlan P = run("stored zeros, lone rows", A, def, four);
    REQUIRE(P.ci_row.size() < (size_t)A.n && P.iso_diag[40] == 0.0 && P.iso_invd[40] == 1.0);
  }
  {  // a row too wide for the four-wave records: the pre-check (> 72 stored entries), a direction without a shape (> 36 entries)
    bool retried = true;
    const SsorSweepPlan P = run("arrow, 80 wide", arrow(120, 80), def, one, nullptr, false, 1, &retried);
    REQUIRE(!retried && P.total_steps > 2 * P.total_stages);  // (the wide row takes several sub-steps)
    run("arrow, 45 wide", arrow(120, 45), def, one, nullptr, false, 1, &retried);
    REQUIRE(retried);
    SsorPlanOptions o; o.phase_chunk = 1;
    run("arrow, 45 wide, chunk 1", arrow(120, 45), o, one, nullptr, false, 1, &retried);
    REQUIRE(retried);
  }
  {  // columns not ascending: the generic sweep; no wave; nothing to plan
    Csr A = five_point(6, 6);
    std::swap(A.col[(size_t)A.rp[7]], A.col[(size_t)A.rp[7] + 1]);
    Want w; w.planned = false; w.generic = "unsorted columns";
    run("unsorted columns", A, def, w);
    SsorPlanOptions o; o.disable_wave = true;
    w.generic = "wave disabled";
    run("wave disabled", five_point(6, 6), o, w);
  }
  {  // the caller's boundaries, uneven, one block empty; balanced cuts; equal runs
    const Csr A = five_point(12, 12);
    const std::vector<int64_t> b1 = {0, 144}, b2 = {0, 50, 144}, b3 = {0, 70, 70, 144};
    run("caller's 1 block", A, def, four, &b1);
    const SsorSweepPlan P2 = run("caller's 2 blocks", A, def, four, &b2);
    REQUIRE(P2.block_rng.size() == 3 && P2.n_self == 4);
    const SsorSweepPlan P3 = run("caller's 3 blocks, one empty", A, def, four, &b3);
    REQUIRE(P3.block_rng[1] == P3.block_rng[2] && P3.block_steps[1] == 0 && P3.n_self == 4);
    const std::vector<int64_t> c3 = {0, 100, 100, 216};
    run("caller's 3 blocks, 27-point", A27, def, four, &c3);
    const SsorSweepPlan PB = run("balanced cuts", A, def, four, nullptr, true, 3);
    REQUIRE(PB.block_rng.size() == 4 && PB.n_self == 6);
    const SsorSweepPlan PE = run("equal runs", A27, def, four, nullptr, false, 3);
    REQUIRE(PE.block_rng.size() == 4);
  }
  // ---- the option sets, each on the 27-point and the pairs case
  for (int c = 0; c < 2; ++c) {
    const Csr &A = c ? A22 : A27;
    const std::string tag = c ? "pairs, " : "27-point, ";
    const SsorSweepPlan D = run(tag + "default", A, def, four);
    {
      SsorPlanOptions o; o.sliding = false;
      const SsorSweepPlan P = run(tag + "sliding off", A, o, four);
      REQUIRE(P.n_self == 0 && P.n_ranges() == 2 && P.pranges[0].own_dir == 1 && P.pranges[1].own_dir != 0);
    }
    {
      SsorPlanOptions o; o.y_slots = 64;
      const SsorSweepPlan P = run(tag + "y_slots 64", A, o, four);
      int with_dir = 0;
      for (const PhRange &R : P.pranges) with_dir += R.own_dir != 0;
      if (c == 0) REQUIRE(P.n_self == 0 && P.n_ranges() > 4 && with_dir > 0 && P.y_slots <= 64);
      else REQUIRE(P.y_slots <= 64);
    }
    {
      SsorPlanOptions o; o.disable_phase = true;
      const SsorSweepPlan P = run(tag + "disable_phase", A, o, one);
      REQUIRE(!P.ranges.empty() && P.pranges.empty());
      for (int g : {1, 4}) {
        o.groups = g;
        const SsorSweepPlan Q = run(tag + "disable_phase, groups " + std::to_string(g), A, o, one);
        for (const SwRange &R : Q.ranges) REQUIRE(R.groups == g);
        if (c == 0 && g == 1) REQUIRE(steps_of(Q) > steps_of(P));  // (rows of more than 8 entries: several sub-steps)
      }
      o.y_slots = 64;
      o.groups = 0;
      const SsorSweepPlan Q = run(tag + "disable_phase, y_slots 64", A, o, one);
      if (c == 0) REQUIRE(Q.n_ranges() > 4);
    }
    {
      Want w; w.dep = true;
      SsorPlanOptions o; o.dep = true;
      const SsorSweepPlan P = run(tag + "dep", A, o, w);
      REQUIRE(P.n_self == 0);
      for (const PhRange &R : P.pranges) REQUIRE(R.pf_step > 0);
    }
    {
      Want w; w.reg = true;
      SsorPlanOptions o; o.reg = true;
      const SsorSweepPlan P = run(tag + "reg", A, o, w);
      REQUIRE(P.n_self == 0);
    }
    {
      SsorPlanOptions o; o.phase_nosplit = true;
      const SsorSweepPlan P = run(tag + "phase_nosplit", A, o, four);
      REQUIRE(P.hist_l2[1] + P.hist_l2[2] + P.hist_l2[3] == 0 && P.hist_l2[0] == P.total_steps);
    }
    {
      SsorPlanOptions o; o.phase_nocascade = true;
      const SsorSweepPlan P = run(tag + "phase_nocascade", A, o, four);
      for (const PhBlkEntry &e : P.blk_tab) REQUIRE((int)(e.word >> 16) == 4 * (int)(e.word >> 3 & 7));
    }
    {
      SsorPlanOptions o; o.phase_chunk = 1;
      run(tag + "phase_chunk 1", A, o, four);
    }
    for (int g : {1, 4}) {
      SsorPlanOptions o; o.groups = g;
      const SsorSweepPlan P = run(tag + "groups " + std::to_string(g), A, o, four);
      REQUIRE(P.stream == D.stream);  // (the four-wave records do not depend on it)
    }
  }
  if (g_failures) { std::fprintf(stderr, "%d requirement(s) failed\n", g_failures); return 1; }
  std::printf("ssor_plan_replay: all plans decode, check and replay\n");
  return 0;
}
