// gmg_sgs_layout.hpp -- the plan of the SSOR sweep, made on the host (DESIGN.md sections 4 and 26).
// Host-only standard C++: no HIP, no context, no device pointer.  From a level's CSR and the block boundaries, ssor_generic_plan
// and ssor_sweep_plan make plain vectors and scalars; setup_sgs (gmg_coulomb.hip) copies them to the device as they are.  The
// kernels that read the plan are in gmg_sgs.hpp, gmg_sgs_phase.hpp, gmg_sgs_dep.hpp and gmg_sgs_reg.hpp, which take the
// constants and the plain structs they share with the planner from here; gmg_sgs_plan.hpp forms the default plan on the device,
// byte for byte.  tests/ssor_plan_replay.cc restates the record layouts, decodes every plan back to the rows it came from and
// replays a sweep from the records alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <queue>
#include <vector>

#include "gmg_layout.hpp"

#ifdef __HIPCC__
#define GMG_HD __host__ __device__
#else
#define GMG_HD
#endif

namespace gmg {

// ---- what the planner shares with the kernels ------------------------------------------------------------------------------
// one-wave sweep (gmg_sgs.hpp)
constexpr int kSwRing = 32768;     // bytes of the record ring in LDS
constexpr int kSwChunk = 4096;     // unit the helper waves copy
constexpr int kSwW = 32;           // most entries per sub-step: a row's sum is formed in groups of 8 products, 1..4 groups per sub-step
constexpr int kSwMaxBlock = 8192;  // bytes of one step's records: 3 blocks + 1 chunk fit the ring (no deadlock)
constexpr int kSwYSlots = 15744;   // doubles of y in LDS (123 KB) by default

// One range = consecutive steps of one sweep direction whose working set fits the LDS.
struct SwRange {
  int64_t stream_off;    // byte offset of the range's records (multiple of kSwChunk)
  int32_t stream_bytes;  // multiple of kSwChunk
  int32_t n_steps;       // sub-steps
  int32_t ws_off;        // first entry of the range in ws_ci
  int32_t n_own;         // slots [0, n_own): rows updated in this range (written back at its end)
  int32_t n_ws;          // slots in use: updated rows + rows only read
  int32_t backward;      // 1: second sweep, its results are final
  int32_t first_raw, first_nrows, groups, pad1;  // groups: g of every sub-step of the range
};
struct SwStepHdr {  // (the record layout behind it: gmg_sgs.hpp)
  uint16_t nrows, flags;       // flags: 1 = first sub-step of its step, 2 = last one
  uint16_t next_nrows, pad;
  uint32_t advance;            // bytes to the next header (>= the raw size: records never straddle the ring end)
  uint32_t next_raw;           // raw bytes of the next sub-step's records (0: last of the range)
};
GMG_HD constexpr int sw_stride(int g) { return 96 * g + 48; }

// four-wave sweep (gmg_sgs_phase.hpp)
constexpr int kPhRegion = 16384;  // bytes of LDS per compute wave for the block it is reading (a block never exceeds it)
constexpr int kPhMaxRows = 32;    // rows per step
constexpr int kPhMaxEntries = 36; // 8 G + L of a range
constexpr int kPhWaves = 4;       // compute waves
constexpr int kPhThreads = 64 * (kPhWaves + 1);  // waves 0..3 compute, wave 4 prefetches the records into the L2
constexpr int kPhJunk = 512;      // LDS bytes behind the regions: [0, 256) the prefetch wave's copies land in, [256, 264) the hand-over words of gmg_sgs_chain.hpp
constexpr int kPhYSlots = (160 * 1024 - kPhWaves * kPhRegion - kPhJunk) / 8 & ~1;  // doubles of y in LDS: 12256
// a range's shape: 8 g head entries, l1 tail entries gathered in the dependent phase, l2 tail entries whose products are formed ahead
GMG_HD constexpr bool ph_shape_ok(int g, int l1, int l2) {
  return g >= 0 && g <= 3 && l1 >= 4 && l1 <= 28 && l1 % 4 == 0 && l2 >= 0 && l2 <= 24 && l2 % 8 == 0 && 8 * g + l1 + l2 <= kPhMaxEntries;
}
GMG_HD constexpr int ph_stride(int g, int l) {
  const int s = 32 + 96 * g + 12 * l;  // multiple of 16 (l is a multiple of 4)
  return (s / 16) % 2 ? s : s + 16;    // odd multiple of 16: 16-byte LDS reads of consecutive lanes hit distinct banks
}
namespace ph {
GMG_HD constexpr int ph_key(int g, int l1, int l2) { return g * 64 + (l1 / 4) * 8 + l2 / 8; }
}  // namespace ph

// One range of the four-wave sweep (the layout of a step's block and of its records: gmg_sgs_phase.hpp).
struct PhRange {
  int64_t stream_off;
  int32_t n_steps, ws_off, n_own, n_ws, backward, G, L;  // L = L1 + L2
  uint32_t blk_tab, L1;               // first entry of the range in the block table
  int32_t own_ci0, own_dir, pad0[2];  // own_dir = +1 / -1: slot k of the rows updated here is ycur[own_ci0 + own_dir * k] (ycur is numbered in sweep order); 0: see ws_ci
                                      // pad0[0] = 1: the range is SELF-CONTAINED (a whole sweep direction of its block, y slots recycled); pad0[1]: its y slots
  uint32_t pf_lead, pf_step;          // prefetch wave: bytes ahead at phase 0, bytes per phase (multiples of 128)
  uint32_t stream_bytes, pad;
};
struct PhBlkEntry { uint32_t off, bytes, word, pad; };  // one step in the block table (the kernels read it as uint4): offset in its range's stream, bytes,
                                                        // shape key | rows << 8 | T1 slots in use << 16

// dependent-wave and register variants (gmg_sgs_dep.hpp, gmg_sgs_reg.hpp)
constexpr int kDpLate = 3;          // a column updated within the last kDpLate steps is gathered by the dependent wave
constexpr int kDpPrep = 3;          // preparing waves
constexpr int kDpSlots = 4;         // ring slots: prep of step t starts when step t - 4 is finished, i.e. when slot t % 4 is free
constexpr int kDpThreads = 64 * (1 + kDpPrep);
constexpr int kDpMaxL1 = 28;        // T1 slots of a compact record (the shapes of gmg_sgs_phase.hpp: 8 g + l1 + l2 <= 36)
constexpr int kDpMaxL2 = 24;
GMG_HD constexpr int dp_cstride(int l1, int l2) {  // bytes of a compact record: odd multiple of 16
  const int s = 48 + 12 * l1 + 8 * l2;
  return (s / 16) % 2 ? s : s + 16;
}
// the widest compact record the shapes allow (l1 + l2 <= 36): (28, 8)
constexpr int kDpMaxStride = dp_cstride(28, 8);
static_assert(dp_cstride(12, 24) <= kDpMaxStride && dp_cstride(20, 16) <= kDpMaxStride && dp_cstride(24, 8) <= kDpMaxStride && dp_cstride(16, 16) <= kDpMaxStride, "slot size");
constexpr int kDpSlotBytes = 16 + kPhMaxRows * kDpMaxStride;  // 14 864
constexpr int kDpFlagBytes = 64;   // done, abort, ready[4]
constexpr int kDpYSlots = ((160 * 1024 - kDpSlots * ((kDpSlotBytes + 15) / 16 * 16) - kDpFlagBytes) / 8) & ~1;
constexpr int kRgYSlots = (160 * 1024 - kPhJunk) / 8 & ~1;  // doubles of y in LDS: 20 416

namespace sp {
// head [0, h0), T1 [h0, h1), T2 [h1, ne) of a row with ne entries whose late columns are first .. last (none: first = ne,
// last = ne - 1): false if the row does not fit the shape (g, l1, l2)
GMG_HD inline bool fits(int ne, int first, int last, int g, int l1, int l2, int *h0o, int *h1o) {
  const int a = last + 1, b = ne - l2;
  const int h1 = a < b ? b : a;
  const int c = first < 8 * g ? first : 8 * g, d = h1 - l1;
  const int h0 = c < d ? d : c;
  if (h0 > first || h0 > 8 * g || h0 < 0) return false;
  if (h0o) { *h0o = h0; *h1o = h1; }
  return true;
}
GMG_HD inline double dmax(double a, double b) { return a < b ? b : a; }
// measured phase costs (cycles) of a step of `rows` rows in shape (g, l1, l2): the four-wave sweep with LDS copies
GMG_HD inline double shape_cost(int g, int l1, int l2, double rows) {
  const int ent = 8 * g + l1 + l2;
  const double crit = 330.0 + 15.0 * l1 + 4.0 * l2, copy = 45.0 * (16.0 + rows * ph_stride(g, l1 + l2)) / 1024.0,
               p1 = 150.0 + 8.0 * (2.0 + 0.75 * ent), p2 = 100.0 + 11.0 * (8 * g + l2);
  return dmax(dmax(crit, copy), dmax(p1, p2)) + 0.1 * (crit + copy + p1 + p2);
}
GMG_HD inline void key_shape(int key, int *g, int *l1, int *l2) { *g = key >> 6; *l1 = 4 * (key >> 3 & 7); *l2 = 8 * (key & 7); }
}  // namespace sp
// ---- end of the shared part -------------------------------------------------------------------------------------------------

struct SsorPlanOptions {  // the context's options that steer a plan
  bool disable_wave = false, disable_phase = false, profile = false, dep = false, reg = false, chain = false, sliding = true;
  int y_slots = 0, groups = 0, phase_chunk = 0;
  bool phase_nosplit = false, phase_nocascade = false;
  int pf_lead_kb = 0;
  bool debug = false;
  int pack = -1;  // rows scheduled by slack (ssor_pack_levels): 0 never, 1 always, < 0 levels of at least kPhPackMinRows rows
};
// Below the gate a sweep direction is a few hundred steps, tens of us: nothing to gain, and every small level keeps the plan
// the stages give (the device builder of gmg_sgs_plan.hpp forms that one).
constexpr int64_t kPhPackMinRows = 8192;
// does the four-wave plan with self-contained ranges of a level of n rows try the packed levels?
inline bool ssor_pack_wanted(const SsorPlanOptions &opt, int64_t n) {
  const bool self = !opt.disable_wave && !opt.disable_phase && !opt.profile && !opt.dep && !opt.reg && !opt.chain && opt.sliding;
  return self && (opt.pack > 0 || (opt.pack < 0 && n >= kPhPackMinRows));
}

// ---- where the SSOR blocks are cut ("Block boundaries").  Modelled sweep time of a block of consecutive rows:
//   cost = kSsorStepNs * sub-steps + stream bytes / kSsorBytesPerNs
// sub-steps: both directions walk the stages of the block's recurrence stage(i) = 1 + max stage(j) over the coupled j in
// [rb, i), at most kPhMaxRows rows of one stage per step -- the count ssor_sweep_plan makes for the four-wave sweep that walks the
// stages, an upper bound where the rows are scheduled by slack (ssor_pack_levels: the model keeps counting stage by stage).  Stream:
// the records scale with rows x width, kSsorRowBytes per coupled row plus kSsorEntryBytes per in-block entry of it (both
// directions; 73 MB for the 92 164 coupled rows of the 64 k-atom level 1).  Uncoupled rows (the prepass) cost nothing.
constexpr double kSsorStepNs = 240.0;     // one dependent step of the four-wave sweep
constexpr double kSsorBytesPerNs = 48.0;  // one CU streams ~20 B per clock at 2.4 GHz
constexpr int64_t kSsorRowBytes = 64, kSsorEntryBytes = 28;

// Pattern of the entries that couple (stored value != 0, or every stored entry without values) and its transpose.
struct SsorPattern {
  int64_t n = 0;
  std::vector<int64_t> rp, trp;
  std::vector<int32_t> col, tcol;
  SsorPattern(int64_t n_, const int64_t *rp_, const int32_t *col_, const double *val) : n(n_) {
    rp.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
      for (int64_t k = rp_[i]; k < rp_[i + 1]; ++k)
        if (!val || val[k] != 0.0) col.push_back(col_[k]);
      rp[(size_t)i + 1] = (int64_t)col.size();
    }
    std::vector<double> ones(col.size(), 1.0), tval;
    transpose_host(n, n, rp.data(), col.data(), ones.data(), trp, tcol, tval);
  }
};

// The model of one block, grown a row at a time (add() never lowers the cost: the greedy cut below relies on it).
struct SsorBlockModel {
  const SsorPattern &P;
  std::vector<int32_t> stage, ent;  // per row of the block: stage, in-block entries so far
  std::vector<char> coupled;
  std::vector<int64_t> cnt;          // coupled rows per stage
  int64_t rb = 0, steps = 0, bytes = 0;
  explicit SsorBlockModel(const SsorPattern &p) : P(p), stage((size_t)p.n, 0), ent((size_t)p.n, 0), coupled((size_t)p.n, 0) {}
  void reset(int64_t r) { rb = r; steps = bytes = 0; cnt.clear(); }
  double cost_ns() const { return kSsorStepNs * (double)steps + (double)bytes / kSsorBytesPerNs; }
  void put(int32_t s) {
    if ((size_t)s >= cnt.size()) cnt.resize((size_t)s + 1, 0);
    if (cnt[(size_t)s]++ % kPhMaxRows == 0) steps += 2;
  }
  void add(int64_t i) {
    int32_t st = 0;
    bool low = false;
    auto touch = [&](int64_t j) {  // j in [rb, i) coupled to i
      low = true;
      if (!coupled[(size_t)j]) {  // coupled only to rows after it: stage 0
        coupled[(size_t)j] = 1; stage[(size_t)j] = 0; put(0);
        bytes += kSsorRowBytes + kSsorEntryBytes * ent[(size_t)j];
      }
      st = std::max(st, stage[(size_t)j] + 1);
    };
    int32_t e = 0;
    for (int64_t k = P.rp[(size_t)i]; k < P.rp[(size_t)i + 1]; ++k) {
      const int64_t c = P.col[(size_t)k];
      if (c < rb || c > i) continue;
      ++e;
      if (c < i) touch(c);
    }
    for (int64_t k = P.trp[(size_t)i]; k < P.trp[(size_t)i + 1]; ++k) {  // entries (j, i) of the earlier rows
      const int64_t j = P.tcol[(size_t)k];
      if (j < rb || j >= i) continue;
      ent[(size_t)j]++;
      if (coupled[(size_t)j]) bytes += kSsorEntryBytes;
      touch(j);
    }
    ent[(size_t)i] = e;
    coupled[(size_t)i] = low;
    stage[(size_t)i] = low ? st : 0;
    if (low) { put(st); bytes += kSsorRowBytes + kSsorEntryBytes * e; }
  }
};

// B - 1 cuts that make the blocks' modelled costs about equal: the greedy pass fills each block up to a target T (the
// fewest blocks for that T), a bisection finds the smallest T that needs at most B of them.  O(nnz) per pass, the same
// arithmetic in the same order on every rank.  B is clamped to (n + 63) / 64 like the equal runs; the boundaries behind
// the last block used are n (empty blocks).  cost_us: each block's modelled time.
inline void ssor_balance(const SsorPattern &P, int n_blocks, std::vector<int64_t> &block_row, std::vector<double> &cost_us) {
  const int64_t n = P.n;
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(n_blocks, (n + 63) / 64));
  SsorBlockModel M(P);
  auto greedy = [&](double T, std::vector<int64_t> *cuts) {
    int count = 1;
    M.reset(0);
    for (int64_t i = 0; i < n; ++i) {
      M.add(i);
      if (M.cost_ns() > T && i > M.rb) {
        if (++count > nb) return count;
        if (cuts) cuts->push_back(i);
        M.reset(i);
        M.add(i);
      }
    }
    return count;
  };
  M.reset(0);
  for (int64_t i = 0; i < n; ++i) M.add(i);
  double lo = 0.0, hi = M.cost_ns();
  while (hi - lo > 1e-4 * hi) {
    const double mid = 0.5 * (lo + hi);
    if (greedy(mid, nullptr) <= nb) hi = mid;
    else lo = mid;
  }
  std::vector<int64_t> cuts;
  greedy(hi, &cuts);
  block_row.assign((size_t)n_blocks + 1, n);
  block_row[0] = 0;
  for (size_t c = 0; c < cuts.size(); ++c) block_row[c + 1] = cuts[c];
  cost_us.assign((size_t)n_blocks, 0.0);
  for (int b = 0; b < n_blocks; ++b) {
    M.reset(block_row[(size_t)b]);
    for (int64_t i = block_row[(size_t)b]; i < block_row[(size_t)b + 1]; ++i) M.add(i);
    cost_us[(size_t)b] = M.cost_ns() * 1e-3;
  }
}

// modelled cost (us) of every block of a partition (the plan log prints it beside what the plan really holds)
inline std::vector<double> ssor_block_costs(const SsorPattern &P, const std::vector<int32_t> &block_row) {
  SsorBlockModel M(P);
  std::vector<double> c(block_row.size() - 1, 0.0);
  for (size_t b = 0; b + 1 < block_row.size(); ++b) {
    M.reset(block_row[b]);
    for (int64_t i = block_row[b]; i < block_row[b + 1]; ++i) M.add(i);
    c[b] = M.cost_ns() * 1e-3;
  }
  return c;
}

// The part of a level matrix one SSOR block [rb, re) sweeps: its pruned entries (stored value != 0, column inside the
// block; local column numbers), which rows couple at all, and the dependency stages
// stage(i) = 1 + max stage(j) over the j < i coupled to i through a_ij or a_ji.  false: a row's columns do not ascend.
struct SsorBlockGraph {
  std::vector<int32_t> prp, pcol, stage, crow, sptr, by_stage;  // crow: coupled rows, ascending; by_stage[sptr[t] .. sptr[t + 1]): those of stage t
  std::vector<double> pval;
  std::vector<char> coupled;
  int n_stages = 0;
};
// sptr / by_stage of the coupled rows crow (ascending) with stages stage[]: rows ascending inside a stage
inline void ssor_rows_by_stage(const std::vector<int32_t> &crow, const std::vector<int32_t> &stage, int n_stages, std::vector<int32_t> &sptr, std::vector<int32_t> &by_stage) {
  sptr.assign((size_t)n_stages + 1, 0);
  by_stage.assign(crow.size(), 0);
  for (int32_t i : crow) sptr[(size_t)stage[(size_t)i] + 1]++;
  for (int t = 0; t < n_stages; ++t) sptr[(size_t)t + 1] += sptr[(size_t)t];
  if (n_stages > 0) {
    std::vector<int32_t> pos(sptr.begin(), sptr.end() - 1);
    for (int32_t i : crow) by_stage[(size_t)pos[(size_t)stage[(size_t)i]]++] = i;
  }
}
inline bool ssor_block_graph(int64_t rb, int64_t re, const int64_t *rp, const int32_t *col, const double *val, SsorBlockGraph &B) {
  const int m = (int)(re - rb);
  B.prp.assign((size_t)m + 1, 0); B.pcol.clear(); B.pval.clear();
  B.coupled.assign((size_t)m, 0);
  std::vector<int32_t> low_cnt((size_t)m + 1, 0);
  for (int i = 0; i < m; ++i) {
    for (int64_t k = rp[rb + i]; k < rp[rb + i + 1]; ++k) {
      const int64_t c = col[k];
      if (k > rp[rb + i] && c <= col[k - 1]) return false;
      if (c < rb || c >= re || val[k] == 0.0) continue;
      B.pcol.push_back((int32_t)(c - rb));
      B.pval.push_back(val[k]);
      if (c != rb + i) {
        B.coupled[(size_t)i] = 1; B.coupled[(size_t)(c - rb)] = 1;
        low_cnt[(size_t)std::max<int64_t>(i, c - rb) + 1]++;
      }
    }
    B.prp[(size_t)i + 1] = (int32_t)B.pcol.size();
  }
  for (int i = 0; i < m; ++i) low_cnt[(size_t)i + 1] += low_cnt[(size_t)i];
  std::vector<int32_t> low((size_t)low_cnt[(size_t)m]), fill(low_cnt.begin(), low_cnt.end() - 1);
  for (int i = 0; i < m; ++i)
    for (int32_t k = B.prp[(size_t)i]; k < B.prp[(size_t)i + 1]; ++k)
      if (B.pcol[(size_t)k] != i) low[(size_t)fill[(size_t)std::max(i, B.pcol[(size_t)k])]++] = std::min(i, B.pcol[(size_t)k]);
  B.stage.assign((size_t)m, 0);
  B.n_stages = 0;
  B.crow.clear();
  for (int i = 0; i < m; ++i) {
    if (!B.coupled[(size_t)i]) continue;
    int st = 0;
    for (int32_t k = low_cnt[(size_t)i]; k < low_cnt[(size_t)i + 1]; ++k) st = std::max(st, B.stage[(size_t)low[(size_t)k]] + 1);
    B.stage[(size_t)i] = st;
    B.n_stages = std::max(B.n_stages, st + 1);
    B.crow.push_back(i);
  }
  ssor_rows_by_stage(B.crow, B.stage, B.n_stages, B.sptr, B.by_stage);
  return true;
}

// ---- rows scheduled by slack ("Rows scheduled by slack") ------------------------------------------------------
// A stage of more than kPhMaxRows rows costs the four-wave sweep several dependent steps, although many of its rows have no
// reader in the next stage and could wait.  The packed LEVELS are a list schedule of the same graph:
//   height(i) = 0 if row i has no higher coupled neighbour, else 1 + max height(k) over its higher neighbours;
//   step t = 0, 1, ...: a row is ready when all its lower coupled neighbours lie in steps < t; the step takes at most
//   kPhMaxRows ready rows, height descending, then row ascending;  level(i) = the row's step.
// Every coupled lower neighbour lies in a lower level, so the levels stand wherever the stages stood: the forward sweep takes
// them ascending, the backward sweep descending, and a row's value -- its CSR-ordered sum over values that are final -- does
// not depend on the step that computes it.  Where no stage has more than kPhMaxRows rows the levels ARE the stages.  Integers
// only, O(nnz + rows log rows), the same result on every rank.  stage_steps: the steps the stages need (kPhMaxRows rows each).
struct SsorLevels {
  std::vector<int32_t> level, sptr, by_level;  // as stage / sptr / by_stage of the block graph
  int n_levels = 0;
  int64_t stage_steps = 0;
};
inline void ssor_pack_levels(const SsorBlockGraph &B, SsorLevels &Lv) {
  const size_t m = B.stage.size();
  Lv.level.assign(m, 0);
  Lv.n_levels = 0;
  Lv.stage_steps = 0;
  for (int t = 0; t < B.n_stages; ++t) Lv.stage_steps += (B.sptr[(size_t)t + 1] - B.sptr[(size_t)t] + kPhMaxRows - 1) / kPhMaxRows;
  // higher neighbours of every row (an entry stored both ways counts twice, here and in the count of lower ones)
  std::vector<int32_t> up_ptr(m + 1, 0), n_low(m, 0), height(m, 0);
  for (size_t i = 0; i < m; ++i)
    for (int32_t k = B.prp[i]; k < B.prp[i + 1]; ++k)
      if (B.pcol[(size_t)k] != (int32_t)i) {
        up_ptr[(size_t)std::min<int32_t>((int32_t)i, B.pcol[(size_t)k]) + 1]++;
        n_low[(size_t)std::max<int32_t>((int32_t)i, B.pcol[(size_t)k])]++;
      }
  for (size_t i = 0; i < m; ++i) up_ptr[i + 1] += up_ptr[i];
  std::vector<int32_t> up((size_t)up_ptr[m]), fill(up_ptr.begin(), up_ptr.end() - 1);
  for (size_t i = 0; i < m; ++i)
    for (int32_t k = B.prp[i]; k < B.prp[i + 1]; ++k)
      if (B.pcol[(size_t)k] != (int32_t)i) up[(size_t)fill[(size_t)std::min<int32_t>((int32_t)i, B.pcol[(size_t)k])]++] = std::max<int32_t>((int32_t)i, B.pcol[(size_t)k]);
  for (size_t i = m; i-- > 0;)
    for (int32_t k = up_ptr[i]; k < up_ptr[i + 1]; ++k) height[i] = std::max(height[i], height[(size_t)up[(size_t)k]] + 1);
  // the ready rows: greatest height first, then the lowest row (key = height << 32 | ~row, the largest key on top)
  auto key = [&](int32_t i) { return (uint64_t)(uint32_t)height[(size_t)i] << 32 | (uint32_t)~(uint32_t)i; };
  std::priority_queue<uint64_t> ready;
  for (int32_t i : B.crow)
    if (n_low[(size_t)i] == 0) ready.push(key(i));
  std::vector<int32_t> taken;
  for (int t = 0; !ready.empty(); ++t) {
    taken.clear();
    while (!ready.empty() && (int)taken.size() < kPhMaxRows) {
      taken.push_back((int32_t)~(uint32_t)(ready.top() & 0xffffffffu));
      ready.pop();
    }
    for (int32_t i : taken) Lv.level[(size_t)i] = t;
    for (int32_t i : taken)  // (after the step is complete: a row freed here is ready for the next step, not for this one)
      for (int32_t k = up_ptr[(size_t)i]; k < up_ptr[(size_t)i + 1]; ++k)
        if (--n_low[(size_t)up[(size_t)k]] == 0) ready.push(key(up[(size_t)k]));
    Lv.n_levels = t + 1;
  }
  ssor_rows_by_stage(B.crow, Lv.level, Lv.n_levels, Lv.sptr, Lv.by_level);
}

// ---- steps of one sweep direction of a block, and the y slots of a self-contained range (gmg_sgs_phase.hpp) ----------
// prp / pcol: the block's pruned entries (stored value != 0, column inside the block; local numbers, ascending);
// sptr / by_stage: its coupled rows stage by stage, ascending inside a stage.  dir 0 = forward, 1 = backward.
struct SsorStep { int32_t first, nrows, len; };  // rows seq[first, first + nrows) of one stage; len: entries of its widest row

inline int ssor_dir_entries(const std::vector<int32_t> &prp, const std::vector<int32_t> &pcol, int dir, int i) {
  int c = 0;
  for (int32_t k = prp[(size_t)i]; k < prp[(size_t)i + 1]; ++k) c += dir == 0 ? pcol[(size_t)k] < i : pcol[(size_t)k] >= i;
  return c;
}

// The steps: the stages in sweep order, at most max_rows rows of a stage per step (one-wave sweep: records of a step
// <= kSwMaxBlock bytes), a step's rows and columns <= y_cap slots.  Rows of a stage are independent: the backward sweep
// takes them in descending order, so that the rows a backward range updates are a DEscending contiguous piece of ycur,
// as those of a forward range are an ascending one.
inline void ssor_build_steps(int dir, int n_stages, const std::vector<int32_t> &sptr, const std::vector<int32_t> &by_stage, const std::vector<int32_t> &prp,
                      const std::vector<int32_t> &pcol, int max_rows, bool ph, int stride, int y_cap, std::vector<int32_t> &seq, std::vector<SsorStep> &steps) {
  seq.clear(); steps.clear();
  seq.reserve(by_stage.size());
  for (int t = 0; t < n_stages; ++t) {
    const int tt = dir == 0 ? t : n_stages - 1 - t;
    SsorStep cur{(int32_t)seq.size(), 0, 0};
    for (int32_t qq = sptr[(size_t)tt]; qq < sptr[(size_t)tt + 1]; ++qq) {
      const int32_t q = dir == 0 ? qq : sptr[(size_t)tt] + sptr[(size_t)tt + 1] - 1 - qq;
      const int i = by_stage[(size_t)q];
      const int li = ssor_dir_entries(prp, pcol, dir, i);
      const int nl = std::max(cur.len, li);
      const int64_t raw = 16 + (int64_t)(cur.nrows + 1) * stride;
      if (cur.nrows > 0 && (cur.nrows == max_rows || (!ph && raw > kSwMaxBlock) || (cur.nrows + 1) * (nl + 1) > y_cap)) {
        steps.push_back(cur);
        cur = SsorStep{(int32_t)seq.size(), 0, 0};
      }
      cur.len = std::max(cur.len, li);
      cur.nrows++;
      seq.push_back(i);
    }
    if (cur.nrows) steps.push_back(cur);
  }
}

// y slots of a whole sweep direction as ONE range: a row owns a slot from its step to the step of its last reader (a
// row i of this direction with a pruned entry a_ic it gathers: c < i forward, c > i backward; the row itself counts).
// Walking the steps in order, the slots of the rows whose last reader is behind are returned to a free list before the
// step's rows take theirs, lowest free slot first -- deterministic.  A slot is free for step s when its owner's last
// reader is < s - 1: a step touches its rows' slots one phase before its dependent phase already (backward, it puts the
// row's forward value there; forward, the padding entries of a record read it), while the step before may still
// read or write (gmg_sgs_phase.hpp).
// A row nobody reads still gets a slot (the step stores to it).  n_slots = the most slots ever live = the highest + 1.
struct SsorSlotPlan {
  std::vector<int32_t> step, last, slot;  // per row of the block; -1: a row without couplings
  int n_slots = 0;
};
inline void ssor_slot_alloc(int m, const std::vector<int32_t> &prp, const std::vector<int32_t> &pcol, int dir, const std::vector<int32_t> &seq,
                     const std::vector<SsorStep> &steps, SsorSlotPlan &out) {
  out.step.assign((size_t)m, -1); out.last.assign((size_t)m, -1); out.slot.assign((size_t)m, -1);
  out.n_slots = 0;
  for (size_t s = 0; s < steps.size(); ++s)
    for (int u = 0; u < steps[s].nrows; ++u) out.step[(size_t)seq[(size_t)(steps[s].first + u)]] = (int32_t)s;
  for (int32_t i : seq) {
    out.last[(size_t)i] = std::max(out.last[(size_t)i], out.step[(size_t)i]);
    for (int32_t k = prp[(size_t)i]; k < prp[(size_t)i + 1]; ++k) {
      const int c = pcol[(size_t)k];
      if (dir == 0 ? c < i : c > i) out.last[(size_t)c] = std::max(out.last[(size_t)c], out.step[(size_t)i]);
    }
  }
  const int hold = 2;  // steps behind the last reader before the slot changes hands
  std::vector<std::vector<int32_t>> due(steps.size() + 1);  // rows whose slot is free from step s on
  std::priority_queue<int32_t, std::vector<int32_t>, std::greater<int32_t>> free_slots;
  for (size_t s = 0; s < steps.size(); ++s) {
    for (int32_t i : due[s]) free_slots.push(out.slot[(size_t)i]);
    for (int u = 0; u < steps[s].nrows; ++u) {
      const int i = seq[(size_t)(steps[s].first + u)];
      if (free_slots.empty()) out.slot[(size_t)i] = out.n_slots++;
      else { out.slot[(size_t)i] = free_slots.top(); free_slots.pop(); }
      const size_t rel = (size_t)out.last[(size_t)i] + (size_t)hold;
      if (rel < steps.size()) due[rel].push_back(i);
    }
  }
}

// ---- block boundaries -------------------------------------------------------------------------------------------------------
// The caller's (explicit_rows, checked by gmg_set_level_matrix), else the balanced cuts if that mode is on, else equal runs of rows.
inline std::vector<int32_t> ssor_block_rows(int64_t n, const int64_t *rp, const int32_t *col, const double *val, const std::vector<int64_t> *explicit_rows,
                                            bool balanced, int blocks) {
  if (explicit_rows) return std::vector<int32_t>(explicit_rows->begin(), explicit_rows->end());
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(blocks, (n + 63) / 64));
  std::vector<int32_t> block_row((size_t)nb + 1);
  if (balanced) {
    std::vector<int64_t> br;
    std::vector<double> cost;
    ssor_balance(SsorPattern(n, rp, col, val), nb, br, cost);
    block_row.assign(br.begin(), br.end());
  } else {
    for (int b = 0; b <= nb; ++b) block_row[(size_t)b] = (int32_t)(n * b / nb);
  }
  return block_row;
}

// ---- the generic sweep: SGS level schedule on the symmetrised pattern, per block of consecutive rows -------------------------
// stage(i) = 1 + max stage(j) over the coupled j < i of the same block; every STORED entry couples, stored zeros included
// (ssor_block_graph prunes them: the two recurrences are not the same).
struct SsorGenericPlan {
  std::vector<int32_t> stage_ptr, stage_rows, block_stage;  // per block its stage offsets (absolute positions in stage_rows); rows stage by stage
  int n_stages_max = 0;
};
inline SsorGenericPlan ssor_generic_plan(int64_t n, const int64_t *rp, const int32_t *col, const std::vector<int32_t> &block_row) {
  std::vector<int64_t> trp;
  std::vector<int32_t> tcol;
  std::vector<double> tval, ones((size_t)rp[n], 1.0);
  transpose_host(n, n, rp, col, ones.data(), trp, tcol, tval);
  const int n_blocks = (int)block_row.size() - 1;
  SsorGenericPlan G;
  G.block_stage.assign((size_t)n_blocks + 1, 0);
  G.stage_rows.resize((size_t)std::max<int64_t>(n, 1));
  std::vector<int32_t> stage((size_t)std::max<int64_t>(n, 1), 0);
  for (int b = 0; b < n_blocks; ++b) {
    const int64_t rb = block_row[(size_t)b], re = block_row[(size_t)b + 1];
    int ns = 0;
    for (int64_t i = rb; i < re; ++i) {
      int s = 0;
      for (int64_t k = rp[i]; k < rp[i + 1]; ++k)
        if (col[k] < i && col[k] >= rb) s = std::max(s, stage[(size_t)col[k]] + 1);
      for (int64_t k = trp[(size_t)i]; k < trp[(size_t)i + 1]; ++k)
        if (tcol[(size_t)k] < i && tcol[(size_t)k] >= rb) s = std::max(s, stage[(size_t)tcol[(size_t)k]] + 1);
      stage[(size_t)i] = s;
      ns = std::max(ns, s + 1);
    }
    if (re == rb) ns = 0;
    std::vector<int32_t> cnt((size_t)ns + 1, 0);
    for (int64_t i = rb; i < re; ++i) cnt[(size_t)stage[(size_t)i] + 1]++;
    for (int t = 0; t < ns; ++t) cnt[(size_t)t + 1] += cnt[(size_t)t];
    std::vector<int32_t> pos(cnt.begin(), cnt.end());
    for (int64_t i = rb; i < re; ++i) G.stage_rows[(size_t)(rb + pos[(size_t)stage[(size_t)i]]++)] = (int32_t)i;
    for (int t = 0; t <= ns; ++t) G.stage_ptr.push_back((int32_t)(rb + cnt[(size_t)t]));
    G.block_stage[(size_t)b + 1] = G.block_stage[(size_t)b] + ns;
    G.n_stages_max = std::max(G.n_stages_max, ns);
  }
  return G;
}

// ---- the plan of the wavefront sweep (gmg_sgs.hpp): per block the pruned rows, the dependency stages, the steps of both ------
// sweep directions, their grouping into LDS-sized ranges (or one self-contained range per direction where the live rows fit),
// and the record stream in consumption order.
enum SsorOutcome {
  kSsorPlanned,      // the vectors below are the plan
  kSsorGeneric,      // the level keeps the generic sweep; message: unsorted columns, stream beyond 2^31, wave disabled, empty level
  kSsorOneWave,      // the four-wave plan cannot be made (a step or a chunk without a shape, stream beyond 2^31): plan again with allow_phase = false
  kSsorUnsupported,  // message: what the matrix asks for that the sweep cannot do
  kSsorInvalid       // message: which of check_sweep_plan's bounds the plan fails (internal error)
};
struct SsorSweepPlan {
  SsorOutcome outcome = kSsorPlanned;
  const char *message = "";
  bool phased = false, dep = false, reg = false;  // four waves in turn; records laid out for gmg_sgs_dep.hpp / gmg_sgs_reg.hpp (both field-major)
  std::vector<SwRange> ranges;     // one-wave plan
  std::vector<PhRange> pranges;    // four-wave plan
  std::vector<PhBlkEntry> blk_tab;
  std::vector<int32_t> block_rng, ws_ci, ci_row, row_ci, rpos_f, rpos_b;
  std::vector<char> stream;
  std::vector<double> iso_diag, iso_invd;
  std::vector<int32_t> bwd_rows;  // the aux words of the self-contained backward records, in stream order
  std::vector<int64_t> block_steps, block_bytes;  // per block: sub-steps of both directions, bytes of the stream
  int y_slots = 0, lds_bytes = 0, n_self = 0, live_max[2] = {0, 0}, n_bwd = 0;
  int64_t total_steps = 0, total_stages = 0;
  // the schedule (gmg_get_ssor_schedule): blocks whose rows are scheduled by slack (their levels count as total_stages), steps of
  // the forward direction, and the steps of a direction if every block walked its stages, the plan's rows per step at a time
  // (kPhMaxRows; one-wave plan: 64 -- there and in a ranged plan fwd_steps can hold more: a step is also cut by its records'
  // bytes and by y_cap).  n_pack_no_slots / n_pack_no_shape: blocks that kept their stages because the packed levels did not
  // fit the y slots / had a step without a shape.
  int n_packed = 0, n_pack_no_slots = 0, n_pack_no_shape = 0;
  int64_t fwd_steps = 0, stage_steps = 0;
  std::vector<int64_t> hist_g = std::vector<int64_t>(4, 0), hist_l1 = std::vector<int64_t>(8, 0), hist_l2 = std::vector<int64_t>(4, 0);  // shapes of the steps
  double laps[4] = {0, 0, 0, 0};  // where the host spends the plan's time (seconds): block graph, steps + slots, shapes, record fill
  int n_ranges() const { return (int)(phased ? pranges.size() : ranges.size()); }
};

struct SsorRowCut { int32_t ne, first, last; };  // a row's entries in a direction, index of the first and of the last late column (none: ne, ne - 1)
struct SsorShape { int g, l1, l2; };

// shape of a step: head (8 G) | T1 (L1: from the first late column to the last, gathered in the dependent phase) | T2 (L2: behind
// the last late column, products formed ahead).  A row may give the end of its head and the start of its T2 to T1; of the shapes
// every row of cut[u0, u1) fits, the one with the cheapest phase (measured costs, cycles) for `rows` rows per step (g < 0: none).
inline SsorShape ssor_choose_shape(const SsorPlanOptions &opt, bool dep, bool reg, const std::vector<SsorRowCut> &cut, size_t u0, size_t u1, double rows) {
  double best = 1e300;
  SsorShape bs{-1, 0, 0};
  for (int g = 0; g <= 3; ++g)
    for (int l1 = 4; l1 <= 28; l1 += 4)
      for (int l2 = 0; l2 <= 24; l2 += 8) {
        if (!ph_shape_ok(g, l1, l2) || (opt.phase_nosplit && l2 > 0) || (dep && l1 > kDpMaxL1)) continue;
        bool ok = true;
        for (size_t u = u0; u < u1 && ok; ++u) ok = sp::fits(cut[u].ne, cut[u].first, cut[u].last, g, l1, l2, nullptr, nullptr);
        if (!ok) continue;
        // default: the measured phase costs (sp::shape_cost, shared with the device builder)
        // (dep: the dependent wave's step is what counts -- ~20 cycles per T1 slot, ~8 per T2 add; the rest is the prep waves')
        // (reg: no copy, no read-back; the record is 2 + 6 g + 0.75 (l1 + l2) load instructions of ~20 cycles)
        double cost;
        if (dep) {
          cost = 20.0 * l1 + 8.0 * l2 + 2.0 * g;
        } else if (reg) {
          const double crit = 330.0 + 15.0 * l1 + 4.0 * l2, p2 = 100.0 + 11.0 * (8 * g + l2), load = 60.0 + 20.0 * (2.0 + 6.0 * g + 0.75 * (l1 + l2));
          cost = std::max(std::max(crit, load), p2) + 0.1 * (crit + load + p2);
        } else {
          cost = sp::shape_cost(g, l1, l2, rows);
        }
        if (cost < best) { best = cost; bs = SsorShape{g, l1, l2}; }
      }
  return bs;
}

// The state of one plan while it is made: the block in work, the direction in work, and one function per piece of the plan.
struct SsorSweepBuilder {
  const SsorPlanOptions &opt;
  SsorSweepPlan &P;
  bool ph = false, dep = false, reg = false, fieldmajor = false, slide_ok = false, pack = false;
  int late_steps = 1, y_max = 0, y_cap = 0, max_ws = 0;
  std::chrono::steady_clock::time_point lap_t = std::chrono::steady_clock::now();
  // the block in work: rows [rb, rb + m) and their graph.  *_stamp[i] == the id of a range: row i is in its working set / has a
  // slot / is updated there; step_of: the step (of that range) that updates it; prefix_pos: index (doubles) of the row's prefix
  // field in the backward records
  int64_t rb = 0;
  SsorBlockGraph B;
  std::vector<int32_t> ws_stamp, own_stamp, tmp_stamp, upd_stamp, slot_of, step_of, prefix_pos;
  int stamp_id = 0, tmp_id = 0;
  std::vector<SwRange> dir_ranges[2];
  std::vector<PhRange> dir_pranges[2];
  // the direction in work (0 = forward, 1 = backward) and its steps
  int dir = 0;
  std::vector<int32_t> seq;
  std::vector<SsorStep> steps;

  SsorSweepBuilder(const SsorPlanOptions &o, SsorSweepPlan &p) : opt(o), P(p) {}
  void lap(int k) {
    const auto t = std::chrono::steady_clock::now();
    P.laps[k] += std::chrono::duration<double>(t - lap_t).count();
    lap_t = t;
  }
  bool stop(SsorOutcome o, const char *why) { P.outcome = o; P.message = why; return false; }
  template <class F>
  void for_rows(size_t s0, size_t s1, F f) const {  // f(step - s0, row) over the rows of steps [s0, s1)
    for (size_t st = s0; st < s1; ++st)
      for (int u = 0; u < steps[st].nrows; ++u) f((int32_t)(st - s0), (int)seq[(size_t)(steps[st].first + u)]);
  }
  // entries of a row in this direction: forward = the columns j < i (y_j = 0 for j >= i); backward = the columns j >= i, continuing
  // the forward sum.  f(k, column)
  template <class F>
  void for_entries(int i, F f) const {
    for (int32_t k = B.prp[(size_t)i]; k < B.prp[(size_t)i + 1]; ++k)
      if (dir == 0 ? B.pcol[(size_t)k] < i : B.pcol[(size_t)k] >= i) f(k, (int)B.pcol[(size_t)k]);
  }

  // groups per sub-step for this direction: every step needs ceil(widest row / 8 g) sub-steps, a sub-step of g groups costs about
  // 3 + g units (measured: ~300 + 100 g cycles); steps are roughly the stages
  int choose_groups() const {
    if (opt.groups > 0) return std::min(4, opt.groups);
    std::vector<int> stage_len((size_t)B.n_stages, 0);
    for (int32_t i : B.crow) stage_len[(size_t)B.stage[(size_t)i]] = std::max(stage_len[(size_t)B.stage[(size_t)i]], ssor_dir_entries(B.prp, B.pcol, dir, i));
    int g_dir = 2;
    double best = 1e300;
    for (int gg = 1; gg <= 4; ++gg) {
      double cost = 0;
      for (int t = 0; t < B.n_stages; ++t) cost += (double)std::max(1, (stage_len[(size_t)t] + 8 * gg - 1) / (8 * gg)) * (3.0 + gg);
      if (cost < best) { best = cost; g_dir = gg; }
    }
    return g_dir;
  }

  // The greedy range from step s0: the longest run of steps whose rows + referenced rows fit y_cap, and its slots -- the rows
  // updated here first (step order), then the rows only read (first touch).  Returns its end; s0: step s0 alone exceeds y_cap.
  size_t greedy_range(size_t s0, SwRange &R) {
    size_t s1 = s0;
    int ws = 0;
    while (s1 < steps.size()) {
      ++tmp_id;
      int add = 0;
      auto count = [&](int r) {
        if (ws_stamp[(size_t)r] != stamp_id && tmp_stamp[(size_t)r] != tmp_id) { tmp_stamp[(size_t)r] = tmp_id; ++add; }
      };
      for_rows(s1, s1 + 1, [&](int32_t, int i) { count(i); for_entries(i, [&](int32_t, int c) { count(c); }); });
      if (ws + add > y_cap) {
        if (s1 > s0) break;
        return s0;
      }
      ws += add;
      for_rows(s1, s1 + 1, [&](int32_t, int i) { ws_stamp[(size_t)i] = stamp_id; for_entries(i, [&](int32_t, int c) { ws_stamp[(size_t)c] = stamp_id; }); });
      ++s1;
    }
    int n_slot = 0;
    auto take = [&](int r) {
      own_stamp[(size_t)r] = stamp_id;  // now "has a slot"
      slot_of[(size_t)r] = n_slot++;
      P.ws_ci.push_back(P.row_ci[(size_t)(rb + r)]);
    };
    for_rows(s0, s1, [&](int32_t, int i) { take(i); });
    R.n_own = n_slot;
    for_rows(s0, s1, [&](int32_t, int i) { for_entries(i, [&](int32_t, int c) { if (own_stamp[(size_t)c] != stamp_id) take(c); }); });
    R.n_ws = n_slot;
    max_ws = std::max(max_ws, n_slot);
    return s1;
  }

  // The row cuts of steps [s0, s1), in step order: a row's TAIL starts at its first column updated by one of the late_steps steps
  // right before its own (step_of / upd_stamp are set for the range)
  std::vector<SsorRowCut> row_cuts(size_t s0, size_t s1) const {
    std::vector<SsorRowCut> cut;
    for_rows(s0, s1, [&](int32_t st, int i) {
      int ne = 0, first_late = -1, last_late = -1;
      for_entries(i, [&](int32_t, int c) {
        if (c != i && upd_stamp[(size_t)c] == stamp_id && step_of[(size_t)c] >= st - late_steps && step_of[(size_t)c] < st) {
          if (first_late < 0) first_late = ne;
          last_late = ne;
        }
        ++ne;
      });
      if (first_late < 0) { first_late = ne; last_late = ne - 1; }
      cut.push_back(SsorRowCut{ne, first_late, last_late});
    });
    return cut;
  }

  // The shapes of steps [s0, s1).  A wave pays ~400 cycles when its next step has another shape (another stretch of code): the
  // steps are taken in chunks, one shape per chunk -- the cheapest that holds every row of the chunk.  false: a step or a chunk
  // has no shape.
  bool choose_shapes(size_t s0, size_t s1, const std::vector<SsorRowCut> &cut, std::vector<SsorShape> &shape_of) const {
    const size_t ns = s1 - s0;
    std::vector<size_t> cpos(ns + 1, 0);
    for (size_t q = 0; q < ns; ++q) cpos[q + 1] = cpos[q] + (size_t)steps[s0 + q].nrows;
    shape_of.resize(ns);
    for (size_t q = 0; q < ns; ++q) {
      shape_of[q] = ssor_choose_shape(opt, dep, reg, cut, cpos[q], cpos[q + 1], (double)steps[s0 + q].nrows);
      if (shape_of[q].g < 0) return false;
    }
    const size_t chunk = (size_t)(opt.phase_chunk > 0 ? opt.phase_chunk : 32);
    for (size_t q0 = 0; q0 < ns; q0 += chunk) {
      const size_t q1 = std::min(ns, q0 + chunk);
      const SsorShape bs = ssor_choose_shape(opt, dep, reg, cut, cpos[q0], cpos[q1], (double)(cpos[q1] - cpos[q0]) / (double)(q1 - q0));
      if (bs.g < 0) return false;
      std::fill(shape_of.begin() + (std::ptrdiff_t)q0, shape_of.begin() + (std::ptrdiff_t)q1, bs);
    }
    return true;
  }

  // One four-wave record (row u of step S, shape sh) into the block at blk = stream + blk_pos.  Four-wave sweep: records lane-major
  // (one row's fields together); dep, reg: FIELD-major -- unit k (16 bytes) of row u at block + 16 + (k * nrows + u) * 16, so that a
  // preparing wave reads a field of all rows with one coalesced load.
  void phase_record(char *blk, int64_t blk_pos, const SsorStep &S, int u, const SsorShape &sh, const SsorRowCut &rc, bool sliding) {
    const int gW = sh.g, l1W = sh.l1, Lr = sh.l1 + sh.l2, pstride = ph_stride(gW, Lr);
    const int i = seq[(size_t)(S.first + u)];
    const int32_t ci = P.row_ci[(size_t)(rb + i)];
    alignas(16) char rec_tmp[32 + 96 * 3 + 12 * kPhMaxEntries + 32];
    char *rec = fieldmajor ? rec_tmp : blk + 16 + (size_t)u * pstride;
    const int64_t rec_pos = fieldmajor ? blk_pos + 16 + (int64_t)u * 16 : blk_pos + 16 + (int64_t)u * pstride;
    const int64_t pre_pos = fieldmajor ? blk_pos + 16 + ((int64_t)S.nrows + u) * 16 : rec_pos + 16;
    (dir == 0 ? P.rpos_f : P.rpos_b)[(size_t)ci] = (int32_t)(rec_pos / 8);
    if (dir == 1) prefix_pos[(size_t)i] = (int32_t)(pre_pos / 8);
    double *f = reinterpret_cast<double *>(rec);
    uint32_t *wv = reinterpret_cast<uint32_t *>(rec);
    const uint32_t my = (uint32_t)slot_of[(size_t)i] * 8u;
    f[0] = 0.0; f[1] = P.iso_invd[(size_t)(rb + i)]; f[2] = 0.0;
    wv[6] = my;
    // aux: forward, where the row's sum goes; backward, self-contained: the level row the result is stored to
    wv[7] = dir == 0 ? (uint32_t)prefix_pos[(size_t)i] : sliding ? (uint32_t)(rb + i) : 0u;
    if (dir == 1 && sliding) P.bwd_rows.push_back((int32_t)wv[7]);  // (host copy of what the records carry: gmg_get_ssor_backward_rows)
    double *hv = f + 4, *tv = f + 4 + 8 * gW;
    uint32_t *ha = reinterpret_cast<uint32_t *>(rec + 32 + 64 * gW + 8 * Lr), *ta = ha + 8 * gW;
    for (int e = 0; e < 8 * gW; ++e) { hv[e] = 0.0; ha[e] = my; }
    for (int e = 0; e < Lr; ++e) { tv[e] = 0.0; ta[e] = my; }
    // head [0, h0), T1 [h0, h1), T2 [h1, ne)
    int h0 = 0, h1 = rc.ne, e = 0;
    (void)sp::fits(rc.ne, rc.first, rc.last, gW, l1W, sh.l2, &h0, &h1);
    for_entries(i, [&](int32_t k, int c) {
      const uint32_t ad = (uint32_t)slot_of[(size_t)c] * 8u;
      if (e < h0) { hv[e] = B.pval[(size_t)k]; ha[e] = ad; }
      else if (e < h1) { tv[e - h0] = B.pval[(size_t)k]; ta[e - h0] = ad; }
      else { tv[l1W + e - h1] = B.pval[(size_t)k]; ta[l1W + e - h1] = ad; }
      ++e;
    });
    if (fieldmajor)
      for (int k = 0; k < (32 + 96 * gW + 12 * Lr) / 16; ++k) std::memcpy(blk + 16 + ((size_t)k * S.nrows + (size_t)u) * 16, rec_tmp + 16 * k, 16);
  }

  // prefetch wave: pf_step bytes per phase starting pf_lead bytes ahead, never behind block p + 12 at phase p (off: the range's bytes)
  void prefetch(PhRange &R, int64_t off) const {
    const PhBlkEntry *tab = P.blk_tab.data() + R.blk_tab;
    const int64_t nph = R.n_steps + kPhWaves - 1;
    const int64_t step_b = ((off + nph - 1) / nph + 127) / 128 * 128;
    int64_t lead = 65536;
    for (int64_t q = 0; q < R.n_steps; ++q) {
      const int64_t need = (int64_t)tab[std::min<int64_t>(q + 12, R.n_steps - 1)].off + kPhRegion;  // by phase q - 2
      lead = std::max(lead, need - std::max<int64_t>(q - 2, 0) * step_b);
    }
    if (opt.pf_lead_kb > 0) lead = std::max<int64_t>(lead, (int64_t)opt.pf_lead_kb * 1024);  // (diagnostics: a longer lead / no prefetch at all)
    R.pf_step = (uint32_t)step_b; R.pf_lead = (uint32_t)((lead + 8191) / 8192 * 8192);
    // Measured in round 3: the four-wave sweep with LDS copies gains nothing from the touches (2.455 ms without, 2.485 with:
    // its copies have two phases to land either way), the register variant loses 10 % without them -- so only that one, or
    // an explicit lead, keeps the fifth wave busy.
    if (opt.pf_lead_kb < 0 || (opt.pf_lead_kb == 0 && !fieldmajor)) R.pf_step = R.pf_lead = 0;
  }

  // The four-wave range of steps [s0, s1) with the slots of R (self-contained: n_slots of the allocator): row cuts, shapes, block
  // table, records, headers.  false: no four-wave plan (outcome kSsorOneWave).
  bool phase_range(size_t s0, size_t s1, const SwRange &R, bool sliding, int n_slots) {
    for_rows(s0, s1, [&](int32_t st, int i) { step_of[(size_t)i] = st; upd_stamp[(size_t)i] = stamp_id; });
    const std::vector<SsorRowCut> cut = row_cuts(s0, s1);
    std::vector<SsorShape> shape_of;
    if (!choose_shapes(s0, s1, cut, shape_of)) return stop(kSsorOneWave, "a step without a shape");
    lap(2);
    PhRange R4{};
    R4.ws_off = R.ws_off; R4.n_own = R.n_own; R4.n_ws = R.n_ws; R4.backward = dir;
    // the rows updated here as a piece of ycur (sweep-order numbering): first index and direction, if they are one
    R4.own_ci0 = R.n_own > 0 ? P.ws_ci[(size_t)R.ws_off] : 0;
    R4.own_dir = dir == 0 ? 1 : -1;
    for (int k = 0; k < R.n_own && R4.own_dir; ++k)
      if (P.ws_ci[(size_t)R.ws_off + (size_t)k] != R4.own_ci0 + R4.own_dir * k) R4.own_dir = 0;
    if (sliding) { R4.own_dir = 0; R4.pad0[0] = 1; R4.pad0[1] = n_slots; ++P.n_self; }
    R4.n_steps = (int32_t)(s1 - s0);
    const int64_t base = ((int64_t)P.stream.size() + 1023) / 1024 * 1024;
    R4.stream_off = base;
    R4.blk_tab = (uint32_t)P.blk_tab.size();
    int64_t off = 0;
    size_t tix = 0;
    for (size_t st = s0; st < s1; ++st) {
      const SsorStep &S = steps[st];
      const SsorShape sh = shape_of[st - s0];
      // T1 slots the step's own rows need of the chunk's shape (the dependent phase stops there)
      int t1_used = 0;
      for (int u = 0; u < S.nrows; ++u) {
        int h0 = 0, h1 = 0;
        (void)sp::fits(cut[tix + (size_t)u].ne, cut[tix + (size_t)u].first, cut[tix + (size_t)u].last, sh.g, sh.l1, sh.l2, &h0, &h1);
        t1_used = std::max(t1_used, h1 - h0);
      }
      t1_used = opt.phase_nocascade ? sh.l1 : std::min(sh.l1, std::max(4, (t1_used + 3) / 4 * 4));
      // (storing the records at the step's OWN width -- head groups, T1 and T2 slots its rows really have -- was measured in
      // round 3: the stream shrinks by 13 % only, a step's widest row is nearly as wide as its chunk's, and the branches that
      // make P2 and CRIT stop at the step's counts cost more than the shorter copy saves: 2.52 against 2.48 ms)
      const int64_t raw = 16 + (int64_t)S.nrows * ph_stride(sh.g, sh.l1 + sh.l2);
      P.blk_tab.push_back(PhBlkEntry{(uint32_t)off, (uint32_t)raw, (uint32_t)ph::ph_key(sh.g, sh.l1, sh.l2) | ((uint32_t)S.nrows << 8) | ((uint32_t)t1_used << 16), 0u});
      P.stream.resize((size_t)(base + off + raw), 0);
      for (int u = 0; u < S.nrows; ++u) phase_record(P.stream.data() + base + off, base + off, S, u, sh, cut[tix++], sliding);
      off += (raw + 15) / 16 * 16;
      P.hist_l1[(size_t)std::min(7, sh.l1 / 4)]++; P.hist_l2[(size_t)(sh.l2 / 8)]++; P.hist_g[(size_t)sh.g]++;
    }
    const PhBlkEntry *tab = P.blk_tab.data() + R4.blk_tab;
    for (int q = 0; q + kPhWaves < R4.n_steps; ++q) {  // a block's header: the block its reader copies next, and that step's shape
      uint32_t *h = reinterpret_cast<uint32_t *>(P.stream.data() + base + tab[q].off);
      h[1] = tab[q + kPhWaves].bytes; h[2] = tab[q + kPhWaves].off; h[3] = tab[q + kPhWaves].word;
    }
    const int64_t padded = (off + 2048 + 1023) / 1024 * 1024;  // the copies read whole KB: up to 1008 bytes beyond a block
    if (padded >= ((int64_t)1 << 31) || (base + padded) / 8 >= ((int64_t)1 << 31)) return stop(kSsorOneWave, "stream positions beyond 2^31");
    P.stream.resize((size_t)(base + padded), 0);
    R4.stream_bytes = (uint32_t)padded;
    prefetch(R4, off);
    P.total_steps += R4.n_steps;
    dir_pranges[dir].push_back(R4);
    lap(3);
    return true;
  }

  // The one-wave range of steps [s0, s1), g groups per sub-step: records in consumption order; a block never straddles the end of
  // the ring.  false: stream positions beyond 2^31 (outcome kSsorGeneric).
  bool wave_range(size_t s0, size_t s1, SwRange &R, int g) {
    const int w_dir = 8 * g, stride = sw_stride(g);
    const int64_t base = ((int64_t)P.stream.size() + kSwChunk - 1) / kSwChunk * kSwChunk;
    R.stream_off = base;
    int64_t off = 0, prev_hdr = -1;
    auto link = [&](uint32_t next_raw, int next_nrows) {  // the header before: how far to the next one, and what lies there
      SwStepHdr h;
      std::memcpy(&h, P.stream.data() + base + prev_hdr, sizeof h);
      h.advance = (uint32_t)(off - prev_hdr); h.next_raw = next_raw;
      if (next_raw) h.next_nrows = (uint16_t)next_nrows;
      std::memcpy(P.stream.data() + base + prev_hdr, &h, sizeof h);
    };
    for (size_t st = s0; st < s1; ++st) {
      const SsorStep &S = steps[st];
      const int nr = S.nrows, n_sub = std::max(1, (S.len + w_dir - 1) / w_dir);
      for (int sub = 0; sub < n_sub; ++sub) {
        const int64_t raw = 16 + (int64_t)nr * stride;
        if (off % kSwRing + raw > kSwRing) off = (off / kSwRing + 1) * kSwRing;
        P.stream.resize((size_t)(base + off + raw), 0);
        char *blk = P.stream.data() + base + off;
        SwStepHdr h{};
        h.nrows = (uint16_t)nr;
        h.flags = (uint16_t)((sub == 0 ? 1 : 0) | (sub == n_sub - 1 ? 2 : 0));
        std::memcpy(blk, &h, sizeof h);
        if (prev_hdr >= 0) link((uint32_t)raw, nr);
        else { R.first_raw = (int32_t)raw; R.first_nrows = nr; }
        prev_hdr = off;
        for (int u = 0; u < nr; ++u) {
          const int i = seq[(size_t)(S.first + u)];
          const int32_t ci = P.row_ci[(size_t)(rb + i)];
          char *rec = blk + 16 + (size_t)u * stride;
          const int64_t rec_pos = base + off + 16 + (int64_t)u * stride;
          if (sub == n_sub - 1) (dir == 0 ? P.rpos_f : P.rpos_b)[(size_t)ci] = (int32_t)(rec_pos / 8);  // the rhs is read when the row is finished
          if (dir == 1 && sub == 0) prefix_pos[(size_t)i] = (int32_t)(rec_pos / 8 + 2);                 // the prefix when it is started
          double *f = reinterpret_cast<double *>(rec);
          uint32_t *w = reinterpret_cast<uint32_t *>(rec);
          const uint32_t my = (uint32_t)slot_of[(size_t)i] * 8u;
          f[0] = 0.0; f[1] = P.iso_invd[(size_t)(rb + i)]; f[2] = 0.0;
          w[6] = my;
          w[7] = dir == 0 ? (uint32_t)prefix_pos[(size_t)i] : 0u;
          uint32_t *ad = reinterpret_cast<uint32_t *>(rec + 32 + 64 * g);
          int e = 0, seen = 0;
          for_entries(i, [&](int32_t k, int c) {
            if (seen++ < sub * w_dir || e >= 8 * g) return;  // entries of earlier / of later sub-steps
            f[4 + e] = B.pval[(size_t)k];
            ad[e++] = (uint32_t)slot_of[(size_t)c] * 8u;
          });
          for (; e < 8 * g; ++e) { f[4 + e] = 0.0; ad[e] = my; }
        }
        off += raw;
        R.n_steps++;
      }
    }
    if (prev_hdr >= 0) link(0, 0);  // last step: advance = its own size, nothing follows
    const int64_t padded = (off + kSwChunk - 1) / kSwChunk * kSwChunk;
    if (padded >= ((int64_t)1 << 31) || (base + padded) / 8 >= ((int64_t)1 << 31)) return stop(kSsorGeneric, "stream positions beyond 2^31");
    P.stream.resize((size_t)(base + padded), 0);
    R.stream_bytes = (int32_t)padded;
    P.total_steps += R.n_steps;
    dir_ranges[dir].push_back(R);
    return true;
  }

  // One block: its graph, the numbering of its coupled rows, and both directions -- backward first: the forward records point
  // into the backward ones.  false: P.outcome says why there is no plan.
  bool block(int64_t rb_, int64_t re, const int64_t *rp, const int32_t *col, const double *val) {
    rb = rb_;
    const int m = (int)(re - rb);
    // in-block nonzero entries of every row (local column numbers), stages; a_ii as stored, and 1 / a_ii (1 where none is stored)
    if (!ssor_block_graph(rb, re, rp, col, val, B)) return stop(kSsorGeneric, "unsorted columns");  // the prefix hand-over needs ascending columns
    for (int64_t i = rb; i < re; ++i)
      for (int64_t k = rp[i]; k < rp[i + 1]; ++k)
        if (col[k] == i) { P.iso_diag[(size_t)i] = val[k]; P.iso_invd[(size_t)i] = 1.0 / val[k]; }
    lap(0);
    const size_t ci_base = P.ci_row.size();
    P.ci_row.resize(ci_base + B.crow.size());
    P.rpos_f.resize(P.ci_row.size(), 0);
    P.rpos_b.resize(P.ci_row.size(), 0);
    if (B.crow.empty()) return true;
    const int step_rows = ph ? kPhMaxRows : 64;  // (the plan's own rows per step, so that the two counts of the schedule compare)
    for (int t = 0; t < B.n_stages; ++t) P.stage_steps += (B.sptr[(size_t)t + 1] - B.sptr[(size_t)t] + step_rows - 1) / step_rows;
    // self-contained ranges: both directions of the block must fit; else the ranged plan, unchanged.  The records are built from
    // the very lists of steps the slots were handed out for.
    SsorSlotPlan slide[2];
    std::vector<int32_t> slide_seq[2];
    std::vector<SsorStep> slide_steps[2];
    auto self_contained = [&]() {  // steps and slots of both directions as one range each; do they fit?
      bool fits = true;
      for (int d = 0; d < 2; ++d) {
        ssor_build_steps(d, B.n_stages, B.sptr, B.by_stage, B.prp, B.pcol, kPhMaxRows, true, 0, y_max, slide_seq[d], slide_steps[d]);
        ssor_slot_alloc(m, B.prp, B.pcol, d, slide_seq[d], slide_steps[d], slide[d]);
        if (((slide[d].n_slots + 1) & ~1) > y_cap) fits = false;
      }
      return fits;
    };
    // every step of both directions has a shape, chunk by chunk: the row cuts and shapes exactly as phase_range forms them for a
    // self-contained range (a whole level in the step before its readers can put more than 28 columns between a row's first and
    // last late column, which no shape holds)
    auto shapes_exist = [&]() {
      bool ok = true;
      for (int d = 0; d < 2 && ok; ++d) {
        dir = d;
        seq.swap(slide_seq[d]); steps.swap(slide_steps[d]);
        ++stamp_id;
        for_rows(0, steps.size(), [&](int32_t st, int i) { step_of[(size_t)i] = st; upd_stamp[(size_t)i] = stamp_id; });
        std::vector<SsorShape> shape_of;
        ok = choose_shapes(0, steps.size(), row_cuts(0, steps.size()), shape_of);
        seq.swap(slide_seq[d]); steps.swap(slide_steps[d]);
      }
      dir = 0;
      return ok;
    };
    // Rows scheduled by slack: the packed levels stand in for the stages if both directions still fit the y slots (the backward
    // sweep takes the same levels in reverse, which keeps its rows near their readers) and every packed step has a shape; else
    // the stages, exactly as without them.
    bool sliding = false, slots_known = false;
    if (pack) {
      SsorLevels Lv;
      ssor_pack_levels(B, Lv);
      auto exchange = [&]() { B.stage.swap(Lv.level); B.sptr.swap(Lv.sptr); B.by_stage.swap(Lv.by_level); std::swap(B.n_stages, Lv.n_levels); };
      exchange();
      for (std::vector<int32_t> *v : {&upd_stamp, &step_of}) v->assign((size_t)m, -1);
      stamp_id = 0;
      const bool fits = self_contained();
      sliding = slots_known = fits && shapes_exist();
      if (sliding) ++P.n_packed;
      else { exchange(); ++(fits ? P.n_pack_no_shape : P.n_pack_no_slots); }
    }
    if (slide_ok && !slots_known) sliding = self_contained();
    if (slide_ok)
      for (int d = 0; d < 2; ++d) P.live_max[d] = std::max(P.live_max[d], slide[d].n_slots);
    lap(1);
    P.total_stages += B.n_stages;
    // The compact copy ycur is numbered in SWEEP order (stage by stage): the rows a forward range updates are one contiguous
    // piece of it, those of a backward range a run of stage-long pieces -- the working-set loads and write-backs at the range
    // boundaries (a tenth of the sweep) then touch consecutive addresses instead of one cache line per row.
    for (size_t q = 0; q < B.by_stage.size(); ++q) {
      P.row_ci[(size_t)(rb + B.by_stage[q])] = (int32_t)(ci_base + q);
      P.ci_row[ci_base + q] = (int32_t)(rb + B.by_stage[q]);
    }
    for (std::vector<int32_t> *v : {&ws_stamp, &own_stamp, &tmp_stamp, &upd_stamp, &step_of}) v->assign((size_t)m, -1);
    slot_of.assign((size_t)m, 0); prefix_pos.assign((size_t)m, 0);
    stamp_id = tmp_id = 0;
    for (int d = 0; d < 2; ++d) { dir_ranges[d].clear(); dir_pranges[d].clear(); }
    for (dir = 1; dir >= 0; --dir) {
      const int g_dir = choose_groups();
      // steps: <= 64 rows of one stage, records of a sub-step <= kSwMaxBlock bytes, working set <= y_cap (self-contained: the
      // allocator's own lists -- the LDS bound is the allocator's, not the step's)
      if (sliding) { seq.swap(slide_seq[dir]); steps.swap(slide_steps[dir]); }
      else ssor_build_steps(dir, B.n_stages, B.sptr, B.by_stage, B.prp, B.pcol, ph ? kPhMaxRows : 64, ph, ph ? ph_stride(3, 12) : sw_stride(g_dir), y_cap, seq, steps);
      if (dir == 0) P.fwd_steps += (int64_t)steps.size();
      for (size_t s0 = 0, s1 = 0; s0 < steps.size(); s0 = s1) {
        ++stamp_id;
        SwRange R{};
        R.ws_off = (int32_t)P.ws_ci.size();
        R.backward = dir;
        R.groups = g_dir;
        if (sliding) {  // the whole direction is the range: the allocator's slots, no working-set list (n_own = n_ws = 0)
          s1 = steps.size();
          for (int32_t i : seq) slot_of[(size_t)i] = slide[dir].slot[(size_t)i];
          max_ws = std::max(max_ws, slide[dir].n_slots);
        } else {
          s1 = greedy_range(s0, R);
          if (s1 == s0) return stop(kSsorUnsupported, "SGS plan: one step exceeds the LDS working set");
        }
        if (!(ph ? phase_range(s0, s1, R, sliding, slide[dir].n_slots) : wave_range(s0, s1, R, g_dir))) return false;
      }
    }
    dir = 0;
    for (int d = 0; d < 2; ++d) P.ranges.insert(P.ranges.end(), dir_ranges[d].begin(), dir_ranges[d].end());
    for (int d = 0; d < 2; ++d) P.pranges.insert(P.pranges.end(), dir_pranges[d].begin(), dir_pranges[d].end());
    return true;
  }
};

// The plan of the level's sweep for block boundaries block_row.  allow_phase: four waves in turn (gmg_sgs_phase.hpp) unless
// switched off; outcome kSsorOneWave asks for a second call without it (rows wider than its records hold, a stream beyond 2^31).
inline void ssor_sweep_plan(const SsorPlanOptions &opt, int64_t n, const int64_t *rp, const int32_t *col, const double *val,
                            const std::vector<int32_t> &block_row, bool allow_phase, SsorSweepPlan &P) {
  P = SsorSweepPlan();
  SsorSweepBuilder S(opt, P);
  if (n <= 0 || opt.disable_wave) { S.stop(kSsorGeneric, n <= 0 ? "empty level" : "wave disabled"); return; }
  const int n_blocks = (int)block_row.size() - 1;
  bool ph = allow_phase && !opt.disable_phase && !opt.profile;
  for (int64_t i = 0; i < n && ph; ++i) ph = rp[i + 1] - rp[i] <= 2 * kPhMaxEntries;  // (cheap pre-check; the exact one is per range)
  S.ph = P.phased = ph;
  S.dep = P.dep = ph && opt.dep;                           // one dependent wave + three preparing waves (gmg_sgs_dep.hpp)
  S.reg = P.reg = ph && !S.dep && opt.reg && !opt.chain;  // four waves, records global -> registers (gmg_sgs_reg.hpp)
  S.fieldmajor = S.dep || S.reg;
  // one self-contained range per direction (gmg_sgs_phase.hpp) where a block's live rows fit: the default four-wave sweep only
  S.slide_ok = ph && !S.dep && !S.reg && !opt.chain && opt.sliding;
  S.pack = S.slide_ok && ssor_pack_wanted(opt, n);  // rows scheduled by slack: this plan only, the others keep the stages
  S.late_steps = S.dep ? kDpLate : 1;
  S.y_max = S.dep ? kDpYSlots : S.reg ? kRgYSlots : ph ? kPhYSlots : kSwYSlots;
  S.y_cap = std::max(64, std::min(opt.y_slots > 0 ? opt.y_slots : S.y_max, S.y_max)) & ~1;
  P.row_ci.assign((size_t)n, -1);
  P.block_rng.assign((size_t)n_blocks + 1, 0);
  P.iso_diag.assign((size_t)n, 0.0); P.iso_invd.assign((size_t)n, 1.0);
  P.block_steps.assign((size_t)n_blocks, 0); P.block_bytes.assign((size_t)n_blocks, 0);
  for (int b = 0; b < n_blocks; ++b) {
    const int64_t steps0 = P.total_steps, bytes0 = (int64_t)P.stream.size();
    P.block_rng[(size_t)b] = P.n_ranges();
    if (block_row[(size_t)b + 1] > block_row[(size_t)b] && !S.block(block_row[(size_t)b], block_row[(size_t)b + 1], rp, col, val)) return;
    P.block_steps[(size_t)b] = P.total_steps - steps0; P.block_bytes[(size_t)b] = (int64_t)P.stream.size() - bytes0;
  }
  P.block_rng[(size_t)n_blocks] = P.n_ranges();
  P.y_slots = std::max(2, (S.max_ws + 1) & ~1);
  P.lds_bytes = P.dep   ? P.y_slots * 8 + kDpSlots * ((kDpSlotBytes + 15) / 16 * 16) + kDpFlagBytes
                : P.reg ? P.y_slots * 8 + kPhJunk
                : ph    ? P.y_slots * 8 + kPhWaves * kPhRegion + kPhJunk
                        : P.y_slots * 8 + kSwRing + 32;
  for (const PhRange &R : P.pranges) P.n_bwd += R.backward;
  for (const SwRange &R : P.ranges) P.n_bwd += R.backward;
  S.lap(3);
}

// The plan is memory-safe by construction, and checked: every address a record carries lies inside what is allocated (DESIGN.md 8:
// both faults this code ever produced were stores through an aux field).  From the plan's arrays alone: the forward records' aux
// (a global store index, in doubles into the stream), the self-contained backward records' aux (a level row), the LDS byte
// addresses of y slots, ws_ci, rpos_*.  nullptr: the plan passes; else which bound it fails.
inline const char *check_sweep_plan(const SsorSweepPlan &P, int64_t n) {
  static const char *const bad_rec = "SSOR plan: a record addresses memory outside the stream / the LDS slots (internal error)",
                    *const bad_bwd = "SSOR plan: a backward record stores outside the level vector (internal error)";
  const uint64_t size = P.stream.size(), lds = (uint64_t)P.y_slots * 8;
  std::atomic<bool> ok{true}, ok_bwd{true};
  // words 6 (own slot), 7 (aux) of a record and its n_ad slot addresses; unit(o): where byte o of the record lies
  auto record = [&](auto unit, int ad_off, int n_ad, bool backward, bool self) {
    const uint32_t my = *reinterpret_cast<const uint32_t *>(unit(24)), aux = *reinterpret_cast<const uint32_t *>(unit(28));
    bool good = (uint64_t)my + 8 <= lds && (backward || (uint64_t)aux * 8 + 8 <= size);
    for (int e = 0; e < n_ad; ++e) good = good && (uint64_t)*reinterpret_cast<const uint32_t *>(unit(ad_off + 4 * e)) + 8 <= lds;
    if (!good) ok = false;
    if (backward && self && aux >= (uint64_t)n) ok_bwd = false;
  };
  for (const PhRange &R : P.pranges) {
    if (R.n_steps < 0 || R.stream_off < 0 || (size_t)R.blk_tab + (size_t)R.n_steps > P.blk_tab.size()) return bad_rec;
    parallel_chunks(R.n_steps, [&](int64_t q0, int64_t q1, int) {  // (on a few threads: the stream of a large level has tens of MB)
      for (int64_t q = q0; q < q1; ++q) {
        const PhBlkEntry &e = P.blk_tab[(size_t)R.blk_tab + (size_t)q];
        int g, l1, l2;
        sp::key_shape((int)(e.word & 255u), &g, &l1, &l2);
        const int nrows = (int)(e.word >> 8 & 255u), stride = ph_stride(g, l1 + l2);
        if (!ph_shape_ok(g, l1, l2) || (uint64_t)R.stream_off + e.off + 16 + (uint64_t)nrows * stride > size) { ok = false; continue; }
        const char *blk = P.stream.data() + R.stream_off + e.off;
        for (int u = 0; u < nrows; ++u)
          record([&](int o) { return P.dep || P.reg ? blk + 16 + ((size_t)(o / 16) * nrows + u) * 16 + o % 16 : blk + 16 + (size_t)u * stride + o; },
                 32 + 64 * g + 8 * (l1 + l2), 8 * g + l1 + l2, R.backward != 0, R.pad0[0] == 1);
      }
    });
  }
  for (const SwRange &R : P.ranges) {
    int64_t pos = R.stream_off;
    for (int s = 0; s < R.n_steps; ++s) {
      if (pos < 0 || (uint64_t)pos + 16 > size) return bad_rec;
      SwStepHdr h;
      std::memcpy(&h, P.stream.data() + pos, sizeof h);
      if (R.groups < 1 || R.groups > 4 || (uint64_t)pos + 16 + (uint64_t)h.nrows * sw_stride(R.groups) > size) return bad_rec;
      for (int u = 0; u < h.nrows; ++u)
        record([&](int o) { return P.stream.data() + pos + 16 + (size_t)u * sw_stride(R.groups) + o; }, 32 + 64 * R.groups, 8 * R.groups, R.backward != 0, false);
      pos += h.advance;
    }
  }
  if (!ok) return bad_rec;
  for (int32_t r : P.bwd_rows) ok_bwd = ok_bwd && r >= 0 && r < n;
  if (!ok_bwd) return bad_bwd;
  for (int32_t ci : P.ws_ci)
    if (ci < 0 || (size_t)ci >= P.ci_row.size()) return "SSOR plan: working-set entry out of range (internal error)";
  for (size_t q = 0; q < P.rpos_f.size(); ++q)
    if ((uint64_t)P.rpos_f[q] * 8 + 8 > size || (uint64_t)P.rpos_b[q] * 8 + 8 > size) return "SSOR plan: rhs position outside the stream (internal error)";
  return nullptr;
}

}  // namespace gmg
