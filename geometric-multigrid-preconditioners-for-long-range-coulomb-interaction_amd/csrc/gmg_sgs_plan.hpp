// gmg_sgs_plan.hpp -- the plan of the four-wave SSOR sweep (gmg_sgs_phase.hpp) formed on the device from a level's CSR.
//
// What ssor_sweep_plan (gmg_sgs_layout.hpp) builds on the host for the default configuration -- four waves, one self-contained
// range per direction in every block -- is a pure function of the CSR, the block boundaries and y_cap.  The kernels below
// form the same plan, byte for byte, from the CSR as it lies on the device; the host text is the definition of every piece.
// Anything else (another sweep variant, a block whose live rows do not fit, a row without a shape, unsorted columns) is
// found here, reported through the flag word, and the level is planned by the host builder as before.
//
// Numbering.  Level rows i in [0, n); the B blocks are [brow[b], brow[b + 1]).  Coupled rows are numbered ci in sweep order
// (block, stage, row): ci_row / row_ci.  A block with S steps per direction owns 2 S consecutive step indices G: the backward
// steps first (they come first in the record stream and in blk_tab), then the forward ones.  Per-direction row arrays have
// 2 n entries, [dir * n + i].
//
// No kernel waits for another workgroup.  The two sequential recurrences -- stages (a longest path) and y slots (a free list)
// -- run inside ONE workgroup per block (and direction) between barriers; their loops are bounded by the block's coupled rows
// and its steps, both known at launch.  Every other kernel is a grid-stride loop over rows, coupled rows or steps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gmg_sgs_phase.hpp"

namespace gmg {
namespace sp {

// ---- what the host builder and the kernels share: a row's cut against a shape, and the cost of a shape -------------------
// (sp::fits, sp::shape_cost: gmg_sgs_layout.hpp)
// the candidates in loop order (g, then l1, then l2): number c <-> shape
constexpr int kCand = 4 * 7 * 4;
__host__ __device__ inline void cand_shape(int c, int *g, int *l1, int *l2) { *g = c / 28; *l1 = 4 + 4 * (c % 28 / 4); *l2 = 8 * (c % 4); }

// ssor_build_steps cuts a step where (rows + 1) * (widest row + 1) exceeds the y slots: with at most kPhMaxRows rows of at
// most 2 kPhMaxEntries entries that cannot happen for kPhYSlots, so the steps here are plain runs of kPhMaxRows rows
static_assert((kPhMaxRows + 1) * (2 * kPhMaxEntries + 1) <= kPhYSlots, "a step of the self-contained plan would be cut by the y slots");
static_assert(16 + kPhMaxRows * ph_stride(3, 12) <= kPhRegion && 16 + kPhMaxRows * ph_stride(0, 36) <= kPhRegion, "a step's block fits its LDS region");

enum : uint32_t { kUnsorted = 1, kWide = 2, kNoShape = 4, kNoFit = 8, kInternal = 16 };

struct Block {  // one SSOR block as the kernels see it
  int32_t rb, re, q0, nc;  // rows, first coupled index, coupled rows
  int32_t S, g0, rng, pad; // steps per direction, first step index, first range
};

struct Args {
  int64_t n;
  int32_t n_blocks, n_coupled, n_steps, y_cap;
  const int32_t *rp, *col;
  const double *val;
  const int32_t *brow;
  const Block *blk;
  uint32_t *flags;
  // pruned graph
  int32_t *prp, *pcol, *indeg, *upptr, *upfill, *uplist, *ccnt, *stage;
  double *pval;
  uint8_t *coupled;
  // stages and steps
  int32_t *queue, *sptr, *spos, *stepbase, *nstages, *nsteps, *su, *st_bd, *st_nrows, *st_row;
  // slots
  int32_t *last, *dueptr, *duefill, *duelist, *slot, *nslots;
  // shapes and offsets
  int32_t *cut, *shape, *word, *bytes, *off16;
  unsigned long long *mask;
  const int64_t *rbase;
  // the plan
  int32_t *row_ci, *ci_row, *rpos;  // rpos: [dir * n_coupled + ci]
  double *iso_diag, *iso_invd;
  char *stream;
  uint4 *blk_tab;
};

__device__ inline int block_of(const int32_t *brow, int nb, int64_t i) {  // the block [brow[b], brow[b + 1]) that holds row i
  int lo = 0, hi = nb;  // first index with brow[idx] > i lies in (lo, hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (brow[mid] > i) hi = mid; else lo = mid;
  }
  return lo;
}
__device__ inline int step_index(const Block &b, int dir, int s) { return b.g0 + (dir ? 0 : b.S) + s; }
#define SP_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---- 1. pruned block graph (ssor_block_graph): count, [scan], fill ---------------------------------------------------------
// FILL = false: per row the pruned entries (prp), coupled[], the in-degree of the row in the symmetrised pattern and the
// number of higher neighbours per row (upptr), the diagonal terms; the checks "columns ascend" and "row fits the records".
template <bool FILL>
__global__ __launch_bounds__(256) void graph_kernel(Args a) {
  SP_LOOP(i, a.n) {
    const int b = block_of(a.brow, a.n_blocks, i);
    const int64_t rb = a.brow[b], re = a.brow[b + 1];
    const int32_t k0 = a.rp[i], k1 = a.rp[i + 1];
    if constexpr (!FILL) {
      uint32_t bad = k1 - k0 > 2 * kPhMaxEntries ? (uint32_t)kWide : 0u;
      double aii = 1.0, dstored = 0.0;
      int cnt = 0;
      for (int32_t k = k0; k < k1; ++k) {
        const int64_t c = a.col[k];
        if (k > k0 && c <= a.col[k - 1]) bad |= kUnsorted;
        if (c == i) { aii = a.val[k]; dstored = a.val[k]; }
        if (c < rb || c >= re || a.val[k] == 0.0) continue;
        ++cnt;
        if (c != i) {
          a.coupled[i] = 1; a.coupled[c] = 1;
          atomicAdd(&a.indeg[c > i ? c : i], 1);
          atomicAdd(&a.upptr[c > i ? i : c], 1);
        }
      }
      a.prp[i] = cnt;
      a.iso_diag[i] = dstored;
      a.iso_invd[i] = 1.0 / aii;
      if (bad) atomicOr(a.flags, bad);
    } else {
      int32_t o = a.prp[i];
      for (int32_t k = k0; k < k1; ++k) {
        const int64_t c = a.col[k];
        if (c < rb || c >= re || a.val[k] == 0.0) continue;
        a.pcol[o] = (int32_t)c; a.pval[o] = a.val[k]; ++o;
        if (c != i) {
          const int64_t lo = c > i ? i : c, hi = c > i ? c : i;
          a.uplist[a.upptr[lo] + atomicAdd(&a.upfill[lo], 1)] = (int32_t)hi;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void coupled_count_kernel(Args a) {
  SP_LOOP(i, a.n)
    if (a.coupled[i]) atomicAdd(&a.ccnt[block_of(a.brow, a.n_blocks, i)], 1);
}

// ---- 2. stages: stage(i) = 1 + max stage(j) over the lower neighbours, by frontier propagation ------------------------------
// One workgroup per block.  The queue of the block holds its coupled rows stage after stage: the rows whose in-degree is 0
// first, then, for every row taken from the queue, the higher neighbours whose last lower neighbour it was.  sptr / stepbase:
// where each stage starts in the queue, and the steps (runs of kPhMaxRows rows) before it.  At most nc stages.
__global__ __launch_bounds__(1024) void stage_kernel(Args a) {
  __shared__ int head_s, lim_s, tail_s, run_s;
  for (int b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
    const Block B = a.blk[b];
    int32_t *queue = a.queue + B.q0, *sptr = a.sptr + B.q0 + b, *spos = a.spos + B.q0 + b, *stepbase = a.stepbase + B.q0 + b;
    __syncthreads();
    if (threadIdx.x == 0) { head_s = 0; tail_s = 0; run_s = 0; }
    __syncthreads();
    for (int i = B.rb + (int)threadIdx.x; i < B.re; i += blockDim.x)
      if (a.coupled[i] && a.indeg[i] == 0) { a.stage[i] = 0; queue[atomicAdd(&tail_s, 1)] = i; }
    __syncthreads();
    if (threadIdx.x == 0) lim_s = tail_s;
    __syncthreads();
    int t = 0;
    for (; t < B.nc; ++t) {
      const int h = head_s, lim = lim_s;
      if (h == lim) break;
      if (threadIdx.x == 0) { sptr[t] = h; spos[t] = h; stepbase[t] = run_s; run_s += (lim - h + kPhMaxRows - 1) / kPhMaxRows; }
      // (16 lanes per row of the frontier: a stage has ~20 rows of ~7 higher neighbours, and the atomics of one row then go out together)
      for (int q = h + (int)threadIdx.x / 16; q < lim; q += blockDim.x / 16) {
        const int j = queue[q];
        for (int32_t k = a.upptr[j] + (int)threadIdx.x % 16; k < a.upptr[j + 1]; k += 16) {
          const int i = a.uplist[k];
          if (atomicSub(&a.indeg[i], 1) == 1) { a.stage[i] = t + 1; queue[atomicAdd(&tail_s, 1)] = i; }
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) { head_s = lim; lim_s = tail_s; }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      sptr[t] = head_s; stepbase[t] = run_s;
      a.nstages[b] = t; a.nsteps[b] = run_s;
      if (head_s != B.nc || lim_s != B.nc) atomicOr(a.flags, (uint32_t)kInternal);
    }
  }
}

// ---- 3./4. by_stage (rows ascending inside a stage), the ci numbering, and the steps of both directions ---------------------
// A stable counting sort by stage, one workgroup per block: the rows are taken in order, 1024 at a time; a row's place is the
// next free one of its stage (spos, which starts as sptr) plus the rows of the same stage before it in its tile.  Linear in
// the block's rows whatever the sizes of the stages; sptr / stage come from stage_kernel, which wrote spos = sptr.
__global__ __launch_bounds__(1024) void rank_kernel(Args a) {
  __shared__ int32_t st[1024];
  const int tid = threadIdx.x;
  for (int b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
    const Block B = a.blk[b];
    int32_t *spos = a.spos + B.q0 + b;
    for (int base = B.rb; base < B.re; base += 1024) {
      const int i = base + tid;
      const int s = i < B.re && a.coupled[i] ? a.stage[i] : -1;
      __syncthreads();  // (the tile before: its reads of st and its writes of spos are done)
      st[tid] = s;
      __syncthreads();
      int before = 0, total = 0, p0 = 0;
      if (s >= 0) {
        for (int y = 0; y < 1024; ++y) {
          const int eq = st[y] == s;
          total += eq;
          before += eq & (y < tid);
        }
        p0 = spos[s];
      }
      __syncthreads();  // (every row of the tile has read its stage's place before the last one moves it on)
      if (s >= 0) {
        if (before == total - 1) spos[s] = p0 + total;
        const int ci = B.q0 + p0 + before;
        a.ci_row[ci] = i; a.row_ci[i] = ci;
      }
    }
  }
}
// One thread per coupled row: its step and its place in it.  Forward steps take the stages and their rows in ascending order,
// backward steps in descending order, kPhMaxRows rows per step.
__global__ __launch_bounds__(256) void order_kernel(Args a) {
  SP_LOOP(ci, a.n_coupled) {
    const int i = a.ci_row[ci];
    const int b = block_of(a.brow, a.n_blocks, i);
    const Block B = a.blk[b];
    const int32_t *sptr = a.sptr + B.q0 + b, *stepbase = a.stepbase + B.q0 + b;
    const int t = a.stage[i], s0 = sptr[t], s1 = sptr[t + 1], k = s1 - s0;
    const int rank = (int)ci - B.q0 - s0;
    for (int dir = 0; dir < 2; ++dir) {
      const int p = dir ? k - 1 - rank : rank;
      const int s = (dir ? B.S - stepbase[t + 1] : stepbase[t]) + p / kPhMaxRows, u = p % kPhMaxRows;
      const int G = step_index(B, dir, s);
      a.su[(int64_t)dir * a.n + i] = s * kPhMaxRows + u;
      a.st_row[(int64_t)G * kPhMaxRows + u] = i;
      if (u == 0) { a.st_nrows[G] = k - p < kPhMaxRows ? k - p : kPhMaxRows; a.st_bd[G] = 2 * b + dir; }
    }
  }
}

// ---- 5. y slots (ssor_slot_alloc) -------------------------------------------------------------------------------------------
// last reader of every row per direction
__global__ __launch_bounds__(256) void last_kernel(Args a) {
  SP_LOOP(e, 2 * (int64_t)a.n_coupled) {
    const int dir = (int)(e / a.n_coupled);
    const int i = a.ci_row[e % a.n_coupled];
    int32_t *last = a.last + (int64_t)dir * a.n;
    const int s = a.su[(int64_t)dir * a.n + i] / kPhMaxRows;
    atomicMax(&last[i], s);
    for (int32_t k = a.prp[i]; k < a.prp[i + 1]; ++k) {
      const int c = a.pcol[k];
      if (dir == 0 ? c < i : c > i) atomicMax(&last[c], s);
    }
  }
}
// rows whose slot is free again from step last + 2 on, listed per step: count, [scan], fill
template <bool FILL>
__global__ __launch_bounds__(256) void due_kernel(Args a) {
  SP_LOOP(e, 2 * (int64_t)a.n_coupled) {
    const int dir = (int)(e / a.n_coupled);
    const int i = a.ci_row[e % a.n_coupled];
    const Block B = a.blk[block_of(a.brow, a.n_blocks, i)];
    const int rel = a.last[(int64_t)dir * a.n + i] + 2;
    if (rel >= B.S) continue;
    const int G = step_index(B, dir, rel);
    if constexpr (!FILL) atomicAdd(&a.dueptr[G], 1);
    else a.duelist[a.dueptr[G] + atomicAdd(&a.duefill[G], 1)] = i;
  }
}
// One workgroup per (block, direction) walks the steps: the slots that are due go back into the bitmap, then the step's rows
// take the lowest clear bits in row order -- the host's "free list, else one more slot".  The bitmap has y_cap bits: a step that
// finds too few clear ones needs more slots than the range may have (the host plan is the ranged one then).
constexpr int kSlotThreads = 256;
static_assert(kPhYSlots <= 64 * kSlotThreads, "one bitmap word per thread");
__global__ __launch_bounds__(kSlotThreads) void slot_kernel(Args a) {
  __shared__ unsigned long long bm[kSlotThreads];
  __shared__ int wsum[kSlotThreads / 64];
  __shared__ int high_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int bd = blockIdx.x; bd < 2 * a.n_blocks; bd += gridDim.x) {
    const int dir = bd & 1;
    const Block B = a.blk[bd >> 1];
    int32_t *slot = a.slot + (int64_t)dir * a.n;
    __syncthreads();
    // bits at and beyond y_cap are never free
    {
      const int lo = tid * 64;
      bm[tid] = lo >= a.y_cap ? ~0ull : a.y_cap - lo >= 64 ? 0ull : ~0ull << (a.y_cap - lo);
    }
    if (tid == 0) high_s = 0;
    __syncthreads();
    bool full = false;
    for (int s = 0; s < B.S && !full; ++s) {
      const int G = step_index(B, dir, s);
      for (int32_t k = a.dueptr[G] + tid; k < a.dueptr[G + 1]; k += kSlotThreads) {
        const int sl = slot[a.duelist[k]];
        atomicAnd(&bm[sl >> 6], ~(1ull << (sl & 63)));
      }
      __syncthreads();
      const int nr = a.st_nrows[G];
      unsigned long long fr = ~bm[tid];
      const int cnt = __popcll(fr);
      int inc = cnt;  // inclusive scan over the workgroup: inside the wave by shuffles, across the waves through LDS
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
      }
      if (lane == 63) wsum[wave] = inc;
      __syncthreads();
      int pre = inc - cnt, total = 0;
      for (int w = 0; w < kSlotThreads / 64; ++w) { if (w < wave) pre += wsum[w]; total += wsum[w]; }
      if (total < nr) {
        full = true;  // (the same for every thread)
      } else {
        int hi = -1;
        unsigned long long take = 0;
        for (int r = pre; r < nr && fr; ++r) {
          const int pos = __ffsll((long long)fr) - 1;
          fr &= fr - 1;
          take |= 1ull << pos;
          hi = tid * 64 + pos;
          slot[a.st_row[(int64_t)G * kPhMaxRows + r]] = hi;
        }
        if (take) { bm[tid] |= take; atomicMax(&high_s, hi + 1); }
      }
      __syncthreads();
    }
    if (tid == 0) {
      a.nslots[bd] = high_s;
      if (full) atomicOr(a.flags, (uint32_t)kNoFit);
    }
  }
}

// ---- 6. row cuts, the shapes every row of a step fits, chunk shapes, t1_used and step words --------------------------------
__global__ __launch_bounds__(256) void cut_kernel(Args a) {
  SP_LOOP(G, a.n_steps) {
    const int bd = a.st_bd[G], dir = bd & 1;
    const Block B = a.blk[bd >> 1];
    const int s = (int)G - step_index(B, dir, 0), nr = a.st_nrows[G];
    const int32_t *su = a.su + (int64_t)dir * a.n;
    unsigned long long m0 = ~0ull, m1 = ~0ull >> (128 - kCand);
    for (int u = 0; u < nr; ++u) {
      const int i = a.st_row[G * kPhMaxRows + u];
      int ne = 0, first = -1, last = -1;
      for (int32_t k = a.prp[i]; k < a.prp[i + 1]; ++k) {
        const int c = a.pcol[k];
        if (!(dir == 0 ? c < i : c >= i)) continue;
        if (c != i && su[c] / kPhMaxRows == s - 1) {
          if (first < 0) first = ne;
          last = ne;
        }
        ++ne;
      }
      if (first < 0) { first = ne; last = ne - 1; }
      a.cut[G * kPhMaxRows + u] = ne | first << 8 | (last + 1) << 16;
      for (int c = 0; c < kCand; ++c) {
        int g, l1, l2;
        cand_shape(c, &g, &l1, &l2);
        if (!ph_shape_ok(g, l1, l2) || !fits(ne, first, last, g, l1, l2, nullptr, nullptr)) {
          if (c < 64) m0 &= ~(1ull << c); else m1 &= ~(1ull << (c - 64));
        }
      }
    }
    a.mask[2 * G] = m0; a.mask[2 * G + 1] = m1;
  }
}
// one shape per chunk of 32 steps: the cheapest that holds every row of the chunk, ties to the first in loop order
__global__ __launch_bounds__(256) void chunk_kernel(Args a) {
  SP_LOOP(G, a.n_steps) {
    const int bd = a.st_bd[G], dir = bd & 1;
    const Block B = a.blk[bd >> 1];
    const int s = (int)G - step_index(B, dir, 0);
    if (s % 32) continue;
    const int q1 = s + 32 < B.S ? s + 32 : B.S;
    unsigned long long m0 = ~0ull, m1 = ~0ull;
    int64_t rows = 0;
    for (int q = s; q < q1; ++q) { m0 &= a.mask[2 * (G + q - s)]; m1 &= a.mask[2 * (G + q - s) + 1]; rows += a.st_nrows[G + q - s]; }
    const double avg_rows = (double)rows / (double)(q1 - s);
    double best = 1e300;
    int key = -1;
    for (int c = 0; c < kCand; ++c) {
      if (!((c < 64 ? m0 >> c : m1 >> (c - 64)) & 1)) continue;
      int g, l1, l2;
      cand_shape(c, &g, &l1, &l2);
      const double cost = shape_cost(g, l1, l2, avg_rows);
      if (cost < best) { best = cost; key = ph::ph_key(g, l1, l2); }
    }
    if (key < 0) atomicOr(a.flags, (uint32_t)kNoShape);
    for (int q = s; q < q1; ++q) a.shape[G + q - s] = key;
  }
}
__global__ __launch_bounds__(256) void word_kernel(Args a) {
  SP_LOOP(G, a.n_steps) {
    const int key = a.shape[G], nr = a.st_nrows[G];
    if (key < 0) { a.word[G] = 0; a.bytes[G] = 0; a.off16[G] = 0; continue; }
    int g, l1, l2;
    key_shape(key, &g, &l1, &l2);
    int t1 = 0;
    for (int u = 0; u < nr; ++u) {
      const int c = a.cut[G * kPhMaxRows + u];
      int h0 = 0, h1 = 0;
      (void)fits(c & 255, c >> 8 & 255, (c >> 16) - 1, g, l1, l2, &h0, &h1);
      t1 = t1 < h1 - h0 ? h1 - h0 : t1;
    }
    t1 = (t1 + 3) / 4 * 4;
    t1 = t1 < 4 ? 4 : t1;
    t1 = t1 < l1 ? t1 : l1;
    const int raw = 16 + nr * ph_stride(g, l1 + l2);
    a.word[G] = (int32_t)((uint32_t)key | (uint32_t)nr << 8 | (uint32_t)t1 << 16);
    a.bytes[G] = raw;
    a.off16[G] = (raw + 15) / 16;  // [scan]: the step's offset in units of 16 bytes
  }
}
// per range the bytes of its steps (units of 16): what the host needs to lay the ranges out
__global__ __launch_bounds__(256) void range_bytes_kernel(Args a, int32_t *out) {
  SP_LOOP(bd, 2 * (int64_t)a.n_blocks) {
    const Block B = a.blk[bd >> 1];
    const int G0 = step_index(B, (int)(bd & 1), 0);
    out[bd] = a.off16[G0 + B.S] - a.off16[G0];
  }
}

// ---- 8. records -------------------------------------------------------------------------------------------------------------
// where the record of row i of direction dir starts in the stream, and the shape of its step
__device__ inline int64_t record_pos(const Args &a, const Block &B, int dir, int i, int *Gout, int *keyout) {
  const int su = a.su[(int64_t)dir * a.n + i], s = su / kPhMaxRows, u = su % kPhMaxRows;
  const int G0 = step_index(B, dir, 0), G = G0 + s, key = a.shape[G];
  int g, l1, l2;
  key_shape(key, &g, &l1, &l2);
  if (Gout) { *Gout = G; *keyout = key; }
  return a.rbase[B.rng + dir] + (int64_t)(a.off16[G] - a.off16[G0]) * 16 + 16 + (int64_t)u * ph_stride(g, l1 + l2);
}
__global__ __launch_bounds__(256) void record_kernel(Args a) {
  SP_LOOP(e, 2 * (int64_t)a.n_coupled) {
    const int dir = (int)(e / a.n_coupled), ci = (int)(e % a.n_coupled);
    const int i = a.ci_row[ci];
    const Block B = a.blk[block_of(a.brow, a.n_blocks, i)];
    int G, key, g, l1, l2;
    const int64_t rec_pos = record_pos(a, B, dir, i, &G, &key);
    key_shape(key, &g, &l1, &l2);
    const int Lr = l1 + l2, u = a.su[(int64_t)dir * a.n + i] % kPhMaxRows;
    a.rpos[(int64_t)dir * a.n_coupled + ci] = (int32_t)(rec_pos / 8);
    char *rec = a.stream + rec_pos;
    double *f = reinterpret_cast<double *>(rec);
    uint32_t *wv = reinterpret_cast<uint32_t *>(rec);
    const int32_t *slot = a.slot + (int64_t)dir * a.n;
    const uint32_t my = (uint32_t)slot[i] * 8u;
    f[0] = 0.0; f[1] = a.iso_invd[i]; f[2] = 0.0;
    wv[6] = my;
    // aux: forward, the prefix field of the row's backward record (index in doubles); backward, the level row
    wv[7] = dir == 0 ? (uint32_t)((record_pos(a, B, 1, i, nullptr, nullptr) + 16) / 8) : (uint32_t)i;
    double *hv = f + 4, *tv = f + 4 + 8 * g;
    uint32_t *ha = reinterpret_cast<uint32_t *>(rec + 32 + 64 * g + 8 * Lr), *ta = ha + 8 * g;
    for (int q = 0; q < 8 * g; ++q) { hv[q] = 0.0; ha[q] = my; }
    for (int q = 0; q < Lr; ++q) { tv[q] = 0.0; ta[q] = my; }
    const int c3 = a.cut[(int64_t)G * kPhMaxRows + u];
    int h0 = 0, h1 = c3 & 255;
    (void)fits(c3 & 255, c3 >> 8 & 255, (c3 >> 16) - 1, g, l1, l2, &h0, &h1);
    int q = 0;
    for (int32_t k = a.prp[i]; k < a.prp[i + 1]; ++k) {
      const int c = a.pcol[k];
      if (!(dir == 0 ? c < i : c >= i)) continue;
      const uint32_t ad = (uint32_t)slot[c] * 8u;
      if (q < h0) { hv[q] = a.pval[k]; ha[q] = ad; }
      else if (q < h1) { tv[q - h0] = a.pval[k]; ta[q - h0] = ad; }
      else { tv[l1 + q - h1] = a.pval[k]; ta[l1 + q - h1] = ad; }
      ++q;
    }
  }
}
// block table and the headers: words 1 .. 3 of a step's header describe the step kPhWaves on (its reader's next copy)
__global__ __launch_bounds__(256) void header_kernel(Args a) {
  SP_LOOP(G, a.n_steps) {
    const int bd = a.st_bd[G], dir = bd & 1;
    const Block B = a.blk[bd >> 1];
    const int G0 = step_index(B, dir, 0), s = (int)G - G0;
    const uint32_t off = (uint32_t)(a.off16[G] - a.off16[G0]) * 16u;
    a.blk_tab[G] = uint4{off, (uint32_t)a.bytes[G], (uint32_t)a.word[G], 0u};
    if (s + kPhWaves < B.S) {
      uint32_t *h = reinterpret_cast<uint32_t *>(a.stream + a.rbase[B.rng + dir] + off);
      h[1] = (uint32_t)a.bytes[G + kPhWaves]; h[2] = (uint32_t)(a.off16[G + kPhWaves] - a.off16[G0]) * 16u; h[3] = (uint32_t)a.word[G + kPhWaves];
    }
  }
}

// ---- the finished plan, checked from its own arrays before a sweep may run on it -------------------------------------------
// out: [0] error bits, [1] largest forward aux, [2] largest LDS address, [3] largest backward aux (a level row), [4] largest rpos
struct CheckArgs {
  const PhRange *ranges;
  const uint4 *blk_tab;
  const char *stream;
  const int32_t *rpos_f, *rpos_b;
  int32_t n_ranges, n_coupled, y_slots;
  int64_t stream_bytes;
  unsigned long long *out;
};
enum : unsigned long long { kChkTab = 1, kChkRows = 2, kChkKey = 4, kChkNext = 8, kChkLds = 16, kChkRange = 32 };
__global__ __launch_bounds__(256) void check_kernel(CheckArgs a) {
  unsigned long long bad = 0, max_aux = 0, max_lds = 0, max_yrow = 0, max_rpos = 0;
  for (int r = blockIdx.x; r < a.n_ranges; r += gridDim.x) {
    const PhRange P = a.ranges[r];
    if (P.stream_off < 0 || P.stream_off + (int64_t)P.stream_bytes > a.stream_bytes || P.n_steps < 0) { bad |= kChkRange; continue; }
    for (int q = threadIdx.x; q < P.n_steps; q += blockDim.x) {
      const uint4 e = a.blk_tab[P.blk_tab + q];
      const int key = (int)(e.z & 255u), rows = (int)(e.z >> 8 & 255u), t1 = (int)(e.z >> 16);
      int g, l1, l2;
      key_shape(key, &g, &l1, &l2);
      if (e.y > (uint32_t)kPhRegion || (uint64_t)e.x + e.y > P.stream_bytes || e.x % 16) { bad |= kChkTab; continue; }
      if (rows < 1 || rows > kPhMaxRows) { bad |= kChkRows; continue; }
      if (!ph_shape_ok(g, l1, l2) || ph::ph_key(g, l1, l2) != key || t1 < 4 || t1 > l1 || t1 % 4) { bad |= kChkKey; continue; }
      const int stride = ph_stride(g, l1 + l2);
      if ((int64_t)e.y != 16 + (int64_t)rows * stride) { bad |= kChkTab; continue; }
      const char *blk = a.stream + P.stream_off + e.x;
      const uint32_t *h = reinterpret_cast<const uint32_t *>(blk);
      if (q + kPhWaves < P.n_steps) {
        const uint4 nx = a.blk_tab[P.blk_tab + q + kPhWaves];
        if (h[1] != nx.y || h[2] != nx.x || h[3] != nx.z) bad |= kChkNext;
      } else if (h[1] | h[2] | h[3]) bad |= kChkNext;
      for (int u = 0; u < rows; ++u) {
        const uint32_t *wv = reinterpret_cast<const uint32_t *>(blk + 16 + (size_t)u * stride);
        const uint32_t *ad = reinterpret_cast<const uint32_t *>(blk + 16 + (size_t)u * stride + 32 + 64 * g + 8 * (l1 + l2));
        unsigned long long m = wv[6];
        for (int k = 0; k < 8 * g + l1 + l2; ++k) m = m < ad[k] ? ad[k] : m;
        max_lds = max_lds < m ? m : max_lds;
        if (P.backward) max_yrow = max_yrow < wv[7] ? wv[7] : max_yrow;
        else max_aux = max_aux < wv[7] ? wv[7] : max_aux;
      }
    }
  }
  SP_LOOP(ci, a.n_coupled) {
    const unsigned long long f = (unsigned long long)(uint32_t)a.rpos_f[ci], b = (unsigned long long)(uint32_t)a.rpos_b[ci];
    max_rpos = max_rpos < f ? f : max_rpos;
    max_rpos = max_rpos < b ? b : max_rpos;
  }
  if (max_lds + 8 > (unsigned long long)a.y_slots * 8) bad |= kChkLds;
  if (bad) atomicOr(&a.out[0], bad);
  if (max_aux) atomicMax(&a.out[1], max_aux);
  if (max_lds) atomicMax(&a.out[2], max_lds);
  if (max_yrow) atomicMax(&a.out[3], max_yrow);
  if (max_rpos) atomicMax(&a.out[4], max_rpos);
}
#undef SP_LOOP

}  // namespace sp
}  // namespace gmg
