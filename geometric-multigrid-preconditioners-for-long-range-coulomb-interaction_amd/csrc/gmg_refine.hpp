// gmg_refine.hpp -- the step between two cycles formed on the device from the forest alone:
//   gmg_refine_forest     Forest::refine_flagged (csrc/host/forest.h): the 2:1 closure of the marks over vertices and the split;
//   gmg_transfer_solution SolutionTransfer::interpolate + constraints.set_zero (src/step-50.cc:1095-1121;
//                         LaplaceProblem::refine_grid in csrc/host/adaptive.inc);
//   gmg_build_face_table  LaplaceProblem::face_table, the input of gmg_estimate_error.
// gmg_build_face_table_resident and gmg_refine_forest_marked run the same kernels on a face table and on
// marks that stay in the context; rf_mark_flag_kernel forms the latter's flags.
// The host restates p4est's refine + balance and deal.II's transfer as sequential loops over hash maps; the kernels here restate
// those loops order-free, with the tools of gmg_mesh_tables.hpp (mt_insert / mt_find, the cell table by coordinates, the
// one-workgroup scan, the flag word):
//   closure   a flag on level l - 1 is caused only by a flagged cell of level l, so one kernel per level from the finest level
//             down to level 1 reaches the fixed point; the flags are set by equal plain stores of 1;
//   split     new level l + 1 = old level l + 1, then the children of the split cells of level l in ascending cell index: the
//             rank of a split cell comes from a scan over the flags, every thread writes its own cell and its own children;
//   transfer  one thread per (cell of level >= 1, vertex) slot: a vertex without an old value takes the Q1 interpolant of the
//             parent cell.  Several slots may supply the same vertex; they store EQUAL bits (argument at gmg_transfer_solution
//             in include/gmg_coulomb.h), so no supplier is chosen: equal plain stores;
//   faces     one thread per (cell, face) slot, look-ups only.
// Every probe loop runs at most once round its table, no thread waits for another, integer atomics (the compare-and-swap of
// mt_insert, atomicOr on the flag word) and plain stores only, no LDS but the scan's.  fp64 without contraction.
#pragma once
#include "gmg_mesh_tables.hpp"

namespace gmg {

constexpr int kRfErrMissing = 8, kRfErrOrphan = 16, kRfErrFace = 32;  // further bits of the flag word (kMtErr*)

// (the loop of gmg_mesh_tables.hpp, which keeps its macro to itself)
#define MT_FOR(i, n) for (int64_t i = (int64_t)blockIdx.x * kMtThreads + threadIdx.x; i < (n); i += (int64_t)gridDim.x * kMtThreads)

// one level's cells by coordinates (mt_cell_insert_kernel): index[position] = the cell's index inside the level
struct RfLevel {
  const unsigned long long *keys;
  const int32_t *index;
  unsigned long long mask;
  int64_t begin, n;  // the level's cells among all cells
};

// the cell of the level at (x, y, z) >= 0, -1: none
__device__ __forceinline__ int64_t rf_cell(const RfLevel &L, int32_t x, int32_t y, int32_t z) {
  const int64_t h = mt_find(L.keys, L.mask, mt_pack((unsigned long long)x, (unsigned long long)y, (unsigned long long)z));
  return h < 0 ? -1 : (int64_t)L.index[h];
}

// ---- gmg_refine_forest
// a flag counts only on an active cell
__global__ __launch_bounds__(kMtThreads) void rf_flag_kernel(const int32_t *first_child, const uint8_t *flag, int64_t n_cells, uint8_t *F) {
  MT_FOR(c, n_cells) F[c] = flag[c] && first_child[c] < 0 ? 1 : 0;
}
// gmg_refine_forest_marked: the flags of the forest's cells from the marks of its active cells; apos is the exclusive scan of
// mt_active_flag_kernel, so apos[c] is the active number of an active cell c (below the number of marks: the entry counts)
__global__ __launch_bounds__(kMtThreads) void rf_mark_flag_kernel(const int32_t *first_child, const int32_t *apos, const uint8_t *mark, int64_t n_cells, uint8_t *flag) {
  MT_FOR(c, n_cells) flag[c] = first_child[c] < 0 ? mark[apos[c]] : 0;
}
// one thread per (cell of the level, neighbour position): reads F on this level, writes F on the level below
__global__ __launch_bounds__(kMtThreads) void rf_closure_kernel(MtForest f, int level, RfLevel cur, RfLevel coarse, uint8_t *F, int *err) {
  const int nn = f.dim == 3 ? 27 : 9;
  MT_FOR(i, cur.n * nn) {
    const int64_t cell = cur.begin + i / nn;
    if (!F[cell]) continue;
    const int k = (int)(i % nn);
    const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = f.dim == 3 ? k / 9 - 1 : 0;
    if (!dx && !dy && !dz) continue;
    const int64_t x = (int64_t)f.coord[3 * cell] + dx, y = (int64_t)f.coord[3 * cell + 1] + dy, z = (int64_t)f.coord[3 * cell + 2] + dz;
    if (x < 0 || y < 0 || z < 0 || x >= ((int64_t)f.n0[0] << level) || y >= ((int64_t)f.n0[1] << level) || (f.dim == 3 && z >= ((int64_t)f.n0[2] << level))) continue;
    if (rf_cell(cur, (int32_t)x, (int32_t)y, (int32_t)z) >= 0) continue;
    const int64_t p = rf_cell(coarse, (int32_t)(x >> 1), (int32_t)(y >> 1), (int32_t)(z >> 1));
    if (p < 0) { atomicOr(err, kMtErrUnbalanced); continue; }
    F[coarse.begin + p] = 1;
  }
}
__global__ __launch_bounds__(kMtThreads) void rf_split_flag_kernel(const uint8_t *F, int64_t n_cells, int32_t *rank) {
  MT_FOR(c, n_cells) rank[c] = F[c];
}
struct RfSplit {
  const uint8_t *F;
  const int32_t *rank;      // exclusive scan of F over all cells
  int32_t rank_base;        // rank of the level's first cell
  int64_t new_begin, new_begin_next, old_size_next;  // the level and the next one among the new cells; the next one's old size
  int32_t *coord, *first_child, *parent;             // the new forest
};
// one thread per old cell of the level: the cell itself, and its children when it is split
__global__ __launch_bounds__(kMtThreads) void rf_split_kernel(MtForest f, int level, RfLevel cur, RfLevel coarse, RfSplit s, int *err) {
  MT_FOR(c, cur.n) {
    const int64_t cell = cur.begin + c, o = s.new_begin + c;
    const int32_t x = f.coord[3 * cell], y = f.coord[3 * cell + 1], z = f.coord[3 * cell + 2];
    s.coord[3 * o] = x; s.coord[3 * o + 1] = y; s.coord[3 * o + 2] = z;
    int64_t p = -1;
    if (level > 0) {
      p = rf_cell(coarse, x >> 1, y >> 1, z >> 1);
      if (p < 0) atomicOr(err, kRfErrOrphan);
    }
    s.parent[o] = (int32_t)p;
    if (!s.F[cell]) { s.first_child[o] = f.first_child[cell]; continue; }
    const int64_t fc = s.old_size_next + (int64_t)f.nv * (s.rank[cell] - s.rank_base);
    s.first_child[o] = (int32_t)fc;
    for (int a = 0; a < f.nv; ++a) {
      const int64_t q = s.new_begin_next + fc + a;
      s.coord[3 * q] = 2 * x + (a & 1); s.coord[3 * q + 1] = 2 * y + ((a >> 1) & 1); s.coord[3 * q + 2] = f.dim == 3 ? 2 * z + ((a >> 2) & 1) : 0;
      s.first_child[q] = -1;
      s.parent[q] = (int32_t)c;
    }
  }
}

// ---- gmg_transfer_solution
// vertex -> its position in the list; a vertex met twice raises kMtErrDuplicate
__global__ __launch_bounds__(kMtThreads) void rf_vertex_insert_kernel(const unsigned long long *vertex, int64_t n, unsigned long long *keys, int32_t *index,
                                                                     unsigned long long mask, int *err) {
  MT_FOR(i, n) {
    bool inserted = false;
    const int64_t h = mt_insert(keys, mask, vertex[i], &inserted);
    if (h < 0) { atomicOr(err, kMtErrFull); continue; }
    if (!inserted) { atomicOr(err, kMtErrDuplicate); continue; }
    index[h] = (int32_t)i;
  }
}
struct RfTransfer {
  const unsigned long long *okeys, *nkeys;  // the old and the new vertices
  const int32_t *oidx, *nidx;
  unsigned long long omask, nmask;
  const double *u_old;
  double *u_new;
  uint8_t *have;  // [n_new]: the DoF has its value
  int *err;
};
// 1. a new DoF whose vertex had a value keeps it
__global__ __launch_bounds__(kMtThreads) void rf_transfer_old_kernel(RfTransfer t, const unsigned long long *new_vertex, int64_t n_new) {
  MT_FOR(i, n_new) {
    const int64_t h = mt_find(t.okeys, t.omask, new_vertex[i]);
    if (h >= 0) t.u_new[i] = t.u_old[t.oidx[h]];
    t.have[i] = h >= 0 ? 1 : 0;
  }
}
// 2. one thread per slot (cell of level >= 1, vertex a): the host's loop verbatim
__global__ __launch_bounds__(kMtThreads) void rf_transfer_interp_kernel(MtForest f, int64_t begin, int64_t n_slots, RfTransfer t) {
  MT_FOR(s, n_slots) {
    const int64_t cell = begin + (s >> f.dim);
    const int a = (int)(s & (f.nv - 1));
    const unsigned long long key = mt_vertex_key(f, cell, a);
    if (mt_find(t.okeys, t.omask, key) >= 0) continue;
    const int32_t *c = f.coord + 3 * cell;
    const int child = (c[0] & 1) | ((c[1] & 1) << 1) | (f.dim == 3 ? (c[2] & 1) << 2 : 0);
    const int sp = kMtShift - ((int)f.level[cell] - 1);
    const unsigned long long px = (unsigned long long)(c[0] >> 1), py = (unsigned long long)(c[1] >> 1), pz = (unsigned long long)(c[2] >> 1);
    double v = 0.0;
    bool ok = true;
    for (int p = 0; p < f.nv; ++p) {
      const int64_t h = mt_find(t.okeys, t.omask, mt_pack((px + (p & 1)) << sp, (py + ((p >> 1) & 1)) << sp, f.dim == 3 ? (pz + ((p >> 2) & 1)) << sp : 0ull));
      if (h < 0) { ok = false; continue; }
      double w = 1.0;
      for (int d = 0; d < f.dim; ++d) {
        const double pos = 0.5 * (double)(((child >> d) & 1) + ((a >> d) & 1));
        w *= ((p >> d) & 1) ? pos : 1.0 - pos;
      }
      v += w * t.u_old[t.oidx[h]];
    }
    const int64_t hn = ok ? mt_find(t.nkeys, t.nmask, key) : -1;
    if (hn < 0) { atomicOr(t.err, kRfErrMissing); continue; }
    const int32_t i = t.nidx[hn];
    t.u_new[i] = v;
    t.have[i] = 1;
  }
}
// 3. every DoF has a value; constraints.set_zero
__global__ __launch_bounds__(kMtThreads) void rf_transfer_finish_kernel(RfTransfer t, const int32_t *constraint_of_dof, int64_t n_new) {
  MT_FOR(i, n_new) {
    if (!t.have[i]) { atomicOr(t.err, kRfErrMissing); continue; }
    if (constraint_of_dof && constraint_of_dof[i] >= 0) t.u_new[i] = 0.0;
  }
}

// ---- gmg_build_face_table: the (cell, face) slots of the level's active cells; apos: a cell's position among the active cells
__global__ __launch_bounds__(kMtThreads) void rf_face_kernel(MtForest f, int level, RfLevel cur, RfLevel coarse, int64_t fine_begin, const int32_t *apos,
                                                            uint8_t *face_kind, int32_t *face_cell, int *err) {
  const int nfc = f.nv >> 1;
  MT_FOR(i, cur.n * f.nf) {
    const int64_t cell = cur.begin + i / f.nf;
    if (f.first_child[cell] >= 0) continue;
    const int face = (int)(i % f.nf), d = face >> 1, side = face & 1;
    const int64_t slot = (int64_t)apos[cell] * f.nf + face;
    const int32_t *c = f.coord + 3 * cell;
    int32_t nb[3] = {c[0], c[1], c[2]};
    nb[d] += side ? 1 : -1;
    if (nb[d] < 0 || (int64_t)nb[d] >= ((int64_t)f.n0[d] << level)) continue;  // boundary face: kind 0
    const int64_t N = rf_cell(cur, nb[0], nb[1], nb[2]);
    if (N < 0) {  // a coarser neighbour; this cell's quadrant of its face from the in-face bits of the cell's own position
      const int64_t P = level > 0 ? rf_cell(coarse, nb[0] >> 1, nb[1] >> 1, nb[2] >> 1) : -1;
      const int32_t pa = P >= 0 && f.first_child[coarse.begin + P] < 0 ? apos[coarse.begin + P] : -1;
      int quad = 0, k = 0;
      for (int e = 0; e < f.dim; ++e)
        if (e != d) quad |= (c[e] & 1) << k++;
      face_kind[slot] = 3;
      face_cell[slot * nfc] = pa;
      face_cell[slot * nfc + 1] = quad;
      if (pa < 0) atomicOr(err, kRfErrFace);
    } else if (f.first_child[cur.begin + N] < 0) {
      face_kind[slot] = 1;
      face_cell[slot * nfc] = apos[cur.begin + N];
    } else {
      face_kind[slot] = 2;
      const int64_t child0 = fine_begin + f.first_child[cur.begin + N];
      int k = 0;
      for (int ch = 0; ch < f.nv; ++ch) {
        if (((ch >> d) & 1) != (side ? 0 : 1)) continue;
        const bool active = f.first_child[child0 + ch] < 0;
        face_cell[slot * nfc + k++] = active ? apos[child0 + ch] : -1;
        if (!active) atomicOr(err, kRfErrFace);
      }
    }
  }
}

#undef MT_FOR

}  // namespace gmg
