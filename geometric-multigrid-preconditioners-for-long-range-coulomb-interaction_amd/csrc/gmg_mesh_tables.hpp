// gmg_mesh_tables.hpp -- DoF numbering, constraints and level flags formed on the device from the forest alone
// (gmg_build_mesh_tables).
//
// Reference: dof_handler.distribute_dofs + distribute_mg_dofs, DoFTools::make_hanging_node_constraints,
// VectorTools::interpolate_boundary_values and MGConstrainedDoFs::initialize + make_zero_boundary_constraints
// (src/step-50.cc:661-706); the host restates them as the sequential loops of LaplaceProblem::distribute_dofs
// and make_constraints (csrc/host/laplace_problem.cc), and the kernels here restate those loops order-free:
//   first-touch numbering   a vertex's DoF is the number of distinct vertices whose first slot lies before its own first
//                           slot: the vertices go into an open-addressing table (64-bit compare-and-swap on the key), every
//                           slot lowers the vertex's first slot with an integer minimum, the slots that ARE a first slot are
//                           flagged and ranked by a scan;
//   neighbours              (level, coordinates) -> cell through a table of the same kind, one level at a time;
//   hanging-node lines      "the first visit that reaches a vertex gives it its line": every visit lowers the vertex's first
//                           visiting ordinal with a 64-bit integer minimum, the visits that ARE a first visit are counted per
//                           cell, ranked by a scan and written by the thread of their cell.
// Minimum and insert-if-absent do not depend on the order the threads arrive in, so the arrays are the host's for any launch
// shape.  Every probe loop runs at most once round its table and reports a full table or a missing key through a flag word
// the host reads after the kernel; no thread waits for another.  Integer atomics and plain stores only, no LDS.
#pragma once
#include "gmg_device.hpp"
#include "gmg_transfer.hpp"

namespace gmg {

constexpr int kMtShift = 12;  // Forest::kMaxLevelShift: vertex keys address level <= 12 below the root lattice
constexpr int kMtThreads = 256;
constexpr int kMtErrFull = 1, kMtErrDuplicate = 2, kMtErrUnbalanced = 4;  // bits of the flag word

struct MtForest {
  const int32_t *coord;        // [n_cells][3], in units of the cell's level
  const int32_t *first_child;  // [n_cells]
  const uint8_t *level;        // [n_cells]
  int dim, nv, nf;
  int32_t n0[3];
  unsigned long long hi[3];  // n0[d] << kMtShift: the upper domain boundary on the finest addressable lattice
};

__device__ __forceinline__ unsigned long long mt_pack(unsigned long long x, unsigned long long y, unsigned long long z) { return x | (y << 21) | (z << 42); }

// Forest::vertex_key of vertex v (bit d set = upper side in direction d) of a cell
__device__ __forceinline__ unsigned long long mt_vertex_key(const MtForest &f, int64_t cell, int v) {
  const int s = kMtShift - (int)f.level[cell];
  const int32_t *c = f.coord + 3 * cell;
  return mt_pack((unsigned long long)(c[0] + (v & 1)) << s, (unsigned long long)(c[1] + ((v >> 1) & 1)) << s,
                 f.dim == 3 ? (unsigned long long)(c[2] + ((v >> 2) & 1)) << s : 0ull);
}

__device__ __forceinline__ bool mt_on_boundary(const MtForest &f, unsigned long long key) {
  unsigned long long v[3];
  tr_unpack(key, v);
  bool b = false;
  for (int d = 0; d < f.dim; ++d) b = b || v[d] == 0 || v[d] == f.hi[d];
  return b;
}

// position of key k in the table, inserted if absent; -1: the table is full.  (A key, once written, never changes: a plain
// read that finds k or another key is final, one that finds the slot free is settled by the compare-and-swap.)
__device__ __forceinline__ int64_t mt_insert(unsigned long long *keys, unsigned long long mask, unsigned long long k, bool *inserted) {
  unsigned long long h = tr_hash(k) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    unsigned long long q = keys[h];
    if (q == kTrEmpty) q = atomicCAS(&keys[h], kTrEmpty, k);
    if (q == kTrEmpty || q == k) {
      if (inserted) *inserted = q == kTrEmpty;
      return (int64_t)h;
    }
    h = (h + 1) & mask;
  }
  return -1;
}

// position of key k in a finished table, -1: absent
__device__ __forceinline__ int64_t mt_find(const unsigned long long *keys, unsigned long long mask, unsigned long long k) {
  unsigned long long h = tr_hash(k) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    const unsigned long long q = keys[h];
    if (q == k) return (int64_t)h;
    if (q == kTrEmpty) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

#define MT_FOR(i, n) for (int64_t i = (int64_t)blockIdx.x * kMtThreads + threadIdx.x; i < (n); i += (int64_t)gridDim.x * kMtThreads)

// ---- active cells: flag[c] = 1 for first_child < 0 (scanned into the cell's position among the active cells)
__global__ __launch_bounds__(kMtThreads) void mt_active_flag_kernel(const int32_t *first_child, int64_t n_cells, int32_t *flag) {
  MT_FOR(c, n_cells) flag[c] = first_child[c] < 0 ? 1 : 0;
}
__global__ __launch_bounds__(kMtThreads) void mt_active_list_kernel(MtForest f, int64_t n_cells, const int32_t *apos, int32_t *active_cell, uint8_t *cell_level) {
  MT_FOR(c, n_cells) {
    if (f.first_child[c] >= 0) continue;
    active_cell[apos[c]] = (int32_t)c;
    cell_level[apos[c]] = f.level[c];
  }
}

// ---- first-touch numbering of the slots s = i * nv + v of a cell list: cells[i], or begin + i where cells is null
// 1. every slot enters its vertex and lowers the vertex's first slot; hpos keeps the slot's table position
__global__ __launch_bounds__(kMtThreads) void mt_vertex_insert_kernel(MtForest f, const int32_t *cells, int64_t begin, int64_t n_slots, unsigned long long *keys,
                                                                     unsigned int *first, unsigned int *hpos, unsigned long long mask, int *err) {
  MT_FOR(s, n_slots) {
    const int64_t i = s >> f.dim, cell = cells ? (int64_t)cells[i] : begin + i;
    const int64_t h = mt_insert(keys, mask, mt_vertex_key(f, cell, (int)(s & (f.nv - 1))), nullptr);
    if (h < 0) { atomicOr(err, kMtErrFull); hpos[s] = 0u; continue; }
    atomicMin(&first[h], (unsigned int)s);
    hpos[s] = (unsigned int)h;
  }
}
// 2. the slots that are their vertex's first slot (scanned into the vertex's DoF)
__global__ __launch_bounds__(kMtThreads) void mt_first_flag_kernel(const unsigned int *first, const unsigned int *hpos, int64_t n_slots, int32_t *is_first) {
  MT_FOR(s, n_slots) is_first[s] = first[hpos[s]] == (unsigned int)s ? 1 : 0;
}
// 3. the cell table, the vertex of every DoF and (tdof non-null) the DoF of every table position
__global__ __launch_bounds__(kMtThreads) void mt_number_kernel(const unsigned long long *keys, const unsigned int *first, const unsigned int *hpos, const int32_t *rank,
                                                              int64_t n_slots, int32_t *cell_dofs, unsigned long long *vertex_of_dof, int32_t *tdof) {
  MT_FOR(s, n_slots) {
    const unsigned int h = hpos[s], fs = first[h];
    const int32_t dof = rank[fs];
    cell_dofs[s] = dof;
    if (fs == (unsigned int)s) {
      vertex_of_dof[dof] = keys[h];
      if (tdof) tdof[h] = dof;
    }
  }
}

// ---- level 0 as the full lattice in lexicographic order: DoF of a vertex = its lattice position
__global__ __launch_bounds__(kMtThreads) void mt_lattice_kernel(MtForest f, int64_t n_cells, int64_t n_dofs, int32_t *cell_dofs, unsigned long long *vertex_of_dof) {
  const int64_t nx = f.n0[0] + 1, ny = f.n0[1] + 1;
  MT_FOR(s, n_cells * f.nv) {
    const int32_t *c = f.coord + 3 * (s >> f.dim);
    const int v = (int)(s & (f.nv - 1));
    cell_dofs[s] = (int32_t)((c[0] + (v & 1)) + nx * ((c[1] + ((v >> 1) & 1)) + ny * (f.dim == 3 ? c[2] + ((v >> 2) & 1) : 0)));
  }
  MT_FOR(i, n_dofs) {
    const unsigned long long x = (unsigned long long)(i % nx), y = (unsigned long long)((i / nx) % ny), z = (unsigned long long)(i / (nx * ny));
    vertex_of_dof[i] = mt_pack(x << kMtShift, y << kMtShift, z << kMtShift);
  }
}

// ---- one level's cells by coordinates; a cell met twice raises kMtErrDuplicate
__global__ __launch_bounds__(kMtThreads) void mt_cell_insert_kernel(MtForest f, int64_t begin, int64_t n_cells, unsigned long long *keys, int32_t *index,
                                                                   unsigned long long mask, int *err) {
  MT_FOR(c, n_cells) {
    const int32_t *x = f.coord + 3 * (begin + c);
    bool inserted = false;
    const int64_t h = mt_insert(keys, mask, mt_pack((unsigned long long)x[0], (unsigned long long)x[1], (unsigned long long)x[2]), &inserted);
    if (h < 0) { atomicOr(err, kMtErrFull); continue; }
    if (!inserted) { atomicOr(err, kMtErrDuplicate); continue; }
    index[h] = (int32_t)c;
  }
}

// ---- the faces (cell c, f = 2 d + side) of one level: a face of an ACTIVE cell whose same-level neighbour exists and is
// refined carries hanging nodes (face_hangs, indexed by the cell's active position); on level >= 1 a face inside the domain
// without a cell of the level behind it puts its vertices on the refinement edge (edge[level DoF] = 1; equal plain stores)
__global__ __launch_bounds__(kMtThreads) void mt_level_face_kernel(MtForest f, int level, int64_t begin, int64_t n_cells, const unsigned long long *keys,
                                                                  const int32_t *index, unsigned long long mask, const int32_t *apos, const int32_t *level_cell_dofs,
                                                                  uint8_t *face_hangs, uint8_t *edge) {
  MT_FOR(i, n_cells * f.nf) {
    const int64_t c = i / f.nf, cell = begin + c;
    const int face = (int)(i % f.nf), d = face >> 1, side = face & 1;
    int32_t nb[3] = {f.coord[3 * cell], f.coord[3 * cell + 1], f.coord[3 * cell + 2]};
    nb[d] += side ? 1 : -1;
    const bool inside = nb[d] >= 0 && (int64_t)nb[d] < ((int64_t)f.n0[d] << level);
    int64_t N = -1;
    if (inside) {
      const int64_t h = mt_find(keys, mask, mt_pack((unsigned long long)nb[0], (unsigned long long)nb[1], (unsigned long long)nb[2]));
      if (h >= 0) N = index[h];
    }
    if (f.first_child[cell] < 0 && N >= 0 && f.first_child[begin + N] >= 0) face_hangs[(int64_t)apos[cell] * f.nf + face] = 1;
    if (level >= 1 && inside && N < 0)
      for (int v = 0; v < f.nv; ++v)
        if (((v >> d) & 1) == side) edge[level_cell_dofs[c * f.nv + v]] = 1;
  }
}
__global__ __launch_bounds__(kMtThreads) void mt_level_flags_kernel(MtForest f, const unsigned long long *vertex_of_dof, const uint8_t *edge, int64_t n_dofs, uint8_t *dof_flags) {
  MT_FOR(i, n_dofs) dof_flags[i] = (uint8_t)((mt_on_boundary(f, vertex_of_dof[i]) ? 1 : 0) | (edge[i] ? 2 : 0));
}

// ---- hanging-node lines.  Visit (a, face, j) has the ordinal (a * nf + face) * 5 + j; j = 0 .. 4 in 3D: the face centre, then
// the mid-points of the edges (0,1), (2,3), (0,2), (1,3) of the face's corners (the cell's vertices on the face, ascending:
// corner k has bit 0 of k in the lower in-face direction t1 and bit 1 in the upper one t2); in 2D j = 0: the mid-point of the
// edge.  Everything below is arithmetic on (d, side, j): no table is indexed by a run-time value.
__device__ __forceinline__ int mt_t1(int d) { return d == 0 ? 1 : 0; }
__device__ __forceinline__ int mt_t2(int d) { return d == 2 ? 1 : 2; }
// the hanging vertex of a visit: the host's sum of the corners' coordinates over their number, here in half cells of the
// cell's level (a face qualifies only next to a refined cell, so the level is at most 11 and the halves are whole numbers)
__device__ __forceinline__ unsigned long long mt_visit_key(const MtForest &f, int64_t cell, int face, int j) {
  const int d = face >> 1, side = face & 1, t1 = mt_t1(d);
  const int a1 = f.dim == 2 ? 1 : j <= 2 ? 1 : j == 3 ? 0 : 2;  // half cells along t1 / t2: (1,1), (1,0), (1,2), (0,1), (2,1)
  const int a2 = f.dim == 2 ? 0 : j == 0 ? 1 : j == 1 ? 0 : j == 2 ? 2 : 1;
  const int s = kMtShift - 1 - (int)f.level[cell];
  const int32_t *c = f.coord + 3 * cell;
  const int o0 = d == 0 ? 2 * side : t1 == 0 ? a1 : a2, o1 = d == 1 ? 2 * side : t1 == 1 ? a1 : a2, o2 = d == 2 ? 2 * side : a2;
  return mt_pack((unsigned long long)(2 * c[0] + o0) << s, (unsigned long long)(2 * c[1] + o1) << s,
                 f.dim == 3 ? (unsigned long long)(2 * c[2] + o2) << s : 0ull);
}
// its masters: m corners of the face (4 for the centre, else 2), as vertices of the cell
__device__ __forceinline__ int mt_visit_masters(int dim, int j) { return dim == 3 && j == 0 ? 4 : 2; }
__device__ __forceinline__ int mt_visit_vertex(int dim, int face, int j, int q) {
  const int d = face >> 1, side = face & 1;
  const int e = dim == 3 ? j - 1 : 0;  // the edge: (0,1), (2,3), (0,2), (1,3)
  const int k = dim == 3 && j == 0 ? q : q == 0 ? (e == 0 ? 0 : e == 1 ? 2 : e == 2 ? 0 : 1) : (e == 0 ? 1 : e == 1 ? 3 : e == 2 ? 2 : 3);
  return (side << d) | ((k & 1) << mt_t1(d)) | (dim == 3 ? (k >> 1) << mt_t2(d) : 0);
}

struct MtHang {
  const int32_t *active_cell;  // [n_active]: index among all cells
  const uint8_t *face_hangs;   // [n_active * nf]
  const int32_t *cell_dofs;    // [n_active * nv]
  const unsigned long long *keys;  // the active mesh's vertex table and the DoF of every position
  const int32_t *tdof;
  unsigned long long mask;
  unsigned long long *visit;  // [n_dofs]: the first visiting ordinal of a vertex (all ones: none)
  int64_t n_active;
  int *err;
  // the count pass writes, the fill pass reads (scanned in between)
  int32_t *line_base, *entry_base;  // [n_active + 1]
  int32_t *constraint_of_dof, *line_dof, *line_ptr, *line_master;
  double *line_weight;
};

// 1. one thread per face: every visit lowers its vertex's first ordinal; a hanging vertex without a DoF: not 2:1 balanced
__global__ __launch_bounds__(kMtThreads) void mt_hang_visit_kernel(MtForest f, MtHang a) {
  MT_FOR(i, a.n_active * f.nf) {
    if (!a.face_hangs[i]) continue;
    const int64_t cell = a.active_cell[i / f.nf];
    const int face = (int)(i % f.nf), nj = f.dim == 3 ? 5 : 1;
    for (int j = 0; j < nj; ++j) {
      const int64_t h = mt_find(a.keys, a.mask, mt_visit_key(f, cell, face, j));
      if (h < 0) { atomicOr(a.err, kMtErrUnbalanced); continue; }
      atomicMin(&a.visit[a.tdof[h]], (unsigned long long)i * 5ull + (unsigned long long)j);
    }
  }
}
// 2. one thread per active cell walks its visits in order: FILL = false counts the lines it creates and their entries,
// FILL = true writes them at the scanned offsets
template <bool FILL>
__global__ __launch_bounds__(kMtThreads) void mt_hang_lines_kernel(MtForest f, MtHang a) {
  MT_FOR(c, a.n_active) {
    int32_t nl = 0, ne = 0;
    for (int face = 0; face < f.nf; ++face) {
      const int64_t i = c * f.nf + face;
      if (!a.face_hangs[i]) continue;
      const int64_t cell = a.active_cell[c];
      const int nj = f.dim == 3 ? 5 : 1;
      for (int j = 0; j < nj; ++j) {
        const int m = mt_visit_masters(f.dim, j);
        const int64_t h = mt_find(a.keys, a.mask, mt_visit_key(f, cell, face, j));
        if (h < 0) continue;
        const int32_t dof = a.tdof[h];
        if (a.visit[dof] != (unsigned long long)i * 5ull + (unsigned long long)j) continue;
        if constexpr (FILL) {
          const int32_t line = a.line_base[c] + nl, p = a.entry_base[c] + ne;
          a.constraint_of_dof[dof] = line;
          a.line_dof[line] = dof;
          a.line_ptr[line] = p;
          for (int q = 0; q < m; ++q) {
            a.line_master[p + q] = a.cell_dofs[c * f.nv + mt_visit_vertex(f.dim, face, j, q)];
            a.line_weight[p + q] = 1.0 / (double)m;
          }
        }
        ++nl;
        ne += m;
      }
    }
    if constexpr (!FILL) { a.line_base[c] = nl; a.entry_base[c] = ne; }
  }
}

// ---- Dirichlet lines: every boundary DoF without a hanging line, ascending, behind the hanging lines; no entries
__global__ __launch_bounds__(kMtThreads) void mt_dirichlet_flag_kernel(MtForest f, const unsigned long long *vertex_of_dof, const unsigned long long *visit, int64_t n_dofs,
                                                                      int32_t *is_line) {
  MT_FOR(i, n_dofs) is_line[i] = mt_on_boundary(f, vertex_of_dof[i]) && visit[i] == kTrEmpty ? 1 : 0;
}
__global__ __launch_bounds__(kMtThreads) void mt_dirichlet_lines_kernel(MtForest f, const unsigned long long *vertex_of_dof, const unsigned long long *visit,
                                                                       const int32_t *rank, int64_t n_dofs, int32_t n_hanging, int32_t n_lines, int32_t n_entries,
                                                                       int32_t *constraint_of_dof, int32_t *line_dof, int32_t *line_ptr) {
  MT_FOR(i, n_dofs) {
    if (!(mt_on_boundary(f, vertex_of_dof[i]) && visit[i] == kTrEmpty)) continue;
    const int32_t line = n_hanging + rank[i];
    constraint_of_dof[i] = line;
    line_dof[line] = (int32_t)i;
    line_ptr[line] = n_entries;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) line_ptr[n_lines] = n_entries;
}

#undef MT_FOR

}  // namespace gmg
