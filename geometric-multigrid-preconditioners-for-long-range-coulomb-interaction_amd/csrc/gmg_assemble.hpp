// gmg_assemble.hpp -- the active-mesh system matrix formed on the device (gmg_assemble_system_matrix):
// the sparsity pattern and the values of LaplaceProblem::assemble_system (csrc/host/laplace_problem.cc) from the cells' DoF
// tables, one cell matrix per level and the constraint lines, with the same bits as the host's sequential loop.
//
// Inputs.  cell_dofs [n_cells][nv] (nv = 2^dim, vertex a = bx + 2 by + 4 bz), cell_level [n_cells] (< 16),
// K [16][nv][nv] row-major (the cell matrix as the host scales it per level), constraint_of_dof [n_dofs] (-1 or a line),
// and the lines in CSR form: line l has the entries e in [line_ptr[l], line_ptr[l + 1]) with master line_master[e] and
// weight line_weight[e].  A Dirichlet line has no entries.
//
// Pattern.  A cell's coupling list is its DoFs plus the masters of its constrained DoFs.  Row r stores the sorted union of
// the coupling lists of all cells whose list contains r.  Stored zeros are kept: a constrained row carries all of its
// couplings as zeros (and its diagonal, below).
//
// Values.  Every stored entry starts at +0.0 and receives, in exactly this order -- cells ascending, then i ascending, then
// j ascending, then the entries ri of line(i), then the entries rj of line(j) --
//   both unconstrained          (dofs[i], dofs[j])       += K[i][j]
//   i constrained               (master(ri), dofs[j])    += w(ri) * K[i][j]
//   j constrained               (dofs[i], master(rj))    += w(rj) * K[i][j]
//   both constrained            (master(ri), master(rj)) += (w(ri) * w(rj)) * K[i][j]
// a pair is skipped when either side is a line without entries; and for every constrained i, before its j loop,
//   (dofs[i], dofs[i]) += |K[i][i]|.
// fp64, no contraction into fused multiply-adds (the library is built with -ffp-contract=off), no floating-point atomics:
// every stored entry is one sequential sum formed by one lane, so the bits depend neither on the grid nor on the order in
// which the rows are visited.
//
// Kernels.  (1) asm_incidence_kernel, one thread per (cell, vertex) slot: the rows that slot contributes to -- its DoF and
// the distinct masters of its line -- counted, scanned (tr_scan_kernel) and filled through integer cursors; (2)
// asm_sort_incidence_kernel, one thread per row: the row's slots ascending, which is the host's (cell, i) order; (3)
// asm_row_kernel, one wavefront per row, twice: the union of the coupling lists of the row's cells is collected in LDS
// (each batch of up to 64 candidates is compared against the set and against itself, the new ones appended by ballot),
// counted, and after the scan of the counts ranked into ascending order and written; then one lane per stored column walks
// the row's slots in order and adds what the host loop adds to (row, column).  The lane that owns the diagonal also writes
// 1 / a_rr, the Jacobi diagonal.  A row may have at most kAsmMaxRow distinct columns (27 away from refinement edges).
// (4) asm_norm_sums_kernel, one thread per row: sum |a| over the row in stored order, and over the column of the same
// index in ascending row order -- the pattern is structurally symmetric, so column c's rows are row c's columns, found in
// each of those rows by bisection (a gather: no atomics, no transpose).
//
// ---- The multigrid level matrices A_l and the interface ("edge") matrices I_l (gmg_assemble_level_matrix, DESIGN.md section
// 17): LaplaceProblem::assemble_level from one level's cell table, with the same machinery (the kernels' LEVEL form).
//
// Inputs.  cell_dofs [n_cells][nv] (all cells of the level, vertex a = bx + 2 by + 4 bz), ONE cell matrix K [nv][nv] row-major
// as the host scales it for the level (Kc[i][j] * pow(h_l, dim - 2)), dof_flags [n_dofs]: bit 0 = the DoF is on the boundary
// (level_boundary), bit 1 = it is on the refinement edge (level_refinement_edge).  There are no constraint lines.
//
// A_l pattern.  Row r stores the sorted union of the DoFs of all cells that contain r.  Stored zeros are kept; a flagged row
// keeps its whole pattern.
// A_l values.  Every entry starts at +0.0; cells ascending, then i ascending: if dof_flags[dofs[i]] != 0,
//   (dofs[i], dofs[i]) += |K[i][i]|   and nothing else from this i;
// otherwise, for j ascending with dof_flags[dofs[j]] == 0,   (dofs[i], dofs[j]) += K[i][j].
// Jacobi diagonal and Chebyshev bound (setup_diag).  invd[r] = 1 / a_rr; cheb_lmax = max_r (sum_k |a_rk| in stored order) /
// |a_rr|: asm_gershgorin_kernel, one sequential sum per row, the maximum through an integer atomicMax on the bits of the
// non-negative ratios (order-independent; a NaN ratio -- an empty row -- is skipped as std::max skips it).
// I_l pattern.  The pairs (dofs[i], dofs[j]) of any cell with dof_flags[dofs[i]] == 2 (on the edge, not on the boundary) and
// dof_flags[dofs[j]] == 0: row r of A_l filtered by the column flags, for the rows r with flag 2.
// I_l values.  The sum of its cells' K[i][j] in ascending cell order (then i, then j), starting from the first contribution;
// entries whose sum == 0.0 are then dropped, as gmg_set_edge_matrix drops them.  The FILL pass of asm_row_kernel forms them
// beside A_l's values (one lane per stored column) and counts the survivors; asm_edge_fill_kernel compacts them.
// I_l^T.  Row j lists the entries (r, j) of I_l in ascending r: the rows that may hold column j are the columns of row j of A_l
// (structural symmetry), and j is found in each of those rows of I_l by bisection (asm_edge_transpose_kernel, count and
// fill) -- what the stable host transpose of gmg_set_edge_matrix gives, without atomics.
//
// ---- The coefficient form of both assemblies (gmg_assemble_system_matrix_coef, gmg_assemble_level_matrix_coef, DESIGN.md
// section 18): a coefficient that varies in space.  Inputs instead of K: nq (1 .. kAsmMaxNq), cell_coef [n_cells][nq] (the
// coefficient at the quadrature points of every cell), G [nq][nv][nv] (the reference-cell products sum_d d_d phi_i d_d phi_j
// at each point; the caller forms them), qw [nq], and scale [16] by cell level (system matrix) or one scale (a level).  The
// cell matrix of cell c is
//   K_c[i][j] = +0.0;   for q ascending:   K_c[i][j] += ((cell_coef[c][q] * G[q][i][j]) * qw[q]) * scale
// (fp64, no contraction), and everything above holds word for word with K_c in place of K[level] / K.  No K_c is stored: a
// lane forms the entry it needs where it consumes it (asm_cell_k), selected by the template flag COEF of the FILL pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gmg {

constexpr int kAsmMaxNq = 64;    // quadrature points per cell the coefficient form takes
constexpr int kAsmMaxRow = 512;  // distinct columns of a row the wavefront's LDS set holds (+ one batch of 64 candidates)

struct AsmArgs {
  int nv, lg_nv;              // vertices per cell, log2
  int max_line;               // longest constraint line (entries)
  int64_t n_dofs, n_slots;    // n_slots = n_cells * nv
  const int32_t *cell_dofs;   // [n_slots]
  const uint8_t *cell_level;  // [n_cells]
  const double *K;            // [16 * nv * nv]
  const int32_t *cons;        // [n_dofs]
  const int32_t *line_ptr;    // [n_lines + 1]
  const int32_t *line_master;
  const double *line_weight;
  const uint8_t *flags;       // LEVEL form: [n_dofs], bit 0 boundary, bit 1 refinement edge (cell_level, cons and the lines are unused, K is one matrix)
  // COEF form (K is unused): the cell matrices are formed from coefficient values where they are consumed (asm_cell_k)
  int nq;                     // quadrature points per cell (1 .. kAsmMaxNq)
  const double *cell_coef;    // [n_cells * nq]
  const double *G;            // [nq * nv * nv]
  const double *qw;           // [nq]
  const double *scale;        // [16] by cell level; LEVEL form: [1]
  int32_t *inc_ptr;   // [n_dofs + 1]: slots of every row (counts before the scan)
  int32_t *inc_pos;   // [n_dofs]: fill cursors
  int32_t *inc_slot;  // [inc_ptr[n_dofs]]
  int32_t *rowptr;    // [n_dofs + 1] (counts before the scan)
  int32_t *col;
  double *val;
  double *invd;                    // [n_dofs]: 1 / a_rr (1 / +0.0 where the row stores no diagonal)
  unsigned long long *total;       // sum of the row lengths in 64 bits (the scan is 32-bit)
  int *overflow;                   // a row with more than kAsmMaxRow columns was met
  double *edge_val;                // LEVEL form: beside val, the interface-matrix sum of every stored entry (0.0: not an entry of I_l); rows with flag 2 only
  int32_t *edge_cnt;               // LEVEL form: [n_dofs + 1]: entries of I_l per row (sums != 0.0)
};

// the rows slot s contributes to: its DoF, and the masters of the DoF's line that are neither the DoF nor an earlier master
// (LEVEL: its DoF)
template <bool FILL, bool LEVEL = false>
__global__ __launch_bounds__(256) void asm_incidence_kernel(AsmArgs a) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.n_slots; s += (int64_t)gridDim.x * blockDim.x) {
    const int32_t d = a.cell_dofs[s];
    auto emit = [&](int32_t x) {
      if constexpr (FILL) a.inc_slot[a.inc_ptr[x] + atomicAdd(&a.inc_pos[x], 1)] = (int32_t)s;
      else atomicAdd(&a.inc_ptr[x], 1);
    };
    emit(d);
    if constexpr (LEVEL) continue;
    const int32_t l = a.cons[d];
    if (l < 0) continue;
    const int32_t e0 = a.line_ptr[l], e1 = a.line_ptr[l + 1];
    for (int32_t e = e0; e < e1; ++e) {
      const int32_t m = a.line_master[e];
      bool seen = m == d;
      for (int32_t f = e0; f < e && !seen; ++f) seen = a.line_master[f] == m;
      if (!seen) emit(m);
    }
  }
}

// every row's slots ascending (insertion sort: a row has 8 slots away from refinement edges)
__global__ __launch_bounds__(256) void asm_sort_incidence_kernel(AsmArgs a) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_dofs; r += (int64_t)gridDim.x * blockDim.x) {
    int32_t *p = a.inc_slot + a.inc_ptr[r];
    const int n = a.inc_ptr[r + 1] - a.inc_ptr[r];
    for (int i = 1; i < n; ++i) {
      const int32_t v = p[i];
      int j = i - 1;
      for (; j >= 0 && p[j] > v; --j) p[j + 1] = p[j];
      p[j + 1] = v;
    }
  }
}

// COEF form: entry (i, j) of the cell matrix of `cell`, one sequential sum over the quadrature points in ascending order.  qw
// and the scale of a level are uniform over the wavefront; G and the cell's coefficients come through the cache.
template <bool LEVEL>
__device__ __forceinline__ double asm_cell_k(const AsmArgs &a, int32_t cell, int i, int j) {
  const int nv = a.nv;
  const double *cc = a.cell_coef + (int64_t)cell * a.nq;
  const double *g = a.G + i * nv + j;
  double s;
  if constexpr (LEVEL) s = a.scale[0];
  else s = a.scale[a.cell_level[cell]];
  double k = 0.0;
  for (int q = 0; q < a.nq; ++q) k += ((cc[q] * g[q * nv * nv]) * a.qw[q]) * s;
  return k;
}

// what the host loop adds to (r, c) for slot (cell, i), in its order of j, ri, rj
template <bool COEF>
__device__ __forceinline__ void asm_add_slot(const AsmArgs &a, int32_t slot, int32_t r, int32_t c, double &acc) {
  const int nv = a.nv;
  const int32_t cell = slot >> a.lg_nv;
  const int i = slot & (nv - 1);
  const int32_t *cd = a.cell_dofs + (int64_t)cell * nv;
  const double *K = COEF ? nullptr : a.K + (int)a.cell_level[cell] * nv * nv;
  const int32_t di = cd[i], li = a.cons[di];
  int32_t i0 = 0, i1 = 0;
  if (li >= 0) {
    i0 = a.line_ptr[li]; i1 = a.line_ptr[li + 1];
    if (di == r && c == r) {
      if constexpr (COEF) acc += fabs(asm_cell_k<false>(a, cell, i, i));
      else acc += fabs(K[i * nv + i]);
    }
  }
  for (int j = 0; j < nv; ++j) {
    const int32_t dj = cd[j], lj = a.cons[dj];
    // (COEF: K_c[i][j] is formed once, by the first term of this j that needs it)
    double kij = 0.0;
    bool have = !COEF;
    if constexpr (!COEF) kij = K[i * nv + j];
    auto k = [&]() {
      if constexpr (COEF) {
        if (!have) { kij = asm_cell_k<false>(a, cell, i, j); have = true; }
      }
      return kij;
    };
    if (li < 0 && lj < 0) {
      if (di == r && dj == c) acc += k();
      continue;
    }
    if (li >= 0 && i0 == i1) continue;
    int32_t j0 = 0, j1 = 0;
    if (lj >= 0) {
      j0 = a.line_ptr[lj]; j1 = a.line_ptr[lj + 1];
      if (j0 == j1) continue;
    }
    if (li >= 0 && lj >= 0) {
      for (int32_t ei = i0; ei < i1; ++ei) {
        if (a.line_master[ei] != r) continue;
        for (int32_t ej = j0; ej < j1; ++ej)
          if (a.line_master[ej] == c) acc += (a.line_weight[ei] * a.line_weight[ej]) * k();
      }
    } else if (li >= 0) {
      if (dj != c) continue;
      for (int32_t ei = i0; ei < i1; ++ei)
        if (a.line_master[ei] == r) acc += a.line_weight[ei] * k();
    } else {
      if (di != r) continue;
      for (int32_t ej = j0; ej < j1; ++ej)
        if (a.line_master[ej] == c) acc += a.line_weight[ej] * k();
    }
  }
}

// LEVEL form: what assemble_level adds to (r, c) of A_l for slot (cell, i) -- dofs[i] == r -- in its order of j
template <bool COEF>
__device__ __forceinline__ void asm_add_level_slot(const AsmArgs &a, int32_t slot, int32_t r, int32_t c, double &acc) {
  const int nv = a.nv;
  const int i = slot & (nv - 1);
  const int32_t cell = slot >> a.lg_nv;
  const int32_t *cd = a.cell_dofs + (int64_t)cell * nv;
  if (a.flags[r] != 0) {
    if (c == r) {
      if constexpr (COEF) acc += fabs(asm_cell_k<true>(a, cell, i, i));
      else acc += fabs(a.K[i * nv + i]);
    }
    return;
  }
  for (int j = 0; j < nv; ++j)
    if (cd[j] == c && a.flags[c] == 0) {
      if constexpr (COEF) acc += asm_cell_k<true>(a, cell, i, j);
      else acc += a.K[i * nv + j];
    }
}

// LEVEL form: what slot (cell, i) contributes to (r, c) of I_l (flag 2 on r, flag 0 on c): the sum starts from its first term
template <bool COEF>
__device__ __forceinline__ void asm_add_edge_slot(const AsmArgs &a, int32_t slot, int32_t c, double &acc, bool &any) {
  const int nv = a.nv;
  const int i = slot & (nv - 1);
  const int32_t cell = slot >> a.lg_nv;
  const int32_t *cd = a.cell_dofs + (int64_t)cell * nv;
  for (int j = 0; j < nv; ++j)
    if (cd[j] == c) {
      double v;
      if constexpr (COEF) v = asm_cell_k<true>(a, cell, i, j);
      else v = a.K[i * nv + j];
      acc = any ? acc + v : v;
      any = true;
    }
}

// One wavefront per row (workgroups of 64).  FILL = false: rowptr[r] = number of distinct columns.  FILL = true (rowptr
// scanned): the columns in ascending order, the values, the Jacobi diagonal.  LEVEL: a cell's coupling list is its DoFs, the
// values are assemble_level's, and the rows with flag 2 also form their interface-matrix sums (edge_val) and count them.
// COEF (FILL pass only; the pattern needs no values): the cell matrices come from asm_cell_k instead of the table K.
template <bool FILL, bool LEVEL = false, bool COEF = false>
__global__ __launch_bounds__(64) void asm_row_kernel(AsmArgs a) {
  static_assert(FILL || !COEF, "the pattern pass reads no cell matrix");
  __shared__ int32_t set[kAsmMaxRow + 64];
  __shared__ int32_t sorted[FILL ? kAsmMaxRow : 1];
  const int lane = threadIdx.x;
  const int nv = a.nv;
  unsigned long long my_total = 0;
  for (int64_t r = blockIdx.x; r < a.n_dofs; r += gridDim.x) {
    const int32_t q0 = a.inc_ptr[r], q1 = a.inc_ptr[r + 1];
    int n = 0;
    bool over = false;
    int32_t prev_cell = -1;
    for (int32_t q = q0; q < q1 && !over; ++q) {
      const int32_t cell = a.inc_slot[q] >> a.lg_nv;
      if (cell == prev_cell) continue;  // (a row's slots are sorted: those of one cell are neighbours)
      prev_cell = cell;
      // the cell's coupling list, 8 candidates per vertex and round: the DoF itself, then its line's masters
      for (int base = 0; base <= a.max_line && !over; base += 8) {
        if (n > kAsmMaxRow) { over = true; break; }
        const int b = lane >> 3, k = base + (lane & 7);
        int32_t c = -1;
        if (b < nv) {
          const int32_t d = a.cell_dofs[(int64_t)cell * nv + b];
          if (k == 0) c = d;
          else if constexpr (!LEVEL) {
            const int32_t l = a.cons[d];
            if (l >= 0) {
              const int32_t e = a.line_ptr[l] + (k - 1);
              if (e < a.line_ptr[l + 1]) c = a.line_master[e];
            }
          }
        }
        set[n + lane] = c;
        __syncthreads();
        bool is_new = c >= 0;
        for (int m = 0; m < n + lane && is_new; ++m) is_new = set[m] != c;
        __syncthreads();
        const unsigned long long mask = __ballot(is_new);
        if (is_new) set[n + __popcll(mask & ((1ull << lane) - 1ull))] = c;
        n += __popcll(mask);
        __syncthreads();
      }
    }
    if (n > kAsmMaxRow) over = true;
    if (over) {
      if (lane == 0) *a.overflow = 1;
      n = 0;
    }
    if constexpr (!FILL) {
      if (lane == 0) { a.rowptr[r] = n; my_total += (unsigned long long)n; }
    } else {
      const int32_t k0 = a.rowptr[r];
      for (int k = lane; k < n; k += 64) {
        const int32_t v = set[k];
        int rank = 0;
        for (int m = 0; m < n; ++m) rank += set[m] < v ? 1 : 0;
        sorted[rank] = v;
        a.col[k0 + rank] = v;
      }
      __syncthreads();
      bool has_diag = false;
      int n_edge = 0;
      const bool edge_row = LEVEL && n > 0 && a.flags[r] == 2;
      for (int k = lane; k < n; k += 64) {
        const int32_t c = sorted[k];
        double acc = 0.0;
        for (int32_t q = q0; q < q1; ++q) {
          if constexpr (LEVEL) asm_add_level_slot<COEF>(a, a.inc_slot[q], (int32_t)r, c, acc);
          else asm_add_slot<COEF>(a, a.inc_slot[q], (int32_t)r, c, acc);
        }
        a.val[k0 + k] = acc;
        if (c == (int32_t)r) { a.invd[r] = 1.0 / acc; has_diag = true; }
        if (edge_row) {
          double e = 0.0;
          if (a.flags[c] == 0) {
            bool any = false;
            for (int32_t q = q0; q < q1; ++q) asm_add_edge_slot<COEF>(a, a.inc_slot[q], c, e, any);
          }
          a.edge_val[k0 + k] = e;
          n_edge += e != 0.0 ? 1 : 0;
        }
      }
      if (__ballot(has_diag) == 0ull && lane == 0) a.invd[r] = __builtin_inf();  // (setup_diag: a row without a diagonal)
      if constexpr (LEVEL) {
        for (int off = 32; off > 0; off >>= 1) n_edge += __shfl_down(n_edge, off);
        if (lane == 0) a.edge_cnt[r] = n_edge;
      }
      __syncthreads();
    }
  }
  if constexpr (!FILL) {
    if (lane == 0 && my_total) atomicAdd(a.total, my_total);
  }
}

// row_sum[r] = sum |a_rk| in stored order (CSRMatrix::linfty_norm before its max), col_sum[c] = sum |a_rc| over the rows r
// that store column c, r ascending (CSRMatrix::l1_norm before its max): column c's rows are row c's columns
__global__ __launch_bounds__(256) void asm_norm_sums_kernel(const int32_t *rowptr, const int32_t *col, const double *val, int64_t n,
                                                            double *row_sum, double *col_sum) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    double rs = 0.0, cs = 0.0;
    for (int32_t k = rowptr[c]; k < rowptr[c + 1]; ++k) {
      rs += fabs(val[k]);
      const int32_t r = col[k];
      int32_t lo = rowptr[r], hi = rowptr[r + 1];
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < (int32_t)c) lo = mid + 1;
        else hi = mid;
      }
      if (lo < rowptr[r + 1] && col[lo] == (int32_t)c) cs += fabs(val[lo]);
    }
    row_sum[c] = rs;
    col_sum[c] = cs;
  }
}

// cheb_lmax of setup_diag on the device's CSR: max over the rows of (sum |a_rk| in stored order) / |a_rr| -- a_rr = 0.0 where
// the row stores no diagonal -- as the bits of a non-negative double (*lmax_bits starts at 0)
__global__ __launch_bounds__(256) void asm_gershgorin_kernel(const int32_t *rowptr, const int32_t *col, const double *val, int64_t n,
                                                             unsigned long long *lmax_bits) {
  double m = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    double aii = 0.0, rs = 0.0;
    for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
      if (col[k] == (int32_t)r) aii = val[k];
      rs += fabs(val[k]);
    }
    const double ratio = rs / fabs(aii);
    if (m < ratio) m = ratio;  // (std::max(m, ratio): a NaN is skipped)
  }
  if (m > 0.0) atomicMax(lmax_bits, (unsigned long long)__double_as_longlong(m));
}

// I_l from the sums the row kernel left beside A_l's values: the entries != 0.0 of every row, in stored order (irp scanned)
__global__ __launch_bounds__(256) void asm_edge_fill_kernel(const int32_t *rowptr, const int32_t *col, const double *edge_val, int64_t n,
                                                            const int32_t *irp, int32_t *icol, double *ival) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int32_t p = irp[r];
    if (p == irp[r + 1]) continue;  // (edge_val is only written for the rows that have entries to count)
    for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k)
      if (edge_val[k] != 0.0) { icol[p] = col[k]; ival[p] = edge_val[k]; ++p; }
  }
}

// I_l^T, one thread per row j of it: the rows r of I_l that store column j, ascending, among the columns of row j of A_l.
// FILL = false: trp[j] = their number; FILL = true (trp scanned): the entries.
template <bool FILL>
__global__ __launch_bounds__(256) void asm_edge_transpose_kernel(const int32_t *rowptr, const int32_t *col, int64_t n, const int32_t *irp,
                                                                 const int32_t *icol, const double *ival, int32_t *trp, int32_t *tcol, double *tval) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    int32_t p = FILL ? trp[j] : 0;
    for (int32_t k = rowptr[j]; k < rowptr[j + 1]; ++k) {
      const int32_t r = col[k];
      int32_t lo = irp[r], hi = irp[r + 1];
      const int32_t end = hi;
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (icol[mid] < (int32_t)j) lo = mid + 1;
        else hi = mid;
      }
      if (lo < end && icol[lo] == (int32_t)j) {
        if constexpr (FILL) { tcol[p] = r; tval[p] = ival[lo]; }
        ++p;
      }
    }
    if constexpr (!FILL) trp[j] = p;
  }
}

}  // namespace gmg
