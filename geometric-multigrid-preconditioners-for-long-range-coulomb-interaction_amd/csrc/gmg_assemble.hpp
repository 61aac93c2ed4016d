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
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gmg {

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
  int32_t *inc_ptr;   // [n_dofs + 1]: slots of every row (counts before the scan)
  int32_t *inc_pos;   // [n_dofs]: fill cursors
  int32_t *inc_slot;  // [inc_ptr[n_dofs]]
  int32_t *rowptr;    // [n_dofs + 1] (counts before the scan)
  int32_t *col;
  double *val;
  double *invd;                    // [n_dofs]: 1 / a_rr (1 / +0.0 where the row stores no diagonal)
  unsigned long long *total;       // sum of the row lengths in 64 bits (the scan is 32-bit)
  int *overflow;                   // a row with more than kAsmMaxRow columns was met
};

// the rows slot s contributes to: its DoF, and the masters of the DoF's line that are neither the DoF nor an earlier master
template <bool FILL>
__global__ __launch_bounds__(256) void asm_incidence_kernel(AsmArgs a) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.n_slots; s += (int64_t)gridDim.x * blockDim.x) {
    const int32_t d = a.cell_dofs[s];
    auto emit = [&](int32_t x) {
      if constexpr (FILL) a.inc_slot[a.inc_ptr[x] + atomicAdd(&a.inc_pos[x], 1)] = (int32_t)s;
      else atomicAdd(&a.inc_ptr[x], 1);
    };
    emit(d);
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

// what the host loop adds to (r, c) for slot (cell, i), in its order of j, ri, rj
__device__ __forceinline__ void asm_add_slot(const AsmArgs &a, int32_t slot, int32_t r, int32_t c, double &acc) {
  const int nv = a.nv;
  const int32_t cell = slot >> a.lg_nv;
  const int i = slot & (nv - 1);
  const int32_t *cd = a.cell_dofs + (int64_t)cell * nv;
  const double *K = a.K + (int)a.cell_level[cell] * nv * nv;
  const int32_t di = cd[i], li = a.cons[di];
  int32_t i0 = 0, i1 = 0;
  if (li >= 0) {
    i0 = a.line_ptr[li]; i1 = a.line_ptr[li + 1];
    if (di == r && c == r) acc += fabs(K[i * nv + i]);
  }
  for (int j = 0; j < nv; ++j) {
    const int32_t dj = cd[j], lj = a.cons[dj];
    const double kij = K[i * nv + j];
    if (li < 0 && lj < 0) {
      if (di == r && dj == c) acc += kij;
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
          if (a.line_master[ej] == c) acc += (a.line_weight[ei] * a.line_weight[ej]) * kij;
      }
    } else if (li >= 0) {
      if (dj != c) continue;
      for (int32_t ei = i0; ei < i1; ++ei)
        if (a.line_master[ei] == r) acc += a.line_weight[ei] * kij;
    } else {
      if (di != r) continue;
      for (int32_t ej = j0; ej < j1; ++ej)
        if (a.line_master[ej] == c) acc += a.line_weight[ej] * kij;
    }
  }
}

// One wavefront per row (workgroups of 64).  FILL = false: rowptr[r] = number of distinct columns.  FILL = true (rowptr
// scanned): the columns in ascending order, the values, the Jacobi diagonal.
template <bool FILL>
__global__ __launch_bounds__(64) void asm_row_kernel(AsmArgs a) {
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
          else {
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
      for (int k = lane; k < n; k += 64) {
        const int32_t c = sorted[k];
        double acc = 0.0;
        for (int32_t q = q0; q < q1; ++q) asm_add_slot(a, a.inc_slot[q], (int32_t)r, c, acc);
        a.val[k0 + k] = acc;
        if (c == (int32_t)r) { a.invd[r] = 1.0 / acc; has_diag = true; }
      }
      if (__ballot(has_diag) == 0ull && lane == 0) a.invd[r] = __builtin_inf();  // (setup_diag: a row without a diagonal)
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

}  // namespace gmg
