// gmg_rhs_cells.hpp -- the right-hand side of LaplaceProblem::assemble_system formed from the cell tables alone
// (gmg_assemble_rhs), and constraints.distribute on the same constraint tables
// (gmg_distribute_constraints).  No host plan: the inputs are what gmg_assemble_system_matrix takes (gmg_assemble.hpp: cell_dofs
// [n_cells][nv], cell_level, K [16][nv][nv], constraint_of_dof, the lines in CSR form) plus line_inhomogeneity [n_lines], the
// quadrature's tables shape [nq][nv], weight [nq], jxw_of_level [16] and the integrand rho [n_cells][nq].
//
// Definition (the header's, restated).  fp64, no contraction into fused multiply-adds (the library is built with
// -ffp-contract=off), no floating-point atomics: every output is one sequential sum formed by one lane, so the bits depend
// neither on the grid nor on the order in which slots or DoFs are visited.  l = cell_level[c], d_i = cell_dofs[c][i], line(i)
// the line of d_i or none.
//   1. per slot s = c nv + i:   F[s] = +0.0;  for q ascending   F[s] += ((shape[q][i] * rho[c][q]) * weight[q]) * jxw_of_level[l]
//      (rhs_cell_kernel of gmg_device.hpp: the operand order of gmg_rhs_assemble)
//   2. then, for j ascending over the vertices of c whose line has line_inhomogeneity != 0.0:
//        F[s] = F[s] - K[l][i][j] * line_inhomogeneity[line(j)]           -- for every i, constrained or not
//   3. per DoF d:   rhs[d] = +0.0;  over the slots s = (c, i) in ascending order:
//        d_i unconstrained and d_i == d:   rhs[d] += F[s]
//        d_i has a line:                   for its entries e in stored order with line_master[e] == d:   rhs[d] += line_weight[e] * F[s]
//      a line without entries (Dirichlet) passes nothing on; a DoF that receives nothing holds +0.0.
//
// Kernels.  Step 1 is rhs_cell_kernel, one thread per cell.  The rows a slot contributes to -- its DoF and the distinct masters
// of its line -- are the incidence lists of the matrix assembly (asm_incidence_kernel, asm_sort_incidence_kernel), so every
// row has its slots in ascending order, which is the host loop's order of additions.  (2) rhs_cells_dirichlet_kernel, one
// thread per slot: K and the line inhomogeneities come through the cache, the loop over j is the same for the nv slots of a
// cell.  (3) rhs_cells_gather_kernel, one thread per DoF: it walks the row's sorted slots, however many (a vertex shared by a
// fan of cells has more than a hundred), and for a constrained slot the entries of the line.  F is nv doubles per cell and
// read once per contributing row: no LDS staging.
//
// gmg_distribute_constraints: for every constrained d with line l,   v = line_inhomogeneity[l];  for the entries e in stored
// order   v += line_weight[e] * u[line_master[e]];   u[d] = v   (LaplaceProblem::distribute_constraints).  One thread per
// constrained DoF, in place: the host checks that no master is itself constrained, so no thread reads what another writes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gmg {

struct RhsCellsArgs {
  int nv, lg_nv;
  int64_t n_dofs, n_slots;
  const int32_t *cell_dofs;   // [n_slots]
  const uint8_t *cell_level;  // [n_cells]
  const double *K;            // [16 * nv * nv]; may be null when no line_inhomogeneity != 0.0 (step 2 is then not launched)
  const int32_t *cons;        // [n_dofs]
  const int32_t *line_ptr;    // [n_lines + 1]
  const int32_t *line_master;
  const double *line_weight;
  const double *line_inhom;   // [n_lines]
  const int32_t *inc_ptr;     // [n_dofs + 1]: the slots of every row
  const int32_t *inc_slot;    // ascending within a row
  double *F;                  // [n_slots]
  double *rhs;                // [n_dofs]
};

// step 2: the inhomogeneous Dirichlet terms of slot (c, i), j ascending
__global__ __launch_bounds__(256) void rhs_cells_dirichlet_kernel(RhsCellsArgs a) {
  const int nv = a.nv;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.n_slots; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = s >> a.lg_nv;
    const int i = (int)(s & (nv - 1));
    const int32_t *dofs = a.cell_dofs + c * nv;
    const double *Ki = a.K + ((int64_t)a.cell_level[c] * nv + i) * nv;
    double f = a.F[s];
    for (int j = 0; j < nv; ++j) {
      const int32_t l = a.cons[dofs[j]];
      if (l < 0) continue;
      const double g = a.line_inhom[l];
      if (g != 0.0) f = f - Ki[j] * g;
    }
    a.F[s] = f;
  }
}

// step 3: one sequential sum per DoF over its slots in ascending order and, for a constrained slot, the line's entries
__global__ __launch_bounds__(256) void rhs_cells_gather_kernel(RhsCellsArgs a) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < a.n_dofs; d += (int64_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    const int32_t p1 = a.inc_ptr[d + 1];
    for (int32_t p = a.inc_ptr[d]; p < p1; ++p) {
      const int32_t s = a.inc_slot[p];
      const int32_t di = a.cell_dofs[s];
      const int32_t l = a.cons[di];
      const double f = a.F[s];
      if (l < 0) {
        if (di == d) acc += f;
        continue;
      }
      const int32_t e1 = a.line_ptr[l + 1];
      for (int32_t e = a.line_ptr[l]; e < e1; ++e)
        if (a.line_master[e] == d) acc += a.line_weight[e] * f;
    }
    a.rhs[d] = acc;
  }
}

// constraints.distribute in place: every constrained entry from its line (no master is constrained: checked on the host)
__global__ __launch_bounds__(256) void distribute_constraints_kernel(int64_t n_dofs, const int32_t *cons, const int32_t *line_ptr,
                                                                     const int32_t *line_master, const double *line_weight,
                                                                     const double *line_inhom, double *u) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_dofs; d += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = cons[d];
    if (l < 0) continue;
    double v = line_inhom[l];
    const int32_t e1 = line_ptr[l + 1];
    for (int32_t e = line_ptr[l]; e < e1; ++e) v += line_weight[e] * u[line_master[e]];
    u[d] = v;
  }
}

}  // namespace gmg
