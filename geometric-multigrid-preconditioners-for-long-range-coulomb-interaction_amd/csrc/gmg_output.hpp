// gmg_output.hpp -- the patches of the graphical output formed on the device (gmg_output_patches): what
// deal.II's DataOut::build_patches(0) hands to write_vtu for the reference's output_results (src/step-50.cc:1149-1308).  One
// patch per active cell, nv = 2^dim patch vertices per cell, nothing shared between cells: slot s = a nv + v, vertex
// v = bx + 2 by + 4 bz.
//
// Values (fp64, no contraction: both sides are built with -ffp-contract=off), k = vertex_of_dof[cell_dofs[s]]:
//   point[s][d]    = origin + (h0 / 4096.0) (double)((k >> 21 d) & 0x1fffff)   for d < dim, +0.0 above: the bits of
//                    Forest::vertex_coords, so the duplicated vertices of neighbouring cells coincide exactly;
//   solution[s]    = U[v] = u[cell_dofs[a nv + v]];
//   grad_phi[s][d] = -g,  g = (U[v | 1 << d] - U[v & ~(1 << d)]) / h_l,  h_l = h0 / (double)(1 << cell_level[a]): the
//                    estimator's g_c (gmg_estimate.hpp) at the vertex's own corner of the face, negated; +0.0 for d >= dim;
//   patch_field_j[s] = f_j[cell_dofs[s]]   for up to kMaxFields DoF vectors.
//
// Like gmg_exact.hpp this one text is compiled twice: into the gfx950 kernel of libgmgcoulomb.so and into the host mirror of
// csrc/host/output.inc.  Every value has one writer and no sum: nothing depends on the launch shape or on how a call is cut
// into launches.
//
// Kernel.  A bandwidth-bound gather, lane = slot; 64 and the workgroup size are multiples of nv, so the nv lanes of a cell
// are contiguous inside one wavefront and the neighbours' U come from a cross-lane exchange (lane ^ 1, 2, 4).  The exchange
// is executed by every lane of the workgroup in every turn of the grid-stride loop (the loop bound is rounded up to whole
// workgroups); loads and stores are under the guard on the CELL, which all lanes of a cell share.
#pragma once
#include "gmg_forces.hpp"  // GMG_FHD

namespace gmg_output {

constexpr int kMaxFields = 8;
constexpr int kMaxLevel = 13;  // 1 << level stays an int, and no forest of this library is deeper

// coordinate d of the vertex with key k; hf = h0 / 4096.0
GMG_FHD inline double coordinate(unsigned long long k, int d, double origin, double hf) {
  return origin + hf * (double)((k >> (21 * d)) & 0x1fffffull);
}

GMG_FHD inline double edge_length(double h0, int level) { return h0 / (double)(1 << level); }

// component d of -grad phi_h at a patch vertex whose bit d is `upper`: own = U[v], other = U[v ^ 1 << d]
GMG_FHD inline double field_component(double own, double other, bool upper, double h) {
  const double g = upper ? (own - other) / h : (other - own) / h;
  return -g;
}

#if defined(__HIPCC__)
constexpr int kPatchThreads = 256;

struct PatchArgs {
  int64_t c0, c1;             // the cells of this launch
  const int32_t *cell_dofs;   // [n_cells * nv]
  const uint8_t *cell_level;  // [n_cells]
  const unsigned long long *vertex_of_dof;
  const double *u;
  double origin, h0, hf;
  int n_fields;
  const double *dof_field[kMaxFields];  // [n_dofs] each
  // outputs of the launch, indexed by the slot minus c0 nv; a null pointer is skipped
  double *point, *solution, *grad_phi;  // [.][3], [.], [.][3]
  double *patch_field[kMaxFields];
};

template <int DIM>
__global__ __launch_bounds__(kPatchThreads) void patch_kernel(PatchArgs a) {
  constexpr int nv = 1 << DIM;
  static_assert(64 % nv == 0 && kPatchThreads % 64 == 0, "a cell's lanes lie in one wavefront");
  const int64_t n_slots = (a.c1 - a.c0) * nv;
  const int64_t n_round = (n_slots + kPatchThreads - 1) / kPatchThreads * kPatchThreads;  // whole workgroups take every turn
  for (int64_t t = (int64_t)blockIdx.x * kPatchThreads + threadIdx.x; t < n_round; t += (int64_t)gridDim.x * kPatchThreads) {
    const int v = (int)(t & (nv - 1));
    const int64_t cell = a.c0 + t / nv;
    const bool valid = cell < a.c1;  // the guard is on the cell: its nv lanes agree
    int32_t dof = 0;
    double U = 0.0;
    if (valid) {
      dof = a.cell_dofs[cell * nv + v];
      U = a.u[dof];
    }
    double other[DIM];
    for (int d = 0; d < DIM; ++d) other[d] = __shfl_xor(U, 1 << d);
    if (!valid) continue;
    if (a.solution) a.solution[t] = U;
    if (a.point) {
      const unsigned long long k = a.vertex_of_dof[dof];
      for (int d = 0; d < 3; ++d) a.point[3 * t + d] = d < DIM ? coordinate(k, d, a.origin, a.hf) : 0.0;
    }
    if (a.grad_phi) {
      const double h = edge_length(a.h0, (int)a.cell_level[cell]);
      for (int d = 0; d < 3; ++d) a.grad_phi[3 * t + d] = d < DIM ? field_component(U, other[d < DIM ? d : 0], ((v >> d) & 1) != 0, h) : 0.0;
    }
    for (int j = 0; j < a.n_fields; ++j)
      if (a.patch_field[j]) a.patch_field[j][t] = a.dof_field[j][dof];
  }
}
#endif

}  // namespace gmg_output
