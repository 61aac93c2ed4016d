// gmg_close.hpp -- boundary values and constraints.close() on the resident mesh tables (gmg_close_constraints, DESIGN.md
// section 22).
//
// Reference: VectorTools::interpolate_boundary_values + constraints.close() (src/step-50.cc:675-696); the host restates them
// as the loop "close(): masters that are themselves (Dirichlet) constrained fold into the inhomogeneity" of
// LaplaceProblem::make_constraints (csrc/host/laplace_problem.cc).  With H = n_hanging and L = n_lines of the tables that
// gmg_build_mesh_tables left on the device:
//   Dirichlet lines   l in [H, L) have no entries; inhom[l] = dirichlet_value[l - H] (+0.0 where the caller gave none);
//   hanging lines     l < H start from inhom[l] = +0.0 and visit their stored entries e in ascending order with
//                     m = constraint_of_dof[line_master[e]]:
//                       m < 0        the entry is kept (kept entries retain their relative order),
//                       m >= H       the entry is dropped and inhom[l] = inhom[l] + line_weight[e] * inhom[m], a rounded
//                                    product and a rounded sum (no fused multiply-add): the host's
//                                    line.inhomogeneity += e.second * m.inhomogeneity,
//                       0 <= m < H   a hanging node constrained to a hanging node: kClErrHanging in the flag word.
// One thread per hanging line counts its kept entries and forms inhom (at most 4 entries, one sequential sum), tr_scan_kernel
// turns the counts into the closed line_ptr, and one thread per hanging line writes the kept entries at its offset.  Every
// output element has one writer; the only atomic is the OR into the flag word, once per wave.  The flag word also says
// which numbers of kept entries occur (bit kClKeptShift + k), from which the host takes the longest closed line.  The unclosed
// tables are read only.  Plain loads and stores, no LDS.
#pragma once
#include "gmg_device.hpp"

namespace gmg {

constexpr int kClThreads = 256;
constexpr int kClErrHanging = 1;  // bit of the flag word: a master with a hanging line of its own
constexpr int kClKeptShift = 8;   // bit kClKeptShift + min(k, kClKeptMax): some hanging line keeps k entries
constexpr int kClKeptMax = 16;

struct ClArgs {
  // the unclosed tables
  const int32_t *cons;         // [n_dofs]: line of a DoF, -1: none
  const int32_t *line_ptr;     // [n_lines + 1]
  const int32_t *line_master;  // [n_entries]
  const double *line_weight;   // [n_entries]
  int64_t n_hanging;
  // the closed lines: ptr holds the counts after the COUNT pass and the offsets after the scan
  int32_t *ptr;     // [n_lines + 1]
  int32_t *master;  // [closed entries]
  double *weight;   // [closed entries]
  double *inhom;    // [n_lines]: [n_hanging, n_lines) is set before the COUNT pass, which writes [0, n_hanging)
  int *flag;
};

// FILL = false: kept entries and inhomogeneity of every hanging line; FILL = true: the kept entries at the scanned offsets
template <bool FILL>
__global__ __launch_bounds__(kClThreads) void cl_close_kernel(ClArgs a) {
  int bits = 0;
  for (int64_t l = (int64_t)blockIdx.x * kClThreads + threadIdx.x; l < a.n_hanging; l += (int64_t)gridDim.x * kClThreads) {
    const int32_t out = FILL ? a.ptr[l] : 0;
    int32_t kept = 0;
    double s = 0.0;
    for (int32_t e = a.line_ptr[l]; e < a.line_ptr[l + 1]; ++e) {
      const int32_t dof = a.line_master[e], m = a.cons[dof];
      if (m < 0) {
        if constexpr (FILL) {
          a.master[out + kept] = dof;
          a.weight[out + kept] = a.line_weight[e];
        }
        ++kept;
      } else if ((int64_t)m >= a.n_hanging) {
        if constexpr (!FILL) s = __dadd_rn(s, __dmul_rn(a.line_weight[e], a.inhom[m]));
      } else {
        bits |= kClErrHanging;
      }
    }
    if constexpr (!FILL) {
      a.ptr[l] = kept;
      a.inhom[l] = s;
      bits |= 1 << (kClKeptShift + (kept < kClKeptMax ? kept : kClKeptMax));
    }
  }
  if constexpr (!FILL) {
    for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off, 64);
    if ((threadIdx.x & 63) == 0 && bits) atomicOr(a.flag, bits);
  }
}

}  // namespace gmg
