// gmg_density.hpp -- charge densities from the resident mesh tables (gmg_charge_density_resident,
// gmg_get_resident_cell_geometry).
//
// Reference: compute_charge_densities() (src/step-50.cc:509-575) with the atom lists of rhs_assembly_optimization()
// (:260-306); the definition is the one of gmg_charge_density in include/gmg_coulomb.h.  What differs from
// charge_density_kernel (gmg_device.hpp):
//   geometry   no per-cell arrays come from the host.  A cell's level and the vertex key of its first DoF -- both in the
//              tables gmg_build_mesh_tables left on the device -- give its integer coordinates, hence its corner, its edge and
//              its root (dr_cell_geometry, which gmg_get_resident_cell_geometry copies out);
//   shape      a cell has a GROUP of g = 2^lg_g lanes, g the smallest power of two >= min(nq, 64), so a wavefront carries
//              64 / g cells.  The group walks the candidates of its root's bin box in order, g at a time: every lane tests
//              the list predicate on one candidate, and the atoms that pass are appended in candidate order to the group's
//              LDS segment as (x, y, z, q) through __ballot and a popcount prefix.  When a segment of the wavefront cannot
//              take another g atoms, or nobody has candidates left, every lane runs over its group's segment for its OWN
//              quadrature point and adds to its own accumulator.  nq > 64 walks the candidates once per 64 points;
//   order      every output value is one sequential sum by one lane in candidate order -- the rows (z, y ascending) of the
//              root's bin box, each row's bins x ascending (one contiguous run of the bin table), a bin's atoms in stored
//              order; all atoms in index order without lists.  No cross-lane reduction: the bits depend neither on the
//              grid, nor on g, nor on the segment length.
// The ballots, the flush decision and the loop over cells are wave-uniform (every lane of the wavefront reaches them);
// everything between them may diverge.  A group lies inside one wavefront, whose LDS operations complete in program order:
// the segment needs no workgroup barrier.  The segments of a workgroup's groups are `cap` atoms = 32 cap bytes apart with cap
// odd, so the groups of a wavefront, which read the same slot j of their segments at once, fall into different banks.
#pragma once
#include "gmg_device.hpp"

namespace gmg {

constexpr int kDrThreads = 256;
constexpr int kDrKeyBits = 21, kDrKeyShift = 12;  // vertex keys: 21 bits per direction, in units of 2^-12 root cells

struct DensityResArgs {
  // the resident tables
  const int32_t *cell_dofs;                 // [n_cells * 8]
  const uint8_t *cell_level;                // [n_cells]
  const unsigned long long *vertex_of_dof;  // [n_dofs]
  int64_t n_cells;
  double origin, h0;
  // the atoms and their bins (gmg_forces::bin_atoms)
  const double *atom_xyz;  // [n_atoms * 3]
  const double *atom_q;
  int n_atoms;
  double bin_lo0, bin_lo1, bin_lo2, bin_size;
  int bin_n0, bin_n1, bin_n2;
  const int32_t *bin_ptr;
  const int32_t *bin_items;
  double cutoff, r_c;
  int use_lists;
  const double *qp;  // [nq * 3] quadrature points on the unit cell
  int nq;
  int lg_g;  // a cell's group has 1 << lg_g lanes
  int cap;   // atoms per LDS segment, odd, >= 1 << lg_g
  double *dens;  // [n_cells * nq]
  // gmg_get_resident_cell_geometry
  double *cell_lo, *cell_h, *root_lo;
};

// corner, edge and root corner of active cell `cell`: a rounded product, then a rounded sum, as Forest::cell_origin
__device__ inline void dr_cell_geometry(const DensityResArgs &a, int64_t cell, double lo[3], double &h, double rlo[3]) {
  const int l = a.cell_level[cell];
  const unsigned long long key = a.vertex_of_dof[a.cell_dofs[8 * cell]];
  h = a.h0 / (double)(1 << l);
  for (int d = 0; d < 3; ++d) {
    const int c = (int)((key >> (kDrKeyBits * d)) & 0x1fffffull) >> (kDrKeyShift - l);
    lo[d] = __dadd_rn(a.origin, __dmul_rn(h, (double)c));
    rlo[d] = __dadd_rn(a.origin, __dmul_rn(a.h0, (double)(c >> l)));
  }
}

__global__ __launch_bounds__(kDrThreads) void dr_geometry_kernel(DensityResArgs a) {
  for (int64_t cell = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; cell < a.n_cells; cell += (int64_t)gridDim.x * kDrThreads) {
    double lo[3], h, rlo[3];
    dr_cell_geometry(a, cell, lo, h, rlo);
    if (a.cell_h) a.cell_h[cell] = h;
    for (int d = 0; d < 3; ++d) {
      if (a.cell_lo) a.cell_lo[3 * cell + d] = lo[d];
      if (a.root_lo) a.root_lo[3 * cell + d] = rlo[d];
    }
  }
}

// dynamic LDS: (kDrThreads >> lg_g) segments of cap atoms, 4 doubles each
__global__ __launch_bounds__(kDrThreads) void density_resident_kernel(DensityResArgs a) {
  extern __shared__ double dr_lds[];
  const int g = 1 << a.lg_g;
  const int gl = (int)threadIdx.x & (g - 1);                  // lane in the group
  const int first = ((int)threadIdx.x & 63) & ~(g - 1);       // the group's first lane in the wavefront
  const unsigned long long gmask = g == 64 ? ~0ull : (1ull << g) - 1ull;
  const unsigned long long below = (1ull << gl) - 1ull;       // the group's lanes before this one
  const int groups = kDrThreads >> a.lg_g;
  double *seg = dr_lds + (size_t)((int)threadIdx.x >> a.lg_g) * (size_t)a.cap * 4;
  const int64_t stride = (int64_t)gridDim.x * groups;
  const int64_t rounds = (a.n_cells + stride - 1) / stride;
  const double constant_value = 4.0 * M_PI / (a.r_c * a.r_c * a.r_c * pow(M_PI, 1.5));
  const double inv = 1.0 / (a.r_c * a.r_c);
  const double blo[3] = {a.bin_lo0, a.bin_lo1, a.bin_lo2};
  const int bn[3] = {a.bin_n0, a.bin_n1, a.bin_n2};
  for (int64_t round = 0; round < rounds; ++round) {  // (wave-uniform: a group past the last cell idles through it)
    const int64_t cell = round * stride + (int64_t)blockIdx.x * groups + ((int)threadIdx.x >> a.lg_g);
    const bool have = cell < a.n_cells;
    double lo[3] = {0, 0, 0}, h = 0, rlo[3] = {0, 0, 0}, rhi[3];
    if (have) dr_cell_geometry(a, cell, lo, h, rlo);
    for (int d = 0; d < 3; ++d) rhi[d] = rlo[d] + a.h0;
    int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
    bool any_row = have;
    if (a.use_lists) {
      for (int d = 0; d < 3; ++d) {  // clamped as doubles: a cell far from the atoms has a bin index no int holds
        b0[d] = (int)fmin(fmax(floor((rlo[d] - a.cutoff - blo[d]) / a.bin_size), 0.0), (double)bn[d]);
        b1[d] = (int)fmin(fmax(floor((rhi[d] + a.cutoff - blo[d]) / a.bin_size), -1.0), (double)(bn[d] - 1));
        any_row = any_row && b0[d] <= b1[d];
      }
    }
    for (int qb = 0; qb < a.nq; qb += g) {
      const int qi = qb + gl;
      const bool point = have && qi < a.nq;
      double xq[3] = {0, 0, 0};
      if (point)
        for (int d = 0; d < 3; ++d) xq[d] = lo[d] + h * a.qp[3 * qi + d];
      double acc = 0.0;
      // the candidates: rows (z, y) of the bin box, each a contiguous run [k, ke) of bin_items; without lists one run of
      // all atoms
      int y = b0[1] - 1, z = b0[2], k = 0, ke = 0;
      bool more = any_row;
      if (!a.use_lists) ke = a.n_atoms;
      int fill = 0;
      for (;;) {
        while (more && k >= ke) {
          if (!a.use_lists) { more = false; break; }
          if (++y > b1[1]) { y = b0[1]; ++z; }
          if (z > b1[2]) { more = false; break; }
          const int64_t row = (int64_t)bn[0] * ((int64_t)y + (int64_t)bn[1] * z);
          k = a.bin_ptr[row + b0[0]];
          ke = a.bin_ptr[row + b1[0] + 1];
        }
        const bool testing = __any(more) != 0;
        if (testing) {
          bool pass = false;
          double ax = 0, ay = 0, az = 0;
          int atom = 0;
          if (more && k + gl < ke) {
            atom = a.use_lists ? a.bin_items[k + gl] : k + gl;
            ax = a.atom_xyz[3 * (size_t)atom]; ay = a.atom_xyz[3 * (size_t)atom + 1]; az = a.atom_xyz[3 * (size_t)atom + 2];
            pass = true;
            if (a.use_lists) {
              const double at[3] = {ax, ay, az};
              double d2 = 0.0;
              for (int d = 0; d < 3; ++d) {
                const double dl = at[d] - rlo[d], dh = at[d] - rhi[d];
                const double m = fabs(dl) <= fabs(dh) ? dl : dh;
                d2 += m * m;
              }
              pass = sqrt(d2) < a.cutoff;
            }
          }
          const unsigned long long bits = (__ballot(pass) >> first) & gmask;
          if (pass) {  // (fill + g <= cap here: the slot is inside the segment)
            double *s = seg + 4 * (size_t)(fill + __popcll(bits & below));
            s[0] = ax; s[1] = ay; s[2] = az; s[3] = a.atom_q[atom];
          }
          fill += __popcll(bits);
          if (more) k += g;
        }
        // consume the segments: when one of them cannot take g more atoms, and at the end
        if (!testing || __any(fill + g > a.cap)) {
          __builtin_amdgcn_wave_barrier();
          if (point)
            for (int j = 0; j < fill; ++j) {
              const double *s = seg + 4 * (size_t)j;
              const double dx = s[0] - xq[0], dy = s[1] - xq[1], dz = s[2] - xq[2];
              const double r = sqrt(dx * dx + dy * dy + dz * dz);  // the reference squares the distance again
              acc += constant_value * exp(-(r * r) * inv) * s[3];
            }
          __builtin_amdgcn_wave_barrier();
          fill = 0;
        }
        if (!testing) break;
      }
      if (point) a.dens[(size_t)cell * (size_t)a.nq + (size_t)qi] = acc;
    }
  }
}

}  // namespace gmg
