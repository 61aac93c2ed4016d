// gmg_forces.hpp -- electrostatic forces on the atoms: the field of the FE potential at the atoms, the short-range pair
// forces and the exact all-pairs Coulomb sum.
//
// Reference: the field E = -grad phi_h is what GradientPostprocessor (src/step-50.cc:1124-1161) writes to the VTU output;
// phi_h at an atom is the value postprocess_electrostatic_energy reads (:1354-1363, LaplaceProblem::fe_value_at here); the
// short-range pair law is the derivative of the erfc pair energy of :1325-1332.  The reference has no forces.
//
// The per-atom evaluations below are compiled twice from this one text: into the gfx950 kernels of libgmgcoulomb.so and
// into the host mirror of csrc/host/laplace_problem.cc (OpenMP).  Both build with -ffp-contract=off, so the field, which
// uses only + - * / floor ceil, has the same bits on both sides; the pair sums differ at most by what erfc / exp of the two
// math libraries differ by.  Every per-atom value is one sequential sum in an order fixed by the atom and bin numbering:
// no atomics, nothing depends on the launch shape.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GMG_FHD __host__ __device__
#else
#define GMG_FHD
#endif

namespace gmg_forces {

// the forest flattened level by level (gmg_set_point_locator): roots first, lexicographic (x fastest); node[k] >= 0 is the
// flat index of child 0 (children a = bx + 2 by + 4 bz contiguous), node[k] < 0 the active cell -node[k]-1, whose vertex v
// (same bit order) carries DoF active_dofs[8 * cell + v]
struct Locator {
  int n0[3];
  double origin[3];
  double h0;
  const int32_t *node;
  const int32_t *active_dofs;
};

// The active cell around x with ties broken toward octant s: bit d of s set sends a coordinate on a cell boundary to the
// upper side in direction d, at the root lattice (floor, or ceil - 1) and at every child split.  Octant 7 with clamp is
// LaplaceProblem::fe_value_at's search (root index clamped into the lattice, x >= mid at every split).  The cell geometry
// is not stored: the integer position c and the level are carried down, the corner is origin + h c as Forest computes it.
// Returns false when the cell leaves the lattice (clamp == false only).
GMG_FHD inline bool locate(const Locator &L, const double x[3], int s, bool clamp, int32_t &cell, int c[3], int &level) {
  for (int d = 0; d < 3; ++d) {
    const bool upper = (s >> d) & 1;
    const double t = (x[d] - L.origin[d]) / L.h0;
    int cd;
    if (!(t > -2.0 && t < (double)L.n0[d] + 2.0)) {  // far outside (or NaN): no integer conversion of huge values
      if (!clamp) return false;
      cd = t > 0.0 ? L.n0[d] - 1 : 0;
    } else {
      cd = upper ? (int)floor(t) : (int)ceil(t) - 1;
    }
    if (clamp) cd = cd < 0 ? 0 : (cd > L.n0[d] - 1 ? L.n0[d] - 1 : cd);
    else if (cd < 0 || cd >= L.n0[d]) return false;
    c[d] = cd;
  }
  int64_t k = (int64_t)c[0] + (int64_t)L.n0[0] * ((int64_t)c[1] + (int64_t)L.n0[1] * c[2]);
  level = 0;
  while (L.node[k] >= 0) {
    const double h = L.h0 / double(1 << level);
    int a = 0;
    for (int d = 0; d < 3; ++d) {
      const double x0 = L.origin[d] + h * c[d];
      const bool up = ((s >> d) & 1) ? x[d] >= x0 + 0.5 * h : x[d] > x0 + 0.5 * h;
      a |= (int)up << d;
      c[d] = 2 * c[d] + (int)up;
    }
    k = (int64_t)L.node[k] + a;
    ++level;
  }
  cell = -L.node[k] - 1;
  return true;
}

// phi_h(x) from fe_value_at's cell with its operation order, and E_h(x) = -(1/n) sum over the n octants s = 0..7 that stay
// in the lattice of grad u_K(s)(x) (trilinear interpolant of u on K(s)), summed in octant order
GMG_FHD inline void atom_field(const Locator &L, const double *u, const double x[3], double &phi, double E[3]) {
  double gs[3] = {0.0, 0.0, 0.0};
  int used = 0;
  for (int s = 0; s < 8; ++s) {
    int32_t cell;
    int c[3], level;
    if (!locate(L, x, s, false, cell, c, level)) continue;
    const double h = L.h0 / double(1 << level);
    double t[3];
    for (int d = 0; d < 3; ++d) t[d] = (x[d] - (L.origin[d] + h * c[d])) / h;
    double g[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 8; ++a) {
      const double ua = u[L.active_dofs[8 * (int64_t)cell + a]];
      for (int d = 0; d < 3; ++d) {
        double w = 1.0;
        for (int e = 0; e < 3; ++e) {
          const bool bit = (a >> e) & 1;
          w *= e == d ? (bit ? 1.0 : -1.0) : (bit ? t[e] : 1.0 - t[e]);
        }
        g[d] += w * ua;
      }
    }
    for (int d = 0; d < 3; ++d) gs[d] += g[d] / h;
    ++used;
  }
  for (int d = 0; d < 3; ++d) E[d] = used ? -(gs[d] / used) : 0.0;
  int32_t cell;
  int c[3], level;
  locate(L, x, 7, true, cell, c, level);
  const double h = L.h0 / double(1 << level);
  double t[3];
  for (int d = 0; d < 3; ++d) t[d] = (x[d] - (L.origin[d] + h * c[d])) / h;
  double v = 0.0;
  for (int a = 0; a < 8; ++a) {
    double w = 1.0;
    for (int d = 0; d < 3; ++d) w *= ((a >> d) & 1) ? t[d] : 1.0 - t[d];
    v += w * u[L.active_dofs[8 * (int64_t)cell + a]];
  }
  phi = v;
}

// phi_h(x) alone: the cell of octant 7 with clamp and the trilinear sum, in fe_value_at's operation order -- one descent per atom,
// where atom_field makes nine (the electrostatic energy needs no field: gmg_electrostatic_energy_resident)
GMG_FHD inline double atom_phi(const Locator &L, const double *u, const double x[3]) {
  int32_t cell;
  int c[3], level;
  locate(L, x, 7, true, cell, c, level);
  const double h = L.h0 / double(1 << level);
  double t[3];
  for (int d = 0; d < 3; ++d) t[d] = (x[d] - (L.origin[d] + h * c[d])) / h;
  double v = 0.0;
  for (int a = 0; a < 8; ++a) {
    double w = 1.0;
    for (int d = 0; d < 3; ++d) w *= ((a >> d) & 1) ? t[d] : 1.0 - t[d];
    v += w * u[L.active_dofs[8 * (int64_t)cell + a]];
  }
  return v;
}

// pair laws: scalar force f (F_i += f (x_i - x_j)) and energy e of one pair at distance r, r2 = r * r as summed
struct ShortLaw {  // erfc(r / r_c) / r and its derivative
  double r_c, c2, rc2;  // c2 = 2 / (sqrt(pi) r_c), rc2 = r_c^2
  static ShortLaw make(double r_c) { return ShortLaw{r_c, 2.0 / (sqrt(M_PI) * r_c), r_c * r_c}; }
  GMG_FHD void operator()(double r, double r2, double qq, double &f, double &e) const {
    const double ec = erfc(r / r_c);
    e = qq * ec / r;
    f = qq * (ec / r2 + c2 * exp(-r2 / rc2) / r) / r;
  }
};
struct DirectLaw {  // 1 / r
  GMG_FHD void operator()(double r, double r2, double qq, double &f, double &e) const {
    e = qq / r;
    f = qq / (r2 * r);
  }
};

// acc[0..2] += force of atom j on atom i, acc[3] += pair energy, for pairs closer than rcut (rcut = inf: all)
template <class Law>
GMG_FHD inline void pair_add(const Law &law, double rcut, const double *xi, const double *xj, double acc[4]) {
  const double dx = xi[0] - xj[0], dy = xi[1] - xj[1], dz = xi[2] - xj[2];
  const double r2 = dx * dx + dy * dy + dz * dz;
  const double r = sqrt(r2);
  if (!(r < rcut)) return;
  double f, e;
  law(r, r2, xi[3] * xj[3], f, e);
  acc[0] += f * dx;
  acc[1] += f * dy;
  acc[2] += f * dz;
  acc[3] += e;
}

// ---- cell bins of the atoms (host): bounding box from the minimum corner, bins of edge `size`, atoms of a bin in
// ascending order.  gmg_charge_density bins its atoms with this too.
struct Bins {
  double lo[3] = {0, 0, 0}, size = 1;
  int n[3] = {1, 1, 1};
  std::vector<int32_t> ptr, items;  // items[ptr[b] .. ptr[b + 1]) are the atoms of bin b = x + n0 (y + n1 z)
  int64_t of(const double *xyz) const {
    int b[3];
    for (int d = 0; d < 3; ++d) b[d] = std::min(n[d] - 1, std::max(0, (int)floor((xyz[d] - lo[d]) / size)));
    return (int64_t)b[0] + n[0] * ((int64_t)b[1] + (int64_t)n[1] * b[2]);
  }
};
// false (nothing built) when more than max_bins bins would be needed
inline bool bin_atoms(int64_t n_atoms, const double *xyz, double size, int64_t max_bins, Bins &B) {
  double hi[3];
  for (int d = 0; d < 3; ++d) { B.lo[d] = 1e300; hi[d] = -1e300; }
  for (int64_t i = 0; i < n_atoms; ++i)
    for (int d = 0; d < 3; ++d) { B.lo[d] = std::min(B.lo[d], xyz[3 * i + d]); hi[d] = std::max(hi[d], xyz[3 * i + d]); }
  if (n_atoms == 0)
    for (int d = 0; d < 3; ++d) B.lo[d] = hi[d] = 0;
  B.size = size;
  int64_t total = 1;
  for (int d = 0; d < 3; ++d) {
    const double nb = floor((hi[d] - B.lo[d]) / size) + 1;
    if (!(nb <= (double)max_bins)) return false;
    B.n[d] = std::max(1, (int)nb);
    total *= B.n[d];
    if (total > max_bins) return false;
  }
  B.ptr.assign((size_t)total + 1, 0);
  B.items.assign((size_t)std::max<int64_t>(n_atoms, 1), 0);
  for (int64_t i = 0; i < n_atoms; ++i) B.ptr[(size_t)B.of(xyz + 3 * i) + 1]++;
  for (int64_t b = 0; b < total; ++b) B.ptr[(size_t)b + 1] += B.ptr[(size_t)b];
  std::vector<int32_t> pos(B.ptr.begin(), B.ptr.end() - 1);
  for (int64_t i = 0; i < n_atoms; ++i) B.items[(size_t)pos[(size_t)B.of(xyz + 3 * i)]++] = (int32_t)i;
  return true;
}
// the bins of the cut-off pair sum: edge rcut, doubled until at most 2^24 bins cover the atoms (a bin edge >= rcut keeps
// every partner within the 27 neighbouring bins)
inline void force_bins(int64_t n_atoms, const double *xyz, double rcut, Bins &B) {
  double size = rcut;
  while (!bin_atoms(n_atoms, xyz, size, (int64_t)1 << 24, B)) size *= 2.0;
}
// the candidate slots of an atom in bin b, in summation order: for z, y ascending (clipped to the grid) the contiguous run of
// slots of the bins x - 1 .. x + 1 of that row
template <class F>
GMG_FHD inline void for_each_row(const int n[3], const int32_t *ptr, int64_t b, F f) {
  const int bx = (int)(b % n[0]), by = (int)((b / n[0]) % n[1]), bz = (int)(b / ((int64_t)n[0] * n[1]));
  const int x0 = bx > 0 ? bx - 1 : 0, x1 = bx + 1 < n[0] ? bx + 1 : n[0] - 1;
  for (int z = (bz > 0 ? bz - 1 : 0); z <= (bz + 1 < n[2] ? bz + 1 : n[2] - 1); ++z)
    for (int y = (by > 0 ? by - 1 : 0); y <= (by + 1 < n[1] ? by + 1 : n[1] - 1); ++y) {
      const int64_t row = (int64_t)n[0] * ((int64_t)y + (int64_t)n[1] * z);
      f(ptr[row + x0], ptr[row + x1 + 1]);
    }
}

#if defined(__HIPCC__)
// ---- kernels

// one lane per atom; xq: [n][4] (x, y, z, q)
__global__ __launch_bounds__(256) void atom_field_kernel(Locator L, const double *u, const double *xq, int n, double *phi, double *E) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x[3] = {xq[4 * (int64_t)i], xq[4 * (int64_t)i + 1], xq[4 * (int64_t)i + 2]};
  double p, e[3];
  atom_field(L, u, x, p, e);
  phi[i] = p;
  for (int d = 0; d < 3; ++d) E[3 * (int64_t)i + d] = e[d];
}

// ---- the resident point locator (gmg_build_point_locator_resident): the forest's first_child array turned into Locator::node.
// level_ptr by value: at most 13 levels, so the level of a cell is a search over constants held in scalar registers.
struct LocLevels {
  int n_levels;
  int64_t ptr[14];  // ptr[l] .. ptr[l + 1]: the cells of level l; entries past n_levels repeat the last one
};
// one thread per forest cell k (grid-stride): node[k] = ptr[level + 1] + first_child[k] for a refined cell, -(active number) - 1
// for an active one; apos[k]: the exclusive count of active cells before k (mt_active_flag_kernel scanned)
__global__ __launch_bounds__(256) void loc_node_kernel(const int32_t *first_child, const int32_t *apos, LocLevels lv, int64_t n_all, int32_t *node) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_all; k += (int64_t)gridDim.x * blockDim.x) {
    const int32_t fc = first_child[k];
    if (fc < 0) {
      node[k] = -apos[k] - 1;
      continue;
    }
    int64_t next = lv.ptr[1];  // the start of the level after k's: the last l < n_levels with ptr[l] <= k is k's level
#pragma unroll
    for (int l = 1; l < 13; ++l)
      if (l < lv.n_levels && lv.ptr[l] <= k) next = lv.ptr[l + 1];
    node[k] = (int32_t)(next + fc);
  }
}

// the per-atom terms of the electrostatic energy, one lane per atom: fe[i] = (0.5 q_i) phi_h(x_i) (phi = 0 where the mesh has
// no cell: located == 0), self[i] = q_i q_i / self_denom with self_denom = sqrt(pi) r_c formed by the caller
__global__ __launch_bounds__(256) void atom_energy_terms_kernel(Locator L, int located, const double *u, const double *xq, int n, double self_denom,
                                                                double *fe, double *self) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x[3] = {xq[4 * (int64_t)i], xq[4 * (int64_t)i + 1], xq[4 * (int64_t)i + 2]};
  const double q = xq[4 * (int64_t)i + 3];
  const double phi = located ? atom_phi(L, u, x) : 0.0;
  fe[i] = (0.5 * q) * phi;
  self[i] = q * q / self_denom;
}

// out[b] = src_b[0] + src_b[stride_b] + ... in ascending index, one sequential fp64 sum per workgroup b = 0, 1, 2: the
// workgroup stages a tile of blockDim.x values in LDS, lane 0 adds them in order.  The bits are those of a host loop over i.
struct EnergySumArgs {
  const double *src[3];
  int stride[3];
  int n;
  double *out;  // [3]
};
__global__ __launch_bounds__(256) void energy_sum_kernel(EnergySumArgs a) {
  __shared__ double tile[256];
  const double *src = blockIdx.x == 0 ? a.src[0] : blockIdx.x == 1 ? a.src[1] : a.src[2];
  const int stride = blockIdx.x == 0 ? a.stride[0] : blockIdx.x == 1 ? a.stride[1] : a.stride[2];
  double sum = 0.0;
  for (int t0 = 0; t0 < a.n; t0 += blockDim.x) {
    const int m = min((int)blockDim.x, a.n - t0);
    __syncthreads();
    if ((int)threadIdx.x < m) tile[threadIdx.x] = src[(int64_t)stride * (t0 + threadIdx.x)];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < m; ++j) sum += tile[j];
  }
  if (threadIdx.x == 0) a.out[blockIdx.x] = sum;
}

// stage slots [t0, t0 + m) of xq in LDS (m <= blockDim.x); every lane then reads the same word: broadcast, no bank conflict
__device__ __forceinline__ void stage_tile(double *tile, const double *xq, int64_t t0, int m) {
  __syncthreads();
  if ((int)threadIdx.x < m)
    for (int c = 0; c < 4; ++c) tile[4 * threadIdx.x + c] = xq[4 * (t0 + threadIdx.x) + c];
  __syncthreads();
}

// all pairs, N-body tiles: lane = atom i, j in ascending tiles of blockDim.x staged in LDS.  out: [n][4] (F, e).
template <class Law>
__global__ __launch_bounds__(256) void pair_all_kernel(Law law, double rcut, const double *xq, int n, double *out) {
  extern __shared__ double tile[];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double xi[4] = {0, 0, 0, 0}, acc[4] = {0, 0, 0, 0};
  if (i < n)
    for (int c = 0; c < 4; ++c) xi[c] = xq[4 * (int64_t)i + c];
  for (int t0 = 0; t0 < n; t0 += blockDim.x) {
    const int m = min((int)blockDim.x, n - t0);
    stage_tile(tile, xq, t0, m);
    if (i < n)
      for (int jj = 0; jj < m; ++jj)
        if (t0 + jj != i) pair_add(law, rcut, xi, tile + 4 * jj, acc);
  }
  if (i < n) {
    for (int c = 0; c < 3; ++c) out[4 * (int64_t)i + c] = acc[c];
    out[4 * (int64_t)i + 3] = 0.5 * acc[3];
  }
}

// cut-off pairs: one workgroup per unit = up to blockDim.x consecutive slots of one bin (xq sorted by bin); the candidates of
// the 27 neighbouring bins are staged row by row in LDS.  items: slot -> atom, out: [n][4] by atom.
struct BinnedArgs {
  const double *xq;
  const int32_t *items, *ptr, *unit_bin, *unit_start;
  int n[3];
  double *out;
};
template <class Law>
__global__ __launch_bounds__(256) void pair_binned_kernel(Law law, double rcut, BinnedArgs a) {
  extern __shared__ double tile[];
  const int64_t b = a.unit_bin[blockIdx.x];
  const int64_t k = (int64_t)a.ptr[b] + a.unit_start[blockIdx.x] + threadIdx.x;
  const bool valid = k < a.ptr[b + 1];
  double xi[4] = {0, 0, 0, 0}, acc[4] = {0, 0, 0, 0};
  if (valid)
    for (int c = 0; c < 4; ++c) xi[c] = a.xq[4 * k + c];
  for_each_row(a.n, a.ptr, b, [&](int64_t ks, int64_t ke) {
    for (int64_t t0 = ks; t0 < ke; t0 += blockDim.x) {
      const int m = (int)min((int64_t)blockDim.x, ke - t0);
      stage_tile(tile, a.xq, t0, m);
      if (valid)
        for (int jj = 0; jj < m; ++jj)
          if (t0 + jj != k) pair_add(law, rcut, xi, tile + 4 * jj, acc);
    }
  });
  if (valid) {
    const int64_t i = a.items[k];
    for (int c = 0; c < 3; ++c) a.out[4 * i + c] = acc[c];
    a.out[4 * i + 3] = 0.5 * acc[3];
  }
}
#endif

}  // namespace gmg_forces
