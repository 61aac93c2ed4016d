// gmg_exact.hpp -- the exact free-space potential of the Gaussian charges, phi(x) = sum_i q_i erf(|x - x_i| / r_c) / |x - x_i|,
// and its gradient, summed over ALL atoms at many points: the boundary values of `Boundary conditions selection = Exact`
// and the error of the FE solution in the energy norm.
//
// Reference: Analytical_Solution::value and ::gradient (include/step_50.h:338-369), called per boundary DoF by
// VectorTools::interpolate_boundary_values (src/step-50.cc:661-696) and per quadrature point by
// postprocess_error_in_energy_norm (:1423-1461).
//
// Like gmg_forces.hpp this one text is compiled twice: into the gfx950 kernels of libgmgcoulomb.so and into the host mirror of
// csrc/host/laplace_problem.cc (OpenMP over the points), both with -ffp-contract=off.  Every output value is one sequential
// sum over the atoms in ascending index: no atomics, nothing depends on the launch shape or on how a call is cut into
// launches.  The two sides differ by what erf / exp of the two math libraries differ by.  fp64 throughout, no cutoff.
#pragma once
#include "gmg_forces.hpp"

namespace gmg_exact {

struct Gauss {
  double r_c, inv;  // inv = 1 / (sqrt(pi) r_c)
  static Gauss make(double r_c) { return Gauss{r_c, 1.0 / (sqrt(M_PI) * r_c)}; }
};

// dir = x - x_i and r = |dir|, the squares added in coordinate order
GMG_FHD inline double distance(const double x[3], const double *a, double dir[3]) {
  double r2 = 0.0;
  for (int d = 0; d < 3; ++d) {
    dir[d] = x[d] - a[d];
    r2 += dir[d] * dir[d];
  }
  return sqrt(r2);
}

// value of atom (x_i, q) at distance r: q erf(r / r_c) / r, and its limit 2 q / (sqrt(pi) r_c) for r < 1e-10 (the operand
// order of LaplaceProblem::boundary_value)
GMG_FHD inline double value(const Gauss &g, double r, double q) { return r < 1e-10 ? q * 2.0 * g.inv : q * (erf(r / g.r_c) / r); }

// g(s) = (2 s exp(-s^2) / sqrt(pi) - erf(s)) / s^2 for s < kGradSeriesBelow by its Taylor series
// (2 / sqrt(pi)) sum_{k >= 1} (-1)^k 2 k / ((2 k + 1) k!) s^(2 k - 1), ten terms in Horner form: the first term left out is
// 4e-8 s^20 of the leading one, below 1e-19 up to the switch
constexpr double kGradSeriesBelow = 0.25;
GMG_FHD inline double grad_series(double s) {
  const double z = s * s;
  double p = 1.0 / 3810240.0;
  p = -1.0 / 383040.0 + z * p;
  p = 1.0 / 42840.0 + z * p;
  p = -1.0 / 5400.0 + z * p;
  p = 1.0 / 780.0 + z * p;
  p = -1.0 / 132.0 + z * p;
  p = 1.0 / 27.0 + z * p;
  p = -1.0 / 7.0 + z * p;
  p = 0.4 + z * p;
  p = -2.0 / 3.0 + z * p;
  return 1.1283791670955126 * (s * p);  // 2 / sqrt(pi)
}

// ga += gradient of that value: f (x - x_i) / r.  For s = r / r_c >= 0.25, f = q (2 r exp(-s^2) / (sqrt(pi) r_c) - erf(s)) / r^2,
// the operand order of postprocess_error_in_energy_norm with its two pow(., 2) written as products.  Its two terms agree to
// O(s^2), so close to the atom their difference keeps no digit (relative error about 3 / s^2 times that of erf; all of it
// at s = 1e-8).  For s < 0.25, f = q g(s) / r_c^2 with g from its series: accurate relative to the contribution itself down
// to r -> 0, where it vanishes.  r == 0 adds nothing: the gradient of a Gaussian charge's potential at its centre is 0 (the
// reference divides by zero there).
GMG_FHD inline void gradient_add(const Gauss &g, double r, double q, const double dir[3], double ga[3]) {
  if (r == 0.0) return;
  const double s = r / g.r_c;
  const double f = s < kGradSeriesBelow ? q * (grad_series(s) / (g.r_c * g.r_c))
                                        : q * (((2.0 * r * exp(-(s * s)) * g.inv) - erf(s)) / (r * r));
  for (int d = 0; d < 3; ++d) ga[d] += f * dir[d] / r;
}

// |grad phi_h - ga|^2 w h^3 at one quadrature point of a cell of edge h: grad phi_h from the cell's 8 DoFs of u with the
// reference gradients sg[a][d] of that point (unit cell), divided by h term by term as the host loop does
GMG_FHD inline double point_err2(const double *u, const int32_t *dofs, const double *sg, double h, double w, const double ga[3]) {
  double gh[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < 8; ++a)
    for (int d = 0; d < 3; ++d) gh[d] += u[dofs[a]] * sg[3 * a + d] / h;
  double n2 = 0.0;
  for (int d = 0; d < 3; ++d) n2 += (gh[d] - ga[d]) * (gh[d] - ga[d]);
  return n2 * w * (h * h * h);
}

#if defined(__HIPCC__)
// ---- kernels: lane = point, the atoms xq [n][4] (x, y, z, q) in ascending tiles of blockDim.x staged in LDS
// (gmg_forces::stage_tile: every lane reads the same word, a broadcast)

// points [p0, p1) of pts [.][3]: phi[p] and / or grad[3 p]
template <bool WANT_PHI, bool WANT_GRAD>
__global__ __launch_bounds__(256) void gauss_potential_kernel(Gauss g, const double *xq, int n_atoms, const double *pts, int64_t p0,
                                                              int64_t p1, double *phi, double *grad) {
  extern __shared__ double tile[];
  const int64_t p = p0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = p < p1;
  double x[3] = {0.0, 0.0, 0.0}, v = 0.0, ga[3] = {0.0, 0.0, 0.0};
  if (valid)
    for (int d = 0; d < 3; ++d) x[d] = pts[3 * p + d];
  for (int t0 = 0; t0 < n_atoms; t0 += blockDim.x) {
    const int m = min((int)blockDim.x, n_atoms - t0);
    gmg_forces::stage_tile(tile, xq, t0, m);
    if (valid)
      for (int jj = 0; jj < m; ++jj) {
        const double *a = tile + 4 * jj;
        double dir[3];
        const double r = distance(x, a, dir);
        if (WANT_PHI) v += value(g, r, a[3]);
        if (WANT_GRAD) gradient_add(g, r, a[3], dir, ga);
      }
  }
  if (!valid) return;
  if (WANT_PHI) phi[p] = v;
  if (WANT_GRAD)
    for (int d = 0; d < 3; ++d) grad[3 * p + d] = ga[d];
}

// cells [c0, c1): a workgroup takes blockDim.x / nq cells, lane = quadrature point q of its cell (point = cell_lo + h qp[q]);
// the nq values of a cell are added in ascending q by the cell's first lane into cell_err2[cell]
struct ErrorArgs {
  Gauss g;
  const double *xq;
  int n_atoms, nq;
  const double *cell_lo, *cell_h;  // [n_cells][3], [n_cells]
  const int32_t *cell_dofs;        // [n_cells][8]
  const double *u;
  const double *qp, *w, *shape_grad;  // [nq][3], [nq], [nq][8][3]
  int64_t c0, c1;
  double *cell_err2;
};
__global__ __launch_bounds__(256) void energy_error_kernel(ErrorArgs a) {
  extern __shared__ double lds[];
  double *tile = lds, *val = lds + 4 * blockDim.x;
  const int per_block = (int)blockDim.x / a.nq;
  const int lc = (int)threadIdx.x / a.nq, q = (int)threadIdx.x % a.nq;
  const int64_t cell = a.c0 + (int64_t)blockIdx.x * per_block + lc;
  const bool valid = lc < per_block && cell < a.c1;
  double x[3] = {0.0, 0.0, 0.0}, ga[3] = {0.0, 0.0, 0.0}, h = 1.0;
  if (valid) {
    h = a.cell_h[cell];
    for (int d = 0; d < 3; ++d) x[d] = a.cell_lo[3 * cell + d] + h * a.qp[3 * q + d];
  }
  for (int t0 = 0; t0 < a.n_atoms; t0 += blockDim.x) {
    const int m = min((int)blockDim.x, a.n_atoms - t0);
    gmg_forces::stage_tile(tile, a.xq, t0, m);
    if (valid)
      for (int jj = 0; jj < m; ++jj) {
        const double *at = tile + 4 * jj;
        double dir[3];
        const double r = distance(x, at, dir);
        gradient_add(a.g, r, at[3], dir, ga);
      }
  }
  val[threadIdx.x] = valid ? point_err2(a.u, a.cell_dofs + 8 * cell, a.shape_grad + 24 * q, h, a.w[q], ga) : 0.0;
  __syncthreads();
  if (valid && q == 0) {
    double s = 0.0;
    for (int k = 0; k < a.nq; ++k) s += val[threadIdx.x + k];
    a.cell_err2[cell] = s;
  }
}
#endif

}  // namespace gmg_exact
