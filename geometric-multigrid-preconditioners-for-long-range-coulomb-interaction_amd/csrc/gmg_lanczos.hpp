// gmg_lanczos.hpp -- the largest eigenvalue of D^-1 A of one level, estimated on the device.
//
// m steps of Jacobi-preconditioned CG without the solution vector, from a fixed start vector, give the Lanczos
// coefficients alpha_j, beta_j; the largest eigenvalue of the tridiagonal matrix they define (the largest Ritz value) is
// a lower bound of lambda_max(D^-1 A) that a safety factor turns into the bound the Chebyshev smoother uses, as deal.II's
// PreconditionChebyshev does.  B = D^-1 is the level's invd, A the level matrix alone:
//   r_i = ((uint32)((i + 1) 2654435761) >> 8) 2^-24 - 0.5,   z = B r,  p = z,  rho_0 = r.z
//   step j:  q = A p;  alpha_j = rho_j / p.q;  r -= alpha_j q;  z = B r;  rho_{j+1} = r.z;  beta_j = rho_{j+1} / rho_j;  p = z + beta_j p
//   T_jj = 1 / alpha_j + beta_{j-1} / alpha_{j-1},   T_{j,j+1} = sqrt(beta_j) / alpha_j
// The steps stop early (breakdown) when rho_j or p.q is not finite or not positive or rho_{j+1} is not finite -- step j then
// does not count -- or when rho_{j+1} <= 2^-100 rho_0 -- step j counts and is the last.
//
// Kernels.  q = A p is the library's product (spmv(), whatever layout the level has).  Around it a step is three launches:
// lanczos_pq_kernel (partials of p.q), lanczos_r_kernel (alpha from the partials, r, partials of rho_{j+1}) and
// lanczos_p_kernel (beta, p, the step's record).  There is no host wait inside the m steps: every workgroup of a consumer
// sums the producer's partials itself (reduce_partials), the rho partials alternate between two slots so that a kernel
// never overwrites partials that its other workgroups still read, and a stop flag in device memory makes every later kernel
// return at once.  z is never stored: it is invd_i r_i wherever it is needed.
//
// The stop flag is the one word that IS written (by workgroup 0) in a launch whose other workgroups read it at entry, in both
// kernels that set it.  lanczos_r_kernel: every workgroup forms the same two sums and finds the breakdown itself, so a
// workgroup that starts late and sees the flag does what it would have done anyway: nothing.  lanczos_p_kernel (rho_{j+1} <=
// 2^-100 rho_0): a workgroup that starts late returns before it updates its rows of p, so p is left partly updated.  That
// is harmless and meant: the record of step j is complete (workgroup 0 writes it before the flag), the recurrence ends
// with this step, every later kernel of this file returns at its first statement, and the products of the remaining steps
// (spmv() knows no flag) read p and write q, which nothing reads after a stop.
//
// Reductions.  Two stages, no atomics.  The partials are those of dot_partial_kernel on grid_for(n) workgroups: partial v
// sums the rows v kThreads + t + k V kThreads (k = 0, 1, ...) of thread t in ascending k and block_sum combines the threads.
// A launch with fewer workgroups (option lanczos_max_blocks) lets each form several of the V partials one after the other:
// the same V partials, so the same bits for every grid.
//
// Every store to a level vector is under the row guard i < n; the partials are written at v < V <= kMaxPartials and the
// record at j < m; nothing else is written.
#pragma once
#include "gmg_device.hpp"

#include <cmath>
#include <cstdint>

namespace gmg {
namespace lanczos {

constexpr int kMaxSteps = 64;

// what one estimate leaves on the device: doubles [0] steps that count, [1] rho_0, [2, 2 + m) alpha, [2 + m, 2 + 2 m) beta
// (this much comes back to the host), [2 + 2 m] the stop flag
inline size_t record_len(int m) { return (size_t)2 * (size_t)m + 3; }

struct Args {
  double *r, *p;         // level vectors
  const double *q;       // A p
  const double *invd;
  int64_t n;
  int n_part;            // V: partials of every dot product
  double *part_pq;       // [V]
  double *part_rho;      // [2][kMaxPartials]: slot j & 1 holds the partials of rho_j
  double *rec;           // record_len(m)
  int m, j;
};

__device__ __forceinline__ double start_entry(int64_t i) {
  const uint32_t h = (uint32_t)((uint64_t)(i + 1) * 2654435761ull);
  return (double)(h >> 8) * 0x1p-24 - 0.5;
}

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }  // (false for NaN)

// r, p = B r and the partials of rho_0 (slot 0)
__global__ __launch_bounds__(kThreads) void lanczos_start_kernel(Args a) {
  __shared__ double red[4];
  for (int v = blockIdx.x; v < a.n_part; v += gridDim.x) {
    double acc = 0.0;
    for (int64_t i = (int64_t)v * kThreads + threadIdx.x; i < a.n; i += (int64_t)a.n_part * kThreads) {
      const double ri = start_entry(i), zi = a.invd[i] * ri;
      a.r[i] = ri;
      a.p[i] = zi;
      acc += ri * zi;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) a.part_rho[v] = s;
  }
}

// partials of p.q
__global__ __launch_bounds__(kThreads) void lanczos_pq_kernel(Args a) {
  __shared__ double red[4];
  if (a.rec[2 * a.m + 2] != 0.0) return;  // (stopped: the same word for every thread)
  for (int v = blockIdx.x; v < a.n_part; v += gridDim.x) {
    double acc = 0.0;
    for (int64_t i = (int64_t)v * kThreads + threadIdx.x; i < a.n; i += (int64_t)a.n_part * kThreads) acc += a.p[i] * a.q[i];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) a.part_pq[v] = s;
  }
}

// alpha_j = rho_j / p.q; r -= alpha_j q; the partials of rho_{j+1} = r.(B r).  A breakdown sets the stop flag and changes nothing:
// every workgroup forms the same two sums and takes the same branch
__global__ __launch_bounds__(kThreads) void lanczos_r_kernel(Args a) {
  __shared__ double red[4];
  if (a.rec[2 * a.m + 2] != 0.0) return;
  const double rho = reduce_partials(a.part_rho + (size_t)(a.j & 1) * kMaxPartials, a.n_part, red);
  const double pq = reduce_partials(a.part_pq, a.n_part, red);
  if (!(rho > 0.0) || !(pq > 0.0) || !is_finite(rho) || !is_finite(pq)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.rec[2 * a.m + 2] = 1.0;
    return;
  }
  const double alpha = rho / pq;
  double *out = a.part_rho + (size_t)((a.j + 1) & 1) * kMaxPartials;
  for (int v = blockIdx.x; v < a.n_part; v += gridDim.x) {
    double acc = 0.0;
    for (int64_t i = (int64_t)v * kThreads + threadIdx.x; i < a.n; i += (int64_t)a.n_part * kThreads) {
      const double ri = a.r[i] - alpha * a.q[i];
      a.r[i] = ri;
      acc += ri * (a.invd[i] * ri);
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) out[v] = s;
  }
}

// beta_j = rho_{j+1} / rho_j; p = B r + beta_j p; workgroup 0 writes the step's record
__global__ __launch_bounds__(kThreads) void lanczos_p_kernel(Args a) {
  __shared__ double red[4];
  if (a.rec[2 * a.m + 2] != 0.0) return;
  const double rho = reduce_partials(a.part_rho + (size_t)(a.j & 1) * kMaxPartials, a.n_part, red);
  const double rho1 = reduce_partials(a.part_rho + (size_t)((a.j + 1) & 1) * kMaxPartials, a.n_part, red);
  const double pq = reduce_partials(a.part_pq, a.n_part, red);
  if (!is_finite(rho1)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.rec[2 * a.m + 2] = 1.0;
    return;
  }
  const double beta = rho1 / rho;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double rho0 = a.j == 0 ? rho : a.rec[1];
    if (a.j == 0) a.rec[1] = rho;
    a.rec[2 + a.j] = rho / pq;  // (alpha_j: the division lanczos_r_kernel did)
    a.rec[2 + a.m + a.j] = beta;
    a.rec[0] = (double)(a.j + 1);
    if (rho1 <= 0x1p-100 * rho0) a.rec[2 * a.m + 2] = 1.0;
  }
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads)
    a.p[i] = a.invd[i] * a.r[i] + beta * a.p[i];
}

// ---- host ------------------------------------------------------------------------------------------------------------

// the largest eigenvalue of the symmetric tridiagonal matrix with diagonal d[0 .. m) and off-diagonal e[0 .. m - 1), by
// bisection on the Sturm count until the interval is two neighbouring doubles
inline double tridiag_largest(const double *d, const double *e, int m) {
  if (m <= 0) return 0.0;
  double lo = d[0], hi = d[0];
  for (int i = 0; i < m; ++i) {
    const double rad = (i > 0 ? std::fabs(e[i - 1]) : 0.0) + (i + 1 < m ? std::fabs(e[i]) : 0.0);
    lo = std::fmin(lo, d[i] - rad);
    hi = std::fmax(hi, d[i] + rad);
  }
  auto below = [&](double x) {  // eigenvalues < x
    int cnt = 0;
    double q = 1.0;
    for (int i = 0; i < m; ++i) {
      const double e2 = i > 0 ? e[i - 1] * e[i - 1] : 0.0;
      q = d[i] - x - (i > 0 ? e2 / q : 0.0);
      if (q == 0.0) q = -1e-300;
      if (q < 0.0) ++cnt;
    }
    return cnt;
  };
  if (m == 1 || !(hi > lo)) return hi;
  for (int it = 0; it < 2000; ++it) {
    const double mid = lo + 0.5 * (hi - lo);
    if (!(mid > lo) || !(mid < hi)) break;
    if (below(mid) >= m) hi = mid; else lo = mid;
  }
  return hi;
}

// the largest Ritz value of steps that count: alpha, beta as the record holds them
inline double ritz_value(const double *alpha, const double *beta, int steps) {
  double d[kMaxSteps], e[kMaxSteps];
  for (int j = 0; j < steps; ++j) {
    d[j] = 1.0 / alpha[j] + (j > 0 ? beta[j - 1] / alpha[j - 1] : 0.0);
    if (j + 1 < steps) e[j] = std::sqrt(beta[j]) / alpha[j];
  }
  return tridiag_largest(d, e, steps);
}

}  // namespace lanczos
}  // namespace gmg
