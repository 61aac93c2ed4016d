// gmg_fastdiag.hpp -- the direct coarse solver on the level-0 lattice by fast diagonalisation.
//
// Reference: MGCoarseGridIterativeSolver::operator()(0, dst, src) (src/step-50.cc:962-967) is an unpreconditioned CG on
// mg_matrices[0]; the reference has no direct coarse solver.  On the undivided lattice with a constant coefficient the
// interior block of that matrix is separable,
//   A_int = s (K_x (x) M_y (x) M_z + M_x (x) K_y (x) M_z + M_x (x) M_y (x) K_z),   K = tridiag(-1, 2, -1),  M = tridiag(1, 4, 1) / 6,
// and K, M of one axis (n cells, m = n - 1 interior vertices) share the eigenvectors S[j][k] = sqrt(2 / n) sin(pi j k / n)
// (j, k = 1 .. m; S symmetric and orthogonal) with eigenvalues lambda_k = 2 - 2 cos(pi k / n), mu_k = (4 + 2 cos(pi k / n)) / 6:
//   x_int = (S_x (x) S_y (x) S_z) D^-1 (S_x (x) S_y (x) S_z) b_int,   D_abc = s (l_a m_b m_c + m_a l_b m_c + m_a m_b l_c),
// a boundary row is x_i = b_i / a_ii.  Six batched products with S and one scaling; no reductions, no convergence test.
//
// Kernels.  One pass is Y = S X along one axis of the m_x x m_y x m_z interior, one launch each.  A wave owns a panel of 16
// lines and forms 16 x 16 tiles of the result with v_mfma_f64_16x16x4_f64 (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j =
// lane & 15], D[row = (lane >> 4) + 4 reg][col = lane & 15]); four tiles along the transformed axis share one fragment of X.
//   * axes y, z (stride nx, nx ny): the 16 lines of a panel are 16 consecutive x, so the B fragment (4 k x 16 x) and the
//     result rows are runs of 128 contiguous bytes straight from / to global memory: D = S X;
//   * axis x (stride 1): the panel is 16 consecutive y; 64 consecutive x of each line are read as one 512-byte run into the
//     wave's own LDS image and the A fragments come from there: D = X S, result rows again 128-byte runs.
// S is stored padded with zeros to a multiple of 64 (its loads need no guard); every load of X is guarded, a fragment
// beyond m or beyond the panel is zero: nothing outside the interior of the vector is read, nothing outside it written.
// Every result element is one accumulator chain of one wave in ascending k: the bits do not depend on the grid.
#pragma once
#include "gmg_device.hpp"

#include <cmath>
#include <vector>

namespace gmg {
namespace fastdiag {

constexpr int kPad = 64;        // S is padded to a multiple of this: the tiles of one group along the transformed axis
constexpr int kMinNv = 5, kMaxNv = 1024;
constexpr int kWaves = kThreads / 64;  // waves of a workgroup: one panel each
static_assert(kThreads == 256, "the passes are written for workgroups of four waves");

// ---- host: tables and the separability check (no device) ------------------------------------------------------------

// sin(pi r / n) for an integer r in [0, 2n): folded into [0, n / 2], where the argument of sin is in [0, pi / 2] and carries
// only its own rounding -- the error of an entry does not grow with j k
inline long double sin_pi_frac(long long r, long long n) {
  long double sign = 1.0L;
  if (r > n) { r = 2 * n - r; sign = -1.0L; }  // sin(pi (2n - r) / n) = -sin(pi r / n)
  if (2 * r > n) r = n - r;                     // sin(pi (n - r) / n) = sin(pi r / n)
  const long double pi = 3.141592653589793238462643383279502884L;
  return sign * sinl(pi * (long double)r / (long double)n);
}

// S [m x m] row-major, lambda [m], mu [m] of an axis with n cells (m = n - 1); any output may be null
inline void tables(int n, double *S, double *lambda, double *mu) {
  const int m = n - 1;
  const long double c = sqrtl(2.0L / (long double)n);
  if (S)
    for (int j = 1; j <= m; ++j)
      for (int k = 1; k <= m; ++k) S[(size_t)(j - 1) * m + (k - 1)] = (double)(c * sin_pi_frac(((long long)j * k) % (2LL * n), n));
  for (int k = 1; k <= m; ++k) {
    // 1 - cos(t) = 2 sin^2(t / 2): no cancellation for small k
    const long double h = sin_pi_frac(k, 2LL * n), h2 = h * h;
    if (lambda) lambda[k - 1] = (double)(4.0L * h2);
    if (mu) mu[k - 1] = (double)(1.0L - 2.0L * h2 / 3.0L);
  }
}

// Ke = s (k (x) m (x) m + m (x) k (x) m + m (x) m (x) k) with s = 3 Ke[0][0], every entry within 64 * 2^-53 * max |Ke|?
// (k = [[1, -1], [-1, 1]], m = [[2, 1], [1, 2]] / 6, local index bit 0 = x, bit 1 = y, bit 2 = z)
inline bool separable(const double *Ke, double *s_out) {
  const double s = 3.0 * Ke[0];
  double amax = 0.0;
  for (int i = 0; i < 64; ++i) {
    if (!std::isfinite(Ke[i])) return false;
    amax = std::max(amax, std::fabs(Ke[i]));
  }
  if (!(s > 0.0)) return false;
  const double tol = 64.0 * 1.1102230246251565e-16 * amax;
  auto k1 = [](int a, int b) { return a == b ? 1.0 : -1.0; };
  auto m1 = [](int a, int b) { return a == b ? 2.0 / 6.0 : 1.0 / 6.0; };
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) {
      const int ix = i & 1, iy = (i >> 1) & 1, iz = i >> 2, jx = j & 1, jy = (j >> 1) & 1, jz = j >> 2;
      const double e = k1(ix, jx) * m1(iy, jy) * m1(iz, jz) + m1(ix, jx) * k1(iy, jy) * m1(iz, jz) + m1(ix, jx) * m1(iy, jy) * k1(iz, jz);
      if (!(std::fabs(Ke[i * 8 + j] - s * e) <= tol)) return false;
    }
  if (s_out) *s_out = s;
  return true;
}

// ---- device -------------------------------------------------------------------------------------------------------------

typedef double d4 __attribute__((ext_vector_type(4)));

struct Axis {
  const double *S;    // [ld][ld], zero beyond m
  const double *lam;  // [m]
  const double *mu;   // [m]
  int m, ld;          // interior vertices, padded size (multiple of kPad)
};

struct PassArgs {
  const double *src;
  double *dst;
  Axis ax[3];
  int nx, nxy;  // line and plane stride of the lattice
  int axis;     // the transformed axis
  double s;     // scale of the operator (the D^-1 pass)
};

// Y = S X along y (axis 1) or z (axis 2); SCALE: the result is divided by D_abc (the last forward pass, axis 2)
template <bool SCALE>
__global__ __launch_bounds__(kThreads) void fastdiag_pass_yz_kernel(PassArgs A) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int a = A.axis, o = 3 - a;  // the other strided axis
  const int m = A.ax[a].m, mx = A.ax[0].m, mo = A.ax[o].m, ld = A.ax[a].ld;
  const long long sa = a == 1 ? A.nx : A.nxy, so = a == 1 ? A.nxy : A.nx;
  const int xt = (mx + 15) >> 4, n_panels = xt * mo;
  const double *S = A.ax[a].S;
  for (int p = (int)blockIdx.x * kWaves + wid; p < n_panels; p += (int)gridDim.x * kWaves) {
    const int io = p / xt, x0 = (p - io * xt) * 16;
    const bool cx = x0 + c < mx;
    const long long base = (long long)(io + 1) * so + 1 + x0 + c;  // vertex (x0 + c, io) of the interior, axis index -1
    for (int j0 = 0; j0 < m; j0 += kPad) {
      d4 acc[4] = {};
      for (int k0 = 0; k0 < m; k0 += 4) {
        const int k = k0 + q;
        const double xv = (cx && k < m) ? A.src[base + (long long)(k + 1) * sa] : 0.0;
        const double *Sr = S + (size_t)k * ld + j0 + c;  // S[j][k] = S[k][j]: 16 consecutive j per k
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (j0 + 16 * t < m) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Sr[16 * t], xv, acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = j0 + 16 * t + q + 4 * r;
          if (cx && j < m) {
            double v = acc[t][r];
            if constexpr (SCALE) {
              // (axis 2: the lane's element is (x0 + c, io, j))
              const double lx = A.ax[0].lam[x0 + c], ux = A.ax[0].mu[x0 + c], ly = A.ax[1].lam[io], uy = A.ax[1].mu[io];
              const double lz = A.ax[2].lam[j], uz = A.ax[2].mu[j];
              v = v / (A.s * (lx * uy * uz + ux * ly * uz + ux * uy * lz));
            }
            A.dst[base + (long long)(j + 1) * sa] = v;
          }
        }
    }
  }
}

// Y = S X along x (axis 0): lines of 16 consecutive y, staged 64 x at a time through the wave's own LDS image
__global__ __launch_bounds__(kThreads) void fastdiag_pass_x_kernel(PassArgs A) {
  __shared__ double stage[kWaves][16 * 65];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int m = A.ax[0].m, my = A.ax[1].m, mz = A.ax[2].m, ld = A.ax[0].ld;
  const int yt = (my + 15) >> 4, n_panels = yt * mz;
  const double *S = A.ax[0].S;
  double *st = stage[wid];
  for (int p = (int)blockIdx.x * kWaves + wid; p < n_panels; p += (int)gridDim.x * kWaves) {
    const int iz = p / yt, y0 = (p - iz * yt) * 16;
    const long long base = (long long)(iz + 1) * A.nxy + (long long)(y0 + 1) * A.nx + 1;  // vertex (0, y0, iz) of the interior
    for (int j0 = 0; j0 < m; j0 += kPad) {
      d4 acc[4] = {};
      for (int kc = 0; kc < m; kc += 64) {
        __builtin_amdgcn_wave_barrier();  // (the fragments of the previous chunk have been read)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          st[i * 65 + lane] = (y0 + i < my && kc + lane < m) ? A.src[base + (long long)i * A.nx + kc + lane] : 0.0;
        __builtin_amdgcn_wave_barrier();
        for (int ks = 0; ks < 16 && kc + 4 * ks < m; ++ks) {
          const double xv = st[c * 65 + 4 * ks + q];
          const double *Sr = S + (size_t)(kc + 4 * ks + q) * ld + j0 + c;
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (j0 + 16 * t < m) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, Sr[16 * t], acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = q + 4 * r, j = j0 + 16 * t + c;
          if (y0 + i < my && j < m) A.dst[base + (long long)i * A.nx + j] = acc[t][r];
        }
    }
  }
}

// boundary rows: x_i = b_i / a_ii, the diagonal from the class table of gmg_set_level_matrix_lattice
__global__ __launch_bounds__(kThreads) void fastdiag_boundary_kernel(double *x, const double *b, const uint8_t *rowcls, const double *ctab, int nx, int ny, int nz) {
  const long long n = (long long)nx * ny * nz;
  for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < n; r += (long long)gridDim.x * kThreads) {
    const int ix = (int)(r % nx), iy = (int)((r / nx) % ny), iz = (int)(r / ((long long)nx * ny));
    if (ix == 0 || ix == nx - 1 || iy == 0 || iy == ny - 1 || iz == 0 || iz == nz - 1) x[r] = b[r] / ctab[(int)rowcls[r] * 27 + 13];
  }
}

}  // namespace fastdiag
}  // namespace gmg
