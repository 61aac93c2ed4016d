// gmg_estimate.hpp -- the error estimator and the refinement marks formed on the device (gmg_estimate_error, DESIGN.md
// section 14): LaplaceProblem::estimate_error_and_mark_cells (csrc/host/adaptive.inc; the reference's Kelly estimator with
// Strategy::cell_diameter, its cell residual and the fixed-fraction-of-the-maximum marks) from the cells' DoFs and levels, a
// face table and the solution vector, with the same bits as the host loop.
//
// Inputs.  cell_dofs [n_cells][nv] (nv = 2^dim, vertex a = bx + 2 by + 4 bz), cell_level [n_cells] (< 16), and per
// (cell a, face f = 2 d + side) slot a kind and nfc = 2^(dim-1) integers:
//   0  boundary                      -- nothing
//   1  active neighbour, same level  -- face_cell[slot * nfc] = its index
//   2  neighbour refined once        -- face_cell[slot * nfc + k] = the active child in quadrant k of the face (bit 0 of k:
//                                       the lower in-face direction)
//   3  neighbour one level coarser   -- face_cell[slot * nfc] = its index, face_cell[slot * nfc + 1] = the quadrant of the
//                                       coarse face this cell occupies
// The host checks the table (indices, levels, quadrants) before anything is launched: the kernels index without checks.
//
// Values (fp64, no contraction: the library is built with -ffp-contract=off).  U[c][v] = u[cell_dofs[c][v]]; the normal
// derivative at the face corners, for v ascending over the vertices with bit d clear,
//   g_c[k] = (U[c][v | 1 << d] - U[c][v]) / h[level(c)];
// B(c, s, t) = c0 (1-s) (1-t) + c1 s (1-t) + c2 (1-s) t + c3 s t, left to right (2D: c0 (1-s) + c1 s);
// a regular face with minus-side cell m and plus-side cell p: jump[k] = g_p[k] - g_m[k],
//   I = sum_{q1} sum_{q0} ((((j j) gw[q0]) gw[q1]) measure[l]),  j = B(jump, gx[q0], gx[q1]),  from +0.0 (2D: gw[q1] = 1.0);
// a sub-face of a coarse cell C (level l) and a fine cell F (level l + 1) in quadrant (Q0, Q1):
//   j = B(g_F, s, t) - B(g_C, 0.5 (Q0 + s), 0.5 (Q1 + t)),  summed the same way with measure[l + 1];
// the kind-3 slot of F holds that integral, the kind-2 slot of C the sum of its nfc sub-faces from +0.0 in ascending k.
// Per cell: float acc = 0; acc += (float)(diameter[l] * face_int[a][f]) for f ascending; kelly_sq = acc; eta = sqrtf(acc).
// residual != 0: error = sum_q ((t t) weight[q]) jxw[l] with t = 0.0 + (4 pi) dens[a nq + q]; residual_sq =
// (diam diam) error; residual == 1: eta = (float)sqrt((double)eta (double)eta + residual_sq).
// mx = max |eta| (fp32), threshold = fraction (double)mx, mark[a] = (double)|eta[a]| >= threshold.
//
// Every slot and every cell has one writer that forms one sequential sum; the maximum is exact in any order; the marks are
// counted with an integer atomic.  No floating-point atomics: the bits depend neither on the grid nor on the visiting order.
//
// Kernels.  (1) est_face_kernel, one thread per (cell, face) slot, a gather: a kind-1 slot forms the integral itself with
// m and p ordered by orientation, so both sides of a face hold the same bits without a scatter; a kind-2 slot recomputes
// the sub-face integrals its children's kind-3 slots hold.  (2) est_cell_kernel, one thread per cell: the float sum over
// the faces, the residual sum over the cell's quadrature points, eta, and the maximum of |eta| per workgroup.  (3)
// est_mark_kernel: every workgroup reduces the partial maxima again (the same value everywhere), one thread per cell
// writes the mark.  All loops are grid-stride.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gmg {

constexpr int kEstThreads = 256;
constexpr int kEstMaxBlocks = 1024;  // workgroups of est_cell_kernel = partial maxima est_mark_kernel reduces again
constexpr int kEstMaxGauss = 8;

struct EstArgs {
  int dim, nv, nfc, nf;  // nf = 2 dim faces
  int ng, nq, residual;
  int64_t n_cells;
  const int32_t *cell_dofs;   // [n_cells * nv]
  const uint8_t *cell_level;  // [n_cells]
  const uint8_t *face_kind;   // [n_cells * nf]
  const int32_t *face_cell;   // [n_cells * nf * nfc]
  const double *u;
  const double *dens;    // [n_cells * nq] (residual != 0)
  const double *weight;  // [nq]
  double h[16], measure[16], diameter[16], jxw[16];
  double gx[kEstMaxGauss], gw[kEstMaxGauss];
  double fraction;
  double *face_int;     // [n_cells * nf]
  double *kelly_sq;     // [n_cells]
  double *residual_sq;  // [n_cells]
  float *eta;           // [n_cells]
  float *partial;       // [gridDim.x of est_cell_kernel]
  int n_partial;
  double *threshold;  // [1]
  uint8_t *mark;      // [n_cells]
  unsigned long long *n_marked;  // [1], zeroed before est_mark_kernel
};

namespace est {

// the normal derivative across direction d at the corners of cell c's faces orthogonal to d
template <int DIM>
__device__ inline void corner_gradients(const EstArgs &a, int64_t c, int d, double (&g)[1 << (DIM - 1)]) {
  constexpr int nv = 1 << DIM;
  const double h = a.h[a.cell_level[c]];
  const int32_t *dofs = a.cell_dofs + c * nv;
  int k = 0;
  for (int v = 0; v < nv; ++v) {
    if ((v >> d) & 1) continue;
    g[k++] = (a.u[dofs[v | (1 << d)]] - a.u[dofs[v]]) / h;
  }
}

template <int DIM>
__device__ inline double interp(const double *c, double s, double t) {
  if (DIM == 2) return c[0] * (1 - s) + c[1] * s;
  return c[0] * (1 - s) * (1 - t) + c[1] * s * (1 - t) + c[2] * (1 - s) * t + c[3] * s * t;
}

// the integral over the sub-face of a coarse cell (corner gradients gC) behind the fine cell F in quadrant q of the face
template <int DIM>
__device__ inline double sub_face(const EstArgs &a, int64_t F, int d, const double *gC, int q) {
  constexpr int nfc = 1 << (DIM - 1);
  double gF[nfc];
  corner_gradients<DIM>(a, F, d, gF);
  const double measure = a.measure[a.cell_level[F]];
  const int Q0 = q & 1, Q1 = (q >> 1) & 1;
  double s = 0;
  for (int q1 = 0; q1 < (DIM == 3 ? a.ng : 1); ++q1)
    for (int q0 = 0; q0 < a.ng; ++q0) {
      const double s0 = a.gx[q0], t0 = DIM == 3 ? a.gx[q1] : 0.0;
      const double jf = interp<DIM>(gF, s0, t0);
      const double jc = interp<DIM>(gC, 0.5 * (Q0 + s0), DIM == 3 ? 0.5 * (Q1 + t0) : 0.0);
      const double j = jf - jc;
      s += j * j * a.gw[q0] * (DIM == 3 ? a.gw[q1] : 1.0) * measure;
    }
  return s;
}

template <int DIM>
__device__ inline double face_integral(const EstArgs &a, int64_t c, int f) {
  constexpr int nfc = 1 << (DIM - 1);
  const int64_t slot = c * a.nf + f;
  const int kind = a.face_kind[slot];
  if (kind == 0) return 0.0;
  const int d = f >> 1, side = f & 1;
  const int32_t *fc = a.face_cell + slot * nfc;
  if (kind == 1) {
    const int64_t m = side ? c : (int64_t)fc[0], p = side ? (int64_t)fc[0] : c;
    double gm[nfc], gp[nfc], jump[nfc];
    corner_gradients<DIM>(a, m, d, gm);
    corner_gradients<DIM>(a, p, d, gp);
    for (int k = 0; k < nfc; ++k) jump[k] = gp[k] - gm[k];
    const double measure = a.measure[a.cell_level[c]];
    double s = 0;
    for (int q1 = 0; q1 < (DIM == 3 ? a.ng : 1); ++q1)
      for (int q0 = 0; q0 < a.ng; ++q0) {
        const double j = interp<DIM>(jump, a.gx[q0], DIM == 3 ? a.gx[q1] : 0.0);
        s += j * j * a.gw[q0] * (DIM == 3 ? a.gw[q1] : 1.0) * measure;
      }
    return s;
  }
  double gC[nfc];
  if (kind == 3) {
    corner_gradients<DIM>(a, (int64_t)fc[0], d, gC);
    return sub_face<DIM>(a, c, d, gC, fc[1]);
  }
  corner_gradients<DIM>(a, c, d, gC);
  double sum = 0;
  for (int k = 0; k < nfc; ++k) sum += sub_face<DIM>(a, (int64_t)fc[k], d, gC, k);
  return sum;
}

}  // namespace est

template <int DIM>
__global__ __launch_bounds__(kEstThreads) void est_face_kernel(EstArgs a) {
  const int64_t n_slots = a.n_cells * a.nf;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += (int64_t)gridDim.x * blockDim.x)
    a.face_int[s] = est::face_integral<DIM>(a, s / a.nf, (int)(s % a.nf));
}

__global__ __launch_bounds__(kEstThreads) void est_cell_kernel(EstArgs a) {
  __shared__ float smax[kEstThreads];
  float mx = 0.f;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.n_cells; c += (int64_t)gridDim.x * blockDim.x) {
    const int l = a.cell_level[c];
    const double diam = a.diameter[l];
    float acc = 0.f;
    for (int f = 0; f < a.nf; ++f) acc += (float)(diam * a.face_int[c * a.nf + f]);
    // (the square root of a float through fp64 and one more rounding is the correctly rounded float square root: 53 >= 2 * 24 + 2)
    float eta = (float)sqrt((double)acc);
    a.kelly_sq[c] = (double)acc;
    double rsq = 0.0;
    if (a.residual) {
      const double jxw = a.jxw[l];
      const double *dens = a.dens + c * a.nq;
      double error = 0;
      for (int q = 0; q < a.nq; ++q) {
        const double temp = 0.0 + 4.0 * 3.14159265358979323846 * dens[q];
        error += temp * temp * a.weight[q] * jxw;
      }
      rsq = diam * diam * error;
      if (a.residual == 1) {
        const double e = (double)eta;
        eta = (float)sqrt(e * e + diam * diam * error);
      }
    }
    a.residual_sq[c] = rsq;
    a.eta[c] = eta;
    const float ae = fabsf(eta);
    mx = ae > mx ? ae : mx;
  }
  smax[threadIdx.x] = mx;
  __syncthreads();
  for (int w = kEstThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const float o = smax[threadIdx.x + w];
      if (o > smax[threadIdx.x]) smax[threadIdx.x] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) a.partial[blockIdx.x] = smax[0];
}

__global__ __launch_bounds__(kEstThreads) void est_mark_kernel(EstArgs a) {
  __shared__ float smax[kEstThreads];
  float mx = 0.f;
  for (int i = threadIdx.x; i < a.n_partial; i += kEstThreads) {
    const float o = a.partial[i];
    mx = o > mx ? o : mx;
  }
  smax[threadIdx.x] = mx;
  __syncthreads();
  for (int w = kEstThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const float o = smax[threadIdx.x + w];
      if (o > smax[threadIdx.x]) smax[threadIdx.x] = o;
    }
    __syncthreads();
  }
  const double threshold = a.fraction * (double)smax[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.threshold = threshold;
  unsigned int count = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.n_cells; c += (int64_t)gridDim.x * blockDim.x) {
    const bool m = (double)fabsf(a.eta[c]) >= threshold;
    a.mark[c] = m ? 1 : 0;
    count += m ? 1u : 0u;
  }
  if (count) atomicAdd(a.n_marked, (unsigned long long)count);
}

}  // namespace gmg
