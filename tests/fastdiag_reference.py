"""Reference for the direct coarse solver (csrc/gmg_fastdiag.hpp), independent of the sine transform.

For every lattice shape of SHAPES the level-0 matrix A_0 comes from oracle.step50_oracle (cell_matrices,
assemble_constrained on a Lattice; a BoxLattice for the shapes the oracle's cubic Lattice cannot describe), the solution
x_ref from scipy's sparse LU plus one step of refinement whose residual is formed in longdouble, and kappa_2 of the interior
block from a dense eigvalsh.  The tolerances are derived here, from the reference alone, with u = 2^-53:

  one transform output   |y_i - y_ref,i| <= (m + 4) u sum_j |S_ij| |x_j|
      m products summed in any order (m u to first order) plus the error of the table's entries (4 ulp, tested apart);
  a solve                ||b - A x||_2 <= c u kappa_2 ||b||_2   and   ||x - x_ref||_2 <= c u kappa_2 ||x_ref||_2,
      c = 6 (m_max + 4) sqrt(m_max): six transforms, each with the componentwise bound above and || |S| ||_2 <= sqrt(m).

It also holds the numpy restatement of the definition (fastdiag_solve), which tests/test_fastdiag_reference_cpu.py proves
inside both bounds and sensitive to a wrong eigenvalue and to confused axes, and the inputs the GPU tests share."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import step50_oracle as so  # noqa: E402

U = 2.0 ** -53
H = 0.25  # cell size: the scale of the operator is s = H
# m = nv - 2 interior vertices per axis: all tile padding; exactly one 16-tile; tile + 1, sub-tile and two tiles + 1;
# another non-cubic one; the production m = 119 on each axis in turn
SHAPES = [(5, 5, 5), (18, 18, 18), (19, 6, 35), (7, 34, 5), (121, 7, 7), (7, 121, 7), (7, 7, 121)]


def shape_id(shape):
    return "x".join(str(v) for v in shape)


class BoxLattice:
    """What cell_matrices / assemble_constrained read of a Lattice, for nv = (nx, ny, nz) vertices: DoFs x fastest, cells x
    fastest."""

    dim = 3

    def __init__(self, nv, h):
        self.nv3, self.h = tuple(int(v) for v in nv), float(h)

    @property
    def n_dofs(self):
        return int(np.prod(self.nv3))

    @property
    def n_cells(self):
        return int(np.prod([v - 1 for v in self.nv3]))

    def boundary_mask(self):
        ex, ey, ez = [(np.arange(v) == 0) | (np.arange(v) == v - 1) for v in self.nv3]
        return (ez[:, None, None] | ey[None, :, None] | ex[None, None, :]).ravel()

    def cell_dofs(self):
        nx, ny, nz = self.nv3
        K, J, I = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
        base = (I + nx * (J + ny * K)).ravel()
        offs = np.array([(i & 1) + nx * (((i >> 1) & 1) + ny * ((i >> 2) & 1)) for i in range(8)])
        return base[:, None] + offs[None, :]


def lattice(shape):
    if shape[0] == shape[1] == shape[2]:
        return so.Lattice(3, shape[0] - 1, 0.0, H)  # the oracle's own
    return BoxLattice(shape, H)


def cell_matrix():
    return np.array(so.cell_matrices(so.Lattice(3, 4, 0.0, H))[0])


def rhs(shape, seed=0):
    """a seeded normal vector plus a ramp that differs per axis: nothing symmetric in it"""
    nx, ny, nz = shape
    rng = np.random.default_rng(1000 + 17 * seed + nx + 131 * ny + 1009 * nz)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return rng.standard_normal(nx * ny * nz) + 0.25 * (x / nx + 2.0 * y / ny - 3.0 * z / nz).ravel()


def _residual_longdouble(A, x, b):
    ld = np.longdouble
    prod = A.data.astype(ld) * x[A.indices].astype(ld)
    return b.astype(ld) - np.add.reduceat(prod, A.indptr[:-1])


@functools.lru_cache(maxsize=None)
def problem(shape):
    """namespace(shape, m, A (scipy CSR), diag, boundary, interior, b, x_ref, kappa, c, tol_res, tol_x)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    lat = lattice(shape)
    bnd = lat.boundary_mask()
    csr, _ = so.assemble_constrained(lat, so.cell_matrices(lat), bnd)
    A = sp.csr_matrix((csr.val, csr.col, csr.rowptr), shape=(csr.n_rows, csr.n_cols))
    b = rhs(shape)
    lu = spla.splu(A.tocsc())
    x0 = lu.solve(b)
    x_ref = x0 + lu.solve(np.asarray(_residual_longdouble(A, x0, b), dtype=np.float64))
    interior = np.flatnonzero(~bnd)
    ev = np.linalg.eigvalsh(A[interior][:, interior].toarray())
    kappa = float(ev[-1] / ev[0])
    m = tuple(v - 2 for v in shape)
    c = 6.0 * (max(m) + 4) * np.sqrt(max(m))
    for a in (b, x_ref):
        a.setflags(write=False)
    return SimpleNamespace(shape=shape, m=m, A=A, diag=A.diagonal(), boundary=bnd, interior=interior, b=b, x_ref=x_ref, kappa=kappa, c=c,
                           tol_res=c * U * kappa * float(np.linalg.norm(b)), tol_x=c * U * kappa * float(np.linalg.norm(x_ref)))


def solve_errors(P, x):
    """(||b - A x||_2, ||x - x_ref||_2) with the residual formed in longdouble"""
    r = _residual_longdouble(P.A, np.asarray(x, dtype=np.float64), P.b)
    return float(np.sqrt(np.sum(r * r))), float(np.linalg.norm(x - P.x_ref))


# ---- the definition, restated in numpy --------------------------------------------------------------------------------

def tables_longdouble(n):
    """(S [m, m], lambda [m], mu [m]) of an axis with n cells in longdouble, sin(pi j k / n) from (j k) mod 2n"""
    ld = np.longdouble
    k = np.arange(1, n)
    r = np.outer(k, k) % (2 * n)
    S = np.sqrt(ld(2) / ld(n)) * np.sin(_pi_ld() * r.astype(ld) / ld(n))
    half = np.sin(_pi_ld() * k.astype(ld) / ld(2 * n)) ** 2
    return S, 4 * half, 1 - 2 * half / 3


def _pi_ld():
    return np.longdouble("3.14159265358979323846264338327950288")


def tables_float64(n):
    return tuple(np.asarray(t, dtype=np.float64) for t in tables_longdouble(n))


def transform(v3, S, axis):
    """S applied along one axis (0 = x, 1 = y, 2 = z) of an interior array indexed [z, y, x]"""
    return np.moveaxis(np.tensordot(S, v3, axes=([1], [2 - axis])), 0, 2 - axis)


def fastdiag_solve(shape, b, diag, tabs=None, s=H):
    """x = (S_x (x) S_y (x) S_z) D^-1 (S_x (x) S_y (x) S_z) b on the interior, b / diag on the boundary; tabs: per axis (S,
    lambda, mu), default tables_float64"""
    nx, ny, nz = shape
    tabs = tabs or [tables_float64(v - 1) for v in shape]
    (Sx, lx, ux), (Sy, ly, uy), (Sz, lz, uz) = tabs
    b3 = np.asarray(b).reshape(nz, ny, nx)
    x = np.asarray(b / diag).reshape(nz, ny, nx).copy()
    t = b3[1:-1, 1:-1, 1:-1]
    for axis, S in enumerate((Sx, Sy, Sz)):
        t = transform(t, S, axis)
    D = s * (uz[:, None, None] * uy[None, :, None] * lx[None, None, :] + uz[:, None, None] * ly[None, :, None] * ux[None, None, :]
             + lz[:, None, None] * uy[None, :, None] * ux[None, None, :])
    t = t / D
    for axis, S in reversed(list(enumerate((Sx, Sy, Sz)))):
        t = transform(t, S, axis)
    x[1:-1, 1:-1, 1:-1] = t
    return x.ravel()


def transform_reference(shape, v, axis):
    """(y_ref, bound) of one pass on the interior of the level-0 vector v, in longdouble with the longdouble table:
    y_ref and bound as full vectors (zero on the boundary rows)"""
    nx, ny, nz = shape
    ld = np.longdouble
    S = tables_longdouble(shape[axis] - 1)[0]
    v3 = np.asarray(v).reshape(nz, ny, nx)[1:-1, 1:-1, 1:-1].astype(ld)
    y = np.zeros((nz, ny, nx), dtype=ld)
    bound = np.zeros((nz, ny, nx), dtype=ld)
    y[1:-1, 1:-1, 1:-1] = transform(v3, S, axis)
    bound[1:-1, 1:-1, 1:-1] = (shape[axis] - 2 + 4) * ld(U) * transform(np.abs(v3), np.abs(S), axis)
    return y.ravel(), bound.ravel()
