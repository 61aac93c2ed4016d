"""ctypes binding of the C-ABI in include/gmg_coulomb.h (libgmgcoulomb.so).

This is plumbing for tests and bench.py: it adds nothing to the ABI.  There is NO CPU
fallback: if the HIP library is missing, or there is no GPU, the calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

OK, ERR_INVALID, ERR_OUTER_NOCONV, ERR_COARSE_NOCONV, ERR_HIP, ERR_COMM, ERR_UNSUPPORTED = range(7)
SYSTEM = -1
JACOBI, SSOR, CHEBYSHEV = 0, 1, 2
PRECOND_GMG, PRECOND_JACOBI, PRECOND_IDENTITY = 0, 1, 2
SSOR_PARTITION_ROWS, SSOR_PARTITION_BALANCED = 0, 1
COARSE_CG, COARSE_DIRECT = 0, 1
CHEB_FIRST_KIND, CHEB_FOURTH_KIND = 0, 1
CHEB_LMAX_GERSHGORIN, CHEB_LMAX_LANCZOS = 0, 1
CHEBYSHEV_KEYS = ("polynomial", "lmax_source", "lanczos_steps", "steps_run", "gershgorin", "ritz", "safety", "lmax")
LEVEL_A, LEVEL_EDGE, LEVEL_EDGE_T = 0, 1, 2
UNIQUE_ID_BYTES = 128

# every symbol include/gmg_coulomb.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "gmg_create", "gmg_destroy", "gmg_reset", "gmg_last_error", "gmg_synchronize",
    "gmg_set_system_matrix", "gmg_set_level_matrix", "gmg_set_level_matrix_lattice", "gmg_set_edge_matrix", "gmg_set_prolongation", "gmg_build_transfer", "gmg_get_transfer",
    "gmg_assemble_system_matrix", "gmg_get_system_matrix", "gmg_system_matrix_norms",
    "gmg_assemble_level_matrix", "gmg_get_level_matrix", "gmg_assemble_system_matrix_coef", "gmg_assemble_level_matrix_coef",
    "gmg_assemble_rhs", "gmg_distribute_constraints",
    "gmg_build_mesh_tables", "gmg_get_mesh_tables", "gmg_get_mesh_level_tables",
    "gmg_close_constraints", "gmg_get_closed_constraints",
    "gmg_assemble_system_matrix_resident", "gmg_assemble_system_matrix_coef_resident", "gmg_assemble_level_matrix_resident",
    "gmg_assemble_level_matrix_coef_resident", "gmg_assemble_rhs_resident", "gmg_distribute_constraints_resident",
    "gmg_refine_forest", "gmg_get_refined_forest", "gmg_transfer_solution", "gmg_build_face_table",
    "gmg_estimate_error",
    "gmg_build_face_table_resident", "gmg_get_face_table", "gmg_estimate_error_resident", "gmg_get_marks", "gmg_refine_forest_marked",
    "gmg_energy_norm_error_resident",
    "gmg_output_patches", "gmg_output_patches_resident",
    "gmg_build_point_locator_resident", "gmg_get_point_locator", "gmg_atom_forces_resident", "gmg_electrostatic_energy_resident",
    "gmg_set_copy_indices", "gmg_set_smoother", "gmg_set_coarse", "gmg_set_chebyshev", "gmg_estimate_lmax", "gmg_get_chebyshev",
    "gmg_set_coarse_solver", "gmg_coarse_direct_tables", "gmg_coarse_direct_separable", "gmg_coarse_direct_transform", "gmg_coarse_direct_profile",
    "gmg_vec_alloc", "gmg_vec_free", "gmg_vec_upload", "gmg_vec_download", "gmg_vec_set_zero", "gmg_vec_equ",
    "gmg_vec_add", "gmg_vec_sadd", "gmg_vec_dot", "gmg_vec_norms", "gmg_vec_all_zero",
    "gmg_spmv", "gmg_precondition", "gmg_precondition_jacobi", "gmg_coarse_solve", "gmg_smoother_step",
    "gmg_prolongate", "gmg_restrict_and_add", "gmg_cg_solve", "gmg_cg_direction_step", "gmg_cg_update_step",
    "gmg_comm_unique_id", "gmg_comm_init", "gmg_comm_barrier", "gmg_comm_info", "gmg_set_halo_plan", "gmg_set_global_sizes", "gmg_partition_range",
    "gmg_vec_allgather",
    "gmg_stats_reset", "gmg_stats_get", "gmg_set_profiling", "gmg_set_tuning", "gmg_set_option", "gmg_set_ssor_blocks",
    "gmg_set_ssor_block_rows", "gmg_set_ssor_partition", "gmg_get_ssor_partition", "gmg_ssor_balance_rows", "gmg_calibrate_hbm", "gmg_charge_density", "gmg_get_charge_density", "gmg_rhs_assemble",
    "gmg_charge_density_resident", "gmg_get_resident_cell_geometry",
    "gmg_set_point_locator", "gmg_atom_forces", "gmg_direct_coulomb",
    "gmg_gaussian_potential", "gmg_energy_norm_error",
    "gmg_get_ssor_plan", "gmg_get_ssor_backward_rows", "gmg_ssor_slot_plan",
    "gmg_get_ssor_plan_array", "gmg_get_ssor_plan_origin",
    "gmg_ssor_pack_levels", "gmg_ssor_slot_plan_packed", "gmg_get_ssor_schedule",
]


class Stats(C.Structure):
    _fields_ = [("coarse_solves", C.c_int64), ("coarse_iterations", C.c_int64), ("vcycles", C.c_int64),
                ("spmv0_samples", C.c_int64), ("spmv0_ms_total", C.c_double), ("spmv0_rows", C.c_int64),
                ("spmv0_nnz", C.c_int64), ("cgupd_samples", C.c_int64), ("cgupd_ms_total", C.c_double),
                ("coarse_variant", C.c_int64), ("spmv0_layout", C.c_int64), ("spmv0_matrix_bytes", C.c_int64),
                ("spmv0_pattern_slices", C.c_int64), ("spmv0_slices", C.c_int64), ("coarse_enqueued", C.c_int64),
                ("spmv0_noop_samples", C.c_int64), ("spmv0_noop_ms_total", C.c_double),
                ("sgs_samples", C.c_int64), ("sgs_ms_total", C.c_double), ("sgs_substeps", C.c_int64), ("sgs_stream_bytes", C.c_int64),
                ("sgs_launches", C.c_int64), ("build_matrices_ms", C.c_double), ("coarse_solver", C.c_int64)]


class GMGError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gmg error {code}: {msg}")
        self.code = code


_lib = None


def load(build_if_missing: bool = False):
    """dlopen libgmgcoulomb.so from the source tree.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        # (GMG_DEVICE_LIB: measurement scripts only -- tools/build_experiments.sh; the host-side C++ always links the shipped library)
        path = os.environ.get("GMG_DEVICE_LIB") or _build.LIB_DEVICE
        if build_if_missing:
            _build.build_device()
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        _lib = C.CDLL(path)
        _lib.gmg_last_error.restype = C.c_char_p
        _lib.gmg_last_error.argtypes = [C.c_void_p]
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _csr(m):
    return (np.ascontiguousarray(m.rowptr, dtype=np.int64), np.ascontiguousarray(m.col, dtype=np.int32),
            np.ascontiguousarray(m.val, dtype=np.float64))


class DeviceVector:
    def __init__(self, ctx: "Context", n: int):
        self.ctx, self.n = ctx, int(n)
        self.ptr = C.POINTER(C.c_double)()
        ctx._chk(ctx.L.gmg_vec_alloc(ctx.h, C.c_int64(self.n), C.byref(self.ptr)))

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n
        self.ctx._chk(self.ctx.L.gmg_vec_upload(self.ctx.h, self.ptr, _p(a, C.c_double), C.c_int64(self.n)))
        return self

    def download(self):
        out = np.empty(self.n)
        self.ctx._chk(self.ctx.L.gmg_vec_download(self.ctx.h, _p(out, C.c_double), self.ptr, C.c_int64(self.n)))
        return out

    def free(self):
        if self.ptr:
            self.ctx.L.gmg_vec_free(self.ctx.h, self.ptr)
            self.ptr = C.POINTER(C.c_double)()


class Context:
    """Thin object view of a gmg_context*."""

    def __init__(self, n_levels: int, device: int = 0):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.gmg_create(C.byref(self.h), C.c_int(device), C.c_int(n_levels))
        if rc != OK:
            raise GMGError(rc, "gmg_create failed (no MI355X visible?)")
        self.n_levels = n_levels
        self.n_system = 0

    @classmethod
    def view(cls, handle):
        """Non-owning view of a gmg_context* created elsewhere (the host-side C++)."""
        self = cls.__new__(cls)
        self.L, self.h, self.owned = load(), handle, False
        self.n_levels = self.n_system = 0
        return self

    owned = True

    def close(self):
        if self.h and self.owned:
            self.L.gmg_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise GMGError(rc, self.L.gmg_last_error(self.h).decode())

    def reset(self, n_levels: int):
        """gmg_reset: drops every operator and every table derived from one; the context then has n_levels empty levels"""
        self._chk(self.L.gmg_reset(self.h, C.c_int(n_levels)))
        self.n_levels = n_levels
        self.n_system = 0

    # ---- operators
    def set_system_matrix(self, m):
        rp, c, v = _csr(m)
        self._chk(self.L.gmg_set_system_matrix(self.h, C.c_int64(m.n_rows), C.c_int64(m.n_cols), _p(rp, C.c_int64),
                                               _p(c, C.c_int32), _p(v, C.c_double)))
        self.n_system = m.n_rows

    def set_level_matrix(self, level, m):
        rp, c, v = _csr(m)
        self._chk(self.L.gmg_set_level_matrix(self.h, C.c_int(level), C.c_int64(m.n_rows), C.c_int64(m.n_cols),
                                              _p(rp, C.c_int64), _p(c, C.c_int32), _p(v, C.c_double)))

    def set_level_matrix_lattice(self, level, nv, Ke):
        """level 0 of an undivided lattice formed on the device: nv vertices per direction, Ke the 8 x 8 cell matrix"""
        nv3 = (C.c_int32 * 3)(*[int(v) for v in nv])
        ke = np.ascontiguousarray(Ke, dtype=np.float64).reshape(64)
        self._chk(self.L.gmg_set_level_matrix_lattice(self.h, C.c_int(level), nv3, _p(ke, C.c_double)))

    def set_edge_matrix(self, level, m):
        rp, c, v = _csr(m)
        self._chk(self.L.gmg_set_edge_matrix(self.h, C.c_int(level), C.c_int64(m.n_rows), C.c_int64(m.n_cols),
                                             _p(rp, C.c_int64), _p(c, C.c_int32), _p(v, C.c_double)))

    def set_prolongation(self, level, m):
        rp, c, v = _csr(m)
        self._chk(self.L.gmg_set_prolongation(self.h, C.c_int(level), C.c_int64(m.n_rows), C.c_int64(m.n_cols),
                                              _p(rp, C.c_int64), _p(c, C.c_int32), _p(v, C.c_double)))

    def build_transfer(self, level, dim, coarse_vertex, coarse_boundary, fine_vertex, fine_spacing):
        """MGTransferPrebuilt::build_matrices on the device; returns the device time in ms"""
        cv = np.ascontiguousarray(coarse_vertex, dtype=np.uint64)
        cb = np.ascontiguousarray(coarse_boundary, dtype=np.uint8)
        fv = np.ascontiguousarray(fine_vertex, dtype=np.uint64)
        ms = C.c_double(0)
        self._chk(self.L.gmg_build_transfer(self.h, C.c_int(level), C.c_int(dim), C.c_int64(len(cv)), _p(cv, C.c_uint64), _p(cb, C.c_uint8),
                                            C.c_int64(len(fv)), _p(fv, C.c_uint64), C.c_uint64(int(fine_spacing)), C.byref(ms)))
        return ms.value

    def get_transfer(self, level, transposed=False):
        from types import SimpleNamespace
        nr, nc, nz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.gmg_get_transfer(self.h, C.c_int(level), C.c_int(1 if transposed else 0), C.byref(nr), C.byref(nc), C.byref(nz), None, None, None))
        rp = np.zeros(nr.value + 1, dtype=np.int64)
        col, val = np.zeros(max(nz.value, 1), dtype=np.int32), np.zeros(max(nz.value, 1))
        self._chk(self.L.gmg_get_transfer(self.h, C.c_int(level), C.c_int(1 if transposed else 0), C.byref(nr), C.byref(nc), C.byref(nz),
                                          _p(rp, C.c_int64), _p(col, C.c_int32), _p(val, C.c_double)))
        return SimpleNamespace(n_rows=nr.value, n_cols=nc.value, nnz=nz.value, rowptr=rp, col=col[:nz.value], val=val[:nz.value])

    def build_mesh_tables(self, dim, n0, level_ptr, cell_coord, cell_first_child, level0_lexicographic=True, n_levels=None):
        """DoF numbering, constraints and level flags from the forest (gmg_build_mesh_tables); the tables stay on the device
        (get_mesh_tables, get_mesh_level_tables).  None for an array passes NULL.  Returns the device time in ms."""
        def opt(a, dt, ct):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=dt)
            return a, _p(a, ct)
        lp, lp_p = opt(level_ptr, np.int64, C.c_int64)
        cc, cc_p = opt(cell_coord, np.int32, C.c_int32)
        fc, fc_p = opt(cell_first_child, np.int32, C.c_int32)
        n03 = None if n0 is None else (C.c_int32 * 3)(*[int(v) for v in n0])
        if n_levels is None:
            n_levels = len(lp) - 1
        ms = C.c_double(0)
        self.mesh_dim = int(dim)
        self._chk(self.L.gmg_build_mesh_tables(self.h, C.c_int(int(dim)), n03, C.c_int(int(n_levels)), lp_p, cc_p, fc_p, C.c_int(1 if level0_lexicographic else 0),
                                               C.byref(ms)))
        return ms.value

    def _mesh_dim(self, dim):
        dim = getattr(self, "mesh_dim", None) if dim is None else dim
        if dim not in (2, 3):
            raise ValueError("the dimension of the mesh tables is not known to this view: pass dim")
        return dim

    def get_mesh_tables(self, dim=None):
        """The active-mesh tables of the last build_mesh_tables as numpy arrays (dim: only for a view of a context whose
        tables were built elsewhere)"""
        from types import SimpleNamespace
        n = [C.c_int64(0) for _ in range(5)]
        self._chk(self.L.gmg_get_mesh_tables(self.h, *[C.byref(v) for v in n], None, None, None, None, None, None, None, None))
        nc, nd, nh, nl, ne = [v.value for v in n]
        cd = np.zeros(nc << self._mesh_dim(dim), dtype=np.int32)
        lv, vk, cons = np.zeros(nc, dtype=np.uint8), np.zeros(nd, dtype=np.uint64), np.zeros(nd, dtype=np.int32)
        lp, lm, lw, ld = np.zeros(nl + 1, dtype=np.int64), np.zeros(ne, dtype=np.int32), np.zeros(ne), np.zeros(nl, dtype=np.int32)
        self._chk(self.L.gmg_get_mesh_tables(self.h, *[C.byref(v) for v in n], _p(cd, C.c_int32), _p(lv, C.c_uint8), _p(vk, C.c_uint64), _p(cons, C.c_int32),
                                             _p(lp, C.c_int64), _p(lm, C.c_int32), _p(lw, C.c_double), _p(ld, C.c_int32)))
        return SimpleNamespace(n_cells=nc, n_dofs=nd, n_hanging=nh, n_lines=nl, n_entries=ne, cell_dofs=cd, cell_level=lv, vertex_of_dof=vk,
                               constraint_of_dof=cons, line_ptr=lp, line_master=lm, line_weight=lw, line_dof=ld)

    def get_mesh_level_tables(self, level, dim=None):
        """One level's tables of the last build_mesh_tables as numpy arrays"""
        from types import SimpleNamespace
        nc, nd = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.gmg_get_mesh_level_tables(self.h, C.c_int(int(level)), C.byref(nc), C.byref(nd), None, None, None))
        cd, vk, fl = np.zeros(nc.value << self._mesh_dim(dim), dtype=np.int32), np.zeros(nd.value, dtype=np.uint64), np.zeros(nd.value, dtype=np.uint8)
        self._chk(self.L.gmg_get_mesh_level_tables(self.h, C.c_int(int(level)), C.byref(nc), C.byref(nd), _p(cd, C.c_int32), _p(vk, C.c_uint64), _p(fl, C.c_uint8)))
        return SimpleNamespace(n_cells=nc.value, n_dofs=nd.value, cell_dofs=cd, vertex_of_dof=vk, dof_flags=fl)

    # ---- boundary values and close() on the resident tables, and the entries that read the tables where they lie
    def close_constraints(self, dirichlet_value=None, n_values=None):
        """Boundary values and close() on the tables of the last build_mesh_tables (gmg_close_constraints); returns the device
        time in ms.  dirichlet_value: one value per Dirichlet line, in line order; None passes NULL (all +0.0), with n_values
        (default: the number of Dirichlet lines of the tables)."""
        ms = C.c_double(0)
        if dirichlet_value is None:
            if n_values is None:
                n = [C.c_int64(0) for _ in range(5)]
                self._chk(self.L.gmg_get_mesh_tables(self.h, *[C.byref(v) for v in n], None, None, None, None, None, None, None, None))
                n_values = n[3].value - n[2].value
            self._chk(self.L.gmg_close_constraints(self.h, C.c_int64(int(n_values)), None, C.byref(ms)))
            return ms.value
        v = np.ascontiguousarray(dirichlet_value, dtype=np.float64)
        self._chk(self.L.gmg_close_constraints(self.h, C.c_int64(len(v) if n_values is None else int(n_values)), _p(v, C.c_double), C.byref(ms)))
        return ms.value

    def get_closed_constraints(self):
        """The closed lines of the last close_constraints as numpy arrays"""
        from types import SimpleNamespace
        nl, ne = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.gmg_get_closed_constraints(self.h, C.byref(nl), C.byref(ne), None, None, None, None))
        lp, lm, lw, li = np.zeros(nl.value + 1, dtype=np.int64), np.zeros(ne.value, dtype=np.int32), np.zeros(ne.value), np.zeros(nl.value)
        self._chk(self.L.gmg_get_closed_constraints(self.h, C.byref(nl), C.byref(ne), _p(lp, C.c_int64), _p(lm, C.c_int32), _p(lw, C.c_double), _p(li, C.c_double)))
        return SimpleNamespace(n_lines=nl.value, n_entries=ne.value, line_ptr=lp, line_master=lm, line_weight=lw, line_inhomogeneity=li)

    def assemble_system_matrix_resident(self, K_of_level):
        """gmg_assemble_system_matrix on the resident tables and closed lines; returns the device time in ms"""
        K = np.ascontiguousarray([] if K_of_level is None else K_of_level, dtype=np.float64)
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_system_matrix_resident(self.h, _p(K, C.c_double) if K.size else None, C.byref(ms)))
        return ms.value

    def assemble_system_matrix_coef_resident(self, nq, cell_coef, G, qw, scale_of_level):
        """gmg_assemble_system_matrix_coef on the resident tables and closed lines; returns the device time in ms"""
        cc, g, w, sc = (np.ascontiguousarray([] if a is None else a, dtype=np.float64) for a in (cell_coef, G, qw, scale_of_level))
        D = lambda a: _p(a, C.c_double) if a.size else None
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_system_matrix_coef_resident(self.h, C.c_int(int(nq)), D(cc), D(g), D(w), D(sc), C.byref(ms)))
        return ms.value

    def assemble_level_matrix_resident(self, level, K):
        """gmg_assemble_level_matrix on the level's resident cell table and flags; returns the device time in ms"""
        k = np.ascontiguousarray([] if K is None else K, dtype=np.float64)
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_level_matrix_resident(self.h, C.c_int(int(level)), _p(k, C.c_double) if k.size else None, C.byref(ms)))
        return ms.value

    def assemble_level_matrix_coef_resident(self, level, nq, cell_coef, G, qw, scale):
        """gmg_assemble_level_matrix_coef on the level's resident cell table and flags; returns the device time in ms"""
        cc, g, w = (np.ascontiguousarray([] if a is None else a, dtype=np.float64) for a in (cell_coef, G, qw))
        D = lambda a: _p(a, C.c_double) if a.size else None
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_level_matrix_coef_resident(self.h, C.c_int(int(level)), C.c_int(int(nq)), D(cc), D(g), D(w), C.c_double(float(scale)),
                                                                 C.byref(ms)))
        return ms.value

    def assemble_rhs_resident(self, inp, rhs, source=True, K_of_level=True):
        """gmg_assemble_rhs on the resident tables and closed lines into rhs (DeviceVector); of inp (see assemble_rhs) only
        K_of_level, nq, shape, weight, jxw_of_level and source are read.  Returns the device time in ms."""
        f64 = lambda a: np.ascontiguousarray([] if a is None else a, dtype=np.float64)
        K = f64(inp.K_of_level if K_of_level is True else K_of_level)
        sh, w, jxw = f64(inp.shape), f64(inp.weight), f64(inp.jxw_of_level)
        src = f64(inp.source if source is True else source)
        D = lambda a: _p(a, C.c_double) if a.size else None
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_rhs_resident(self.h, D(K), C.c_int(int(inp.nq)), D(sh), D(w), D(jxw), D(src), None if rhs is None else rhs.ptr,
                                                   C.byref(ms)))
        return ms.value

    def distribute_constraints_resident(self, u, n_dofs=None):
        """constraints.distribute in place on the DeviceVector u with the resident closed lines"""
        self._chk(self.L.gmg_distribute_constraints_resident(self.h, C.c_int64(u.n if n_dofs is None else int(n_dofs)), None if u is None else u.ptr))

    @staticmethod
    def _forest_args(dim, n0, level_ptr, cell_coord, cell_first_child, n_levels):
        """the forest as the entries take it; None for an array passes NULL.  Returns (ctypes arguments, arrays to keep alive)"""
        def opt(a, dt, ct):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=dt)
            return a, _p(a, ct)
        lp, lp_p = opt(level_ptr, np.int64, C.c_int64)
        cc, cc_p = opt(cell_coord, np.int32, C.c_int32)
        fc, fc_p = opt(cell_first_child, np.int32, C.c_int32)
        n03 = None if n0 is None else (C.c_int32 * 3)(*[int(v) for v in n0])
        if n_levels is None:
            n_levels = len(lp) - 1
        return (C.c_int(int(dim)), n03, C.c_int(int(n_levels)), lp_p, cc_p, fc_p), (lp, cc, fc, n03)

    def refine_forest(self, dim, n0, level_ptr, cell_coord, cell_first_child, flag, n_levels=None):
        """The 2:1 closure of the marks and the split (gmg_refine_forest); the new forest stays on the device
        (get_refined_forest).  Returns namespace(n_levels, n_cells, n_split, build_ms)."""
        from types import SimpleNamespace
        args, keep = self._forest_args(dim, n0, level_ptr, cell_coord, cell_first_child, n_levels)
        fl = None if flag is None else np.ascontiguousarray(flag, dtype=np.uint8)
        nl, nc, ns, ms = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        self._chk(self.L.gmg_refine_forest(self.h, *args, None if fl is None else _p(fl, C.c_uint8), C.byref(nl), C.byref(nc), C.byref(ns), C.byref(ms)))
        return SimpleNamespace(n_levels=nl.value, n_cells=nc.value, n_split=ns.value, build_ms=ms.value)

    def get_refined_forest(self):
        """The forest of the last refine_forest as numpy arrays: namespace(n_levels, n_cells, n_split, level_ptr, cell_coord
        [n, 3], cell_first_child, cell_parent, closed_flag [cells of the forest that went in])"""
        from types import SimpleNamespace
        nl, nc, nf, ns = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.gmg_get_refined_forest(self.h, C.byref(nl), C.byref(nc), C.byref(nf), C.byref(ns), None, None, None, None, None))
        lp, cc = np.zeros(nl.value + 1, dtype=np.int64), np.zeros((nc.value, 3), dtype=np.int32)
        fc, pa, cl = np.zeros(nc.value, dtype=np.int32), np.zeros(nc.value, dtype=np.int32), np.zeros(nf.value, dtype=np.uint8)
        self._chk(self.L.gmg_get_refined_forest(self.h, None, None, None, None, _p(lp, C.c_int64), _p(cc, C.c_int32), _p(fc, C.c_int32), _p(pa, C.c_int32),
                                                _p(cl, C.c_uint8)))
        return SimpleNamespace(n_levels=nl.value, n_cells=nc.value, n_split=ns.value, level_ptr=lp, cell_coord=cc, cell_first_child=fc, cell_parent=pa,
                               closed_flag=cl)

    def transfer_solution(self, dim, n0, level_ptr, cell_coord, cell_first_child, old_vertex_of_dof, u_old, new_vertex_of_dof, constraint_of_dof, u_new,
                          n_levels=None, n_old=None, n_new=None):
        """SolutionTransfer::interpolate + constraints.set_zero on the new forest (gmg_transfer_solution): u_old and u_new are
        DeviceVectors (or None: NULL), the vertex lists and constraint_of_dof host arrays (None: NULL).  Returns the device
        time in ms."""
        args, keep = self._forest_args(dim, n0, level_ptr, cell_coord, cell_first_child, n_levels)
        ov = None if old_vertex_of_dof is None else np.ascontiguousarray(old_vertex_of_dof, dtype=np.uint64)
        nv = None if new_vertex_of_dof is None else np.ascontiguousarray(new_vertex_of_dof, dtype=np.uint64)
        co = None if constraint_of_dof is None else np.ascontiguousarray(constraint_of_dof, dtype=np.int32)
        n_old = (0 if ov is None else len(ov)) if n_old is None else n_old
        n_new = (0 if nv is None else len(nv)) if n_new is None else n_new
        ms = C.c_double(0)
        self._chk(self.L.gmg_transfer_solution(self.h, *args, C.c_int64(n_old), None if ov is None else _p(ov, C.c_uint64), None if u_old is None else u_old.ptr,
                                               C.c_int64(n_new), None if nv is None else _p(nv, C.c_uint64), None if co is None else _p(co, C.c_int32),
                                               None if u_new is None else u_new.ptr, C.byref(ms)))
        return ms.value

    def build_face_table(self, dim, n0, level_ptr, cell_coord, cell_first_child, n_levels=None):
        """The estimator's face table from the forest (gmg_build_face_table): namespace(n_active, face_kind [n_active, 2 dim],
        face_cell [n_active, 2 dim, 2^(dim-1)], build_ms)"""
        from types import SimpleNamespace
        args, keep = self._forest_args(dim, n0, level_ptr, cell_coord, cell_first_child, n_levels)
        na, ms = C.c_int64(0), C.c_double(0)
        self._chk(self.L.gmg_build_face_table(self.h, *args, C.byref(na), None, None, None))
        dim = int(dim)
        fk, fcell = np.zeros((na.value, 2 * dim), dtype=np.uint8), np.zeros((na.value, 2 * dim, 1 << (dim - 1)), dtype=np.int32)
        # (a buffer of one entry stands in for an empty array: the arrays' being NULL asks for the size alone)
        k1, c1 = (fk, fcell) if na.value else (np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int32))
        self._chk(self.L.gmg_build_face_table(self.h, *args, C.byref(na), _p(k1, C.c_uint8), _p(c1, C.c_int32), C.byref(ms)))
        return SimpleNamespace(n_active=na.value, face_kind=fk, face_cell=fcell, build_ms=ms.value)

    def set_copy_indices(self, level, global_idx, level_idx):
        g = np.ascontiguousarray(global_idx, dtype=np.int32)
        l = np.ascontiguousarray(level_idx, dtype=np.int32)
        self._chk(self.L.gmg_set_copy_indices(self.h, C.c_int(level), C.c_int64(len(g)), _p(g, C.c_int32), _p(l, C.c_int32)))

    def set_smoother(self, kind, omega=0.5, steps=2, cheb_degree=2, cheb_ratio=30.0, cheb_lmax=0.0):
        self._chk(self.L.gmg_set_smoother(self.h, C.c_int(kind), C.c_double(omega), C.c_int(steps), C.c_int(cheb_degree),
                                          C.c_double(cheb_ratio), C.c_double(cheb_lmax)))

    def set_chebyshev(self, polynomial=CHEB_FIRST_KIND, lmax_source=CHEB_LMAX_GERSHGORIN, lanczos_steps=0, safety=0.0):
        """gmg_set_chebyshev: the polynomial and the source of lambda_max; lanczos_steps = 0 / safety = 0 keep their values"""
        self._chk(self.L.gmg_set_chebyshev(self.h, C.c_int(polynomial), C.c_int(lmax_source), C.c_int(lanczos_steps), C.c_double(safety)))

    def estimate_lmax(self, level, steps=10, coefficients=True):
        """gmg_estimate_lmax: dict(ritz, steps_run, alpha [steps], beta [steps]) of the Lanczos estimate on `level`"""
        ritz, run = C.c_double(0.0), C.c_int(0)
        alpha, beta = np.zeros(max(int(steps), 1)), np.zeros(max(int(steps), 1))
        pa, pb = (_p(alpha, C.c_double), _p(beta, C.c_double)) if coefficients else (None, None)
        self._chk(self.L.gmg_estimate_lmax(self.h, C.c_int(level), C.c_int(steps), C.byref(ritz), pa, pb, C.byref(run)))
        return {"ritz": ritz.value, "steps_run": run.value, "alpha": alpha, "beta": beta}

    def get_chebyshev(self, level):
        """gmg_get_chebyshev as a dict over CHEBYSHEV_KEYS"""
        out = np.zeros(8)
        self._chk(self.L.gmg_get_chebyshev(self.h, C.c_int(level), _p(out, C.c_double)))
        return dict(zip(CHEBYSHEV_KEYS, out.tolist()))

    def set_coarse(self, abs_tol=1e-10, max_it=1000):
        self._chk(self.L.gmg_set_coarse(self.h, C.c_double(abs_tol), C.c_int(max_it)))

    def set_coarse_solver(self, kind):
        """COARSE_CG or COARSE_DIRECT (fast diagonalisation on a lattice level 0); GMGError with code ERR_UNSUPPORTED and
        the reason where level 0 does not qualify -- the coarse CG then stays selected."""
        self._chk(self.L.gmg_set_coarse_solver(self.h, C.c_int(kind)))

    def coarse_direct_transform(self, axis, dst, src):
        """dst <- S_axis src on the interior of a level-0 vector (one pass of the direct coarse solver)"""
        self._chk(self.L.gmg_coarse_direct_transform(self.h, C.c_int(axis), dst.ptr, src.ptr))

    def coarse_direct_profile(self, dst, src):
        """one direct coarse solve; the kernel times in ms of its seven launches (x, y, z + scaling, z, y, x, boundary rows)"""
        ms = np.zeros(7)
        self._chk(self.L.gmg_coarse_direct_profile(self.h, dst.ptr, src.ptr, _p(ms, C.c_double)))
        return ms

    def load_hierarchy(self, hier):
        """Upload everything LaplaceProblem::solve consumes (any object with the attribute
        names of the hierarchy the host side produces)."""
        self.set_system_matrix(hier.system_matrix)
        for l, A in enumerate(hier.level_matrices):
            self.set_level_matrix(l, A)
            I = hier.edge_matrices[l]
            if I is not None and I.nnz > 0:
                self.set_edge_matrix(l, I)
            self.set_copy_indices(l, hier.copy_global[l], hier.copy_level[l])
        for l, P in enumerate(hier.prolongations):
            self.set_prolongation(l, P)

    # ---- vectors
    def vector(self, n, data=None):
        v = DeviceVector(self, n)
        if data is not None:
            v.upload(data)
        return v

    def dot(self, x, y):
        out = C.c_double(0)
        self._chk(self.L.gmg_vec_dot(self.h, x.ptr, y.ptr, C.c_int64(x.n), C.byref(out)))
        return out.value

    def norms(self, x):
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self.L.gmg_vec_norms(self.h, x.ptr, C.c_int64(x.n), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def all_zero(self, x):
        out = C.c_int(0)
        self._chk(self.L.gmg_vec_all_zero(self.h, x.ptr, C.c_int64(x.n), C.byref(out)))
        return bool(out.value)

    def equ(self, y, a, x):
        self._chk(self.L.gmg_vec_equ(self.h, y.ptr, C.c_double(a), x.ptr, C.c_int64(y.n)))

    def add(self, y, a, x):
        self._chk(self.L.gmg_vec_add(self.h, y.ptr, C.c_double(a), x.ptr, C.c_int64(y.n)))

    def sadd(self, y, s, a, x):
        self._chk(self.L.gmg_vec_sadd(self.h, y.ptr, C.c_double(s), C.c_double(a), x.ptr, C.c_int64(y.n)))

    def set_zero(self, x):
        self._chk(self.L.gmg_vec_set_zero(self.h, x.ptr, C.c_int64(x.n)))

    # ---- concepts
    def spmv(self, which, dst, src):
        self._chk(self.L.gmg_spmv(self.h, C.c_int(which), dst.ptr, src.ptr))

    def precondition(self, dst, src):
        self._chk(self.L.gmg_precondition(self.h, dst.ptr, src.ptr))

    def precondition_jacobi(self, omega, dst, src):
        self._chk(self.L.gmg_precondition_jacobi(self.h, C.c_double(omega), dst.ptr, src.ptr))

    def coarse_solve(self, dst, src, want_residual=True):
        it, res = C.c_int(0), C.c_double(0)
        rc = self.L.gmg_coarse_solve(self.h, dst.ptr, src.ptr, C.byref(it), C.byref(res) if want_residual else None)
        return it.value, res.value, rc

    def smoother_step(self, level, u, rhs, from_zero):
        self._chk(self.L.gmg_smoother_step(self.h, C.c_int(level), u.ptr, rhs.ptr, C.c_int(1 if from_zero else 0)))

    def prolongate(self, level, dst, src):
        self._chk(self.L.gmg_prolongate(self.h, C.c_int(level), dst.ptr, src.ptr))

    def restrict_and_add(self, level, dst, src):
        self._chk(self.L.gmg_restrict_and_add(self.h, C.c_int(level), dst.ptr, src.ptr))

    def cg_solve(self, x, b, rel_tol=1e-8, max_it=500, precond=PRECOND_GMG):
        it, r0, r = C.c_int(0), C.c_double(0), C.c_double(0)
        rc = self.L.gmg_cg_solve(self.h, x.ptr, b.ptr, C.c_double(rel_tol), C.c_int(max_it), C.c_int(precond),
                                 C.byref(it), C.byref(r0), C.byref(r))
        return {"iterations": it.value, "starting_value": r0.value, "convergence_value": r.value, "status": rc}

    def cg_direction_step(self, d, g, h, first):
        """first: d = -h; else d = beta d - h with beta = g.h / (the g.h of the previous call).  g.h stays in the context."""
        self._chk(self.L.gmg_cg_direction_step(self.h, d.ptr, g.ptr, h.ptr, C.c_int64(d.n), C.c_int(1 if first else 0)))

    def cg_update_step(self, x, g, d, h):
        """alpha = (kept g.h) / d.h; x += alpha d; g += alpha h; returns g.g."""
        gg = C.c_double(0)
        self._chk(self.L.gmg_cg_update_step(self.h, x.ptr, g.ptr, d.ptr, h.ptr, C.c_int64(x.n), C.byref(gg)))
        return gg.value

    # ---- forces on the atoms (gmg_forces.hpp)
    def set_point_locator(self, n0, origin, h0, node, active_dofs):
        """The forest flattened level by level (node[k] >= 0: child 0, < 0: active cell -node[k]-1) and the DoFs of the
        active cells' vertices [n_active, 8]."""
        n0 = np.ascontiguousarray(n0, dtype=np.int32)
        org = np.ascontiguousarray(origin, dtype=np.float64)
        node = np.ascontiguousarray(node, dtype=np.int32)
        dofs = np.ascontiguousarray(active_dofs, dtype=np.int32).reshape(-1)
        self._chk(self.L.gmg_set_point_locator(self.h, _p(n0, C.c_int32), _p(org, C.c_double), C.c_double(h0), C.c_int64(node.size),
                                               _p(node, C.c_int32), C.c_int64(dofs.size // 8), _p(dofs, C.c_int32)))

    def atom_forces(self, xyz, q, u, r_c, cutoff=0.0):
        """u: DeviceVector of the constraint-distributed solution -> dict phi [n], field [n, 3], force [n, 3],
        force_short [n, 3], e_short [n]."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(q, dtype=np.float64)
        n = len(q)
        out = dict(phi=np.zeros(n), field=np.zeros((n, 3)), force=np.zeros((n, 3)), force_short=np.zeros((n, 3)), e_short=np.zeros(n))
        D = lambda k: _p(out[k], C.c_double)
        self._chk(self.L.gmg_atom_forces(self.h, C.c_int64(n), _p(xyz, C.c_double), _p(q, C.c_double), u.ptr, C.c_int64(u.n),
                                         C.c_double(r_c), C.c_double(cutoff), D("phi"), D("field"), D("force"), D("force_short"),
                                         D("e_short")))
        return out

    def direct_coulomb(self, xyz, q):
        """Exact all-pairs Coulomb forces [n, 3] and per-atom energies [n]."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(q, dtype=np.float64)
        F, e = np.zeros((len(q), 3)), np.zeros(len(q))
        self._chk(self.L.gmg_direct_coulomb(self.h, C.c_int64(len(q)), _p(xyz, C.c_double), _p(q, C.c_double), _p(F, C.c_double),
                                            _p(e, C.c_double)))
        return F, e

    # ---- exact free-space potential of the Gaussian charges (gmg_exact.hpp)
    def gaussian_potential(self, atom_xyz, atom_q, r_c, points, want_phi=True, want_grad=True):
        """phi [n] and grad [n, 3] (None when not wanted) of all atoms at the points [n, 3]."""
        xyz = np.ascontiguousarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(atom_q, dtype=np.float64)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        phi = np.zeros(len(pts)) if want_phi else None
        grad = np.zeros((len(pts), 3)) if want_grad else None
        D = lambda a: _p(a, C.c_double) if a is not None else None
        self._chk(self.L.gmg_gaussian_potential(self.h, C.c_int64(len(q)), D(xyz), D(q), C.c_double(r_c), C.c_int64(len(pts)), D(pts),
                                                D(phi), D(grad)))
        return phi, grad

    def energy_norm_error(self, cell_lo, cell_h, cell_dofs, u, atom_xyz, atom_q, r_c, quadrature_points, weights, shape_grad):
        """u: DeviceVector of the constraint-distributed solution -> (error, cell_err2 [n_cells])."""
        lo = np.ascontiguousarray(cell_lo, dtype=np.float64).reshape(-1, 3)
        hh = np.ascontiguousarray(cell_h, dtype=np.float64)
        dofs = np.ascontiguousarray(cell_dofs, dtype=np.int32).reshape(-1, 8)
        xyz = np.ascontiguousarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(atom_q, dtype=np.float64)
        qp = np.ascontiguousarray(quadrature_points, dtype=np.float64).reshape(-1, 3)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        sg = np.ascontiguousarray(shape_grad, dtype=np.float64).reshape(len(w), 8, 3)
        err, ce = C.c_double(0), np.zeros(len(hh))
        D = lambda a: _p(a, C.c_double)
        self._chk(self.L.gmg_energy_norm_error(self.h, C.c_int64(len(hh)), D(lo), D(hh), _p(dofs, C.c_int32), u.ptr, C.c_int64(u.n),
                                               C.c_int64(len(q)), D(xyz), D(q), C.c_double(r_c), C.c_int(len(w)), D(qp), D(w), D(sg),
                                               C.byref(err), D(ce)))
        return err.value, ce

    # ---- charge densities and the right-hand side integrated from them
    def charge_density(self, cell_lo, cell_h, root_lo, root_h, atom_xyz, atom_q, r_c, cutoff, use_lists, quadrature_points, dens=True):
        """rho [n_cells, nq] at the points cell_lo + cell_h * quadrature_points of every cell (cutoff: a distance).
        dens=None keeps the densities on the device for rhs_assemble / get_charge_density and returns None."""
        lo = np.ascontiguousarray(cell_lo, dtype=np.float64).reshape(-1, 3)
        hh = np.ascontiguousarray(cell_h, dtype=np.float64)
        rlo = np.ascontiguousarray(root_lo, dtype=np.float64).reshape(-1, 3)
        xyz = np.ascontiguousarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(atom_q, dtype=np.float64)
        qp = np.ascontiguousarray(quadrature_points, dtype=np.float64).reshape(-1, 3)
        assert len(lo) == len(hh) == len(rlo) and len(xyz) == len(q)
        out = None if dens is None else np.zeros((len(hh), len(qp)))
        D = lambda a: _p(a, C.c_double)
        self._chk(self.L.gmg_charge_density(self.h, C.c_int64(len(hh)), D(lo), D(hh), D(rlo), C.c_double(root_h), C.c_int64(len(q)),
                                            D(xyz), D(q), C.c_double(r_c), C.c_double(cutoff), C.c_int(1 if use_lists else 0),
                                            C.c_int(len(qp)), D(qp), None if out is None else D(out)))
        return out

    def charge_density_resident(self, origin, h0, atom_xyz, atom_q, r_c, cutoff, use_lists, quadrature_points, dens=True, n_cells=None, nq=None,
                                n_atoms=None):
        """rho [n_cells, nq] for the active cells of the resident mesh tables (gmg_charge_density_resident): (rho, device time in
        ms).  dens=None keeps the densities on the device and returns (None, ms).  None for an array passes NULL (with n_atoms /
        nq); n_cells: the cells of the tables when this view did not build them."""
        xyz = None if atom_xyz is None else np.ascontiguousarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
        q = None if atom_q is None else np.ascontiguousarray(atom_q, dtype=np.float64)
        qp = None if quadrature_points is None else np.ascontiguousarray(quadrature_points, dtype=np.float64).reshape(-1, 3)
        if n_atoms is None:
            n_atoms = len(q) if q is not None else len(xyz) if xyz is not None else 0
        if nq is None:
            nq = len(qp)
        D = lambda a: None if a is None else _p(a, C.c_double)
        out = None
        if dens is not None:
            if n_cells is None:
                n = [C.c_int64(0) for _ in range(5)]
                rc = self.L.gmg_get_mesh_tables(self.h, *[C.byref(v) for v in n], None, None, None, None, None, None, None, None)
                n_cells = n[0].value if rc == OK else 0
            out = np.zeros((int(n_cells), max(int(nq), 0)))
        ms = C.c_double(0)
        self._chk(self.L.gmg_charge_density_resident(self.h, C.c_double(origin), C.c_double(h0), C.c_int64(int(n_atoms)), D(xyz), D(q), C.c_double(r_c),
                                                     C.c_double(cutoff), C.c_int(1 if use_lists else 0), C.c_int(int(nq)), D(qp), D(out), C.byref(ms)))
        return out, ms.value

    def get_resident_cell_geometry(self, origin, h0, want=(True, True, True)):
        """(cell_lo [n_cells, 3], cell_h [n_cells], root_lo [n_cells, 3]) as gmg_charge_density_resident forms them from the
        resident mesh tables; want: which of the three to fetch (the others are None)"""
        n = [C.c_int64(0) for _ in range(5)]
        rc = self.L.gmg_get_mesh_tables(self.h, *[C.byref(v) for v in n], None, None, None, None, None, None, None, None)
        nc = n[0].value if rc == OK else 0
        lo = np.zeros((nc, 3)) if want[0] else None
        hh = np.zeros(nc) if want[1] else None
        rlo = np.zeros((nc, 3)) if want[2] else None
        D = lambda a: None if a is None else _p(a, C.c_double)
        self._chk(self.L.gmg_get_resident_cell_geometry(self.h, C.c_double(origin), C.c_double(h0), D(lo), D(hh), D(rlo)))
        return lo, hh, rlo

    def get_charge_density(self, n_cells, nq):
        """the densities charge_density(..., dens=None) left on the device: [n_cells, nq]"""
        out = np.zeros((int(n_cells), int(nq)))
        self._chk(self.L.gmg_get_charge_density(self.h, C.c_int64(n_cells), C.c_int(nq), _p(out, C.c_double)))
        return out

    def rhs_assemble(self, n_cells, dim, shape, weight, cell_level, jxw_of_level, term_slot, term_value, dof_ptr, entry_slot,
                     entry_coef, coef_table, rhs):
        """rhs (DeviceVector of len(dof_ptr) - 1 entries) from the densities kept on the device; shape [nq, 2^dim]."""
        w = np.ascontiguousarray(weight, dtype=np.float64)
        sh = np.ascontiguousarray(shape, dtype=np.float64).reshape(len(w), 1 << dim)
        lv = np.ascontiguousarray(cell_level, dtype=np.uint8)
        jxw = np.ascontiguousarray(jxw_of_level, dtype=np.float64)
        ts = np.ascontiguousarray(term_slot, dtype=np.int32)
        tv = np.ascontiguousarray(term_value, dtype=np.float64)
        ptr = np.ascontiguousarray(dof_ptr, dtype=np.int64)
        es = np.ascontiguousarray(entry_slot, dtype=np.int32)
        ec = np.ascontiguousarray(entry_coef, dtype=np.uint8)
        ct = np.ascontiguousarray(coef_table, dtype=np.float64)
        assert len(jxw) == 16 and len(ct) == 256 and len(ts) == len(tv) and len(es) == len(ec) and len(ptr) >= 1
        D = lambda a: _p(a, C.c_double)
        self._chk(self.L.gmg_rhs_assemble(self.h, C.c_int64(n_cells), C.c_int(len(w)), C.c_int(dim), D(sh), D(w), _p(lv, C.c_uint8), D(jxw),
                                          C.c_int64(len(ts)), _p(ts, C.c_int32), D(tv), C.c_int64(len(ptr) - 1), _p(ptr, C.c_int64),
                                          _p(es, C.c_int32), _p(ec, C.c_uint8), D(ct), rhs.ptr))

    def assemble_system_matrix(self, dim, n_dofs, cell_dofs, cell_level, K_of_level, constraint_of_dof, line_ptr, line_master, line_weight,
                               validate=True):
        """The active-mesh system matrix formed on the device (gmg_assemble_system_matrix); returns the device time in ms.
        cell_dofs [n_cells, 2^dim], cell_level [n_cells], K_of_level [16, 2^dim, 2^dim], constraint_of_dof [n_dofs], the lines
        in CSR form (line_ptr [n_lines + 1]; None or empty: no lines).  validate=True checks the shapes here (ValueError)
        before the library sees them; the library checks the contents."""
        nv = 1 << int(dim) if dim in (2, 3) else 0
        cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
        lv = np.ascontiguousarray(cell_level, dtype=np.uint8)
        K = np.ascontiguousarray(K_of_level, dtype=np.float64)
        cons = np.ascontiguousarray(constraint_of_dof, dtype=np.int32)
        lp = np.ascontiguousarray([] if line_ptr is None else line_ptr, dtype=np.int64)
        lm = np.ascontiguousarray([] if line_master is None else line_master, dtype=np.int32)
        lw = np.ascontiguousarray([] if line_weight is None else line_weight, dtype=np.float64)
        n_cells, n_lines = len(lv), max(len(lp) - 1, 0)
        if validate:
            if nv == 0:
                raise ValueError("assemble_system_matrix: dim must be 2 or 3")
            if n_dofs < 0 or cons.size != n_dofs:
                raise ValueError("assemble_system_matrix: constraint_of_dof must have n_dofs entries")
            if cd.size != n_cells * nv:
                raise ValueError("assemble_system_matrix: cell_dofs must be [n_cells, 2^dim]")
            if K.size != 16 * nv * nv:
                raise ValueError("assemble_system_matrix: K_of_level must be [16, 2^dim, 2^dim]")
            if len(lm) != len(lw) or (n_lines and len(lm) < lp[-1]) or (not n_lines and len(lm)):
                raise ValueError("assemble_system_matrix: line_master / line_weight do not match line_ptr")
        opt = lambda a, t: _p(a, t) if a.size else None
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_system_matrix(self.h, C.c_int(int(dim)), C.c_int64(int(n_dofs)), C.c_int64(n_cells), opt(cd, C.c_int32),
                                                    opt(lv, C.c_uint8), opt(K, C.c_double), opt(cons, C.c_int32), C.c_int64(n_lines),
                                                    opt(lp, C.c_int64), opt(lm, C.c_int32), opt(lw, C.c_double), C.byref(ms)))
        self.n_system = int(n_dofs)
        return ms.value

    def assemble_rhs(self, inp, rhs, source=True, K_of_level=True):
        """The right-hand side formed on the device from the cell tables (gmg_assemble_rhs) into rhs (DeviceVector of inp.n_dofs
        entries); returns the device time in ms.  inp: the fields of Problem.rhs_assembly_inputs() (dim, n_dofs, cell_dofs
        [n_cells, 2^dim], cell_level, constraint_of_dof, line_ptr, line_master, line_weight, line_inhomogeneity, K_of_level, nq,
        shape [nq, 2^dim], weight, jxw_of_level, source [n_cells, nq]).  source=None passes NULL: the densities
        charge_density(..., dens=None) left on the device; K_of_level=None passes NULL.  Arrays of length 0 are passed as NULL;
        the library checks everything."""
        i32, u8, f64 = (lambda a, t=t: np.ascontiguousarray([] if a is None else a, dtype=t) for t in (np.int32, np.uint8, np.float64))
        cd, lv, cons = i32(inp.cell_dofs), u8(inp.cell_level), i32(inp.constraint_of_dof)
        lp, lm = np.ascontiguousarray([] if inp.line_ptr is None else inp.line_ptr, dtype=np.int64), i32(inp.line_master)
        lw, li = f64(inp.line_weight), f64(inp.line_inhomogeneity)
        K = f64(inp.K_of_level if K_of_level is True else K_of_level)
        sh, w, jxw = f64(inp.shape), f64(inp.weight), f64(inp.jxw_of_level)
        src = f64(inp.source if source is True else source)
        opt = lambda a, t: _p(a, t) if a.size else None
        D = lambda a: opt(a, C.c_double)
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_rhs(self.h, C.c_int(int(inp.dim)), C.c_int64(int(inp.n_dofs)), C.c_int64(len(lv)), opt(cd, C.c_int32),
                                          opt(lv, C.c_uint8), opt(cons, C.c_int32), C.c_int64(max(len(lp) - 1, 0)), opt(lp, C.c_int64),
                                          opt(lm, C.c_int32), D(lw), D(li), D(K), C.c_int(int(inp.nq)), D(sh), D(w), D(jxw), D(src),
                                          None if rhs is None else rhs.ptr, C.byref(ms)))
        return ms.value

    def distribute_constraints(self, u, constraint_of_dof, line_ptr, line_master, line_weight, line_inhomogeneity):
        """constraints.distribute in place on the DeviceVector u (gmg_distribute_constraints)."""
        cons = np.ascontiguousarray(constraint_of_dof, dtype=np.int32)
        lp = np.ascontiguousarray([] if line_ptr is None else line_ptr, dtype=np.int64)
        lm = np.ascontiguousarray([] if line_master is None else line_master, dtype=np.int32)
        lw = np.ascontiguousarray([] if line_weight is None else line_weight, dtype=np.float64)
        li = np.ascontiguousarray([] if line_inhomogeneity is None else line_inhomogeneity, dtype=np.float64)
        opt = lambda a, t: _p(a, t) if a.size else None
        self._chk(self.L.gmg_distribute_constraints(self.h, C.c_int64(u.n), u.ptr, opt(cons, C.c_int32), C.c_int64(max(len(lp) - 1, 0)),
                                                    opt(lp, C.c_int64), opt(lm, C.c_int32), opt(lw, C.c_double), opt(li, C.c_double)))

    def assemble_system_matrix_coef(self, dim, n_dofs, cell_dofs, cell_level, nq, cell_coef, G, qw, scale_of_level, constraint_of_dof, line_ptr,
                                    line_master, line_weight, validate=True):
        """The active-mesh system matrix of a variable coefficient formed on the device (gmg_assemble_system_matrix_coef);
        returns the device time in ms.  As assemble_system_matrix with, instead of K_of_level, nq, cell_coef [n_cells, nq], G
        [nq, 2^dim, 2^dim], qw [nq] and scale_of_level [16].  validate=True checks the shapes here (ValueError) before the
        library sees them; the library checks the contents."""
        nv = 1 << int(dim) if dim in (2, 3) else 0
        cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
        lv = np.ascontiguousarray(cell_level, dtype=np.uint8)
        cc, g, w, sc = (np.ascontiguousarray([] if a is None else a, dtype=np.float64) for a in (cell_coef, G, qw, scale_of_level))
        cons = np.ascontiguousarray(constraint_of_dof, dtype=np.int32)
        lp = np.ascontiguousarray([] if line_ptr is None else line_ptr, dtype=np.int64)
        lm = np.ascontiguousarray([] if line_master is None else line_master, dtype=np.int32)
        lw = np.ascontiguousarray([] if line_weight is None else line_weight, dtype=np.float64)
        n_cells, n_lines = len(lv), max(len(lp) - 1, 0)
        if validate:
            if nv == 0:
                raise ValueError("assemble_system_matrix_coef: dim must be 2 or 3")
            if n_dofs < 0 or cons.size != n_dofs:
                raise ValueError("assemble_system_matrix_coef: constraint_of_dof must have n_dofs entries")
            if cd.size != n_cells * nv:
                raise ValueError("assemble_system_matrix_coef: cell_dofs must be [n_cells, 2^dim]")
            if not 1 <= nq <= 64 or cc.size != n_cells * nq or g.size != nq * nv * nv or w.size != nq or sc.size != 16:
                raise ValueError("assemble_system_matrix_coef: nq in 1 .. 64, cell_coef [n_cells, nq], G [nq, 2^dim, 2^dim], qw [nq], scale_of_level [16]")
            if len(lm) != len(lw) or (n_lines and len(lm) < lp[-1]) or (not n_lines and len(lm)):
                raise ValueError("assemble_system_matrix_coef: line_master / line_weight do not match line_ptr")
        opt = lambda a, t: _p(a, t) if a.size else None
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_system_matrix_coef(self.h, C.c_int(int(dim)), C.c_int64(int(n_dofs)), C.c_int64(n_cells), opt(cd, C.c_int32),
                                                         opt(lv, C.c_uint8), C.c_int(int(nq)), opt(cc, C.c_double), opt(g, C.c_double),
                                                         opt(w, C.c_double), opt(sc, C.c_double), opt(cons, C.c_int32), C.c_int64(n_lines),
                                                         opt(lp, C.c_int64), opt(lm, C.c_int32), opt(lw, C.c_double), C.byref(ms)))
        self.n_system = int(n_dofs)
        return ms.value

    def get_system_matrix(self):
        """The CSR of the system matrix as the device holds it (after assemble_system_matrix)."""
        from types import SimpleNamespace
        nr, nz = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.gmg_get_system_matrix(self.h, C.byref(nr), C.byref(nz), None, None, None))
        rp = np.zeros(nr.value + 1, dtype=np.int64)
        col, val = np.zeros(max(nz.value, 1), dtype=np.int32), np.zeros(max(nz.value, 1))
        self._chk(self.L.gmg_get_system_matrix(self.h, C.byref(nr), C.byref(nz), _p(rp, C.c_int64), _p(col, C.c_int32), _p(val, C.c_double)))
        return SimpleNamespace(n_rows=nr.value, n_cols=nr.value, nnz=nz.value, rowptr=rp, col=col[:nz.value], val=val[:nz.value])

    def system_matrix_norms(self):
        """(l1, linf, frobenius) of the device's system matrix CSR"""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self.L.gmg_system_matrix_norms(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def assemble_level_matrix(self, level, dim, n_dofs, cell_dofs, K, dof_flags, validate=True):
        """A level matrix and its interface matrix formed on the device (gmg_assemble_level_matrix); returns the device time in
        ms.  cell_dofs [n_cells, 2^dim], K [2^dim, 2^dim], dof_flags [n_dofs] (bit 0 boundary, bit 1 refinement edge).
        validate=True checks the shapes here (ValueError) before the library sees them; the library checks the contents."""
        nv = 1 << int(dim) if dim in (2, 3) else 0
        cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
        k = np.ascontiguousarray(K, dtype=np.float64)
        fl = np.ascontiguousarray(dof_flags, dtype=np.uint8)
        if validate:
            if nv == 0:
                raise ValueError("assemble_level_matrix: dim must be 2 or 3")
            if cd.size % nv or (cd.ndim == 2 and cd.shape[1] != nv):
                raise ValueError("assemble_level_matrix: cell_dofs must be [n_cells, 2^dim]")
            if k.size != nv * nv:
                raise ValueError("assemble_level_matrix: K must be [2^dim, 2^dim]")
            if n_dofs < 0 or fl.size != n_dofs:
                raise ValueError("assemble_level_matrix: dof_flags must have n_dofs entries")
        n_cells = cd.size // nv if nv else len(cd)
        opt = lambda a, t: _p(a, t) if a.size else None
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_level_matrix(self.h, C.c_int(int(level)), C.c_int(int(dim)), C.c_int64(int(n_dofs)), C.c_int64(n_cells),
                                                   opt(cd, C.c_int32), opt(k, C.c_double), opt(fl, C.c_uint8), C.byref(ms)))
        return ms.value

    def assemble_level_matrix_coef(self, level, dim, n_dofs, cell_dofs, nq, cell_coef, G, qw, scale, dof_flags, validate=True):
        """A level matrix and its interface matrix of a variable coefficient formed on the device
        (gmg_assemble_level_matrix_coef); returns the device time in ms.  As assemble_level_matrix with, instead of K, nq,
        cell_coef [n_cells, nq], G [nq, 2^dim, 2^dim], qw [nq] and one scale.  validate=True checks the shapes here (ValueError)
        before the library sees them; the library checks the contents."""
        nv = 1 << int(dim) if dim in (2, 3) else 0
        cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
        cc, g, w = (np.ascontiguousarray([] if a is None else a, dtype=np.float64) for a in (cell_coef, G, qw))
        fl = np.ascontiguousarray(dof_flags, dtype=np.uint8)
        n_cells = cd.size // nv if nv else len(cd)
        if validate:
            if nv == 0:
                raise ValueError("assemble_level_matrix_coef: dim must be 2 or 3")
            if cd.size % nv or (cd.ndim == 2 and cd.shape[1] != nv):
                raise ValueError("assemble_level_matrix_coef: cell_dofs must be [n_cells, 2^dim]")
            if not 1 <= nq <= 64 or cc.size != n_cells * nq or g.size != nq * nv * nv or w.size != nq:
                raise ValueError("assemble_level_matrix_coef: nq in 1 .. 64, cell_coef [n_cells, nq], G [nq, 2^dim, 2^dim], qw [nq]")
            if n_dofs < 0 or fl.size != n_dofs:
                raise ValueError("assemble_level_matrix_coef: dof_flags must have n_dofs entries")
        opt = lambda a, t: _p(a, t) if a.size else None
        ms = C.c_double(0)
        self._chk(self.L.gmg_assemble_level_matrix_coef(self.h, C.c_int(int(level)), C.c_int(int(dim)), C.c_int64(int(n_dofs)), C.c_int64(n_cells),
                                                        opt(cd, C.c_int32), C.c_int(int(nq)), opt(cc, C.c_double), opt(g, C.c_double),
                                                        opt(w, C.c_double), C.c_double(float(scale)), opt(fl, C.c_uint8), C.byref(ms)))
        return ms.value

    def get_level_matrix(self, level, which=LEVEL_A):
        """The CSR of a level's operator as the device holds it (gmg_get_level_matrix): which = LEVEL_A, LEVEL_EDGE or
        LEVEL_EDGE_T; an absent interface matrix comes back with nnz 0."""
        from types import SimpleNamespace
        nr, nc, nz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.gmg_get_level_matrix(self.h, C.c_int(level), C.c_int(which), C.byref(nr), C.byref(nc), C.byref(nz), None, None, None))
        rp = np.zeros(nr.value + 1, dtype=np.int64)
        col, val = np.zeros(max(nz.value, 1), dtype=np.int32), np.zeros(max(nz.value, 1))
        self._chk(self.L.gmg_get_level_matrix(self.h, C.c_int(level), C.c_int(which), C.byref(nr), C.byref(nc), C.byref(nz),
                                              _p(rp, C.c_int64), _p(col, C.c_int32), _p(val, C.c_double)))
        return SimpleNamespace(n_rows=nr.value, n_cols=nc.value, nnz=nz.value, rowptr=rp, col=col[:nz.value], val=val[:nz.value])

    def estimate_error(self, dim, cell_dofs, cell_level, face_kind, face_cell, h_of_level, face_measure_of_level, diameter_of_level,
                       gauss_x, gauss_w, u, residual=0, weight=None, jxw_of_level=None, dens=None, fraction=0.6, n_u=None, validate=True):
        """The error estimator and the refinement marks formed on the device (gmg_estimate_error): namespace(eta [n_cells]
        float32, kelly_sq, residual_sq [n_cells], face_int [n_cells, 2 dim], threshold, mark [n_cells] uint8, n_marked,
        build_ms).  u: a DeviceVector with the constraint-distributed solution; dens: [n_cells, nq] host array, or None for
        the densities charge_density(..., dens=None) left on the device (nq = len(weight)).  validate=True checks the shapes
        here (ValueError) before the library sees them; the library checks the contents."""
        from types import SimpleNamespace
        ok = dim in (2, 3)
        nv, nfc, nf = (1 << int(dim), 1 << (int(dim) - 1), 2 * int(dim)) if ok else (8, 4, 6)
        cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
        lv = np.ascontiguousarray(cell_level, dtype=np.uint8)
        fk = np.ascontiguousarray(face_kind, dtype=np.uint8)
        fc = np.ascontiguousarray(face_cell, dtype=np.int32)
        tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in (h_of_level, face_measure_of_level, diameter_of_level)]
        gx, gw = np.ascontiguousarray(gauss_x, dtype=np.float64), np.ascontiguousarray(gauss_w, dtype=np.float64)
        w = np.ascontiguousarray([] if weight is None else weight, dtype=np.float64)
        jxw = np.ascontiguousarray([] if jxw_of_level is None else jxw_of_level, dtype=np.float64)
        de = None if dens is None else np.ascontiguousarray(dens, dtype=np.float64)
        n_cells, nq = len(lv), len(w)
        if validate:
            if not ok:
                raise ValueError("estimate_error: dim must be 2 or 3")
            if cd.size != n_cells * nv or fk.size != n_cells * nf or fc.size != n_cells * nf * nfc:
                raise ValueError("estimate_error: cell_dofs / face_kind / face_cell do not match cell_level")
            if any(t.size != 16 for t in tabs) or (residual and jxw.size != 16):
                raise ValueError("estimate_error: the per-level tables have 16 entries")
            if len(gx) != len(gw):
                raise ValueError("estimate_error: gauss_x / gauss_w differ in length")
            if de is not None and de.size != n_cells * nq:
                raise ValueError("estimate_error: dens must be [n_cells, nq]")
        eta, mark = np.zeros(n_cells, dtype=np.float32), np.zeros(n_cells, dtype=np.uint8)
        ksq, rsq, fi = np.zeros(n_cells), np.zeros(n_cells), np.zeros((n_cells, nf))
        thr, ms, nm = C.c_double(0), C.c_double(0), C.c_int64(0)
        opt = lambda a, t: _p(a, t) if a is not None and a.size else None
        D = C.c_double
        self._chk(self.L.gmg_estimate_error(self.h, C.c_int(int(dim)), C.c_int64(n_cells), opt(cd, C.c_int32), opt(lv, C.c_uint8), opt(fk, C.c_uint8),
                                            opt(fc, C.c_int32), opt(tabs[0], D), opt(tabs[1], D), opt(tabs[2], D), C.c_int(len(gx)), opt(gx, D),
                                            opt(gw, D), u.ptr if u is not None else None, C.c_int64(int(u.n if n_u is None else n_u) if u is not None else 0),
                                            C.c_int(int(residual)), C.c_int(nq), opt(w, D), opt(jxw, D), opt(de, D), C.c_double(fraction),
                                            opt(eta, C.c_float), opt(ksq, D), opt(rsq, D), opt(fi, D), C.byref(thr), opt(mark, C.c_uint8),
                                            C.byref(nm), C.byref(ms)))
        return SimpleNamespace(eta=eta, kelly_sq=ksq, residual_sq=rsq, face_int=fi, threshold=thr.value, mark=mark, n_marked=nm.value,
                               build_ms=ms.value)

    # ---- the end of a cycle on the resident mesh tables: face table, estimator and marks, refinement, error norm
    def _mesh_sizes(self):
        """(n_cells, n_dofs) of the resident mesh tables, (0, 0) when the context holds none"""
        n = [C.c_int64(0) for _ in range(5)]
        rc = self.L.gmg_get_mesh_tables(self.h, *[C.byref(v) for v in n], None, None, None, None, None, None, None, None)
        return (n[0].value, n[1].value) if rc == OK else (0, 0)

    def build_face_table_resident(self, dim, n0, level_ptr, cell_coord, cell_first_child, n_levels=None):
        """gmg_build_face_table with the table kept in the context (gmg_build_face_table_resident; get_face_table copies it
        out): namespace(n_active, build_ms)"""
        from types import SimpleNamespace
        args, keep = self._forest_args(dim, n0, level_ptr, cell_coord, cell_first_child, n_levels)
        na, ms = C.c_int64(0), C.c_double(0)
        self._chk(self.L.gmg_build_face_table_resident(self.h, *args, C.byref(na), C.byref(ms)))
        return SimpleNamespace(n_active=na.value, build_ms=ms.value)

    def get_face_table(self, dim=None):
        """The kept face table as numpy arrays: namespace(n_active, face_kind [n_active, 2 dim], face_cell [n_active, 2 dim,
        2^(dim-1)])"""
        from types import SimpleNamespace
        na = C.c_int64(0)
        self._chk(self.L.gmg_get_face_table(self.h, C.byref(na), None, None))
        dim = self._mesh_dim(dim)
        fk, fcell = np.zeros((na.value, 2 * dim), dtype=np.uint8), np.zeros((na.value, 2 * dim, 1 << (dim - 1)), dtype=np.int32)
        self._chk(self.L.gmg_get_face_table(self.h, C.byref(na), _p(fk, C.c_uint8) if fk.size else None, _p(fcell, C.c_int32) if fcell.size else None))
        return SimpleNamespace(n_active=na.value, face_kind=fk, face_cell=fcell)

    # ---- energy and forces at the atoms on the resident mesh tables
    def build_point_locator_resident(self, dim, n0, level_ptr, cell_coord, cell_first_child, n_levels=None):
        """The node array of set_point_locator formed on the device from the forest the tables were built from and kept in the
        context next to them (gmg_build_point_locator_resident; get_point_locator copies it out): namespace(n_nodes, build_ms)"""
        from types import SimpleNamespace
        args, keep = self._forest_args(dim, n0, level_ptr, cell_coord, cell_first_child, n_levels)
        nn, ms = C.c_int64(0), C.c_double(0)
        self._chk(self.L.gmg_build_point_locator_resident(self.h, *args, C.byref(nn), C.byref(ms)))
        return SimpleNamespace(n_nodes=nn.value, build_ms=ms.value)

    def get_point_locator(self):
        """The kept node array [cells of all levels] (int32)"""
        nn = C.c_int64(0)
        self._chk(self.L.gmg_get_point_locator(self.h, C.byref(nn), None))
        node = np.zeros(nn.value, dtype=np.int32)
        self._chk(self.L.gmg_get_point_locator(self.h, C.byref(nn), _p(node, C.c_int32) if node.size else None))
        return node

    def atom_forces_resident(self, origin, h0, xyz, q, u, r_c, cutoff=0.0, n_u=None):
        """atom_forces on the resident locator and the tables' cell_dofs (gmg_atom_forces_resident): the same dict"""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(q, dtype=np.float64)
        n = len(q)
        out = dict(phi=np.zeros(n), field=np.zeros((n, 3)), force=np.zeros((n, 3)), force_short=np.zeros((n, 3)), e_short=np.zeros(n))
        D = lambda a: _p(a, C.c_double) if a.size else None
        self._chk(self.L.gmg_atom_forces_resident(self.h, C.c_double(origin), C.c_double(h0), C.c_int64(n), D(xyz), D(q), u.ptr if u is not None else None,
                                                  C.c_int64(int((u.n if u is not None else 0) if n_u is None else n_u)), C.c_double(r_c), C.c_double(cutoff),
                                                  D(out["phi"]), D(out["field"]), D(out["force"]), D(out["force_short"]), D(out["e_short"])))
        return out

    def electrostatic_energy_resident(self, origin, h0, xyz, q, u, r_c, cutoff=0.0, n_u=None):
        """The three ascending sums of the electrostatic energy formed on the device (gmg_electrostatic_energy_resident):
        namespace(short, fe_long, self_energy, build_ms)"""
        from types import SimpleNamespace
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(q, dtype=np.float64)
        D = lambda a: _p(a, C.c_double) if a.size else None
        out, ms = np.zeros(3), C.c_double(0)
        self._chk(self.L.gmg_electrostatic_energy_resident(self.h, C.c_double(origin), C.c_double(h0), C.c_int64(len(q)), D(xyz), D(q),
                                                           u.ptr if u is not None else None,
                                                           C.c_int64(int((u.n if u is not None else 0) if n_u is None else n_u)), C.c_double(r_c),
                                                           C.c_double(cutoff), _p(out, C.c_double), C.byref(ms)))
        return SimpleNamespace(short=out[0], fe_long=out[1], self_energy=out[2], build_ms=ms.value)

    def estimate_error_resident(self, h_of_level, face_measure_of_level, diameter_of_level, gauss_x, gauss_w, u, residual=0, weight=None,
                                jxw_of_level=None, dens=None, fraction=0.6, n_u=None, dim=None):
        """gmg_estimate_error on the resident mesh tables and the kept face table (gmg_estimate_error_resident): the namespace
        of estimate_error.  The marks also stay in the context (get_marks, refine_forest_marked)."""
        from types import SimpleNamespace
        n_cells, _ = self._mesh_sizes()
        dim = getattr(self, "mesh_dim", 3) if dim is None else dim
        nf = 2 * int(dim)
        tabs = [np.ascontiguousarray([] if t is None else t, dtype=np.float64) for t in (h_of_level, face_measure_of_level, diameter_of_level)]
        gx = np.ascontiguousarray([] if gauss_x is None else gauss_x, dtype=np.float64)
        gw = np.ascontiguousarray([] if gauss_w is None else gauss_w, dtype=np.float64)
        w = np.ascontiguousarray([] if weight is None else weight, dtype=np.float64)
        jxw = np.ascontiguousarray([] if jxw_of_level is None else jxw_of_level, dtype=np.float64)
        de = None if dens is None else np.ascontiguousarray(dens, dtype=np.float64)
        eta, mark = np.zeros(n_cells, dtype=np.float32), np.zeros(n_cells, dtype=np.uint8)
        ksq, rsq, fi = np.zeros(n_cells), np.zeros(n_cells), np.zeros((n_cells, nf))
        thr, ms, nm = C.c_double(0), C.c_double(0), C.c_int64(0)
        opt = lambda a, t: _p(a, t) if a is not None and a.size else None
        D = C.c_double
        self._chk(self.L.gmg_estimate_error_resident(self.h, opt(tabs[0], D), opt(tabs[1], D), opt(tabs[2], D), C.c_int(len(gx)), opt(gx, D), opt(gw, D),
                                                     u.ptr if u is not None else None,
                                                     C.c_int64(int(u.n if n_u is None else n_u) if u is not None else int(n_u or 0)),
                                                     C.c_int(int(residual)), C.c_int(len(w)), opt(w, D), opt(jxw, D), opt(de, D), C.c_double(fraction),
                                                     opt(eta, C.c_float), opt(ksq, D), opt(rsq, D), opt(fi, D), C.byref(thr), opt(mark, C.c_uint8),
                                                     C.byref(nm), C.byref(ms)))
        return SimpleNamespace(eta=eta, kelly_sq=ksq, residual_sq=rsq, face_int=fi, threshold=thr.value, mark=mark, n_marked=nm.value,
                               build_ms=ms.value)

    def get_marks(self):
        """The marks the last estimate_error_resident kept: namespace(n_cells, mark [n_cells] uint8, n_marked)"""
        from types import SimpleNamespace
        nc, nm = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.gmg_get_marks(self.h, C.byref(nc), None, C.byref(nm)))
        mark = np.zeros(nc.value, dtype=np.uint8)
        self._chk(self.L.gmg_get_marks(self.h, C.byref(nc), _p(mark, C.c_uint8) if mark.size else None, C.byref(nm)))
        return SimpleNamespace(n_cells=nc.value, mark=mark, n_marked=nm.value)

    def refine_forest_marked(self, dim, n0, level_ptr, cell_coord, cell_first_child, n_levels=None):
        """refine_forest with the flags formed on the device from the kept marks (gmg_refine_forest_marked)"""
        from types import SimpleNamespace
        args, keep = self._forest_args(dim, n0, level_ptr, cell_coord, cell_first_child, n_levels)
        nl, nc, ns, ms = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        self._chk(self.L.gmg_refine_forest_marked(self.h, *args, C.byref(nl), C.byref(nc), C.byref(ns), C.byref(ms)))
        return SimpleNamespace(n_levels=nl.value, n_cells=nc.value, n_split=ns.value, build_ms=ms.value)

    def energy_norm_error_resident(self, origin, h0, u, atom_xyz, atom_q, r_c, quadrature_points, weights, shape_grad, n_u=None):
        """energy_norm_error on the resident mesh tables (gmg_energy_norm_error_resident) -> (error, cell_err2 [n_cells])."""
        n_cells, _ = self._mesh_sizes()
        xyz = np.ascontiguousarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(atom_q, dtype=np.float64)
        qp = np.ascontiguousarray(quadrature_points, dtype=np.float64).reshape(-1, 3)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        sg = np.ascontiguousarray(shape_grad, dtype=np.float64).reshape(len(w), 8, 3)
        err, ce = C.c_double(0), np.zeros(n_cells)
        D = lambda a: _p(a, C.c_double) if a.size else None
        self._chk(self.L.gmg_energy_norm_error_resident(self.h, C.c_double(origin), C.c_double(h0), u.ptr, C.c_int64(u.n if n_u is None else int(n_u)),
                                                        C.c_int64(len(q)), D(xyz), D(q), C.c_double(r_c), C.c_int(len(w)), D(qp), D(w), D(sg),
                                                        C.byref(err), D(ce)))
        return err.value, ce

    # ---- the patches of the graphical output
    def _output_patches(self, call, n_cells, nv, n_dofs, u, n_u, fields, want):
        from types import SimpleNamespace
        D = C.c_double
        n_slots = n_cells * nv
        fs = [None if f is None else np.ascontiguousarray(f, dtype=np.float64) for f in (fields or [])]
        out = dict(point=np.zeros((n_slots, 3)), solution=np.zeros(n_slots), grad_phi=np.zeros((n_slots, 3)))
        pf = [np.zeros(n_slots) for _ in fs]
        want = tuple(out) + ("patch_field",) if want is None else want
        ptr = lambda a: _p(a, D) if a is not None and a.size else None
        fin = (C.POINTER(D) * max(len(fs), 1))(*[ptr(f) for f in fs]) if fs else None
        fout = (C.POINTER(D) * max(len(fs), 1))(*[ptr(f) for f in pf]) if fs and "patch_field" in want else None
        ms = C.c_double(0)
        self._chk(call(u.ptr if u is not None else None, C.c_int64(int((u.n if u is not None else 0) if n_u is None else n_u)), C.c_int(len(fs)), fin,
                       *[ptr(out[k]) if k in want else None for k in ("point", "solution", "grad_phi")], fout, C.byref(ms)))
        return SimpleNamespace(point=out["point"], solution=out["solution"], grad_phi=out["grad_phi"], patch_field=pf, build_ms=ms.value)

    def output_patches(self, dim, cell_dofs, cell_level, vertex_of_dof, origin, h0, u, fields=None, n_u=None, n_dofs=None, want=None):
        """One patch per active cell with 2^dim vertices formed on the device (gmg_output_patches): namespace(point [n_slots, 3],
        solution [n_slots], grad_phi [n_slots, 3], patch_field [one [n_slots] per field], build_ms).  u: a DeviceVector;
        fields: up to 8 host vectors [n_dofs]; want: the names of the outputs to ask for (the others are passed as NULL and
        come back 0), None for all."""
        nv = 1 << int(dim) if dim in (2, 3) else 8
        cd = None if cell_dofs is None else np.ascontiguousarray(cell_dofs, dtype=np.int32)
        lv = None if cell_level is None else np.ascontiguousarray(cell_level, dtype=np.uint8)
        vk = None if vertex_of_dof is None else np.ascontiguousarray(vertex_of_dof, dtype=np.uint64)
        n_cells = 0 if lv is None else len(lv)
        n_dofs = (0 if vk is None else len(vk)) if n_dofs is None else int(n_dofs)
        opt = lambda a, t: _p(a, t) if a is not None and a.size else None
        call = lambda *rest: self.L.gmg_output_patches(self.h, C.c_int(int(dim)), C.c_int64(n_cells), opt(cd, C.c_int32), opt(lv, C.c_uint8),
                                                       opt(vk, C.c_uint64), C.c_int64(n_dofs), C.c_double(origin), C.c_double(h0), *rest)
        return self._output_patches(call, n_cells, nv, n_dofs, u, n_u, fields, want)

    def output_patches_resident(self, origin, h0, u, fields=None, n_u=None, want=None, dim=None):
        """output_patches on the resident mesh tables (gmg_output_patches_resident): the same namespace"""
        n_cells, n_dofs = self._mesh_sizes()
        call = lambda *rest: self.L.gmg_output_patches_resident(self.h, C.c_double(origin), C.c_double(h0), *rest)
        dim = getattr(self, "mesh_dim", 3) if dim is None else dim  # (without tables the library refuses the call itself)
        return self._output_patches(call, n_cells, 1 << int(dim), n_dofs, u, n_u, fields, want)

    def synchronize(self):
        self._chk(self.L.gmg_synchronize(self.h))

    # ---- distributed
    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        rc = load().gmg_comm_unique_id(buf)
        if rc != OK:
            raise GMGError(rc, "gmg_comm_unique_id failed")
        return buf.raw

    def comm_init(self, rank, n_ranks, uid: bytes):
        buf = C.create_string_buffer(uid, UNIQUE_ID_BYTES)
        self._chk(self.L.gmg_comm_init(self.h, C.c_int(rank), C.c_int(n_ranks), buf))

    def comm_barrier(self):
        """the ranks meet on the host: when the operators are set, before the first solve (gmg_comm_barrier)"""
        self._chk(self.L.gmg_comm_barrier(self.h))

    def comm_info(self) -> dict:
        out = (C.c_int64 * 8)()
        self._chk(self.L.gmg_comm_info(self.h, out))
        return {"ranks": int(out[0]), "transport": {0: "none", 1: "rccl", 2: "peer"}[int(out[1])], "mailbox_finegrained": bool(out[2]),
                "ring_memory": {-1: "not allocated", 0: "hipMalloc (coarse-grained)", 1: "fine-grained"}[int(out[3])],
                "devices": int(out[4]), "level0_partitioned": bool(out[5])}

    def set_global_sizes(self, n_system, n_level0):
        self._chk(self.L.gmg_set_global_sizes(self.h, C.c_int64(n_system), C.c_int64(n_level0)))

    def allgather(self, n_global, dst_full, src_local):
        self._chk(self.L.gmg_vec_allgather(self.h, C.c_int64(n_global), dst_full.ptr, src_local.ptr))

    def set_halo_plan(self, which, neighbor_rank, send_count, send_idx, recv_count):
        nr = np.ascontiguousarray(neighbor_rank, dtype=np.int32)
        sc = np.ascontiguousarray(send_count, dtype=np.int32)
        si = np.ascontiguousarray(send_idx, dtype=np.int32)
        rc_ = np.ascontiguousarray(recv_count, dtype=np.int32)
        self._chk(self.L.gmg_set_halo_plan(self.h, C.c_int(which), C.c_int(len(nr)), _p(nr, C.c_int32), _p(sc, C.c_int32),
                                           _p(si, C.c_int32), _p(rc_, C.c_int32)))

    # ---- measurement
    def stats(self) -> Stats:
        s = Stats()
        self._chk(self.L.gmg_stats_get(self.h, C.byref(s)))
        return s

    def stats_reset(self):
        self._chk(self.L.gmg_stats_reset(self.h))

    def set_profiling(self, every):
        self._chk(self.L.gmg_set_profiling(self.h, C.c_int(every)))

    def calibrate_hbm(self, n_bytes=1 << 30, reps=10):
        r, c = C.c_double(0), C.c_double(0)
        self._chk(self.L.gmg_calibrate_hbm(self.h, C.c_int64(n_bytes), C.c_int(reps), C.byref(r), C.byref(c)))
        return r.value, c.value

    def set_tuning(self, coarse_chunk=0, cg_variant=0, ssor_blocks=0):
        self._chk(self.L.gmg_set_tuning(self.h, C.c_int(coarse_chunk), C.c_int(cg_variant)))
        if ssor_blocks:
            self._chk(self.L.gmg_set_ssor_blocks(self.h, C.c_int(ssor_blocks)))

    def set_option(self, key: str, value: float = 1.0):
        """Diagnostic / measurement options by name (include/gmg_coulomb.h: gmg_set_option)."""
        self._chk(self.L.gmg_set_option(self.h, key.encode(), C.c_double(value)))

    def set_ssor_block_rows(self, level, block_row):
        """Explicit SSOR block boundaries of one level (n_blocks + 1 entries; an empty list clears them)."""
        b = np.ascontiguousarray(block_row, dtype=np.int64)
        n_blocks = max(len(b) - 1, 0)
        self._chk(self.L.gmg_set_ssor_block_rows(self.h, C.c_int(level), C.c_int(n_blocks), _p(b, C.c_int64) if len(b) else None))

    def set_ssor_partition(self, kind):
        self._chk(self.L.gmg_set_ssor_partition(self.h, C.c_int(kind)))

    def get_ssor_partition(self, level):
        """(block_row, block_steps) of the level's SSOR plan."""
        nb = C.c_int(0)
        self._chk(self.L.gmg_get_ssor_partition(self.h, C.c_int(level), C.byref(nb), None, None))
        br, st = np.zeros(nb.value + 1, dtype=np.int64), np.zeros(max(nb.value, 1), dtype=np.int64)
        self._chk(self.L.gmg_get_ssor_partition(self.h, C.c_int(level), C.byref(nb), _p(br, C.c_int64), _p(st, C.c_int64)))
        return br, st[:nb.value]

    def get_ssor_plan(self, level):
        """gmg_get_ssor_plan as a dict (SSOR_PLAN_KEYS)."""
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.L.gmg_get_ssor_plan(self.h, C.c_int(level), _p(out, C.c_int64)))
        return dict(zip(SSOR_PLAN_KEYS, (int(v) for v in out)))

    def get_ssor_schedule(self, level):
        """gmg_get_ssor_schedule as a dict (SSOR_SCHEDULE_KEYS)."""
        out = np.zeros(4, dtype=np.int64)
        self._chk(self.L.gmg_get_ssor_schedule(self.h, C.c_int(level), _p(out, C.c_int64)))
        return dict(zip(SSOR_SCHEDULE_KEYS, (int(v) for v in out)))

    def get_ssor_backward_rows(self, level):
        """gmg_get_ssor_backward_rows: the level rows the self-contained backward records store to, in stream order."""
        cnt = C.c_int64(0)
        self._chk(self.L.gmg_get_ssor_backward_rows(self.h, C.c_int(level), C.byref(cnt), None))
        rows = np.zeros(max(cnt.value, 1), dtype=np.int32)
        self._chk(self.L.gmg_get_ssor_backward_rows(self.h, C.c_int(level), C.byref(cnt), _p(rows, C.c_int32)))
        return rows[:cnt.value]

    def get_ssor_plan_array(self, level, which):
        """gmg_get_ssor_plan_array: one array of the level's four-wave plan as raw bytes (which: a name of SSOR_PLAN_ARRAYS or its index)."""
        w = SSOR_PLAN_ARRAYS.index(which) if isinstance(which, str) else int(which)
        nbytes = C.c_int64(0)
        self._chk(self.L.gmg_get_ssor_plan_array(self.h, C.c_int(level), C.c_int(w), C.byref(nbytes), None))
        out = np.zeros(max(nbytes.value, 1), dtype=np.uint8)
        self._chk(self.L.gmg_get_ssor_plan_array(self.h, C.c_int(level), C.c_int(w), C.byref(nbytes), out.ctypes.data_as(C.c_void_p)))
        return out[:nbytes.value]

    def get_ssor_plan_origin(self, level):
        """gmg_get_ssor_plan_origin: (on_device, bytes of col / val downloaded for the plan, why the host built it or '')."""
        on_dev, moved, why = C.c_int(0), C.c_int64(0), C.c_char_p()
        self._chk(self.L.gmg_get_ssor_plan_origin(self.h, C.c_int(level), C.byref(on_dev), C.byref(moved), C.byref(why)))
        return bool(on_dev.value), int(moved.value), (why.value or b"").decode()


# gmg_get_ssor_plan_array: the values of GMG_SSOR_PLAN_* in order
SSOR_PLAN_ARRAYS = ("stream", "ranges", "blk_tab", "block_rng", "row_ci", "ci_row", "rpos_f", "rpos_b", "iso_diag", "iso_invd")
SSOR_PLAN_KEYS = ("forward_ranges", "backward_ranges", "self_contained_ranges", "y_slots", "max_live_forward", "max_live_backward", "steps", "stream_bytes")
SSOR_SCHEDULE_KEYS = ("packed", "levels", "steps_per_direction", "stage_steps")


def ssor_slot_plan(m, row_begin, row_end, backward, packed=False):
    """gmg_ssor_slot_plan on a host CSR (needs no device): (step, last_reader, slot, n_steps, n_slots) of one block and direction;
    the three arrays have one entry per row of the block, -1 for a row without couplings inside it.  packed: over the packed
    levels (gmg_ssor_slot_plan_packed) instead of the stages."""
    rp, col, val = _csr(m)
    n = len(rp) - 1
    k = max(int(row_end) - int(row_begin), 1)
    step, last, slot = (np.full(k, -1, dtype=np.int32) for _ in range(3))
    ns, nl = C.c_int64(0), C.c_int64(0)
    name = "gmg_ssor_slot_plan_packed" if packed else "gmg_ssor_slot_plan"
    rc = getattr(load(), name)(C.c_int64(n), _p(rp, C.c_int64), _p(col, C.c_int32), _p(val, C.c_double), C.c_int64(int(row_begin)), C.c_int64(int(row_end)),
                               C.c_int(int(bool(backward))), _p(step, C.c_int32), _p(last, C.c_int32), _p(slot, C.c_int32), C.byref(ns), C.byref(nl))
    if rc != OK:
        raise GMGError(rc, name)
    k = int(row_end) - int(row_begin)
    return step[:k], last[:k], slot[:k], ns.value, nl.value


def ssor_pack_levels(m, row_begin, row_end):
    """gmg_ssor_pack_levels on a host CSR (needs no device): (level per row of the block, -1 for a row without couplings inside
    it; number of levels; steps of a direction when the stages are walked 32 rows at a time)."""
    rp, col, val = _csr(m)
    n = len(rp) - 1
    k = int(row_end) - int(row_begin)
    level = np.full(max(k, 1), -1, dtype=np.int32)
    nl, ns = C.c_int64(0), C.c_int64(0)
    rc = load().gmg_ssor_pack_levels(C.c_int64(n), _p(rp, C.c_int64), _p(col, C.c_int32), _p(val, C.c_double), C.c_int64(int(row_begin)), C.c_int64(int(row_end)),
                                     _p(level, C.c_int32), C.byref(nl), C.byref(ns))
    if rc != OK:
        raise GMGError(rc, "gmg_ssor_pack_levels")
    return level[:k], nl.value, ns.value


def ssor_balance_rows(m, n_blocks, use_values=True):
    """gmg_ssor_balance_rows on a host CSR (needs no device): (block_row, modelled cost per block in us)."""
    rp, col, val = _csr(m)
    n = len(rp) - 1
    br, cost = np.zeros(n_blocks + 1, dtype=np.int64), np.zeros(n_blocks)
    rc = load().gmg_ssor_balance_rows(C.c_int64(n), _p(rp, C.c_int64), _p(col, C.c_int32), _p(val, C.c_double) if use_values else None,
                                      C.c_int(n_blocks), _p(br, C.c_int64), _p(cost, C.c_double))
    if rc != OK:
        raise GMGError(rc, "gmg_ssor_balance_rows")
    return br, cost


def coarse_direct_tables(n_cells):
    """gmg_coarse_direct_tables (needs no device): (S [m, m], lambda [m], mu [m]) of an axis with n_cells cells, m = n_cells - 1."""
    m = int(n_cells) - 1
    S, lam, mu = np.zeros((max(m, 1), max(m, 1))), np.zeros(max(m, 1)), np.zeros(max(m, 1))
    rc = load().gmg_coarse_direct_tables(C.c_int(int(n_cells)), _p(S, C.c_double), _p(lam, C.c_double), _p(mu, C.c_double))
    if rc != OK:
        raise GMGError(rc, "gmg_coarse_direct_tables")
    return S, lam, mu


def coarse_direct_separable(Ke):
    """gmg_coarse_direct_separable (needs no device): the scale s if Ke is the separable Q1 Laplacian cell matrix, else None."""
    ke = np.ascontiguousarray(Ke, dtype=np.float64).reshape(64)
    s = C.c_double(0)
    rc = load().gmg_coarse_direct_separable(_p(ke, C.c_double), C.byref(s))
    if rc == ERR_UNSUPPORTED:
        return None
    if rc != OK:
        raise GMGError(rc, "gmg_coarse_direct_separable")
    return s.value
