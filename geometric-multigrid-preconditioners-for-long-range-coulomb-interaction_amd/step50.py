"""ctypes binding of the host-side C++ (csrc/host/libstep50host.so): the mirror of the
reference's LaplaceProblem<dim> and main.cc.  Drives mesh/assembly on the CPU and the solve
on the MI355X through the C-ABI.  No CPU fallback for the solve."""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

from . import build as _build

_lib = None


class Report(C.Structure):
    _fields_ = [("cycle", C.c_int32), ("cg_iterations", C.c_int32), ("status", C.c_int32), ("has_energy", C.c_int32),
                ("n_levels", C.c_int32), ("pad", C.c_int32),
                ("active_cells", C.c_int64), ("dofs", C.c_int64), ("coarse_iterations", C.c_int64),
                ("dofs_by_level", C.c_int64 * 16),
                ("rhs_l1", C.c_double), ("rhs_l2", C.c_double), ("rhs_linf", C.c_double),
                ("matrix_l1", C.c_double), ("matrix_linf", C.c_double), ("matrix_frobenius", C.c_double),
                ("starting_value", C.c_double), ("convergence_value", C.c_double),
                ("sol_l1", C.c_double), ("sol_l2", C.c_double), ("sol_linf", C.c_double), ("refine_threshold", C.c_double),
                ("energy_analytical", C.c_double), ("energy_short", C.c_double), ("energy_fe_long", C.c_double),
                ("energy_self", C.c_double), ("energy_total", C.c_double), ("energy_abs_error", C.c_double),
                ("solve_seconds", C.c_double), ("energy_norm_error", C.c_double), ("build_matrices_ms", C.c_double),
                ("has_forces", C.c_int32), ("pad2", C.c_int32),
                ("force_net", C.c_double * 3), ("force_max", C.c_double), ("force_rel_error", C.c_double),
                ("coarse_solver", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("dofs_by_level", "pad", "pad2", "force_net")}
        d["dofs_by_level"] = [int(self.dofs_by_level[i]) for i in range(self.n_levels)]
        d["force_net"] = [float(v) for v in self.force_net]
        return d


def load(build_if_missing: bool = False):
    global _lib
    if _lib is None:
        if build_if_missing:
            _build.build_all()
        if not os.path.exists(_build.LIB_HOST):
            raise FileNotFoundError(f"{_build.LIB_HOST} missing: run __graft_entry__.build()")
        _lib = C.CDLL(_build.LIB_HOST)
        _lib.step50_create.restype = C.c_void_p
        _lib.step50_last_error.restype = C.c_char_p
        _lib.step50_log.restype = C.c_char_p
        _lib.step50_gmg_context.restype = C.c_void_p
        for f in ("step50_n_atoms", "step50_copy_indices_size", "step50_n_dofs"):
            getattr(_lib, f).restype = C.c_int64
        # host-side setup threads: a GPU box shares its cores between GPUs (16 per GPU)
        _lib.step50_set_threads(C.c_int(max(1, min(16, os.cpu_count() or 1))))
    return _lib


def set_threads(n: int):
    load().step50_set_threads(C.c_int(n))


def prm_text(**kw) -> str:
    """A .prm file body with the reference's keys (src/step-50.cc:13-95)."""
    keymap = {
        "global_refinement": ("Geometry", "Number of global refinement"),
        "left": ("Geometry", "Domain limit left"), "right": ("Geometry", "Domain limit right"),
        "mesh_size": ("Geometry", "Mesh size"), "vacuum": ("Geometry", "Vacuum repetitions"),
        "problem": ("Problem Selection", "Problem"), "dim": ("Problem Selection", "Dimension"),
        "bc": ("Problem Selection", "Boundary conditions selection"),
        "cycles": ("Misc", "Number of Adaptive Refinement"), "r_c": ("Misc", "smoothing length"),
        "cutoff": ("Misc", "Nonzero Density radius parameter around each charge"),
        "rhs_optimization": ("Misc", "Flag for RHS evaluation optimization"),
        "quad_rhs": ("Misc", "Quadrature points for RHS function"),
        "preconditioner": ("Solver input data", "Preconditioner"),
        "lammps": ("Lammps data", "Lammps input file"),
        "smoother": ("Solver input data", "Smoother"), "omega": ("Solver input data", "Smoother damping"),
        "steps": ("Solver input data", "Smoother steps"), "cheb_degree": ("Solver input data", "Chebyshev degree"),
        "cheb_polynomial": ("Solver input data", "Chebyshev polynomial"),
        "cheb_estimate": ("Solver input data", "Chebyshev eigenvalue estimate"),
        "cheb_lanczos_steps": ("Solver input data", "Chebyshev Lanczos steps"),
        "cheb_safety": ("Solver input data", "Chebyshev safety factor"),
        "device_cg": ("Solver input data", "Device resident outer CG"),
        "ssor_blocks": ("Solver input data", "SSOR blocks"),
        "ssor_partition": ("Solver input data", "SSOR block partition"),
        "densities_on_device": ("Misc", "Charge densities on device"),
        "partition_level0": ("Solver input data", "Partition level 0"),
        "refinement_estimator": ("Misc", "Refinement estimator"),
        "level0_numbering": ("Misc", "Level 0 numbering"),
        "level0_on_device": ("Misc", "Level 0 matrix on device"),
        "system_matrix_on_device": ("Misc", "System matrix on device"),
        "level_matrices_on_device": ("Misc", "Level matrices on device"),
        "ssor_plan_on_device": ("Misc", "SSOR plan on device"),
        "rhs_from_cell_tables": ("Misc", "RHS from cell tables"),
        "mesh_tables_on_device": ("Misc", "Mesh tables on device"),
        "operators_from_resident_tables": ("Misc", "Operators from resident tables"),
        "densities_from_resident_tables": ("Misc", "Charge densities from resident tables"),
        "estimator_from_resident_tables": ("Misc", "Estimator from resident tables"),
        "energy_forces_from_resident_tables": ("Misc", "Energy and forces from resident tables"),
        "refinement_on_device": ("Misc", "Refinement on device"),
        "coarse_solver": ("Solver input data", "Coarse solver"),
        "estimator_on_device": ("Misc", "Error estimator on device"),
        "transfer_on_device": ("Misc", "Transfer matrices on device"),
        "rhs_on_device": ("Misc", "RHS on device"),
        "short_range_cutoff": ("Misc", "Short-range cutoff in smoothing lengths"),
        "energy_for_large_systems": ("Misc", "Energy for large systems"),
        "compute_forces": ("Misc", "Compute forces"),
        "direct_coulomb_check": ("Misc", "Direct Coulomb check"),
        "analytical_on_device": ("Misc", "Analytical solution on device"),
        "error_norm_for_large_systems": ("Misc", "Error norm for large systems"),
        "output_analytical": ("Misc", "Output and calculation of Analytical solution"),
        "output_rhs_field": ("Misc", "Output of RHS field"),
        "output_atom_support": ("Misc", "Output of support of each atom"),
        "output_results": ("Misc", "Output results"),
        "output_directory": ("Misc", "Output directory"),
    }
    sections = {}
    for k, v in kw.items():
        sec, key = keymap[k]
        if isinstance(v, bool):
            v = "true" if v else "false"
        sections.setdefault(sec, []).append(f"  set {key} = {v}")
    out = ["set Polynomial degree = 1"]
    for sec, lines in sections.items():
        out += [f"subsection {sec}"] + lines + ["end"]
    return "\n".join(out) + "\n"


class Problem:
    def __init__(self, prm: str):
        self.L = load()
        err = C.create_string_buffer(512)
        self.h = C.c_void_p(self.L.step50_create(prm.encode(), err, 512))
        if not self.h:
            raise RuntimeError(err.value.decode())

    def close(self):
        if self.h:
            self.L.step50_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed (rc={rc}): {self.L.step50_last_error(self.h).decode()}")

    def read_lammps(self, path):
        self._chk(self.L.step50_read_lammps(self.h, path.encode()), "read_lammps_input_file")

    def set_atoms(self, q, xyz):
        q = np.ascontiguousarray(q, dtype=np.float64)
        x = np.ascontiguousarray(xyz, dtype=np.float64)
        self._chk(self.L.step50_set_atoms(self.h, C.c_int64(len(q)), q.ctypes.data_as(C.POINTER(C.c_double)),
                                          x.ctypes.data_as(C.POINTER(C.c_double))), "set_atoms")

    def set_nacl_atoms(self, n_cells):
        self._chk(self.L.step50_set_nacl_atoms(self.h, C.c_int(n_cells)), "set_nacl_atoms")

    def atoms(self):
        n = self.L.step50_n_atoms(self.h)
        q, x = np.empty(n), np.empty((n, 3))
        self.L.step50_get_atoms(self.h, q.ctypes.data_as(C.POINTER(C.c_double)), x.ctypes.data_as(C.POINTER(C.c_double)))
        return q, x

    def run_cycle(self, cycle: int, on_device: bool = True):
        self._chk(self.L.step50_run_cycle(self.h, C.c_int(cycle), C.c_int(1 if on_device else 0)), f"cycle {cycle}")
        return self.report(-1)

    def finish_cycle_with(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._chk(self.L.step50_finish_cycle_with(self.h, x.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(len(x))), "finish_cycle")
        return self.report(-1)

    def solve_again(self):
        self._chk(self.L.step50_solve_again(self.h), "solve")
        return self.report(-1)

    def atom_forces(self, on_device=None, cutoff=None, parts=False):
        """Forces on the atoms from the current solution: (phi_h, E_h, F) with F = q E_h + F^s, as numpy arrays [n], [n, 3],
        [n, 3].  on_device None: where the cycle's solve ran; False: the host mirror; True: the device.  cutoff in units of
        r_c (None: the prm's short-range cutoff, 0: all pairs).  parts=True adds F^s [n, 3] and the per-atom short-range
        energies e_short [n]."""
        n = self.L.step50_n_atoms(self.h)
        phi, E, F, Fs, es = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        where = -1 if on_device is None else int(bool(on_device))
        self._chk(self.L.step50_atom_forces_ex(self.h, C.c_int(where), C.c_double(-1.0 if cutoff is None else cutoff), P(phi), P(E), P(F),
                                               P(Fs), P(es)), "atom_forces")
        return (phi, E, F, Fs, es) if parts else (phi, E, F)

    def direct_coulomb(self, on_device=None):
        """Exact all-pairs Coulomb forces [n, 3] and per-atom energies [n] (on_device as in atom_forces)."""
        n = self.L.step50_n_atoms(self.h)
        F, e = np.zeros((n, 3)), np.zeros(n)
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        where = -1 if on_device is None else int(bool(on_device))
        self._chk(self.L.step50_direct_coulomb_ex(self.h, C.c_int(where), P(F), P(e)), "direct_coulomb")
        return F, e

    def gaussian_potential(self, points, on_device=None, grad=False, phi=True):
        """The exact free-space potential of all atoms at the points [n, 3]: phi [n], with grad=True
        (phi, grad [n, 3]); phi=False leaves the values out of the sums (they come back 0).  on_device None: the device when
        the cycle runs there; False: the host mirror; True: the device."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        want_phi, phi, g = phi, np.zeros(len(pts)), np.zeros((len(pts), 3))
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        where = -1 if on_device is None else int(bool(on_device))
        self._chk(self.L.step50_gaussian_potential(self.h, C.c_int(where), C.c_int64(len(pts)), P(pts), P(phi) if want_phi else None,
                                                   P(g) if grad else None), "gaussian_potential")
        return (phi, g) if grad else phi

    def cell_errors(self, on_device=None, norm=False):
        """Per active cell, the square of the error of the current solution in the energy norm, int_K |grad phi_h - grad phi|^2
        (the true local error beside the Kelly indicator); norm=True adds the norm itself, the square root of their sum:
        (cell_err2, error).  on_device as in gaussian_potential."""
        self.L.step50_n_cells.restype = C.c_int64
        ce, err = np.zeros(self.L.step50_n_cells(self.h)), C.c_double(0)
        where = -1 if on_device is None else int(bool(on_device))
        self._chk(self.L.step50_cell_errors(self.h, C.c_int(where), C.byref(err), ce.ctypes.data_as(C.POINTER(C.c_double))), "cell_errors")
        return (ce, err.value) if norm else ce

    def constraint_inhomogeneities(self):
        """Per DoF, the inhomogeneity of its constraint line (Dirichlet values and what the hanging-node lines inherit; 0 for
        unconstrained DoFs)."""
        out = np.zeros(self.n_dofs())
        self.L.step50_constraint_inhomogeneities(self.h, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def estimator_components(self):
        """Per active cell of the cycle just estimated: (Kelly face sum eta_K^2, residual term, level, centre)."""
        self.L.step50_n_active_cells.restype = C.c_int64
        n = self.L.step50_n_active_cells(self.h)
        k, r, lv, ctr = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros((n, 3))
        self._chk(self.L.step50_estimator_components(self.h, k.ctypes.data_as(C.POINTER(C.c_double)), r.ctypes.data_as(C.POINTER(C.c_double)),
                                                     lv.ctypes.data_as(C.POINTER(C.c_int32)), ctr.ctypes.data_as(C.POINTER(C.c_double))), "estimator_components")
        return k, r, lv, ctr

    def set_smoother(self, smoother: str, ssor_blocks: int = 1):
        """Another smoother on the operators of the cycle just run (re-uploads them; the next solve_again uses it)."""
        self._chk(self.L.step50_set_smoother(self.h, smoother.encode(), C.c_int(ssor_blocks)), "set_smoother")

    def report(self, i=-1) -> dict:
        r = Report()
        self._chk(self.L.step50_get_report(self.h, C.c_int(i), C.byref(r)), "get_report")
        return r.as_dict()

    def log(self) -> str:
        return self.L.step50_log(self.h).decode()

    def n_levels(self):
        return int(self.L.step50_n_levels(self.h))

    def n_dofs(self):
        return int(self.L.step50_n_dofs(self.h))

    def matrix(self, kind, level=0):
        """kind: 'system' | 'level' | 'edge' | 'prolongation' -> namespace(n_rows, n_cols, rowptr, col, val, nnz)"""
        k = {"system": 0, "level": 1, "edge": 2, "prolongation": 3}[kind]
        nr, nc, nz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.step50_matrix_shape(self.h, C.c_int(k), C.c_int(level), C.byref(nr), C.byref(nc), C.byref(nz)), "matrix")
        rp = np.zeros(nr.value + 1, dtype=np.int64)
        col = np.zeros(max(nz.value, 1), dtype=np.int32)
        val = np.zeros(max(nz.value, 1), dtype=np.float64)
        if nr.value > 0:
            self.L.step50_matrix_copy(self.h, C.c_int(k), C.c_int(level), rp.ctypes.data_as(C.POINTER(C.c_int64)),
                                      col.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_double)))
        return SimpleNamespace(n_rows=nr.value, n_cols=nc.value, rowptr=rp, col=col[:nz.value], val=val[:nz.value], nnz=nz.value)

    def matrix_shape(self, kind, level=0):
        """(n_rows, nnz) of an operator of the current cycle without copying it."""
        k = {"system": 0, "level": 1, "edge": 2, "prolongation": 3}[kind]
        nr, nc, nz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.step50_matrix_shape(self.h, C.c_int(k), C.c_int(level), C.byref(nr), C.byref(nc), C.byref(nz)), "matrix_shape")
        return int(nr.value), int(nz.value)

    def copy_indices(self, level):
        n = self.L.step50_copy_indices_size(self.h, C.c_int(level))
        g, l = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        if n:
            self.L.step50_copy_indices(self.h, C.c_int(level), g.ctypes.data_as(C.POINTER(C.c_int32)),
                                       l.ctypes.data_as(C.POINTER(C.c_int32)))
        return g[:n], l[:n]

    def vector(self, which):
        w = {"rhs": 0, "solution": 1, "initial_guess": 2}[which]
        out = np.zeros(self.n_dofs())
        self.L.step50_get_vector(self.h, C.c_int(w), out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def total_charge_density(self):
        """Per DoF, the integrated charge density of its cells (the check vector of tests_rhs_rc_variation)."""
        out = np.zeros(self.n_dofs())
        self.L.step50_total_charge_density(self.h, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def dof_coordinates(self):
        out = np.zeros((self.n_dofs(), 3))
        self.L.step50_dof_coordinates(self.h, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def constrained_mask(self):
        out = np.zeros(self.n_dofs(), dtype=np.int8)
        self.L.step50_constrained_mask(self.h, out.ctypes.data_as(C.POINTER(C.c_int8)))
        return out.astype(bool)

    def hierarchy(self):
        """What LaplaceProblem::solve consumes, as plain arrays (for the oracle in tests)."""
        L = self.n_levels()
        return SimpleNamespace(
            system_matrix=self.matrix("system"), system_rhs=self.vector("rhs"),
            level_matrices=[self.matrix("level", l) for l in range(L)],
            edge_matrices=[self.matrix("edge", l) for l in range(L)],
            prolongations=[self.matrix("prolongation", l) for l in range(L - 1)],
            copy_global=[self.copy_indices(l)[0] for l in range(L)],
            copy_level=[self.copy_indices(l)[1] for l in range(L)],
            constrained=self.constrained_mask())

    def system_assembly_inputs(self):
        """The arrays the driver hands to gmg_assemble_system_matrix for the current mesh: namespace(dim, n_dofs, cell_dofs
        [n_cells, 2^dim], cell_level, K_of_level [16, 2^dim, 2^dim], constraint_of_dof, line_ptr, line_master, line_weight,
        line_inhomogeneity [n_lines])."""
        sz = (C.c_int64 * 4)()
        self._chk(self.L.step50_system_assembly_sizes(self.h, sz), "system_assembly_inputs")
        n_dofs, n_cells, n_lines, n_ent = (int(v) for v in sz)
        dim = int(self.L.step50_dim(self.h))
        nv = 1 << dim
        cd, lv = np.zeros((n_cells, nv), dtype=np.int32), np.zeros(n_cells, dtype=np.uint8)
        K, cons = np.zeros((16, nv, nv)), np.zeros(n_dofs, dtype=np.int32)
        lp, lm, lw, li = np.zeros(n_lines + 1, dtype=np.int64), np.zeros(n_ent, dtype=np.int32), np.zeros(n_ent), np.zeros(n_lines)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._chk(self.L.step50_system_assembly_inputs(self.h, P(cd, C.c_int32), P(lv, C.c_uint8), P(K, C.c_double), P(cons, C.c_int32),
                                                       P(lp, C.c_int64), P(lm, C.c_int32), P(lw, C.c_double), P(li, C.c_double)),
                  "system_assembly_inputs")
        return SimpleNamespace(dim=dim, n_dofs=n_dofs, cell_dofs=cd, cell_level=lv, K_of_level=K, constraint_of_dof=cons, line_ptr=lp,
                               line_master=lm, line_weight=lw, line_inhomogeneity=li)

    def _coefficient_fields(self, sizes_call, inputs_call, what):
        sz = (C.c_int64 * 4)()
        self._chk(sizes_call(sz), what)
        nq, n_cells, nv, n_scale = (int(v) for v in sz)
        cc, G, qw, sc = np.zeros((n_cells, nq)), np.zeros((nq, nv, nv)), np.zeros(nq), np.zeros(n_scale)
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(inputs_call(P(cc), P(G), P(qw), P(sc)), what)
        return dict(nq=nq, cell_coef=cc, G=G, qw=qw), sc

    def system_coefficient_inputs(self):
        """The arrays the driver hands to gmg_assemble_system_matrix_coef for the current mesh: the fields of
        system_assembly_inputs() plus nq, cell_coef [n_cells, nq] (the coefficient at the quadrature points of every active
        cell), G [nq, 2^dim, 2^dim], qw [nq] and scale_of_level [16] (pow(h, dim - 2))."""
        new, sc = self._coefficient_fields(lambda sz: self.L.step50_system_coefficient_sizes(self.h, sz),
                                           lambda *a: self.L.step50_system_coefficient_inputs(self.h, *a), "system_coefficient_inputs")
        return SimpleNamespace(**vars(self.system_assembly_inputs()), **new, scale_of_level=sc)

    def level_coefficient_inputs(self, level):
        """The arrays the driver hands to gmg_assemble_level_matrix_coef for one level of the current mesh: the fields of
        level_assembly_inputs(level) plus nq, cell_coef [n_cells, nq] (all cells of the level), G, qw and scale."""
        new, sc = self._coefficient_fields(lambda sz: self.L.step50_level_coefficient_sizes(self.h, C.c_int(level), sz),
                                           lambda *a: self.L.step50_level_coefficient_inputs(self.h, C.c_int(level), *a),
                                           "level_coefficient_inputs")
        return SimpleNamespace(**vars(self.level_assembly_inputs(level)), **new, scale=float(sc[0]))

    def rhs_assembly_inputs(self):
        """The arrays the driver hands to gmg_assemble_rhs for the current mesh: the fields of system_assembly_inputs() plus nq,
        shape [nq, 2^dim], weight [nq], jxw_of_level [16] and source [n_cells, nq]: the integrand at the quadrature points of
        every active cell -- the charge densities as the host forms them, or Step16's function values."""
        sz = (C.c_int64 * 3)()
        self._chk(self.L.step50_rhs_assembly_sizes(self.h, sz), "rhs_assembly_inputs")
        nq, n_cells, nv = (int(v) for v in sz)
        sh, w, jxw, src = np.zeros((nq, nv)), np.zeros(nq), np.zeros(16), np.zeros((n_cells, nq))
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(self.L.step50_rhs_assembly_inputs(self.h, P(sh), P(w), P(jxw), P(src)), "rhs_assembly_inputs")
        return SimpleNamespace(**vars(self.system_assembly_inputs()), nq=nq, shape=sh, weight=w, jxw_of_level=jxw, source=src)

    def rhs_from_cell_tables(self) -> bool:
        """Did the last assembly form the right-hand side through gmg_assemble_rhs?"""
        return bool(self.L.step50_rhs_from_cell_tables(self.h))

    def forest_cells(self):
        """The arrays the driver hands to gmg_build_mesh_tables for the current forest: namespace(dim, n0 [3], n_levels,
        level_ptr [n_levels + 1], cell_coord [n, 3], cell_first_child [n], level0_lexicographic)."""
        sz = (C.c_int64 * 3)()
        self._chk(self.L.step50_forest_sizes(self.h, sz), "forest_cells")
        n_levels, n, lex = (int(v) for v in sz)
        n0, lp = np.zeros(3, dtype=np.int32), np.zeros(n_levels + 1, dtype=np.int64)
        cc, fc = np.zeros((n, 3), dtype=np.int32), np.zeros(n, dtype=np.int32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._chk(self.L.step50_forest_cells(self.h, P(n0, C.c_int32), P(lp, C.c_int64), P(cc, C.c_int32), P(fc, C.c_int32)), "forest_cells")
        return SimpleNamespace(dim=int(self.L.step50_dim(self.h)), n0=n0, n_levels=n_levels, level_ptr=lp, cell_coord=cc, cell_first_child=fc,
                               level0_lexicographic=bool(lex))

    def mesh_tables_on_device(self) -> bool:
        """Did the last setup_system form the DoF numbering, the constraints and the level flags through gmg_build_mesh_tables?"""
        return bool(self.L.step50_mesh_tables_on_device(self.h))

    def operators_resident(self) -> bool:
        """Do this cycle's device entries read the context's mesh tables ("Operators from resident tables" took effect)?"""
        return bool(self.L.step50_operators_resident(self.h))

    def densities_resident(self) -> bool:
        """Did the last setup_system form the densities through gmg_charge_density_resident ("Charge densities from resident
        tables" took effect)?"""
        return bool(self.L.step50_densities_resident(self.h))

    def estimator_resident(self) -> bool:
        """Did the last estimate go through gmg_build_face_table_resident and gmg_estimate_error_resident ("Estimator from
        resident tables" took effect)?"""
        return bool(self.L.step50_estimator_resident(self.h))

    def energy_forces_resident(self) -> bool:
        """Did the last finish_cycle take the energy's sums and the forces from gmg_electrostatic_energy_resident and
        gmg_atom_forces_resident ("Energy and forces from resident tables" took effect)?"""
        return bool(self.L.step50_energy_forces_resident(self.h))

    def refined_on_device(self) -> bool:
        """Did the last refine_grid go through gmg_refine_forest and gmg_transfer_solution ("Refinement on device")?"""
        return bool(self.L.step50_refined_on_device(self.h))

    def forest_parents(self):
        """cell_parent of every cell of forest_cells(): the index inside the previous level, -1 on level 0."""
        out = np.zeros(len(self.forest_cells().cell_first_child), dtype=np.int32)
        self.L.step50_forest_parents(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out

    def vertex_keys(self):
        """The vertex key of every active DoF (x | y << 21 | z << 42 on the level-12 lattice)."""
        out = np.zeros(self.n_dofs(), dtype=np.uint64)
        self.L.step50_vertex_keys(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def closed_flags(self):
        """The marks of the last refine_grid after the 2:1 closure, over the cells of all levels of the forest it refined."""
        self.L.step50_closed_flags.restype = C.c_int64
        out = np.zeros(max(self.L.step50_closed_flags(self.h, None), 1), dtype=np.uint8)
        n = self.L.step50_closed_flags(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out[:n]

    def refine_with_flags(self, flags, on_device: bool = False):
        """refine_grid on a given flag array (one per cell of every level of forest_cells()): the closure, the split, the next
        cycle's setup_system and the solution transfer, on the path the prm selects for a cycle that runs on the device
        (on_device) or not.  forest_cells(), forest_parents(), closed_flags() and vector("solution") show the result."""
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        self._chk(self.L.step50_refine_with_flags(self.h, f.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int64(len(f)), C.c_int(1 if on_device else 0)),
                  "refine_with_flags")

    def device_system_matrix(self):
        """The system matrix as the device holds it after a cycle with "System matrix on device" (gmg_get_system_matrix)."""
        from . import capi
        return capi.Context.view(self.gmg_context()).get_system_matrix()

    def system_matrix_on_device(self) -> bool:
        """Did the last upload form the system matrix on the device?"""
        return bool(self.L.step50_system_matrix_on_device(self.h))

    def level_assembly_inputs(self, level):
        """The arrays the driver hands to gmg_assemble_level_matrix for one level of the current mesh: namespace(dim, n_dofs,
        cell_dofs [n_cells, 2^dim], K [2^dim, 2^dim], dof_flags [n_dofs]: bit 0 boundary, bit 1 refinement edge)."""
        sz = (C.c_int64 * 3)()
        self._chk(self.L.step50_level_assembly_sizes(self.h, C.c_int(level), sz), "level_assembly_inputs")
        dim, n_dofs, n_cells = (int(v) for v in sz)
        nv = 1 << dim
        cd, K, fl = np.zeros((n_cells, nv), dtype=np.int32), np.zeros((nv, nv)), np.zeros(n_dofs, dtype=np.uint8)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._chk(self.L.step50_level_assembly_inputs(self.h, C.c_int(level), P(cd, C.c_int32), P(K, C.c_double), P(fl, C.c_uint8)),
                  "level_assembly_inputs")
        return SimpleNamespace(dim=dim, n_dofs=n_dofs, cell_dofs=cd, K=K, dof_flags=fl)

    def device_level_matrix(self, level, which="level"):
        """A level's operator as the device holds it (gmg_get_level_matrix): which = 'level' (A_l) | 'edge' (I_l, without
        its zeros) | 'edge_t' (I_l^T)."""
        from . import capi
        w = {"level": capi.LEVEL_A, "edge": capi.LEVEL_EDGE, "edge_t": capi.LEVEL_EDGE_T}[which]
        return capi.Context.view(self.gmg_context()).get_level_matrix(level, w)

    def level_matrices_on_device(self) -> bool:
        """Did the last upload form the level and interface matrices on the device?"""
        return bool(self.L.step50_level_matrices_on_device(self.h))

    def ssor_plan_origin(self, level):
        """gmg_get_ssor_plan_origin of the last upload: (built on the device?, bytes of col / val downloaded for it, why the host built it or '')."""
        on_dev, moved, why = C.c_int(0), C.c_int64(0), C.c_char_p()
        rc = self.L.step50_ssor_plan_origin(self.h, C.c_int(level), C.byref(on_dev), C.byref(moved), C.byref(why))
        if rc != 0:
            raise RuntimeError(f"step50_ssor_plan_origin: level {level} has no plan (error {rc})")
        return bool(on_dev.value), int(moved.value), (why.value or b"").decode()

    def refine_flags(self):
        """The refinement marks of the cycle just estimated, all levels concatenated (uint8)."""
        self.L.step50_refine_flags.restype = C.c_int64
        n = self.L.step50_refine_flags(self.h, None)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self.L.step50_refine_flags(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out[:n]

    def estimator_inputs(self):
        """The arrays the driver hands to gmg_estimate_error for the current mesh: namespace(dim, n_cells, n_u, ng, nq,
        residual, dens_resident, cell_dofs [n_cells, 2^dim], cell_level, face_kind [n_cells, 2 dim], face_cell [n_cells, 2 dim,
        2^(dim-1)], h_of_level, face_measure_of_level, diameter_of_level, jxw_of_level [16], gauss_x, gauss_w [ng], weight [nq],
        dens [n_cells, nq] or None (residual 0, or dens_resident: the driver passes NULL and the library takes the densities
        gmg_charge_density left on the device), fraction)."""
        sz = (C.c_int64 * 8)()
        self._chk(self.L.step50_estimator_sizes(self.h, sz), "estimator_inputs")
        dim, n_cells, n_u, ng, nq, residual, resident, n_dens = (int(v) for v in sz)
        nv, nfc, nf = 1 << dim, 1 << (dim - 1), 2 * dim
        cd, lv = np.zeros((n_cells, nv), dtype=np.int32), np.zeros(n_cells, dtype=np.uint8)
        fk, fc = np.zeros((n_cells, nf), dtype=np.uint8), np.zeros((n_cells, nf, nfc), dtype=np.int32)
        hl, fm, dl, jl = np.zeros(16), np.zeros(16), np.zeros(16), np.zeros(16)
        gx, gw, w, dens, frac = np.zeros(ng), np.zeros(ng), np.zeros(nq), np.zeros(max(n_dens, 1)), C.c_double(0)
        P = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        self._chk(self.L.step50_estimator_inputs(self.h, P(cd, C.c_int32), P(lv, C.c_uint8), P(fk, C.c_uint8), P(fc, C.c_int32), P(hl), P(fm),
                                                 P(dl), P(gx), P(gw), P(w), P(jl), P(dens), C.byref(frac)), "estimator_inputs")
        return SimpleNamespace(dim=dim, n_cells=n_cells, n_u=n_u, ng=ng, nq=nq, residual=residual, dens_resident=bool(resident), cell_dofs=cd,
                               cell_level=lv, face_kind=fk, face_cell=fc, h_of_level=hl, face_measure_of_level=fm, diameter_of_level=dl,
                               jxw_of_level=jl, gauss_x=gx, gauss_w=gw, weight=w,
                               dens=dens[:n_dens].reshape(n_cells, nq) if n_dens else None, fraction=frac.value)

    def estimate(self, on_device: bool):
        """Re-run the estimator and the marking on the current solution: the host loops (False) or gmg_estimate_error (True),
        whatever the prm says.  Returns the report with the new refine_threshold."""
        self._chk(self.L.step50_estimate(self.h, C.c_int(1 if on_device else 0)), "estimate")
        return self.report(-1)

    def estimated_on_device(self) -> bool:
        """Did the last estimate come from gmg_estimate_error?"""
        return bool(self.L.step50_estimated_on_device(self.h))

    def host_density_copies(self) -> int:
        """How often device-resident charge densities were copied to the host (ensure_host_densities)."""
        self.L.step50_host_density_copies.restype = C.c_int64
        return int(self.L.step50_host_density_copies(self.h))

    def electrostatic_energy(self):
        """The electrostatic energy of the current solution once more, by the path the cycle took (host loops, or
        gmg_electrostatic_energy_resident where "Energy and forces from resident tables" took effect): the report."""
        self._chk(self.L.step50_electrostatic_energy(self.h), "electrostatic_energy")
        return self.report(-1)

    def point_locator(self):
        """The host's flattened forest as gmg_set_point_locator takes it (LaplaceProblem::point_locator): node [cells of all
        levels], >= 0 the flat index of child 0, < 0 the active cell -node - 1."""
        self.L.step50_point_locator.restype = C.c_int64
        out = np.zeros(self.L.step50_point_locator(self.h, None), dtype=np.int32)
        if out.size:
            self.L.step50_point_locator(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out

    def dof_map_builds(self) -> int:
        """How often the host built its vertex -> DoF hash tables (ensure_dof_maps)."""
        self.L.step50_dof_map_builds.restype = C.c_int64
        return int(self.L.step50_dof_map_builds(self.h))

    def error_per_cell(self):
        """eta per active cell of the last estimate (float32)."""
        self.L.step50_n_cells.restype = C.c_int64
        out = np.zeros(self.L.step50_n_cells(self.h), dtype=np.float32)
        self.L.step50_error_per_cell(self.h, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def output_results(self, cycle, directory=None):
        """Write solution-CCCCC.0000.vtu, solution-CCCCC.pvtu and solution-CCCCC.visit of the current solution and estimate
        into `directory` (None: the prm's "Output directory"), whether or not "Output results" is set (DESIGN.md section
        35).  Returns the path the patches took: 0 host mirror, 1 gmg_output_patches, 2 gmg_output_patches_resident."""
        self._chk(self.L.step50_output_results(self.h, C.c_int(int(cycle)), None if directory is None else os.fsencode(directory)), "output_results")
        return int(self.L.step50_output_path(self.h))

    def output_path(self) -> int:
        """Where the last output_results (the cycle's or an explicit one) formed its patches: 0, 1 or 2 as above."""
        return int(self.L.step50_output_path(self.h))

    def output_patches(self, on_device=False):
        """The patch arrays of the graphical output, one patch per active cell with 2^dim vertices: (point [slots, 3],
        solution [slots], grad_phi [slots, 3]).  on_device False: the host mirror; True: the device (the resident mesh tables
        where the context holds them and the solution, else host arrays)."""
        self.L.step50_n_cells.restype = C.c_int64
        ns = self.L.step50_n_cells(self.h) << int(self.L.step50_dim(self.h))
        pt, sol, g = np.zeros((ns, 3)), np.zeros(ns), np.zeros((ns, 3))
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(self.L.step50_output_patches(self.h, C.c_int(1 if on_device else 0), P(pt), P(sol), P(g)), "output_patches")
        return pt, sol, g

    def marks(self):
        """The refinement marks of the last estimate per active cell (uint8)."""
        self.L.step50_n_cells.restype = C.c_int64
        out = np.zeros(self.L.step50_n_cells(self.h), dtype=np.uint8)
        self._chk(self.L.step50_marks(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))), "marks")
        return out

    def face_integrals(self):
        """The face integrals of the last estimate, [active cells, 2 dim]."""
        self.L.step50_n_cells.restype = C.c_int64
        out = np.zeros((self.L.step50_n_cells(self.h), 2 * int(self.L.step50_dim(self.h))))
        self.L.step50_face_integrals(self.h, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def set_communicator(self, rank, n_ranks, uid: bytes):
        buf = C.create_string_buffer(uid, 128)
        self._chk(self.L.step50_set_communicator(self.h, C.c_int(rank), C.c_int(n_ranks), buf), "set_communicator")

    def localize(self, kind, level, rank, n_ranks):
        """partition.h applied to one operator: local CSR ([owned | ghost] columns) + halo plan."""
        k = {"system": 0, "level": 1}[kind]

        class Info(C.Structure):
            _fields_ = [(n, C.c_int64) for n in ("n_rows", "n_cols", "nnz", "row_begin", "n_neighbors", "n_send")]

        info = Info()
        self._chk(self.L.step50_localize(self.h, C.c_int(k), C.c_int(level), C.c_int(rank), C.c_int(n_ranks), C.byref(info)), "localize")
        rp = np.zeros(info.n_rows + 1, dtype=np.int64)
        col = np.zeros(max(info.nnz, 1), dtype=np.int32)
        val = np.zeros(max(info.nnz, 1))
        nb = np.zeros(max(info.n_neighbors, 1), dtype=np.int32)
        sc, rc = np.zeros_like(nb), np.zeros_like(nb)
        si = np.zeros(max(info.n_send, 1), dtype=np.int32)
        gg = np.zeros(max(info.n_cols - info.n_rows, 1), dtype=np.int64)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self.L.step50_localize_copy(P(rp, C.c_int64), P(col, C.c_int32), P(val, C.c_double), P(nb, C.c_int32), P(sc, C.c_int32),
                                    P(si, C.c_int32), P(rc, C.c_int32), P(gg, C.c_int64))
        nn = info.n_neighbors
        return SimpleNamespace(n_rows=info.n_rows, n_cols=info.n_cols, rowptr=rp, col=col[:info.nnz], val=val[:info.nnz],
                               nnz=info.nnz, row_begin=info.row_begin, neighbor_rank=nb[:nn], send_count=sc[:nn],
                               recv_count=rc[:nn], send_idx=si[:info.n_send], ghost_global=gg[:info.n_cols - info.n_rows])

    def gmg_context(self):
        return C.c_void_p(self.L.step50_gmg_context(self.h))
