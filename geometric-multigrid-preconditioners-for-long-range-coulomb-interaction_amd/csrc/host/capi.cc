// capi.cc -- flat C entry points over LaplaceProblem<dim> for tests/ and bench.py (ctypes).
// Not part of the drop-in boundary (that is include/gmg_coulomb.h); this is how Python drives
// the host-side C++ the same way src/main.cc of the reference drives LaplaceProblem.
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "laplace_problem.h"
#include "partition.h"
#ifdef _OPENMP
#include <omp.h>
#endif

using namespace step50;

struct step50_problem {
  int dim = 3;
  std::unique_ptr<LaplaceProblem<2>> p2;
  std::unique_ptr<LaplaceProblem<3>> p3;
  std::string err;
};

#define DISPATCH(h, expr) ((h)->dim == 2 ? (h)->p2->expr : (h)->p3->expr)

namespace {
template <class F>
int guarded(step50_problem *h, F f) {
  try {
    return f();
  } catch (const std::exception &e) {
    h->err = e.what();
    return -1;
  }
}
const CSRMatrix *pick_matrix(step50_problem *h, int kind, int level) {
  // kind 0 system, 1 level, 2 edge, 3 prolongation
  if (kind == 0) { DISPATCH(h, ensure_system_matrix()); return &DISPATCH(h, system_matrix); }  // (it may have been left to the device)
  if (kind == 1) DISPATCH(h, ensure_level_matrix(level));  // (level 0 may have been left to the device: assemble it now)
  if (kind == 2 && DISPATCH(h, par.level_matrices_on_device)) DISPATCH(h, ensure_level_matrix(level));  // (I_l comes with A_l)
  if (kind == 3) DISPATCH(h, ensure_prolongation(level));   // (the transfers likewise)
  auto &v = kind == 1 ? DISPATCH(h, mg_matrices) : kind == 2 ? DISPATCH(h, mg_interface_matrices) : DISPATCH(h, mg_prolongation);
  if (level < 0 || level >= (int)v.size()) return nullptr;
  return &v[(size_t)level];
}
}  // namespace

extern "C" {

step50_problem *step50_create(const char *prm_text, char *err, int err_len) {
  auto *h = new step50_problem();
  try {
    ParameterReader prm;
    prm.declare_parameters();
    prm.parse_input_from_string(prm_text);
    Parameters par = Parameters::from(prm);
    h->dim = par.dim;
    if (par.dim == 2) h->p2.reset(new LaplaceProblem<2>(par));
    else if (par.dim == 3) h->p3.reset(new LaplaceProblem<3>(par));
    else throw std::runtime_error("Only 2d and 3d dimensions are supported.");  // src/main.cc:92-95
    return h;
  } catch (const std::exception &e) {
    if (err && err_len > 0) { std::strncpy(err, e.what(), (size_t)err_len - 1); err[err_len - 1] = 0; }
    delete h;
    return nullptr;
  }
}
void step50_destroy(step50_problem *h) { delete h; }
const char *step50_last_error(step50_problem *h) {
  const std::string &le = DISPATCH(h, last_error);
  return h->err.empty() ? le.c_str() : h->err.c_str();
}
const char *step50_log(step50_problem *h) { return DISPATCH(h, log).c_str(); }
void step50_set_echo(step50_problem *h, int on) { DISPATCH(h, echo) = on != 0; }

int step50_read_lammps(step50_problem *h, const char *path) {
  return guarded(h, [&] { DISPATCH(h, read_lammps_input_file(path)); return DISPATCH(h, lammpsinput) ? 0 : 1; });
}
int step50_set_atoms(step50_problem *h, int64_t n, const double *q, const double *xyz) {
  return guarded(h, [&] {
    std::vector<double> qq(q, q + n), xx(xyz, xyz + 3 * n);
    DISPATCH(h, set_atoms(qq, xx));
    return 0;
  });
}
int step50_set_nacl_atoms(step50_problem *h, int n_cells) {
  return guarded(h, [&] {
    std::vector<double> q;
    std::vector<double> x = nacl_lattice(n_cells, q);
    DISPATCH(h, set_atoms(q, x));
    return 0;
  });
}
int64_t step50_n_atoms(step50_problem *h) { return (int64_t)DISPATCH(h, number_of_atoms); }
int step50_get_atoms(step50_problem *h, double *q, double *xyz) {
  const auto &qq = DISPATCH(h, charges);
  const auto &xx = DISPATCH(h, atom_positions);
  std::memcpy(q, qq.data(), sizeof(double) * qq.size());
  std::memcpy(xyz, xx.data(), sizeof(double) * xx.size());
  return 0;
}

// one pass of the loop body of LaplaceProblem::run (src/step-50.cc:1484-1561)
int step50_run_cycle(step50_problem *h, int cycle, int on_device) {
  return guarded(h, [&] { return DISPATCH(h, run_cycle((unsigned)cycle, on_device != 0)); });
}
// the timed bench step: repeat solve() of the current cycle from the same initial guess
int step50_solve_again(step50_problem *h) {
  return guarded(h, [&] { return DISPATCH(h, solve_again()); });
}
// marking-rule study (tools/marking_rule_scan.py): per active cell of the cycle just estimated, the Kelly face sum
// eta_K^2, the residual term h_K^2 int_K (4 pi rho)^2, the cell's level, and its centre
int64_t step50_n_active_cells(step50_problem *h) { return (int64_t)DISPATCH(h, estimator_kelly_sq).size(); }
int step50_estimator_components(step50_problem *h, double *kelly_sq, double *residual_sq, int32_t *level, double *centre) {
  return guarded(h, [&] {
    const auto &k = DISPATCH(h, estimator_kelly_sq);
    const auto &r = DISPATCH(h, estimator_residual_sq);
    std::memcpy(kelly_sq, k.data(), sizeof(double) * k.size());
    std::memcpy(residual_sq, r.data(), sizeof(double) * r.size());
    auto fill = [&](auto &P) {
      for (size_t a = 0; a < P.active_cells.size(); ++a) {
        const auto &ac = P.active_cells[a];
        level[a] = ac.level;
        double x0[3] = {0, 0, 0};
        const double hh = P.triangulation.cell_size(ac.level);
        P.triangulation.cell_origin(ac.level, P.triangulation.levels[(size_t)ac.level][(size_t)ac.index], x0);
        for (int d = 0; d < 3; ++d) centre[3 * a + d] = x0[d] + 0.5 * hh;
      }
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
// bench: re-upload the current cycle's operators with another smoother
int step50_set_smoother(step50_problem *h, const char *smoother, int ssor_blocks) {
  return guarded(h, [&] { return DISPATCH(h, set_smoother(std::string(smoother), ssor_blocks)); });
}
// CPU-only continuation of a cycle for tests: inject a solution, then estimator + energy
int step50_finish_cycle_with(step50_problem *h, const double *x, int64_t n) {
  return guarded(h, [&] {
    std::vector<double> v(x, x + n);
    DISPATCH(h, set_solution(v));
    DISPATCH(h, finish_cycle());
    return 0;
  });
}
int step50_n_reports(step50_problem *h) { return (int)DISPATCH(h, reports).size(); }

struct step50_report {
  int32_t cycle, cg_iterations, status, has_energy, n_levels, pad;
  int64_t active_cells, dofs, coarse_iterations;
  int64_t dofs_by_level[16];
  double rhs_l1, rhs_l2, rhs_linf, matrix_l1, matrix_linf, matrix_frobenius;
  double starting_value, convergence_value, sol_l1, sol_l2, sol_linf, refine_threshold;
  double energy_analytical, energy_short, energy_fe_long, energy_self, energy_total, energy_abs_error;
  double solve_seconds, energy_norm_error;
  double build_matrices_ms;  // device time of MGTransferPrebuilt::build_matrices (gmg_build_transfer) for this cycle; 0: built on the host
  int32_t has_forces, pad2;  // "Compute forces": net force, largest |F_i|, relative RMS error against the direct sum (0: not checked)
  double force_net[3], force_max, force_rel_error;
  int64_t coarse_solver;  // GMG_COARSE_CG (0) / GMG_COARSE_DIRECT (1): what the cycle's last coarse solve ran
};
int step50_get_report(step50_problem *h, int i, step50_report *out) {
  const auto &reps = DISPATCH(h, reports);
  if (i < 0) i += (int)reps.size();
  if (i < 0 || i >= (int)reps.size()) return 1;
  const CycleReport &r = reps[(size_t)i];
  std::memset(out, 0, sizeof *out);
  out->cycle = r.cycle; out->cg_iterations = r.cg_iterations; out->status = r.status; out->has_energy = r.has_energy;
  out->n_levels = (int32_t)r.dofs_by_level.size();
  out->active_cells = r.active_cells; out->dofs = r.dofs; out->coarse_iterations = r.coarse_iterations;
  for (size_t l = 0; l < r.dofs_by_level.size() && l < 16; ++l) out->dofs_by_level[l] = r.dofs_by_level[l];
  out->rhs_l1 = r.rhs_l1; out->rhs_l2 = r.rhs_l2; out->rhs_linf = r.rhs_linf;
  out->matrix_l1 = r.matrix_l1; out->matrix_linf = r.matrix_linf; out->matrix_frobenius = r.matrix_frobenius;
  out->starting_value = r.starting_value; out->convergence_value = r.convergence_value;
  out->sol_l1 = r.sol_l1; out->sol_l2 = r.sol_l2; out->sol_linf = r.sol_linf; out->refine_threshold = r.refine_threshold;
  out->energy_analytical = r.energy_analytical; out->energy_short = r.energy_short; out->energy_fe_long = r.energy_fe_long;
  out->energy_self = r.energy_self; out->energy_total = r.energy_total; out->energy_abs_error = r.energy_abs_error;
  out->solve_seconds = r.solve_seconds;
  out->energy_norm_error = r.energy_norm_error;
  out->build_matrices_ms = r.build_matrices_ms;
  out->has_forces = r.has_forces;
  for (int d = 0; d < 3; ++d) out->force_net[d] = r.force_net[d];
  out->force_max = r.force_max; out->force_rel_error = r.force_rel_error;
  out->coarse_solver = r.coarse_solver;
  return 0;
}

// ---- forces on the atoms of the current solution: phi_h [n], E_h [3n], F = q E_h + F^s [3n]; any
// output may be null.  On the device when the cycle's solve ran there, else by the host mirror; cutoff = the prm's
// "Short-range cutoff in smoothing lengths".
namespace {
int copy_out(const std::vector<double> &v, double *out) {
  if (out) std::memcpy(out, v.data(), sizeof(double) * v.size());
  return 0;
}
int atom_forces_impl(step50_problem *h, int where, double cutoff, double *phi, double *field, double *force, double *force_short,
                     double *e_short) {
  if (h->dim != 3) { h->err = "atom forces: 3D only"; return GMG_ERR_UNSUPPORTED; }
  auto &P = *h->p3;
  const bool dev = where < 0 ? P.forces_on_device() : where != 0;
  std::vector<double> a, b, c, d, e;
  const int rc = P.atom_forces(dev, cutoff < 0 ? P.par.short_range_cutoff : cutoff, phi ? &a : nullptr, field ? &b : nullptr,
                               force ? &c : nullptr, force_short ? &d : nullptr, e_short ? &e : nullptr);
  if (rc != GMG_OK) return rc;
  copy_out(a, phi); copy_out(b, field); copy_out(c, force); copy_out(d, force_short); copy_out(e, e_short);
  return 0;
}
int direct_coulomb_impl(step50_problem *h, int where, double *force, double *energy) {
  if (h->dim != 3) { h->err = "direct Coulomb sum: 3D only"; return GMG_ERR_UNSUPPORTED; }
  auto &P = *h->p3;
  std::vector<double> f, e;
  const int rc = P.direct_coulomb(where < 0 ? P.forces_on_device() : where != 0, force ? &f : nullptr, energy ? &e : nullptr);
  if (rc != GMG_OK) return rc;
  copy_out(f, force); copy_out(e, energy);
  return 0;
}
}  // namespace
int step50_atom_forces(step50_problem *h, double *phi, double *field, double *force) {
  return guarded(h, [&] { return atom_forces_impl(h, -1, -1.0, phi, field, force, nullptr, nullptr); });
}
// exact all-pairs Coulomb forces [3n] and per-atom energies [n] (either may be null)
int step50_direct_coulomb(step50_problem *h, double *force, double *energy) {
  return guarded(h, [&] { return direct_coulomb_impl(h, -1, force, energy); });
}
// the same with the backend chosen (where: -1 as the cycle ran, 0 host mirror, 1 device), the cutoff given (< 0: the
// prm's), and the pair part F^s and the per-atom short-range energies (tests compare the two backends on one solution)
int step50_atom_forces_ex(step50_problem *h, int where, double cutoff, double *phi, double *field, double *force, double *force_short,
                          double *e_short) {
  return guarded(h, [&] { return atom_forces_impl(h, where, cutoff, phi, field, force, force_short, e_short); });
}
int step50_direct_coulomb_ex(step50_problem *h, int where, double *force, double *energy) {
  return guarded(h, [&] { return direct_coulomb_impl(h, where, force, energy); });
}

// ---- the exact free-space potential of the atoms; where: -1 as the cycle ran, 0 host mirror, 1 device.
// phi [n] and grad [3n] at n points [3n] (either output may be null)
int step50_gaussian_potential(step50_problem *h, int where, int64_t n, const double *points, double *phi, double *grad) {
  return guarded(h, [&] {
    if (h->dim != 3) { h->err = "exact potential: 3D only"; return (int)GMG_ERR_UNSUPPORTED; }
    auto &P = *h->p3;
    return P.gaussian_potential(where < 0 ? P.exact_on_device() : where != 0, n, points, phi, grad);
  });
}
// error of the current solution in the energy norm and its per-cell squares [step50_n_cells] (either may be null)
int64_t step50_n_cells(step50_problem *h) { return (int64_t)DISPATCH(h, active_cells.size()); }
int step50_cell_errors(step50_problem *h, int where, double *error, double *cell_err2) {
  return guarded(h, [&] {
    if (h->dim != 3) { h->err = "energy norm error: 3D only"; return (int)GMG_ERR_UNSUPPORTED; }
    auto &P = *h->p3;
    std::vector<double> ce;
    const int rc = P.energy_norm_error(where < 0 ? P.exact_on_device() : where != 0, error, cell_err2 ? &ce : nullptr);
    if (rc == GMG_OK) copy_out(ce, cell_err2);
    return rc;
  });
}
// the inhomogeneity of every DoF's constraint line (0 for unconstrained DoFs): Dirichlet values, and what close() folded
// into the hanging-node lines
int step50_constraint_inhomogeneities(step50_problem *h, double *out) {
  const auto &c = DISPATCH(h, constraint_of_dof);
  auto fill = [&](auto &P) {
    for (size_t i = 0; i < c.size(); ++i) out[i] = c[i] >= 0 ? P.constraint_lines[(size_t)c[i]].inhomogeneity : 0.0;
  };
  if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
  return 0;
}

// ---- access to what solve() consumes, so tests can hand the same inputs to the oracle
int step50_n_levels(step50_problem *h) { return h->dim == 2 ? h->p2->triangulation.n_levels() : h->p3->triangulation.n_levels(); }
int step50_matrix_shape(step50_problem *h, int kind, int level, int64_t *n_rows, int64_t *n_cols, int64_t *nnz) {
  const CSRMatrix *m = pick_matrix(h, kind, level);
  if (!m) return 1;
  *n_rows = m->n_rows; *n_cols = m->n_cols; *nnz = m->nnz();
  return 0;
}
int step50_matrix_copy(step50_problem *h, int kind, int level, int64_t *rowptr, int32_t *col, double *val) {
  const CSRMatrix *m = pick_matrix(h, kind, level);
  if (!m) return 1;
  std::memcpy(rowptr, m->rowptr.data(), sizeof(int64_t) * m->rowptr.size());
  std::memcpy(col, m->col.data(), sizeof(int32_t) * m->col.size());
  std::memcpy(val, m->val.data(), sizeof(double) * m->val.size());
  return 0;
}
int64_t step50_copy_indices_size(step50_problem *h, int level) { return (int64_t)DISPATCH(h, copy_global)[(size_t)level].size(); }
int step50_copy_indices(step50_problem *h, int level, int32_t *global_idx, int32_t *level_idx) {
  const auto &g = DISPATCH(h, copy_global)[(size_t)level];
  const auto &l = DISPATCH(h, copy_level)[(size_t)level];
  std::memcpy(global_idx, g.data(), sizeof(int32_t) * g.size());
  std::memcpy(level_idx, l.data(), sizeof(int32_t) * l.size());
  return 0;
}
int64_t step50_n_dofs(step50_problem *h) { return (int64_t)DISPATCH(h, vertex_of_dof).size(); }
int step50_get_vector(step50_problem *h, int which, double *out) {
  // 0 system_rhs, 1 solution (after constraints.distribute), 2 initial guess
  const auto &v = which == 0 ? DISPATCH(h, system_rhs) : which == 1 ? DISPATCH(h, solution) : DISPATCH(h, initial_guess);
  std::memcpy(out, v.data(), sizeof(double) * v.size());
  return 0;
}
// check vector of the reference's rhs test: per DoF, the integrated charge density of its cells
int step50_total_charge_density(step50_problem *h, double *out) {
  const std::vector<double> v = DISPATCH(h, total_charge_density_vector());
  std::memcpy(out, v.data(), sizeof(double) * v.size());
  return 0;
}
int step50_dof_coordinates(step50_problem *h, double *xyz) {
  const auto &keys = DISPATCH(h, vertex_of_dof);
  for (size_t i = 0; i < keys.size(); ++i) {
    if (h->dim == 2) h->p2->triangulation.vertex_coords(keys[i], xyz + 3 * i);
    else h->p3->triangulation.vertex_coords(keys[i], xyz + 3 * i);
  }
  return 0;
}
int step50_constrained_mask(step50_problem *h, int8_t *out) {
  const auto &c = DISPATCH(h, constraint_of_dof);
  for (size_t i = 0; i < c.size(); ++i) out[i] = c[i] >= 0;
  return 0;
}
void *step50_gmg_context(step50_problem *h) { return DISPATCH(h, gmg); }

// ---- "System matrix on device" (DESIGN.md section 12): the arrays the driver hands to gmg_assemble_system_matrix for the
// current mesh, so that a test can restate the assembly from the same inputs.  sizes: n_dofs, n_cells, n_lines, n_entries
int step50_dim(step50_problem *h) { return h->dim; }
int step50_system_matrix_on_device(step50_problem *h) { return DISPATCH(h, system_on_device) ? 1 : 0; }
int step50_system_assembly_sizes(step50_problem *h, int64_t sizes[4]) {
  return guarded(h, [&] {
    auto fill = [&](auto &P) {
      sizes[0] = (int64_t)P.vertex_of_dof.size(); sizes[1] = (int64_t)P.active_cells.size(); sizes[2] = (int64_t)P.constraint_lines.size();
      sizes[3] = 0;
      for (auto &l : P.constraint_lines) sizes[3] += (int64_t)l.entries.size();
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
int step50_system_assembly_inputs(step50_problem *h, int32_t *cell_dofs, uint8_t *cell_level, double *K_of_level, int32_t *constraint_of_dof,
                                  int64_t *line_ptr, int32_t *line_master, double *line_weight, double *line_inhomogeneity) {
  return guarded(h, [&] {
    auto fill = [&](auto &P) {
      const auto in = P.system_assembly_inputs();
      auto put = [](const auto &v, auto *out) { if (!v.empty()) std::memcpy(out, v.data(), sizeof(v[0]) * v.size()); };
      put(in.cell_dofs, cell_dofs); put(in.cell_level, cell_level); put(in.K_of_level, K_of_level); put(P.constraint_of_dof, constraint_of_dof);
      put(in.line_ptr, line_ptr); put(in.line_master, line_master); put(in.line_weight, line_weight); put(in.line_inhomogeneity, line_inhomogeneity);
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
// ---- "Mesh tables on device" (DESIGN.md section 20): what the driver hands to gmg_build_mesh_tables for the current forest.
// sizes: n_levels, cells of all levels, level0_lexicographic
int step50_mesh_tables_on_device(step50_problem *h) { return DISPATCH(h, mesh_on_device) ? 1 : 0; }
// "Operators from resident tables" (DESIGN.md section 22): did the key take effect in the last setup_system?
int step50_operators_resident(step50_problem *h) { return DISPATCH(h, operators_resident) ? 1 : 0; }
// "Charge densities from resident tables" (DESIGN.md section 23): did the key take effect in the last setup_system?
int step50_densities_resident(step50_problem *h) { return DISPATCH(h, densities_resident) ? 1 : 0; }
// "Estimator from resident tables" (DESIGN.md section 24): did the key take effect in the last estimate?
int step50_estimator_resident(step50_problem *h) { return DISPATCH(h, estimator_resident) ? 1 : 0; }
// "Energy and forces from resident tables" (DESIGN.md section 25): did the key take effect in the last finish_cycle?
int step50_energy_forces_resident(step50_problem *h) { return DISPATCH(h, energy_forces_resident) ? 1 : 0; }
// postprocess_electrostatic_energy() of the current solution once more: the path the cycle took (its six lines are appended to the
// log, the energies of the last report are overwritten with the same values)
int step50_electrostatic_energy(step50_problem *h) {
  return guarded(h, [&] {
    auto run = [&](auto &P) {
      if (P.reports.empty() || !P.lammpsinput) throw std::runtime_error("step50_electrostatic_energy: no cycle with atoms has run");
      P.postprocess_electrostatic_energy();
    };
    if (h->dim == 2) run(*h->p2); else run(*h->p3);
    return 0;
  });
}
// the host's point_locator() of the current forest: returns its length (cells of all levels), node may be null
int64_t step50_point_locator(step50_problem *h, int32_t *node) {
  std::vector<int32_t> v;
  DISPATCH(h, point_locator(v));
  if (node && !v.empty()) std::memcpy(node, v.data(), sizeof(int32_t) * v.size());
  return (int64_t)v.size();
}
int step50_forest_sizes(step50_problem *h, int64_t sizes[3]) {
  return guarded(h, [&] {
    const auto fc = DISPATCH(h, forest_cells());
    sizes[0] = (int64_t)fc.level_ptr.size() - 1; sizes[1] = fc.level_ptr.back(); sizes[2] = fc.level0_lexicographic;
    return 0;
  });
}
int step50_forest_cells(step50_problem *h, int32_t n0[3], int64_t *level_ptr, int32_t *cell_coord, int32_t *cell_first_child) {
  return guarded(h, [&] {
    const auto fc = DISPATCH(h, forest_cells());
    auto put = [](const auto &v, auto *out) { if (!v.empty()) std::memcpy(out, v.data(), sizeof(v[0]) * v.size()); };
    for (int d = 0; d < 3; ++d) n0[d] = fc.n0[d];
    put(fc.level_ptr, level_ptr); put(fc.cell_coord, cell_coord); put(fc.cell_first_child, cell_first_child);
    return 0;
  });
}
// ---- "Refinement on device" (DESIGN.md section 21): did the last refine_grid go through the device entries; the parents of
// the forest's cells and the vertex keys of the active DoFs (beside step50_forest_cells); the marks of the last refine_grid after
// the 2:1 closure (returns their number, out may be null); and refine_grid on a given flag array [cells of all levels] -- the
// path the prm selects, the next cycle's setup_system and solution transfer included, without the cycle's assembly and solve
int step50_refined_on_device(step50_problem *h) { return DISPATCH(h, refined_on_device) ? 1 : 0; }
int step50_forest_parents(step50_problem *h, int32_t *parent) {
  auto fill = [&](auto &P) {
    size_t n = 0;
    for (const auto &lv : P.triangulation.levels)
      for (const auto &c : lv) parent[n++] = c.parent;
  };
  if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
  return 0;
}
int step50_vertex_keys(step50_problem *h, uint64_t *key) {
  const auto &v = DISPATCH(h, vertex_of_dof);
  if (!v.empty()) std::memcpy(key, v.data(), sizeof(uint64_t) * v.size());
  return 0;
}
int64_t step50_closed_flags(step50_problem *h, uint8_t *out) {
  const auto &f = DISPATCH(h, closed_refine_flags);
  if (out && !f.empty()) std::memcpy(out, f.data(), f.size());
  return (int64_t)f.size();
}
int step50_refine_with_flags(step50_problem *h, const uint8_t *flag, int64_t n, int on_device) {
  return guarded(h, [&] {
    auto run = [&](auto &P) {
      if (P.reports.empty()) throw std::runtime_error("step50_refine_with_flags: no cycle has run");
      int64_t k = 0;
      P.refine_flags.assign(P.triangulation.levels.size(), {});
      for (size_t l = 0; l < P.triangulation.levels.size(); ++l) {
        P.refine_flags[l].assign(P.triangulation.levels[l].size(), 0);
        for (auto &f : P.refine_flags[l]) f = k < n ? (char)(flag[k] != 0) : 0, ++k;
      }
      if (k != n) throw std::runtime_error("step50_refine_with_flags: one flag per cell of every level");
      P.marks_resident = false;  // (the caller's flags, not the marks the context may hold)
      P.solve_on_device_requested = on_device != 0;
      P.densities_on_device = on_device != 0 && P.par.densities_on_device;
      P.refine_grid((unsigned)P.reports.size());
    };
    if (h->dim == 2) run(*h->p2); else run(*h->p3);
    return 0;
  });
}
// ---- "RHS from cell tables" (DESIGN.md section 19): what the driver hands to gmg_assemble_rhs beyond the arrays above.
// sizes: nq, n_cells, 2^dim.  source: the charge densities as the host holds them, or rhs_function at the quadrature points
int step50_rhs_from_cell_tables(step50_problem *h) { return DISPATCH(h, rhs_from_cells) ? 1 : 0; }
int step50_rhs_assembly_sizes(step50_problem *h, int64_t sizes[3]) {
  return guarded(h, [&] {
    sizes[0] = (int64_t)DISPATCH(h, rhs_assembly_inputs(false).nq); sizes[1] = (int64_t)DISPATCH(h, active_cells.size());
    sizes[2] = (int64_t)1 << h->dim;
    return 0;
  });
}
int step50_rhs_assembly_inputs(step50_problem *h, double *shape, double *weight, double *jxw_of_level, double *source) {
  return guarded(h, [&] {
    auto fill = [&](auto &P) {
      const auto in = P.rhs_assembly_inputs(true);
      auto put = [](const auto &v, auto *out) { if (!v.empty()) std::memcpy(out, v.data(), sizeof(v[0]) * v.size()); };
      put(in.shape, shape); put(in.weight, weight); put(in.jxw_of_level, jxw_of_level); put(in.source, source);
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
// ---- "Level matrices on device" (DESIGN.md section 17): what the driver hands to gmg_assemble_level_matrix for one level of
// the current mesh.  sizes: dim, n_dofs, n_cells
int step50_level_matrices_on_device(step50_problem *h) { return DISPATCH(h, levels_on_device) ? 1 : 0; }
// "SSOR plan on device" (DESIGN.md section 26): gmg_get_ssor_plan_origin of the driver's context for one level >= 1
int step50_ssor_plan_origin(step50_problem *h, int level, int *on_device, int64_t *csr_bytes_downloaded, const char **reason) {
  gmg_context *g = DISPATCH(h, gmg);
  return g ? gmg_get_ssor_plan_origin(g, level, on_device, csr_bytes_downloaded, reason) : GMG_ERR_INVALID;
}
int step50_level_assembly_sizes(step50_problem *h, int level, int64_t sizes[3]) {
  return guarded(h, [&] {
    if (level < 0 || level >= step50_n_levels(h)) throw std::runtime_error("level_assembly_inputs: no such level");
    sizes[0] = h->dim;
    sizes[1] = (int64_t)DISPATCH(h, level_vertex_of_dof)[(size_t)level].size();
    sizes[2] = (int64_t)DISPATCH(h, level_cell_dof_table)[(size_t)level].size() >> h->dim;
    return 0;
  });
}
int step50_level_assembly_inputs(step50_problem *h, int level, int32_t *cell_dofs, double *K, uint8_t *dof_flags) {
  return guarded(h, [&] {
    if (level < 0 || level >= step50_n_levels(h)) throw std::runtime_error("level_assembly_inputs: no such level");
    auto fill = [&](auto &P) {
      const auto in = P.level_assembly_inputs(level);
      auto put = [](const auto &v, auto *out) { if (!v.empty()) std::memcpy(out, v.data(), sizeof(v[0]) * v.size()); };
      put(P.level_cell_dof_table[(size_t)level], cell_dofs); put(in.K, K); put(in.dof_flags, dof_flags);
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
// ---- the coefficient form: what the driver hands to gmg_assemble_system_matrix_coef /
// gmg_assemble_level_matrix_coef beyond the arrays above.  sizes: nq, n_cells, 2^dim, number of scales (16 / 1)
int step50_system_coefficient_sizes(step50_problem *h, int64_t sizes[4]) {
  return guarded(h, [&] {
    sizes[0] = (int64_t)DISPATCH(h, coefficient_tables().nq); sizes[1] = (int64_t)DISPATCH(h, active_cells.size());
    sizes[2] = (int64_t)1 << h->dim; sizes[3] = 16;
    return 0;
  });
}
int step50_system_coefficient_inputs(step50_problem *h, double *cell_coef, double *G, double *qw, double *scale_of_level) {
  return guarded(h, [&] {
    auto fill = [&](auto &P) {
      const auto in = P.system_coefficient_inputs();
      auto put = [](const auto &v, auto *out) { if (!v.empty()) std::memcpy(out, v.data(), sizeof(v[0]) * v.size()); };
      put(in.cell_coef, cell_coef); put(in.G, G); put(in.qw, qw); put(in.scale, scale_of_level);
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
int step50_level_coefficient_sizes(step50_problem *h, int level, int64_t sizes[4]) {
  return guarded(h, [&] {
    if (level < 0 || level >= step50_n_levels(h)) throw std::runtime_error("level_coefficient_inputs: no such level");
    sizes[0] = (int64_t)DISPATCH(h, coefficient_tables().nq);
    sizes[1] = (int64_t)DISPATCH(h, level_cell_dof_table)[(size_t)level].size() >> h->dim;
    sizes[2] = (int64_t)1 << h->dim; sizes[3] = 1;
    return 0;
  });
}
int step50_level_coefficient_inputs(step50_problem *h, int level, double *cell_coef, double *G, double *qw, double *scale) {
  return guarded(h, [&] {
    if (level < 0 || level >= step50_n_levels(h)) throw std::runtime_error("level_coefficient_inputs: no such level");
    auto fill = [&](auto &P) {
      const auto in = P.level_coefficient_inputs(level);
      auto put = [](const auto &v, auto *out) { if (!v.empty()) std::memcpy(out, v.data(), sizeof(v[0]) * v.size()); };
      put(in.cell_coef, cell_coef); put(in.G, G); put(in.qw, qw); put(in.scale, scale);
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
// the refinement marks of the cycle just estimated, all levels concatenated; returns their number (out may be null)
int64_t step50_refine_flags(step50_problem *h, uint8_t *out) {
  int64_t n = 0;
  for (auto &lv : DISPATCH(h, refine_flags))
    for (char f : lv) { if (out) out[n] = (uint8_t)(f != 0); ++n; }
  return n;
}

// ---- "Error estimator on device" (DESIGN.md section 14).  step50_estimate re-runs the estimator on the current solution
// (where: 0 the host loops, 1 gmg_estimate_error); the outputs of the last estimate; and the arrays the driver hands to
// gmg_estimate_error for the current mesh.  sizes: dim, n_cells, n_u, ng, nq, residual, densities resident on the device
// (dens is then not written: the driver passes NULL), length of dens
int step50_estimate(step50_problem *h, int where) {
  return guarded(h, [&] {
    if (DISPATCH(h, reports).empty()) throw std::runtime_error("step50_estimate: no cycle has run");
    if (where == 0) { DISPATCH(h, estimate_error_host()); return 0; }
    return DISPATCH(h, estimate_error_device());
  });
}
int step50_estimated_on_device(step50_problem *h) { return DISPATCH(h, estimated_on_device) ? 1 : 0; }
int64_t step50_host_density_copies(step50_problem *h) { return DISPATCH(h, host_density_copies); }
// how often ensure_dof_maps() built the vertex -> DoF hash tables ("Mesh tables on device" leaves them to their first use)
int64_t step50_dof_map_builds(step50_problem *h) { return DISPATCH(h, dof_map_builds); }
int step50_error_per_cell(step50_problem *h, float *eta) {
  const auto &e = DISPATCH(h, error_per_cell);
  if (!e.empty()) std::memcpy(eta, e.data(), sizeof(float) * e.size());
  return 0;
}
// the refinement marks per active cell (step50_refine_flags: per cell of every level)
int step50_marks(step50_problem *h, uint8_t *mark) {
  return guarded(h, [&] {
    auto fill = [&](auto &P) {
      if (P.refine_flags.empty()) throw std::runtime_error("step50_marks: no cells were marked (run the estimator first)");
      for (size_t a = 0; a < P.active_cells.size(); ++a)
        mark[a] = P.refine_flags[(size_t)P.active_cells[a].level][(size_t)P.active_cells[a].index] != 0;
    };
    if (h->dim == 2) fill(*h->p2); else fill(*h->p3);
    return 0;
  });
}
int step50_face_integrals(step50_problem *h, double *face_int) {
  const auto &f = DISPATCH(h, face_integrals);
  if (!f.empty()) std::memcpy(face_int, f.data(), sizeof(double) * f.size());
  return 0;
}
int step50_estimator_sizes(step50_problem *h, int64_t sizes[8]) {
  return guarded(h, [&] {
    auto fill = [&](const auto &in, int64_t n_u) {
      sizes[0] = h->dim; sizes[1] = (int64_t)in.cell_level.size(); sizes[2] = n_u; sizes[3] = (int64_t)in.gauss_x.size();
      sizes[4] = in.nq; sizes[5] = in.residual; sizes[6] = in.dens_resident ? 1 : 0; sizes[7] = (int64_t)in.dens.size();
    };
    if (h->dim == 2) fill(h->p2->estimator_inputs(), (int64_t)h->p2->vertex_of_dof.size());
    else fill(h->p3->estimator_inputs(), (int64_t)h->p3->vertex_of_dof.size());
    return 0;
  });
}
int step50_estimator_inputs(step50_problem *h, int32_t *cell_dofs, uint8_t *cell_level, uint8_t *face_kind, int32_t *face_cell, double *h_of_level,
                            double *face_measure_of_level, double *diameter_of_level, double *gauss_x, double *gauss_w, double *weight,
                            double *jxw_of_level, double *dens, double *fraction) {
  return guarded(h, [&] {
    auto fill = [&](const auto &in, int64_t) {
      auto put = [](const auto &v, auto *out) { if (!v.empty()) std::memcpy(out, v.data(), sizeof(v[0]) * v.size()); };
      put(in.cell_dofs, cell_dofs); put(in.cell_level, cell_level); put(in.face_kind, face_kind); put(in.face_cell, face_cell);
      put(in.h_of_level, h_of_level); put(in.face_measure_of_level, face_measure_of_level); put(in.diameter_of_level, diameter_of_level);
      put(in.gauss_x, gauss_x); put(in.gauss_w, gauss_w); put(in.weight, weight); put(in.jxw_of_level, jxw_of_level); put(in.dens, dens);
      *fraction = in.fraction;
    };
    if (h->dim == 2) fill(h->p2->estimator_inputs(), (int64_t)h->p2->vertex_of_dof.size());
    else fill(h->p3->estimator_inputs(), (int64_t)h->p3->vertex_of_dof.size());
    return 0;
  });
}

// ---- graphical output.  step50_output_results writes solution-CCCCC.0000.vtu, .pvtu and .visit of the
// current solution and estimate into `directory` (NULL: the prm's "Output directory"), whether or not "Output results" is set.
// step50_output_patches: the patch arrays alone, point [slots][3], solution [slots], grad_phi [slots][3] with slots =
// step50_n_cells * 2^dim (any may be null); where: 0 the host mirror, 1 the device (the resident tables where the context
// holds this cycle's and the solution, else host arrays).  step50_output_path: where the last output_results formed them
// (0 host mirror, 1 gmg_output_patches, 2 gmg_output_patches_resident)
int step50_output_results(step50_problem *h, int cycle, const char *directory) {
  return guarded(h, [&] {
    auto run = [&](auto &P) {
      if (P.reports.empty()) throw std::runtime_error("step50_output_results: no cycle has run");
      P.write_output_files((unsigned)cycle, directory ? std::string(directory) : P.par.output_directory);
    };
    if (h->dim == 2) run(*h->p2); else run(*h->p3);
    return 0;
  });
}
int step50_output_patches(step50_problem *h, int where, double *point, double *solution, double *grad_phi) {
  return guarded(h, [&] {
    auto run = [&](auto &P) {
      return P.output_patches(where == 0 ? P.kPatchesMirror : P.patches_on_device(), 0, nullptr, point, solution, grad_phi, nullptr);
    };
    return h->dim == 2 ? run(*h->p2) : run(*h->p3);
  });
}
int step50_output_path(step50_problem *h) { return h->dim == 2 ? (int)h->p2->output_path : (int)h->p3->output_path; }

// host threads of the replicated setup (one process per GPU: cores / world size)
void step50_set_threads(int n) {
#ifdef _OPENMP
  omp_set_num_threads(n > 0 ? n : 1);
#else
  (void)n;
#endif
}

// one process per GPU: rank, world size and the 128-byte id of gmg_comm_unique_id (rank 0)
int step50_set_communicator(step50_problem *h, int rank, int n_ranks, const void *id128) {
  return guarded(h, [&] {
    DISPATCH(h, set_communicator(rank, n_ranks, std::string((const char *)id128, 128)));
    return 0;
  });
}

// partition.h on one operator, for the CPU tests of the distributed layout: kind/level as in
// step50_matrix_shape.  Two calls: sizes first, then the arrays.
struct step50_local_info { int64_t n_rows, n_cols, nnz, row_begin, n_neighbors, n_send; };
static LocalOperator g_last_local;
int step50_localize(step50_problem *h, int kind, int level, int rank, int n_ranks, step50_local_info *out) {
  return guarded(h, [&] {
    const CSRMatrix *m = pick_matrix(h, kind, level);
    if (!m) return 1;
    g_last_local = localize(*m, rank, n_ranks);
    out->n_rows = g_last_local.A.n_rows; out->n_cols = g_last_local.A.n_cols; out->nnz = g_last_local.A.nnz();
    out->row_begin = g_last_local.row_begin; out->n_neighbors = (int64_t)g_last_local.halo.neighbor_rank.size();
    out->n_send = (int64_t)g_last_local.halo.send_idx.size();
    return 0;
  });
}
int step50_localize_copy(int64_t *rowptr, int32_t *col, double *val, int32_t *neighbor_rank, int32_t *send_count,
                         int32_t *send_idx, int32_t *recv_count, int64_t *ghost_global) {
  const LocalOperator &L = g_last_local;
  std::memcpy(rowptr, L.A.rowptr.data(), sizeof(int64_t) * L.A.rowptr.size());
  std::memcpy(col, L.A.col.data(), sizeof(int32_t) * L.A.col.size());
  std::memcpy(val, L.A.val.data(), sizeof(double) * L.A.val.size());
  std::memcpy(neighbor_rank, L.halo.neighbor_rank.data(), sizeof(int32_t) * L.halo.neighbor_rank.size());
  std::memcpy(send_count, L.halo.send_count.data(), sizeof(int32_t) * L.halo.send_count.size());
  std::memcpy(send_idx, L.halo.send_idx.data(), sizeof(int32_t) * L.halo.send_idx.size());
  std::memcpy(recv_count, L.halo.recv_count.data(), sizeof(int32_t) * L.halo.recv_count.size());
  std::memcpy(ghost_global, L.ghost_global.data(), sizeof(int64_t) * L.ghost_global.size());
  return 0;
}

}  // extern "C"
