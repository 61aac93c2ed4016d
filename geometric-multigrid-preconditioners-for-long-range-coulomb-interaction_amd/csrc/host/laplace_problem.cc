// laplace_problem.cc -- see laplace_problem.h.  Reference line numbers are those of
// /root/reference/src/step-50.cc unless another file is named.
#include "laplace_problem.h"
#ifdef _OPENMP
#include <omp.h>
#endif
#include "partition.h"
#include "../gmg_forces.hpp"
#include "../gmg_exact.hpp"
#include "../gmg_output.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>

namespace step50 {

// STEP50_TIMING=2: wall time of the pieces of a host phase on stderr (since the previous call; nullptr restarts the clock)
bool sublap_on() {
  static const bool on = std::getenv("STEP50_TIMING") != nullptr && std::atoi(std::getenv("STEP50_TIMING")) >= 2;
  return on;
}
void sublap(const char *what) {
  const bool on = sublap_on();
  static auto t_last = std::chrono::steady_clock::now();
  if (!on) return;
  const auto now = std::chrono::steady_clock::now();
  if (what) std::fprintf(stderr, "[step50]     . %-32s %8.3f s\n", what, std::chrono::duration<double>(now - t_last).count());
  t_last = now;
}

// ======================================================================== CSR helpers

void CSRMatrix::add(int32_t r, int32_t c, double v) {
  const int32_t *b = col.data() + rowptr[(size_t)r], *e = col.data() + rowptr[(size_t)r + 1];
  const int32_t *p = std::lower_bound(b, e, c);
  if (p == e || *p != c) throw std::logic_error("CSRMatrix::add: entry outside the sparsity pattern");
  val[(size_t)(p - col.data())] += v;
}
double CSRMatrix::l1_norm() const {
  std::vector<double> s((size_t)n_cols, 0.0);
  for (int64_t k = 0; k < nnz(); ++k) s[(size_t)col[(size_t)k]] += std::fabs(val[(size_t)k]);
  double m = 0;
  for (double v : s) m = std::max(m, v);
  return m;
}
double CSRMatrix::linfty_norm() const {
  double m = 0;
  for (int64_t i = 0; i < n_rows; ++i) {
    double s = 0;
    for (int64_t k = rowptr[(size_t)i]; k < rowptr[(size_t)i + 1]; ++k) s += std::fabs(val[(size_t)k]);
    m = std::max(m, s);
  }
  return m;
}
double CSRMatrix::frobenius_norm() const {
  double s = 0;
  for (double v : val) s += v * v;
  return std::sqrt(s);
}

namespace {

// Pattern from per-cell coupling lists: all pairs inside a list are stored entries (value 0).
CSRMatrix pattern_from_cells(int64_t n, const std::vector<int64_t> &cptr, const std::vector<int32_t> &citems) {
  const int64_t n_cells = (int64_t)cptr.size() - 1;
  std::vector<int64_t> dptr((size_t)n + 1, 0);
  for (int32_t d : citems) dptr[(size_t)d + 1]++;
  for (int64_t i = 0; i < n; ++i) dptr[(size_t)i + 1] += dptr[(size_t)i];
  std::vector<int32_t> dcells((size_t)dptr[(size_t)n]);
  {
    std::vector<int64_t> pos(dptr.begin(), dptr.end() - 1);
    for (int64_t c = 0; c < n_cells; ++c)
      for (int64_t k = cptr[(size_t)c]; k < cptr[(size_t)c + 1]; ++k) dcells[(size_t)pos[(size_t)citems[(size_t)k]]++] = (int32_t)c;
  }
  CSRMatrix A;
  A.n_rows = A.n_cols = n;
  A.rowptr.assign((size_t)n + 1, 0);
  // rows in chunks, one thread per chunk: the sorted union of the row's cell lists goes to the chunk's buffer, the buffers
  // are copied to their place once the row pointers are known (each row is sorted once)
  const int64_t chunk = 1 << 13;
  const int64_t n_chunks = (n + chunk - 1) / chunk;
  std::vector<std::vector<int32_t>> ccols((size_t)n_chunks);
#pragma omp parallel
  {
    std::vector<int32_t> tmp;
#pragma omp for schedule(dynamic, 1)
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
      std::vector<int32_t> &out = ccols[(size_t)ch];
      const int64_t i1 = std::min(n, (ch + 1) * chunk);
      out.reserve((size_t)(i1 - ch * chunk) * 27);
      for (int64_t i = ch * chunk; i < i1; ++i) {
        tmp.clear();
        for (int64_t q = dptr[(size_t)i]; q < dptr[(size_t)i + 1]; ++q) {
          const int32_t c = dcells[(size_t)q];
          tmp.insert(tmp.end(), citems.begin() + cptr[(size_t)c], citems.begin() + cptr[(size_t)c + 1]);
        }
        std::sort(tmp.begin(), tmp.end());
        const auto e = std::unique(tmp.begin(), tmp.end());
        A.rowptr[(size_t)i + 1] = e - tmp.begin();
        out.insert(out.end(), tmp.begin(), e);
      }
    }
  }
  for (int64_t i = 0; i < n; ++i) A.rowptr[(size_t)i + 1] += A.rowptr[(size_t)i];
  A.col.resize((size_t)A.rowptr[(size_t)n]);
  A.val.assign((size_t)A.rowptr[(size_t)n], 0.0);
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t ch = 0; ch < n_chunks; ++ch) {
    std::copy(ccols[(size_t)ch].begin(), ccols[(size_t)ch].end(), A.col.begin() + A.rowptr[(size_t)(ch * chunk)]);
    std::vector<int32_t>().swap(ccols[(size_t)ch]);
  }
  return A;
}

CSRMatrix csr_from_triplets(int64_t n_rows, int64_t n_cols, std::vector<std::array<int64_t, 2>> &rc, std::vector<double> &v,
                            bool sum_duplicates) {
  std::vector<size_t> order(rc.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return rc[a] < rc[b]; });
  CSRMatrix A;
  A.n_rows = n_rows; A.n_cols = n_cols;
  A.rowptr.assign((size_t)n_rows + 1, 0);
  for (size_t q = 0; q < order.size(); ++q) {
    const size_t i = order[q];
    if (q > 0 && rc[i] == rc[order[q - 1]]) {
      if (sum_duplicates) A.val.back() += v[i];
      continue;  // "set" semantics: first writer wins, later ones are identical
    }
    A.col.push_back((int32_t)rc[i][1]);
    A.val.push_back(v[i]);
    A.rowptr[(size_t)rc[i][0] + 1]++;
  }
  for (int64_t i = 0; i < n_rows; ++i) A.rowptr[(size_t)i + 1] += A.rowptr[(size_t)i];
  return A;
}

// Gauss-Legendre on [0,1]
void gauss01(int n, std::vector<double> &x, std::vector<double> &w) {
  x.resize((size_t)n); w.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5)), pp = 0;
    for (int it = 0; it < 100; ++it) {
      double p1 = 1, p2 = 0;
      for (int j = 1; j <= n; ++j) { const double p3 = p2; p2 = p1; p1 = ((2.0 * j - 1) * z * p2 - (j - 1.0) * p3) / j; }
      pp = n * (z * p1 - p2) / (z * z - 1);
      const double dz = p1 / pp;
      z -= dz;
      if (std::fabs(dz) < 1e-16) break;
    }
    x[(size_t)(n - 1 - i)] = 0.5 * (z + 1);
    w[(size_t)(n - 1 - i)] = 1.0 / ((1 - z * z) * pp * pp);
  }
}

template <int dim>
struct Quadrature {  // QGauss<dim>(n), tensor product with x fastest
  std::vector<std::array<double, 3>> p;
  std::vector<double> w;
  std::vector<std::array<double, 1 << dim>> shape;                       // [q][i]
  std::vector<std::array<std::array<double, 3>, 1 << dim>> grad;        // [q][i][d], unit cell
  explicit Quadrature(int n) {
    std::vector<double> x1, w1;
    gauss01(n, x1, w1);
    const int nz = dim == 3 ? n : 1;
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
          p.push_back({x1[(size_t)i], x1[(size_t)j], dim == 3 ? x1[(size_t)k] : 0.0});
          w.push_back(w1[(size_t)i] * w1[(size_t)j] * (dim == 3 ? w1[(size_t)k] : 1.0));
        }
    shape.resize(p.size()); grad.resize(p.size());
    for (size_t q = 0; q < p.size(); ++q)
      for (int a = 0; a < (1 << dim); ++a) {
        double f[3], df[3];
        for (int d = 0; d < dim; ++d) {
          const int b = (a >> d) & 1;
          f[d] = b ? p[q][(size_t)d] : 1.0 - p[q][(size_t)d];
          df[d] = b ? 1.0 : -1.0;
        }
        double v = 1;
        for (int d = 0; d < dim; ++d) v *= f[d];
        shape[q][(size_t)a] = v;
        for (int e = 0; e < 3; ++e) {
          double g = 0;
          if (e < dim) { g = 1; for (int d = 0; d < dim; ++d) g *= (d == e) ? df[d] : f[d]; }
          grad[q][(size_t)a][(size_t)e] = g;
        }
      }
  }
};

std::string fmt(const char *f, double v) {
  char buf[64];
  std::snprintf(buf, sizeof buf, f, v);
  return buf;
}

}  // namespace

// ======================================================================== parameters

void ParameterReader::declare_parameters() {
  values = {{"Number of global refinement", "2"}, {"Domain limit left", "-1"}, {"Domain limit right", "1"},
            {"Mesh size", "0.25"}, {"Vacuum repetitions", "1"}, {"Problem", "Step16"}, {"Dimension", "2"},
            {"Boundary conditions selection", "Inhomogeneous"}, {"Number of Adaptive Refinement", "2"},
            {"smoothing length", "0.5"}, {"Nonzero Density radius parameter around each charge", "3"},
            {"Output and calculation of Analytical solution", "false"}, {"Output of RHS field", "false"},
            {"Output of support of each atom", "false"}, {"Flag for RHS evaluation optimization", "false"},
            {"Quadrature points for RHS function", "1"}, {"Output time summary table", "true"},
            {"Polynomial degree", "1"}, {"Preconditioner", "GMG"}, {"Lammps input file", "atom_8.data"},
            // additions of this build (the reference selects the smoother by editing :969-970)
            {"Smoother", "SSOR"}, {"Smoother damping", "0.5"}, {"Smoother steps", "2"}, {"Chebyshev degree", "2"},
            // the Chebyshev smoother's polynomial and its bound of lambda_max(D^-1 A) (gmg_set_chebyshev)
            {"Chebyshev polynomial", "first kind"}, {"Chebyshev eigenvalue estimate", "Gershgorin"}, {"Chebyshev Lanczos steps", "10"},
            {"Chebyshev safety factor", "1.2"},
            {"Device resident outer CG", "false"}, {"SSOR blocks", "1"}, {"SSOR block partition", "equal rows"}, {"Charge densities on device", "true"},
            {"Partition level 0", "auto"},
            // HEAD marks with Kelly + the cell residual (:1040-1089); the cluster logs (January 2018) are reproduced by
            // the Kelly indicator alone (tools/marking_rule_scan.py)
            {"Refinement estimator", "Kelly + residual"},
            // level 0 is the undivided lattice: numbered lexicographically (x fastest) its operator is a pure 27-point
            // stencil for the device's plane-by-plane kernel; "cell-wise" = deal.II's first-touch order on level 0 as well
            {"Level 0 numbering", "lexicographic"},
            // the level-0 matrix formed on the device from (lattice size, cell matrix) instead of assembled here and uploaded
            // as CSR (gmg_set_level_matrix_lattice; 3D constant-coefficient problems with a lexicographic, unpartitioned level 0)
            {"Level 0 matrix on device", "true"},
            // the active-mesh system matrix formed on the device from the cells' DoFs, the per-level cell matrix and the
            // constraint lines (gmg_assemble_system_matrix) instead of assembled here and uploaded as CSR; one rank, DESIGN.md
            // section 12 (Step16: the coefficient's values at the quadrature points instead of cell matrices, section 18)
            {"System matrix on device", "false"},
            // the level matrices A_l and the interface matrices I_l formed on the device from the levels' cell tables, one
            // cell matrix and the boundary / refinement-edge flags (gmg_assemble_level_matrix) instead of assembled here and
            // uploaded as CSR; one rank, DESIGN.md section 17 (Step16: section 18)
            {"Level matrices on device", "false"},
            // the SSOR plan of every level >= 1 formed on the device from the level's CSR (option ssor_plan_device of the context)
            // where the default four-wave plan applies, else by the host as without the key; DESIGN.md section 26
            {"SSOR plan on device", "false"},
            // what stands behind mg_coarse: the reference's unpreconditioned CG (:962-967), or fast diagonalisation on the
            // level-0 lattice (gmg_set_coarse_solver; where level 0 does not qualify the CG stays), DESIGN.md section 15
            {"Coarse solver", "CG"},
            // the error estimator and the refinement marks formed on the device from a face table of the forest and the
            // solution (gmg_estimate_error) instead of the host loops of estimate_error_and_mark_cells; cycles that ran on
            // the device, one rank, DESIGN.md section 14
            {"Error estimator on device", "false"},
            // MGTransferPrebuilt::build_matrices on the device (gmg_build_transfer) instead of here + upload
            {"Transfer matrices on device", "true"},
            // the right-hand side integrated on the device from densities that stay there (gmg_rhs_assemble)
            {"RHS on device", "true"},
            // the right-hand side formed on the device from the cell tables the matrix assembly takes (gmg_assemble_rhs) instead
            // of the sequential cell loop and its gather plan, and constraints.distribute of the solution on the device
            // (gmg_distribute_constraints), whose vector the estimator, the forces and the error norm then take; cycles that
            // run on the device, one rank, DESIGN.md section 19
            {"RHS from cell tables", "false"},
            // gmg_build_mesh_tables instead of the sequential loops of distribute_dofs and make_constraints: DoF numbering of the
            // active mesh and of every level, hanging-node and Dirichlet lines, level flags; boundary values and close() stay
            // here; cycles that run on the device, one rank, DESIGN.md section 20
            {"Mesh tables on device", "false"},
            // gmg_close_constraints and the _resident entries: the system matrix, the level matrices, the right-hand side and
            // constraints.distribute read the tables gmg_build_mesh_tables left on the device instead of taking them back as
            // host arrays; cycles in which "Mesh tables on device" took effect, with "System matrix on device", "Level matrices
            // on device" and "RHS from cell tables" set, DESIGN.md section 22
            {"Operators from resident tables", "false"},
            // gmg_charge_density_resident: the densities of the active cells from the tables gmg_build_mesh_tables left on the
            // device instead of per-cell corner / edge / root arrays built here and uploaded; cycles in which "Mesh tables on
            // device" took effect, with "Charge densities on device" set, 3D LAMMPS input, one rank, DESIGN.md section 23
            {"Charge densities from resident tables", "false"},
            // gmg_build_face_table_resident, gmg_estimate_error_resident, gmg_refine_forest_marked and
            // gmg_energy_norm_error_resident: the face table, the marks and the cells of the error norm stay on the device next
            // to the tables; cycles in which "Operators from resident tables" took effect, with "Error estimator on device" and
            // "Refinement on device" set, one rank, DESIGN.md section 24
            {"Estimator from resident tables", "false"},
            // gmg_build_point_locator_resident, gmg_electrostatic_energy_resident and gmg_atom_forces_resident: the point
            // locator is formed on the device next to the tables, the energy's three sums and the forces at the atoms read
            // cell_dofs and the solution there; cycles in which "Operators from resident tables" took effect with the solution
            // on the device ("RHS from cell tables"), 3D LAMMPS input, one rank, DESIGN.md section 25
            {"Energy and forces from resident tables", "false"},
            // gmg_refine_forest (2:1 closure of the marks and the split), gmg_transfer_solution (SolutionTransfer::interpolate
            // and constraints.set_zero) and gmg_build_face_table (the estimator's face table) instead of Forest::refine_flagged,
            // the interpolation loop of refine_grid and face_table; cycles that run on the device, one rank, DESIGN.md section 21
            {"Refinement on device", "false"},
            // the short-ranged pair sum over the pairs closer than this many smoothing lengths, found through
            // cell bins (erfc(6) = 2e-17: beyond 6 r_c a pair contributes nothing in double precision); 0 = all pairs as the
            // reference (:1325-1332).  With it the energy is also evaluated for the large systems the reference skips (:1554).
            {"Short-range cutoff in smoothing lengths", "0"}, {"Energy for large systems", "false"},
            // forces on the atoms after the energy (LAMMPS input, 3D), and with them the exact all-pairs
            // Coulomb forces and the relative RMS error against them
            {"Compute forces", "false"}, {"Direct Coulomb check", "false"},
            // the exact free-space potential summed over all atoms in batches (gmg_exact.hpp): the
            // Exact boundary values and the error norm on the device (or by its host mirror), and with it the error norm
            // beyond the reference's 300-atom gate (:1554-1556)
            {"Analytical solution on device", "false"}, {"Error norm for large systems", "false"},
            // the reference's output_results (:1149-1308) after every cycle's estimate: solution-CCCCC.0000.vtu with the
            // potential, grad_phi = -grad phi_h, the indicators and, on request of the reference's three output keys, the
            // analytical solution, the interpolated right-hand side and the atoms' supports; a .pvtu and a .visit record beside
            // it.  The patches are formed on the device where the cycle ran there (gmg_output_patches)
            {"Output results", "false"}, {"Output directory", "."}};
}
void ParameterReader::parse_input_from_string(const std::string &text) {
  std::istringstream in(text);
  std::string line;
  while (std::getline(in, line)) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    const size_t s = line.find("set ");
    if (s == std::string::npos) continue;
    const size_t eq = line.find('=', s);
    if (eq == std::string::npos) continue;
    auto trim = [](std::string t) {
      const size_t a = t.find_first_not_of(" \t\r"), b = t.find_last_not_of(" \t\r");
      return a == std::string::npos ? std::string() : t.substr(a, b - a + 1);
    };
    const std::string key = trim(line.substr(s + 4, eq - s - 4));
    if (!values.count(key)) throw std::runtime_error("ParameterHandler: undeclared entry <" + key + ">");
    values[key] = trim(line.substr(eq + 1));
  }
}
void ParameterReader::read_parameters(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("cannot open parameter file " + file);
  std::stringstream ss;
  ss << in.rdbuf();
  parse_input_from_string(ss.str());
}
std::string ParameterReader::get(const std::string &k) const { return values.at(k); }
double ParameterReader::get_double(const std::string &k) const { return std::stod(values.at(k)); }
long ParameterReader::get_integer(const std::string &k) const { return std::stol(values.at(k)); }
bool ParameterReader::get_bool(const std::string &k) const { return values.at(k) == "true"; }

Parameters Parameters::from(const ParameterReader &prm) {  // src/main.cc:25-68
  Parameters p;
  p.number_of_global_refinement = (unsigned)prm.get_integer("Number of global refinement");
  p.domain_size_left = prm.get_double("Domain limit left");
  p.domain_size_right = prm.get_double("Domain limit right");
  p.mesh_size_h = prm.get_double("Mesh size");
  p.repetitions_for_vacuum = (unsigned)prm.get_integer("Vacuum repetitions");
  p.number_of_adaptive_refinement_cycles = (unsigned)prm.get_integer("Number of Adaptive Refinement");
  p.r_c = prm.get_double("smoothing length");
  p.nonzero_density_radius_parameter = prm.get_double("Nonzero Density radius parameter around each charge");
  p.flag_analytical_solution = prm.get_bool("Output and calculation of Analytical solution");
  p.flag_rhs_field = prm.get_bool("Output of RHS field");
  p.flag_atoms_support = prm.get_bool("Output of support of each atom");
  p.flag_rhs_assembly = prm.get_bool("Flag for RHS evaluation optimization");
  p.quadrature_degree_rhs = (unsigned)prm.get_integer("Quadrature points for RHS function");
  p.flag_output_time = prm.get_bool("Output time summary table");
  p.degree = (unsigned)prm.get_integer("Polynomial degree");
  p.PreconditionerType = prm.get("Preconditioner");
  p.Problemtype = prm.get("Problem");
  p.dim = (int)prm.get_integer("Dimension");
  p.Boundary_conditions = prm.get("Boundary conditions selection");
  p.LammpsInputFile = prm.get("Lammps input file");
  p.smoother = prm.get("Smoother");
  p.smoother_omega = prm.get_double("Smoother damping");
  p.smoother_steps = (int)prm.get_integer("Smoother steps");
  p.chebyshev_degree = (int)prm.get_integer("Chebyshev degree");
  p.chebyshev_polynomial = prm.get("Chebyshev polynomial");
  if (p.chebyshev_polynomial != "first kind" && p.chebyshev_polynomial != "fourth kind")
    throw std::runtime_error("Chebyshev polynomial must be <first kind> or <fourth kind>");
  p.chebyshev_estimate = prm.get("Chebyshev eigenvalue estimate");
  if (p.chebyshev_estimate != "Gershgorin" && p.chebyshev_estimate != "Lanczos")
    throw std::runtime_error("Chebyshev eigenvalue estimate must be <Gershgorin> or <Lanczos>");
  p.chebyshev_lanczos_steps = (int)prm.get_integer("Chebyshev Lanczos steps");
  if (p.chebyshev_lanczos_steps < 1 || p.chebyshev_lanczos_steps > 64) throw std::runtime_error("Chebyshev Lanczos steps must be 1 .. 64");
  p.chebyshev_safety = prm.get_double("Chebyshev safety factor");
  if (!(p.chebyshev_safety >= 1.0)) throw std::runtime_error("Chebyshev safety factor must be >= 1");
  p.device_resident_outer_cg = prm.get_bool("Device resident outer CG");
  p.ssor_blocks = (int)prm.get_integer("SSOR blocks");
  p.ssor_partition = prm.get("SSOR block partition");
  if (p.ssor_partition != "equal rows" && p.ssor_partition != "balanced")
    throw std::runtime_error("SSOR block partition must be <equal rows> or <balanced>");
  p.densities_on_device = prm.get_bool("Charge densities on device");
  p.partition_level0 = prm.get("Partition level 0");
  p.refinement_estimator = prm.get("Refinement estimator");
  if (p.refinement_estimator != "Kelly + residual" && p.refinement_estimator != "Kelly")
    throw std::runtime_error("Refinement estimator must be <Kelly + residual> or <Kelly>");
  p.level0_matrix_on_device = prm.get_bool("Level 0 matrix on device");
  p.system_matrix_on_device = prm.get_bool("System matrix on device");
  p.level_matrices_on_device = prm.get_bool("Level matrices on device");
  p.ssor_plan_on_device = prm.get_bool("SSOR plan on device");
  p.coarse_solver = prm.get("Coarse solver");
  if (p.coarse_solver != "CG" && p.coarse_solver != "direct") throw std::runtime_error("Coarse solver must be <CG> or <direct>");
  p.estimator_on_device = prm.get_bool("Error estimator on device");
  p.transfer_on_device = prm.get_bool("Transfer matrices on device");
  p.rhs_on_device = prm.get_bool("RHS on device");
  p.rhs_from_cell_tables = prm.get_bool("RHS from cell tables");
  p.mesh_tables_on_device = prm.get_bool("Mesh tables on device");
  p.operators_from_resident_tables = prm.get_bool("Operators from resident tables");
  p.densities_from_resident_tables = prm.get_bool("Charge densities from resident tables");
  p.estimator_from_resident_tables = prm.get_bool("Estimator from resident tables");
  p.energy_forces_from_resident_tables = prm.get_bool("Energy and forces from resident tables");
  p.refinement_on_device = prm.get_bool("Refinement on device");
  p.short_range_cutoff = prm.get_double("Short-range cutoff in smoothing lengths");
  p.energy_for_large_systems = prm.get_bool("Energy for large systems");
  p.compute_forces = prm.get_bool("Compute forces");
  p.direct_coulomb_check = prm.get_bool("Direct Coulomb check");
  p.analytical_on_device = prm.get_bool("Analytical solution on device");
  p.error_norm_for_large_systems = prm.get_bool("Error norm for large systems");
  p.output_results = prm.get_bool("Output results");
  p.output_directory = prm.get("Output directory");
  p.level0_numbering = prm.get("Level 0 numbering");
  if (p.level0_numbering != "lexicographic" && p.level0_numbering != "cell-wise")
    throw std::runtime_error("Level 0 numbering must be <lexicographic> or <cell-wise>");
  return p;
}

std::vector<double> nacl_lattice(int n, std::vector<double> &q) {
  // atom/atom_n{1,3,5,7,10,20}_*.data of the reference: n^3 unit cells of 8 ions, spacing 0.5,
  // cells ordered x outermost, z innermost (verified against the files, tests/test_host.py)
  static const double base[8][3] = {{0, 0, 0}, {.5, 0, 0}, {.5, .5, 0}, {0, .5, 0}, {.5, 0, .5}, {0, 0, .5}, {0, .5, .5}, {.5, .5, .5}};
  std::vector<double> x;
  q.clear();
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      for (int c = 0; c < n; ++c)
        for (int k = 0; k < 8; ++k) {
          x.push_back(base[k][0] + a); x.push_back(base[k][1] + b); x.push_back(base[k][2] + c);
          q.push_back(k % 2 == 0 ? 1.0 : -1.0);
        }
  return x;
}

// ======================================================================== atoms

template <int dim>
struct LaplaceProblem<dim>::AtomBins {
  double lo[3] = {0, 0, 0}, size = 1;
  int n[3] = {1, 1, 1};
  std::vector<int64_t> ptr;
  std::vector<int32_t> items;
};

template <int dim>
LaplaceProblem<dim>::LaplaceProblem(const Parameters &p) : par(p) {
  if (p.degree != 1) throw std::runtime_error("only Q1 elements (Polynomial degree = 1) are supported");
  pcout("Problem type is:   " + par.Problemtype);
  pcout("Preconditioner :    " + par.PreconditionerType);
  pcout(par.flag_rhs_assembly ? "Rhs assembly optimization ENABLED" : "Without rhs assembly optimization");
}

template <int dim>
LaplaceProblem<dim>::~LaplaceProblem() {
  if (gmg) {
    for (double *p : {d_solution, d_rhs, d_full})
      if (p) gmg_vec_free(gmg, p);
    gmg_destroy(gmg);
  }
}

template <int dim>
void LaplaceProblem<dim>::pcout(const std::string &s) {
  log += s;
  log += '\n';
  if (echo) std::cout << s << std::endl;
}

template <int dim>
void LaplaceProblem<dim>::read_lammps_input_file(const std::string &filename) {
  // token-counting reader of :181-258: token #2 = number of atoms, token #35 starts the records
  if (dim != 3) {
    lammpsinput = false;
    pcout("\nReading of Lammps input file implemented for 3D only\n");
    return;
  }
  std::ifstream file(filename);
  if (!file.is_open()) {
    lammpsinput = false;
    pcout("Unable to open the file.");
    return;
  }
  lammpsinput = true;
  std::string tok;
  unsigned int count = 0;
  while (!file.eof()) {
    if (count == 2) {
      file >> number_of_atoms;
      pcout("Number of atoms: " + std::to_string(number_of_atoms));
      charges.resize(number_of_atoms);
      atom_positions.resize(3 * (size_t)number_of_atoms);
    } else if (count == 35) {
      for (unsigned int i = 0; i < number_of_atoms; ++i) {
        double a, b, type;
        file >> a >> b >> type >> charges[i] >> atom_positions[3 * i] >> atom_positions[3 * i + 1] >> atom_positions[3 * i + 2];
      }
    } else {
      file >> tok;
    }
    ++count;
  }
}

template <int dim>
void LaplaceProblem<dim>::set_atoms(const std::vector<double> &q, const std::vector<double> &xyz) {
  charges = q;
  atom_positions = xyz;
  number_of_atoms = (unsigned)q.size();
  lammpsinput = true;
  pcout("Number of atoms: " + std::to_string(number_of_atoms));
}

template <int dim>
void LaplaceProblem<dim>::rhs_assembly_optimization() {
  // :260-306 keeps, per cell, the atoms with ANY cell vertex closer than cutoff * r_c; children
  // inherit the list unchanged (:441-450), so the list is a function of the root cell alone.
  // Instead of the O(cells x atoms) scan the atoms are binned once; atoms_of_root_cell()
  // evaluates the same predicate on the candidates of the neighbouring bins.
  bins.reset(new AtomBins());
  AtomBins &B = *bins;
  const double cut = par.nonzero_density_radius_parameter * par.r_c;
  double hi[3];
  for (int d = 0; d < 3; ++d) { B.lo[d] = 1e300; hi[d] = -1e300; }
  for (unsigned i = 0; i < number_of_atoms; ++i)
    for (int d = 0; d < 3; ++d) {
      B.lo[d] = std::min(B.lo[d], atom_positions[3 * i + (size_t)d]);
      hi[d] = std::max(hi[d], atom_positions[3 * i + (size_t)d]);
    }
  B.size = std::max(cut, 1e-12);
  int64_t total = 1;
  for (int d = 0; d < 3; ++d) { B.n[d] = std::max(1, (int)std::floor((hi[d] - B.lo[d]) / B.size) + 1); total *= B.n[d]; }
  B.ptr.assign((size_t)total + 1, 0);
  auto bin_of = [&](unsigned i) {
    int b[3];
    for (int d = 0; d < 3; ++d) b[d] = std::min(B.n[d] - 1, std::max(0, (int)std::floor((atom_positions[3 * i + (size_t)d] - B.lo[d]) / B.size)));
    return (int64_t)b[0] + B.n[0] * ((int64_t)b[1] + (int64_t)B.n[1] * b[2]);
  };
  for (unsigned i = 0; i < number_of_atoms; ++i) B.ptr[(size_t)bin_of(i) + 1]++;
  for (int64_t b = 0; b < total; ++b) B.ptr[(size_t)b + 1] += B.ptr[(size_t)b];
  B.items.resize(number_of_atoms);
  std::vector<int64_t> pos(B.ptr.begin(), B.ptr.end() - 1);
  for (unsigned i = 0; i < number_of_atoms; ++i) B.items[(size_t)pos[(size_t)bin_of(i)]++] = (int32_t)i;
}

template <int dim>
void LaplaceProblem<dim>::atoms_of_root_cell(const int rc[3], std::vector<int32_t> &out) const {
  out.clear();
  const AtomBins &B = *bins;
  const double cut = par.nonzero_density_radius_parameter * par.r_c;
  const double h = triangulation.h0;
  double lo[3], hi[3];
  int b0[3], b1[3];
  for (int d = 0; d < 3; ++d) {
    lo[d] = triangulation.origin + h * rc[d];
    hi[d] = triangulation.origin + h * (rc[d] + 1);
    b0[d] = (int)std::floor((lo[d] - cut - B.lo[d]) / B.size);
    b1[d] = (int)std::floor((hi[d] + cut - B.lo[d]) / B.size);
    b0[d] = std::max(b0[d], 0);
    b1[d] = std::min(b1[d], B.n[d] - 1);
  }
  for (int z = b0[2]; z <= b1[2]; ++z)
    for (int y = b0[1]; y <= b1[1]; ++y)
      for (int x = b0[0]; x <= b1[0]; ++x) {
        const int64_t b = (int64_t)x + B.n[0] * ((int64_t)y + (int64_t)B.n[1] * z);
        for (int64_t k = B.ptr[(size_t)b]; k < B.ptr[(size_t)b + 1]; ++k) {
          const int32_t i = B.items[(size_t)k];
          double d2 = 0;
          for (int d = 0; d < 3; ++d) {  // nearest vertex, direction by direction
            const double a = atom_positions[3 * (size_t)i + (size_t)d];
            const double dl = a - lo[d], dh = a - hi[d];
            const double m = std::fabs(dl) <= std::fabs(dh) ? dl : dh;
            d2 += m * m;
          }
          if (std::sqrt(d2) < cut) out.push_back(i);
        }
      }
  std::sort(out.begin(), out.end());  // std::set iteration order of the reference (:559-560)
}

// ======================================================================== problem functions

template <int dim>
double LaplaceProblem<dim>::coefficient(const double x[3]) const {
  if (par.Problemtype == "Step16") {  // include/step_50.h:246-254
    double s = 0;
    for (int d = 0; d < dim; ++d) s += x[d] * x[d];
    return s < 0.25 ? 5.0 : 1.0;
  }
  return 1.0;
}

template <int dim>
double LaplaceProblem<dim>::rhs_function(const double x[3]) const {
  if (par.Problemtype == "Step16") return 10.0;  // include/step_50.h:240-244
  double s = 0;                                   // include/step_50.h:321-329
  for (int d = 0; d < dim; ++d) s += x[d] * x[d];
  const double c = s / (par.r_c * par.r_c);
  return (8.0 * std::exp(-4.0 * c) - std::exp(-c)) / (std::pow(par.r_c, 3) * std::pow(M_PI, 1.5));
}

template <int dim>
double LaplaceProblem<dim>::boundary_value(const double x[3]) const {
  if (par.Boundary_conditions == "Homogeneous") return 0.0;
  if (par.Boundary_conditions == "Exact") {  // Analytical_Solution::value, include/step_50.h:338-353
    if (par.Problemtype != "GaussianCharges") return 0.0;
    double v = 0;
    const double inv = 1.0 / (std::sqrt(M_PI) * par.r_c);
    for (unsigned i = 0; i < number_of_atoms; ++i) {
      double r2 = 0;
      for (int d = 0; d < dim; ++d) { const double t = x[d] - atom_positions[3 * i + (size_t)d]; r2 += t * t; }
      const double r = std::sqrt(r2);
      v += r < 1e-10 ? charges[i] * 2.0 * inv : charges[i] * (std::erf(r / par.r_c) / r);
    }
    return v;
  }
  // Inhomogeneous: NonZeroDBC with x0 = 0, dipole p0, quadrupole forced to 0 (:623-624, step_50.h:378-385)
  double r2 = 0, px = 0;
  for (int d = 0; d < dim; ++d) { r2 += x[d] * x[d]; px += dipole_moment[d] * x[d]; }
  const double r = std::sqrt(r2);
  return px / std::pow(r, 3) + (0.5 * 0.0) / std::pow(r, 5);
}

// ======================================================================== mesh + DoFs

template <int dim>
void LaplaceProblem<dim>::make_initial_grid() {
  if (par.Problemtype == "Step16") {  // :1496-1497
    triangulation.create_lattice(1, par.domain_size_left, par.domain_size_right - par.domain_size_left);
    triangulation.refine_global((int)par.number_of_global_refinement);
  } else {  // :1504-1526
    const double a = 2 * par.mesh_size_h;
    const double N = (par.domain_size_right - par.domain_size_left) / a;
    const double M = par.repetitions_for_vacuum;
    const unsigned int reps = (unsigned int)(2 * (N + 2 * M));
    const double lo = par.domain_size_left - M * a, hi = par.domain_size_right + M * a;
    if (std::pow((double)reps, dim) > 2.0e8) throw std::runtime_error("initial lattice too large for this host");
    // "Need to set #Global_ref = 0" (:1503): the reference applies no global refinement here
    triangulation.create_lattice((int)reps, lo, (hi - lo) / reps);
  }
}

template <int dim>
void LaplaceProblem<dim>::cell_dofs(const ActiveCell &c, int32_t *out) const {
  // (tables filled by distribute_dofs: the assembly, the estimator and the transfer loops ask for the same cell again and again,
  // and a hash look-up per vertex was a third of assemble_system)
  const int32_t *t = &active_cell_dof_table[(size_t)active_index_of_cell[(size_t)c.level][(size_t)c.index] * (1 << dim)];
  for (int a = 0; a < (1 << dim); ++a) out[a] = t[a];
}
template <int dim>
void LaplaceProblem<dim>::level_cell_dofs(int level, int32_t ci, int32_t *out) const {
  const int32_t *t = &level_cell_dof_table[(size_t)level][(size_t)ci * (1 << dim)];
  for (int a = 0; a < (1 << dim); ++a) out[a] = t[a];
}

template <int dim>
void LaplaceProblem<dim>::distribute_dofs() {
  // DoFs are numbered in the order cells meet their vertices: active cells by (level, index) for
  // the active mesh, all cells of a level by index for the level DoFs.
  const int L = triangulation.n_levels();
  active_cells.clear();
  sublap(nullptr);
  active_index_of_cell.assign((size_t)L, {});
  for (int l = 0; l < L; ++l) {
    active_index_of_cell[(size_t)l].assign(triangulation.levels[(size_t)l].size(), -1);
    for (size_t c = 0; c < triangulation.levels[(size_t)l].size(); ++c)
      if (triangulation.levels[(size_t)l][c].first_child < 0) {
        active_index_of_cell[(size_t)l][c] = (int32_t)active_cells.size();
        active_cells.push_back({l, (int32_t)c});
      }
  }
  // (level-0 vertices index a dense array by lattice position, the others a hash table: flat_map.h)
  const int lattice[3] = {triangulation.n0 + 1, triangulation.n0 + 1, dim == 3 ? triangulation.n0 + 1 : 1};
  dof_of_vertex.reset(kMaxLevelShift, lattice);
  vertex_of_dof.clear();
  sublap("dofs: active cell list");
  mesh_on_device = decide_mesh_tables_on_device();
  if (mesh_on_device) { distribute_dofs_on_device(); return; }
  dof_maps_ready = true;
  dof_of_vertex.reserve_sparse(active_cells.size() - (size_t)std::min<int64_t>((int64_t)active_cells.size(), (int64_t)triangulation.levels[0].size()));
  active_cell_dof_table.resize(active_cells.size() * (size_t)(1 << dim));
  size_t slot = 0;
  for (const ActiveCell &ac : active_cells) {
    const Cell &cell = triangulation.levels[(size_t)ac.level][(size_t)ac.index];
    for (int a = 0; a < (1 << dim); ++a) {
      const uint64_t key = triangulation.vertex_key(ac.level, cell, a);
      const auto ins = dof_of_vertex.emplace(key, (int32_t)vertex_of_dof.size());
      if (ins.second) vertex_of_dof.push_back(key);
      active_cell_dof_table[slot++] = *ins.first;
    }
  }
  level_dof_of_vertex.assign((size_t)L, {});
  sublap("dofs: active numbering");
  level_vertex_of_dof.assign((size_t)L, {});
  level_cell_dof_table.assign((size_t)L, {});
  for (int l = 0; l < L; ++l) {
    auto &map = level_dof_of_vertex[(size_t)l];
    auto &vec = level_vertex_of_dof[(size_t)l];
    auto &tab = level_cell_dof_table[(size_t)l];
    const int none[3] = {0, 0, 0};
    map.reset(kMaxLevelShift, l == 0 ? lattice : none);
    if (l > 0) map.reserve_sparse(triangulation.levels[(size_t)l].size() * 2);
    tab.resize(triangulation.levels[(size_t)l].size() * (size_t)(1 << dim));
    if (l == 0 && par.level0_numbering == "lexicographic") {
      // Level 0 is the undivided lattice (subdivided_hyper_rectangle, src/step-50.cc:1526) and carries no smoother: its
      // numbering only permutes rows / columns of A_0, P_0 and the copy indices (results change in the last bits of a few
      // sums).  Vertex keys order by (z, y, x): ascending keys = lexicographic DoFs, and A_0 becomes a pure 27-point stencil
      // with strides 1, nx, nx ny -- what the device's plane-by-plane kernel (csrc/gmg_lattice.hpp) wants.  deal.II's real
      // level numbering on the reference's p4est partition is not reproducible here either way.
      // DoF of a vertex = its lattice position: no table is searched, no key is sorted.
      const int64_t nx = lattice[0], ny = lattice[1], nz = lattice[2];
      vec.resize((size_t)(nx * ny * nz));
#pragma omp parallel for schedule(static)
      for (int64_t k = 0; k < nz; ++k)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const uint64_t key = pack3((uint64_t)i << kMaxLevelShift, (uint64_t)j << kMaxLevelShift, (uint64_t)k << kMaxLevelShift);
            vec[(size_t)(i + nx * (j + ny * k))] = key;
          }
      for (size_t i = 0; i < vec.size(); ++i) map.emplace(vec[i], (int32_t)i);
      const auto &cells = triangulation.levels[0];
#pragma omp parallel for schedule(static)
      for (int64_t c = 0; c < (int64_t)cells.size(); ++c)
        for (int a = 0; a < (1 << dim); ++a) {
          const Cell &cell = cells[(size_t)c];
          tab[(size_t)c * (size_t)(1 << dim) + (size_t)a] =
              (int32_t)((cell.c[0] + (a & 1)) + nx * ((cell.c[1] + ((a >> 1) & 1)) + ny * (dim == 3 ? cell.c[2] + ((a >> 2) & 1) : 0)));
        }
      continue;
    }
    size_t ls = 0;
    for (const Cell &cell : triangulation.levels[(size_t)l])
      for (int a = 0; a < (1 << dim); ++a) {
        const uint64_t key = triangulation.vertex_key(l, cell, a);
        const auto ins = map.emplace(key, (int32_t)vec.size());
        if (ins.second) vec.push_back(key);
        tab[ls++] = *ins.first;
      }
  }
  sublap("dofs: level numbering");
}

// Is this cycle's mesh one whose tables gmg_build_mesh_tables forms?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_mesh_tables_on_device() {
  if (!par.mesh_tables_on_device) return false;
  const char *why = !solve_on_device_requested ? "the cycle does not run on the device"
                    : distributed              ? "the run is distributed"
                                               : nullptr;
  if (!why) return true;
  if (!mesh_fallback_reported) pcout(std::string("   Mesh tables on device: not applicable (") + why + "), formed on the host");
  mesh_fallback_reported = true;
  return false;
}

// what gmg_build_mesh_tables takes: the cells of every level in index order
template <int dim>
ForestCells LaplaceProblem<dim>::forest_cells() const {
  ForestCells fc;
  const int L = triangulation.n_levels();
  fc.n0[0] = fc.n0[1] = triangulation.n0;
  fc.n0[2] = dim == 3 ? triangulation.n0 : 1;
  fc.level_ptr.assign((size_t)L + 1, 0);
  for (int l = 0; l < L; ++l) fc.level_ptr[(size_t)l + 1] = fc.level_ptr[(size_t)l] + (int64_t)triangulation.levels[(size_t)l].size();
  fc.cell_coord.resize((size_t)fc.level_ptr[(size_t)L] * 3);
  fc.cell_first_child.resize((size_t)fc.level_ptr[(size_t)L]);
  for (int l = 0; l < L; ++l) {
    const auto &cells = triangulation.levels[(size_t)l];
    const int64_t b = fc.level_ptr[(size_t)l];
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < (int64_t)cells.size(); ++c) {
      for (int d = 0; d < 3; ++d) fc.cell_coord[(size_t)(b + c) * 3 + (size_t)d] = cells[(size_t)c].c[d];
      fc.cell_first_child[(size_t)(b + c)] = cells[(size_t)c].first_child;
    }
  }
  fc.level0_lexicographic = par.level0_numbering == "lexicographic" ? 1 : 0;
  return fc;
}

// distribute_dofs() through gmg_build_mesh_tables: one call, then the tables come back into the containers the host loops
// fill; the lines and the level flags wait in device_mesh for make_constraints().  The vertex -> DoF hash tables are not
// built here (ensure_dof_maps).
template <int dim>
void LaplaceProblem<dim>::distribute_dofs_on_device() {
  auto chk = [&](int rc, const char *what) {
    if (rc != GMG_OK) throw std::runtime_error(std::string("Mesh tables on device: ") + what + ": " + (gmg ? gmg_last_error(gmg) : last_error.c_str()));
  };
  chk(ensure_context(), "context");
  constexpr int nv = 1 << dim;
  const int L = triangulation.n_levels();
  const ForestCells fc = forest_cells();
  chk(gmg_build_mesh_tables(gmg, dim, fc.n0, L, fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), fc.level0_lexicographic, &mesh_tables_ms),
      "gmg_build_mesh_tables");
  sublap("dofs + constraints on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     .   build_ms %.3f\n", mesh_tables_ms);
  int64_t n_cells = 0, n_dofs = 0, n_lines = 0, n_entries = 0;
  DeviceMeshTables &t = device_mesh;
  chk(gmg_get_mesh_tables(gmg, &n_cells, &n_dofs, &t.n_hanging, &n_lines, &n_entries, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "sizes");
  if (n_cells != (int64_t)active_cells.size()) throw std::logic_error("Mesh tables on device: the active cell lists differ");
  active_cell_dof_table.resize((size_t)n_cells * nv);
  vertex_of_dof.resize((size_t)n_dofs);
  t.constraint_of_dof.resize((size_t)n_dofs);
  t.line_ptr.resize((size_t)n_lines + 1);
  t.line_master.resize((size_t)n_entries);
  t.line_weight.resize((size_t)n_entries);
  t.line_dof.resize((size_t)n_lines);
  chk(gmg_get_mesh_tables(gmg, nullptr, nullptr, nullptr, nullptr, nullptr, active_cell_dof_table.data(), nullptr, vertex_of_dof.data(), t.constraint_of_dof.data(),
                          t.line_ptr.data(), t.line_master.data(), t.line_weight.data(), t.line_dof.data()),
      "download");
  level_vertex_of_dof.assign((size_t)L, {});
  level_cell_dof_table.assign((size_t)L, {});
  t.dof_flags.assign((size_t)L, {});
  for (int l = 0; l < L; ++l) {
    int64_t nc = 0, nd = 0;
    chk(gmg_get_mesh_level_tables(gmg, l, &nc, &nd, nullptr, nullptr, nullptr), "level sizes");
    level_cell_dof_table[(size_t)l].resize((size_t)nc * nv);
    level_vertex_of_dof[(size_t)l].resize((size_t)nd);
    t.dof_flags[(size_t)l].resize((size_t)nd);
    chk(gmg_get_mesh_level_tables(gmg, l, nullptr, nullptr, level_cell_dof_table[(size_t)l].data(), level_vertex_of_dof[(size_t)l].data(), t.dof_flags[(size_t)l].data()),
        "level download");
  }
  dof_of_vertex.clear();
  level_dof_of_vertex.assign((size_t)L, {});
  dof_maps_ready = false;
  sublap("dofs + constraints: download");
}

// dof_of_vertex and level_dof_of_vertex from vertex_of_dof / level_vertex_of_dof, on first use after "Mesh tables on device"
// left them out (fe_value_at, the host path of make_constraints)
template <int dim>
void LaplaceProblem<dim>::ensure_dof_maps() {
  if (dof_maps_ready) return;
  ++dof_map_builds;
  const int L = triangulation.n_levels();
  const int lattice[3] = {triangulation.n0 + 1, triangulation.n0 + 1, dim == 3 ? triangulation.n0 + 1 : 1};
  const int none[3] = {0, 0, 0};
  dof_of_vertex.reset(kMaxLevelShift, lattice);
  dof_of_vertex.reserve_sparse(vertex_of_dof.size() - std::min(vertex_of_dof.size(), (size_t)lattice[0] * lattice[1] * lattice[2]));
  for (size_t i = 0; i < vertex_of_dof.size(); ++i) dof_of_vertex.emplace(vertex_of_dof[i], (int32_t)i);
  level_dof_of_vertex.assign((size_t)L, {});
  for (int l = 0; l < L; ++l) {
    auto &map = level_dof_of_vertex[(size_t)l];
    const auto &vec = level_vertex_of_dof[(size_t)l];
    map.reset(kMaxLevelShift, l == 0 ? lattice : none);
    if (l > 0) map.reserve_sparse(vec.size());
    for (size_t i = 0; i < vec.size(); ++i) map.emplace(vec[i], (int32_t)i);
  }
  dof_maps_ready = true;
}

template <int dim>
void LaplaceProblem<dim>::make_constraints() {
  // DoFTools::make_hanging_node_constraints + VectorTools::interpolate_boundary_values +
  // constraints.close() (:661-696), and MGConstrainedDoFs (:704-706).
  const int64_t n = (int64_t)vertex_of_dof.size();
  constraint_of_dof.assign((size_t)n, -1);
  constraint_lines.clear();
  const int shift0 = kMaxLevelShift;
  if (mesh_on_device) {  // the hanging lines as gmg_build_mesh_tables numbered them (unclosed); the Dirichlet lines follow below
    const DeviceMeshTables &t = device_mesh;
    constraint_lines.resize((size_t)t.n_hanging);
    for (int64_t l = 0; l < t.n_hanging; ++l) {
      ConstraintLine &line = constraint_lines[(size_t)l];
      line.hanging = true;
      for (int64_t e = t.line_ptr[(size_t)l]; e < t.line_ptr[(size_t)l + 1]; ++e) line.entries.push_back({t.line_master[(size_t)e], t.line_weight[(size_t)e]});
      constraint_of_dof[(size_t)t.line_dof[(size_t)l]] = (int32_t)l;
    }
  } else ensure_dof_maps();
  static const std::vector<ActiveCell> no_cells;  // (the host's loop over the faces runs over no cell when the device formed the lines)
  for (const ActiveCell &ac : mesh_on_device ? no_cells : active_cells) {
    const int l = ac.level;
    const Cell &c = triangulation.levels[(size_t)l][(size_t)ac.index];
    for (int d = 0; d < dim; ++d)
      for (int side = 0; side < 2; ++side) {
        int nb[3] = {c.c[0], c.c[1], c.c[2]};
        nb[d] += side ? 1 : -1;
        const int32_t N = triangulation.find(l, nb[0], nb[1], nb[2]);
        if (N < 0 || triangulation.active(l, N)) continue;
        // the face of this coarse cell is refined on the other side: its centre and edge
        // mid-points are hanging nodes
        uint64_t corner[4][3];
        int nc = 0;
        for (int a = 0; a < (1 << dim); ++a)
          if (((a >> d) & 1) == side) {
            uint64_t v[3];
            Forest<dim>::unpack(triangulation.vertex_key(l, c, a), v);
            for (int e = 0; e < 3; ++e) corner[nc][e] = v[e];
            ++nc;
          }
        auto add_line = [&](const int *ids, int m) {
          uint64_t s[3] = {0, 0, 0};
          for (int q = 0; q < m; ++q)
            for (int e = 0; e < 3; ++e) s[e] += corner[ids[q]][e];
          const uint64_t key = pack3(s[0] / (uint64_t)m, s[1] / (uint64_t)m, s[2] / (uint64_t)m);
          const int32_t *it = dof_of_vertex.find(key);
          if (!it) throw std::logic_error("hanging node without a DoF: mesh is not 2:1 balanced");
          if (constraint_of_dof[(size_t)*it] >= 0) return;
          ConstraintLine line;
          line.hanging = true;
          for (int q = 0; q < m; ++q)
            line.entries.push_back({dof_of_vertex.at(pack3(corner[ids[q]][0], corner[ids[q]][1], corner[ids[q]][2])), 1.0 / m});
          constraint_of_dof[(size_t)*it] = (int32_t)constraint_lines.size();
          constraint_lines.push_back(line);
        };
        if (dim == 2) {
          const int e[2] = {0, 1};
          add_line(e, 2);
        } else {
          const int all[4] = {0, 1, 2, 3};
          add_line(all, 4);
          const int edges[4][2] = {{0, 1}, {2, 3}, {0, 2}, {1, 3}};
          for (auto &e : edges) add_line(e, 2);
        }
      }
  }
  (void)shift0;
  // Dirichlet lines for boundary DoFs that are not already (hanging-node) constrained
  if (lammpsinput) compute_moments();
  // "Analytical solution on device": the Exact values of all boundary DoFs in one batch (gmg_exact.hpp) instead of one
  // sequential sum over the atoms per DoF; the lines are created in the same DoF order either way
  const bool batch = par.analytical_on_device && dim == 3 && par.Boundary_conditions == "Exact" && par.Problemtype == "GaussianCharges";
  std::vector<int32_t> batch_line;
  std::vector<double> batch_x;
  // (the device lists the DoFs of the Dirichlet lines in the same ascending order: line_dof behind the hanging lines)
  std::vector<int32_t> dirichlet_dof;
  if (mesh_on_device) dirichlet_dof.assign(device_mesh.line_dof.begin() + device_mesh.n_hanging, device_mesh.line_dof.end());
  else
    for (int64_t i = 0; i < n; ++i)
      if (triangulation.vertex_on_boundary(vertex_of_dof[(size_t)i]) && constraint_of_dof[(size_t)i] < 0) dirichlet_dof.push_back((int32_t)i);
  for (const int32_t i : dirichlet_dof) {
    double x[3];
    triangulation.vertex_coords(vertex_of_dof[(size_t)i], x);
    ConstraintLine line;
    if (batch) {
      batch_line.push_back((int32_t)constraint_lines.size());
      batch_x.insert(batch_x.end(), x, x + 3);
    } else {
      line.inhomogeneity = boundary_value(x);
    }
    constraint_of_dof[(size_t)i] = (int32_t)constraint_lines.size();
    constraint_lines.push_back(line);
  }
  if (!batch_line.empty()) {
    std::vector<double> v(batch_line.size());
    if (gaussian_potential(exact_on_device(), (int64_t)v.size(), batch_x.data(), v.data(), nullptr) != GMG_OK)
      throw std::runtime_error("exact boundary values: " + last_error);
    for (size_t k = 0; k < v.size(); ++k) constraint_lines[(size_t)batch_line[k]].inhomogeneity = v[k];
  }
  // close(): masters that are themselves (Dirichlet) constrained fold into the inhomogeneity
  for (ConstraintLine &line : constraint_lines) {
    if (!line.hanging) continue;
    std::vector<std::pair<int32_t, double>> kept;
    for (auto &e : line.entries) {
      const int32_t cm = constraint_of_dof[(size_t)e.first];
      if (cm < 0) { kept.push_back(e); continue; }
      const ConstraintLine &m = constraint_lines[(size_t)cm];
      if (m.hanging) throw std::logic_error("hanging node constrained to a hanging node");
      line.inhomogeneity += e.second * m.inhomogeneity;
    }
    line.entries.swap(kept);
  }
  // MGConstrainedDoFs: boundary indices and refinement-edge indices per level
  const int L = triangulation.n_levels();
  level_boundary.assign((size_t)L, {});
  level_refinement_edge.assign((size_t)L, {});
  for (int l = 0; l < L; ++l) {
    const auto &vec = level_vertex_of_dof[(size_t)l];
    level_boundary[(size_t)l].assign(vec.size(), 0);
    level_refinement_edge[(size_t)l].assign(vec.size(), 0);
    if (mesh_on_device) {
      const auto &fl = device_mesh.dof_flags[(size_t)l];
      for (size_t i = 0; i < vec.size(); ++i) { level_boundary[(size_t)l][i] = fl[i] & 1; level_refinement_edge[(size_t)l][i] = (fl[i] >> 1) & 1; }
      continue;
    }
    for (size_t i = 0; i < vec.size(); ++i) level_boundary[(size_t)l][i] = triangulation.vertex_on_boundary(vec[i]);
    if (l == 0) continue;
    const int nl = triangulation.n0 << l;
    for (size_t ci = 0; ci < triangulation.levels[(size_t)l].size(); ++ci) {
      const Cell &c = triangulation.levels[(size_t)l][ci];
      for (int d = 0; d < dim; ++d)
        for (int side = 0; side < 2; ++side) {
          int nb[3] = {c.c[0], c.c[1], c.c[2]};
          nb[d] += side ? 1 : -1;
          if (nb[d] < 0 || nb[d] >= nl) continue;  // domain boundary
          if (triangulation.find(l, nb[0], nb[1], nb[2]) >= 0) continue;
          for (int a = 0; a < (1 << dim); ++a)
            if (((a >> d) & 1) == side)
              level_refinement_edge[(size_t)l][(size_t)level_dof_of_vertex[(size_t)l].at(triangulation.vertex_key(l, c, a))] = 1;
        }
    }
  }
  if (mesh_on_device) {  // (the same lines, numbered the same: anything else is a defect of the entry, not of the mesh)
    if (constraint_of_dof != device_mesh.constraint_of_dof) throw std::logic_error("Mesh tables on device: constraint_of_dof differs from the lines");
    device_mesh = DeviceMeshTables();  // (the host copy; the context keeps its tables until the next build, gmg_reset or gmg_destroy)
  }
  operators_resident = decide_operators_resident();
  if (operators_resident) close_constraints_on_device();
}

// Do this cycle's device entries read the context's mesh tables?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_operators_resident() {
  if (!par.operators_from_resident_tables) return false;
  const char *why = distributed                      ? "the run is distributed"
                    : !mesh_on_device                ? "the mesh tables were not formed on the device"
                    : !par.system_matrix_on_device   ? "System matrix on device is not set"
                    : !par.level_matrices_on_device  ? "Level matrices on device is not set"
                    : !par.rhs_from_cell_tables      ? "RHS from cell tables is not set"
                                                     : nullptr;
  if (!why) return true;
  if (!resident_fallback_reported) pcout(std::string("   Operators from resident tables: not applicable (") + why + "), host arrays");
  resident_fallback_reported = true;
  return false;
}

// The boundary values make_constraints computed (boundary_value, or the gmg_gaussian_potential batch) go to the Dirichlet
// lines of the resident tables, in line order, and close() runs there.  The host's closed constraint_lines stay: other host
// loops read them.  STEP50_CHECK_RESIDENT=1 holds the device's closed lines against them.
template <int dim>
void LaplaceProblem<dim>::close_constraints_on_device() {
  auto chk = [&](int rc, const char *what) { if (rc != GMG_OK) throw std::runtime_error(std::string("Operators from resident tables: ") + what + ": " + gmg_last_error(gmg)); };
  sublap("make_constraints: host");  // (everything before this call; setup_system's lap "make_constraints" then holds the tail only)
  size_t H = 0;
  while (H < constraint_lines.size() && constraint_lines[H].hanging) ++H;
  std::vector<double> value(constraint_lines.size() - H);
  for (size_t l = H; l < constraint_lines.size(); ++l) value[l - H] = constraint_lines[l].inhomogeneity;
  double build_ms = 0.0;
  chk(gmg_close_constraints(gmg, (int64_t)value.size(), value.data(), &build_ms), "gmg_close_constraints");
  sublap("constraints: close on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
  const char *check = std::getenv("STEP50_CHECK_RESIDENT");
  if (!check || std::atoi(check) == 0) return;
  int64_t n_lines = 0, n_entries = 0;
  chk(gmg_get_closed_constraints(gmg, &n_lines, &n_entries, nullptr, nullptr, nullptr, nullptr), "sizes");
  std::vector<int64_t> lp((size_t)n_lines + 1), h_lp;
  std::vector<int32_t> lm((size_t)n_entries), h_lm;
  std::vector<double> lw((size_t)n_entries), li((size_t)n_lines), h_lw, h_li;
  chk(gmg_get_closed_constraints(gmg, nullptr, nullptr, lp.data(), lm.data(), lw.data(), li.data()), "gmg_get_closed_constraints");
  line_tables(h_lp, h_lm, h_lw, h_li);
  if (lp != h_lp || lm != h_lm || lw.size() != h_lw.size() || li.size() != h_li.size() ||
      (!lw.empty() && std::memcmp(lw.data(), h_lw.data(), sizeof(double) * lw.size()) != 0) ||
      (!li.empty() && std::memcmp(li.data(), h_li.data(), sizeof(double) * li.size()) != 0))
    throw std::logic_error("Operators from resident tables: the device's closed lines differ from the host's");
}

template <int dim>
void LaplaceProblem<dim>::setup_system(unsigned int cycle) {
  distribute_dofs();
  const int64_t n = (int64_t)vertex_of_dof.size();
  solution.assign((size_t)n, 0.0);
  solution_on_device = false;
  system_rhs.assign((size_t)n, 0.0);
  if (cycle == 0 && par.flag_rhs_assembly && lammpsinput) rhs_assembly_optimization();
  sublap("rhs_assembly_optimization");
  densities_resident = decide_densities_resident();
  if (lammpsinput) compute_charge_densities();
  sublap("compute_charge_densities");
  if (densities_resident && sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", densities_resident_ms);
  make_constraints();  // calls compute_moments() first when atoms are present (:675-679)
  sublap("make_constraints");
}

// Does this cycle's compute_charge_densities read the context's mesh tables?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_densities_resident() {
  if (!par.densities_from_resident_tables) return false;
  const char *why = distributed                 ? "the run is distributed"
                    : dim != 3                  ? "the problem is not 3D"
                    : !lammpsinput              ? "no LAMMPS input"
                    : !mesh_on_device           ? "the mesh tables were not formed on the device"
                    : !par.densities_on_device  ? "Charge densities on device is not set"
                                                : nullptr;
  if (!why) return true;
  if (!densities_fallback_reported) pcout(std::string("   Charge densities from resident tables: not applicable (") + why + "), per-cell arrays from the host");
  densities_fallback_reported = true;
  return false;
}

template <int dim>
void LaplaceProblem<dim>::compute_charge_densities() {
  // :509-575, rho(x_q) = 4 pi / (r_c^3 pi^1.5) sum_k q_k exp(-|x_q - x_k|^2 / r_c^2)
  const Quadrature<dim> quad((int)(par.degree + par.quadrature_degree_rhs));
  const size_t nq = quad.p.size();
  density_values_for_each_cell.assign(active_cells.size(), {});
  densities_device_resident = false;
  if (densities_on_device && dim == 3) {
    // the same sums on the MI355X (gmg_charge_density), cell geometry in, rho out
    if (ensure_context() != GMG_OK) throw std::runtime_error("charge densities on the device: " + last_error);
    const size_t nc = active_cells.size();
    const char *check = std::getenv("STEP50_CHECK_RESIDENT");
    const bool hold = densities_resident && check && std::atoi(check) != 0;  // the device's geometry against the loop below
    const size_t ng = densities_resident && !hold ? 0 : nc;                  // (resident: no per-cell array is built)
    std::vector<double> lo(3 * ng), hh(ng), rlo(3 * ng), qp(3 * nq), dens(densities_resident && par.rhs_on_device ? 0 : nc * nq);
    for (size_t ci = 0; ci < ng; ++ci) {
      const ActiveCell &ac = active_cells[ci];
      const Cell &cell = triangulation.levels[(size_t)ac.level][(size_t)ac.index];
      double x0[3];
      triangulation.cell_origin(ac.level, cell, x0);
      hh[ci] = triangulation.cell_size(ac.level);
      for (int d = 0; d < 3; ++d) {
        lo[3 * ci + (size_t)d] = x0[d];
        rlo[3 * ci + (size_t)d] = triangulation.origin + triangulation.h0 * (cell.c[d] >> ac.level);
      }
    }
    for (size_t q = 0; q < nq; ++q)
      for (int d = 0; d < 3; ++d) qp[3 * q + (size_t)d] = quad.p[q][(size_t)d];
    // "RHS on device": the densities stay in HBM (dens = NULL) and gmg_rhs_assemble integrates them there; the host gets a
    // copy only if something asks for it (HEAD's residual estimator, the rc_variation check vector): ensure_host_densities()
    densities_device_resident = par.rhs_on_device;
    if (densities_resident) {
      // "Charge densities from resident tables": the cells' geometry follows from cell_level and vertex_of_dof where they lie
      int rc = gmg_charge_density_resident(gmg, triangulation.origin, triangulation.h0, (int64_t)number_of_atoms, atom_positions.data(), charges.data(),
                                           par.r_c, par.nonzero_density_radius_parameter * par.r_c, par.flag_rhs_assembly ? 1 : 0, (int)nq, qp.data(),
                                           densities_device_resident ? nullptr : dens.data(), &densities_resident_ms);
      if (rc != GMG_OK) throw std::runtime_error(std::string("gmg_charge_density_resident: ") + gmg_last_error(gmg));
      if (hold) {
        std::vector<double> d_lo(3 * nc), d_hh(nc), d_rlo(3 * nc);
        rc = gmg_get_resident_cell_geometry(gmg, triangulation.origin, triangulation.h0, d_lo.data(), d_hh.data(), d_rlo.data());
        if (rc != GMG_OK) throw std::runtime_error(std::string("gmg_get_resident_cell_geometry: ") + gmg_last_error(gmg));
        if (nc && (std::memcmp(d_lo.data(), lo.data(), sizeof(double) * 3 * nc) != 0 || std::memcmp(d_hh.data(), hh.data(), sizeof(double) * nc) != 0 ||
                   std::memcmp(d_rlo.data(), rlo.data(), sizeof(double) * 3 * nc) != 0))
          throw std::logic_error("Charge densities from resident tables: the device's cell geometry differs from the host's");
      }
      if (densities_device_resident) { density_values_for_each_cell.clear(); return; }
      for (size_t ci = 0; ci < nc; ++ci) density_values_for_each_cell[ci].assign(dens.begin() + (std::ptrdiff_t)(ci * nq), dens.begin() + (std::ptrdiff_t)((ci + 1) * nq));
      return;
    }
    const int rc = gmg_charge_density(gmg, (int64_t)nc, lo.data(), hh.data(), rlo.data(), triangulation.h0, (int64_t)number_of_atoms,
                                      atom_positions.data(), charges.data(), par.r_c, par.nonzero_density_radius_parameter * par.r_c,
                                      par.flag_rhs_assembly ? 1 : 0, (int)nq, qp.data(), densities_device_resident ? nullptr : dens.data());
    if (rc != GMG_OK) throw std::runtime_error(std::string("gmg_charge_density: ") + gmg_last_error(gmg));
    if (densities_device_resident) { density_values_for_each_cell.clear(); return; }
    for (size_t ci = 0; ci < nc; ++ci) density_values_for_each_cell[ci].assign(dens.begin() + (std::ptrdiff_t)(ci * nq), dens.begin() + (std::ptrdiff_t)((ci + 1) * nq));
    return;
  }
  const double constant_value = 4.0 * M_PI / (std::pow(par.r_c, 3) * std::pow(M_PI, 1.5));
  const double r_c_squared_inverse = 1.0 / (par.r_c * par.r_c);
#pragma omp parallel
  {
    std::vector<int32_t> atoms;
#pragma omp for schedule(dynamic, 256)
    for (int64_t ci = 0; ci < (int64_t)active_cells.size(); ++ci) {
      const ActiveCell &ac = active_cells[(size_t)ci];
      const Cell &cell = triangulation.levels[(size_t)ac.level][(size_t)ac.index];
      double x0[3];
      triangulation.cell_origin(ac.level, cell, x0);
      const double h = triangulation.cell_size(ac.level);
      const bool use_list = par.flag_rhs_assembly;
      if (use_list) {
        const int rc[3] = {cell.c[0] >> ac.level, cell.c[1] >> ac.level, cell.c[2] >> ac.level};
        atoms_of_root_cell(rc, atoms);
      }
      std::vector<double> &dens = density_values_for_each_cell[(size_t)ci];
      dens.assign(nq, 0.0);
      const size_t na = use_list ? atoms.size() : (size_t)number_of_atoms;
      for (size_t q = 0; q < nq; ++q) {
        double xq[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) xq[d] = x0[d] + h * quad.p[q][(size_t)d];
        double s = 0.0;
        for (size_t t = 0; t < na; ++t) {
          const size_t k = use_list ? (size_t)atoms[t] : t;
          double r2 = 0;
          for (int d = 0; d < 3; ++d) { const double dd = atom_positions[3 * k + (size_t)d] - xq[d]; r2 += dd * dd; }
          const double r = std::sqrt(r2);  // the reference squares the distance again (:547-548)
          s += constant_value * std::exp(-(r * r) * r_c_squared_inverse) * charges[k];
        }
        dens[q] = s;
      }
    }
  }
}

template <int dim>
void LaplaceProblem<dim>::ensure_host_densities() {
  if (!lammpsinput || !densities_device_resident || density_values_for_each_cell.size() == active_cells.size()) return;
  const Quadrature<dim> quad((int)(par.degree + par.quadrature_degree_rhs));
  const size_t nq = quad.p.size(), nc = active_cells.size();
  std::vector<double> dens(nc * nq);
  ++host_density_copies;
  if (gmg_get_charge_density(gmg, (int64_t)nc, (int)nq, dens.data()) != GMG_OK) throw std::runtime_error(std::string("gmg_get_charge_density: ") + gmg_last_error(gmg));
  density_values_for_each_cell.assign(nc, {});
  for (size_t ci = 0; ci < nc; ++ci) density_values_for_each_cell[ci].assign(dens.begin() + (std::ptrdiff_t)(ci * nq), dens.begin() + (std::ptrdiff_t)((ci + 1) * nq));
}

template <int dim>
void LaplaceProblem<dim>::compute_moments() {
  // :577-644 -- the quadrupole is integrated and then overwritten with 0 (:623-624): only the
  // dipole survives.
  for (int d = 0; d < 3; ++d) dipole_moment[d] = 0;
  for (unsigned k = 0; k < number_of_atoms; ++k)
    for (int d = 0; d < 3; ++d) dipole_moment[d] += charges[k] * atom_positions[3 * k + (size_t)d];
}

// ======================================================================== assembly

namespace {
// sum_d d_d phi_i d_d phi_j at quadrature point q of the reference cell: the G[q][i][j] of gmg_assemble_*_matrix_coef
template <int dim>
inline double gradient_product(const Quadrature<dim> &q2, size_t q, int i, int j) {
  double g = 0;
  for (int d = 0; d < dim; ++d) g += q2.grad[q][(size_t)i][(size_t)d] * q2.grad[q][(size_t)j][(size_t)d];
  return g;
}

// the cell matrix of a cell with edge h from the coefficient's values at its quadrature points (coef == nullptr: 1.0
// everywhere); gmg_assemble_*_matrix_coef forms the same sums from the same values
template <int dim>
void cell_matrix(const Quadrature<dim> &q2, double h, const double *coef, double K[1 << dim][1 << dim]) {
  constexpr int nv = 1 << dim;
  for (int i = 0; i < nv; ++i)
    for (int j = 0; j < nv; ++j) K[i][j] = 0;
  const double scale = std::pow(h, dim - 2);  // JxW / h^2 from the two gradients
  for (size_t q = 0; q < q2.p.size(); ++q) {
    const double c = coef ? coef[q] : 1.0;
    for (int i = 0; i < nv; ++i)
      for (int j = 0; j < nv; ++j) {
        const double g = gradient_product<dim>(q2, q, i, j);
        K[i][j] += c * g * q2.w[q] * scale;
      }
  }
}

constexpr int kMaxCoefficientPoints = 64;  // (degree 1: 2^dim points)

// The coefficient at the quadrature points of a cell with origin x0 and edge h, q ascending.  The one text for these values:
// the host's cell matrices and the tables of gmg_assemble_*_matrix_coef are made from it, so a point near the sphere is on
// the same side for both.
template <int dim>
void coefficient_values(const LaplaceProblem<dim> &P, const Quadrature<dim> &q2, double h, const double x0[3], double *out) {
  for (size_t q = 0; q < q2.p.size(); ++q) {
    double x[3] = {0, 0, 0};
    for (int d = 0; d < dim; ++d) x[d] = x0[d] + h * q2.p[q][(size_t)d];
    out[q] = P.coefficient(x);
  }
}

// The cell matrix and the constraint lines of an active cell as assemble_system takes them.  One text for the matrix pass,
// the right-hand-side pass and the K_of_level table of gmg_assemble_system_matrix: the device's matrix has the host's bits
// only as long as all three scale the cell matrix the same way.
template <int dim>
struct CellAssembly {
  static constexpr int nv = 1 << dim;
  using Line = typename LaplaceProblem<dim>::ConstraintLine;
  const LaplaceProblem<dim> &P;
  const Quadrature<dim> q_laplace;
  const bool constant_coef;
  double Kc[nv][nv];  // constant coefficient: the cell matrix of the unit cell
  explicit CellAssembly(const LaplaceProblem<dim> &p) : P(p), q_laplace((int)p.par.degree + 1), constant_coef(p.par.Problemtype != "Step16") {
    cell_matrix<dim>(q_laplace, 1.0, nullptr, Kc);
  }
  // constant coefficient: the cell matrix of a cell with edge h
  void scaled(double h, double (&K)[nv][nv]) const {
    const double s = std::pow(h, dim - 2);
    for (int i = 0; i < nv; ++i)
      for (int j = 0; j < nv; ++j) K[i][j] = Kc[i][j] * s;
  }
  void cell_K(size_t ci, double (&K)[nv][nv], double (&x0)[3], double &h) const {
    const auto &ac = P.active_cells[ci];
    const Cell &cell = P.triangulation.levels[(size_t)ac.level][(size_t)ac.index];
    h = P.triangulation.cell_size(ac.level);
    P.triangulation.cell_origin(ac.level, cell, x0);
    if (constant_coef) { scaled(h, K); return; }
    double c[kMaxCoefficientPoints];
    coefficient_values<dim>(P, q_laplace, h, x0, c);
    cell_matrix<dim>(q_laplace, h, c, K);
  }
  // ConstraintMatrix::distribute_local_to_global (:793-795, 825-828)
  void cell_lines(size_t ci, int32_t (&dofs)[nv], const Line *(&line)[nv]) const {
    P.cell_dofs(P.active_cells[ci], dofs);
    for (int a = 0; a < nv; ++a) {
      const int32_t cl = P.constraint_of_dof[(size_t)dofs[a]];
      line[a] = cl >= 0 ? &P.constraint_lines[(size_t)cl] : nullptr;
    }
  }
};
}  // namespace

// Is the system matrix the kind of operator gmg_assemble_system_matrix forms?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_system_on_device() {
  if (!par.system_matrix_on_device) return false;
  const char *why = !solve_on_device_requested ? "the cycle does not run on the device"
                    : distributed              ? "the run is distributed"
                                               : nullptr;
  if (!why) return true;
  if (!system_fallback_reported) pcout(std::string("   System matrix on device: not applicable (") + why + "), assembled on the host");
  system_fallback_reported = true;
  return false;
}

template <int dim>
void LaplaceProblem<dim>::ensure_system_matrix() {
  // (outside assemble_system: without its sublaps, which belong to that phase's clock)
  if (system_on_device && system_matrix.n_rows == 0 && !vertex_of_dof.empty()) assemble_system_matrix_host(false);
}

// the arrays of gmg_assemble_system_matrix: cell DoFs and levels, the cell matrix as cell_K scales it per level, the lines
template <int dim>
typename LaplaceProblem<dim>::SystemAssemblyInputs LaplaceProblem<dim>::system_assembly_inputs(bool mesh_arrays) const {
  constexpr int nv = 1 << dim;
  SystemAssemblyInputs in;
  in.cell_dofs.resize(mesh_arrays ? active_cells.size() * nv : 0);
  in.cell_level.resize(mesh_arrays ? active_cells.size() : 0);
  for (size_t ci = 0; mesh_arrays && ci < active_cells.size(); ++ci) {
    cell_dofs(active_cells[ci], &in.cell_dofs[ci * nv]);
    if (active_cells[ci].level > 15) throw std::runtime_error("System matrix on device: more than 16 levels");
    in.cell_level[ci] = (uint8_t)active_cells[ci].level;
  }
  const CellAssembly<dim> ca(*this);
  in.K_of_level.resize((size_t)16 * nv * nv);
  for (int l = 0; l < 16; ++l) {
    double K[nv][nv];
    ca.scaled(triangulation.cell_size(l), K);
    for (int i = 0; i < nv; ++i)
      for (int j = 0; j < nv; ++j) in.K_of_level[((size_t)l * nv + (size_t)i) * nv + (size_t)j] = K[i][j];
  }
  if (mesh_arrays) line_tables(in.line_ptr, in.line_master, in.line_weight, in.line_inhomogeneity);
  return in;
}

// the constraint lines in the CSR form the device entries take (a Dirichlet line has no entries)
template <int dim>
void LaplaceProblem<dim>::line_tables(std::vector<int64_t> &line_ptr, std::vector<int32_t> &line_master, std::vector<double> &line_weight,
                                      std::vector<double> &line_inhomogeneity) const {
  line_ptr.assign(constraint_lines.size() + 1, 0);
  line_master.clear(); line_weight.clear(); line_inhomogeneity.clear();
  for (size_t l = 0; l < constraint_lines.size(); ++l) {
    line_ptr[l + 1] = line_ptr[l] + (int64_t)constraint_lines[l].entries.size();
    line_inhomogeneity.push_back(constraint_lines[l].inhomogeneity);
    for (auto &e : constraint_lines[l].entries) { line_master.push_back(e.first); line_weight.push_back(e.second); }
  }
}

// what the coefficient form takes beyond the cell tables: the quadrature's tables and, filled by the callers below, the
// coefficient values and the scale(s)
template <int dim>
typename LaplaceProblem<dim>::CoefficientInputs LaplaceProblem<dim>::coefficient_tables() const {
  constexpr int nv = 1 << dim;
  const Quadrature<dim> q2((int)par.degree + 1);
  CoefficientInputs in;
  in.nq = (int)q2.p.size();
  if (in.nq > kMaxCoefficientPoints) throw std::runtime_error("coefficient inputs: more than 64 quadrature points");
  in.qw.assign(q2.w.begin(), q2.w.end());
  in.G.resize((size_t)in.nq * nv * nv);
  for (size_t q = 0; q < q2.p.size(); ++q)
    for (int i = 0; i < nv; ++i)
      for (int j = 0; j < nv; ++j) in.G[(q * nv + (size_t)i) * nv + (size_t)j] = gradient_product<dim>(q2, q, i, j);
  return in;
}

// gmg_assemble_system_matrix_coef: the coefficient at the quadrature points of every active cell (the host's threads, one
// cell per iteration: the values do not depend on their number) and pow(h, dim - 2) of every level, as cell_matrix scales
template <int dim>
typename LaplaceProblem<dim>::CoefficientInputs LaplaceProblem<dim>::system_coefficient_inputs() const {
  const Quadrature<dim> q2((int)par.degree + 1);
  CoefficientInputs in = coefficient_tables();
  const int64_t nc = (int64_t)active_cells.size();
  in.cell_coef.resize((size_t)nc * (size_t)in.nq);
#pragma omp parallel for schedule(static)
  for (int64_t ci = 0; ci < nc; ++ci) {
    const auto &ac = active_cells[(size_t)ci];
    double x0[3];
    triangulation.cell_origin(ac.level, triangulation.levels[(size_t)ac.level][(size_t)ac.index], x0);
    coefficient_values<dim>(*this, q2, triangulation.cell_size(ac.level), x0, &in.cell_coef[(size_t)ci * (size_t)in.nq]);
  }
  in.scale.resize(16);
  for (int l = 0; l < 16; ++l) in.scale[(size_t)l] = std::pow(triangulation.cell_size(l), dim - 2);
  return in;
}

// gmg_assemble_level_matrix_coef: likewise for all cells of level l, with the level's one scale
template <int dim>
typename LaplaceProblem<dim>::CoefficientInputs LaplaceProblem<dim>::level_coefficient_inputs(int l) const {
  const Quadrature<dim> q2((int)par.degree + 1);
  CoefficientInputs in = coefficient_tables();
  const auto &cells = triangulation.levels[(size_t)l];
  const int64_t nc = (int64_t)cells.size();
  const double h = triangulation.cell_size(l);
  in.cell_coef.resize((size_t)nc * (size_t)in.nq);
#pragma omp parallel for schedule(static)
  for (int64_t ci = 0; ci < nc; ++ci) {
    double x0[3];
    triangulation.cell_origin(l, cells[(size_t)ci], x0);
    coefficient_values<dim>(*this, q2, h, x0, &in.cell_coef[(size_t)ci * (size_t)in.nq]);
  }
  in.scale.assign(1, std::pow(h, dim - 2));
  return in;
}

template <int dim>
void LaplaceProblem<dim>::assemble_system_matrix_host(bool laps) {
  constexpr int nv = 1 << dim;
  const int64_t n = (int64_t)vertex_of_dof.size();
  // coupling lists: the cell's DoFs plus the masters of its constrained DoFs
  if (laps) sublap(nullptr);
  std::vector<int64_t> cptr(active_cells.size() + 1, 0);
  std::vector<int32_t> citems;
  citems.reserve(active_cells.size() * nv);
  for (size_t ci = 0; ci < active_cells.size(); ++ci) {
    int32_t dofs[nv];
    cell_dofs(active_cells[ci], dofs);
    const size_t begin = citems.size();
    for (int a = 0; a < nv; ++a) {
      citems.push_back(dofs[a]);
      const int32_t cl = constraint_of_dof[(size_t)dofs[a]];
      if (cl >= 0)
        for (auto &e : constraint_lines[(size_t)cl].entries) citems.push_back(e.first);
    }
    std::sort(citems.begin() + (std::ptrdiff_t)begin, citems.end());
    citems.erase(std::unique(citems.begin() + (std::ptrdiff_t)begin, citems.end()), citems.end());
    cptr[ci + 1] = (int64_t)citems.size();
  }
  if (laps) sublap("assemble: coupling lists");
  system_matrix = pattern_from_cells(n, cptr, citems);
  if (laps) sublap("assemble: sparsity pattern");
  // One pass over the cells per THREAD for the matrix, restricted to the rows the thread owns (SURVEY 8 / VERDICT r02 #8:
  // threaded host setup): a cell is visited by the threads whose row range meets its coupling list, every entry still
  // receives its cells' contributions in cell order -- the same bits as the sequential loop, whatever the thread count.
  // The right-hand side (or the plan for gmg_rhs_assemble) follows in a sequential pass of its own.
  const CellAssembly<dim> ca(*this);
#pragma omp parallel
  {
    int nt = 1, tid = 0;
#ifdef _OPENMP
    nt = omp_get_num_threads(); tid = omp_get_thread_num();
#endif
    const int64_t r0 = n * tid / nt, r1 = n * (tid + 1) / nt;
    auto add = [&](int32_t r, int32_t c, double v) { if (r >= r0 && r < r1) system_matrix.add(r, c, v); };
    for (size_t ci = 0; ci < active_cells.size(); ++ci) {
      // (the coupling list of a cell is sorted: its first and last entries bound the rows the cell can touch)
      if (citems[(size_t)cptr[ci + 1] - 1] < r0 || citems[(size_t)cptr[ci]] >= r1) continue;
      double K[nv][nv], x0[3], h;
      ca.cell_K(ci, K, x0, h);
      int32_t dofs[nv];
      const ConstraintLine *line[nv];
      ca.cell_lines(ci, dofs, line);
      for (int i = 0; i < nv; ++i) {
        if (line[i]) add(dofs[i], dofs[i], std::fabs(K[i][i]));
        for (int j = 0; j < nv; ++j) {
          if (!line[i] && !line[j]) { add(dofs[i], dofs[j], K[i][j]); continue; }
          if (line[i] && line[i]->entries.empty()) continue;
          if (line[j] && line[j]->entries.empty()) continue;
          if (line[i] && line[j]) {
            for (auto &ri : line[i]->entries)
              for (auto &rj : line[j]->entries) add(ri.first, rj.first, ri.second * rj.second * K[i][j]);
          } else if (line[i]) {
            for (auto &ri : line[i]->entries) add(ri.first, dofs[j], ri.second * K[i][j]);
          } else {
            for (auto &rj : line[j]->entries) add(dofs[i], rj.first, rj.second * K[i][j]);
          }
        }
      }
    }
  }
  if (laps) sublap("assemble: matrix pass");
}

template <int dim>
void LaplaceProblem<dim>::assemble_system() {
  constexpr int nv = 1 << dim;
  const int64_t n = (int64_t)vertex_of_dof.size();
  const Quadrature<dim> q_rhs((int)(par.degree + par.quadrature_degree_rhs));
  // "System matrix on device": coupling lists, pattern and matrix pass are left to gmg_assemble_system_matrix at upload();
  // the host forms the matrix only when somebody asks for it (ensure_system_matrix)
  system_on_device = decide_system_on_device();
  if (system_on_device) { system_matrix = CSRMatrix(); sublap(nullptr); }
  else assemble_system_matrix_host();
  system_rhs.assign((size_t)n, 0.0);
  // "RHS from cell tables": no cell loop and no plan here, gmg_assemble_rhs forms the vector from the cell tables
  rhs_from_cells = decide_rhs_from_cell_tables();
  if (rhs_from_cells) { assemble_rhs_from_cell_tables(); return; }
  // "RHS on device": the cell loop records WHERE every F_i goes (DoF, slot = cell * 2^dim + i, weight) and which Dirichlet
  // terms it loses instead of forming F from densities the host does not have; gmg_rhs_assemble does the arithmetic
  const bool rhs_dev = lammpsinput && densities_device_resident;
  std::vector<int32_t> plan_dof, plan_slot, term_slot;
  std::vector<uint8_t> plan_code;
  std::vector<double> term_value, coef_table(256, 0.0);
  int n_codes = 1;  // code 0: the slot's value as it is
  auto code_of = [&](double w) -> int {
    for (int c = 1; c < n_codes; ++c)
      if (coef_table[(size_t)c] == w) return c;
    if (n_codes >= 256) throw std::runtime_error("RHS on device: more than 255 distinct constraint weights");
    coef_table[(size_t)n_codes] = w;
    return n_codes++;
  };
  if (rhs_dev) { plan_dof.reserve(active_cells.size() * nv); plan_slot.reserve(active_cells.size() * nv); plan_code.reserve(active_cells.size() * nv); }

  const CellAssembly<dim> ca(*this);
  for (size_t ci = 0; ci < active_cells.size(); ++ci) {
    double K[nv][nv], x0[3], h;
    int32_t dofs[nv];
    const ConstraintLine *line[nv];
    ca.cell_lines(ci, dofs, line);
    bool any_inhom = false;
    for (int a = 0; a < nv; ++a) any_inhom = any_inhom || (line[a] && line[a]->inhomogeneity != 0.0);
    // (the cell matrix only for the inhomogeneous Dirichlet terms below: with "System matrix on device" nobody else forms it)
    if (any_inhom) ca.cell_K(ci, K, x0, h);
    else { h = triangulation.cell_size(active_cells[ci].level); }
    double F[nv];
    for (int i = 0; i < nv; ++i) F[i] = 0;
    const double jxw = std::pow(h, dim);
    if (!rhs_dev && !lammpsinput) triangulation.cell_origin(active_cells[ci].level, triangulation.levels[(size_t)active_cells[ci].level][(size_t)active_cells[ci].index], x0);
    for (size_t q = 0; q < q_rhs.p.size() && !rhs_dev; ++q) {
      double dens;
      if (lammpsinput) dens = density_values_for_each_cell[ci][q];
      else {
        double x[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) x[d] = x0[d] + h * q_rhs.p[q][(size_t)d];
        dens = rhs_function(x);
      }
      for (int i = 0; i < nv; ++i) F[i] += q_rhs.shape[q][(size_t)i] * dens * q_rhs.w[q] * jxw;
    }
    for (int i = 0; i < nv; ++i) {
      double Fi = F[i];
      const int32_t slot = (int32_t)(ci * nv + (size_t)i);
      for (int j = 0; j < nv && any_inhom; ++j)
        if (line[j] && line[j]->inhomogeneity != 0.0) {
          if (rhs_dev) { term_slot.push_back(slot); term_value.push_back(K[i][j] * line[j]->inhomogeneity); }
          else Fi -= K[i][j] * line[j]->inhomogeneity;
        }
      if (line[i]) {
        for (auto &ri : line[i]->entries) {
          if (rhs_dev) { plan_dof.push_back(ri.first); plan_slot.push_back(slot); plan_code.push_back((uint8_t)code_of(ri.second)); }
          else system_rhs[(size_t)ri.first] += ri.second * Fi;
        }
      } else if (rhs_dev) {
        plan_dof.push_back(dofs[i]); plan_slot.push_back(slot); plan_code.push_back(0);
      } else {
        system_rhs[(size_t)dofs[i]] += Fi;
      }
    }
  }
  sublap("assemble: rhs pass");
  if (rhs_dev) {
    // per-DoF gather lists in the order the loop above would have added (a stable counting sort by DoF)
    std::vector<int64_t> dof_ptr((size_t)n + 1, 0);
    for (int32_t d : plan_dof) dof_ptr[(size_t)d + 1]++;
    for (int64_t i = 0; i < n; ++i) dof_ptr[(size_t)i + 1] += dof_ptr[(size_t)i];
    std::vector<int32_t> entry_slot(plan_dof.size());
    std::vector<uint8_t> entry_code(plan_dof.size());
    {
      std::vector<int64_t> pos(dof_ptr.begin(), dof_ptr.end() - 1);
      for (size_t e = 0; e < plan_dof.size(); ++e) {
        const int64_t q = pos[(size_t)plan_dof[e]]++;
        entry_slot[(size_t)q] = plan_slot[e];
        entry_code[(size_t)q] = plan_code[e];
      }
    }
    std::vector<uint8_t> cell_level(active_cells.size());
    for (size_t ci = 0; ci < active_cells.size(); ++ci) cell_level[ci] = (uint8_t)active_cells[ci].level;
    double jxw_of_level[16];
    for (int l = 0; l < 16; ++l) jxw_of_level[l] = std::pow(triangulation.cell_size(l), dim);
    std::vector<double> shape(q_rhs.p.size() * nv), weight(q_rhs.p.size());
    for (size_t q = 0; q < q_rhs.p.size(); ++q) {
      weight[q] = q_rhs.w[q];
      for (int i = 0; i < nv; ++i) shape[q * nv + (size_t)i] = q_rhs.shape[q][(size_t)i];
    }
    double *d_out = nullptr;
    auto chk = [&](int rc, const char *what) { if (rc != GMG_OK) throw std::runtime_error(std::string(what) + ": " + gmg_last_error(gmg)); };
    chk(gmg_vec_alloc(gmg, n, &d_out), "gmg_vec_alloc");
    chk(gmg_rhs_assemble(gmg, (int64_t)active_cells.size(), (int)q_rhs.p.size(), dim, shape.data(), weight.data(), cell_level.data(), jxw_of_level,
                         (int64_t)term_slot.size(), term_slot.data(), term_value.data(), n, dof_ptr.data(), entry_slot.data(), entry_code.data(),
                         coef_table.data(), d_out), "gmg_rhs_assemble");
    chk(gmg_vec_download(gmg, system_rhs.data(), d_out, n), "gmg_vec_download");
    gmg_vec_free(gmg, d_out);
    sublap("assemble: rhs on device");
  }
}

// Is this cycle's right-hand side one gmg_assemble_rhs forms?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_rhs_from_cell_tables() {
  if (!par.rhs_from_cell_tables) return false;
  bool any_inhom = false;
  for (auto &l : constraint_lines) any_inhom = any_inhom || l.inhomogeneity != 0.0;
  const char *why = !solve_on_device_requested                    ? "the cycle does not run on the device"
                    : distributed                                 ? "the run is distributed"
                    : lammpsinput && !densities_device_resident   ? "the charge densities are not on the device"
                    : par.Problemtype == "Step16" && any_inhom    ? "variable coefficient with a nonzero boundary value"
                                                                  : nullptr;
  if (!why) return true;
  if (!rhs_cells_fallback_reported) pcout(std::string("   RHS from cell tables: not applicable (") + why + "), assembled on the host");
  rhs_cells_fallback_reported = true;
  return false;
}

// the tables of the right-hand side's quadrature as assemble_system uses them, and (with_source) the integrand per cell
template <int dim>
typename LaplaceProblem<dim>::RhsAssemblyInputs LaplaceProblem<dim>::rhs_assembly_inputs(bool with_source) {
  constexpr int nv = 1 << dim;
  const Quadrature<dim> q_rhs((int)(par.degree + par.quadrature_degree_rhs));
  RhsAssemblyInputs in;
  const size_t nq = q_rhs.p.size();
  in.nq = (int)nq;
  in.shape.resize(nq * nv);
  in.weight.assign(q_rhs.w.begin(), q_rhs.w.end());
  for (size_t q = 0; q < nq; ++q)
    for (int i = 0; i < nv; ++i) in.shape[q * nv + (size_t)i] = q_rhs.shape[q][(size_t)i];
  in.jxw_of_level.resize(16);
  for (int l = 0; l < 16; ++l) in.jxw_of_level[(size_t)l] = std::pow(triangulation.cell_size(l), dim);
  if (!with_source) return in;
  const int64_t nc = (int64_t)active_cells.size();
  in.source.resize((size_t)nc * nq);
  if (lammpsinput) {
    ensure_host_densities();
    if (density_values_for_each_cell.size() != (size_t)nc) throw std::runtime_error("rhs_assembly_inputs: the charge densities are not those of this mesh");
    for (int64_t ci = 0; ci < nc; ++ci)
      if (density_values_for_each_cell[(size_t)ci].size() != nq) throw std::runtime_error("rhs_assembly_inputs: the charge densities are not those of this quadrature");
    for (int64_t ci = 0; ci < nc; ++ci) std::copy(density_values_for_each_cell[(size_t)ci].begin(), density_values_for_each_cell[(size_t)ci].end(), in.source.begin() + (std::ptrdiff_t)((size_t)ci * nq));
    return in;
  }
#pragma omp parallel for schedule(static)
  for (int64_t ci = 0; ci < nc; ++ci) {
    const auto &ac = active_cells[(size_t)ci];
    const double h = triangulation.cell_size(ac.level);
    double x0[3];
    triangulation.cell_origin(ac.level, triangulation.levels[(size_t)ac.level][(size_t)ac.index], x0);
    for (size_t q = 0; q < nq; ++q) {
      double x[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d) x[d] = x0[d] + h * q_rhs.p[q][(size_t)d];
      in.source[(size_t)ci * nq + q] = rhs_function(x);
    }
  }
  return in;
}

template <int dim>
void LaplaceProblem<dim>::assemble_rhs_from_cell_tables() {
  auto chk = [&](int rc, const char *what) { if (rc != GMG_OK) throw std::runtime_error(std::string(what) + ": " + (gmg ? gmg_last_error(gmg) : last_error.c_str())); };
  chk(ensure_context(), "RHS from cell tables");
  const int64_t n = (int64_t)vertex_of_dof.size();
  SystemAssemblyInputs in = system_assembly_inputs(!operators_resident);
  // GaussianCharges: the densities gmg_charge_density left on the device (source = NULL); otherwise the function's values
  const RhsAssemblyInputs r = rhs_assembly_inputs(!lammpsinput);
  const bool constant_coef = par.Problemtype != "Step16";  // (K_of_level is the constant-coefficient cell matrix: decide_rhs_from_cell_tables)
  double *d_out = nullptr, build_ms = 0.0;
  chk(gmg_vec_alloc(gmg, n, &d_out), "gmg_vec_alloc");
  int rc;
  if (operators_resident)  // the cell tables and the closed lines are the context's
    rc = gmg_assemble_rhs_resident(gmg, constant_coef ? in.K_of_level.data() : nullptr, r.nq, r.shape.data(), r.weight.data(), r.jxw_of_level.data(),
                                   lammpsinput ? nullptr : r.source.data(), d_out, &build_ms);
  else
    rc = gmg_assemble_rhs(gmg, dim, n, (int64_t)active_cells.size(), in.cell_dofs.data(), in.cell_level.data(), constraint_of_dof.data(),
                          (int64_t)constraint_lines.size(), in.line_ptr.data(), in.line_master.data(), in.line_weight.data(),
                          in.line_inhomogeneity.data(), constant_coef ? in.K_of_level.data() : nullptr, r.nq, r.shape.data(), r.weight.data(),
                          r.jxw_of_level.data(), lammpsinput ? nullptr : r.source.data(), d_out, &build_ms);
  if (rc == GMG_OK) rc = gmg_vec_download(gmg, system_rhs.data(), d_out, n);
  gmg_vec_free(gmg, d_out);
  chk(rc, "gmg_assemble_rhs");
  // the line tables stay for gmg_distribute_constraints after this cycle's solves
  cycle_line_tables = SystemAssemblyInputs();
  cycle_line_tables.line_ptr.swap(in.line_ptr); cycle_line_tables.line_master.swap(in.line_master);
  cycle_line_tables.line_weight.swap(in.line_weight); cycle_line_tables.line_inhomogeneity.swap(in.line_inhomogeneity);
  sublap("assemble: rhs from cell tables");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
}

// constraints.distribute of a device vector with this cycle's lines (gmg_distribute_constraints)
template <int dim>
int LaplaceProblem<dim>::distribute_constraints_on_device(double *d_u) {
  // (the tables assemble_rhs_from_cell_tables kept for this cycle: repeated solves of one cycle build nothing)
  if (operators_resident) {  // the closed lines are the context's
    const int rc = gmg_distribute_constraints_resident(gmg, (int64_t)constraint_of_dof.size(), d_u);
    if (rc != GMG_OK) last_error = std::string("gmg_distribute_constraints_resident: ") + gmg_last_error(gmg);
    return rc;
  }
  const SystemAssemblyInputs &t = cycle_line_tables;
  if (t.line_ptr.size() != constraint_lines.size() + 1) { last_error = "gmg_distribute_constraints: no line tables of this cycle"; return GMG_ERR_INVALID; }
  const int rc = gmg_distribute_constraints(gmg, (int64_t)constraint_of_dof.size(), d_u, constraint_of_dof.data(), (int64_t)constraint_lines.size(),
                                            t.line_ptr.data(), t.line_master.data(), t.line_weight.data(), t.line_inhomogeneity.data());
  if (rc != GMG_OK) last_error = std::string("gmg_distribute_constraints: ") + gmg_last_error(gmg);
  return rc;
}

template <int dim>
void LaplaceProblem<dim>::assemble_multigrid() {
  const int L = triangulation.n_levels();
  mg_matrices.assign((size_t)L, {});
  mg_interface_matrices.assign((size_t)L, {});
  level0_on_device = decide_level0_on_device();
  levels_on_device = decide_levels_on_device();
  for (int l = 0; l < L; ++l) {
    if (l == 0 && level0_on_device) continue;  // formed on the device at upload; assembled here only when somebody asks for it
    if (levels_on_device) continue;            // likewise, by gmg_assemble_level_matrix
    assemble_level(l);
  }
}

// Are the level matrices the kind of operator gmg_assemble_level_matrix forms?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_levels_on_device() {
  if (!par.level_matrices_on_device) return false;
  const char *why = !solve_on_device_requested ? "the cycle does not run on the device"
                    : distributed              ? "the run is distributed"
                                               : nullptr;
  if (!why) return true;
  if (!levels_fallback_reported) pcout(std::string("   Level matrices on device: not applicable (") + why + "), assembled on the host");
  levels_fallback_reported = true;
  return false;
}

// the arrays of gmg_assemble_level_matrix besides the cell table: the cell matrix exactly as assemble_level scales it (the
// device's matrices have the host's bits only as long as both scale it the same way) and the two flags of every DoF
template <int dim>
typename LaplaceProblem<dim>::LevelAssemblyInputs LaplaceProblem<dim>::level_assembly_inputs(int l, bool flags) const {
  constexpr int nv = 1 << dim;
  LevelAssemblyInputs in;
  const Quadrature<dim> q_laplace((int)par.degree + 1);
  double Kc[nv][nv];
  cell_matrix<dim>(q_laplace, 1.0, nullptr, Kc);
  const double s = std::pow(triangulation.cell_size(l), dim - 2);
  in.K.resize((size_t)nv * nv);
  for (int i = 0; i < nv; ++i)
    for (int j = 0; j < nv; ++j) in.K[(size_t)i * nv + (size_t)j] = Kc[i][j] * s;
  if (!flags) return in;
  const auto &bnd = level_boundary[(size_t)l];
  const auto &edge = level_refinement_edge[(size_t)l];
  in.dof_flags.resize(bnd.size());
  for (size_t d = 0; d < bnd.size(); ++d) in.dof_flags[d] = (uint8_t)((bnd[d] ? 1 : 0) | (edge[d] ? 2 : 0));
  return in;
}

// Is level 0 the kind of operator gmg_set_level_matrix_lattice forms (and is it going to stay whole on this rank)?
template <int dim>
bool LaplaceProblem<dim>::decide_level0_on_device() const {
  if (!par.level0_matrix_on_device || !solve_on_device_requested || dim != 3 || par.Problemtype == "Step16" || par.level0_numbering != "lexicographic") return false;
  if (triangulation.n0 + 1 < 5) return false;
  if (distributed) {  // the same decision upload() takes about partitioning level 0
    const int64_t n0 = (int64_t)level_vertex_of_dof[0].size();
    const bool peer_transport = comm_id.compare(0, 8, "GMGPEER:") == 0;
    const bool part = par.partition_level0 == "always" ||
                      (par.partition_level0 != "never" && n0 - n0 / n_ranks >= (peer_transport ? kPartitionMinRowsSavedPeer : kPartitionMinRowsSaved));
    if (part) return false;
  }
  return true;
}

// the 8 x 8 cell matrix every level-0 cell adds (constant coefficient), as assemble_level forms it
template <int dim>
void LaplaceProblem<dim>::level0_cell_matrix(double *Ke) const {
  constexpr int nv = 1 << dim;
  const Quadrature<dim> q_laplace((int)par.degree + 1);
  double Kc[nv][nv];
  cell_matrix<dim>(q_laplace, 1.0, nullptr, Kc);
  const double s = std::pow(triangulation.cell_size(0), dim - 2);
  for (int i = 0; i < nv; ++i)
    for (int j = 0; j < nv; ++j) Ke[i * nv + j] = Kc[i][j] * s;
}

template <int dim>
void LaplaceProblem<dim>::ensure_level_matrix(int l) {
  if (l >= 0 && l < (int)mg_matrices.size() && mg_matrices[(size_t)l].n_rows == 0 && !level_vertex_of_dof[(size_t)l].empty()) assemble_level(l);
}

template <int dim>
void LaplaceProblem<dim>::assemble_level(int l) {
  constexpr int nv = 1 << dim;
  const Quadrature<dim> q_laplace((int)par.degree + 1);
  const bool constant_coef = par.Problemtype != "Step16";
  double Kc[nv][nv];
  if (constant_coef) cell_matrix<dim>(q_laplace, 1.0, nullptr, Kc);
  {
    const auto &cells = triangulation.levels[(size_t)l];
    const int64_t n = (int64_t)level_vertex_of_dof[(size_t)l].size();
    std::vector<int64_t> cptr(cells.size() + 1, 0);
    std::vector<int32_t> citems(cells.size() * nv);
    for (size_t ci = 0; ci < cells.size(); ++ci) {
      level_cell_dofs(l, (int32_t)ci, &citems[ci * nv]);
      cptr[ci + 1] = (int64_t)(ci + 1) * nv;
    }
    CSRMatrix &A = mg_matrices[(size_t)l];
    A = pattern_from_cells(n, cptr, citems);
    const auto &bnd = level_boundary[(size_t)l];
    const auto &edge = level_refinement_edge[(size_t)l];
    std::vector<std::array<int64_t, 2>> irc;
    std::vector<double> iv;
    const double h = triangulation.cell_size(l);
    for (size_t ci = 0; ci < cells.size(); ++ci) {
      double K[nv][nv];
      if (constant_coef) {
        const double s = std::pow(h, dim - 2);
        for (int i = 0; i < nv; ++i)
          for (int j = 0; j < nv; ++j) K[i][j] = Kc[i][j] * s;
      } else {
        double x0[3], c[kMaxCoefficientPoints];
        triangulation.cell_origin(l, cells[ci], x0);
        coefficient_values<dim>(*this, q_laplace, h, x0, c);
        cell_matrix<dim>(q_laplace, h, c, K);
      }
      const int32_t *dofs = &citems[ci * nv];
      for (int i = 0; i < nv; ++i) {
        const bool ci_ = bnd[(size_t)dofs[i]] || edge[(size_t)dofs[i]];
        if (ci_) { A.add(dofs[i], dofs[i], std::fabs(K[i][i])); continue; }
        for (int j = 0; j < nv; ++j) {
          const bool cj = bnd[(size_t)dofs[j]] || edge[(size_t)dofs[j]];
          if (!cj) A.add(dofs[i], dofs[j], K[i][j]);
        }
      }
      // interface ("edge") matrix, :892-925: i on the refinement edge, j not, neither on the boundary
      for (int i = 0; i < nv; ++i) {
        if (!edge[(size_t)dofs[i]] || bnd[(size_t)dofs[i]]) continue;
        for (int j = 0; j < nv; ++j)
          if (!edge[(size_t)dofs[j]] && !bnd[(size_t)dofs[j]]) {
            irc.push_back({dofs[i], dofs[j]});
            iv.push_back(K[i][j]);
          }
      }
    }
    mg_interface_matrices[(size_t)l] = csr_from_triplets(n, n, irc, iv, true);
  }
}

template <int dim>
void LaplaceProblem<dim>::build_prolongation(int l) {
  // MGTransferPrebuilt::build_matrices (:957-958) for one level pair: Q1 embedding per child, columns of coarse boundary DoFs
  // zeroed.  With "Transfer matrices on device" the device forms the same operator from the two levels' vertex tables
  // (gmg_build_transfer) and this host version only runs when somebody asks for the matrix (tests, the CPU oracle).
  constexpr int nv = 1 << dim;
  {
    std::vector<std::array<int64_t, 2>> rc;
    std::vector<double> v;
    const auto &cells = triangulation.levels[(size_t)l];
    for (size_t ci = 0; ci < cells.size(); ++ci) {
      if (cells[ci].first_child < 0) continue;
      int32_t pd[nv];
      level_cell_dofs(l, (int32_t)ci, pd);
      for (int a = 0; a < nv; ++a) {
        int32_t cd[nv];
        level_cell_dofs(l + 1, cells[ci].first_child + a, cd);
        for (int b = 0; b < nv; ++b)
          for (int p = 0; p < nv; ++p) {
            double w = 1;
            for (int d = 0; d < dim; ++d) {
              const double pos = 0.5 * (((a >> d) & 1) + ((b >> d) & 1));
              w *= ((p >> d) & 1) ? pos : 1.0 - pos;
            }
            if (w == 0.0 || level_boundary[(size_t)l][(size_t)pd[p]]) continue;
            rc.push_back({cd[b], pd[p]});
            v.push_back(w);
          }
      }
    }
    mg_prolongation[(size_t)l] =
        csr_from_triplets((int64_t)level_vertex_of_dof[(size_t)l + 1].size(), (int64_t)level_vertex_of_dof[(size_t)l].size(), rc, v, false);
  }
}

template <int dim>
void LaplaceProblem<dim>::ensure_prolongation(int l) {
  if (l >= 0 && l < (int)mg_prolongation.size() && mg_prolongation[(size_t)l].n_rows == 0) build_prolongation(l);
}

template <int dim>
void LaplaceProblem<dim>::build_transfer() {
  // mg_transfer.build_matrices (:957-958) + the copy_indices of PreconditionMG (active cells, not on the refinement edge)
  constexpr int nv = 1 << dim;
  const int L = triangulation.n_levels();
  mg_prolongation.assign((size_t)std::max(0, L - 1), {});
  transfer_on_device = par.transfer_on_device && solve_on_device_requested;
  for (int l = 0; l + 1 < L && !transfer_on_device; ++l) build_prolongation(l);
  copy_global.assign((size_t)L, {});
  copy_level.assign((size_t)L, {});
  // (active cells are listed by level, then index: one pass; DoFs from the cell tables, no vertex is looked up)
  std::vector<std::vector<char>> seen((size_t)L);
  for (int l = 0; l < L; ++l) seen[(size_t)l].assign(level_vertex_of_dof[(size_t)l].size(), 0);
  for (size_t ai = 0; ai < active_cells.size(); ++ai) {
    const ActiveCell &ac = active_cells[ai];
    const size_t l = (size_t)ac.level;
    for (int a = 0; a < nv; ++a) {
      const int32_t ld = level_cell_dof_table[l][(size_t)ac.index * nv + (size_t)a];
      if (seen[l][(size_t)ld] || level_refinement_edge[l][(size_t)ld]) continue;
      seen[l][(size_t)ld] = 1;
      copy_global[l].push_back(active_cell_dof_table[ai * nv + (size_t)a]);
      copy_level[l].push_back(ld);
    }
  }
}

// ======================================================================== device hand-over + solve

#define GMGC(call)                                                    \
  do {                                                                \
    const int rc_ = (call);                                           \
    if (rc_ != GMG_OK) {                                              \
      last_error = std::string(#call) + ": " + (gmg ? gmg_last_error(gmg) : "no context"); \
      return rc_;                                                     \
    }                                                                 \
  } while (0)

template <int dim>
int LaplaceProblem<dim>::ensure_context() {
  if (gmg) return GMG_OK;
  const char *dev_env = std::getenv("STEP50_DEVICE");  // one process per GPU: LOCAL_RANK
  const int rc = gmg_create(&gmg, dev_env ? std::atoi(dev_env) : 0, 1);
  if (rc != GMG_OK) { last_error = "gmg_create failed: no usable MI355X / HIP runtime"; gmg = nullptr; return rc; }
  if (distributed) GMGC(gmg_comm_init(gmg, rank, n_ranks, comm_id.data()));  // once: the id is single-use
  return GMG_OK;
}

// "SSOR plan on device": why the host planned a level after all, once per run and cause.  STEP50_CHECK_RESIDENT=1 holds the
// eight numbers of gmg_get_ssor_plan of a device-planned level against a second, host-planned build of the same level.
template <int dim>
int LaplaceProblem<dim>::report_ssor_plan_origin(int l) {
  int on_device = 0;
  const char *why = "";
  GMGC(gmg_get_ssor_plan_origin(gmg, l, &on_device, nullptr, &why));
  if (!on_device) {
    if (why[0] && ssor_plan_reasons_reported.insert(why).second) pcout(std::string("   SSOR plan on device: not applicable (") + why + "), planned on the host");
    return GMG_OK;
  }
  const char *check = std::getenv("STEP50_CHECK_RESIDENT");
  if (!check || check[0] != '1') return GMG_OK;
  int64_t n_rows = 0, n_cols = 0, nnz = 0, dev_plan[8], host_plan[8];
  GMGC(gmg_get_level_matrix(gmg, l, GMG_LEVEL_A, &n_rows, &n_cols, &nnz, nullptr, nullptr, nullptr));
  std::vector<int64_t> rp((size_t)n_rows + 1);
  std::vector<int32_t> col((size_t)std::max<int64_t>(nnz, 1));
  std::vector<double> val((size_t)std::max<int64_t>(nnz, 1));
  GMGC(gmg_get_level_matrix(gmg, l, GMG_LEVEL_A, &n_rows, &n_cols, &nnz, rp.data(), col.data(), val.data()));
  GMGC(gmg_get_ssor_plan(gmg, l, dev_plan));
  // (a context of its own: the level of this run keeps the operator and the plan it has)
  gmg_context *second = nullptr;
  const char *dev_env = std::getenv("STEP50_DEVICE");
  if (gmg_create(&second, dev_env ? std::atoi(dev_env) : 0, l + 1) != GMG_OK) { last_error = "STEP50_CHECK_RESIDENT: no second context"; return GMG_ERR_HIP; }
  int rc2 = gmg_set_option(second, "ssor_plan_device", 0.0);
  if (rc2 == GMG_OK) rc2 = gmg_set_ssor_blocks(second, par.ssor_blocks > 0 ? par.ssor_blocks : 1);
  if (rc2 == GMG_OK) rc2 = gmg_set_level_matrix(second, l, n_rows, n_cols, rp.data(), col.data(), val.data());
  if (rc2 == GMG_OK) rc2 = gmg_get_ssor_plan(second, l, host_plan);
  gmg_destroy(second);
  if (rc2 != GMG_OK) { last_error = "STEP50_CHECK_RESIDENT: the host-planned second build of a level failed"; return rc2; }
  for (int k = 0; k < 8; ++k)
    if (dev_plan[k] != host_plan[k])
      throw std::runtime_error("STEP50_CHECK_RESIDENT: the SSOR plan of level " + std::to_string(l) + " formed on the device differs from the host's (number " +
                               std::to_string(k) + ": " + std::to_string(dev_plan[k]) + " against " + std::to_string(host_plan[k]) + ")");
  return GMG_OK;
}

template <int dim>
int LaplaceProblem<dim>::upload() {
  const int L = triangulation.n_levels();
  const bool had_context = gmg != nullptr && operators_uploaded;
  int rc = ensure_context();
  if (rc != GMG_OK) return rc;
  if (had_context) {  // next adaptive cycle: same context (stream, RCCL communicator), new operators
    for (double *p : {d_solution, d_rhs, d_full})
      if (p) gmg_vec_free(gmg, p);
    d_solution = d_rhs = d_full = nullptr;
    solution_on_device = false;
  }
  // (first upload: the context may have been created early (charge densities) with 1 level.)  gmg_reset drops the mesh
  // tables; with "Operators from resident tables" they are this cycle's and the entries below read them
  if (operators_resident) GMGC(gmg_set_option(gmg, "reset_keeps_mesh_tables", 1.0));
  // "Preconditioner = Jacobi" (:996-1004) needs the system matrix alone: run_cycle assembles no level operator for it, and none
  // is uploaded.  The context is then reset to one (empty) level, the smallest count gmg_reset takes.
  const bool with_levels = par.PreconditionerType == "GMG";
  const int rc_reset = gmg_reset(gmg, with_levels ? L : 1);
  if (operators_resident) GMGC(gmg_set_option(gmg, "reset_keeps_mesh_tables", 0.0));
  GMGC(rc_reset);
  operators_uploaded = true;
  build_matrices_ms = 0.0;
  // before the level matrices: sizes the SGS schedule.  0 = one block per rank: the reference's smoother on that many ranks
  GMGC(gmg_set_ssor_blocks(gmg, par.ssor_blocks > 0 ? par.ssor_blocks : std::max(1, distributed ? n_ranks : 1)));
  // (the default leaves the context's own setting: GMG_OPTIONS=ssor_balanced=1 measures the unchanged driver)
  if (par.ssor_partition == "balanced") GMGC(gmg_set_ssor_partition(gmg, GMG_SSOR_PARTITION_BALANCED));
  if (par.ssor_plan_on_device) GMGC(gmg_set_option(gmg, "ssor_plan_device", 1.0));  // (unset: the context's own setting, as above)
  const CSRMatrix &S = system_matrix;
  const int64_t n_system = (int64_t)vertex_of_dof.size();
  if (system_on_device) {
    // the active-mesh matrix is formed on the device from the cells' DoFs and the constraint lines
    const SystemAssemblyInputs in = system_assembly_inputs(!operators_resident);
    sublap(nullptr);
    double build_ms = 0.0;
    int rc_asm;
    if (operators_resident && par.Problemtype == "Step16") {  // section 22: the cell tables and the closed lines are the context's
      const CoefficientInputs co = system_coefficient_inputs();
      sublap("assemble: coefficient values");
      rc_asm = gmg_assemble_system_matrix_coef_resident(gmg, co.nq, co.cell_coef.data(), co.G.data(), co.qw.data(), co.scale.data(), &build_ms);
    } else if (operators_resident) {
      rc_asm = gmg_assemble_system_matrix_resident(gmg, in.K_of_level.data(), &build_ms);
    } else if (par.Problemtype == "Step16") {
      // section 18: the coefficient varies -- its values at the cells' quadrature points instead of one cell matrix per level
      const CoefficientInputs co = system_coefficient_inputs();
      sublap("assemble: coefficient values");
      rc_asm = gmg_assemble_system_matrix_coef(gmg, dim, n_system, (int64_t)active_cells.size(), in.cell_dofs.data(), in.cell_level.data(), co.nq,
                                               co.cell_coef.data(), co.G.data(), co.qw.data(), co.scale.data(), constraint_of_dof.data(),
                                               (int64_t)constraint_lines.size(), in.line_ptr.data(), in.line_master.data(), in.line_weight.data(),
                                               &build_ms);
    } else {
      rc_asm = gmg_assemble_system_matrix(gmg, dim, n_system, (int64_t)active_cells.size(), in.cell_dofs.data(), in.cell_level.data(),
                                          in.K_of_level.data(), constraint_of_dof.data(), (int64_t)constraint_lines.size(), in.line_ptr.data(),
                                          in.line_master.data(), in.line_weight.data(), &build_ms);
    }
    if (rc_asm == GMG_ERR_UNSUPPORTED) {
      // a mesh the device assembly does not take (a row wider than its limit, sizes beyond 32-bit indices): the host path
      if (!system_fallback_reported) pcout(std::string("   System matrix on device: not applicable (") + gmg_last_error(gmg) + "), assembled on the host");
      system_fallback_reported = true;
      system_on_device = false;
      assemble_system_matrix_host(false);
    } else if (rc_asm != GMG_OK) {
      last_error = std::string("gmg_assemble_system_matrix: ") + gmg_last_error(gmg);
      return rc_asm;
    } else {
      sublap("assemble: matrix on device");
      if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
      d_begin = 0; d_n = d_nvec = n_system;
    }
  }
  if (system_on_device) {  // (formed above)
  } else if (distributed) {
    // system matrix + outer-CG vectors and level 0 are row-partitioned (canonical equal chunks),
    // levels >= 1, transfers and copy indices are replicated.  A level 0 whose
    // coarse-CG iteration is shorter than the three collectives it would need stays replicated.
    const int64_t n0 = (int64_t)level_vertex_of_dof[0].size();
    // rows taken off every rank's coarse iteration against what the exchange costs on the transport in use
    const bool peer_transport = comm_id.compare(0, 8, "GMGPEER:") == 0;
    level0_partitioned = par.partition_level0 == "always" ||
                         (par.partition_level0 != "never" && n0 - n0 / n_ranks >= (peer_transport ? kPartitionMinRowsSavedPeer : kPartitionMinRowsSaved));
    GMGC(gmg_set_global_sizes(gmg, S.n_rows, level0_partitioned ? n0 : 0));
    const LocalOperator Sl = localize(S, rank, n_ranks);
    GMGC(gmg_set_system_matrix(gmg, Sl.A.n_rows, Sl.A.n_cols, Sl.A.rowptr.data(), Sl.A.col.data(), Sl.A.val.data()));
    GMGC(gmg_set_halo_plan(gmg, GMG_SYSTEM, (int)Sl.halo.neighbor_rank.size(), Sl.halo.neighbor_rank.data(),
                           Sl.halo.send_count.data(), Sl.halo.send_idx.data(), Sl.halo.recv_count.data()));
    d_begin = Sl.row_begin; d_n = Sl.A.n_rows; d_nvec = Sl.A.n_cols;
  } else {
    GMGC(gmg_set_system_matrix(gmg, S.n_rows, S.n_cols, S.rowptr.data(), S.col.data(), S.val.data()));
    d_begin = 0; d_n = d_nvec = S.n_rows;
  }
  double levels_build_ms = 0.0, levels_wall_s = 0.0;  // (STEP50_TIMING=2: the device-formed levels, inputs included)
  for (int l = 0; with_levels && l < L; ++l) {
    const bool lattice0 = l == 0 && level0_on_device && !(distributed && level0_partitioned);
    bool level_formed = false;  // A_l and I_l by gmg_assemble_level_matrix
    if (lattice0) {
      // the lattice operator is formed on the device from its size and the cell matrix
      double Ke[64];
      level0_cell_matrix(Ke);
      const int32_t nvv[3] = {triangulation.n0 + 1, triangulation.n0 + 1, triangulation.n0 + 1};
      GMGC(gmg_set_level_matrix_lattice(gmg, 0, nvv, Ke));
    } else if (levels_on_device) {
      // the level's operators are formed on the device from its cell table and the DoF flags
      const auto t_level = std::chrono::steady_clock::now();
      const LevelAssemblyInputs in = level_assembly_inputs(l, !operators_resident);
      double build_ms = 0.0;
      const int64_t n_level = (int64_t)level_vertex_of_dof[(size_t)l].size(), n_level_cells = (int64_t)triangulation.levels[(size_t)l].size();
      int rc_asm;
      if (operators_resident && par.Problemtype == "Step16") {  // section 22: the level's cell table and flags are the context's
        const CoefficientInputs co = level_coefficient_inputs(l);
        rc_asm = gmg_assemble_level_matrix_coef_resident(gmg, l, co.nq, co.cell_coef.data(), co.G.data(), co.qw.data(), co.scale[0], &build_ms);
      } else if (operators_resident) {
        rc_asm = gmg_assemble_level_matrix_resident(gmg, l, in.K.data(), &build_ms);
      } else if (par.Problemtype == "Step16") {  // section 18
        const CoefficientInputs co = level_coefficient_inputs(l);
        rc_asm = gmg_assemble_level_matrix_coef(gmg, l, dim, n_level, n_level_cells, level_cell_dof_table[(size_t)l].data(), co.nq, co.cell_coef.data(),
                                                co.G.data(), co.qw.data(), co.scale[0], in.dof_flags.data(), &build_ms);
      } else {
        rc_asm = gmg_assemble_level_matrix(gmg, l, dim, n_level, n_level_cells, level_cell_dof_table[(size_t)l].data(), in.K.data(), in.dof_flags.data(),
                                           &build_ms);
      }
      if (rc_asm == GMG_ERR_UNSUPPORTED) {
        // a level the device assembly does not take (a row wider than its limit, sizes beyond 32-bit indices): the host path
        if (!levels_fallback_reported) pcout(std::string("   Level matrices on device: not applicable (") + gmg_last_error(gmg) + "), assembled on the host");
        levels_fallback_reported = true;
        levels_on_device = false;
        ensure_level_matrix(l);
      } else if (rc_asm != GMG_OK) {
        last_error = std::string("gmg_assemble_level_matrix: ") + gmg_last_error(gmg);
        return rc_asm;
      } else {
        level_formed = true;
        levels_build_ms += build_ms;
        levels_wall_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_level).count();
      }
    } else {
      ensure_level_matrix(l);
    }
    const CSRMatrix &A = mg_matrices[(size_t)l];
    if (lattice0 || level_formed) {
    } else if (distributed && level0_partitioned && l == 0) {
      const LocalOperator Al = localize(A, rank, n_ranks);
      GMGC(gmg_set_level_matrix(gmg, 0, Al.A.n_rows, Al.A.n_cols, Al.A.rowptr.data(), Al.A.col.data(), Al.A.val.data()));
      GMGC(gmg_set_halo_plan(gmg, 0, (int)Al.halo.neighbor_rank.size(), Al.halo.neighbor_rank.data(), Al.halo.send_count.data(),
                             Al.halo.send_idx.data(), Al.halo.recv_count.data()));
    } else {
      GMGC(gmg_set_level_matrix(gmg, l, A.n_rows, A.n_cols, A.rowptr.data(), A.col.data(), A.val.data()));
    }
    const CSRMatrix &I = mg_interface_matrices[(size_t)l];
    if (!level_formed && I.nnz() > 0) GMGC(gmg_set_edge_matrix(gmg, l, I.n_rows, I.n_cols, I.rowptr.data(), I.col.data(), I.val.data()));
    GMGC(gmg_set_copy_indices(gmg, l, (int64_t)copy_global[(size_t)l].size(), copy_global[(size_t)l].data(), copy_level[(size_t)l].data()));
    if (par.ssor_plan_on_device && l > 0) GMGC(report_ssor_plan_origin(l));
    if (l + 1 < L && transfer_on_device) {
      // P_l and its transpose are formed on the device from the vertex tables of the two levels
      std::vector<uint8_t> bnd(level_boundary[(size_t)l].begin(), level_boundary[(size_t)l].end());
      double ms = 0.0;
      GMGC(gmg_build_transfer(gmg, l, dim, (int64_t)level_vertex_of_dof[(size_t)l].size(), level_vertex_of_dof[(size_t)l].data(), bnd.data(),
                              (int64_t)level_vertex_of_dof[(size_t)l + 1].size(), level_vertex_of_dof[(size_t)l + 1].data(),
                              (uint64_t)1 << (kMaxLevelShift - (l + 1)), &ms));
      build_matrices_ms += ms;
    } else if (l + 1 < L) {
      const CSRMatrix &P = mg_prolongation[(size_t)l];
      GMGC(gmg_set_prolongation(gmg, l, P.n_rows, P.n_cols, P.rowptr.data(), P.col.data(), P.val.data()));
    }
  }
  if (with_levels && levels_on_device && sublap_on()) {
    std::fprintf(stderr, "[step50]     . %-32s %8.3f s\n", "level matrices on device", levels_wall_s);
    std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", levels_build_ms);
  }
  const int kind = par.smoother == "Jacobi" ? GMG_SMOOTHER_JACOBI : par.smoother == "Chebyshev" ? GMG_SMOOTHER_CHEBYSHEV : GMG_SMOOTHER_SSOR;
  if (with_levels) GMGC(gmg_set_smoother(gmg, kind, par.smoother_omega, par.smoother_steps, par.chebyshev_degree, 0.0, 0.0));
  // (all four keys at their defaults: the call is left out, so that the option keys of the context stay in force)
  if (with_levels && (par.chebyshev_polynomial != "first kind" || par.chebyshev_estimate != "Gershgorin" || par.chebyshev_lanczos_steps != 10 ||
                      par.chebyshev_safety != 1.2))
    GMGC(gmg_set_chebyshev(gmg, par.chebyshev_polynomial == "fourth kind" ? GMG_CHEB_FOURTH_KIND : GMG_CHEB_FIRST_KIND,
                           par.chebyshev_estimate == "Lanczos" ? GMG_CHEB_LMAX_LANCZOS : GMG_CHEB_LMAX_GERSHGORIN, par.chebyshev_lanczos_steps,
                           par.chebyshev_safety));
  if (with_levels) GMGC(gmg_set_coarse(gmg, 1e-10, 1000));  // :962
  if (with_levels && par.coarse_solver == "direct") {
    const int rc_cs = gmg_set_coarse_solver(gmg, GMG_COARSE_DIRECT);
    if (rc_cs == GMG_ERR_UNSUPPORTED) {
      if (!coarse_fallback_reported) pcout(std::string("   Coarse solver direct: not applicable (") + gmg_last_error(gmg) + "), coarse CG");
      coarse_fallback_reported = true;
    } else if (rc_cs != GMG_OK) {
      last_error = std::string("gmg_set_coarse_solver: ") + gmg_last_error(gmg);
      return rc_cs;
    }
  }
  GMGC(gmg_vec_alloc(gmg, d_nvec, &d_solution));
  GMGC(gmg_vec_alloc(gmg, d_nvec, &d_rhs));
  const int64_t chunk = (n_system + n_ranks - 1) / n_ranks;
  GMGC(gmg_vec_alloc(gmg, chunk * n_ranks, &d_full));
  GMGC(gmg_vec_upload(gmg, d_rhs, system_rhs.data() + d_begin, d_n));
  GMGC(gmg_comm_barrier(gmg));  // the ranks' assembly times differ by seconds; inside the solve they wait for each other in kernels
  return GMG_OK;
}

int SolverCG_solve(gmg_context *ctx, SolverControl &control, int64_t n, int64_t n_vec, double *x, const double *b,
                   const std::string &preconditioner) {
  // deal.II SolverCG<vector_t>::solve; "GMG" -> PreconditionMG::vmult, "Jacobi" -> omega 0.6 (:996-1004)
  double *g = nullptr, *d = nullptr, *h = nullptr;
  int rc = GMG_OK;
  if ((rc = gmg_vec_alloc(ctx, n_vec, &g)) || (rc = gmg_vec_alloc(ctx, n_vec, &d)) || (rc = gmg_vec_alloc(ctx, n_vec, &h))) return rc;
  auto precondition = [&](double *dst, const double *src) {
    return preconditioner == "GMG" ? gmg_precondition(ctx, dst, src) : gmg_precondition_jacobi(ctx, 0.6, dst, src);
  };
  int it = 0, zero = 0;
  double res = 0, tmp = 0;
  do {
    if ((rc = gmg_vec_all_zero(ctx, x, n, &zero))) break;
    if (!zero) {
      if ((rc = gmg_spmv(ctx, GMG_SYSTEM, g, x))) break;
      gmg_vec_add(ctx, g, -1.0, b, n);
    } else {
      gmg_vec_equ(ctx, g, -1.0, b, n);
    }
    if ((rc = gmg_vec_dot(ctx, g, g, n, &tmp))) break;
    res = std::sqrt(tmp);
    control.initial_value = res;
    if (res <= control.tolerance) break;
    if ((rc = precondition(h, g))) break;
    if ((rc = gmg_cg_direction_step(ctx, d, g, h, n, 1))) break;  // d = -h; gh = g.h, kept by the library
    for (;;) {
      ++it;
      if ((rc = gmg_spmv(ctx, GMG_SYSTEM, h, d))) break;
      // alpha = gh / d.h; x += alpha d; g += alpha h; |g|^2: the one value SolverControl needs on the host
      if ((rc = gmg_cg_update_step(ctx, x, g, d, h, n, &tmp))) break;
      res = std::sqrt(tmp);
      if (res <= control.tolerance) break;
      if (it >= control.max_steps || res != res) { rc = GMG_ERR_OUTER_NOCONV; break; }
      if ((rc = precondition(h, g))) break;
      if ((rc = gmg_cg_direction_step(ctx, d, g, h, n, 0))) break;  // beta = g.h / gh; d = beta d - h; gh = g.h
    }
  } while (0);
  control.last_step = it;
  control.last_value = res;
  gmg_synchronize(ctx);
  gmg_vec_free(ctx, g); gmg_vec_free(ctx, d); gmg_vec_free(ctx, h);
  return rc;
}

template <int dim>
int LaplaceProblem<dim>::solve_on_device(CycleReport &rep) {
  GMGC(gmg_vec_upload(gmg, d_solution, initial_guess.data() + d_begin, d_n));
  gmg_stats st0;
  gmg_stats_get(gmg, &st0);
  double l1, l2, li;
  GMGC(gmg_vec_norms(gmg, d_rhs, d_n, &l1, &l2, &li));  // system_rhs.l2_norm(), :942
  SolverControl control{500, 1e-8 * l2};
  GMGC(gmg_synchronize(gmg));
  const auto t0 = std::chrono::steady_clock::now();
  int rc;
  if (par.device_resident_outer_cg) {
    rc = gmg_cg_solve(gmg, d_solution, d_rhs, 1e-8, 500, par.PreconditionerType == "GMG" ? GMG_PRECOND_GMG : GMG_PRECOND_JACOBI,
                      &control.last_step, &control.initial_value, &control.last_value);
  } else {
    rc = SolverCG_solve(gmg, control, d_n, d_nvec, d_solution, d_rhs, par.PreconditionerType);
  }
  gmg_synchronize(gmg);
  rep.solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  rep.build_matrices_ms = build_matrices_ms;
  rep.starting_value = control.initial_value;
  rep.cg_iterations = control.last_step;
  rep.convergence_value = control.last_value;
  rep.status = rc;
  gmg_stats st;
  gmg_stats_get(gmg, &st);
  rep.coarse_iterations = st.coarse_iterations - st0.coarse_iterations;
  rep.coarse_solver = (int)st.coarse_solver;
  if (rc != GMG_OK) { last_error = std::string("solve: ") + gmg_last_error(gmg); return rc; }
  GMGC(gmg_vec_norms(gmg, d_solution, d_n, &rep.sol_l1, &rep.sol_l2, &rep.sol_linf));  // :1012-1014
  GMGC(gmg_vec_allgather(gmg, (int64_t)solution.size(), d_full, d_solution));  // every rank keeps the whole solution
  // "RHS from cell tables": constraints.distribute (:1016) on the device before the one download; d_full then stays the
  // solution for the estimator, the forces and the error norm (device_solution) until the next cycle
  if (rhs_from_cells) {
    sublap("solve: up to the distribution");  // (a labelled lap, not a restart: whatever a caller's next lap covers, it covers with the key off and on)
    GMGC(distribute_constraints_on_device(d_full));
    sublap("solve: distribute on device");
  }
  GMGC(gmg_vec_download(gmg, solution.data(), d_full, (int64_t)solution.size()));
  solution_on_device = rhs_from_cells;
  return GMG_OK;
}

template <int dim>
int LaplaceProblem<dim>::solve() {
  // :938-1017.  The operators were handed over by upload(); this is the timed hot path.
  CycleReport &rep = reports.back();
  rep.rhs_l1 = rep.rhs_l2 = rep.rhs_linf = 0;
  for (double v : system_rhs) { rep.rhs_l1 += std::fabs(v); rep.rhs_l2 += v * v; rep.rhs_linf = std::max(rep.rhs_linf, std::fabs(v)); }
  rep.rhs_l2 = std::sqrt(rep.rhs_l2);
  if (system_on_device && system_matrix.n_rows == 0) {  // the matrix exists on the device only
    GMGC(gmg_system_matrix_norms(gmg, &rep.matrix_l1, &rep.matrix_linf, &rep.matrix_frobenius));
  } else {
    rep.matrix_l1 = system_matrix.l1_norm();
    rep.matrix_linf = system_matrix.linfty_norm();
    rep.matrix_frobenius = system_matrix.frobenius_norm();
  }
  pcout("   L1 rhs norm " + fmt("%.10e", rep.rhs_l1));
  pcout("   L2 rhs norm " + fmt("%.10e", rep.rhs_l2));
  pcout("   LInfinity rhs norm " + fmt("%.10e", rep.rhs_linf));
  pcout("   L1 Matrix norm " + fmt("%.10e", rep.matrix_l1));
  pcout("   LInfinity Matrix norm " + fmt("%.10e", rep.matrix_linf));
  pcout("   Frobenius Matrix norm " + fmt("%.10e", rep.matrix_frobenius));
  const int rc = solve_on_device(rep);
  if (rc != GMG_OK) return rc;
  pcout("   Starting value " + fmt("%.10f", rep.starting_value));
  pcout("   CG converged in " + std::to_string(rep.cg_iterations) + " iterations.");
  pcout("   Convergence value " + fmt("%.10e", rep.convergence_value));
  pcout("   L1 solution norm " + fmt("%.10e", rep.sol_l1));
  pcout("   L2 solution norm " + fmt("%.10e", rep.sol_l2));
  pcout("   LInfinity solution norm " + fmt("%.10e", rep.sol_linf));
  if (!solution_on_device) distribute_constraints(solution);  // :1016 (else: done on the device before the download)
  return GMG_OK;
}

template <int dim>
int LaplaceProblem<dim>::solve_again() {
  CycleReport rep = reports.back();
  const int rc = solve_on_device(rep);
  reports.back().solve_seconds = rep.solve_seconds;
  reports.back().cg_iterations = rep.cg_iterations;
  reports.back().coarse_iterations = rep.coarse_iterations;
  reports.back().coarse_solver = rep.coarse_solver;
  return rc;
}

// bench: the operators of the current cycle with another smoother ("Jacobi" | "SSOR" | "Chebyshev"; SSOR in
// `ssor_blocks` blocks = the reference's smoother on that many ranks, cut as "SSOR block partition" says).  The SGS schedule
// is built at upload.
template <int dim>
int LaplaceProblem<dim>::set_smoother(const std::string &smoother, int ssor_blocks) {
  if (smoother != "Jacobi" && smoother != "SSOR" && smoother != "Chebyshev") { last_error = "unknown smoother " + smoother; return GMG_ERR_INVALID; }
  if (!operators_uploaded) { last_error = "set_smoother: no cycle has been run"; return GMG_ERR_INVALID; }
  par.smoother = smoother;
  par.ssor_blocks = std::max(0, ssor_blocks);
  return upload();
}

template <int dim>
void LaplaceProblem<dim>::distribute_constraints(std::vector<double> &u) const {
  for (size_t i = 0; i < constraint_of_dof.size(); ++i) {
    const int32_t cl = constraint_of_dof[i];
    if (cl < 0) continue;
    const ConstraintLine &line = constraint_lines[(size_t)cl];
    double v = line.inhomogeneity;
    for (auto &e : line.entries) v += e.second * u[(size_t)e.first];
    u[i] = v;
  }
}
template <int dim>
void LaplaceProblem<dim>::set_zero_constraints(std::vector<double> &u) const {
  for (size_t i = 0; i < constraint_of_dof.size(); ++i)
    if (constraint_of_dof[i] >= 0) u[i] = 0.0;
}

// ======================================================================== post-processing

template <int dim>
double LaplaceProblem<dim>::fe_value_at(const std::vector<double> &u, const double x[3]) const {
  // GridTools::find_active_cell_around_point + FEValues::get_function_values (:1354-1363)
  int c[3] = {0, 0, 0};
  for (int d = 0; d < dim; ++d) {
    c[d] = (int)std::floor((x[d] - triangulation.origin) / triangulation.h0);
    c[d] = std::min(std::max(c[d], 0), triangulation.n0 - 1);
  }
  int level = 0;
  int32_t ci = triangulation.find(0, c[0], c[1], c[2]);
  while (!triangulation.active(level, ci)) {
    const Cell &cell = triangulation.levels[(size_t)level][(size_t)ci];
    const double h = triangulation.cell_size(level);
    double x0[3];
    triangulation.cell_origin(level, cell, x0);
    int a = 0;
    for (int d = 0; d < dim; ++d)
      if (x[d] >= x0[d] + 0.5 * h) a |= 1 << d;
    ci = cell.first_child + a;
    ++level;
  }
  const Cell &cell = triangulation.levels[(size_t)level][(size_t)ci];
  const double h = triangulation.cell_size(level);
  double x0[3];
  triangulation.cell_origin(level, cell, x0);
  double t[3] = {0, 0, 0};
  for (int d = 0; d < dim; ++d) t[d] = (x[d] - x0[d]) / h;
  double v = 0;
  const_cast<LaplaceProblem<dim> *>(this)->ensure_dof_maps();  // ("Mesh tables on device" leaves the hash tables to their first use; callers are sequential)
  for (int a = 0; a < (1 << dim); ++a) {
    double w = 1;
    for (int d = 0; d < dim; ++d) w *= ((a >> d) & 1) ? t[d] : 1.0 - t[d];
    v += w * u[(size_t)dof_of_vertex.at(triangulation.vertex_key(level, cell, a))];
  }
  return v;
}

template <int dim>
void LaplaceProblem<dim>::postprocess_electrostatic_energy() {
  // :1310-1420
  CycleReport &rep = reports.back();
  double analytical = 0, shortr = 0, fe = 0, self = 0;
  const bool large = number_of_atoms >= 300;  // the reference's gate (:1554): the all-pairs sums are O(N^2)
  const double rcut = par.short_range_cutoff * par.r_c;
  // "Energy and forces from resident tables" (DESIGN.md section 25): the three sums come back from the device, 24 bytes
  const bool resident = energy_forces_resident_applies() && gmg != nullptr;
  if (!large)
    for (unsigned i = 0; i < number_of_atoms; ++i)
      for (unsigned j = i + 1; j < number_of_atoms; ++j) {
        double r2 = 0;
        for (int d = 0; d < 3; ++d) { const double t = atom_positions[3 * i + (size_t)d] - atom_positions[3 * j + (size_t)d]; r2 += t * t; }
        analytical += charges[i] * charges[j] / std::sqrt(r2);
      }
  if (resident) {
    ensure_point_locator_resident();
    double sums[3] = {0, 0, 0}, build_ms = 0.0;
    sublap(nullptr);
    if (gmg_electrostatic_energy_resident(gmg, triangulation.origin, triangulation.h0, (int64_t)number_of_atoms, atom_positions.data(), charges.data(),
                                          device_solution(), (int64_t)solution.size(), par.r_c, std::max(par.short_range_cutoff, 0.0), sums, &build_ms) != GMG_OK)
      throw std::runtime_error(std::string("gmg_electrostatic_energy_resident: ") + gmg_last_error(gmg));
    sublap("energy: sums on device");
    if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
    shortr = sums[0]; fe = sums[1]; self = sums[2];
    const char *check = std::getenv("STEP50_CHECK_RESIDENT");
    if (check && std::atoi(check) != 0) {  // fe and self by the host's loops (phi_h through the host mirror of atom_phi: no hash tables)
      std::vector<int32_t> node;
      point_locator(node);
      const gmg_forces::Locator L{{triangulation.n0, triangulation.n0, triangulation.n0}, {triangulation.origin, triangulation.origin, triangulation.origin},
                                  triangulation.h0, node.data(), active_cell_dof_table.data()};
      double h_fe = 0, h_self = 0;
      for (unsigned i = 0; i < number_of_atoms; ++i) {
        h_fe += 0.5 * charges[i] * gmg_forces::atom_phi(L, solution.data(), &atom_positions[3 * i]);
        h_self += charges[i] * charges[i] / (std::sqrt(M_PI) * par.r_c);
      }
      if (std::memcmp(&h_fe, &fe, sizeof(double)) != 0 || std::memcmp(&h_self, &self, sizeof(double)) != 0)
        throw std::logic_error("Energy and forces from resident tables: the device's fe or self sum differs from the host's");
    }
  } else if (rcut <= 0.0) {  // the reference's loop (:1325-1332)
    for (unsigned i = 0; i < number_of_atoms; ++i)
      for (unsigned j = i + 1; j < number_of_atoms; ++j) {
        double r2 = 0;
        for (int d = 0; d < 3; ++d) { const double t = atom_positions[3 * i + (size_t)d] - atom_positions[3 * j + (size_t)d]; r2 += t * t; }
        const double r = std::sqrt(r2);
        shortr += charges[i] * (charges[j] * (std::erfc(r / par.r_c) / r));
      }
  } else {
    // pairs closer than rcut through bins of edge rcut: per atom i the atoms j > i of the 27 neighbouring bins, j ascending
    // -- the reference's i < j order restricted to the pairs that contribute
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (unsigned i = 0; i < number_of_atoms; ++i)
      for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], atom_positions[3 * i + (size_t)d]); hi[d] = std::max(hi[d], atom_positions[3 * i + (size_t)d]); }
    int bn[3];
    for (int d = 0; d < 3; ++d) bn[d] = std::max(1, std::min(512, (int)std::floor((hi[d] - lo[d]) / rcut) + 1));
    auto bin_of = [&](unsigned i, int b[3]) { for (int d = 0; d < 3; ++d) b[d] = std::min(bn[d] - 1, std::max(0, (int)std::floor((atom_positions[3 * i + (size_t)d] - lo[d]) / rcut))); };
    std::vector<std::vector<unsigned>> bins((size_t)bn[0] * bn[1] * bn[2]);
    for (unsigned i = 0; i < number_of_atoms; ++i) { int b[3]; bin_of(i, b); bins[(size_t)b[0] + (size_t)bn[0] * ((size_t)b[1] + (size_t)bn[1] * b[2])].push_back(i); }
    std::vector<double> part(number_of_atoms, 0.0);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t ii = 0; ii < (int64_t)number_of_atoms; ++ii) {
      const unsigned i = (unsigned)ii;
      int b[3];
      bin_of(i, b);
      std::vector<unsigned> cand;
      for (int z = std::max(0, b[2] - 1); z <= std::min(bn[2] - 1, b[2] + 1); ++z)
        for (int y = std::max(0, b[1] - 1); y <= std::min(bn[1] - 1, b[1] + 1); ++y)
          for (int x = std::max(0, b[0] - 1); x <= std::min(bn[0] - 1, b[0] + 1); ++x)
            for (unsigned j : bins[(size_t)x + (size_t)bn[0] * ((size_t)y + (size_t)bn[1] * z)])
              if (j > i) cand.push_back(j);
      std::sort(cand.begin(), cand.end());
      double acc = 0.0;
      for (unsigned j : cand) {
        double r2 = 0;
        for (int d = 0; d < 3; ++d) { const double t = atom_positions[3 * i + (size_t)d] - atom_positions[3 * j + (size_t)d]; r2 += t * t; }
        const double r = std::sqrt(r2);
        if (r < rcut) acc += charges[i] * (charges[j] * (std::erfc(r / par.r_c) / r));
      }
      part[i] = acc;
    }
    for (unsigned i = 0; i < number_of_atoms; ++i) shortr += part[i];  // fixed order: deterministic
  }
  if (!resident)
    for (unsigned i = 0; i < number_of_atoms; ++i) {
      fe += 0.5 * charges[i] * fe_value_at(solution, &atom_positions[3 * i]);
      self += charges[i] * charges[i] / (std::sqrt(M_PI) * par.r_c);
    }
  rep.has_energy = true;
  rep.energy_analytical = analytical; rep.energy_short = shortr; rep.energy_fe_long = fe; rep.energy_self = self;
  rep.energy_total = shortr + fe - self;
  rep.energy_abs_error = std::fabs(std::fabs(analytical) - std::fabs(rep.energy_total));
  if (large) pcout("\nTotal analytical electrostatic energy :   (not evaluated: all pairs of " + std::to_string(number_of_atoms) + " atoms)");
  else pcout("\nTotal analytical electrostatic energy :   " + fmt("%.10e", analytical));
  pcout("Short-ranged energy contribution :  " + fmt("%.10e", shortr));
  pcout("FE solution long-ranged energy contribution :    " + fmt("%.10e", fe));
  pcout("Self energy contribution : " + fmt("%.10e", self));
  pcout("Total electrostatic energy with split in short- and long-ranged : " + fmt("%.10e", rep.energy_total));
  pcout("Absolute Error between both energies :\t" + fmt("%.10e", rep.energy_abs_error) + "\n");
  pcout("Relative Error in total electrostatic energy :\t" + fmt("%.10e", std::fabs((std::fabs(analytical) - std::fabs(rep.energy_total)) / analytical)));
}

template <int dim>
void LaplaceProblem<dim>::point_locator(std::vector<int32_t> &node) const {
  const int L = triangulation.n_levels();
  std::vector<int64_t> off((size_t)L + 1, 0);
  for (int l = 0; l < L; ++l) off[(size_t)l + 1] = off[(size_t)l] + (int64_t)triangulation.levels[(size_t)l].size();
  node.resize((size_t)off[(size_t)L]);
  for (int l = 0; l < L; ++l)
    for (size_t c = 0; c < triangulation.levels[(size_t)l].size(); ++c) {
      const Cell &cell = triangulation.levels[(size_t)l][c];
      node[(size_t)off[(size_t)l] + c] = cell.first_child >= 0 ? (int32_t)(off[(size_t)l + 1] + cell.first_child)
                                                                : -active_index_of_cell[(size_t)l][c] - 1;
    }
}

template <int dim>
int LaplaceProblem<dim>::atom_forces(bool on_device, double cutoff, std::vector<double> *phi, std::vector<double> *field,
                                     std::vector<double> *force, std::vector<double> *force_short, std::vector<double> *e_short) {
  if (dim != 3) { last_error = "atom forces: 3D only"; return GMG_ERR_UNSUPPORTED; }
  if (solution.size() != vertex_of_dof.size() || active_cells.empty()) { last_error = "atom forces: no solution of this mesh"; return GMG_ERR_INVALID; }
  const int64_t n = number_of_atoms;
  for (std::vector<double> *v : {phi, e_short})
    if (v) v->assign((size_t)n, 0.0);
  for (std::vector<double> *v : {field, force, force_short})
    if (v) v->assign((size_t)n * 3, 0.0);
  auto data = [](std::vector<double> *v) { return v ? v->data() : nullptr; };
  if (on_device && gmg != nullptr && energy_forces_resident_applies()) {  // no node array, no cell table crosses the bus
    ensure_point_locator_resident();
    const int rc = gmg_atom_forces_resident(gmg, triangulation.origin, triangulation.h0, n, atom_positions.data(), charges.data(), device_solution(),
                                            (int64_t)solution.size(), par.r_c, cutoff, data(phi), data(field), data(force), data(force_short), data(e_short));
    if (rc != GMG_OK) last_error = std::string("gmg_atom_forces_resident: ") + gmg_last_error(gmg);
    return rc;
  }
  std::vector<int32_t> node;
  point_locator(node);
  const int32_t n0[3] = {triangulation.n0, triangulation.n0, triangulation.n0};
  const double origin[3] = {triangulation.origin, triangulation.origin, triangulation.origin};
  if (on_device) {
    GMGC(ensure_context());
    GMGC(gmg_set_point_locator(gmg, n0, origin, triangulation.h0, (int64_t)node.size(), node.data(), (int64_t)active_cells.size(),
                               active_cell_dof_table.data()));
    const double *u_dev = device_solution();  // ("RHS from cell tables": the device kept the distributed solution)
    double *d_u = nullptr;
    if (!u_dev) GMGC(gmg_vec_alloc(gmg, (int64_t)solution.size(), &d_u));
    int rc = u_dev ? GMG_OK : gmg_vec_upload(gmg, d_u, solution.data(), (int64_t)solution.size());
    if (!u_dev) u_dev = d_u;
    if (rc == GMG_OK)
      rc = gmg_atom_forces(gmg, n, atom_positions.data(), charges.data(), u_dev, (int64_t)solution.size(), par.r_c, cutoff, data(phi),
                           data(field), data(force), data(force_short), data(e_short));
    if (rc != GMG_OK) last_error = std::string("gmg_atom_forces: ") + gmg_last_error(gmg);
    if (d_u) gmg_vec_free(gmg, d_u);
    return rc;
  }
  // host mirror: the same per-atom functions (gmg_forces.hpp), one atom per iteration
  const gmg_forces::Locator L{{n0[0], n0[1], n0[2]}, {origin[0], origin[1], origin[2]}, triangulation.h0, node.data(),
                              active_cell_dof_table.data()};
  std::vector<double> E((size_t)n * 3), pair((size_t)n * 4, 0.0), xq((size_t)n * 4);
  for (int64_t i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) xq[(size_t)(4 * i + d)] = atom_positions[(size_t)(3 * i + d)];
    xq[(size_t)(4 * i + 3)] = charges[(size_t)i];
  }
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; ++i) {
    double p;
    gmg_forces::atom_field(L, solution.data(), &atom_positions[(size_t)(3 * i)], p, &E[(size_t)(3 * i)]);
    if (phi) (*phi)[(size_t)i] = p;
  }
  const gmg_forces::ShortLaw law = gmg_forces::ShortLaw::make(par.r_c);
  if (cutoff > 0.0) {
    gmg_forces::Bins B;
    gmg_forces::force_bins(n, atom_positions.data(), cutoff * par.r_c, B);
    std::vector<double> sorted((size_t)n * 4);
    for (int64_t k = 0; k < n; ++k)
      for (int c = 0; c < 4; ++c) sorted[(size_t)(4 * k + c)] = xq[4 * (size_t)B.items[(size_t)k] + c];
    const int64_t n_bins = (int64_t)B.ptr.size() - 1;
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t b = 0; b < n_bins; ++b)
      for (int64_t k = B.ptr[(size_t)b]; k < B.ptr[(size_t)b + 1]; ++k) {
        double acc[4] = {0, 0, 0, 0};
        gmg_forces::for_each_row(B.n, B.ptr.data(), b, [&](int64_t ks, int64_t ke) {
          for (int64_t kj = ks; kj < ke; ++kj)
            if (kj != k) gmg_forces::pair_add(law, cutoff * par.r_c, &sorted[(size_t)(4 * k)], &sorted[(size_t)(4 * kj)], acc);
        });
        double *o = &pair[4 * (size_t)B.items[(size_t)k]];
        for (int c = 0; c < 3; ++c) o[c] = acc[c];
        o[3] = 0.5 * acc[3];
      }
  } else {
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n; ++i) {
      double acc[4] = {0, 0, 0, 0};
      for (int64_t j = 0; j < n; ++j)
        if (j != i) gmg_forces::pair_add(law, INFINITY, &xq[(size_t)(4 * i)], &xq[(size_t)(4 * j)], acc);
      for (int c = 0; c < 3; ++c) pair[(size_t)(4 * i + c)] = acc[c];
      pair[(size_t)(4 * i + 3)] = 0.5 * acc[3];
    }
  }
  for (int64_t i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) {
      if (field) (*field)[(size_t)(3 * i + d)] = E[(size_t)(3 * i + d)];
      if (force_short) (*force_short)[(size_t)(3 * i + d)] = pair[(size_t)(4 * i + d)];
      if (force) (*force)[(size_t)(3 * i + d)] = charges[(size_t)i] * E[(size_t)(3 * i + d)] + pair[(size_t)(4 * i + d)];
    }
    if (e_short) (*e_short)[(size_t)i] = pair[(size_t)(4 * i + 3)];
  }
  return GMG_OK;
}

template <int dim>
int LaplaceProblem<dim>::direct_coulomb(bool on_device, std::vector<double> *force, std::vector<double> *energy) {
  const int64_t n = number_of_atoms;
  if (force) force->assign((size_t)n * 3, 0.0);
  if (energy) energy->assign((size_t)n, 0.0);
  if (on_device) {
    GMGC(ensure_context());
    GMGC(gmg_direct_coulomb(gmg, n, atom_positions.data(), charges.data(), force ? force->data() : nullptr, energy ? energy->data() : nullptr));
    return GMG_OK;
  }
  std::vector<double> xq((size_t)n * 4);
  for (int64_t i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) xq[(size_t)(4 * i + d)] = atom_positions[(size_t)(3 * i + d)];
    xq[(size_t)(4 * i + 3)] = charges[(size_t)i];
  }
  const gmg_forces::DirectLaw law;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < n; ++i) {
    double acc[4] = {0, 0, 0, 0};
    for (int64_t j = 0; j < n; ++j)
      if (j != i) gmg_forces::pair_add(law, INFINITY, &xq[(size_t)(4 * i)], &xq[(size_t)(4 * j)], acc);
    if (force)
      for (int c = 0; c < 3; ++c) (*force)[(size_t)(3 * i + c)] = acc[c];
    if (energy) (*energy)[(size_t)i] = 0.5 * acc[3];
  }
  return GMG_OK;
}

template <int dim>
int LaplaceProblem<dim>::gaussian_potential(bool on_device, int64_t n_points, const double *points, double *phi, double *grad) {
  if (dim != 3) { last_error = "exact potential: 3D only"; return GMG_ERR_UNSUPPORTED; }
  const int64_t n = number_of_atoms;
  if (on_device) {
    // (a context is enough: the call uses no level data, so it also works before the cycle's operators exist)
    GMGC(ensure_context());
    GMGC(gmg_gaussian_potential(gmg, n, atom_positions.data(), charges.data(), par.r_c, n_points, points, phi, grad));
    return GMG_OK;
  }
  // host mirror: the same per-pair functions (gmg_exact.hpp), one point per iteration, atoms in ascending order
  const gmg_exact::Gauss g = gmg_exact::Gauss::make(par.r_c);
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t p = 0; p < n_points; ++p) {
    double v = 0.0, ga[3] = {0.0, 0.0, 0.0};
    for (int64_t i = 0; i < n; ++i) {
      double dir[3];
      const double r = gmg_exact::distance(points + 3 * p, &atom_positions[(size_t)(3 * i)], dir);
      if (phi) v += gmg_exact::value(g, r, charges[(size_t)i]);
      if (grad) gmg_exact::gradient_add(g, r, charges[(size_t)i], dir, ga);
    }
    if (phi) phi[p] = v;
    if (grad)
      for (int d = 0; d < 3; ++d) grad[3 * p + d] = ga[d];
  }
  return GMG_OK;
}

template <int dim>
int LaplaceProblem<dim>::energy_norm_error(bool on_device, double *error, std::vector<double> *cell_err2) {
  if (dim != 3) { last_error = "energy norm error: 3D only"; return GMG_ERR_UNSUPPORTED; }
  if (solution.size() != vertex_of_dof.size() || active_cells.empty()) { last_error = "energy norm error: no solution of this mesh"; return GMG_ERR_INVALID; }
  constexpr int nv = 1 << dim;
  const Quadrature<dim> quad((int)par.degree + 1);  // QGauss(degree + 1), :1427
  const int nq = (int)quad.p.size();
  const int64_t nc = (int64_t)active_cells.size(), n = number_of_atoms;
  // ("Estimator from resident tables": the device forms the cells' corners and edges from its own tables, section 24)
  const bool resident = on_device && lammpsinput && estimator_resident_applies();
  const int64_t ng = resident ? 0 : nc;
  std::vector<double> lo((size_t)(3 * ng)), hh((size_t)ng), qp((size_t)(3 * nq)), sg((size_t)(24 * nq), 0.0), ce((size_t)nc, 0.0);
  for (int64_t ci = 0; ci < ng; ++ci) {
    const ActiveCell &ac = active_cells[(size_t)ci];
    double x0[3];
    triangulation.cell_origin(ac.level, triangulation.levels[(size_t)ac.level][(size_t)ac.index], x0);
    for (int d = 0; d < 3; ++d) lo[(size_t)(3 * ci + d)] = x0[d];
    hh[(size_t)ci] = triangulation.cell_size(ac.level);
  }
  for (int q = 0; q < nq; ++q)
    for (int d = 0; d < 3; ++d) {
      qp[(size_t)(3 * q + d)] = quad.p[(size_t)q][(size_t)d];
      for (int a = 0; a < nv; ++a) sg[(size_t)(24 * q + 3 * a + d)] = quad.grad[(size_t)q][(size_t)a][(size_t)d];
    }
  if (on_device) {
    GMGC(ensure_context());
    const double *u_dev = device_solution();  // ("RHS from cell tables": the device kept the distributed solution)
    double *d_u = nullptr;
    if (!u_dev) GMGC(gmg_vec_alloc(gmg, (int64_t)solution.size(), &d_u));
    int rc = u_dev ? GMG_OK : gmg_vec_upload(gmg, d_u, solution.data(), (int64_t)solution.size());
    if (!u_dev) u_dev = d_u;
    if (rc == GMG_OK && resident)
      rc = gmg_energy_norm_error_resident(gmg, triangulation.origin, triangulation.h0, u_dev, (int64_t)solution.size(), n, atom_positions.data(),
                                          charges.data(), par.r_c, nq, qp.data(), quad.w.data(), sg.data(), error, cell_err2 ? ce.data() : nullptr);
    else if (rc == GMG_OK)
      rc = gmg_energy_norm_error(gmg, nc, lo.data(), hh.data(), active_cell_dof_table.data(), u_dev, (int64_t)solution.size(), n,
                                 atom_positions.data(), charges.data(), par.r_c, nq, qp.data(), quad.w.data(), sg.data(), error,
                                 cell_err2 ? ce.data() : nullptr);
    if (rc != GMG_OK) last_error = std::string(resident ? "gmg_energy_norm_error_resident: " : "gmg_energy_norm_error: ") + gmg_last_error(gmg);
    if (d_u) gmg_vec_free(gmg, d_u);
    if (rc == GMG_OK && cell_err2) cell_err2->swap(ce);
    return rc;
  }
  // host mirror: one cell per iteration, its quadrature points in ascending order, then the cells in ascending order
  const gmg_exact::Gauss g = gmg_exact::Gauss::make(par.r_c);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t ci = 0; ci < nc; ++ci) {
    const double h = hh[(size_t)ci];
    double s = 0.0;
    for (int q = 0; q < nq; ++q) {
      double x[3], ga[3] = {0.0, 0.0, 0.0};
      for (int d = 0; d < 3; ++d) x[d] = lo[(size_t)(3 * ci + d)] + h * qp[(size_t)(3 * q + d)];
      for (int64_t i = 0; i < n; ++i) {
        double dir[3];
        const double r = gmg_exact::distance(x, &atom_positions[(size_t)(3 * i)], dir);
        gmg_exact::gradient_add(g, r, charges[(size_t)i], dir, ga);
      }
      s += gmg_exact::point_err2(solution.data(), &active_cell_dof_table[(size_t)(8 * ci)], &sg[(size_t)(24 * q)], h, quad.w[(size_t)q], ga);
    }
    ce[(size_t)ci] = s;
  }
  double total = 0.0;
  for (int64_t ci = 0; ci < nc; ++ci) total += ce[(size_t)ci];
  if (error) *error = std::sqrt(total);
  if (cell_err2) cell_err2->swap(ce);
  return GMG_OK;
}

template <int dim>
void LaplaceProblem<dim>::postprocess_forces() {
  CycleReport &rep = reports.back();
  const bool dev = forces_on_device();
  std::vector<double> F, Fd;
  if (atom_forces(dev, par.short_range_cutoff, nullptr, nullptr, &F, nullptr, nullptr) != GMG_OK) throw std::runtime_error(last_error);
  double net[3] = {0, 0, 0}, fmax = 0;
  for (unsigned i = 0; i < number_of_atoms; ++i) {
    double f2 = 0;
    for (int d = 0; d < 3; ++d) { net[d] += F[3 * i + (size_t)d]; f2 += F[3 * i + (size_t)d] * F[3 * i + (size_t)d]; }
    fmax = std::max(fmax, std::sqrt(f2));
  }
  rep.has_forces = true;
  for (int d = 0; d < 3; ++d) rep.force_net[d] = net[d];
  rep.force_max = fmax;
  pcout("Net force on the atoms : (" + fmt("%.10e", net[0]) + ", " + fmt("%.10e", net[1]) + ", " + fmt("%.10e", net[2]) + ")");
  pcout("Largest force on an atom :  " + fmt("%.10e", fmax));
  if (!par.direct_coulomb_check) return;
  if (direct_coulomb(dev, &Fd, nullptr) != GMG_OK) throw std::runtime_error(last_error);
  double num = 0, den = 0;
  for (size_t k = 0; k < F.size(); ++k) { num += (F[k] - Fd[k]) * (F[k] - Fd[k]); den += Fd[k] * Fd[k]; }
  rep.force_rel_error = den > 0 ? std::sqrt(num) / std::sqrt(den) : 0.0;
  pcout("Relative RMS error of the forces against the direct Coulomb sum :  " + fmt("%.10e", rep.force_rel_error));
}

template <int dim>
void LaplaceProblem<dim>::postprocess_error_in_energy_norm() {
  // :1423-1461 -- || grad phi_h - grad phi_exact ||_L2 with QGauss(degree+1) per cell and the
  // analytical gradient of include/step_50.h:355-369 (GaussianCharges only; the reference
  // dereferences a null exact_solution for Step16).
  if (par.Problemtype != "GaussianCharges") return;
  if (par.analytical_on_device && dim == 3) {  // the same norm through gmg_exact.hpp: the device, or its host mirror
    double e = 0.0;
    if (energy_norm_error(exact_on_device(), &e, nullptr) != GMG_OK) throw std::runtime_error(last_error);
    reports.back().energy_norm_error = e;
    pcout("Error in FE solution in energy norm:  " + fmt("%.10e", e));
    return;
  }
  constexpr int nv = 1 << dim;
  const Quadrature<dim> quad((int)par.degree + 1);
  const double inv_constant = 1.0 / (std::sqrt(M_PI) * par.r_c);
  double Error = 0.0;
#pragma omp parallel for reduction(+ : Error) schedule(dynamic, 512)
  for (int64_t ci = 0; ci < (int64_t)active_cells.size(); ++ci) {
    const ActiveCell &ac = active_cells[(size_t)ci];
    const Cell &cell = triangulation.levels[(size_t)ac.level][(size_t)ac.index];
    const double h = triangulation.cell_size(ac.level);
    double x0[3];
    triangulation.cell_origin(ac.level, cell, x0);
    int32_t dofs[nv];
    cell_dofs(ac, dofs);
    for (size_t q = 0; q < quad.p.size(); ++q) {
      double xq[3] = {0, 0, 0}, gh[3] = {0, 0, 0}, ga[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d) xq[d] = x0[d] + h * quad.p[q][(size_t)d];
      for (int a = 0; a < nv; ++a)
        for (int d = 0; d < dim; ++d) gh[d] += solution[(size_t)dofs[a]] * quad.grad[q][(size_t)a][(size_t)d] / h;
      for (unsigned i = 0; i < number_of_atoms; ++i) {
        double r2 = 0, dir[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) { dir[d] = xq[d] - atom_positions[3 * i + (size_t)d]; r2 += dir[d] * dir[d]; }
        const double r = std::sqrt(r2);
        const double f = charges[i] * (((2.0 * r * std::exp(-std::pow(r / par.r_c, 2)) * inv_constant) - std::erf(r / par.r_c)) / std::pow(r, 2));
        for (int d = 0; d < dim; ++d) ga[d] += f * dir[d] / r;
      }
      double n2 = 0;
      for (int d = 0; d < dim; ++d) n2 += (gh[d] - ga[d]) * (gh[d] - ga[d]);
      Error += n2 * quad.w[q] * std::pow(h, dim);
    }
  }
  reports.back().energy_norm_error = std::sqrt(Error);
  pcout("Error in FE solution in energy norm:  " + fmt("%.10e", std::sqrt(Error)));
}

// ======================================================================== adaptive loop

template <int dim>
int LaplaceProblem<dim>::run_cycle(unsigned int cycle, bool on_device) {
  pcout("Cycle " + std::to_string(cycle) + ":");
  // STEP50_TIMING=1: wall time of the host phases on stderr (the reference's TimerOutput sections, :1463-1560)
  static const bool timing = std::getenv("STEP50_TIMING") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!timing) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[step50] cycle %u %-22s %8.3f s\n", cycle, what, std::chrono::duration<double>(now - t_last).count());
    t_last = now;
  };
  densities_on_device = on_device && par.densities_on_device;
  solve_on_device_requested = on_device;
  if (cycle == 0) make_initial_grid();
  else refine_grid(cycle);
  lap("mesh");
  reports.emplace_back();
  CycleReport &rep = reports.back();
  rep.cycle = (int)cycle;
  rep.active_cells = triangulation.n_active_cells();
  pcout("   Number of active cells:       " + std::to_string(rep.active_cells));
  if (cycle == 0) {
    setup_system(cycle);
    initial_guess.assign(vertex_of_dof.size(), 0.0);
  }
  rep.dofs = (int64_t)vertex_of_dof.size();
  std::string s = "   Number of degrees of freedom: " + std::to_string(rep.dofs) + " (by level: ";
  for (int l = 0; l < triangulation.n_levels(); ++l) {
    rep.dofs_by_level.push_back((int64_t)level_vertex_of_dof[(size_t)l].size());
    s += std::to_string(rep.dofs_by_level.back()) + (l == triangulation.n_levels() - 1 ? ")" : ", ");
  }
  pcout(s);
  lap("setup_system");
  assemble_system();
  lap("assemble_system");
  if (par.PreconditionerType == "GMG") assemble_multigrid();
  lap("assemble_multigrid");
  build_transfer();
  lap("build_transfer");
  if (!on_device) return GMG_OK;
  int rc = upload();
  lap("upload");
  if (rc != GMG_OK) return rc;
  rc = solve();
  lap("solve");
  if (rc != GMG_OK) return rc;
  finish_cycle();
  lap("estimate + mark");
  return GMG_OK;
}

// The check vector of the reference's rhs test (tests_rhs_rc_variation/rc_variation.cc:110-215,
// charge_density_test): every DoF of a cell receives sum_q rho(x_q) JxW_q of that cell (no shape
// function weights), constrained DoFs receive nothing (homogeneous lines: distribute_local_to_global
// drops them).  Uses the densities of the last assembled right-hand side.
template <int dim>
std::vector<double> LaplaceProblem<dim>::total_charge_density_vector() const {
  constexpr int nv = 1 << dim;
  std::vector<double> t(vertex_of_dof.size(), 0.0);
  const_cast<LaplaceProblem<dim> *>(this)->ensure_host_densities();
  if (!lammpsinput || density_values_for_each_cell.size() != active_cells.size()) return t;
  const Quadrature<dim> q_rhs((int)(par.degree + par.quadrature_degree_rhs));
  for (size_t ci = 0; ci < active_cells.size(); ++ci) {
    const ActiveCell &ac = active_cells[ci];
    const double jxw = std::pow(triangulation.cell_size(ac.level), dim);
    double cell_sum = 0.0;
    for (size_t q = 0; q < q_rhs.p.size(); ++q) cell_sum += density_values_for_each_cell[ci][q] * (q_rhs.w[q] * jxw);
    int32_t dofs[nv];
    cell_dofs(ac, dofs);
    for (int a = 0; a < nv; ++a) {
      const int32_t cl = constraint_of_dof[(size_t)dofs[a]];
      if (cl < 0) t[(size_t)dofs[a]] += cell_sum;
      else
        for (auto &e : constraint_lines[(size_t)cl].entries) t[(size_t)e.first] += e.second * cell_sum;
    }
  }
  return t;
}

template <int dim>
void LaplaceProblem<dim>::finish_cycle() {
  estimate_error_and_mark_cells();                                               // :1552
  if (par.output_results) output_results((unsigned)reports.back().cycle);       // :1553
  energy_forces_resident = decide_energy_forces_resident();
  if (lammpsinput && (number_of_atoms < 300 || (par.energy_for_large_systems && par.short_range_cutoff > 0.0))) {
    postprocess_electrostatic_energy();     // :1554-1555
    if (number_of_atoms < 300) postprocess_error_in_energy_norm();  // :1556 (O(cells x atoms): under the reference's small-system gate only)
  }
  // "Error norm for large systems": past that gate only through gmg_exact.hpp (the legacy host loop stays gated)
  if (lammpsinput && number_of_atoms >= 300 && par.error_norm_for_large_systems && par.analytical_on_device && dim == 3)
    postprocess_error_in_energy_norm();
  if (lammpsinput && dim == 3 && par.compute_forces) postprocess_forces();  // (3D atoms exist only with LAMMPS input)
}

// Test hook: a solution computed elsewhere (the CPU oracle in tests/) takes the place of solve();
// x is the pre-distribute vector as the solver returns it.
template <int dim>
void LaplaceProblem<dim>::set_solution(const std::vector<double> &x) {
  solution = x;
  solution_on_device = false;
  distribute_constraints(solution);
}

template <int dim>
void LaplaceProblem<dim>::run() {
  pcout("Running with the MI355X C-ABI backend on " + std::to_string(n_ranks) + " rank(s)...");  // :1466-1474
  pcout("Dimension:\t" + std::to_string(dim));
  if (!lammpsinput && number_of_atoms == 0) read_lammps_input_file(par.LammpsInputFile);
  for (unsigned int cycle = 0; cycle < par.number_of_adaptive_refinement_cycles; ++cycle) {
    const int rc = run_cycle(cycle, true);
    if (rc != GMG_OK) throw std::runtime_error("cycle " + std::to_string(cycle) + " failed: " + last_error);
  }
}

}  // namespace step50

#include "adaptive.inc"
#include "output.inc"

namespace step50 {
template class LaplaceProblem<2>;
template class LaplaceProblem<3>;
}  // namespace step50
