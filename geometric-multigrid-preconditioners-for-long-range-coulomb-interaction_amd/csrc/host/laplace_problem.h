// laplace_problem.h -- host-side C++ mirror of the reference's Step50::LaplaceProblem<dim>
// (/root/reference/include/step_50.h:111-202) for the GMG-CG hot path on MI355X.
//
// Same member names and meaning as the reference class; what the reference delegates to
// deal.II / Trilinos / p4est is done here by forest.h (mesh), plain CSR containers (matrices)
// and -- for everything on the hot path -- by the C-ABI of include/gmg_coulomb.h.  The outer
// CG loop of solve() stays in this C++ (SolverCG below) and calls through that ABI.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>

#include "flat_map.h"
#include <vector>

#include "forest.h"
#include "gmg_coulomb.h"

namespace step50 {

struct CSRMatrix {
  int64_t n_rows = 0, n_cols = 0;
  std::vector<int64_t> rowptr;
  std::vector<int32_t> col;
  std::vector<double> val;
  int64_t nnz() const { return rowptr.empty() ? 0 : rowptr.back(); }
  void add(int32_t r, int32_t c, double v);  // entry must be in the pattern
  double l1_norm() const, linfty_norm() const, frobenius_norm() const;  // src/step-50.cc:950-952
};

// flat view of a deal.II .prm file (ParameterHandler keys of src/step-50.cc:13-95)
class ParameterReader {
 public:
  void declare_parameters();                      // defaults, src/step-50.cc:13-95
  void read_parameters(const std::string &file);  // src/step-50.cc:98-101
  void parse_input_from_string(const std::string &text);
  std::string get(const std::string &key) const;
  double get_double(const std::string &key) const;
  long get_integer(const std::string &key) const;
  bool get_bool(const std::string &key) const;
  void set(const std::string &key, const std::string &value) { values[key] = value; }

 private:
  std::map<std::string, std::string> values;
};

// the reference's 20 constructor arguments (include/step_50.h:115-118) + this build's additions
struct Parameters {
  unsigned int degree = 1;
  std::string Problemtype = "Step16", PreconditionerType = "GMG", LammpsInputFile = "atom_8.data",
              Boundary_conditions = "Inhomogeneous";
  double domain_size_left = -1, domain_size_right = 1, mesh_size_h = 0.25;
  unsigned int repetitions_for_vacuum = 1, number_of_global_refinement = 2, number_of_adaptive_refinement_cycles = 2;
  double r_c = 0.5, nonzero_density_radius_parameter = 3;
  bool flag_rhs_assembly = false, flag_analytical_solution = false, flag_rhs_field = false, flag_atoms_support = false,
       flag_output_time = true;
  unsigned int quadrature_degree_rhs = 1;
  int dim = 2;
  // additions (the smoother is a source edit in the reference, src/step-50.cc:969-970)
  std::string smoother = "SSOR";  // Jacobi | SSOR | Chebyshev
  double smoother_omega = 0.5;
  int smoother_steps = 2, chebyshev_degree = 2;
  std::string chebyshev_polynomial = "first kind";  // first kind | fourth kind
  std::string chebyshev_estimate = "Gershgorin";    // Gershgorin | Lanczos
  int chebyshev_lanczos_steps = 10;
  double chebyshev_safety = 1.2;
  bool densities_on_device = true;  // compute_charge_densities() through gmg_charge_density when a device is in use
  int ssor_blocks = 1;  // 1: exact sequential SGS (mpirun=1); B: rank-local SGS on B blocks (mpirun=B)
  std::string ssor_partition = "equal rows";  // where the B blocks are cut: "equal rows" | "balanced" (modelled sweep time)
  bool device_resident_outer_cg = false;  // true: gmg_cg_solve instead of the host SolverCG
  std::string partition_level0 = "auto";  // one process per GPU: auto | always | never
  std::string refinement_estimator = "Kelly + residual";  // HEAD (:1040-1089) | "Kelly": the indicator of the older cluster runs
  double short_range_cutoff = 0.0;        // in smoothing lengths; 0: all pairs (the reference)
  bool energy_for_large_systems = false;
  bool compute_forces = false;        // forces on the atoms after the energy (LAMMPS input, 3D), DESIGN.md section 9
  bool direct_coulomb_check = false;  // with them the exact all-pairs Coulomb forces and the relative RMS error against them  // evaluate the energy also for >= 300 atoms (needs the cutoff; the reference skips it, :1554)
  // the Exact boundary values in one batch and the error norm through gmg_exact.hpp (device or host
  // mirror); with it the error norm may also be evaluated beyond the reference's 300-atom gate
  bool analytical_on_device = false, error_norm_for_large_systems = false;
  bool rhs_on_device = true;            // gmg_rhs_assemble: F integrated on the device from densities that stay there
  bool transfer_on_device = true;       // gmg_build_transfer instead of building P_l here and uploading it
  bool level0_matrix_on_device = true;  // gmg_set_level_matrix_lattice instead of assembling + uploading level 0 (3D, constant coefficient, lexicographic, unpartitioned)
  bool system_matrix_on_device = false;  // gmg_assemble_system_matrix instead of assembling + uploading the active-mesh matrix (one rank; Step16: the _coef entry)
  bool ssor_plan_on_device = false;  // option ssor_plan_device of the context: the SSOR plans of the levels >= 1 formed by kernels where that applies
  bool level_matrices_on_device = false;  // gmg_assemble_level_matrix instead of assembling + uploading A_l and I_l (one rank; Step16: the _coef entry)
  bool rhs_from_cell_tables = false;     // gmg_assemble_rhs instead of the sequential cell loop (and its gather plan), and constraints.distribute on the device (one rank)
  bool mesh_tables_on_device = false;    // gmg_build_mesh_tables instead of the sequential loops of distribute_dofs and make_constraints (cycle on the device, one rank)
  bool operators_from_resident_tables = false;  // gmg_close_constraints and the _resident entries: operators, right-hand side and distribution read the tables gmg_build_mesh_tables left on the device
  bool densities_from_resident_tables = false;  // gmg_charge_density_resident: the densities read the cells' geometry from the tables gmg_build_mesh_tables left on the device
  bool estimator_from_resident_tables = false;  // gmg_build_face_table_resident, gmg_estimate_error_resident, gmg_refine_forest_marked and gmg_energy_norm_error_resident: the end of the cycle reads the tables, the face table and the marks where they lie
  bool energy_forces_from_resident_tables = false;  // gmg_build_point_locator_resident, gmg_electrostatic_energy_resident and gmg_atom_forces_resident: the energy's sums and the forces read the tables and the solution where they lie
  bool refinement_on_device = false;     // gmg_refine_forest, gmg_transfer_solution and gmg_build_face_table instead of refine_flagged, the interpolation loop of refine_grid and face_table (cycle on the device, one rank)
  bool estimator_on_device = false;      // gmg_estimate_error instead of the host loops of estimate_error_and_mark_cells (cycle on the device, one rank)
  std::string level0_numbering = "lexicographic";  // lexicographic | cell-wise (deal.II's first-touch order): level 0 carries no smoother
  std::string coarse_solver = "CG";  // CG (the reference, :962-967) | direct (gmg_set_coarse_solver: fast diagonalisation on a lattice level 0)
  // graphical output (the reference's output_results, :1149-1308).  The three flags above that the
  // reference reads there -- flag_analytical_solution, flag_rhs_field, flag_atoms_support -- select the optional arrays.
  bool output_results = false;         // "Output results": write solution-CCCCC.0000.vtu, .pvtu and .visit after every cycle's estimate
  std::string output_directory = ".";  // "Output directory"
  static Parameters from(const ParameterReader &prm);
};

struct CycleReport {  // the values the reference prints per cycle (src/step-50.cc:946-952, 1009-1014, ...)
  int cycle = 0;
  int64_t active_cells = 0, dofs = 0;
  std::vector<int64_t> dofs_by_level;
  double rhs_l1 = 0, rhs_l2 = 0, rhs_linf = 0, matrix_l1 = 0, matrix_linf = 0, matrix_frobenius = 0;
  double starting_value = 0, convergence_value = 0, sol_l1 = 0, sol_l2 = 0, sol_linf = 0;
  int cg_iterations = 0;
  int64_t coarse_iterations = 0;
  double refine_threshold = 0;
  bool has_energy = false;
  double energy_analytical = 0, energy_short = 0, energy_fe_long = 0, energy_self = 0, energy_total = 0, energy_abs_error = 0;
  double energy_norm_error = 0;
  double solve_seconds = 0;  // first residual to convergence, excluding upload / build_matrices
  double build_matrices_ms = 0;  // device time of mg_transfer.build_matrices (:957-958) when the device builds the transfers
  int status = 0;
  int coarse_solver = 0;  // GMG_COARSE_CG / GMG_COARSE_DIRECT: what the cycle's last coarse solve ran (gmg_stats.coarse_solver)
  bool has_forces = false;  // "Compute forces": sum_i F_i, max_i |F_i|, ||F - F^d|| / ||F^d|| ("Direct Coulomb check", else 0)
  double force_net[3] = {0, 0, 0}, force_max = 0, force_rel_error = 0;
};

// "Mesh tables on device" (DESIGN.md section 20): what gmg_build_mesh_tables takes, from the forest alone
struct ForestCells {
  int32_t n0[3] = {0, 0, 0};
  std::vector<int64_t> level_ptr;
  std::vector<int32_t> cell_coord, cell_first_child;  // [n][3], [n]: every cell of every level in index order
  int level0_lexicographic = 0;
};

template <int dim>
class LaplaceProblem {
 public:
  explicit LaplaceProblem(const Parameters &p);
  ~LaplaceProblem();
  void run();  // src/step-50.cc:1463-1573

  // ---- protected in the reference (tests subclass it); public here for the C binding
  void read_lammps_input_file(const std::string &filename);              // :181-258
  void set_atoms(const std::vector<double> &q, const std::vector<double> &xyz);  // synthetic input of the same shape
  void make_initial_grid();                                              // :1490-1528
  void setup_system(unsigned int cycle);                                 // :646-732
  void rhs_assembly_optimization();                                      // :260-306
  void compute_charge_densities();                                       // :509-575
  void ensure_host_densities();                                          // copy device-resident densities out when the host needs them
  void compute_moments();                                                // :577-644
  void assemble_system();                                                // :735-833
  void assemble_system_matrix_host(bool laps = true);                               // the matrix part of assemble_system: coupling lists, pattern, values
  void ensure_system_matrix();                                           // assemble a system matrix that was left to the device, on demand
  bool decide_system_on_device();                                        // system matrix formed on the device (gmg_assemble_system_matrix)?
  // what gmg_assemble_system_matrix takes, from the current mesh and constraints
  struct SystemAssemblyInputs {
    std::vector<int32_t> cell_dofs, line_master;
    std::vector<uint8_t> cell_level;
    std::vector<double> K_of_level, line_weight, line_inhomogeneity;
    std::vector<int64_t> line_ptr;
  };
  SystemAssemblyInputs system_assembly_inputs(bool mesh_arrays = true) const;  // (false: K_of_level alone, what the resident entries take)
  void line_tables(std::vector<int64_t> &line_ptr, std::vector<int32_t> &line_master, std::vector<double> &line_weight,
                   std::vector<double> &line_inhomogeneity) const;  // the constraint lines in CSR form
  SystemAssemblyInputs cycle_line_tables;  // "RHS from cell tables": the line tables of this cycle, kept for gmg_distribute_constraints
  // what gmg_assemble_rhs takes beyond them: the tables of the right-hand side's quadrature and the
  // integrand at the quadrature points of every active cell -- the charge densities as the host holds them, or
  // rhs_function(x0 + h p_q) (filled one cell per iteration: the values do not depend on the number of threads)
  struct RhsAssemblyInputs {
    int nq = 0;
    std::vector<double> shape, weight, jxw_of_level;  // [nq][nv], [nq], [16]
    std::vector<double> source;                       // [n_cells][nq]
  };
  RhsAssemblyInputs rhs_assembly_inputs(bool with_source = true);
  bool decide_rhs_from_cell_tables();                                    // right-hand side formed by gmg_assemble_rhs?
  void assemble_rhs_from_cell_tables();                                  // system_rhs through gmg_assemble_rhs
  int distribute_constraints_on_device(double *d_u);                     // gmg_distribute_constraints with this cycle's lines
  // the distributed solution as the device holds it after a solve with "RHS from cell tables" (nullptr: upload `solution`)
  const double *device_solution() const { return solution_on_device ? d_full : nullptr; }
  void assemble_multigrid();                                             // :835-933
  void assemble_level(int l);                                            // one level's matrix + interface matrix (:869-931)
  void ensure_level_matrix(int l);                                       // assemble a level that was left to the device, on demand
  bool decide_levels_on_device();                                        // level + interface matrices formed on the device (gmg_assemble_level_matrix)?
  // what gmg_assemble_level_matrix takes for one level: the cell table is level_cell_dof_table[l]
  struct LevelAssemblyInputs {
    std::vector<double> K;           // [nv][nv]: the cell matrix as assemble_level scales it
    std::vector<uint8_t> dof_flags;  // bit 0 level_boundary, bit 1 level_refinement_edge
  };
  LevelAssemblyInputs level_assembly_inputs(int l, bool flags = true) const;  // (false: K alone, what the resident entry takes)
  // what gmg_assemble_system_matrix_coef / gmg_assemble_level_matrix_coef take beyond the cell tables
  struct CoefficientInputs {
    int nq = 0;
    std::vector<double> cell_coef;  // [n_cells][nq]: coefficient(x0 + h p_q), q ascending
    std::vector<double> G, qw;      // [nq][nv][nv], [nq]
    std::vector<double> scale;      // [16] by level (system) or [1] (one level): pow(h, dim - 2)
  };
  CoefficientInputs coefficient_tables() const;
  CoefficientInputs system_coefficient_inputs() const;
  CoefficientInputs level_coefficient_inputs(int l) const;
  bool decide_level0_on_device() const;                                  // level 0 formed on the device (gmg_set_level_matrix_lattice)?
  void level0_cell_matrix(double *Ke) const;
  void build_transfer();                                                 // mg_transfer.build_matrices, :957-958
  void build_prolongation(int l);                                        // P_l on the host (the device builds it otherwise)
  void ensure_prolongation(int l);
  int ensure_context();                                                  // gmg_create (+ communicator) on first use
  int report_ssor_plan_origin(int level);                                // "SSOR plan on device": the fallback line, the check against a host plan
  int upload();                                                          // hand the operators over the C-ABI
  int solve();                                                           // :938-1017
  void estimate_error_and_mark_cells();                                  // :1020-1090
  void estimate_error_host();                                            // its host loops
  int estimate_error_device();                                           // the same through gmg_estimate_error
  bool decide_estimator_on_device();                                     // "Error estimator on device" set and applicable to this cycle?
  // what gmg_estimate_error takes, from the current forest, the parameters and the densities
  struct EstimatorInputs {
    std::vector<int32_t> cell_dofs, face_cell;
    std::vector<uint8_t> cell_level, face_kind;
    std::vector<double> h_of_level, face_measure_of_level, diameter_of_level, jxw_of_level, gauss_x, gauss_w, weight, dens;
    int residual = 0, nq = 0;    // residual: 0 Kelly term only, 1 HEAD's rule, 2 the residual term beside the Kelly rule
    bool dens_resident = false;  // dens stays NULL: the densities gmg_charge_density left on the device
    double fraction = 0.6;       // :1084
  };
  EstimatorInputs estimator_inputs(bool mesh_arrays = true);  // (false: no cell_dofs, cell_level or face table, what the resident entry takes)
  // "Estimator from resident tables" (DESIGN.md section 24): face table, estimate, marks and error norm on the context's tables
  bool decide_estimator_resident();       // says so once when the key asks for it in vain
  bool estimator_resident_applies() const {
    return par.estimator_from_resident_tables && operators_resident && par.estimator_on_device && par.refinement_on_device && !distributed;
  }
  void face_table_resident();             // gmg_build_face_table_resident for the current forest
  bool estimator_resident = false;        // the last estimate went through gmg_estimate_error_resident
  bool marks_resident = false;            // the context holds the marks of refine_flags (until the next estimate or mesh)
  bool estimator_resident_fallback_reported = false;
  void face_table(std::vector<uint8_t> &face_kind, std::vector<int32_t> &face_cell) const;  // the forest's faces by kind
  // Graphical output (csrc/host/output.inc).  output_results: the three files of one cycle in
  // par.output_directory (rank 0 alone writes, one piece); write_output_files: the same into a given directory.
  void output_results(unsigned int cycle);                               // :1149-1308
  void write_output_files(unsigned int cycle, const std::string &directory);
  // One patch per active cell, 2^dim vertices each: point [slots][3], solution [slots], grad_phi [slots][3] and the gathered
  // DoF vectors patch_field[j] [slots] (any output may be null).  path: kPatchesMirror the host mirror of gmg_output.hpp,
  // kPatchesHostArrays gmg_output_patches, kPatchesResident gmg_output_patches_resident.
  enum PatchPath { kPatchesMirror = 0, kPatchesHostArrays = 1, kPatchesResident = 2 };
  int output_patches(PatchPath path, int n_fields, const double *const *dof_field, double *point, double *patch_solution, double *grad_phi,
                     double *const *patch_field, double *build_ms = nullptr);
  PatchPath patches_on_device() const {  // where an explicit "on the device" forms them
    return operators_resident && device_solution() != nullptr && !distributed ? kPatchesResident : kPatchesHostArrays;
  }
  PatchPath decide_output_patches();     // where this cycle's patches are formed; says so once per fallback
  bool output_host_arrays_reported = false, output_mirror_reported = false;
  PatchPath output_path = kPatchesMirror;  // where the last output_results formed its patches
  void refine_grid(unsigned int cycle);                                  // :1095-1121
  // "Refinement on device" 
  bool refinement_applies() const { return par.refinement_on_device && solve_on_device_requested && !distributed; }
  bool decide_refinement_on_device();                                    // set and applicable to this cycle?  Says so once when not
  void refine_grid_on_device(unsigned int cycle);                        // refine_grid through gmg_refine_forest and gmg_transfer_solution
  void face_table_on_device(std::vector<uint8_t> &face_kind, std::vector<int32_t> &face_cell);  // face_table through gmg_build_face_table
  bool refined_on_device = false;              // the last refine_grid went through the device entries
  bool refinement_fallback_reported = false;   // "Refinement on device" was set but not applicable: said once
  std::vector<uint8_t> closed_refine_flags;    // the marks of the last refine_grid after the 2:1 closure, all levels of the old forest (tests)
  void postprocess_electrostatic_energy();                               // :1310-1420
  void postprocess_error_in_energy_norm();                               // :1423-1461
  void postprocess_forces();                                             // forces on the atoms (no counterpart in the reference)
  // Per-atom phi_h, E_h, F = q E_h + F^s, F^s, e_short (any output may be null) of the current solution, cutoff in units of
  // r_c (0: all pairs); on the device through gmg_atom_forces, or by the host mirror of the same definitions (gmg_forces.hpp).
  int atom_forces(bool on_device, double cutoff, std::vector<double> *phi, std::vector<double> *field, std::vector<double> *force,
                  std::vector<double> *force_short, std::vector<double> *e_short);
  int direct_coulomb(bool on_device, std::vector<double> *force, std::vector<double> *energy);  // exact all-pairs sum
  bool forces_on_device() const { return solve_on_device_requested && gmg != nullptr; }  // where the cycle's solve ran
  void point_locator(std::vector<int32_t> &node) const;  // the forest flattened for gmg_set_point_locator
  // "Energy and forces from resident tables" (DESIGN.md section 25): the locator is formed on the device next to the tables,
  // the energy's three sums and the forces read cell_dofs and the solution there
  bool decide_energy_forces_resident();   // says so once when the key asks for it in vain
  bool energy_forces_resident_applies() const {
    return par.energy_forces_from_resident_tables && operators_resident && device_solution() != nullptr && dim == 3 && lammpsinput && !distributed;
  }
  void ensure_point_locator_resident();   // gmg_build_point_locator_resident for the current forest, once per mesh
  bool energy_forces_resident = false;    // the last finish_cycle took energy and forces from the resident entries
  bool energy_forces_fallback_reported = false;
  // The exact free-space potential of all atoms (Analytical_Solution, include/step_50.h:338-369) and / or its gradient at
  // n_points points [3 n] (3D): through gmg_gaussian_potential, or by the host mirror of the same text (gmg_exact.hpp).
  int gaussian_potential(bool on_device, int64_t n_points, const double *points, double *phi, double *grad);
  // || grad phi_h - grad phi ||_L2 of the current solution and the per-cell squares [active cells] (either may be null):
  // through gmg_energy_norm_error, or by the host mirror
  int energy_norm_error(bool on_device, double *error, std::vector<double> *cell_err2);
  // where "Analytical solution on device" evaluates: on the device when the cycle runs there, 3D Gaussian charges from atoms
  bool exact_on_device() const { return solve_on_device_requested && dim == 3 && par.Problemtype == "GaussianCharges" && lammpsinput; }
  std::vector<double> total_charge_density_vector() const;               // tests_rhs_rc_variation/rc_variation.cc:110-215
  int run_cycle(unsigned int cycle, bool on_device = true);              // one iteration of the loop in run()
  void finish_cycle();                                   // estimator + energy, the tail of the loop body
  void set_solution(const std::vector<double> &x);       // test hook, see laplace_problem.cc
  int solve_again();  // repeat the solve of the current cycle from the same initial guess (bench step)
  int set_smoother(const std::string &smoother, int ssor_blocks);  // other smoother on the current cycle's operators (re-uploads them)

  // ---- data, named as in the reference where it exists (include/step_50.h:146-200)
  Parameters par;
  Forest<dim> triangulation;
  std::vector<double> charges, atom_positions;  // positions: 3 * n
  unsigned int number_of_atoms = 0;
  bool lammpsinput = false;
  CSRMatrix system_matrix;
  std::vector<double> solution, system_rhs, initial_guess;
  std::vector<CSRMatrix> mg_matrices, mg_interface_matrices, mg_prolongation;  // P_l: level l -> l+1
  std::vector<std::vector<int32_t>> copy_global, copy_level;
  double dipole_moment[3] = {0, 0, 0};
  std::vector<CycleReport> reports;
  std::string log;  // everything pcout would have printed
  bool echo = false;
  gmg_context *gmg = nullptr;
  bool operators_uploaded = false, densities_on_device = false;
  bool solve_on_device_requested = false, level0_on_device = false, transfer_on_device = false;
  bool system_on_device = false;           // this cycle's system matrix is formed by gmg_assemble_system_matrix at upload()
  bool levels_on_device = false;           // this cycle's level and interface matrices are formed by gmg_assemble_level_matrix at upload()
  std::set<std::string> ssor_plan_reasons_reported;  // "SSOR plan on device": the causes of host-built plans said so far (once per run and cause)
  bool levels_fallback_reported = false;   // "Level matrices on device" was set but not applicable: said once
  bool system_fallback_reported = false;   // "System matrix on device" was set but not applicable: said once
  bool rhs_from_cells = false;             // this cycle's right-hand side was formed by gmg_assemble_rhs
  bool rhs_cells_fallback_reported = false;  // "RHS from cell tables" was set but not applicable: said once
  bool solution_on_device = false;         // d_full holds `solution` as constraints.distribute left it (gmg_distribute_constraints)
  bool coarse_fallback_reported = false;   // "Coarse solver = direct" was set but not applicable: said once
  bool densities_device_resident = false;  // compute_charge_densities left them in HBM for gmg_rhs_assemble
  double build_matrices_ms = 0.0;  // device time of gmg_build_transfer for the current cycle's operators
  std::string last_error;
  // one process per GPU (the reference: one MPI rank per subdomain, src/main.cc:8); the host
  // setup is replicated, the operators are cut by partition.h at upload()
  int rank = 0, n_ranks = 1;
  bool distributed = false;
  bool level0_partitioned = false;  // decided per cycle in upload() ("Partition level 0")
  // rows a rank must get rid of for a partitioned level 0 to pay (24 ps per row and coarse iteration on one MI355X):
  // over RCCL an iteration gains three collectives + their launches (~60 us), over the peer transport three
  // one-workgroup kernels and three flag latencies (~17 us)
  static constexpr int64_t kPartitionMinRowsSaved = 2500000, kPartitionMinRowsSavedPeer = 700000;
  std::string comm_id;  // gmg_comm_unique_id of rank 0, broadcast by the launcher
  void set_communicator(int rank_, int n_ranks_, const std::string &id) { rank = rank_; n_ranks = n_ranks_; comm_id = id; distributed = true; }

  // DoF bookkeeping (Q1: DoFs = vertices)
  struct ActiveCell { int32_t level, index; };
  std::vector<ActiveCell> active_cells;
  std::vector<std::vector<int32_t>> active_index_of_cell;  // [level][cell] -> position in active_cells or -1
  VertexMap dof_of_vertex;
  std::vector<uint64_t> vertex_of_dof;
  std::vector<VertexMap> level_dof_of_vertex;
  std::vector<std::vector<uint64_t>> level_vertex_of_dof;
  std::vector<int32_t> active_cell_dof_table;                 // [active cell][vertex]: the DoFs of every active cell (cell_dofs)
  std::vector<std::vector<int32_t>> level_cell_dof_table;     // [level][cell][vertex] (level_cell_dofs)
  // constraints (hanging nodes + Dirichlet), resolved: masters are unconstrained DoFs
  struct ConstraintLine { std::vector<std::pair<int32_t, double>> entries; double inhomogeneity = 0; bool hanging = false; };
  std::vector<int32_t> constraint_of_dof;  // -1 = unconstrained
  std::vector<ConstraintLine> constraint_lines;
  std::vector<std::vector<char>> level_boundary, level_refinement_edge;  // MGConstrainedDoFs
  std::vector<std::vector<double>> density_values_for_each_cell;         // [active cell][q]
  std::vector<float> error_per_cell;
  std::vector<double> estimator_kelly_sq, estimator_residual_sq;  // per active cell: face-jump sum / h_K^2 int (4 pi rho)^2 (kept for the marking-rule study)
  std::vector<std::vector<char>> refine_flags;
  std::vector<double> face_integrals;      // [active cell][face]: the face integrals of the last estimate (tests)
  bool estimated_on_device = false;        // the last estimate came from gmg_estimate_error
  bool estimator_fallback_reported = false;  // "Error estimator on device" was set but not applicable: said once
  int64_t host_density_copies = 0;         // how often ensure_host_densities() fetched device-resident densities
  int64_t dof_map_builds = 0;              // how often ensure_dof_maps() built the vertex -> DoF hash tables

  ForestCells forest_cells() const;     // "Mesh tables on device": the input of gmg_build_mesh_tables
  bool decide_mesh_tables_on_device();  // this cycle's numbering, constraints and level flags formed by gmg_build_mesh_tables?
  void distribute_dofs_on_device();     // the one call, and the download of the DoF tables
  void ensure_dof_maps();               // the vertex -> DoF hash tables, built from vertex_of_dof on first use
  bool mesh_on_device = false;            // this cycle's tables came from gmg_build_mesh_tables
  // "Operators from resident tables" (DESIGN.md section 22): this cycle's device entries read the context's tables
  bool decide_operators_resident();       // says so once when the key asks for it in vain
  void close_constraints_on_device();     // gmg_close_constraints with the Dirichlet values of constraint_lines
  bool operators_resident = false;        // the context holds this cycle's tables and their closed lines
  bool resident_fallback_reported = false;
  // "Charge densities from resident tables" 
  bool decide_densities_resident();       // says so once when the key asks for it in vain
  bool densities_resident = false;        // this cycle's densities came from gmg_charge_density_resident
  bool densities_fallback_reported = false;
  double densities_resident_ms = 0.0;     // device time of that call
  bool mesh_fallback_reported = false;    // "Mesh tables on device" was set but not applicable: said once
  bool dof_maps_ready = false;            // dof_of_vertex / level_dof_of_vertex match vertex_of_dof / level_vertex_of_dof
  double mesh_tables_ms = 0.0;            // device time of gmg_build_mesh_tables for the current mesh
  struct DeviceMeshTables {               // what make_constraints() takes from the same result
    int64_t n_hanging = 0;
    std::vector<int32_t> constraint_of_dof, line_master, line_dof;
    std::vector<int64_t> line_ptr;
    std::vector<double> line_weight;
    std::vector<std::vector<uint8_t>> dof_flags;
  } device_mesh;

  void pcout(const std::string &s);
  void distribute_dofs();
  void make_constraints();
  void cell_dofs(const ActiveCell &c, int32_t *out) const;
  void level_cell_dofs(int level, int32_t cell, int32_t *out) const;
  double boundary_value(const double x[3]) const;
  double rhs_function(const double x[3]) const;
  double coefficient(const double x[3]) const;
  void atoms_of_root_cell(const int rc[3], std::vector<int32_t> &out) const;
  double fe_value_at(const std::vector<double> &u, const double x[3]) const;
  void distribute_constraints(std::vector<double> &u) const;  // constraints.distribute, :1016
  void set_zero_constraints(std::vector<double> &u) const;    // constraints.set_zero, :1119

 private:
  struct AtomBins;
  std::unique_ptr<AtomBins> bins;
  double *d_solution = nullptr, *d_rhs = nullptr, *d_full = nullptr;
  int64_t d_n = 0, d_nvec = 0, d_begin = 0;
  int solve_on_device(CycleReport &rep);
};

// deal.II SolverCG<vector_t> restated on top of the C-ABI: every vector is a device pointer,
// every operation one ABI call (reference: src/step-50.cc:943, 991-992; operation order as in
// oracle/gmg_oracle.c:cg_solve).
struct SolverControl {
  int max_steps;
  double tolerance;
  double initial_value = 0, last_value = 0;
  int last_step = 0;
};
int SolverCG_solve(gmg_context *ctx, SolverControl &control, int64_t n, int64_t n_vec, double *x, const double *b,
                   const std::string &preconditioner);

std::vector<double> nacl_lattice(int n_cells, std::vector<double> &charges);  // the reference's atom/*.data generator

}  // namespace step50
