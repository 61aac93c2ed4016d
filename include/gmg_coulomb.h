/* gmg_coulomb.h -- C-ABI of libgmgcoulomb.so: the MI355X (gfx950) implementation of the
 * GMG-preconditioned CG hot path of the Step50 Poisson/Coulomb solver.
 *
 * The reference (vinayak-gholap1993/Geometric-Multigrid-preconditioners-for-long-range-
 * Coulomb-interaction) has no FFI for this path: LaplaceProblem::solve()
 * (src/step-50.cc:938-1017) wires deal.II class templates together inline.  The seams are
 * deal.II's duck-typed concepts; every entry point below names the concept
 * member / call site it stands in for.  A maintainer binds them with the 20-line adapter
 * classes shown in INTEGRATION.md and passes those to SolverCG::solve at :991.
 *
 * Conventions
 *   - every function returns int: GMG_OK or a GMG_ERR_* code; no C++ exception crosses the ABI;
 *     gmg_last_error() gives the text of the last failure on that context.
 *   - matrices are handed over as host CSR arrays (int64 rowptr, int32 col, fp64 val) and
 *     copied; they are immutable until replaced (the reference rebuilds them once per
 *     adaptive cycle, src/step-50.cc:1545-1548).  Explicitly stored zeros are kept.
 *   - vectors are device pointers (fp64) obtained from gmg_vec_alloc(); the caller owns them.
 *   - one host thread per context, one HIP stream per context; calls on one context are
 *     serialised by the caller (the reference runs single-threaded ranks, src/main.cc:8).
 *   - functions that return a scalar to the host (dot, norms, solves) block until it is
 *     available; everything else is asynchronous on the context's stream.
 *   - distributed runs: one process per GPU, rows of every operator are the locally owned
 *     range, columns index [owned | ghost] entries; see gmg_set_halo_plan().
 */
#ifndef GMG_COULOMB_H
#define GMG_COULOMB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMG_OK 0
#define GMG_ERR_INVALID 1        /* bad argument / wrong call order                         */
#define GMG_ERR_OUTER_NOCONV 2   /* outer CG hit max_it: deal.II SolverControl::NoConvergence, :942 */
#define GMG_ERR_COARSE_NOCONV 3  /* coarse CG hit 1000 its: NoConvergence from :962-967     */
#define GMG_ERR_HIP 4            /* a HIP runtime call failed                               */
#define GMG_ERR_COMM 5           /* RCCL failure / communicator not initialised             */
#define GMG_ERR_UNSUPPORTED 6

/* `which` argument of gmg_spmv & co.: a level number >= 0, or the active-mesh matrix */
#define GMG_SYSTEM (-1)

/* smoother kinds: src/step-50.cc:969 (Jacobi, commented), :970 (SSOR); Chebyshev is this
 * build's addition for BASELINE config 3 (not in the reference, parity unpinned)        */
#define GMG_SMOOTHER_JACOBI 0
#define GMG_SMOOTHER_SSOR 1
#define GMG_SMOOTHER_CHEBYSHEV 2

/* preconditioner of gmg_cg_solve: prm "Preconditioner = GMG | Jacobi", src/step-50.cc:954, :996 */
#define GMG_PRECOND_GMG 0
#define GMG_PRECOND_JACOBI 1
#define GMG_PRECOND_IDENTITY 2

typedef struct gmg_context gmg_context;

/* ---- lifetime ----------------------------------------------------------------------- */
/* Replaces the construction of the object graph in solve(), src/step-50.cc:954-989.
 * n_levels = triangulation.n_global_levels() (:709).                                      */
int gmg_create(gmg_context **ctx, int device_id, int n_levels);
int gmg_destroy(gmg_context *ctx);
/* New adaptive cycle (src/step-50.cc:1484): drops every operator, keeps stream + communicator; no table derived from an
 * operator or a copy list survives it (the inverse indices of the fused copies included).   */
int gmg_reset(gmg_context *ctx, int n_levels);
const char *gmg_last_error(const gmg_context *ctx);
int gmg_synchronize(gmg_context *ctx);

/* ---- operators ---------------------------------------------------------------------- */
/* system_matrix (include/step_50.h:156; filled src/step-50.cc:793-795, 831).              */
int gmg_set_system_matrix(gmg_context *ctx, int64_t n_rows, int64_t n_cols, const int64_t *rowptr,
                          const int32_t *col, const double *val);
/* mg_matrices[level] (include/step_50.h:168; filled src/step-50.cc:869-889, 930).
 * A call refused with GMG_ERR_INVALID for its rowptr or col (found on the host, before any launch) leaves the level WITHOUT
 * an operator, not with the previous one: gmg_precondition then returns GMG_ERR_INVALID ("level matrix not set") until a
 * valid matrix is set for the level, after which the context is as if the refused call had not been made.              */
int gmg_set_level_matrix(gmg_context *ctx, int level, int64_t n_rows, int64_t n_cols, const int64_t *rowptr,
                         const int32_t *col, const double *val);
/* mg_matrices[0] of the undivided lattice (Triangulation::subdivided_hyper_rectangle, src/step-50.cc:1526; assembled
 * :869-889) FORMED ON THE DEVICE instead of handed over as CSR: nv[0..2] vertices per direction
 * (>= 5), level DoFs numbered lexicographically (x fastest), Ke = the 8 x 8 cell matrix every cell adds (row-major, vertex a
 * = bx + 2 by + 4 bz, as deal.II orders them), all faces Dirichlet (MGConstrainedDoFs boundary indices, :704-706: the row of
 * a boundary DoF keeps sum |Ke[a][a]| on the diagonal, its couplings become stored zeros).  Values are the same bits
 * gmg_set_level_matrix would receive (a vertex's cells added in cell order).  Level 0 only; not with a row-partitioned
 * level 0.  The operator then serves y = A x (gmg_spmv) and the coarse CG.                                                */
int gmg_set_level_matrix_lattice(gmg_context *ctx, int level, const int32_t nv[3], const double Ke[64]);
/* mg_interface_matrices[level] (include/step_50.h:169; src/step-50.cc:892-925, 931); used as
 * both edge_out and edge_in, mg.set_edge_matrices(down, up) at :986.  Zeros may be pruned. */
int gmg_set_edge_matrix(gmg_context *ctx, int level, int64_t n_rows, int64_t n_cols, const int64_t *rowptr,
                        const int32_t *col, const double *val);
/* MGTransferPrebuilt::build_matrices product (src/step-50.cc:957-958): P maps `level` to
 * `level+1`, n_fine x n_coarse; the library builds the transpose for restrict_and_add.     */
int gmg_set_prolongation(gmg_context *ctx, int level, int64_t n_fine, int64_t n_coarse, const int64_t *rowptr,
                         const int32_t *col, const double *val);
/* MGTransferPrebuilt copy_indices[level] (used by PreconditionMG::vmult, :988-989).        */
int gmg_set_copy_indices(gmg_context *ctx, int level, int64_t n, const int32_t *global_idx, const int32_t *level_idx);
/* mg_smoother.initialize(mg_matrices, AdditionalData(omega)); set_steps(steps), :971-973.
 * cheb_*: Chebyshev degree, eigenvalue ratio and lambda_max of D^-1 A (0 = Gershgorin).    */
int gmg_set_smoother(gmg_context *ctx, int kind, double omega, int steps, int cheb_degree, double cheb_ratio,
                     double cheb_lmax);
/* The Chebyshev smoother's polynomial and where its lambda_max of D^-1 A comes from (not in the
 * reference).  Both choices are independent and both defaults are what the library did before this call existed.
 *   polynomial   GMG_CHEB_FIRST_KIND: the first-kind polynomial on [lmax / cheb_ratio, lmax] (default);
 *                GMG_CHEB_FOURTH_KIND: the fourth-kind polynomial of Lottes (2022), which needs lmax only: from a zero start
 *                  d = (4 / (3 lmax)) D^-1 r, y = d;  d = ((2j-1)/(2j+3)) d + ((8j+4)/((2j+3) lmax)) D^-1 (r - A y), y += d,
 *                  j = 1 .. degree - 1; cheb_ratio is not read
 *   lmax_source  GMG_CHEB_LMAX_GERSHGORIN: max_i sum_j |a_ij| / |a_ii| (default);
 *                GMG_CHEB_LMAX_LANCZOS: min(safety x the largest Ritz value of lanczos_steps steps of Jacobi-preconditioned
 *                  CG on the level, Gershgorin), formed on the device at the level's first Chebyshev use after its matrix was
 *                  set and kept until the matrix, lanczos_steps or safety changes
 *   lanczos_steps  1 .. 64, 0 keeps the current value (default 10);  safety >= 1, 0 keeps the current value (default 1.2)
 * A cheb_lmax > 0 given to gmg_set_smoother wins over both sources.  Anything else: GMG_ERR_INVALID. */
#define GMG_CHEB_FIRST_KIND 0
#define GMG_CHEB_FOURTH_KIND 1
#define GMG_CHEB_LMAX_GERSHGORIN 0
#define GMG_CHEB_LMAX_LANCZOS 1
int gmg_set_chebyshev(gmg_context *ctx, int polynomial, int lmax_source, int lanczos_steps, double safety);
/* The Lanczos estimate of `level` now (level 0 included), whatever the smoother is; it changes nothing the smoother uses.
 * steps 1 .. 64.  *ritz: the largest Ritz value; *steps_run: the steps that count (fewer than `steps` after a breakdown:
 * a level with D^-1 A = I ends after one step with ritz = 1); alpha, beta: `steps` entries each (zeros beyond steps_run) or
 * NULL.  The same bits from call to call.  GMG_ERR_UNSUPPORTED for a row-partitioned operator, GMG_ERR_INVALID before
 * the level matrix is set or for bad arguments. */
int gmg_estimate_lmax(gmg_context *ctx, int level, int steps, double *ritz, double *alpha, double *beta, int *steps_run);
/* out: polynomial, lmax source, Lanczos steps asked, steps run, Gershgorin bound, Ritz value, safety, lambda in use on
 * `level`; zeros where a value is not known (yet). */
int gmg_get_chebyshev(gmg_context *ctx, int level, double out[8]);
/* SolverControl coarse_solver_control(1000, 1e-10, false, false), :962.                    */
int gmg_set_coarse(gmg_context *ctx, double abs_tol, int max_it);
/* Which solver stands behind mg_coarse (:965-967): GMG_COARSE_CG, the reference's unpreconditioned CG (default), or
 * GMG_COARSE_DIRECT, fast diagonalisation on the level-0 lattice (not in the reference):
 *   x_int = (S_x (x) S_y (x) S_z) D^-1 (S_x (x) S_y (x) S_z) b_int,   x_i = b_i / a_ii on a boundary row,
 * six batched products with the sine matrices of the axes and one scaling, no iterations and no reductions.  Call it after
 * level 0 has been set.  DIRECT is accepted only if level 0 was formed by gmg_set_level_matrix_lattice, is not partitioned
 * over ranks, has 5 .. 1024 vertices in every direction, and its Ke is separable (gmg_coarse_direct_separable); otherwise
 * GMG_ERR_UNSUPPORTED with the reason in gmg_last_error, and the CG stays selected.  gmg_reset and a new level-0 matrix
 * return the context to the CG.  The option coarse_direct (gmg_set_option / GMG_OPTIONS) selects DIRECT whenever a later
 * gmg_set_level_matrix_lattice forms a level 0 that qualifies and silently leaves the CG otherwise.  With DIRECT,
 * gmg_coarse_solve reports iterations = 0 and, only when `residual` is non-NULL, the true |b - A_0 x|_2 (one more product
 * and a host wait); gmg_stats.coarse_iterations does not move.  Results are deterministic and independent of the launch
 * shape (option coarse_direct_max_blocks); they are not the bits of the CG.                                             */
#define GMG_COARSE_CG 0
#define GMG_COARSE_DIRECT 1
int gmg_set_coarse_solver(gmg_context *ctx, int kind);
/* The tables of one axis with n_cells cells (4 .. 1023), m = n_cells - 1 interior vertices, without a context or a device:
 *   S[(j-1) m + (k-1)] = sqrt(2 / n) sin(pi j k / n),  lambda[k-1] = 2 - 2 cos(pi k / n),  mu[k-1] = (4 + 2 cos(pi k / n)) / 6
 * (j, k = 1 .. m; any output may be NULL).  The sine is taken of the integer (j k) mod 2n folded into [0, n / 2], so the
 * error of an entry is a few ulp whatever the size of j k.  These are the numbers the device uses.                      */
int gmg_coarse_direct_tables(int n_cells, double *S, double *lambda, double *mu);
/* Is Ke (8 x 8, row-major, local index bit 0 = x, bit 1 = y, bit 2 = z) the cell matrix of the constant-coefficient Q1
 * Laplacian, Ke = s (k (x) m (x) m + m (x) k (x) m + m (x) m (x) k) with k = [[1, -1], [-1, 1]], m = [[2, 1], [1, 2]] / 6 and
 * s = 3 Ke[0][0] > 0, every entry within 64 * 2^-53 * max |Ke|?  GMG_OK and *s (may be NULL), or GMG_ERR_UNSUPPORTED.
 * Host only.                                                                                                            */
int gmg_coarse_direct_separable(const double Ke[64], double *s);
/* dst <- S_axis src along one axis (0 = x, 1 = y, 2 = z) on the interior of a level-0 vector, one pass of the direct
 * solver (which must be selected); boundary rows of dst are left untouched; dst != src.  Asynchronous.                 */
int gmg_coarse_direct_transform(gmg_context *ctx, int axis, double *dst, const double *src);
/* One direct coarse solve dst <- A_0^-1 src with HIP events attached to each of its seven launches: pass_ms[0..6] = the
 * kernels' own begin-to-end times of x, y, z + scaling, z, y, x and the boundary rows (what a kernel trace reports; launch
 * gaps are not in them).  Blocks.  For tools/coarse_direct_probe.py; the direct solver must be selected.               */
int gmg_coarse_direct_profile(gmg_context *ctx, double *dst, const double *src, double pass_ms[7]);

/* ---- vector_t (LA::MPI::Vector, include/step_50.h:154) ----------------------------- */
int gmg_vec_alloc(gmg_context *ctx, int64_t n, double **dptr);
int gmg_vec_free(gmg_context *ctx, double *dptr);
int gmg_vec_upload(gmg_context *ctx, double *dst_dev, const double *src_host, int64_t n);
int gmg_vec_download(gmg_context *ctx, double *dst_host, const double *src_dev, int64_t n);
int gmg_vec_set_zero(gmg_context *ctx, double *x, int64_t n);                               /* v = 0        */
int gmg_vec_equ(gmg_context *ctx, double *y, double a, const double *x, int64_t n);         /* y.equ(a,x)   */
int gmg_vec_add(gmg_context *ctx, double *y, double a, const double *x, int64_t n);         /* y.add(a,x)   */
int gmg_vec_sadd(gmg_context *ctx, double *y, double s, double a, const double *x, int64_t n); /* y.sadd(s,a,x) */
int gmg_vec_dot(gmg_context *ctx, const double *x, const double *y, int64_t n, double *out); /* x*y (all-reduced) */
int gmg_vec_norms(gmg_context *ctx, const double *x, int64_t n, double *l1, double *l2, double *linf); /* :946-948, :1012-1014 */
int gmg_vec_all_zero(gmg_context *ctx, const double *x, int64_t n, int *out);               /* x.all_zero() */

/* ---- the concepts SolverCG / Multigrid consume ------------------------------------- */
/* matrix.vmult(dst, src): SolverCG matrix concept (:991 system_matrix, :965 coarse_matrix);
 * also mg::Matrix::vmult(level, ...) (:975).  Includes the ghost import.                  */
int gmg_spmv(gmg_context *ctx, int which, double *dst, const double *src);
/* PreconditionMG::vmult(dst, src): copy_to_mg, one V-cycle (Multigrid::cycle), copy_from_mg
 * (:980-989).  Fails with GMG_ERR_COARSE_NOCONV like the reference's exception.  dst is
 * zeroed first (entries outside every copy list come back exactly 0).  With steps = 0 no
 * level is smoothed: the cycle restricts the defects, solves level 0 and prolongates.     */
int gmg_precondition(gmg_context *ctx, double *dst, const double *src);
/* PreconditionJacobi(omega).vmult on the system matrix (:999-1004, omega = 0.6).           */
int gmg_precondition_jacobi(gmg_context *ctx, double omega, double *dst, const double *src);
/* MGCoarseGridIterativeSolver::operator()(0, dst, src) (:965-967): unpreconditioned CG from
 * zero on mg_matrices[0], device resident; returns iteration count and final residual.
 * After GMG_ERR_COARSE_NOCONV (max_it reached, or a NaN residual) dst holds the iterate after
 * `iterations` steps, as SolverCG leaves it in dst when SolverControl throws; the context
 * stays usable.                                                                            */
int gmg_coarse_solve(gmg_context *ctx, double *dst, const double *src, int *iterations, double *residual);
/* MGSmootherBase::apply (from_zero != 0) / ::smooth (from_zero == 0) on one level (:983-984):
 * `steps` steps of u <- u + S (rhs - A u), the first of apply from u = 0 (the caller's u is
 * not read).  With steps = 0 both leave u as the caller gave it; apply does not zero it.   */
int gmg_smoother_step(gmg_context *ctx, int level, double *u, const double *rhs, int from_zero);
/* MGTransferBase::prolongate(level+1, dst, src) / restrict_and_add(level+1, dst, src).     */
int gmg_prolongate(gmg_context *ctx, int level, double *dst_fine, const double *src_coarse);
int gmg_restrict_and_add(gmg_context *ctx, int level, double *dst_coarse, const double *src_fine);

/* ---- optional: the whole outer solve on the device side of the ABI ------------------ */
/* solver.solve(system_matrix, solution, system_rhs, preconditioner) (:991-992 / :1003-1004)
 * with tol = rel_tol * |b|_2 (:942).  The north-star layout keeps this loop in the host C++
 * (csrc/host/laplace_problem.cc) on top of the calls above; this entry runs the same
 * operation order inside the library to avoid the per-call launch latency.               */
int gmg_cg_solve(gmg_context *ctx, double *x, const double *b, double rel_tol, int max_it, int precond,
                 int *iterations, double *starting_value, double *convergence_value);

/* The two steps of one SolverCG iteration around the preconditioner (src/step-50.cc:991-992), for a caller that keeps the
 * loop itself (csrc/host/laplace_problem.cc) and for gmg_cg_solve.  g.h stays inside the context between the steps: on one
 * rank in device memory, where alpha = g.h / d.h and beta = g.h / (the previous g.h) are formed by the same IEEE divisions
 * the host did, so an iteration waits for the device once (|g|^2, which SolverControl checks) instead of three times.
 * Vectors, partial sums and their order are those of gmg_vec_dot / gmg_vec_add / gmg_vec_sadd: results are bit for bit
 * the same.  Several ranks, or option disable_outer_cg_fused: the steps run exactly those calls.
 *   direction step: first != 0: d = -h, g.h kept; first == 0: beta = g.h / (kept g.h), d.sadd(beta, -1, h), g.h kept.
 *                   Asynchronous on one rank.
 *   update step:    alpha = (kept g.h) / d.h, x.add(alpha, d), g.add(alpha, h), *gg = g.g.  Blocks.                        */
int gmg_cg_direction_step(gmg_context *ctx, double *d, const double *g, const double *h, int64_t n, int first);
int gmg_cg_update_step(gmg_context *ctx, double *x, double *g, const double *d, const double *h, int64_t n, double *gg);

/* ---- next row N1: Gaussian charge density at the quadrature points -------- */
/* compute_charge_densities() (src/step-50.cc:509-575) with the atom lists of
 * rhs_assembly_optimization() (:260-306) evaluated on the fly: for every cell, rho at its nq
 * quadrature points, summed over the atoms closer than `cutoff` to any vertex of the cell's
 * ROOT cell (use_lists != 0; children inherit the parent's list, :441-450) or over all atoms.
 * Host arrays in, host array out (dens[n_cells * nq], incl. the factor 4 pi of :522).
 *   rho(x) = 4 pi / (r_c^3 pi^1.5) * sum_k q_k exp(-|x - x_k|^2 / r_c^2)
 *   x      = cell_lo + cell_h * quadrature_points[q] per coordinate, as fp64 evaluates it (quadrature_points: [nq][3] on the
 *            unit cell); cell_lo, root_lo: [3 n_cells], cell_h: [n_cells]; a child's root_lo is its root cell's corner
 *   list   : atom k counts for a cell when its distance to the nearest of the 8 vertices root_lo + {0, root_h}^3 is below
 *            `cutoff` -- a distance, not a multiple of r_c; an atom at exactly `cutoff` does not count.  In fp64: per
 *            direction the nearer of root_lo and root_lo + root_h (the lower one on a tie), sqrt(mx^2 + my^2 + mz^2) < cutoff
 * The order in which a point's atoms are summed is not specified (a wavefront shares them).  A point with no atom on its
 * list, or n_atoms = 0, gives exactly +0.0.                                                                           */
/* dens == NULL keeps the densities on the device for gmg_rhs_assemble (gmg_get_charge_density copies them out on demand).   */
int gmg_charge_density(gmg_context *ctx, int64_t n_cells, const double *cell_lo, const double *cell_h,
                       const double *root_lo, double root_h, int64_t n_atoms, const double *atom_xyz,
                       const double *atom_q, double r_c, double cutoff, int use_lists, int nq,
                       const double *quadrature_points, double *dens);
/* the densities gmg_charge_density kept on the device (dens == NULL), copied out: [n_cells * nq]                        */
int gmg_get_charge_density(gmg_context *ctx, int64_t n_cells, int nq, double *dens);
/* The same densities for the active cells of the 3D tables the last gmg_build_mesh_tables left on the device: no per-cell
 * array crosses the bus.  With n_cells, cell_dofs, cell_level and vertex_of_dof of those tables, active cell a of level l has
 *   k = vertex_of_dof[cell_dofs[8 a]],   c[d] = ((k >> 21 d) & 0x1fffff) >> (12 - l),   h = h0 / 2^l,
 *   cell_lo[d] = origin + h * c[d],   root_lo[d] = origin + h0 * (c[d] >> l),
 * each a rounded product followed by a rounded sum (no fused multiply-add): what Forest::cell_origin and the driver's loop
 * give for origin and h0 of the root lattice.  The definition of gmg_charge_density then applies word for word to this
 * geometry with cell_h = h and root_h = h0: rho, the points cell_lo + h * quadrature_points[q], the list predicate on the
 * nearest root vertex with a strict <, use_lists = 0 meaning all atoms, exactly +0.0 for an empty list or n_atoms = 0.
 * One point is tighter than there: every output value is ONE sequential sum from +0.0 by a single lane, without a
 * cross-lane reduction, of the addends (constant * exp(-(r * r) * (1 / r_c^2))) * q_k, r = sqrt(dx dx + dy dy + dz dz), in
 * an order that depends only on the atoms and on the cell's root: with B = gmg_forces::bin_atoms(atoms, edge max(cutoff,
 * 1e-12)), the candidate bins floor((root_lo[d] - cutoff - B.lo[d]) / edge) .. floor((root_lo[d] + h0 + cutoff - B.lo[d]) /
 * edge), clipped to the grid, ascending with x fastest, a bin's atoms in the bin's stored order (ascending atom index), the
 * atoms that fail the predicate left out; with use_lists = 0 all atoms in index order.  The bits therefore do not depend on
 * the launch shape (option assemble_max_blocks caps the workgroups; option density_segment, diagnostic, sets the atoms a
 * cell's lanes stage in LDS at a time, 0 = by nq).
 * dens == NULL leaves the densities on the device exactly as gmg_charge_density does (gmg_get_charge_density,
 * gmg_rhs_assemble, gmg_assemble_rhs_resident with source = NULL and gmg_estimate_error find n_cells x nq of them); a host
 * dens [n_cells * nq] receives them and none are kept.  The atoms are host arguments and are binned on the host.  build_ms
 * (may be NULL): device time of the kernel.  Zero cells and zero atoms are valid.
 * Found on the host before anything is launched: GMG_ERR_UNSUPPORTED on a communicator, for 2D tables and for a bin grid
 * of more than 2^28 bins (use_lists != 0); GMG_ERR_INVALID without mesh tables, for nq < 1, r_c <= 0, h0 <= 0, a negative
 * cutoff, n_atoms outside [0, 2^31), or a NULL input of nonzero length.  After any failure the context holds no densities. */
int gmg_charge_density_resident(gmg_context *ctx, double origin, double h0, int64_t n_atoms, const double *atom_xyz,
                                const double *atom_q, double r_c, double cutoff, int use_lists, int nq,
                                const double *quadrature_points, double *dens /* host [n_cells*nq] or NULL */, double *build_ms);
/* cell_lo [3 n_cells], cell_h [n_cells], root_lo [3 n_cells] as gmg_charge_density_resident forms them (the same device
 * function), copied out so that they can be held against the host's bit for bit; an array passed as NULL is skipped.  The
 * same refusals for the communicator, the tables and h0.  The context's densities are left alone.                        */
int gmg_get_resident_cell_geometry(gmg_context *ctx, double origin, double h0, double *cell_lo, double *cell_h, double *root_lo);
/* The right-hand side of assemble_system (src/step-50.cc:813-828) from the densities the preceding
 * gmg_charge_density(..., dens = NULL) left on the device -- they never cross PCIe:
 *   per cell   F_i = sum_q shape[q][i] * rho_q * weight[q] * jxw_of_level[level]      (:813-820, the reference's operand order)
 *   Dirichlet  F[term_slot[t]] -= term_value[t], t ascending   (term_value = K_ij g_j, :825-828; slots ascending in the list)
 *   per DoF d  rhs[d] = sum over e in [dof_ptr[d], dof_ptr[d+1]) of (entry_coef[e] == 0 ? F[slot] : coef_table[code] * F[slot])
 * with slot = cell * 2^dim + vertex, the entries of a DoF in the order the reference's cell loop adds them
 * (distribute_local_to_global: hanging-node rows contribute to their masters with the constraint weight).  Every output
 * value is one sequential sum: deterministic, no atomics.  shape: [nq][2^dim]; cell_level: [n_cells]; rhs: device vector.
 * The arithmetic, exactly (fp64, no contraction into fused multiply-adds), so that a restatement gives the same bits:
 *   F_i starts at +0.0 and adds ((shape[q][i] * rho_q) * weight[q]) * jxw_of_level[cell_level[cell]] for q = 0 .. nq - 1;
 *   then F[term_slot[t]] = F[term_slot[t]] - term_value[t] for t = 0 .. n_terms - 1;
 *   rhs[d] starts at +0.0 and adds, e ascending, F[entry_slot[e]] (entry_coef[e] == 0) or coef_table[entry_coef[e]] *
 *   F[entry_slot[e]] (codes 1 .. 255); a DoF without entries gets +0.0.
 * 1 <= nq <= 512, dim 2 or 3, cell_level < 16.  GMG_ERR_INVALID -- found on the host, before anything is launched -- for
 * other values, without densities of n_cells x nq on the device, for a slot outside [0, n_cells 2^dim), term slots that do
 * not ascend, a dof_ptr that starts below 0 or decreases, or a NULL list of nonzero length.                              */
int gmg_rhs_assemble(gmg_context *ctx, int64_t n_cells, int nq, int dim, const double *shape, const double *weight,
                     const uint8_t *cell_level, const double *jxw_of_level /* [16] */, int64_t n_terms, const int32_t *term_slot,
                     const double *term_value, int64_t n_dofs, const int64_t *dof_ptr, const int32_t *entry_slot,
                     const uint8_t *entry_coef, const double *coef_table /* [256] */, double *rhs);

/* ---- forces on the atoms ------------------------------------------- */
/* The field E = -grad phi_h that GradientPostprocessor writes (src/step-50.cc:1124-1161), taken at the atoms, plus the
 * short-range pair forces of the erfc split (:1325-1332): F_i = q_i E_h(x_i) + F^s_i.  Definitions (gmg_forces.hpp):
 *   E_h(x) = -(1/n) sum over the octants s = 0..7 that stay in the lattice of grad u_K(s)(x), K(s) the active cell around x
 *            with coordinates on a cell boundary sent to the upper side in the directions of the bits of s (root lattice and
 *            every child split), u_K the trilinear interpolant; octant 7 is the cell of the energy's phi_h(x_i) (:1354-1363)
 *   F^s_i  = sum_{j != i, r < cutoff r_c} q_i q_j [erfc(r/r_c)/r^2 + 2/(sqrt(pi) r_c) exp(-r^2/r_c^2)/r] (x_i - x_j)/r
 *   e_i    = 1/2 sum_{j != i, r < cutoff r_c} q_i q_j erfc(r/r_c)/r
 * Every per-atom value is one sequential sum (atom / bin order): deterministic, independent of the launch shape.
 *
 * Point location (kept until gmg_reset): root lattice n0[3] at origin with cell size h0; the forest flattened level by
 * level, roots first in lexicographic order (x fastest); node[k] >= 0: flat index of child 0 (children contiguous, child
 * a = bx + 2 by + 4 bz), node[k] < 0: active cell -node[k]-1; active_dofs[8 * a + v]: DoF of vertex v of active cell a.
 * 3D only (there is no 2D entry).  GMG_ERR_INVALID for bad sizes, a node index out of range or behind its parent, or more
 * than 20 levels.                                                                                                         */
int gmg_set_point_locator(gmg_context *ctx, const int32_t n0[3], const double origin[3], double h0, int64_t n_nodes,
                          const int32_t *node, int64_t n_active, const int32_t *active_dofs);
/* phi/field/force/force_short (host arrays [n], [3n], [3n], [3n]) and the per-atom short-range energy e_short [n] (any may
 * be NULL) from the constraint-distributed solution u (device vector of n_u entries, all DoFs); cutoff in units of r_c,
 * 0 = all pairs (N-body tiles), > 0 = the pairs of the 27 neighbouring cell bins.  Two additions to the plain form:
 * n_u, so that a DoF of the locator beyond the end of u is refused (GMG_ERR_INVALID) instead of read, and force_short,
 * the pair part alone, which F - q E would return only up to cancellation.  GMG_ERR_INVALID before gmg_set_point_locator. */
int gmg_atom_forces(gmg_context *ctx, int64_t n_atoms, const double *atom_xyz, const double *atom_q, const double *u, int64_t n_u,
                    double r_c, double cutoff, double *phi, double *field, double *force, double *force_short, double *e_short);
/* exact all-pairs Coulomb forces F^d_i = sum_{j != i} q_i q_j (x_i - x_j)/r^3 and per-atom energies 1/2 sum_{j != i}
 * q_i q_j / r (either may be NULL).                                                                                     */
int gmg_direct_coulomb(gmg_context *ctx, int64_t n_atoms, const double *atom_xyz, const double *atom_q, double *force,
                       double *energy);

/* ---- exact free-space potential of the Gaussian charges ----------- */
/* Analytical_Solution::value / ::gradient (include/step_50.h:338-369) summed over ALL atoms at n_points points at once:
 *   phi(x)  = sum_i (r < 1e-10 ? 2 q_i / (sqrt(pi) r_c) : q_i erf(r / r_c) / r),                      r = |x - x_i|
 *   grad(x) = sum_i q_i (2 r exp(-(r/r_c)^2) / (sqrt(pi) r_c) - erf(r / r_c)) / r^2 * (x - x_i) / r   (0 for r = 0; for
 *             r < 0.25 r_c the factor is evaluated by its series in r / r_c, which does not cancel)
 * It stands where VectorTools::interpolate_boundary_values calls the function once per boundary DoF for
 * `Boundary conditions selection = Exact` (src/step-50.cc:661-696).  Host arrays in and out: point_xyz [3 n], phi [n] or
 * NULL, grad [3 n] or NULL.  3D only.  Every value is one sequential sum over the atoms in ascending index (definitions:
 * gmg_exact.hpp): deterministic, independent of the workgroup size (option force_block) and of how the points are cut into
 * launches (option exact_chunk_log2).  GMG_ERR_INVALID for negative sizes, r_c <= 0 or a NULL input of nonzero size; zero
 * atoms (phi = grad = 0) or zero points are valid calls.                                                              */
int gmg_gaussian_potential(gmg_context *ctx, int64_t n_atoms, const double *atom_xyz, const double *atom_q, double r_c,
                           int64_t n_points, const double *point_xyz, double *phi, double *grad);
/* postprocess_error_in_energy_norm (src/step-50.cc:1423-1461): error = || grad phi_h - grad phi ||_L2 with grad phi as
 * above, over n_cells cubes (lower corner cell_lo [3 n_cells], edge cell_h [n_cells], as gmg_charge_density takes them) with
 * nq quadrature points each (quadrature_points [nq][3] on the unit cell, weights [nq]).  grad phi_h at a point is formed
 * from the cell's 8 DoFs cell_dofs [8 n_cells] (vertex a = bx + 2 by + 4 bz) of the constraint-distributed solution u
 * (device vector of n_u entries) with the unit-cell shape gradients shape_grad [nq][8][3] divided by the cell's edge.  Per
 * cell, cell_err2 = sum_q |grad phi_h - grad phi|^2 w_q h^3 in ascending q (host array [n_cells] or NULL: the true local
 * error beside the Kelly indicator); error (may be NULL) = sqrt of their sum, formed by the two-stage partial reduction
 * (no atomics).  GMG_ERR_INVALID as above and for a DoF outside [0, n_u); GMG_ERR_UNSUPPORTED for nq > 64; zero cells
 * give error = 0.                                                                                                      */
int gmg_energy_norm_error(gmg_context *ctx, int64_t n_cells, const double *cell_lo, const double *cell_h,
                          const int32_t *cell_dofs, const double *u, int64_t n_u, int64_t n_atoms, const double *atom_xyz,
                          const double *atom_q, double r_c, int nq, const double *quadrature_points, const double *weights,
                          const double *shape_grad, double *error, double *cell_err2);

/* ---- distributed (one process per GPU, RCCL over xGMI) ------------------------------ */
#define GMG_UNIQUE_ID_BYTES 128
int gmg_comm_unique_id(void *out_id);                       /* rank 0, then broadcast by the host.  Default: an RCCL id.  With
                                                             * GMG_COMM_TRANSPORT=peer in the environment the id names the
                                                             * peer-to-peer transport for the GPUs of one node (mailboxes mapped
                                                             * with hipIpc, messages written by kernels straight into the peer's
                                                             * HBM, flags instead of collectives); it also works between
                                                             * processes sharing one GPU (tests)                              */
int gmg_comm_init(gmg_context *ctx, int rank, int n_ranks, const void *id);
/* The ranks meet on the host (call it when the operators are set, before the solve: the ranks' host-side setup times
 * differ by seconds, the kernels of the peer transport wait for each other by polling).  No-op without a communicator. */
int gmg_comm_barrier(gmg_context *ctx);
/* What the communicator turned out to be (bench.py records it): out[0] ranks, out[1] transport (0 none, 1 RCCL,
 * 2 peer-to-peer stores), out[2] peer mailbox in fine-grained memory (0 / 1), out[3] shared direction ring of the
 * coarse CG (-1 not allocated, 0 plain hipMalloc, 1 fine-grained), out[4] distinct GPUs under the ranks, out[5]
 * level 0 row-partitioned (0 / 1), out[6..7] reserved (0).  Stands where the reference would print
 * Utilities::MPI::n_mpi_processes (src/step-50.cc:120-122).                                                      */
int gmg_comm_info(gmg_context *ctx, int64_t out[8]);
/* Distributed layout: the system matrix / outer-CG vectors and level 0 (matrix,
 * coarse CG) are row-partitioned in equal chunks -- gmg_partition_range gives the canonical
 * owned range, mirroring locally_owned_dofs() of the reference (:656-657) -- while levels >= 1,
 * the transfers and the copy-index lists are passed whole (global numbering) on every rank.
 * n_level0_global = 0 keeps level 0 replicated as well (matrix passed whole, every rank runs
 * the single-GPU coarse CG): for a level 0 too small to pay three collectives per iteration.
 * Call order: gmg_comm_init, gmg_set_global_sizes, then the gmg_set_* of the operators.   */
int gmg_set_global_sizes(gmg_context *ctx, int64_t n_system_global, int64_t n_level0_global);
int gmg_partition_range(int64_t n_global, int rank, int n_ranks, int64_t *begin, int64_t *end);
/* dst_full (n_global entries, padded to n_ranks * ceil(n_global / n_ranks)) <- every rank's
 * owned slice; the reference does this with a ghosted vector assignment (:1026-1028).     */
int gmg_vec_allgather(gmg_context *ctx, int64_t n_global, double *dst_full, const double *src_local);
/* Epetra_Import plan of one operator: for each neighbour the owned local rows to send and
 * the number of ghost values received; ghosts are stored behind the owned entries in
 * neighbour order.  `which` as in gmg_spmv.                                              */
int gmg_set_halo_plan(gmg_context *ctx, int which, int n_neighbors, const int32_t *neighbor_rank,
                      const int32_t *send_count, const int32_t *send_idx, const int32_t *recv_count);

/* mg_transfer.build_matrices(mg_dof_handler) (src/step-50.cc:957-958, inside the Solve timer) ON THE DEVICE: P_level (level
 * -> level + 1, Q1 embedding, columns of coarse boundary DoFs dropped) and its transpose from the two levels' DoF tables
 * instead of a host-built CSR (gmg_set_prolongation).  coarse_vertex[i] / fine_vertex[i]: the vertex of level DoF i as
 * x | y << 21 | z << 42 in units of a lattice on which the fine level's vertices are `fine_spacing` apart (a power of two)
 * and the coarse level's 2 * fine_spacing; coarse_boundary[i] = 1 for DoFs on the domain boundary (MGConstrainedDoFs,
 * :704-706).  Rows come out in ascending column order, the transpose in ascending source-row order (the order of the
 * reference's sequential Tvmult): identical to what gmg_set_prolongation receives / derives.  build_ms (may be NULL)
 * returns the device time of the build.                                                                              */
int gmg_build_transfer(gmg_context *ctx, int level, int dim, int64_t n_coarse, const uint64_t *coarse_vertex,
                       const uint8_t *coarse_boundary, int64_t n_fine, const uint64_t *fine_vertex, uint64_t fine_spacing,
                       double *build_ms);
/* The CSR of P_level (transposed = 0) or of its transpose as the device holds it (for tests of gmg_build_transfer against
 * the host-built operator): with rowptr == NULL only the sizes are returned.                                          */
int gmg_get_transfer(gmg_context *ctx, int level, int transposed, int64_t *n_rows, int64_t *n_cols, int64_t *nnz,
                     int64_t *rowptr, int32_t *col, double *val);

/* The active-mesh system matrix formed on the device instead of a host-assembled CSR (gmg_set_system_matrix): pattern and
 * values of LaplaceProblem::assemble_system for a constant-coefficient problem, from the cells' DoFs cell_dofs
 * [n_cells * 2^dim] (vertex a = bx + 2 by + 4 bz), their levels cell_level [n_cells] (< 16), the cell matrix as the host
 * scales it per level K_of_level [16][2^dim][2^dim] (row-major), constraint_of_dof [n_dofs] (-1 or a line index) and the
 * constraint lines in CSR form (line l: entries e in [line_ptr[l], line_ptr[l + 1]) with master line_master[e] and weight
 * line_weight[e]; a Dirichlet line has no entries).  Afterwards the context is in the state gmg_set_system_matrix leaves
 * it in (operator, Jacobi diagonal, scratch): gmg_spmv(GMG_SYSTEM), gmg_precondition_jacobi and gmg_cg_solve work on it;
 * the operator is kept as CSR and applied by the row-window kernel, whose rows are summed in stored order.
 * Pattern: a cell's coupling list is its DoFs plus the masters of its constrained DoFs; row r stores the sorted union of
 * the coupling lists of all cells whose list contains r.  Stored zeros are kept (a constrained row carries all of its
 * couplings as zeros).
 * Values: every stored entry starts at +0.0 and receives its contributions in the order of the sequential loop -- cells
 * ascending, then i, then j, then the entries ri of i's line, then the entries rj of j's line:
 *   neither constrained: (dofs[i], dofs[j]) += K[i][j];   i constrained: (master(ri), dofs[j]) += w(ri) * K[i][j];
 *   j constrained: (dofs[i], master(rj)) += w(rj) * K[i][j];   both: (master(ri), master(rj)) += (w(ri) * w(rj)) * K[i][j];
 * a pair is skipped when either side is a line without entries, and a constrained i adds |K[i][i]| to (dofs[i], dofs[i])
 * before its j loop.  fp64, no contraction into fused multiply-adds, no floating-point atomics: the same bits as the host's
 * CSRMatrix for any launch shape (option assemble_max_blocks).  build_ms (may be NULL): device time of the build.
 * GMG_ERR_INVALID -- found on the host, before anything is launched -- for dim other than 2 or 3, a DoF or master outside
 * [0, n_dofs), a line index outside [0, n_lines), a line_ptr that starts below 0 or decreases, a level of 16 or more, or a
 * NULL array of nonzero length.  GMG_ERR_UNSUPPORTED on a context with a communicator, for a row with more than 512
 * columns and for sizes beyond 32-bit device indices; the context then holds no system matrix and the caller assembles on
 * the host (gmg_set_system_matrix).  Zero cells are valid: n_dofs empty rows.                                          */
int gmg_assemble_system_matrix(gmg_context *ctx, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs,
                               const uint8_t *cell_level, const double *K_of_level, const int32_t *constraint_of_dof,
                               int64_t n_lines, const int64_t *line_ptr, const int32_t *line_master, const double *line_weight,
                               double *build_ms);
/* gmg_assemble_system_matrix for a coefficient that varies in space: instead of one cell matrix per level the caller hands
 * over the coefficient VALUES at the quadrature points of every cell, and the cell matrices are formed on the device where
 * they are consumed (none is stored).  Inputs beyond those of gmg_assemble_system_matrix: nq (1 <= nq <= 64) quadrature
 * points per cell; cell_coef [n_cells][nq], the coefficient at point q of cell c (a deal.II adapter passes
 * coefficient.value_list(fe_values.get_quadrature_points(), ...) per cell); G [nq][2^dim][2^dim], the reference-cell
 * products sum_d d_d phi_i d_d phi_j at each point -- the caller forms them, their bits are the caller's; qw [nq], the
 * weights; scale_of_level [16], the factor of a cell of that level (the driver passes pow(h, dim - 2)).  The cell matrix of
 * cell c is
 *   K_c[i][j] = +0.0;   for q ascending:   K_c[i][j] += ((cell_coef[c][q] * G[q][i][j]) * qw[q]) * scale_of_level[cell_level[c]]
 * in fp64 without contraction.  Everything else is word for word the definition of gmg_assemble_system_matrix with K_c in
 * place of K[level]: the pattern, the order of the sums, |K_c[i][i]| for a constrained i, the Jacobi diagonal, the error
 * codes and the state the context is left in (gmg_get_system_matrix, gmg_system_matrix_norms, gmg_spmv, gmg_cg_solve work on
 * it).  GMG_ERR_INVALID -- found on the host, before anything is launched -- additionally for nq outside [1, 64], a NULL
 * cell_coef with n_cells > 0 and a NULL G, qw or scale_of_level.  After ANY failure the context holds no system matrix. */
int gmg_assemble_system_matrix_coef(gmg_context *ctx, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs,
                                    const uint8_t *cell_level, int nq, const double *cell_coef, const double *G, const double *qw,
                                    const double *scale_of_level, const int32_t *constraint_of_dof, int64_t n_lines,
                                    const int64_t *line_ptr, const int32_t *line_master, const double *line_weight, double *build_ms);
/* The inputs of the entries above -- DoF numbering, constraints and level flags -- formed on the device from the forest alone
 * (dof_handler.distribute_dofs / distribute_mg_dofs, make_hanging_node_constraints, interpolate_boundary_values' line list and
 * MGConstrainedDoFs, src/step-50.cc:661-706; LaplaceProblem::distribute_dofs and make_constraints on the host).
 * Input: dim (2 or 3); the root lattice n0[3] (cells per direction, 1 .. 511; n0[2] is not read in 2D); n_levels (0 .. 13) and
 * level_ptr [n_levels + 1] (level l owns the cells level_ptr[l] .. level_ptr[l + 1] - 1, level_ptr[0] = 0); for every cell of
 * every level, in the host's index order, cell_coord [n][3] (in units of that level's cell size; z = 0 in 2D) and
 * cell_first_child [n] (the index of child 0 inside the next level, the 2^dim children contiguous, or negative for an active
 * cell); level0_lexicographic (0 or 1).  Vertex keys are x | y << 21 | z << 42 with the vertex coordinates shifted by
 * 12 - level (what gmg_build_transfer takes with fine_spacing = 1 << (12 - fine level)).
 * Definitions -- integer work, the results equal the host's arrays exactly and do not depend on the launch shape (option
 * assemble_max_blocks):
 *   active cells     the cells with first_child < 0 ordered by (level, index); cell_level[a] is the level.
 *   active numbering slot s = a * 2^dim + v, v = bx + 2 by + 4 bz; the DoF of a vertex is the number of distinct vertices whose
 *                    first slot lies before its own first slot (first-touch order).  cell_dofs, n_dofs, vertex_of_dof [n_dofs].
 *   level numbering  the same rule over all cells of level l in index order; level 0 with level0_lexicographic = 1 must be the
 *                    full lattice in lexicographic cell order (x fastest) and gets dof = x + (n0[0] + 1) (y + (n0[1] + 1) z).
 *   dof_flags of a level   bit 0: the vertex lies on the domain boundary (a coordinate is 0 or n0[d] << 12); bit 1: the vertex
 *                    belongs to a face of a level-l cell (l >= 1) that lies inside the domain and has no level-l cell behind it.
 *   hanging lines    visit the active cells a ascending, then the direction d ascending, then side 0 before side 1; a face
 *                    qualifies when the same-level neighbour across it exists and is not active.  Its corners are the cell's
 *                    vertices on the face in ascending v; in 3D the constrained vertices are the face centre (masters: the 4
 *                    corners, weights 1.0 / 4), then the mid-points of the edges (0,1), (2,3), (0,2), (1,3) (masters: the 2
 *                    corners, weights 1.0 / 2), in 2D the one edge mid-point.  A vertex gets its line from the first visit
 *                    that reaches it; lines are numbered in that order and list their masters in corner order.
 *   Dirichlet lines  every DoF in ascending order whose vertex has bit-0 geometry and no hanging line gets the next line index;
 *                    such a line has no entries.
 * The lines come back UNCLOSED and without inhomogeneities (a master may itself carry a Dirichlet line): boundary values and
 * close() stay with the caller.  The tables stay on the device, owned by the context, until the next build, gmg_reset
 * (unless the option reset_keeps_mesh_tables is set, see gmg_set_option) or gmg_destroy; nothing else in the context changes.  build_ms (may be NULL): device time of the build.
 * GMG_ERR_INVALID -- found on the host, before anything is launched -- for dim other than 2 or 3, a NULL array of nonzero
 * length, a level_ptr that does not start at 0 or decreases, more than 13 levels, n0[d] outside 1 .. 511, a coordinate outside
 * its level's lattice, a first_child that points outside the next level, or level0_lexicographic = 1 with a level 0 that is
 * not the full lattice in lexicographic order; found on the device: the same cell twice in a level, or a hanging vertex without
 * a DoF (the mesh is not 2:1 balanced).  GMG_ERR_UNSUPPORTED on a context with a communicator and for 2^31 slots or more.
 * After ANY failure the context holds no mesh tables and the getters return GMG_ERR_INVALID.  Zero cells are valid.      */
int gmg_build_mesh_tables(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr,
                          const int32_t *cell_coord, const int32_t *cell_first_child, int level0_lexicographic, double *build_ms);
/* The tables of the last gmg_build_mesh_tables.  Sizes: n_cells (active cells), n_dofs, n_hanging (lines 0 .. n_hanging - 1 are
 * the hanging lines), n_lines, n_entries (= line_ptr[n_lines]).  Arrays -- any may be NULL and is then skipped, so a first call
 * with all of them NULL returns the sizes: cell_dofs [n_cells * 2^dim], cell_level [n_cells], vertex_of_dof [n_dofs],
 * constraint_of_dof [n_dofs] (-1 or a line index), line_ptr [n_lines + 1], line_master / line_weight [n_entries] in the CSR
 * form gmg_assemble_system_matrix takes, line_dof [n_lines] (the DoF each line constrains).                                */
int gmg_get_mesh_tables(gmg_context *ctx, int64_t *n_cells, int64_t *n_dofs, int64_t *n_hanging, int64_t *n_lines,
                        int64_t *n_entries, int32_t *cell_dofs, uint8_t *cell_level, uint64_t *vertex_of_dof,
                        int32_t *constraint_of_dof, int64_t *line_ptr, int32_t *line_master, double *line_weight, int32_t *line_dof);
/* One level of them: n_cells, n_dofs, cell_dofs [n_cells * 2^dim], vertex_of_dof [n_dofs], dof_flags [n_dofs] (what
 * gmg_assemble_level_matrix takes); NULL arrays are skipped.  GMG_ERR_INVALID for a level the build did not have.          */
int gmg_get_mesh_level_tables(gmg_context *ctx, int level, int64_t *n_cells, int64_t *n_dofs, int32_t *cell_dofs,
                              uint64_t *vertex_of_dof, uint8_t *dof_flags);
/* Boundary values and constraints.close() on the tables of the last gmg_build_mesh_tables, where they lie (DESIGN.md section
 * 22; the loop "close()" of LaplaceProblem::make_constraints on the host).  With H = n_hanging and L = n_lines of the tables:
 *   Dirichlet lines  l in [H, L) have no entries; inhom[l] = dirichlet_value[l - H] (host array, in line order: the DoF of
 *                    value i is line_dof[H + i]).  dirichlet_value == NULL means all values are +0.0, for any n_values.
 *   hanging lines    l < H start from inhom[l] = +0.0 and visit their stored entries e in ascending order, with
 *                    m = constraint_of_dof[line_master[e]]:  m < 0: the entry is kept, and kept entries retain their relative
 *                    order;  m >= H: the entry is dropped and inhom[l] = inhom[l] + line_weight[e] * inhom[m], in fp64 with a
 *                    rounded product and a rounded sum (no fused multiply-add);  0 <= m < H: a hanging node constrained to a
 *                    hanging node, GMG_ERR_INVALID (found on the device).
 * The closed lines -- line_ptr [L + 1], line_master / line_weight [line_ptr[L]], line_inhomogeneity [L] -- stay on the device,
 * owned by the context next to the mesh tables, until the next gmg_close_constraints (which replaces them), the next
 * gmg_build_mesh_tables, gmg_reset (unless the option reset_keeps_mesh_tables is set) or gmg_destroy.  The unclosed tables are not modified: gmg_get_mesh_tables returns what it
 * returned before.  The results do not depend on the launch shape (option assemble_max_blocks).  build_ms (may be NULL):
 * device time.  GMG_ERR_INVALID -- found on the host, before anything is launched -- without mesh tables and for
 * n_values != L - H; GMG_ERR_UNSUPPORTED on a context with a communicator.  After ANY failure the context holds no closed
 * constraints.  Zero lines are valid.                                                                                       */
int gmg_close_constraints(gmg_context *ctx, int64_t n_values, const double *dirichlet_value /* host, or NULL = all +0.0 */,
                          double *build_ms);
/* The closed lines of the last gmg_close_constraints: n_lines, n_entries (= line_ptr[n_lines]) and the arrays in the form
 * gmg_assemble_system_matrix / gmg_assemble_rhs take; NULL arrays are skipped, so a first call with all of them NULL returns
 * the sizes.  GMG_ERR_INVALID when the context holds no closed constraints.                                                */
int gmg_get_closed_constraints(gmg_context *ctx, int64_t *n_lines, int64_t *n_entries, int64_t *line_ptr,
                               int32_t *line_master, double *line_weight, double *line_inhomogeneity);
/* The resident forms of the assemblies, the right-hand side and the distribution.  Each one is, word for
 * word, its host-array sibling -- gmg_assemble_system_matrix[_coef], gmg_assemble_level_matrix[_coef], gmg_assemble_rhs,
 * gmg_distribute_constraints -- applied to dim, n_dofs, n_cells, cell_dofs and cell_level of the resident mesh tables (the
 * level entries: to the level's n_dofs, n_cells, cell_dofs and dof_flags), and, for the system matrix, the right-hand side and
 * the distribution, to constraint_of_dof and the CLOSED lines of gmg_close_constraints: the same pattern, the same order of
 * every sum, the same bits, the same state left in the context or the level.  No mesh array crosses the bus.  The remaining
 * arguments are the sibling's small host arrays and the per-cell values the host evaluates (cell_coef, source), checked as
 * the sibling checks them.  The sibling's host loops over the mesh arrays are not repeated: the tables were produced by the
 * library and are in range by construction (in particular no master of a closed line is constrained, which is what
 * gmg_distribute_constraints verifies).  Instead, on the host before anything is launched: GMG_ERR_UNSUPPORTED on a context
 * with a communicator; GMG_ERR_INVALID without mesh tables, without closed constraints (system matrix, right-hand side,
 * distribution), for a level the build did not have, for n_dofs other than the tables' (distribution), and for source == NULL
 * without device densities of n_cells x nq.  After a refusal the context or level is as the sibling leaves it (the cell-matrix
 * system form: untouched; the _coef system form and both level forms: no operator), and rhs / u are untouched.              */
int gmg_assemble_system_matrix_resident(gmg_context *ctx, const double *K_of_level, double *build_ms);
int gmg_assemble_system_matrix_coef_resident(gmg_context *ctx, int nq, const double *cell_coef, const double *G, const double *qw,
                                             const double *scale_of_level, double *build_ms);
int gmg_assemble_level_matrix_resident(gmg_context *ctx, int level, const double *K, double *build_ms);
int gmg_assemble_level_matrix_coef_resident(gmg_context *ctx, int level, int nq, const double *cell_coef, const double *G,
                                            const double *qw, double scale, double *build_ms);
int gmg_assemble_rhs_resident(gmg_context *ctx, const double *K_of_level, int nq, const double *shape, const double *weight,
                              const double *jxw_of_level, const double *source, double *rhs /* device */, double *build_ms);
int gmg_distribute_constraints_resident(gmg_context *ctx, int64_t n_dofs, double *u /* device, in place */);
/* The step between two cycles, formed on the device from the forest alone.  The three entries below take
 * the forest exactly as gmg_build_mesh_tables does -- dim, n0, n_levels, level_ptr, cell_coord, cell_first_child -- and run
 * the same checks on the host before anything is launched, with the same codes: GMG_ERR_INVALID for dim other than 2 or 3, a
 * NULL array of nonzero length, a level_ptr that does not start at 0 or decreases, more than 13 levels, n0[d] outside 1 .. 511,
 * a coordinate outside its level's lattice or a first_child that points outside the next level; GMG_ERR_UNSUPPORTED on a context
 * with a communicator and for 2^31 slots or more; found on the device by the two entries that look cells up (gmg_refine_forest,
 * gmg_build_face_table), GMG_ERR_INVALID for the same cell twice in a level.
 * Zero cells are valid.  After ANY failure the outputs are not written and the context is what it was.  Integer work and
 * look-ups: the results do not depend on the launch shape (option assemble_max_blocks).  build_ms (may be NULL): device time.
 *
 * gmg_refine_forest -- Forest::refine_flagged (csrc/host/forest.h; p4est refine + balance over vertices, deal.II's
 * limit_level_difference_at_vertices, src/step-50.cc:1095-1100).  Input beyond the forest: flag [cells of all levels], in index
 * order.
 *   closure  A flag counts only on an active cell (first_child < 0).  F is the smallest set of cells that holds the counted
 *            flags and is closed under: for an active cell c of level l >= 1 in F and each of its 3^dim - 1 neighbour positions
 *            c + {-1, 0, 1}^dim that lies inside the level-l lattice (0 <= x_d < n0[d] << l): if no level-l cell sits there, the
 *            level-(l - 1) cell at (x >> 1, y >> 1, z >> 1) is in F (it has no children, so it is active).  If that cell does
 *            not exist either the forest is not vertex-balanced: GMG_ERR_INVALID (the host calls abort()).  A flag on level
 *            l - 1 is caused only by level l: one pass from the finest level down to level 1 is the fixed point.
 *   split    Every cell of F is split, the levels independently: the new level l + 1 is the old cells of level l + 1 in
 *            their old order and, behind them, the 2^dim children of the split cells of level l in ascending cell index; child
 *            a sits at 2 c + (a & 1, (a >> 1) & 1, (a >> 2) & 1) (z = 0 in 2D), is active, and its parent's first_child becomes
 *            old_size(l + 1) + 2^dim * (number of split cells of level l before the parent).  Level 0 keeps its cells.  A split
 *            on the finest level adds a level; a new level beyond 12 is GMG_ERR_UNSUPPORTED.
 *   parent   cell_parent of a cell of level l >= 1 is the index inside level l - 1 of the cell at (x >> 1, y >> 1, z >> 1), -1
 *            on level 0; a cell of the input without one is GMG_ERR_INVALID.
 * Every cell of the old forest keeps its index inside its level.  The result stays on the device, owned by the context, until
 * the next gmg_refine_forest that succeeds, gmg_reset or gmg_destroy; new_n_levels, new_n_cells (all levels) and n_split (any may
 * be NULL) return its sizes.                                                                                                  */
int gmg_refine_forest(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr,
                      const int32_t *cell_coord, const int32_t *cell_first_child, const uint8_t *flag, int *new_n_levels,
                      int64_t *new_n_cells, int64_t *n_split, double *build_ms);
/* The forest of the last gmg_refine_forest.  Sizes: n_levels, n_cells (all levels), n_flags (the cells of the forest that went
 * in), n_split.  Arrays -- any may be NULL and is then skipped, so a first call with all of them NULL returns the sizes:
 * level_ptr [n_levels + 1], cell_coord [n_cells][3], cell_first_child [n_cells], cell_parent [n_cells], closed_flag [n_flags]
 * (the set F over the cells that went in).  GMG_ERR_INVALID when the context holds no refined forest.                       */
int gmg_get_refined_forest(gmg_context *ctx, int *n_levels, int64_t *n_cells, int64_t *n_flags, int64_t *n_split,
                           int64_t *level_ptr, int32_t *cell_coord, int32_t *cell_first_child, int32_t *cell_parent,
                           uint8_t *closed_flag);
/* gmg_transfer_solution -- SolutionTransfer::interpolate and constraints.set_zero (src/step-50.cc:1101-1121; the loop of
 * LaplaceProblem::refine_grid).  Input beyond the NEW forest: old_vertex_of_dof [n_old] and the device vector u_old [n_old]
 * (the distributed solution of the old mesh), new_vertex_of_dof [n_new], constraint_of_dof [n_new] (may be NULL: nothing is
 * zeroed).  Output: the device vector u_new [n_new].  Vertex keys as in gmg_build_mesh_tables.
 *   A new DoF whose key occurs among the old vertices takes that old value.  Any other new vertex is vertex a of some cell of
 *   level l >= 1 at c; with child = the parity bits of c and pv[p] the old value at vertex p of the cell c >> 1 of level l - 1,
 *       v = 0.0;   for p ascending:   v += w_p * pv[p]
 *       w_p = 1.0;   for d ascending:   pos_d = 0.5 * (bit_d(child) + bit_d(a));   w_p *= bit_d(p) ? pos_d : 1.0 - pos_d
 *   in fp64 without contraction into fused multiply-adds -- the host's loop verbatim.  Then u_new[i] = 0.0 wherever
 *   constraint_of_dof[i] >= 0.
 * The host takes the value from the first (level, cell, vertex) slot that finds the vertex missing; here every such slot
 * computes it and stores it, by EQUAL plain stores, no supplier is chosen.  They are equal because the value does not depend on
 * the slot: a new vertex is the mid-point of an edge, the centre of a face or the centre of a cell of level l - 1.  Its nonzero
 * weights are 0.5 on the edge's two corners, 0.25 on the face's four, 0.125 on the cell's eight; every cell that shares the edge
 * or face meets those corners in the same ascending order (vertex numbers ascend with (z, y, x) in every cell), and the other
 * addends are w_p * pv[p] = +-0.0 added to a sum that starts at +0.0 and stays the same for finite pv.  The tests hold this.
 * GMG_ERR_INVALID, found on the device, for a vertex that occurs twice in a list, a parent vertex without an old value, a
 * vertex of a cell that is not among the new vertices, or a new DoF that neither had a value nor belongs to a cell of level
 * >= 1; GMG_ERR_UNSUPPORTED for 2^31 DoFs or more.  u_new is written only on success.                                         */
int gmg_transfer_solution(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr,
                          const int32_t *cell_coord, const int32_t *cell_first_child, int64_t n_old,
                          const uint64_t *old_vertex_of_dof, const double *u_old /* device */, int64_t n_new,
                          const uint64_t *new_vertex_of_dof, const int32_t *constraint_of_dof /* or NULL */,
                          double *u_new /* device */, double *build_ms);
/* gmg_build_face_table -- LaplaceProblem::face_table: face_kind [n_active * 2 dim] and face_cell [n_active * 2 dim * 2^(dim-1)]
 * exactly as gmg_estimate_error takes them.  Active cells are numbered by (level, index); face = 2 d + side.  Per slot, with nb
 * the position across the face on the cell's level l: outside the lattice: kind 0.  A level-l cell N there: active -> kind 1,
 * face_cell[0] = N's active number; refined -> kind 2, face_cell[k] = the active numbers of the children first_child(N) + ch for
 * the ch whose bit d faces this cell (bit d of ch = 0 for side 1, 1 for side 0), ascending.  No level-l cell there: kind 3,
 * face_cell[0] = the active number of the level-(l - 1) cell at nb >> 1, face_cell[1] = this cell's quadrant of that face: the
 * parity of the cell's own in-face coordinates, lower direction in bit 0.  Unused entries are 0.  GMG_ERR_INVALID "mesh not 2:1
 * balanced across a face" for a kind-3 neighbour that is missing or not active and for a kind-2 child that is not active.
 * n_active (may be NULL) returns the number of active cells; with face_kind and face_cell both NULL nothing else is done.   */
int gmg_build_face_table(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr,
                         const int32_t *cell_coord, const int32_t *cell_first_child, int64_t *n_active, uint8_t *face_kind,
                         int32_t *face_cell, double *build_ms);
/* The right-hand side of LaplaceProblem::assemble_system formed on the device from the cell tables, without a host plan
 * (gmg_rhs_assemble wants gather lists that the host walks every cell to build): cell_dofs, cell_level, constraint_of_dof and
 * the lines are exactly what gmg_assemble_system_matrix takes, nv = 2^dim; new are line_inhomogeneity [n_lines], the
 * quadrature's tables shape [nq][nv], weight [nq], jxw_of_level [16] and the integrand at the quadrature points, source
 * [n_cells][nq] on the host (the driver's Step16 passes rhs_function(x0 + h p_q)), or source == NULL: the densities rho that
 * gmg_charge_density(..., dens = NULL) left on the device, which must be n_cells x nq.  K_of_level [16][nv][nv] may be NULL
 * when every line_inhomogeneity is 0.0.  rhs: a device vector of n_dofs entries.
 * Definition -- fp64, no contraction into fused multiply-adds, no floating-point atomics: every output is one sequential sum
 * formed by one lane, so the bits do not depend on the launch shape (option assemble_max_blocks).  With l = cell_level[c],
 * d_i = cell_dofs[c][i] and line(i) the line of d_i or none:
 *   1. per slot s = c * nv + i:   F[s] = +0.0;   for q ascending:   F[s] += ((shape[q][i] * rho[c][q]) * weight[q]) * jxw_of_level[l]
 *      (the operand order of gmg_rhs_assemble);
 *   2. then, for j ascending over the vertices of c whose line has line_inhomogeneity != 0.0:
 *        F[s] = F[s] - K_of_level[l][i][j] * line_inhomogeneity[line(j)]      -- for every i, constrained or not;
 *   3. per DoF d:   rhs[d] = +0.0;   over the slots s = (c, i) in ascending order:   if d_i is unconstrained and d_i == d:
 *        rhs[d] += F[s];   if d_i has a line: for its entries e in stored order with line_master[e] == d:
 *        rhs[d] += line_weight[e] * F[s].   A line without entries (Dirichlet) passes nothing on; a DoF that receives nothing
 *      holds +0.0.
 * These are the bits of system_rhs after LaplaceProblem::assemble_system on either of its paths (the per-DoF order is (cell,
 * vertex, entry), what the stable counting sort of the gmg_rhs_assemble plan produces).  build_ms (may be NULL): device time.
 * GMG_ERR_INVALID -- found on the host, before anything is launched -- for dim other than 2 or 3, a DoF or master outside
 * [0, n_dofs), a line index outside [0, n_lines), a line_ptr that starts below 0 or decreases, a level of 16 or more, nq
 * outside 1 .. 512, a NULL array of nonzero length, source == NULL without device densities of n_cells x nq, or K_of_level ==
 * NULL while some line_inhomogeneity != 0.0.  GMG_ERR_UNSUPPORTED on a context with a communicator and for sizes beyond
 * 32-bit device indices.  rhs is not touched after a refusal.  Zero cells are valid: rhs is all +0.0.                     */
int gmg_assemble_rhs(gmg_context *ctx, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs,
                     const uint8_t *cell_level, const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr,
                     const int32_t *line_master, const double *line_weight, const double *line_inhomogeneity,
                     const double *K_of_level /* [16][nv][nv] or NULL */, int nq, const double *shape /* [nq][nv] */,
                     const double *weight /* [nq] */, const double *jxw_of_level /* [16] */,
                     const double *source /* [n_cells][nq] or NULL */, double *rhs /* device vector, n_dofs */, double *build_ms);
/* constraints.distribute on the same constraint tables (LaplaceProblem::distribute_constraints), in place on the device vector
 * u [n_dofs]: for every constrained d with line l
 *   v = line_inhomogeneity[l];   for the entries e in stored order:   v += line_weight[e] * u[line_master[e]];   u[d] = v
 * (fp64, no contraction), one thread per constrained DoF.  The host loop runs in place and ascending, so the two agree only
 * when no master is itself constrained: the entry checks that on the host.  GMG_ERR_INVALID -- before anything is launched, u
 * untouched -- for a constrained master, a master or line index out of range, a line_ptr that starts below 0 or decreases,
 * or a NULL array of nonzero length; GMG_ERR_UNSUPPORTED beyond 32-bit device indices.                                  */
int gmg_distribute_constraints(gmg_context *ctx, int64_t n_dofs, double *u /* device, in place */,
                               const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr,
                               const int32_t *line_master, const double *line_weight, const double *line_inhomogeneity);
/* The CSR of the system matrix as the device holds it (after gmg_assemble_system_matrix; gmg_set_system_matrix keeps no CSR
 * copy: GMG_ERR_UNSUPPORTED): with rowptr == NULL only the sizes are returned.                                         */
int gmg_get_system_matrix(gmg_context *ctx, int64_t *n_rows, int64_t *nnz, int64_t *rowptr, int32_t *col, double *val);
/* Norms of that CSR (any output may be NULL).  linf: the maximum over rows of the sequential sum of |a| in stored order;
 * l1: the maximum over columns of the sum of |a| in ascending row order, gathered through the structurally symmetric
 * pattern -- both bit-equal to the host's CSRMatrix::linfty_norm / l1_norm.  frobenius: sqrt of the sum of squares by the
 * two-stage partial reduction (not bit-equal: relative error at most (nnz + 2) 2^-53).                                 */
int gmg_system_matrix_norms(gmg_context *ctx, double *l1, double *linf, double *frobenius);

/* A multigrid level matrix A_l and its interface ("edge") matrix I_l formed on the device instead of host-assembled CSRs
 * (gmg_set_level_matrix + gmg_set_edge_matrix): LaplaceProblem::assemble_level for a constant-coefficient problem, from
 * the level's cell table cell_dofs [n_cells * 2^dim] (vertex a = bx + 2 by + 4 bz), ONE cell matrix K [2^dim][2^dim]
 * (row-major, as the host scales it for the level) and dof_flags [n_dofs]: bit 0 = on the boundary, bit 1 = on the
 * refinement edge.  Afterwards the level is in the state gmg_set_level_matrix followed by gmg_set_edge_matrix leaves it in
 * with the host's matrices: operator, Jacobi diagonal, Chebyshev bound, SSOR plan (gmg_set_ssor_blocks /
 * gmg_set_ssor_block_rows / gmg_set_ssor_partition are honoured; the plan is built on the host from one download of the
 * CSR), work vectors, on level 0 the coarse CG's vectors and the coarse CG selected, I_l and I_l^T (or none).  A_l is kept as
 * CSR and applied by the row-window kernel.
 * A_l pattern: row r stores the sorted union of the DoFs of all cells that contain r; stored zeros are kept.
 * A_l values: every entry starts at +0.0; cells ascending, then i ascending: if dof_flags[dofs[i]] != 0, (dofs[i], dofs[i])
 * += |K[i][i]| and nothing else from this i; otherwise, for j ascending with dof_flags[dofs[j]] == 0, (dofs[i], dofs[j]) +=
 * K[i][j].  Jacobi diagonal 1 / a_rr; Chebyshev bound max_r (sum_k |a_rk| in stored order) / |a_rr|.
 * I_l: the pairs (dofs[i], dofs[j]) of any cell with dof_flags[dofs[i]] == 2 and dof_flags[dofs[j]] == 0, each the sum of its
 * cells' K[i][j] in ascending cell order starting from the first contribution; sums == 0.0 are dropped (as
 * gmg_set_edge_matrix drops them); I_l^T lists every column's entries in ascending row.  A level without a surviving entry
 * has no interface matrix.  fp64, no contraction into fused multiply-adds, no floating-point atomics: the same bits as the
 * host's matrices for any launch shape (option assemble_max_blocks).  build_ms (may be NULL): device time of the build.
 * GMG_ERR_INVALID -- found on the host, before anything is launched -- for dim other than 2 or 3, a level outside the
 * context, a DoF outside [0, n_dofs), flag bits above 1, a NULL array of nonzero length, a negative size, or SSOR block
 * boundaries of this level that do not end at n_dofs.  GMG_ERR_UNSUPPORTED on a context with a communicator (a
 * row-partitioned level 0 included), for a row with more than 512 columns and for sizes beyond 32-bit device indices.
 * After any failure the level holds no operator.  Zero cells are valid: n_dofs empty rows.                              */
int gmg_assemble_level_matrix(gmg_context *ctx, int level, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs,
                              const double *K, const uint8_t *dof_flags, double *build_ms);
/* gmg_assemble_level_matrix for a coefficient that varies in space: nq, cell_coef [n_cells][nq] (all cells of the level), G
 * and qw as for gmg_assemble_system_matrix_coef, and ONE scale (the driver passes pow(h_l, dim - 2)); the cell matrix of cell
 * c is
 *   K_c[i][j] = +0.0;   for q ascending:   K_c[i][j] += ((cell_coef[c][q] * G[q][i][j]) * qw[q]) * scale
 * in fp64 without contraction.  Everything else is word for word the definition of gmg_assemble_level_matrix with K_c in
 * place of K: the patterns, the order of the sums, |K_c[i][i]| for a flagged i, the Jacobi diagonal, the Chebyshev bound, I_l
 * with its dropped zeros, I_l^T, the SSOR plan, the error codes and the state the level is left in.  GMG_ERR_INVALID
 * additionally for nq outside [1, 64], a NULL cell_coef with n_cells > 0 and a NULL G or qw.  After any failure the level
 * holds no operator.                                                                                                    */
int gmg_assemble_level_matrix_coef(gmg_context *ctx, int level, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs,
                                   int nq, const double *cell_coef, const double *G, const double *qw, double scale,
                                   const uint8_t *dof_flags, double *build_ms);
/* The CSR of a level's operators as the device holds them: which = GMG_LEVEL_A, GMG_LEVEL_EDGE (I_l) or GMG_LEVEL_EDGE_T
 * (I_l^T).  With rowptr == NULL only the sizes are returned.  GMG_ERR_UNSUPPORTED where the device keeps no CSR copy (a
 * lattice level 0, an operator stored in a SELL layout); an absent interface matrix returns nnz = 0.                       */
#define GMG_LEVEL_A 0
#define GMG_LEVEL_EDGE 1
#define GMG_LEVEL_EDGE_T 2
int gmg_get_level_matrix(gmg_context *ctx, int level, int which, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int64_t *rowptr,
                         int32_t *col, double *val);

/* The error estimator and the refinement marks of an adaptive cycle (src/step-50.cc:1020-1089: KellyErrorEstimator with the
 * cell diameter as scaling, the cell residual, cells at or above a fraction of the largest indicator are marked) formed on
 * the device from the cells' DoFs cell_dofs [n_cells * 2^dim] (vertex a = bx + 2 by + 4 bz), their levels cell_level
 * [n_cells] (< 16), a face table and the constraint-distributed solution u (device vector, n_u entries).
 * Face table: slot = cell * 2 dim + f, face f = 2 d + side (deal.II order), nfc = 2^(dim-1) integers per slot:
 *   face_kind 0  domain boundary; the slot contributes nothing
 *   face_kind 1  active neighbour on the same level; face_cell[slot * nfc] is its index
 *   face_kind 2  the neighbour is refined once; face_cell[slot * nfc + k] is the active child occupying quadrant k of the
 *                face (children in ascending child number; bit 0 of k is the lower in-face direction)
 *   face_kind 3  the neighbour is one level coarser; face_cell[slot * nfc] is its index, face_cell[slot * nfc + 1] the
 *                quadrant of the coarse face this cell occupies
 * Values (fp64, no contraction into fused multiply-adds, this operand order):
 *   U[c][v] = u[cell_dofs[c * 2^dim + v]];   for v ascending over the vertices with bit d clear,
 *   g_c[k] = (U[c][v | 1 << d] - U[c][v]) / h_of_level[level(c)];
 *   B(c, s, t) = c0 * (1 - s) * (1 - t) + c1 * s * (1 - t) + c2 * (1 - s) * t + c3 * s * t, left to right
 *                (2D: c0 * (1 - s) + c1 * s);   gx, gw: the 1-D Gauss rule on [0, 1] with ng = degree + 1 points;
 *   kind 1, m the minus-side and p the plus-side cell of the face: jump[k] = g_p[k] - g_m[k],
 *     I = sum_{q1} sum_{q0} ((((j * j) * gw[q0]) * gw[q1]) * face_measure_of_level[l]) from +0.0, j = B(jump, gx[q0], gx[q1])
 *     (2D: one q1 with weight 1.0); both cells' slots hold the same I;
 *   sub-face of a coarse cell C (level l) and a fine cell F (level l + 1) in quadrant (Q0, Q1):
 *     j = B(g_F, s, t) - B(g_C, 0.5 * (Q0 + s), 0.5 * (Q1 + t)), I_sub summed the same way with
 *     face_measure_of_level[l + 1]; the kind-3 slot of F holds I_sub, the kind-2 slot of C the sum of its nfc sub-face
 *     integrals from +0.0 in ascending k;
 *   per cell: float acc = 0; for f ascending acc += (float)(diameter_of_level[l] * face_int[a][f]);
 *     kelly_sq = (double)acc; eta = sqrtf(acc), correctly rounded;
 *   residual != 0: error = sum_q ((t * t) * weight[q]) * jxw_of_level[l] with t = 0.0 + (4.0 * pi) * dens[a * nq + q] (the
 *     densities already carry one factor 4 pi: the reference's quirk is kept); residual_sq = (diam * diam) * error;
 *     residual == 1 (Kelly + residual): eta = (float)sqrt((double)e * e + residual_sq) with e the Kelly eta and a correctly
 *     rounded fp64 square root; residual == 2 forms residual_sq only.  dens == NULL: the densities
 *     gmg_charge_density(..., dens = NULL) left on the device (they must be n_cells x nq); otherwise a host array;
 *   mx = max |eta| in fp32, threshold = fraction * (double)mx, mark[a] = |eta[a]| >= threshold, n_marked their number.
 *     Zero cells, or u constant, give threshold 0 (and every cell marked).
 * Every output is one sequential sum, or a maximum, per slot or cell; no floating-point atomics: the same bits as
 * LaplaceProblem::estimate_error_and_mark_cells for any launch shape (option estimate_max_blocks).  The outputs eta
 * [n_cells], kelly_sq, residual_sq [n_cells], face_int [n_cells * 2 dim], threshold, mark [n_cells], n_marked and build_ms
 * (device time of the three kernels) are host memory and any of them may be NULL.  Nothing is kept in the context.
 * GMG_ERR_INVALID -- found on the host, before anything is launched -- for dim other than 2 or 3, a level of 16 or more, a
 * DoF outside [0, n_u), a kind above 3, a face_cell index outside [0, n_cells), a kind-1, -2 or -3 neighbour whose level is
 * not l, l + 1 or l - 1, a quadrant of 2^(dim-1) or more, ng outside 1 .. 8, residual outside 0 .. 2, nq outside 1 .. 512
 * when residual != 0, a fraction that is negative or not finite, device densities that are missing or of another shape,
 * or a NULL array of nonzero length.                                                                                    */
int gmg_estimate_error(gmg_context *ctx, int dim, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level,
                       const uint8_t *face_kind, const int32_t *face_cell, const double *h_of_level,
                       const double *face_measure_of_level, const double *diameter_of_level, int ng, const double *gauss_x,
                       const double *gauss_w, const double *u, int64_t n_u, int residual, int nq, const double *weight,
                       const double *jxw_of_level, const double *dens, double fraction, float *eta, double *kelly_sq,
                       double *residual_sq, double *face_int, double *threshold, uint8_t *mark, int64_t *n_marked,
                       double *build_ms);

/* The step that ends an adaptive cycle on the tables the last gmg_build_mesh_tables left on the device:
 * face table, estimator and marks, the refinement from those marks, and the error norm, without a mesh array crossing the bus.
 * What the six entries below share: GMG_ERR_UNSUPPORTED on a context with a communicator; GMG_ERR_INVALID when the context
 * holds no mesh tables; zero cells are valid.  The face table and the marks are owned by the context INSIDE the mesh tables, as
 * the closed lines of gmg_close_constraints are: the next gmg_build_mesh_tables, gmg_reset (unless the option
 * reset_keeps_mesh_tables is set) and gmg_destroy drop them with the tables.
 *
 * gmg_build_face_table_resident -- gmg_build_face_table word for word (the same forest checks with the same codes, the same
 * kernels, the same integers), but face_kind and face_cell are not downloaded: they stay on the device, moved into the context
 * after the last step that can fail.  The forest must be the one the tables were built from: GMG_ERR_INVALID if dim differs
 * from the tables' dim or the forest's number of active cells is not the tables' n_cells.  The call first drops the face table
 * and the marks the context holds (marks belong to the table they were formed with), so the table of the last successful call
 * is the one kept and after ANY failure the context holds no face table.  Device memory kept: 28 bytes per (cell, face) slot
 * in 3D (1 byte of kind, 4 integers), 9 in 2D -- 168 bytes per active cell in 3D.  n_active, build_ms: may be NULL.          */
int gmg_build_face_table_resident(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr,
                                  const int32_t *cell_coord, const int32_t *cell_first_child, int64_t *n_active, double *build_ms);
/* The kept face table copied out: n_active (= the tables' n_cells), face_kind [n_active * 2 dim], face_cell [n_active * 2 dim *
 * 2^(dim-1)]; NULL arrays are skipped.  GMG_ERR_INVALID when the context holds none.                                        */
int gmg_get_face_table(gmg_context *ctx, int64_t *n_active, uint8_t *face_kind, int32_t *face_cell);
/* gmg_estimate_error_resident -- gmg_estimate_error applied to dim, n_cells, cell_dofs and cell_level of the resident tables and
 * to the kept face table: the same three kernels, the same order of every sum, the same bits in every output, for any launch
 * shape (option estimate_max_blocks).  The remaining arguments are the sibling's and are checked as the sibling checks them;
 * the sibling's host loops over the mesh arrays are not repeated (the tables and the face table were produced by the library
 * and are in range by construction).  Instead: GMG_ERR_INVALID without a face table, for n_u other than the tables' n_dofs,
 * and, with residual != 0 and dens == NULL, for device densities that are missing or not n_cells x nq.
 * New: on success the marks (uint8_t [n_cells]) and n_marked stay on the device in the context, with the lifetime of the face
 * table, for gmg_refine_forest_marked.  They are dropped first thing in the call: after ANY failure the context holds no marks.
 * The host outputs are the sibling's and any may be NULL.                                                                   */
int gmg_estimate_error_resident(gmg_context *ctx, const double *h_of_level, const double *face_measure_of_level,
                                const double *diameter_of_level, int ng, const double *gauss_x, const double *gauss_w, const double *u,
                                int64_t n_u, int residual, int nq, const double *weight, const double *jxw_of_level, const double *dens,
                                double fraction, float *eta, double *kelly_sq, double *residual_sq, double *face_int, double *threshold,
                                uint8_t *mark, int64_t *n_marked, double *build_ms);
/* The kept marks copied out: n_cells, mark [n_cells] (NULL is skipped), n_marked.  GMG_ERR_INVALID when the context holds none. */
int gmg_get_marks(gmg_context *ctx, int64_t *n_cells, uint8_t *mark, int64_t *n_marked);
/* gmg_refine_forest_marked -- gmg_refine_forest with flag[c] = first_child[c] < 0 ? mark[active number of c] : 0, formed on the
 * device from the kept marks.  The active number of a cell is the number of active cells before it in (level, index) order
 * (the scan gmg_build_face_table forms), which is how the tables number their cells.  Closure, split, parents, the result read
 * by gmg_get_refined_forest (closed_flag included) and every refusal are the sibling's.  GMG_ERR_INVALID when the context holds
 * no marks or the forest's number of active cells is not the marks' length.  The marks are left in place.                    */
int gmg_refine_forest_marked(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr,
                             const int32_t *cell_coord, const int32_t *cell_first_child, int *new_n_levels, int64_t *new_n_cells,
                             int64_t *n_split, double *build_ms);
/* gmg_energy_norm_error_resident -- gmg_energy_norm_error applied to n_cells and cell_dofs of the resident tables and to
 * cell_lo / cell_h as gmg_charge_density_resident defines them from origin and h0 (the same device function, written into
 * temporaries of the call; gmg_get_resident_cell_geometry copies the same values out): the same kernel, the same bits in error
 * and cell_err2.  3D tables only: GMG_ERR_UNSUPPORTED for 2D tables and, as in the sibling, for nq > 64.  GMG_ERR_INVALID for
 * h0 <= 0, for n_u other than the tables' n_dofs, and for what the sibling refuses of the remaining arguments.               */
int gmg_energy_norm_error_resident(gmg_context *ctx, double origin, double h0, const double *u, int64_t n_u, int64_t n_atoms,
                                   const double *atom_xyz, const double *atom_q, double r_c, int nq, const double *quadrature_points,
                                   const double *weights, const double *shape_grad, double *error, double *cell_err2);

/* The patches of the graphical output (the reference's output_results, src/step-50.cc:1149-1308: what deal.II's
 * DataOut::build_patches(0) forms) on the device.  One patch per active cell with nv = 2^dim patch
 * vertices and nothing shared between cells: slot s = a * nv + v, vertex v = bx + 2 by + 4 bz.  cell_dofs [n_cells * nv],
 * cell_level [n_cells], vertex_of_dof [n_dofs] (21 bits per direction on the level-12 lattice, as gmg_get_mesh_tables returns
 * them) and up to 8 DoF vectors dof_field[j] [n_dofs] are host arrays; u is a device vector of n_u = n_dofs entries.
 * Values (fp64, no contraction into fused multiply-adds, this operand order), k = vertex_of_dof[cell_dofs[s]]:
 *   point[3 s + d]    = origin + (h0 / 4096.0) * (double)((k >> 21 d) & 0x1fffff) for d < dim, +0.0 for d >= dim: the bits of
 *                       the driver's vertex coordinates, so duplicated vertices of neighbouring cells coincide exactly;
 *   U[v] = u[cell_dofs[a * nv + v]];   solution[s] = U[v];
 *   g = (U[v | 1 << d] - U[v & ~(1 << d)]) / h_l,  h_l = h0 / (double)(1 << cell_level[a])  (g_c of gmg_estimate_error);
 *   grad_phi[3 s + d] = -g for d < dim, +0.0 for d >= dim;
 *   patch_field[j][s] = dof_field[j][cell_dofs[s]].
 * The outputs point [n_cells * nv * 3], solution [n_cells * nv], grad_phi [n_cells * nv * 3], patch_field[j] [n_cells * nv]
 * and build_ms (device time of the kernels) are host memory; any of them, patch_field itself included, may be NULL and is then
 * skipped.  The work is cut into launches of at most 2^k cells, k = option output_chunk_log2; the device temporaries of the
 * call hold one launch's results (56 bytes per slot and 8 per gathered field).  Every value has one writer and no sum: the
 * results depend neither on k nor on the launch shape (option assemble_max_blocks).  Nothing is kept in the context.
 * GMG_ERR_INVALID -- found on the host, before anything is launched -- for dim other than 2 or 3, a level above 13, a DoF
 * outside [0, n_dofs), n_u other than n_dofs, n_fields outside 0 .. 8, h0 <= 0, or a NULL input of nonzero length;
 * GMG_ERR_UNSUPPORTED on a context with a communicator.  Zero cells are valid.                                              */
int gmg_output_patches(gmg_context *ctx, int dim, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level,
                       const uint64_t *vertex_of_dof, int64_t n_dofs, double origin, double h0, const double *u, int64_t n_u,
                       int n_fields, const double *const *dof_field, double *point, double *solution, double *grad_phi,
                       double *const *patch_field, double *build_ms);
/* gmg_output_patches_resident -- gmg_output_patches applied to dim, n_cells, n_dofs, cell_dofs, cell_level and vertex_of_dof
 * of the tables the last gmg_build_mesh_tables left on the device: the same kernel, the same bits, and no mesh array crosses
 * the bus.  The sibling's host loops over the mesh arrays are not repeated (the tables are in range by construction).
 * GMG_ERR_INVALID when the context holds no mesh tables, for n_u other than the tables' n_dofs, and for what the sibling
 * refuses of the remaining arguments; GMG_ERR_UNSUPPORTED on a context with a communicator.                                 */
int gmg_output_patches_resident(gmg_context *ctx, double origin, double h0, const double *u, int64_t n_u, int n_fields,
                                const double *const *dof_field, double *point, double *solution, double *grad_phi,
                                double *const *patch_field, double *build_ms);

/* Energy and forces at the atoms on the tables the last gmg_build_mesh_tables left on the device.  What
 * the four entries below share: GMG_ERR_UNSUPPORTED on a context with a communicator and for 2D tables; GMG_ERR_INVALID when
 * the context holds no mesh tables; zero cells and zero atoms are valid (without cells phi_h and the field are 0).  The
 * resident locator is owned by the context INSIDE the mesh tables, as the face table is: the next gmg_build_mesh_tables,
 * gmg_reset (unless the option reset_keeps_mesh_tables is set) and gmg_destroy drop it with the tables.  It is separate from
 * the locator of gmg_set_point_locator: neither form sees the other's.
 *
 * gmg_build_point_locator_resident -- the node array of gmg_set_point_locator formed on the device from the forest the tables
 * were built from (arguments and host checks of gmg_build_face_table_resident, with its codes).  With k = level_ptr[l] + c:
 *   node[k] = level_ptr[l + 1] + first_child[k]        where first_child[k] >= 0,
 *   node[k] = -(active number of k) - 1                otherwise,
 * the active number being the number of active cells before k in (level, index) order, which is how the tables number their
 * cells.  GMG_ERR_INVALID, found on the host before anything is launched, if dim differs from the tables' dim, the forest's
 * number of active cells is not the tables' n_cells, or level 0 is not the full n0 lattice in lexicographic cell order (x
 * fastest; the check of gmg_build_mesh_tables with level0_lexicographic = 1): the roots are indexed by coordinate.  The
 * cells' DoFs are not copied: the locator reads the tables' cell_dofs.  Device memory kept: 4 bytes per forest cell.  The call
 * first drops the locator the context holds, so after ANY failure none is held.  n_nodes, build_ms: may be NULL.            */
int gmg_build_point_locator_resident(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr,
                                     const int32_t *cell_coord, const int32_t *cell_first_child, int64_t *n_nodes, double *build_ms);
/* The kept node array copied out: n_nodes (cells of all levels), node [n_nodes]; NULL is skipped.  GMG_ERR_INVALID when the
 * context holds none.                                                                                                      */
int gmg_get_point_locator(gmg_context *ctx, int64_t *n_nodes, int32_t *node);
/* gmg_atom_forces_resident -- gmg_atom_forces on the resident locator: root lattice n0 of the forest the locator was built from,
 * origin (the same in every direction) and h0 as gmg_charge_density_resident takes them.  The same kernels, the same bins, the
 * same bits in every output.  GMG_ERR_INVALID without a resident locator, for h0 <= 0, for n_u other than the tables' n_dofs
 * (which covers every DoF of cell_dofs), and for what the sibling refuses of the remaining arguments.                       */
int gmg_atom_forces_resident(gmg_context *ctx, double origin, double h0, int64_t n_atoms, const double *atom_xyz, const double *atom_q,
                             const double *u, int64_t n_u, double r_c, double cutoff, double *phi, double *field, double *force,
                             double *force_short, double *e_short);
/* gmg_electrostatic_energy_resident -- the three sums of the electrostatic energy (src/step-50.cc:1310-1420), formed on the
 * device; 24 bytes return.  out = {short, fe_long, self}, each ONE sequential sum over the atoms in ascending index, fp64, no
 * contraction into fused multiply-adds:
 *   short   = sum_i e_i                               e_i exactly as gmg_atom_forces returns it in e_short (same kernels)
 *   fe_long = sum_i (0.5 * q_i) * phi_i               phi_i = phi_h(x_i) of octant 7 with clamp, as gmg_atom_forces returns phi
 *   self    = sum_i q_i * q_i / (sqrt(pi) * r_c)      the divisor formed once
 * total = short + fe_long - self is left to the caller.  The sums do not depend on the launch shape (options force_block,
 * assemble_max_blocks).  Arguments and refusals of gmg_atom_forces_resident; out must not be NULL; build_ms (may be NULL):
 * device time from the first kernel to the last.                                                                           */
int gmg_electrostatic_energy_resident(gmg_context *ctx, double origin, double h0, int64_t n_atoms, const double *atom_xyz,
                                      const double *atom_q, const double *u, int64_t n_u, double r_c, double cutoff, double out[3],
                                      double *build_ms);

/* ---- measurement -------------------------------------------------------------------- */
typedef struct gmg_stats {
  int64_t coarse_solves;        /* calls of the coarse solver since the last reset           */
  int64_t coarse_iterations;    /* inner CG iterations summed over those calls               */
  int64_t vcycles;
  int64_t spmv0_samples;        /* live level-0 SpMV launches bracketed by HIP events        */
  double spmv0_ms_total;        /* summed event time of those launches                       */
  int64_t spmv0_rows, spmv0_nnz; /* shape of the level-0 operator (for algorithmic bytes)    */
  int64_t cgupd_samples;
  double cgupd_ms_total;
  int64_t coarse_variant;       /* 1 = fused (SpMV + direction update), 2 = unfused, of the last solve */
  int64_t spmv0_layout;         /* 0 = CSR row windows; else 1 (SELL-64) + 2 (8-bit value codes) + 4 (16-bit column offsets) + 8 (pattern-run kernel) + 16 (row classes) + 32 (plane-by-plane lattice kernel) + 64 (formed on the device: no CSR behind it) */
  int64_t spmv0_matrix_bytes;   /* bytes of the level-0 operator one SpMV streams in its device layout */
  int64_t spmv0_pattern_slices, spmv0_slices; /* slices served by a column pattern / all slices */
  int64_t coarse_enqueued;      /* coarse iterations enqueued, incl. those that returned at once after convergence */
  int64_t spmv0_noop_samples;   /* sampled level-0 launches that returned at once (after convergence): ...    */
  double spmv0_noop_ms_total;   /* ... their summed event time                                                */
  int64_t sgs_samples;          /* SSOR sweep launches (levels >= 1) bracketed by HIP events while profiling is on   */
  double sgs_ms_total;          /* their summed event time                                                           */
  int64_t sgs_substeps;         /* dependent steps those launches walked (the sweep is latency bound)                */
  int64_t sgs_stream_bytes;     /* record bytes they streamed                                                        */
  int64_t sgs_launches;         /* all SSOR sweep launches while profiling was on (every sample_every-th one is timed)  */
  double build_matrices_ms;     /* device time of gmg_build_transfer calls since the last reset (the reference counts build_matrices in its Solve timer, :941-958) */
  int64_t coarse_solver;        /* GMG_COARSE_CG (0) or GMG_COARSE_DIRECT (1), of the last coarse solve */
} gmg_stats;
int gmg_stats_reset(gmg_context *ctx);
int gmg_stats_get(gmg_context *ctx, gmg_stats *out);
/* attach HIP start / stop events to every `sample_every`-th level-0 SpMV launch and every `sample_every`-th SSOR
 * sweep launch (0 = off); when the event pool is full the sampling stops, nothing ever synchronises.        */
int gmg_set_profiling(gmg_context *ctx, int sample_every);
/* streaming-read and copy bandwidth of this device (GB/s) on n_bytes per array: the measured
 * ceiling bench.py prints beside the 8 TB/s spec peak.                                    */
int gmg_calibrate_hbm(gmg_context *ctx, int64_t n_bytes, int reps, double *read_gbps, double *copy_gbps);
/* tuning knobs: coarse_chunk = iterations enqueued between host convergence checks (0 = predicted
 * from the previous solve); cg_variant = 0 auto by size, 1 fused two-kernel iteration (SpMV also
 * forms d = beta d - g), 2 three-kernel iteration.                                          */
int gmg_set_tuning(gmg_context *ctx, int coarse_chunk, int cg_variant);
/* Diagnostic / measurement options by name (defaults are the production paths).  Keys: host_threads,
 * debug_upload, disable_sell, disable_patterns, disable_compression, disable_sellp, disable_rowclass, sell_grid, sellp_cost,
 * cg_variant, coarse_chunk, coarse_direct (0 / 1, see gmg_set_coarse_solver), coarse_direct_max_blocks (cap on the grids of the direct
 * coarse solver's passes, 0 = by size; the results do not depend on it), sgs_y_slots (doubles of LDS the SSOR sweep may use for y: small values force
 * several LDS ranges), sgs_sliding (default 1: the four-wave sweep takes a whole sweep direction of a block as one self-contained LDS range, y slots
 * recycled, wherever the block's live rows fit; 0: always the ranged plan; same bits either way, see gmg_get_ssor_plan), sgs_pack (rows scheduled by slack, see gmg_ssor_pack_levels), sgs_disable_wave (SSOR through the generic CSR sweep), sgs_disable_phase (the one-wave sweep),
 * sgs_phase_profile (cycle counters of the four-wave sweep: same results, one rank only), sgs_profile (instrumented
 * one-wave sweep; its wrong-result timing modes exist only in a -DGMG_EXPERIMENTS build, tools/build_experiments.sh),
 * sgs_lds_bytes_override (tests: a value over the CU's 160 KB makes the sweep's launch fail -> GMG_ERR_HIP), force_block (64 | 128 |
 * 256: workgroup size of the force kernels and of the exact-potential kernels; the results do not depend on it),
 * exact_chunk_log2 (0 .. 35, default 35: gmg_gaussian_potential and gmg_energy_norm_error do at most 2^k point-atom
 * evaluations per launch; tests force many launches on small inputs, the results do not depend on it), output_chunk_log2
 * (0 .. 30, default 20: gmg_output_patches forms at most 2^k cells per launch, which is also the size of its device
 * temporaries; the results do not depend on it), density_segment
 * (0 .. 2047, default 0 = by nq: atoms per LDS segment of gmg_charge_density_resident, made odd and fitted to the group size
 * and to 64 KB per workgroup; the results do not depend on it), reset_keeps_mesh_tables
 * (0 / 1, default 0: while it is 1, gmg_reset leaves the tables of gmg_build_mesh_tables and the closed lines of
 * gmg_close_constraints in the context instead of dropping them -- for a caller that resets the context between the build and
 * the resident assemblies; the caller must set it back to 0 after that reset, or every later gmg_reset keeps the tables too;
 * the next gmg_build_mesh_tables and gmg_destroy drop them regardless), cheb_polynomial, cheb_lmax_source,
 * cheb_lanczos_steps (1 .. 64), cheb_safety (>= 1): the arguments of gmg_set_chebyshev, one at a time; cheb_degree (0 .. 64,
 * default 0: a value > 0 overrides the degree given to gmg_set_smoother); lanczos_max_blocks (0 .. 65536, default 0 = by
 * size: cap on the grids of the Lanczos estimate's kernels; the results do not depend on it).  Options that shape a device
 * layout take effect at the next gmg_set_*_matrix.  The same keys are read once from the environment
 * variable GMG_OPTIONS="key=value,..." at gmg_create (for profiling scripts around bench.py).        */
int gmg_set_option(gmg_context *ctx, const char *key, double value);
/* SSOR blocks B: 1 = exact sequential sweep (the reference on one rank); B > 1 = what the
 * reference's smoother does on B MPI ranks: symmetric Gauss-Seidel inside each block of
 * consecutive rows, couplings between blocks dropped (Ifpack's rank-local matrix).  Call before
 * the level matrices are set.                                                              */
int gmg_set_ssor_blocks(gmg_context *ctx, int n_blocks);
/* Where the SSOR blocks of a level start and end.  The reference's ranks each sweep the rows they own on that level
 * (mg_matrices[level] over locally_owned_mg_dofs(level), src/step-50.cc:722-723, smoothed by the rank-local
 * PreconditionSSOR of :970-973) -- p4est's cell-balanced chunks (:120-122), not equal runs of rows.  A level's boundaries
 * come from the first source that applies: the explicit ones of gmg_set_ssor_block_rows, the balanced cuts if
 * gmg_set_ssor_partition chose them, equal runs of rows (the default).
 *   gmg_set_ssor_block_rows: block_row[0..n_blocks], 0 first, never decreasing, empty blocks allowed (a rank may own no
 *     row of a level); levels >= 1 only (level 0 is the coarse CG).  Kept until cleared with n_blocks = 0 (also across
 *     gmg_reset).  Call before the level's matrix is set; a last entry that is not that matrix's n_rows makes
 *     gmg_set_level_matrix fail with GMG_ERR_INVALID before anything is uploaded.  n_blocks replaces gmg_set_ssor_blocks
 *     for that level (several ranks: n_blocks = n_ranks, or a multiple, block b swept by rank b / (n_blocks / n_ranks)).
 *   gmg_set_ssor_partition: GMG_SSOR_PARTITION_ROWS (default) or _BALANCED: B - 1 cuts, with B of gmg_set_ssor_blocks
 *     (clamped to (n_rows + 63) / 64 as the equal runs are), that equalise the modelled sweep time of the blocks
 *     (DESIGN.md 4).  Also the gmg_set_option / GMG_OPTIONS key ssor_balanced.
 *   gmg_get_ssor_partition: the boundaries the level's plan uses (block_row: n_blocks + 1 entries, may be NULL) and each
 *     block's dependent sub-steps, both sweep directions (block_steps: n_blocks entries, may be NULL).                  */
#define GMG_SSOR_PARTITION_ROWS 0
#define GMG_SSOR_PARTITION_BALANCED 1
int gmg_set_ssor_block_rows(gmg_context *ctx, int level, int n_blocks, const int64_t *block_row);
int gmg_set_ssor_partition(gmg_context *ctx, int kind);
int gmg_get_ssor_partition(gmg_context *ctx, int level, int *n_blocks, int64_t *block_row, int64_t *block_steps);
/* The balanced cuts of gmg_set_ssor_partition for one level matrix (host CSR, ascending columns), without a context or a
 * device: the same routine, deterministic (every rank computes the same cuts from the replicated level matrix).  val may
 * be NULL (every stored entry couples; else stored zeros do not, as in the sweep's plan).  block_row: n_blocks + 1
 * entries, those behind min(n_blocks, (n + 63) / 64) blocks equal n; block_cost (may be NULL): each block's modelled
 * sweep time in microseconds.                                                                                         */
int gmg_ssor_balance_rows(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int n_blocks,
                          int64_t *block_row, double *block_cost);
/* What the SSOR sweep's plan of a level (>= 1) looks like.  out: [0] forward LDS ranges, [1] backward LDS ranges (all blocks),
 * [2] how many of them are self-contained (a whole sweep direction of a block in one range, nothing loaded or written back at
 * its ends: option sgs_sliding), [3] y slots (doubles of LDS) the sweep kernel is launched with, [4] / [5] the most y slots
 * live at once in a forward / backward direction of any block as the slot allocator found them (0: it did not run), [6]
 * dependent sub-steps, [7] bytes of the record stream.  All 0 for a level on the generic CSR sweep.                          */
int gmg_get_ssor_plan(gmg_context *ctx, int level, int64_t out[8]);
/* The level rows the self-contained backward ranges of a level store their results to: the row number every backward
 * record carries, as written into the record stream, in stream order (block by block, step by step).  count: how many
 * (0 without self-contained ranges); rows: count entries, may be NULL (call twice).  Each coupled row of each
 * self-contained block appears exactly once.                                                                       */
int gmg_get_ssor_backward_rows(gmg_context *ctx, int level, int64_t *count, int32_t *rows);
/* Option ssor_plan_device (gmg_set_option / GMG_OPTIONS, default 0): the plan of a level >= 1 is formed by kernels from the
 * level's CSR as it lies on the device, where the default four-wave plan with one self-contained range per direction in every
 * block applies -- and is then the host builder's plan byte for byte (every array, header word and padding byte).  Where it
 * does not apply (a communicator, the balanced partition, one of the sgs_* diagnostic options, unsorted columns, a row with
 * more than 72 stored entries, a step no shape holds, a block whose live rows exceed the y slots, stream positions beyond
 * 2^31) the WHOLE level is planned by the host builder as without the option; never a mix inside a level.  Both
 * gmg_set_level_matrix and every gmg_assemble_level_matrix* take part; the latter then no longer copy col / val of the level
 * matrix back to the host (except with option debug_upload, for the modelled block costs of its log).  A device-built plan is
 * checked from its own arrays before it is accepted (block table inside the ranges, rows per step, shape keys, header links,
 * LDS addresses below the y slots, aux words and rhs positions inside the stream / the level vector): on a miss the entry
 * returns GMG_ERR_INVALID, the level is left without an operator and no sweep runs on that plan.
 *   gmg_get_ssor_plan_array: one array of a level's four-wave plan as it lies on the device, host-built or device-built.
 *     which: GMG_SSOR_PLAN_*.  out == NULL: *bytes <- the array's size.  Else *bytes is the capacity of out on entry
 *     (GMG_ERR_INVALID if too small) and the size copied on return.  GMG_ERR_INVALID for a level without a four-wave plan.
 *   gmg_get_ssor_plan_origin: who built the level's plan (*on_device 1 / 0), how many bytes of col / val came back to the host
 *     for it (0 for a device-built plan from gmg_assemble_level_matrix*, and for gmg_set_level_matrix, whose caller holds
 *     them), and, where the option was set and the host built it anyway, why -- one fixed text per cause: "communicator",
 *     "balanced partition", "option <key> set" ("option sgs_sliding unset"), "packed schedule", "unsorted columns", "row too wide", "no shape",
 *     "block does not fit", "stream positions beyond 2^31", "empty level"; "" otherwise.  Any pointer may be NULL; the text
 *     is static.                                                                                                          */
#define GMG_SSOR_PLAN_STREAM 0
#define GMG_SSOR_PLAN_RANGES 1
#define GMG_SSOR_PLAN_BLK_TAB 2
#define GMG_SSOR_PLAN_BLOCK_RNG 3
#define GMG_SSOR_PLAN_ROW_CI 4
#define GMG_SSOR_PLAN_CI_ROW 5
#define GMG_SSOR_PLAN_RPOS_F 6
#define GMG_SSOR_PLAN_RPOS_B 7
#define GMG_SSOR_PLAN_ISO_DIAG 8
#define GMG_SSOR_PLAN_ISO_INVD 9
int gmg_get_ssor_plan_array(gmg_context *ctx, int level, int which, int64_t *bytes, void *out);
int gmg_get_ssor_plan_origin(gmg_context *ctx, int level, int *on_device, int64_t *csr_bytes_downloaded, const char **reason);
/* The slot allocator of the self-contained ranges for ONE block [row_begin, row_end) and one direction (backward: 0 / 1) of
 * a level matrix (host CSR, ascending columns, values required: stored zeros do not couple), without a context or a device:
 * the routine the plan uses.  Per row of the block (row_end - row_begin entries each, any may be NULL; -1 for a row without
 * couplings inside the block): the step that updates it, the step of its last reader (a row of this direction that gathers
 * it: c < i forward, c > i backward; at least its own step), its y slot.  A slot changes hands two steps after the last
 * reader at the earliest.  n_steps: steps of the direction; n_slots: slots used = the
 * most ever live (the lowest free slot is always taken).                                                                  */
int gmg_ssor_slot_plan(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t row_begin, int64_t row_end,
                       int backward, int32_t *step, int32_t *last_reader, int32_t *slot, int64_t *n_steps, int64_t *n_slots);
/* Rows scheduled by slack (option sgs_pack).  The stages of a block are walked at most 32 rows at a time, so a
 * stage of 40 rows costs two dependent steps although many of its rows have no reader in the next stage.  The packed levels
 * are a list schedule of the same dependency graph: height(i) = 0 for a row without a higher coupled neighbour, else 1 + the
 * greatest height of its higher neighbours; step t takes at most 32 of the rows whose lower coupled neighbours all lie in
 * steps < t, height descending, then row ascending; level(i) = the row's step.  The forward sweep takes the levels
 * ascending, the backward sweep descending; the results are the same bits as with the stages.
 *   gmg_ssor_pack_levels: the levels of ONE block [row_begin, row_end) of a level matrix (host CSR, ascending columns,
 *     values required), without a context or a device: the routine the plan uses.  level: row_end - row_begin entries, -1
 *     for a row without couplings inside the block (may be NULL); n_levels; n_stage_steps: the steps of a direction when
 *     the stages are walked 32 rows at a time (gmg_ssor_slot_plan's n_steps).
 *   gmg_ssor_slot_plan_packed: gmg_ssor_slot_plan over the packed levels.
 *   gmg_get_ssor_schedule: out = [0] 1 if a block of the level's plan is packed, [1] stages or levels, [2] steps of a sweep
 *     direction (the forward one), [3] the steps the stages need when walked with the plan's rows per step (32; one-wave
 *     plan: 64); [1] .. [3] summed over the blocks.  [2] and [3] compare for the four-wave plan with self-contained ranges,
 *     where [2] < [3] is what packing saved; a ranged or a one-wave plan cuts a step also by the y slots and by the bytes of
 *     its records, so its [2] may exceed [3].  All 0 for a level on the generic CSR sweep.
 * Option sgs_pack: 0 never, 1 always, unset (or < 0) for levels of at least 8192 rows.  Only the four-wave plan with
 * self-contained ranges packs, and only a block whose packed directions both fit the y slots and whose packed steps all have
 * a record shape; such a block otherwise, and every other plan, keeps the stages, exactly as with sgs_pack = 0.  With option
 * ssor_plan_device a level that would be tried is planned by the host ("packed schedule"), whatever the trial gives.      */
int gmg_ssor_pack_levels(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t row_begin, int64_t row_end,
                         int32_t *level, int64_t *n_levels, int64_t *n_stage_steps);
int gmg_ssor_slot_plan_packed(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t row_begin, int64_t row_end,
                              int backward, int32_t *step, int32_t *last_reader, int32_t *slot, int64_t *n_steps, int64_t *n_slots);
int gmg_get_ssor_schedule(gmg_context *ctx, int level, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* GMG_COULOMB_H */
