// adaptive.inc -- error estimator, marking, refinement and solution transfer
// (reference: src/step-50.cc:1020-1121).  Included by laplace_problem.cc.
//
// What deal.II does for the reference and is restated here:
//   KellyErrorEstimator<dim>::estimate(..., QGauss<dim-1>(degree+1), ..., cell_diameter)  (:1040-1050)
//     eta_K^2 = h_K * sum over the interior faces F of K of  int_F [d u_h / d n]^2 ,
//     h_K = diameter of K itself (deal.II stores the bare face integrals and multiplies by cell->diameter() when it
//     adds them to a cell); faces with a refined neighbour are integrated sub-face by sub-face from the coarse side,
//     the coarse cell gets their sum and each fine cell behind a sub-face gets that sub-face's integral -- times its
//     OWN diameter (pinned by the cluster logs' cycle 3: with the coarse diameter there, 48 level-1 cells next to the
//     refinement edge end 0.08 % above the threshold and are refined, which the logs do not show); Dirichlet
//     boundary faces contribute nothing.  The per-cell sum over faces (deal.II face order
//     -x,+x,-y,+y,-z,+z) is accumulated in the Vector<float> itself, then sqrt'ed in float.
//   the reference then adds the cell residual  h_K^2 int_K (Laplace u_h + 4 pi rho)^2  (:1055-1082)
//     with the RHS quadrature; Laplace u_h vanishes for Q1 on axis-parallel cells, and rho
//     already contains one factor 4 pi (:522) -- the quirk is kept.
//   threshold = 0.6 * max eta (float), cells with eta >= threshold are refined      (:1084-1089)
//   p4est refine + full 2:1 balance, SolutionTransfer::interpolate, constraints.set_zero (:1095-1121)
namespace step50 {

template <int dim>
void LaplaceProblem<dim>::estimate_error_host() {
  constexpr int nv = 1 << dim;
  constexpr int nfc = 1 << (dim - 1);  // corners of a face
  const size_t nc = active_cells.size();
  // vertex values of the (distributed) solution per active cell
  std::vector<double> cu(nc * nv);
#pragma omp parallel for schedule(static)
  for (int64_t ai = 0; ai < (int64_t)nc; ++ai) {
    const size_t a = (size_t)ai;
    int32_t dofs[nv];
    cell_dofs(active_cells[a], dofs);
    for (int v = 0; v < nv; ++v) cu[a * nv + (size_t)v] = solution[(size_t)dofs[v]];
  }
  // Gauss points on the reference face, tensor order (lower direction fastest)
  std::vector<double> gx, gw;
  gauss01((int)par.degree + 1, gx, gw);
  const int ng = (int)gx.size();
  // normal derivative at the 2^(dim-1) corners of the faces orthogonal to d (same on both sides)
  auto corner_gradients = [&](size_t a, int d, double h, double *out) {
    int k = 0;
    for (int v = 0; v < nv; ++v) {
      if ((v >> d) & 1) continue;
      out[k++] = (cu[a * nv + (size_t)(v | (1 << d))] - cu[a * nv + (size_t)v]) / h;
    }
  };
  // bilinear interpolation of corner values at reference face point (s, t)
  auto face_interp = [&](const double *c, double s, double t) {
    if (dim == 2) return c[0] * (1 - s) + c[1] * s;
    return c[0] * (1 - s) * (1 - t) + c[1] * s * (1 - t) + c[2] * (1 - s) * t + c[3] * s * t;
  };
  // face integrals, booked per (cell, face) so that the float accumulation order is deal.II's.  Every (cell, face) slot
  // has ONE writer (a regular face: its minus-side cell; an irregular one: the coarse cell), so the cells are taken in
  // parallel and the table comes out the same for any thread count.
  std::vector<double> face_int(nc * 2 * dim, 0.0);
  bool unbalanced = false;
#pragma omp parallel for schedule(dynamic, 2048)
  for (int64_t ai = 0; ai < (int64_t)nc; ++ai) {
    const size_t a = (size_t)ai;
    const ActiveCell &ac = active_cells[a];
    const int l = ac.level;
    const Cell &c = triangulation.levels[(size_t)l][(size_t)ac.index];
    const double h = triangulation.cell_size(l);
    const int nl = triangulation.n0 << l;
    for (int d = 0; d < dim; ++d)
      for (int side = 0; side < 2; ++side) {
        int nb[3] = {c.c[0], c.c[1], c.c[2]};
        nb[d] += side ? 1 : -1;
        if (nb[d] < 0 || nb[d] >= nl) continue;  // boundary face, Dirichlet: no contribution
        const int32_t N = triangulation.find(l, nb[0], nb[1], nb[2]);
        if (N < 0) continue;  // coarser neighbour: integrated from its side
        double gc[nfc];
        corner_gradients(a, d, h, gc);
        if (triangulation.active(l, N)) {
          if (side == 0) continue;  // each regular face once, from its minus-side cell
          const size_t b = (size_t)active_index_of_cell[(size_t)l][(size_t)N];
          double gn[nfc];
          corner_gradients(b, d, h, gn);
          double jump[nfc];
          for (int k = 0; k < nfc; ++k) jump[k] = gn[k] - gc[k];
          double s = 0;
          for (int q1 = 0; q1 < (dim == 3 ? ng : 1); ++q1)
            for (int q0 = 0; q0 < ng; ++q0) {
              const double j = face_interp(jump, gx[(size_t)q0], dim == 3 ? gx[(size_t)q1] : 0.0);
              s += j * j * gw[(size_t)q0] * (dim == 3 ? gw[(size_t)q1] : 1.0) * std::pow(h, dim - 1);
            }
          // Strategy::cell_diameter: the factor h_K (no 1/24; pinned by the golden thresholds) is applied per cell below
          face_int[a * 2 * dim + (size_t)(2 * d + 1)] = s;
          face_int[b * 2 * dim + (size_t)(2 * d)] = s;
        } else {
          // irregular face: this cell is the coarse one; children of N touching the face
          const Cell &nc_ = triangulation.levels[(size_t)l][(size_t)N];
          const double hf = 0.5 * h;
          double sum = 0;
          for (int ch = 0; ch < nv; ++ch) {
            if (((ch >> d) & 1) != (side ? 0 : 1)) continue;
            const int32_t fc = nc_.first_child + ch;
            const int32_t fa = active_index_of_cell[(size_t)l + 1][(size_t)fc];
            if (fa < 0) {  // (reported after the loop: no exception leaves a parallel region)
#pragma omp atomic write
              unbalanced = true;
              continue;
            }
            double gf[nfc];
            corner_gradients((size_t)fa, d, hf, gf);
            // quadrant of the coarse face occupied by this child (in-face directions, ascending)
            int quad[2] = {0, 0}, k = 0;
            for (int e = 0; e < dim; ++e)
              if (e != d) quad[k++] = (ch >> e) & 1;
            double s = 0;
            for (int q1 = 0; q1 < (dim == 3 ? ng : 1); ++q1)
              for (int q0 = 0; q0 < ng; ++q0) {
                const double s0 = gx[(size_t)q0], t0 = dim == 3 ? gx[(size_t)q1] : 0.0;
                const double jf = face_interp(gf, s0, t0);
                const double jc = face_interp(gc, 0.5 * (quad[0] + s0), dim == 3 ? 0.5 * (quad[1] + t0) : 0.0);
                const double j = side ? jf - jc : jc - jf;
                s += j * j * gw[(size_t)q0] * (dim == 3 ? gw[(size_t)q1] : 1.0) * std::pow(hf, dim - 1);
              }
            face_int[(size_t)fa * 2 * dim + (size_t)(2 * d + (side ? 0 : 1))] = s;
            sum += s;
          }
          face_int[a * 2 * dim + (size_t)(2 * d + side)] = sum;
        }
      }
  }
  if (unbalanced) throw std::logic_error("mesh not 2:1 balanced across a face");
  std::vector<float> estimated_error_per_cell(nc, 0.f);
  estimator_kelly_sq.assign(nc, 0.0);
  estimator_residual_sq.assign(nc, 0.0);
#pragma omp parallel for schedule(static)
  for (int64_t ai = 0; ai < (int64_t)nc; ++ai) {
    const size_t a = (size_t)ai;
    const double diam_a = triangulation.cell_size(active_cells[a].level) * std::sqrt((double)dim);
    float acc = 0.f;
    for (int f = 0; f < 2 * dim; ++f) acc += (float)(diam_a * face_int[a * 2 * dim + (size_t)f]);  // Vector<float> +=
    estimated_error_per_cell[a] = std::sqrt(acc);
    estimator_kelly_sq[a] = (double)acc;
  }
  // residual term (:1055-1082)
  const Quadrature<dim> q_rhs((int)(par.degree + par.quadrature_degree_rhs));
  if (par.refinement_estimator != "Kelly") ensure_host_densities();  // (device-resident densities come over only for HEAD's residual term)
  // the Kelly-only rule does not use the residual term: with the densities left on the device it is not formed at all
  // (estimator_residual_sq stays 0; tools/marking_rule_scan.py runs with "RHS on device = false")
  const bool have_dens = !lammpsinput || density_values_for_each_cell.size() == nc;
  for (size_t a = 0; a < nc && have_dens; ++a) {
    const ActiveCell &ac = active_cells[a];
    const Cell &c = triangulation.levels[(size_t)ac.level][(size_t)ac.index];
    const double h = triangulation.cell_size(ac.level);
    const double jxw = std::pow(h, dim);
    double x0[3];
    triangulation.cell_origin(ac.level, c, x0);
    double error = 0;
    for (size_t q = 0; q < q_rhs.p.size(); ++q) {
      double dens;
      if (lammpsinput) dens = density_values_for_each_cell[a][q];
      else {
        double x[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) x[d] = x0[d] + h * q_rhs.p[q][(size_t)d];
        dens = rhs_function(x);
      }
      const double temp = 0.0 + 4.0 * M_PI * dens;  // fe_solution_laplacians == 0 for Q1
      error += temp * temp * q_rhs.w[q] * jxw;
    }
    const double diam = h * std::sqrt((double)dim);
    const double e = (double)estimated_error_per_cell[a];
    estimator_residual_sq[a] = diam * diam * error;
    if (par.refinement_estimator == "Kelly") continue;  // the indicator of the revision behind the cluster logs
    estimated_error_per_cell[a] = (float)std::sqrt(e * e + diam * diam * error);
  }
  float mx = 0.f;
  for (float v : estimated_error_per_cell) mx = std::max(mx, std::fabs(v));
  if (std::getenv("STEP50_DEBUG_ESTIMATOR"))
    for (size_t a = 0; a < nc; ++a)
      if (estimated_error_per_cell[a] == mx) {
        const double diam_a = triangulation.cell_size(active_cells[a].level) * std::sqrt((double)dim);
        float acc = 0.f;
        for (int f = 0; f < 2 * dim; ++f) acc += (float)(diam_a * face_int[a * 2 * dim + (size_t)f]);
        std::fprintf(stderr, "max cell %zu level %d: kelly^2 %.10e total %.10e\n", a, active_cells[a].level, (double)acc, (double)mx);
        for (int f = 0; f < 2 * dim; ++f) std::fprintf(stderr, "   face %d: %.10e\n", f, face_int[a * 2 * dim + (size_t)f]);
        break;
      }
  const double threshold = 0.6 * mx;
  reports.back().refine_threshold = threshold;
  pcout("Threshold value for refinement:\t" + fmt("%.10e", threshold));
  error_per_cell = estimated_error_per_cell;
  face_integrals.swap(face_int);
  estimated_on_device = false;
  estimator_resident = marks_resident = false;  // (marks the context may still hold are not these)
  refine_flags.assign(triangulation.levels.size(), {});
  for (size_t l = 0; l < triangulation.levels.size(); ++l) refine_flags[l].assign(triangulation.levels[l].size(), 0);
  for (size_t a = 0; a < nc; ++a)
    if ((double)std::fabs(estimated_error_per_cell[a]) >= threshold)
      refine_flags[(size_t)active_cells[a].level][(size_t)active_cells[a].index] = 1;
}

// ---- "Error estimator on device" (DESIGN.md section 14): the same estimate through gmg_estimate_error

// Every (cell, face) slot by kind, as include/gmg_coulomb.h defines them: 0 boundary, 1 active neighbour of the same level,
// 2 neighbour refined once (its children on the face by quadrant), 3 neighbour one level coarser (its index, this cell's
// quadrant of the coarse face).
template <int dim>
void LaplaceProblem<dim>::face_table(std::vector<uint8_t> &face_kind, std::vector<int32_t> &face_cell) const {
  constexpr int nv = 1 << dim;
  constexpr int nfc = 1 << (dim - 1);
  const size_t nc = active_cells.size();
  face_kind.assign(nc * 2 * dim, 0);
  face_cell.assign(nc * 2 * dim * nfc, 0);
  bool unbalanced = false;
#pragma omp parallel for schedule(static)
  for (int64_t ai = 0; ai < (int64_t)nc; ++ai) {
    const size_t a = (size_t)ai;
    const int l = active_cells[a].level;
    const Cell &c = triangulation.levels[(size_t)l][(size_t)active_cells[a].index];
    const int nl = triangulation.n0 << l;
    for (int d = 0; d < dim; ++d)
      for (int side = 0; side < 2; ++side) {
        const size_t slot = a * 2 * dim + (size_t)(2 * d + side);
        int nb[3] = {c.c[0], c.c[1], c.c[2]};
        nb[d] += side ? 1 : -1;
        if (nb[d] < 0 || nb[d] >= nl) continue;  // boundary face
        const int32_t N = triangulation.find(l, nb[0], nb[1], nb[2]);
        int32_t bad = 0;
        if (N < 0) {
          // coarser neighbour; this cell's quadrant of its face from the in-face bits of the cell's own position
          const int32_t P = l > 0 ? triangulation.find(l - 1, nb[0] >> 1, nb[1] >> 1, dim == 3 ? nb[2] >> 1 : 0) : -1;
          const int32_t pa = P >= 0 ? active_index_of_cell[(size_t)l - 1][(size_t)P] : -1;
          int quad = 0, k = 0;
          for (int e = 0; e < dim; ++e)
            if (e != d) quad |= (c.c[e] & 1) << k++;
          face_kind[slot] = 3;
          face_cell[slot * nfc] = pa;
          face_cell[slot * nfc + 1] = quad;
          bad = pa < 0;
        } else if (triangulation.active(l, N)) {
          face_kind[slot] = 1;
          face_cell[slot * nfc] = active_index_of_cell[(size_t)l][(size_t)N];
        } else {
          const Cell &nc_ = triangulation.levels[(size_t)l][(size_t)N];
          face_kind[slot] = 2;
          int k = 0;
          for (int ch = 0; ch < nv; ++ch) {
            if (((ch >> d) & 1) != (side ? 0 : 1)) continue;
            const int32_t fa = active_index_of_cell[(size_t)l + 1][(size_t)(nc_.first_child + ch)];
            face_cell[slot * nfc + (size_t)k++] = fa;
            bad |= fa < 0;
          }
        }
        if (bad) {  // (reported after the loop: no exception leaves a parallel region)
#pragma omp atomic write
          unbalanced = true;
        }
      }
  }
  if (unbalanced) throw std::logic_error("mesh not 2:1 balanced across a face");
}

template <int dim>
typename LaplaceProblem<dim>::EstimatorInputs LaplaceProblem<dim>::estimator_inputs(bool mesh_arrays) {
  EstimatorInputs in;
  const size_t nc = active_cells.size();
  if (mesh_arrays) {  // (otherwise the context's tables and its face table stand for them, DESIGN.md section 24)
    in.cell_dofs = active_cell_dof_table;
    in.cell_level.resize(nc);
    for (size_t a = 0; a < nc; ++a) {
      if (active_cells[a].level > 15) throw std::runtime_error("Error estimator on device: more than 16 levels");
      in.cell_level[a] = (uint8_t)active_cells[a].level;
    }
    if (decide_refinement_on_device()) face_table_on_device(in.face_kind, in.face_cell);
    else face_table(in.face_kind, in.face_cell);
  }
  // the per-level factors exactly as the host loop forms them
  for (int l = 0; l < 16; ++l) {
    const double h = triangulation.cell_size(l);
    in.h_of_level.push_back(h);
    in.face_measure_of_level.push_back(std::pow(h, dim - 1));
    in.diameter_of_level.push_back(h * std::sqrt((double)dim));
    in.jxw_of_level.push_back(std::pow(h, dim));
  }
  gauss01((int)par.degree + 1, in.gauss_x, in.gauss_w);
  const Quadrature<dim> q_rhs((int)(par.degree + par.quadrature_degree_rhs));
  in.nq = (int)q_rhs.p.size();
  in.weight = q_rhs.w;
  const bool kelly_only = par.refinement_estimator == "Kelly";
  // HEAD's rule takes the densities where they are; the Kelly rule forms the residual term only from densities the host
  // has anyway (estimate_error_host: with the densities left on the device it is not formed at all)
  if (!kelly_only && lammpsinput && densities_device_resident) {
    in.residual = 1;
    in.dens_resident = true;
    return in;
  }
  if (lammpsinput && density_values_for_each_cell.size() != nc) return in;  // residual 0
  in.residual = kelly_only ? 2 : 1;
  in.dens.resize(nc * (size_t)in.nq);
#pragma omp parallel for schedule(static)
  for (int64_t ai = 0; ai < (int64_t)nc; ++ai) {
    const size_t a = (size_t)ai;
    if (lammpsinput) {
      std::copy(density_values_for_each_cell[a].begin(), density_values_for_each_cell[a].end(), in.dens.begin() + (std::ptrdiff_t)(a * (size_t)in.nq));
      continue;
    }
    const ActiveCell &ac = active_cells[a];
    const double h = triangulation.cell_size(ac.level);
    double x0[3];
    triangulation.cell_origin(ac.level, triangulation.levels[(size_t)ac.level][(size_t)ac.index], x0);
    for (size_t q = 0; q < q_rhs.p.size(); ++q) {
      double x[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d) x[d] = x0[d] + h * q_rhs.p[q][(size_t)d];
      in.dens[a * (size_t)in.nq + q] = rhs_function(x);
    }
  }
  return in;
}

// Is this cycle's estimate one gmg_estimate_error forms?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_estimator_on_device() {
  if (!par.estimator_on_device) return false;
  const char *why = !solve_on_device_requested ? "the cycle does not run on the device" : distributed ? "the run is distributed" : nullptr;
  if (!why) return true;
  if (!estimator_fallback_reported) pcout(std::string("   Error estimator on device: not applicable (") + why + "), estimated on the host");
  estimator_fallback_reported = true;
  return false;
}

// Does this cycle's estimate read the context's mesh tables?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_estimator_resident() {
  if (!par.estimator_from_resident_tables) return false;
  const char *why = distributed                  ? "the run is distributed"
                    : !operators_resident        ? "Operators from resident tables did not take effect"
                    : !par.estimator_on_device   ? "Error estimator on device is not set"
                    : !par.refinement_on_device  ? "Refinement on device is not set"
                                                 : nullptr;
  if (!why) return true;
  if (!estimator_resident_fallback_reported) pcout(std::string("   Estimator from resident tables: not applicable (") + why + "), host arrays");
  estimator_resident_fallback_reported = true;
  return false;
}

// Do this cycle's energy and forces read the context's mesh tables?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_energy_forces_resident() {
  if (!par.energy_forces_from_resident_tables) return false;
  const char *why = distributed                    ? "the run is distributed"
                    : !operators_resident          ? "Operators from resident tables did not take effect"
                    : device_solution() == nullptr ? "the solution is not on the device"
                    : (dim != 3 || !lammpsinput)   ? "not a 3D problem with LAMMPS input"
                                                   : nullptr;
  if (!why) return true;
  if (!energy_forces_fallback_reported) pcout(std::string("   Energy and forces from resident tables: not applicable (") + why + "), host arrays");
  energy_forces_fallback_reported = true;
  return false;
}

// gmg_build_point_locator_resident, once per mesh: the context drops the locator with the tables it belongs to, so a kept one
// with this forest's number of cells is this mesh's.  STEP50_CHECK_RESIDENT=1 holds it against point_locator().
template <int dim>
void LaplaceProblem<dim>::ensure_point_locator_resident() {
  if (ensure_context() != GMG_OK) throw std::runtime_error("Energy and forces from resident tables: context: " + last_error);
  int64_t n_all = 0, n_nodes = -1;
  for (const auto &lv : triangulation.levels) n_all += (int64_t)lv.size();
  if (gmg_get_point_locator(gmg, &n_nodes, nullptr) == GMG_OK && n_nodes == n_all) return;
  const ForestCells fc = forest_cells();
  double build_ms = 0.0;
  sublap(nullptr);
  if (gmg_build_point_locator_resident(gmg, dim, fc.n0, triangulation.n_levels(), fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), &n_nodes,
                                       &build_ms) != GMG_OK)
    throw std::logic_error(gmg_last_error(gmg));
  sublap("point locator on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
  const char *check = std::getenv("STEP50_CHECK_RESIDENT");
  if (!check || std::atoi(check) == 0) return;
  std::vector<int32_t> h_node, d_node;
  point_locator(h_node);
  d_node.assign(h_node.size(), 0);
  if (n_nodes != (int64_t)h_node.size()) throw std::logic_error("Energy and forces from resident tables: the forests differ in size");
  if (gmg_get_point_locator(gmg, &n_nodes, d_node.data()) != GMG_OK) throw std::runtime_error(std::string("gmg_get_point_locator: ") + gmg_last_error(gmg));
  if (d_node != h_node) throw std::logic_error("Energy and forces from resident tables: the device's point locator differs from the host's");
}

// gmg_build_face_table_resident: the face table stays in the context.  STEP50_CHECK_RESIDENT=1 holds it against face_table().
template <int dim>
void LaplaceProblem<dim>::face_table_resident() {
  if (ensure_context() != GMG_OK) throw std::runtime_error("Estimator from resident tables: context: " + last_error);
  const ForestCells fc = forest_cells();
  const size_t nc = active_cells.size();
  int64_t n_active = 0;
  double build_ms = 0.0;
  sublap(nullptr);
  if (gmg_build_face_table_resident(gmg, dim, fc.n0, triangulation.n_levels(), fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), &n_active,
                                    &build_ms) != GMG_OK)
    throw std::logic_error(gmg_last_error(gmg));
  if (n_active != (int64_t)nc) throw std::logic_error("Estimator from resident tables: the active cell lists differ");
  sublap("estimate: face table on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
  const char *check = std::getenv("STEP50_CHECK_RESIDENT");
  if (!check || std::atoi(check) == 0) return;
  std::vector<uint8_t> h_kind, d_kind;
  std::vector<int32_t> h_cell, d_cell;
  face_table(h_kind, h_cell);
  d_kind.assign(h_kind.size(), 0);
  d_cell.assign(h_cell.size(), 0);
  if (gmg_get_face_table(gmg, &n_active, d_kind.data(), d_cell.data()) != GMG_OK) throw std::runtime_error(std::string("gmg_get_face_table: ") + gmg_last_error(gmg));
  if (n_active != (int64_t)nc || d_kind != h_kind || d_cell != h_cell) throw std::logic_error("Estimator from resident tables: the device's face table differs from the host's");
}

template <int dim>
int LaplaceProblem<dim>::estimate_error_device() {
  if (solution.size() != vertex_of_dof.size()) { last_error = "error estimator: no solution of this mesh"; return GMG_ERR_INVALID; }
  const size_t nc = active_cells.size();
  estimator_resident = decide_estimator_resident();
  marks_resident = false;
  sublap(nullptr);
  const EstimatorInputs in = estimator_inputs(!estimator_resident);
  if (estimator_resident) face_table_resident();
  sublap("estimate: face table, inputs");
  if (ensure_context() != GMG_OK) return GMG_ERR_HIP;
  // (the solution the device kept after gmg_distribute_constraints, "RHS from cell tables"; otherwise a copy of the host's)
  const double *u_dev = device_solution();
  double *d_u = nullptr;
  if (!u_dev && gmg_vec_alloc(gmg, (int64_t)solution.size(), &d_u) != GMG_OK) { last_error = std::string("gmg_vec_alloc: ") + gmg_last_error(gmg); return GMG_ERR_HIP; }
  std::vector<float> eta(nc, 0.f);
  std::vector<double> kelly(nc, 0.0), res(nc, 0.0), fi(nc * 2 * dim, 0.0);
  std::vector<uint8_t> mark(nc, 0);
  double threshold = 0.0, build_ms = 0.0;
  int64_t n_marked = 0;
  int rc = u_dev ? GMG_OK : gmg_vec_upload(gmg, d_u, solution.data(), (int64_t)solution.size());
  if (!u_dev) u_dev = d_u;
  sublap("estimate: upload of u");
  if (rc == GMG_OK && estimator_resident)  // DESIGN.md section 24: the cell tables and the face table are the context's; the marks stay there too
    rc = gmg_estimate_error_resident(gmg, in.h_of_level.data(), in.face_measure_of_level.data(), in.diameter_of_level.data(), (int)in.gauss_x.size(),
                                     in.gauss_x.data(), in.gauss_w.data(), u_dev, (int64_t)solution.size(), in.residual, in.nq, in.weight.data(),
                                     in.jxw_of_level.data(), in.dens_resident || in.dens.empty() ? nullptr : in.dens.data(), in.fraction, eta.data(),
                                     kelly.data(), res.data(), fi.data(), &threshold, mark.data(), &n_marked, &build_ms);
  else if (rc == GMG_OK)
    rc = gmg_estimate_error(gmg, dim, (int64_t)nc, in.cell_dofs.data(), in.cell_level.data(), in.face_kind.data(), in.face_cell.data(),
                            in.h_of_level.data(), in.face_measure_of_level.data(), in.diameter_of_level.data(), (int)in.gauss_x.size(),
                            in.gauss_x.data(), in.gauss_w.data(), u_dev, (int64_t)solution.size(), in.residual, in.nq, in.weight.data(),
                            in.jxw_of_level.data(), in.dens_resident || in.dens.empty() ? nullptr : in.dens.data(), in.fraction, eta.data(),
                            kelly.data(), res.data(), fi.data(), &threshold, mark.data(), &n_marked, &build_ms);
  if (rc != GMG_OK) last_error = std::string(estimator_resident ? "gmg_estimate_error_resident: " : "gmg_estimate_error: ") + gmg_last_error(gmg);
  if (d_u) gmg_vec_free(gmg, d_u);
  if (rc != GMG_OK) return rc;
  sublap("estimate: on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
  error_per_cell.swap(eta);
  estimator_kelly_sq.swap(kelly);
  estimator_residual_sq.swap(res);
  face_integrals.swap(fi);
  estimated_on_device = true;
  reports.back().refine_threshold = threshold;
  pcout("Threshold value for refinement:\t" + fmt("%.10e", threshold));
  refine_flags.assign(triangulation.levels.size(), {});
  for (size_t l = 0; l < triangulation.levels.size(); ++l) refine_flags[l].assign(triangulation.levels[l].size(), 0);
  for (size_t a = 0; a < nc; ++a)
    if (mark[a]) refine_flags[(size_t)active_cells[a].level][(size_t)active_cells[a].index] = 1;
  marks_resident = estimator_resident;
  sublap("estimate: marks");
  return GMG_OK;
}

template <int dim>
void LaplaceProblem<dim>::estimate_error_and_mark_cells() {
  if (decide_estimator_on_device()) {
    if (estimate_error_device() != GMG_OK) throw std::runtime_error(last_error);
  } else {
    (void)decide_estimator_resident();  // (says why the key has no effect here; estimate_error_host clears the rest)
    estimate_error_host();
  }
}

template <int dim>
void LaplaceProblem<dim>::refine_grid(unsigned int cycle) {
  constexpr int nv = 1 << dim;
  if (refine_flags.empty()) throw std::runtime_error("refine_grid: no cells were marked (run the estimator first)");
  refined_on_device = decide_refinement_on_device();
  if (refined_on_device) { refine_grid_on_device(cycle); return; }
  // values of the previous (distributed) solution by vertex
  FlatMap<double> value_of_vertex;
  value_of_vertex.reserve(vertex_of_dof.size() * 2);
  sublap(nullptr);
  for (size_t i = 0; i < vertex_of_dof.size(); ++i) value_of_vertex.emplace(vertex_of_dof[i], solution[i]);
  sublap("refine: values by vertex");
  // (a mark counts only on an active cell: refine_flagged skips the others, the record of the closure leaves them out)
  for (size_t l = 0; l < refine_flags.size() && l < triangulation.levels.size(); ++l)
    for (size_t c = 0; c < refine_flags[l].size() && c < triangulation.levels[l].size(); ++c)
      if (triangulation.levels[l][c].first_child >= 0) refine_flags[l][c] = 0;
  triangulation.refine_flagged(refine_flags);
  closed_refine_flags.clear();
  for (const auto &lv : refine_flags) closed_refine_flags.insert(closed_refine_flags.end(), lv.begin(), lv.end());
  refine_flags.clear();
  sublap("refine: refine_flagged");
  setup_system(cycle);
  // SolutionTransfer::interpolate: new vertices take the Q1 interpolant of their parent cell
  for (int l = 1; l < triangulation.n_levels(); ++l)
    for (const Cell &cell : triangulation.levels[(size_t)l]) {
      bool missing = false;
      for (int a = 0; a < nv && !missing; ++a) missing = !value_of_vertex.count(triangulation.vertex_key(l, cell, a));
      if (!missing) continue;
      const Cell &parent = triangulation.levels[(size_t)l - 1][(size_t)cell.parent];
      double pv[nv];
      for (int p = 0; p < nv; ++p) pv[p] = value_of_vertex.at(triangulation.vertex_key(l - 1, parent, p));
      const int child = (cell.c[0] & 1) | ((cell.c[1] & 1) << 1) | (dim == 3 ? (cell.c[2] & 1) << 2 : 0);
      for (int a = 0; a < nv; ++a) {
        const uint64_t key = triangulation.vertex_key(l, cell, a);
        if (value_of_vertex.count(key)) continue;
        double v = 0;
        for (int p = 0; p < nv; ++p) {
          double w = 1;
          for (int d = 0; d < dim; ++d) {
            const double pos = 0.5 * (((child >> d) & 1) + ((a >> d) & 1));
            w *= ((p >> d) & 1) ? pos : 1.0 - pos;
          }
          v += w * pv[p];
        }
        value_of_vertex.emplace(key, v);
      }
    }
  solution.assign(vertex_of_dof.size(), 0.0);
  solution_on_device = false;
  for (size_t i = 0; i < vertex_of_dof.size(); ++i) solution[i] = value_of_vertex.at(vertex_of_dof[i]);
  set_zero_constraints(solution);  // :1119
  initial_guess = solution;
  sublap("refine: interpolate");
}

// ---- "Refinement on device" (DESIGN.md section 21)

// Is this cycle one whose refinement, transfer and face table the device forms?  Says so once when the key asks for it in vain.
template <int dim>
bool LaplaceProblem<dim>::decide_refinement_on_device() {
  if (!par.refinement_on_device) return false;
  const char *why = !solve_on_device_requested ? "the cycle does not run on the device" : distributed ? "the run is distributed" : nullptr;
  if (!why) return true;
  if (!refinement_fallback_reported) pcout(std::string("   Refinement on device: not applicable (") + why + "), refined on the host");
  refinement_fallback_reported = true;
  return false;
}

template <int dim>
void LaplaceProblem<dim>::face_table_on_device(std::vector<uint8_t> &face_kind, std::vector<int32_t> &face_cell) {
  constexpr int nfc = 1 << (dim - 1);
  if (ensure_context() != GMG_OK) throw std::runtime_error("Refinement on device: context: " + last_error);
  const ForestCells fc = forest_cells();
  const size_t nc = active_cells.size();
  face_kind.assign(nc * 2 * dim, 0);
  face_cell.assign(nc * 2 * dim * nfc, 0);
  int64_t n_active = 0;
  double build_ms = 0.0;
  sublap(nullptr);
  if (gmg_build_face_table(gmg, dim, fc.n0, triangulation.n_levels(), fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), &n_active,
                           face_kind.data(), face_cell.data(), &build_ms) != GMG_OK)
    throw std::logic_error(gmg_last_error(gmg));
  if (n_active != (int64_t)nc) throw std::logic_error("Refinement on device: the active cell lists differ");
  sublap("estimate: face table on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", build_ms);
}

// refine_grid through gmg_refine_forest and gmg_transfer_solution: the marks go up with the forest, the new forest comes back
// into `triangulation` (Forest::install), setup_system runs as before, and the old solution -- the vector the device kept
// where "RHS from cell tables" left one, otherwise an upload -- is carried over on the device and downloaded once.
template <int dim>
void LaplaceProblem<dim>::refine_grid_on_device(unsigned int cycle) {
  auto chk = [&](int rc, const char *what) {
    if (rc != GMG_OK) throw std::runtime_error(std::string("Refinement on device: ") + what + ": " + (gmg ? gmg_last_error(gmg) : last_error.c_str()));
  };
  chk(ensure_context(), "context");
  sublap(nullptr);
  ForestCells fc = forest_cells();
  // "Estimator from resident tables" (DESIGN.md section 24): the marks of the last estimate lie in the context and the flags are
  // formed from them there.  STEP50_CHECK_RESIDENT=1: the marks come back once more, the flags are formed here as below and go
  // through gmg_refine_forest first; the closed flags of both refinements must agree.
  int64_t n_held = -1;
  const bool marked = marks_resident && estimator_resident_applies() && gmg_get_marks(gmg, &n_held, nullptr, nullptr) == GMG_OK && n_held == (int64_t)active_cells.size();
  const char *check = std::getenv("STEP50_CHECK_RESIDENT");
  const bool hold = marked && check && std::atoi(check) != 0;
  std::vector<uint8_t> flag, held_closed;
  if (hold) {
    std::vector<uint8_t> mark(active_cells.size(), 0);
    int64_t n_marks = 0;
    chk(gmg_get_marks(gmg, &n_marks, mark.data(), nullptr), "gmg_get_marks");
    if (n_marks != (int64_t)active_cells.size()) throw std::logic_error("Estimator from resident tables: the marks are not this mesh's");
    refine_flags.assign(triangulation.levels.size(), {});
    for (size_t l = 0; l < triangulation.levels.size(); ++l) refine_flags[l].assign(triangulation.levels[l].size(), 0);
    for (size_t a = 0; a < active_cells.size(); ++a)
      if (mark[a]) refine_flags[(size_t)active_cells[a].level][(size_t)active_cells[a].index] = 1;
  }
  if (!marked || hold) {
    flag.reserve(fc.cell_first_child.size());
    for (const auto &lv : refine_flags)
      for (char f : lv) flag.push_back((uint8_t)(f != 0));
    flag.resize(fc.cell_first_child.size(), 0);
  }
  int L = 0;
  int64_t n_cells = 0, n_flags = 0, n_split = 0;
  double refine_ms = 0.0, transfer_ms = 0.0;
  if (!marked || hold)
    chk(gmg_refine_forest(gmg, dim, fc.n0, triangulation.n_levels(), fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), flag.data(), &L, &n_cells,
                          &n_split, &refine_ms),
        "gmg_refine_forest");
  if (hold) {
    held_closed.assign(flag.size(), 0);
    chk(gmg_get_refined_forest(gmg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, held_closed.data()), "download");
  }
  if (marked)
    chk(gmg_refine_forest_marked(gmg, dim, fc.n0, triangulation.n_levels(), fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), &L, &n_cells,
                                 &n_split, &refine_ms),
        "gmg_refine_forest_marked");
  marks_resident = false;
  std::vector<int32_t> parent((size_t)n_cells);
  const size_t n_old_cells = fc.cell_first_child.size();
  fc.level_ptr.assign((size_t)L + 1, 0);
  fc.cell_coord.resize((size_t)n_cells * 3);
  fc.cell_first_child.resize((size_t)n_cells);
  closed_refine_flags.assign(n_old_cells, 0);
  chk(gmg_get_refined_forest(gmg, nullptr, nullptr, &n_flags, nullptr, fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), parent.data(),
                             closed_refine_flags.data()),
      "download");
  if (hold && closed_refine_flags != held_closed) throw std::logic_error("Estimator from resident tables: the flags formed from the marks on the device differ from the host's");
  triangulation.install(L, fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), parent.data());
  refine_flags.clear();
  sublap("refine: forest on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", refine_ms);
  // the old solution by vertex: setup_system replaces both containers and leaves d_full alone
  const std::vector<uint64_t> old_vertex = std::move(vertex_of_dof);
  const std::vector<double> old_solution = std::move(solution);
  const double *u_old = device_solution();
  setup_system(cycle);
  const int64_t n_old = (int64_t)old_vertex.size(), n_new = (int64_t)vertex_of_dof.size();
  double *d_old = nullptr, *d_new = nullptr;
  int rc = gmg_vec_alloc(gmg, n_new, &d_new);
  if (rc == GMG_OK && !u_old) {
    rc = gmg_vec_alloc(gmg, n_old, &d_old);
    if (rc == GMG_OK) rc = gmg_vec_upload(gmg, d_old, old_solution.data(), n_old);
    u_old = d_old;
  }
  if (rc == GMG_OK)
    rc = gmg_transfer_solution(gmg, dim, fc.n0, L, fc.level_ptr.data(), fc.cell_coord.data(), fc.cell_first_child.data(), n_old, old_vertex.data(), u_old, n_new,
                               vertex_of_dof.data(), constraint_of_dof.data(), d_new, &transfer_ms);
  solution.assign((size_t)n_new, 0.0);
  solution_on_device = false;
  if (rc == GMG_OK) rc = gmg_vec_download(gmg, solution.data(), d_new, n_new);
  const std::string why = rc != GMG_OK ? gmg_last_error(gmg) : "";
  if (d_old) gmg_vec_free(gmg, d_old);
  if (d_new) gmg_vec_free(gmg, d_new);
  if (rc != GMG_OK) throw std::runtime_error("Refinement on device: gmg_transfer_solution: " + why);
  initial_guess = solution;
  sublap("refine: transfer on device");
  if (sublap_on()) std::fprintf(stderr, "[step50]     . %-32s %8.3f ms\n", "  of it on the device (build_ms)", transfer_ms);
}

}  // namespace step50
