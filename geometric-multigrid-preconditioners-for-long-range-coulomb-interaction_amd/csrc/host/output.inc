// output.inc -- the graphical output of a cycle (reference: output_results, src/step-50.cc:1149-1308).  Included by
// laplace_problem.cc.  DESIGN.md section 35.
//
// What deal.II does for the reference and is restated here:
//   DataOut::build_patches(0): one patch per active cell with 2^dim vertices, nothing shared between cells; DoF vectors are
//     evaluated at the patch vertices, cell vectors repeated on them; GradientPostprocessor writes grad_phi = -grad phi_h.
//     The patch arrays come from gmg_output_patches(_resident) where the cycle ran on the device, else from the host mirror
//     of the same text (gmg_output.hpp): the same bits either way.
//   write_vtu / write_pvtu_record / write_visit_record: here VTK's documented uncompressed inline-binary form (every
//     DataArray format="binary": a UInt64 byte count and the bytes, encoded in one base64 run), one piece written by rank 0,
//     and no date, host name or timing in the files, so that two runs give identical bytes.
#include <filesystem>

namespace step50 {

namespace output {

// base64 of a UInt64 byte count followed by the bytes, appended to out
inline void append_base64(std::string &out, const void *data, uint64_t n_bytes) {
  static const char tab[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  // n bytes at p to o: whole groups of three, then a padded tail
  auto encode = [](char *o, const unsigned char *p, uint64_t n) {
    uint64_t i = 0;
    for (; i + 3 <= n; i += 3, o += 4) {
      const unsigned w = ((unsigned)p[i] << 16) | ((unsigned)p[i + 1] << 8) | p[i + 2];
      o[0] = tab[w >> 18]; o[1] = tab[(w >> 12) & 63]; o[2] = tab[(w >> 6) & 63]; o[3] = tab[w & 63];
    }
    if (i < n) {
      const bool two = i + 2 == n;
      const unsigned w = ((unsigned)p[i] << 16) | (two ? (unsigned)p[i + 1] << 8 : 0u);
      o[0] = tab[w >> 18]; o[1] = tab[(w >> 12) & 63]; o[2] = two ? tab[(w >> 6) & 63] : '='; o[3] = '=';
    }
  };
  // the count's 8 bytes and the first byte of the data make three whole groups; the rest of the data follows them
  const unsigned char *body = (const unsigned char *)data;
  unsigned char front[9];
  std::memcpy(front, &n_bytes, 8);
  if (n_bytes > 0) front[8] = body[0];
  const size_t o = out.size();
  out.resize(o + (size_t)((8 + n_bytes + 2) / 3 * 4));
  encode(&out[o], front, n_bytes > 0 ? 9 : 8);
  if (n_bytes > 1) encode(&out[o + 12], body + 1, n_bytes - 1);
}

struct Array {  // one DataArray of the piece: the bytes stay with their owner
  std::string type, name;
  int components;
  const void *data;
  uint64_t n_bytes;
};

inline void write_file(const std::string &path, const std::string &text) {
  std::FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("Output results: cannot open " + path);
  const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
  if (std::fclose(f) != 0 || !ok) throw std::runtime_error("Output results: cannot write " + path);
}

inline std::string array_head(const char *tag, const Array &a, bool named) {
  std::string s = std::string("<") + tag + " type=\"" + a.type + "\"";
  if (named) s += " Name=\"" + a.name + "\"";
  if (a.components > 1) s += " NumberOfComponents=\"" + std::to_string(a.components) + "\"";
  return s;
}

}  // namespace output

// Where this cycle's patches are formed; each fallback is said once.
template <int dim>
typename LaplaceProblem<dim>::PatchPath LaplaceProblem<dim>::decide_output_patches() {
  const char *why = !solve_on_device_requested ? "the cycle does not run on the device" : distributed ? "the run is distributed" : nullptr;
  if (why) {
    if (!output_mirror_reported) pcout(std::string("   Output results: patches formed on the host (") + why + ")");
    output_mirror_reported = true;
    return kPatchesMirror;
  }
  if (operators_resident && device_solution() != nullptr) return kPatchesResident;
  if (!output_host_arrays_reported)
    pcout(std::string("   Output results: patches from host arrays (") +
          (!operators_resident ? "Operators from resident tables did not take effect" : "the solution is not on the device") + ")");
  output_host_arrays_reported = true;
  return kPatchesHostArrays;
}

template <int dim>
int LaplaceProblem<dim>::output_patches(PatchPath path, int n_fields, const double *const *dof_field, double *point, double *patch_solution,
                                        double *grad_phi, double *const *patch_field, double *build_ms) {
  constexpr int nv = 1 << dim;
  const int64_t nc = (int64_t)active_cells.size(), n_dofs = (int64_t)vertex_of_dof.size();
  if ((int64_t)solution.size() != n_dofs) { last_error = "output patches: no solution of this mesh"; return GMG_ERR_INVALID; }
  if (n_fields < 0 || n_fields > gmg_output::kMaxFields) { last_error = "output patches: n_fields must be in 0 .. 8"; return GMG_ERR_INVALID; }
  if (build_ms) *build_ms = 0.0;
  if (path != kPatchesMirror) {
    if (ensure_context() != GMG_OK) return GMG_ERR_HIP;
    // (the solution the device kept after gmg_distribute_constraints, "RHS from cell tables"; otherwise a copy of the host's)
    const double *u_dev = device_solution();
    double *d_u = nullptr;
    if (!u_dev && gmg_vec_alloc(gmg, n_dofs, &d_u) != GMG_OK) { last_error = std::string("gmg_vec_alloc: ") + gmg_last_error(gmg); return GMG_ERR_HIP; }
    int rc = u_dev ? GMG_OK : gmg_vec_upload(gmg, d_u, solution.data(), n_dofs);
    if (!u_dev) u_dev = d_u;
    if (rc == GMG_OK && path == kPatchesResident)
      rc = gmg_output_patches_resident(gmg, triangulation.origin, triangulation.h0, u_dev, n_dofs, n_fields, dof_field, point, patch_solution, grad_phi,
                                       patch_field, build_ms);
    else if (rc == GMG_OK) {
      std::vector<uint8_t> level((size_t)nc);
      for (int64_t a = 0; a < nc; ++a) level[(size_t)a] = (uint8_t)std::min(active_cells[(size_t)a].level, 255);
      rc = gmg_output_patches(gmg, dim, nc, active_cell_dof_table.data(), level.data(), vertex_of_dof.data(), n_dofs, triangulation.origin, triangulation.h0,
                              u_dev, n_dofs, n_fields, dof_field, point, patch_solution, grad_phi, patch_field, build_ms);
    }
    if (rc != GMG_OK) last_error = std::string(path == kPatchesResident ? "gmg_output_patches_resident: " : "gmg_output_patches: ") + gmg_last_error(gmg);
    if (d_u) gmg_vec_free(gmg, d_u);
    return rc;
  }
  // host mirror: the same functions (gmg_output.hpp), one cell per iteration; every value has one writer
  const double origin = triangulation.origin, h0 = triangulation.h0, hf = h0 / 4096.0;
  for (int64_t a = 0; a < nc; ++a)
    if (active_cells[(size_t)a].level > gmg_output::kMaxLevel) { last_error = "output patches: cell level above 13"; return GMG_ERR_INVALID; }
#pragma omp parallel for schedule(static)
  for (int64_t a = 0; a < nc; ++a) {
    const int32_t *dofs = &active_cell_dof_table[(size_t)(a * nv)];
    const double h = gmg_output::edge_length(h0, active_cells[(size_t)a].level);
    double U[nv];
    for (int v = 0; v < nv; ++v) U[v] = solution[(size_t)dofs[v]];
    for (int v = 0; v < nv; ++v) {
      const int64_t s = a * nv + v;
      const unsigned long long k = vertex_of_dof[(size_t)dofs[v]];
      if (patch_solution) patch_solution[s] = U[v];
      for (int d = 0; d < 3; ++d) {
        if (point) point[3 * s + d] = d < dim ? gmg_output::coordinate(k, d, origin, hf) : 0.0;
        if (grad_phi) grad_phi[3 * s + d] = d < dim ? gmg_output::field_component(U[v], U[v ^ (1 << (d < dim ? d : 0))], ((v >> d) & 1) != 0, h) : 0.0;
      }
      for (int j = 0; j < n_fields; ++j)
        if (patch_field && patch_field[j]) patch_field[j][s] = dof_field[j][(size_t)dofs[v]];
    }
  }
  return GMG_OK;
}

template <int dim>
void LaplaceProblem<dim>::output_results(unsigned int cycle) {
  write_output_files(cycle, par.output_directory);
}

template <int dim>
void LaplaceProblem<dim>::write_output_files(unsigned int cycle, const std::string &directory) {
  constexpr int nv = 1 << dim;
  static const bool timing = std::getenv("STEP50_TIMING") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  const size_t nc = active_cells.size(), n_dofs = vertex_of_dof.size(), ns = nc * nv;
  if (solution.size() != n_dofs) throw std::runtime_error("Output results: no solution of this mesh");
  if (ns >= ((size_t)1 << 31)) throw std::runtime_error("Output results: more than 2^31 patch vertices");
  output_path = decide_output_patches();
  if (distributed && rank != 0) return;  // rank 0 alone writes, one piece (per-rank pieces do not exist)

  // ---- DoF vectors beyond the solution: evaluated at the DoFs' coordinates here, gathered to the patch vertices with it
  std::vector<std::pair<std::string, std::vector<double>>> dof_vectors;
  auto coordinates = [&]() {
    std::vector<double> x(3 * n_dofs);
    for (size_t i = 0; i < n_dofs; ++i) triangulation.vertex_coords(vertex_of_dof[i], &x[3 * i]);
    return x;
  };
  if (par.flag_analytical_solution && par.Problemtype == "GaussianCharges") {  // :1167-1198
    if (!lammpsinput) {  // Analytical_Solution_without_lammps::value, include/step_50.h:372-376
      const std::vector<double> x = coordinates();
      std::vector<double> f(n_dofs);
      for (size_t i = 0; i < n_dofs; ++i) {
        double sq = 0;
        for (int d = 0; d < dim; ++d) sq += x[3 * i + (size_t)d] * x[3 * i + (size_t)d];
        const double radial_distance = std::sqrt(sq);
        f[i] = (std::erf(2.0 * radial_distance / par.r_c) - std::erf(radial_distance / par.r_c)) / (4.0 * M_PI * radial_distance);
      }
      dof_vectors.emplace_back("Analytical_Solution_without_lammps", std::move(f));
    } else if (number_of_atoms < 10 || (par.analytical_on_device && dim == 3)) {
      const std::vector<double> x = coordinates();
      std::vector<double> f(n_dofs);
      if (dim == 3) {
        if (gaussian_potential(exact_on_device(), (int64_t)n_dofs, x.data(), f.data(), nullptr) != GMG_OK) throw std::runtime_error(last_error);
      } else {  // (gmg_exact.hpp is 3D: the same sum over the atoms in the plane, include/step_50.h:338-353)
        const double inv = 1.0 / (std::sqrt(M_PI) * par.r_c);
        for (size_t i = 0; i < n_dofs; ++i) {
          double v = 0;
          for (unsigned k = 0; k < number_of_atoms; ++k) {
            double r2 = 0;
            for (int d = 0; d < dim; ++d) { const double t = x[3 * i + (size_t)d] - atom_positions[3 * k + (size_t)d]; r2 += t * t; }
            const double r = std::sqrt(r2);
            v += r < 1e-10 ? charges[k] * 2.0 * inv : charges[k] * (std::erf(r / par.r_c) / r);
          }
          f[i] = v;
        }
      }
      dof_vectors.emplace_back("Analytical_Solution_atoms", std::move(f));
    }
  }
  if (par.flag_rhs_field && lammpsinput && number_of_atoms < 10) {  // :1201-1218
    const std::vector<double> x = coordinates();
    std::vector<double> f(n_dofs);
    for (size_t i = 0; i < n_dofs; ++i) f[i] = rhs_function(&x[3 * i]);
    dof_vectors.emplace_back("interpolated_rhs", std::move(f));
  }

  // ---- cell vectors (Float32), repeated on the cell's patch vertices
  std::vector<std::pair<std::string, std::vector<float>>> cell_vectors;
  auto repeated = [&](const std::vector<float> &c) {
    std::vector<float> p(ns);
    for (size_t a = 0; a < nc; ++a)
      for (int v = 0; v < nv; ++v) p[a * nv + (size_t)v] = c[a];
    return p;
  };
  if (par.flag_atoms_support && lammpsinput && par.flag_rhs_assembly) {  // :1230-1262
    if (number_of_atoms > 100) pcout("   Output results: support of each atom skipped (" + std::to_string(number_of_atoms) + " atoms, at most 100 are written)");
    else {
      if (!bins) rhs_assembly_optimization();
      std::vector<std::vector<float>> support(number_of_atoms, std::vector<float>(nc, 0.f));
      std::vector<int32_t> atoms;
      for (size_t a = 0; a < nc; ++a) {  // the list of compute_charge_densities: a function of the root cell alone
        const ActiveCell &ac = active_cells[a];
        const Cell &cell = triangulation.levels[(size_t)ac.level][(size_t)ac.index];
        const int rc[3] = {cell.c[0] >> ac.level, cell.c[1] >> ac.level, cell.c[2] >> ac.level};
        atoms_of_root_cell(rc, atoms);
        for (int32_t i : atoms) support[(size_t)i][a] = 1.f;
      }
      for (unsigned i = 0; i < number_of_atoms; ++i) cell_vectors.emplace_back("support_" + std::to_string(i), repeated(support[i]));
    }
  }
  cell_vectors.emplace_back("subdomain", std::vector<float>(ns, 0.f));  // :1264-1267, one piece
  if (error_per_cell.size() != nc) throw std::runtime_error("Output results: no error indicator of this mesh (the estimator has not run)");
  cell_vectors.emplace_back("error_indicator", repeated(error_per_cell));  // :1269

  // ---- the patches
  if (dof_vectors.size() > (size_t)gmg_output::kMaxFields) throw std::logic_error("Output results: more DoF vectors than a call gathers");
  std::vector<double> point(3 * ns), psol(ns), grad(3 * ns);
  std::vector<std::vector<double>> gathered(dof_vectors.size(), std::vector<double>(ns));
  std::vector<const double *> fin;
  std::vector<double *> fout;
  for (size_t j = 0; j < dof_vectors.size(); ++j) { fin.push_back(dof_vectors[j].second.data()); fout.push_back(gathered[j].data()); }
  double build_ms = 0.0;
  const auto t_patch0 = std::chrono::steady_clock::now();
  if (output_patches(output_path, (int)fin.size(), fin.data(), point.data(), psol.data(), grad.data(), fout.data(), &build_ms) != GMG_OK)
    throw std::runtime_error(last_error);
  const auto t_patch1 = std::chrono::steady_clock::now();

  // ---- connectivity (:1271, build_patches(0) and write_vtu: VTK's vertex order of a hexahedron / quadrilateral)
  static const int order[8] = {0, 1, 3, 2, 4, 5, 7, 6};
  std::vector<int32_t> connectivity(ns), offsets(nc);
  std::vector<uint8_t> types(nc, dim == 3 ? 12 : 9);
  for (size_t a = 0; a < nc; ++a) {
    for (int v = 0; v < nv; ++v) connectivity[a * nv + (size_t)v] = (int32_t)(a * nv) + order[v];
    offsets[a] = (int32_t)((a + 1) * nv);
  }

  // ---- the three files
  std::vector<output::Array> point_data;
  point_data.push_back({"Float64", "solution", 1, psol.data(), sizeof(double) * ns});
  point_data.push_back({"Float64", "grad_phi", 3, grad.data(), sizeof(double) * 3 * ns});
  for (size_t j = 0; j < dof_vectors.size(); ++j) point_data.push_back({"Float64", dof_vectors[j].first, 1, gathered[j].data(), sizeof(double) * ns});
  for (const auto &c : cell_vectors) point_data.push_back({"Float32", c.first, 1, c.second.data(), sizeof(float) * ns});
  const output::Array points{"Float64", "", 3, point.data(), sizeof(double) * 3 * ns};
  const output::Array cells[3] = {{"Int32", "connectivity", 1, connectivity.data(), sizeof(int32_t) * ns},
                                  {"Int32", "offsets", 1, offsets.data(), sizeof(int32_t) * nc},
                                  {"UInt8", "types", 1, types.data(), nc}};
  char number[32];
  std::snprintf(number, sizeof number, "%05u", cycle);
  const std::string stem = std::string("solution-") + number, piece = stem + ".0000.vtu";
  std::error_code ec;
  std::filesystem::create_directories(directory.empty() ? "." : directory, ec);  // (a failure shows when the file is opened)
  const std::string dir = directory.empty() ? std::string(".") : directory;
  const char *vtk_open = " version=\"1.0\" byte_order=\"LittleEndian\" header_type=\"UInt64\">\n";
  std::string text = std::string("<?xml version=\"1.0\"?>\n<VTKFile type=\"UnstructuredGrid\"") + vtk_open + "<UnstructuredGrid>\n<Piece NumberOfPoints=\"" +
                     std::to_string(ns) + "\" NumberOfCells=\"" + std::to_string(nc) + "\">\n";
  auto put = [&](const output::Array &a, bool named) {
    text += output::array_head("DataArray", a, named) + " format=\"binary\">\n";
    output::append_base64(text, a.data, a.n_bytes);
    text += "\n</DataArray>\n";
  };
  text += "<Points>\n";
  put(points, false);
  text += "</Points>\n<Cells>\n";
  for (const auto &a : cells) put(a, true);
  text += "</Cells>\n<PointData Scalars=\"scalars\">\n";
  for (const auto &a : point_data) put(a, true);
  text += "</PointData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n";
  output::write_file(dir + "/" + piece, text);
  const size_t vtu_bytes = text.size();

  text = std::string("<?xml version=\"1.0\"?>\n<VTKFile type=\"PUnstructuredGrid\"") + vtk_open + "<PUnstructuredGrid GhostLevel=\"0\">\n<PPoints>\n" +
         output::array_head("PDataArray", points, false) + "/>\n</PPoints>\n<PPointData Scalars=\"scalars\">\n";
  for (const auto &a : point_data) text += output::array_head("PDataArray", a, true) + "/>\n";
  text += "</PPointData>\n<Piece Source=\"" + piece + "\"/>\n</PUnstructuredGrid>\n</VTKFile>\n";
  output::write_file(dir + "/" + stem + ".pvtu", text);
  output::write_file(dir + "/" + stem + ".visit", "!NBLOCKS 1\n" + piece + "\n");

  if (timing) {
    const auto t_end = std::chrono::steady_clock::now();
    auto sec = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
    std::fprintf(stderr, "[step50] cycle %u %-22s %8.3f s\n", cycle, "output", sec(t_start, t_end));
    if (sublap_on()) {
      static const char *const where[3] = {"host mirror", "gmg_output_patches", "gmg_output_patches_resident"};
      std::fprintf(stderr, "[step50]     . %-32s %8.3f s  (%s, %.3f ms on the device)\n", "output: patches", sec(t_patch0, t_patch1), where[(int)output_path], build_ms);
      std::fprintf(stderr, "[step50]     . %-32s %8.3f s\n", "output: fields before them", sec(t_start, t_patch0));
      std::fprintf(stderr, "[step50]     . %-32s %8.3f s  (%zu bytes in the .vtu)\n", "output: encode + write", sec(t_patch1, t_end), vtu_bytes);
    }
  }
}

}  // namespace step50
