// gmg_coulomb.hip -- implementation of the C-ABI in include/gmg_coulomb.h for MI355X (gfx950).
//
// Host-side orchestration of the kernels in gmg_device.hpp: operator upload (tiling for the
// LDS row-window SpMV, explicit transposes, inverse diagonals, SGS level schedule), the
// V-cycle of deal.II's Multigrid::level_v_step, the device-resident coarse CG, and the
// vector_t primitives the host-side outer CG calls.  Reference call sites are cited in the
// header next to each entry point; operation order follows /root/reference/src/step-50.cc
// :938-1017 as restated in SURVEY.md 3.2.
#include "../../include/gmg_coulomb.h"
#include "gmg_device.hpp"
#include "gmg_sgs_layout.hpp"
#include "gmg_sgs.hpp"
#include "gmg_sgs_phase.hpp"
#include "gmg_sgs_dep.hpp"
#include "gmg_sgs_reg.hpp"
#include "gmg_sgs_plan.hpp"
#ifdef GMG_EXPERIMENTS
#include "gmg_sgs_chain.hpp"  // hand-over through an LDS word instead of s_barrier: measured slower, kept as an experiment
#endif
#include "gmg_lattice.hpp"
#include "gmg_transfer.hpp"
#include "gmg_forces.hpp"
#include "gmg_exact.hpp"
#include "gmg_assemble.hpp"
#include "gmg_rhs_cells.hpp"
#include "gmg_estimate.hpp"
#include "gmg_output.hpp"
#include "gmg_fastdiag.hpp"
#include "gmg_lanczos.hpp"
#include "gmg_mesh_tables.hpp"
#include "gmg_close.hpp"
#include "gmg_refine.hpp"
#include "gmg_density.hpp"
#include "gmg_mem.hpp"
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <map>
#include <queue>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "gmg_comm.hpp"

using namespace gmg;

namespace {

struct DevCSR {
  int64_t n_rows = 0, n_cols = 0, nnz = 0;
  DevPtr<int32_t> rowptr, col;
  DevPtr<double> val;
  DevPtr<int32_t> tile_row;
  int n_tiles = 0, tiles_per_xcd = 0, grid = 0;
  bool valid = false;
  HaloPlan halo;
  // SELL-64 copy (regular-width operators only), see gmg_device.hpp
  bool sell = false;
  DevPtr<int32_t> slice_ptr;   // in quads
  DevPtr<int32_t> slice_base;  // COL16: smallest column per slice
  DevPtr<void> sell_vals;      // uchar4 codes (VAL8) or double2 pairs
  DevPtr<void> sell_cols;      // ushort4 offsets (COL16) or int4 columns
  DevPtr<double> sell_dict;    // VAL8: 256 doubles
  DevPtr<int32_t> sell_spat, sell_pat;  // column-pattern ids per slice / pattern table
  int sellp_pid = -1, sellp_centre[9] = {};  // the nine-runs-of-three pattern served by spmv_sellp_kernel
  DevPtr<int32_t> sellp_wave_ptr;             // slice range of every wave of spmv_sellp_kernel
  DevPtr<int4> sellp_wave_rr;                 // strided fast waves: {first slice, stride, pairs, one more slice or -1}
  bool use_sellp = false;
  bool rowclass = false;  // run-pattern slices take their coefficients from a per-row class table (N4)
  DevPtr<uint8_t> sellp_rowcls;
  DevPtr<double> sellp_ctab;
  int n_classes = 0;
  int n_patterns = 0, n_pattern_slices = 0;
  bool val8 = false, col16 = false;
  int n_slices = 0, sell_grid = 0;
  int64_t sell_quads = 0;
  // lattice interior walked plane by plane (gmg_lattice.hpp): rows [lat_R0, lat_R1) by class table, the other slices from the SELL streams
  bool lattice = false;
  DevPtr<uint8_t> lat_rowcls;
  DevPtr<double> lat_ctab;
  DevPtr<int32_t> lat_gen;
  bool lat_only = false;       // made by gmg_set_level_matrix_lattice: class table + row classes, no CSR / SELL copy
  int lat_W = 0;               // rows of the window that repeats with the plane stride (== lat_nxy: one contiguous interior)
  int64_t lat_fast_rows = 0;
  int lat_classes = 0, lat_nx = 0, lat_nxy = 0, lat_R0 = 0, lat_R1 = 0, lat_C = 0, lat_K = 0, lat_S = 0, lat_fast_blocks = 0, lat_n_gen = 0, lat_grid = 0;
  int64_t lat_gen_bytes = 0;  // stream bytes of the slices outside the interior
  // hybrid layout (plan_hybrid, gmg_layout.hpp): y = A x reads the regular slices from SELL streams of their own and the rows of the other
  // slices from the CSR copy above, in one launch (spmv_hybrid_kernel); every other mode uses the CSR copy
  bool hyb = false, hyb_val8 = false;
  DevPtr<int32_t> hyb_qptr, hyb_spat, hyb_pat, hyb_tiles, hyb_reg;
  DevPtr<void> hyb_vals, hyb_cols;
  DevPtr<double> hyb_dict;
  int hyb_n_slices = 0, hyb_n_reg = 0, hyb_n_pattern_slices = 0, hyb_n_tiles = 0, hyb_tile_blocks = 0, hyb_grid = 0;
  int64_t hyb_stream_bytes = 0, hyb_csr_bytes = 0;  // bytes one product streams: SELL part, CSR part
  int lat_nv[3] = {0, 0, 0};  // lat_only: what gmg_set_level_matrix_lattice was given (the direct coarse solver reads them)
  double lat_Ke[64] = {};
};

struct SgsPlan {
  // generic level-scheduled sweep straight from the CSR copy (fallback: rows with unsorted columns).  Read only when !wave:
  // a plan built on the device (gmg_sgs_plan.hpp) always has wave set and leaves these four tables and n_stages_max empty
  DevPtr<int32_t> stage_ptr, stage_rows, block_row, block_stage;
  int n_blocks = 0;
  int n_stages_max = 0;
  // wavefront sweep with y in LDS (gmg_sgs.hpp)
  bool wave = false;
  DevPtr<SwRange> w_ranges;
  DevPtr<int32_t> w_block_rng, w_ws_ci, w_ci_row, w_row_ci, w_rpos_f, w_rpos_b;
  DevPtr<char> w_stream;
  DevPtr<double> w_ycur, w_iso_diag, w_iso_invd;
  int w_y_slots = 0, w_lds_bytes = 0, w_n_ranges = 0;
  int n_bwd = 0;  // backward ranges among w_n_ranges
  std::vector<int32_t> host_bwd_rows;  // level rows the self-contained backward records store their results to (their aux words, stream order)
  int n_self = 0, live_max[2] = {0, 0};  // self-contained ranges of the four-wave sweep; most y slots live at once per direction, as the allocator found them (0: not run)
  int64_t w_n_coupled = 0, w_stream_bytes = 0, w_steps = 0, w_stages = 0;
  int n_packed = 0;  // blocks whose rows are scheduled by slack (w_stages counts their levels); gmg_get_ssor_schedule
  int64_t w_fwd_steps = 0, w_stage_steps = 0;  // steps of a direction: the plan's, and what the stages need
  std::vector<int32_t> host_block_row;  // n_blocks + 1 (several ranks: who sweeps which rows)
  std::vector<int64_t> host_block_steps;  // n_blocks: sub-steps of each block's chain (both directions; gmg_get_ssor_partition)
  std::vector<int64_t> host_block_bytes;  // n_blocks: record-stream bytes of each block (plan log)
  std::vector<int32_t> host_block_rng;    // n_blocks + 1: ranges of each block (sgs_phase_profile: cycles per block)
  DevPtr<double> w_stage;               // staging of the all-gather of the swept pieces
  int64_t w_stage_len = 0;
  // four-wave variant (gmg_sgs_phase.hpp): same lists, its own ranges and record stream
  bool phased = false;
  bool dep = false;  // records laid out for gmg_sgs_dep.hpp (field-major, late = updated within the last three steps)
  bool reg = false;  // records laid out for gmg_sgs_reg.hpp (field-major, loaded straight into registers; no staging regions in LDS)
  DevPtr<PhRange> p_ranges;
  DevPtr<uint4> p_blk_tab;
  std::vector<PhRange> host_pranges;
  // who built the plan (gmg_get_ssor_plan_origin): the kernels of gmg_sgs_plan.hpp or the host; the bytes of col / val that came
  // back to the host for it; with option ssor_plan_device set and a host-built plan, why (a fixed text)
  bool on_device = false;
  int64_t csr_bytes_down = 0;
  const char *host_reason = "";
};

struct Level {
  DevCSR A, I, It, P, Pt;  // P: this level -> next finer one; Pt its transpose
  bool has_I = false, has_P = false;
  int64_t n = 0;       // owned rows
  int64_t n_vec = 0;   // owned + ghost entries of a level vector
  int64_t n_copy = 0;
  DevPtr<int32_t> copy_g, copy_l;
  std::vector<int32_t> host_copy_g, host_copy_l;  // the same lists on the host (mg_copy_tables)
  int copy_version = 0;                           // counts gmg_set_copy_indices calls
  DevPtr<double> sol, def, t, w1, w2, w3;
  // distributed runs keep levels >= 1 replicated and level 0 row-partitioned: the V-cycle sees
  // level 0 through these full-length replicas: views of sol/def on a single GPU, of the two owners below when
  // level 0 is partitioned (the only case in which those are allocated)
  double *sol_full = nullptr, *def_full = nullptr;
  DevPtr<double> sol_full_own, def_full_own;
  DevPtr<double> invd;
  double cheb_lmax = 0.0;
  // the Lanczos bound of D^-1 A (gmg_lanczos.hpp), formed at the level's first Chebyshev use with lmax_source Lanczos and kept
  // until the level matrix, the step count or the safety factor changes (drop_cheb_estimate)
  struct ChebEstimate {
    bool valid = false;
    int steps_run = 0;
    double ritz = 0.0;
  } cheb_est;
  SgsPlan sgs;
};

// the direct coarse solver's tables and scratch (gmg_fastdiag.hpp); ready while GMG_COARSE_DIRECT is selected
struct FastDiag {
  bool ready = false;
  double s = 0.0;
  int m[3] = {0, 0, 0}, ld[3] = {0, 0, 0};
  DevPtr<double> S[3], lam[3], mu[3];
  DevPtr<double> t1, t2;  // level-0 vectors between the passes
};

// what gmg_build_mesh_tables leaves on the device (gmg_mesh_tables.hpp): valid until the next build, gmg_reset or gmg_destroy
struct MeshTables {
  bool valid = false;
  int dim = 0;
  int64_t n_cells = 0, n_dofs = 0, n_hanging = 0, n_lines = 0, n_entries = 0;  // active cells, active DoFs, lines, line entries
  DevPtr<int32_t> cell_dofs, constraint_of_dof, line_ptr, line_master, line_dof;
  DevPtr<uint8_t> cell_level;
  DevPtr<unsigned long long> vertex_of_dof;
  DevPtr<double> line_weight;
  struct PerLevel {
    int64_t n_cells = 0, n_dofs = 0;
    DevPtr<int32_t> cell_dofs;
    DevPtr<unsigned long long> vertex_of_dof;
    DevPtr<uint8_t> dof_flags;
  };
  std::vector<PerLevel> level;
  // what gmg_close_constraints adds (gmg_close.hpp): the closed lines of these tables, dropped with them
  struct Closed {
    bool valid = false;
    int64_t n_entries = 0;
    int max_line = 0;        // entries of the longest closed line
    bool any_inhom = false;  // some line_inhomogeneity is not 0
    DevPtr<int32_t> line_ptr, line_master;
    DevPtr<double> line_weight, line_inhom;
  } closed;
  // what gmg_build_face_table_resident adds (gmg_refine.hpp): the face table of these tables' active cells, dropped with them
  struct Faces {
    bool valid = false;
    DevPtr<uint8_t> kind;   // [n_cells * 2 dim]
    DevPtr<int32_t> cell;   // [n_cells * 2 dim * 2^(dim-1)]
  } faces;
  // what gmg_estimate_error_resident adds (gmg_estimate.hpp): the marks of these tables' active cells, dropped with them
  struct Marks {
    bool valid = false;
    int64_t n_marked = 0;
    DevPtr<uint8_t> mark;   // [n_cells]
  } marks;
  // what gmg_build_point_locator_resident adds (gmg_forces.hpp): the forest flattened for locate(); the cells' DoFs are
  // cell_dofs above, so 4 bytes per forest cell are all it keeps.  Dropped with the tables.
  struct PointLocator {
    bool valid = false;
    int64_t n_nodes = 0;
    int32_t n0[3] = {0, 0, 0};
    DevPtr<int32_t> node;   // [n_nodes]
  } locator;
};

// what gmg_refine_forest leaves on the device (gmg_refine.hpp): valid until the next refinement, gmg_reset or gmg_destroy
struct RefinedForest {
  bool valid = false;
  int n_levels = 0;
  int64_t n_cells = 0, n_flags = 0, n_split = 0;  // new cells of all levels, cells of the forest that went in, cells split
  std::vector<int64_t> level_ptr;
  DevPtr<int32_t> coord, first_child, parent;
  DevPtr<uint8_t> closed;  // [n_flags]
};

}  // namespace

struct gmg_context {
  int device = 0;
  hipStream_t stream = nullptr;
  int n_levels = 0;
  std::vector<Level> lv;
  DevCSR S;
  DevPtr<double> S_invd;
  DevPtr<double> S_tmp;  // system-sized scratch with ghost tail (halo import of src)
  // smoother / coarse parameters (src/step-50.cc:962, 970-973)
  int smoother = GMG_SMOOTHER_SSOR;
  double omega = 0.5;
  int steps = 2;
  int cheb_degree = 2;
  double cheb_ratio = 30.0, cheb_lmax_user = 0.0;
  // gmg_set_chebyshev / options cheb_*: the polynomial, where lmax comes from, the Lanczos steps and the safety factor
  int cheb_polynomial = GMG_CHEB_FIRST_KIND, cheb_lmax_source = GMG_CHEB_LMAX_GERSHGORIN, cheb_lanczos_steps = 10;
  double cheb_safety = 1.2;
  int cheb_degree_opt = 0;      // option "cheb_degree": > 0 overrides the degree gmg_set_smoother was given
  int lanczos_max_blocks = 0;   // option "lanczos_max_blocks": cap on the grids of the estimator's kernels (0: by size); results do not depend on it
  double coarse_tol = 1e-10;
  int coarse_maxit = 1000;
  int coarse_solver = GMG_COARSE_CG;  // gmg_set_coarse_solver; back to CG with every new level-0 matrix and gmg_reset
  bool coarse_direct_opt = false;     // option coarse_direct: select the direct solver whenever a lattice level 0 qualifies
  int coarse_direct_max_blocks = 0;   // option coarse_direct_max_blocks: cap on the grids of its passes (0: by size); results do not depend on it
  FastDiag fd;
  // coarse CG work space (level-0 sized)
  int64_t cg_n = 0;
  DevPtr<double> cg_g, cg_d0, cg_d1, cg_h;
  // direction vectors of the last kXRing iterations (three-kernel coarse CG), allocated on first use: views of cg_ring_own, or
  // of ring_shared on the peer transport.  ring_shared is mapped by every rank and freed collectively (free_cg_ring): it stays
  // manual, like Comm::box and what comm_share_alloc returns
  double *cg_ring[kXRing] = {};
  DevPtr<double> cg_ring_own[kXRing];
  int64_t cg_ring_len = 0;
  // peer transport, partitioned level 0: the ring is one shared allocation the neighbours write their halo entries into
  char *ring_shared[kPeerMaxRanks] = {};
  int64_t ring_stride = 0;                      // doubles between my ring slots
  int64_t peer_meta[kPeerMaxRanks][4 + kPeerMaxRanks] = {};  // per rank: ring stride, owned rows, ghost offset of every source
  unsigned long long peer_tag0 = 1;             // tags of the next coarse solve start here
  DevPtr<unsigned int> peer_push_cnt;
  DevPtr<CGState> st;        // device
  HostPtr<CGState> st_host;  // pinned, 2 slots (the chunk being checked / the speculative one)
  CGState st_final{};
  Event ev_chunk[2];
  DevPtr<double> part_a, part_b;  // reduction partials (4 * kMaxPartials each)
  DevPtr<double> lanczos_rec;     // the record of one Lanczos estimate (gmg_lanczos.hpp: record_len(kMaxSteps) doubles)
  DevPtr<double> scal_dev;        // 8 doubles
  HostPtr<double> scal_host;      // pinned, 8 doubles
  // outer CG steps (gmg_cg_direction_step / gmg_cg_update_step): g.h stays on the device between the steps
  DevPtr<double> ocg_dev;         // [0], [1]: g.h of this and of the previous iteration (ocg_cur names this one's); [2]: d.h
  int ocg_cur = 0;
  double ocg_gh = 0.0;            // g.h on the host (option disable_outer_cg_fused, several ranks)
  // copy_to_mg / copy_from_mg as one kernel each (mg_copy_tables); option "disable_vcycle_fused": the memsets, gathers and the
  // separate t = def - t of the coarse-level residual, as before
  bool disable_vcycle_fused = false;
  DevPtr<int32_t> mgcopy_to, mgcopy_from_level, mgcopy_from_row;
  std::vector<int64_t> mgcopy_sig;  // what the tables were built for: n_sys, then (n_vec, n_copy, copy_version) per level
  bool mgcopy_ok = false;
  bool hybrid_two_launches = false;  // option "hybrid_two_launches": the CSR tiles and the SELL slices of a hybrid operator as two kernels (measured slower or equal: DESIGN.md section 28)
  bool disable_hybrid = false;  // option "disable_hybrid": operators the SELL rule refuses stay on the CSR row-window kernel for y = A x too (checked at upload and at launch)
  bool disable_outer_cg_fused = false;  // option "disable_outer_cg_fused": three host waits and six kernels per iteration, as before the fused steps
  HostPtr<int> sgs_abort;         // pinned, device-visible: set by the SSOR sweep if its wave protocol broke
  // tuning / measurement
  int coarse_chunk = 0;
  // diagnostic options (gmg_set_option / GMG_OPTIONS); the defaults are the fast paths
  int sgs_y_slots = 0;      // 0 = kSwYSlots; tests shrink it to force several LDS ranges
  bool ssor_plan_device = false;  // option "ssor_plan_device": the default four-wave plan of a level is formed by kernels (gmg_sgs_plan.hpp) where it applies
  bool sgs_sliding = true;  // four-wave sweep: one self-contained range per direction where a block's live rows fit the y slots
  int sgs_pack = -1;        // self-contained ranges: rows scheduled by slack (ssor_pack_levels).  0 never, 1 always, -1 (unset) by the level's size
  bool sgs_disable_wave = false, sgs_disable_phase = false, sgs_chain = false, sgs_dep = false, sgs_reg = false, debug_upload = false, sgs_profile = false;
  int sgs_profile_mode = 0;
  int sgs_phase_chunk = 0;         // steps per chunk of one shape (0: default)
  int sgs_pf_lead_kb = 0;          // diagnostics: minimum lead of the prefetch wave in KB (0: default; < 0: no prefetch)
  bool sgs_phase_nocascade = false;  // every step gathers all T1 slots of its shape (comparison)
  bool sgs_phase_nosplit = false;  // the whole tail is gathered in the dependent phase (comparison / tests)
  int sgs_phase_profile = 0;  // > 0: print cycles per step of every range of the four-wave sweep
  int sgs_groups = 0;  // 0: chosen per sweep direction; 1..4: forced (experiments)
  int sgs_lds_bytes_override = 0;  // tests: request this much dynamic LDS for the SSOR sweep (over the limit: the launch is rejected)
  bool disable_sell = false, disable_patterns = false, disable_compression = false, disable_sellp = false, disable_rowclass = false, disable_lattice = false;
  int lattice_segments = 0;  // segments per XCD slab of the lattice kernel (0: by size)
  int lattice_max_blocks = 0;  // cap on the marching workgroups (0: only the reduction partials cap them)
  int sell_grid = 0;        // workgroups of the SELL kernels (0 = by size)
  int sellp_rr = 0;         // round-robin slice order of the fast waves: 0 by size, 1 on, 2 off
  double sellp_cost = 4.0;  // cost of a streamed slice in pattern slices (wave balancing of spmv_sellp_kernel)
  int ssor_blocks = 1;  // 1 = exact sequential SGS; B > 1 = block Jacobi of SGS (the reference on B ranks)
  int ssor_partition = GMG_SSOR_PARTITION_ROWS;          // where the B blocks' boundaries come from (setup_sgs)
  std::map<int, std::vector<int64_t>> ssor_block_rows;   // explicit boundaries per level (gmg_set_ssor_block_rows): these win
  int cg_variant = 0;  // 0 auto, 1 fused 2-kernel iteration, 2 unfused 3-kernel iteration
  int last_coarse_iters = 0;
  int prof_every = 0;
  std::vector<Event> ev_a, ev_b;  // sampled level-0 SpMV launches
  std::vector<Event> ev_c, ev_d;  // sampled update-kernel launches
  std::vector<Event> ev_e, ev_f;  // SSOR sweep launches
  bool launch_refused = false;  // launch_op met an operator / mode combination it has no kernel for (reported by launch_status)
  int ev_used = 0, ev2_used = 0, ev3_used = 0;
  long long sgs_launch_no = 0;
  hipEvent_t timed_start = nullptr, timed_stop = nullptr;  // next launch carries these as its dispatch start / stop events
  gmg_stats stats{};
  DevPtr<double> dens_dev;  // charge densities kept on the device (gmg_charge_density with dens == NULL): [cells][nq]
  int64_t dens_cells = 0;
  int dens_nq = 0;
  // point location for the atom forces (gmg_set_point_locator; kept until gmg_reset)
  gmg_forces::Locator loc{};
  DevPtr<int32_t> loc_node, loc_dofs;
  int64_t loc_max_dof = -1;  // -1: no locator set
  int force_block = 64;      // workgroup size of the force kernels (gmg_set_option "force_block"); results do not depend on it
  int exact_chunk_log2 = 35;  // gmg_exact.hpp: at most 2^this point-atom evaluations per launch (option "exact_chunk_log2")
  int output_chunk_log2 = 20;  // gmg_output.hpp: at most 2^this cells per launch, the size of the call's device temporaries (option "output_chunk_log2")
  bool reset_keeps_mesh_tables = false;  // option "reset_keeps_mesh_tables": gmg_reset leaves the mesh tables and their closed lines alone
  int assemble_max_blocks = 0;  // gmg_assemble.hpp: cap on the workgroups of every assembly kernel (option "assemble_max_blocks"; 0: by size); results do not depend on it
  MeshTables mesh;              // gmg_build_mesh_tables: the tables of the last build
  RefinedForest refined;        // gmg_refine_forest: the forest of the last refinement
  int density_segment = 0;      // gmg_density.hpp: atoms per LDS segment of a cell's lane group (option "density_segment"; 0: by group size); results do not depend on it
  int estimate_max_blocks = 0;  // gmg_estimate.hpp: the same cap for the estimator's kernels (option "estimate_max_blocks"); results do not depend on it
  Comm comm;
  bool dist = false;             // communicator initialised: level 0 + system rows are partitioned
  int64_t sys_global = 0, l0_global = 0;  // l0_global == 0 on a communicator: level 0 is replicated, only the outer CG is partitioned
  DevPtr<double> sys_full_a, sys_full_b;  // replicated src / dst of the V-cycle
  std::string err;
};

namespace {

#define HIPC(call)                                                                                   \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) {                                                                          \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                                  \
      return GMG_ERR_HIP;                                                                            \
    }                                                                                                \
  } while (0)

#define CHK(call)                 \
  do {                            \
    int rc_ = (call);             \
    if (rc_ != GMG_OK) return rc_; \
  } while (0)

// a rejected launch (bad grid, too much dynamic LDS, ...) leaves no trace but hipGetLastError: every entry point that
// enqueued kernels ends with this, so the failure surfaces as GMG_ERR_HIP instead of a silently missing result
#define RETURN_LAUNCHED(ctx)                                                      \
  do {                                                                            \
    const hipError_t e_ = hipGetLastError();                                      \
    if (e_ != hipSuccess) {                                                       \
      (ctx)->err = std::string("kernel launch: ") + hipGetErrorString(e_);       \
      return GMG_ERR_HIP;                                                         \
    }                                                                             \
    return GMG_OK;                                                                \
  } while (0)

int launch_status(gmg_context *ctx) {
  if (ctx->launch_refused) { ctx->launch_refused = false; return GMG_ERR_UNSUPPORTED; }
  RETURN_LAUNCHED(ctx);
}

int fail(gmg_context *ctx, int code, const char *msg) {
  ctx->err = msg;
  return code;
}

// Host wait on the context's stream by polling: hipStreamSynchronize sleeps on an interrupt and
// wakes ~50-100 us late, which shows up as GPU idle time at every convergence check of the
// coarse CG and every dot product of the outer CG.
inline hipError_t stream_wait(hipStream_t s) {
  for (;;) {
    const hipError_t e = hipStreamQuery(s);
    if (e != hipErrorNotReady) return e;
  }
}

// level 0 (matrix, coarse CG vectors) is row-partitioned over the ranks
inline bool l0_partitioned(const gmg_context *ctx) { return ctx->dist && ctx->l0_global > 0; }

inline int grid_for(int64_t n) {
  int64_t g = (n + kThreads - 1) / kThreads;
  if (g < 1) g = 1;
  if (g > kMaxPartials) g = kMaxPartials;
  return (int)g;
}

// a fresh operator that keeps its halo plan (set before the matrix, once per operator)
void reset_keep_halo(DevCSR &m) {
  HaloPlan keep = std::move(m.halo);
  m = DevCSR();
  m.halo = std::move(keep);
}

// the options of the context that steer an operator's layout
LayoutOptions layout_options(const gmg_context *ctx) {
  LayoutOptions o;
  o.disable_sell = ctx->disable_sell; o.disable_patterns = ctx->disable_patterns; o.disable_compression = ctx->disable_compression;
  o.disable_sellp = ctx->disable_sellp; o.disable_rowclass = ctx->disable_rowclass; o.disable_lattice = ctx->disable_lattice;
  o.disable_hybrid = ctx->disable_hybrid;
  o.sell_grid = ctx->sell_grid; o.sellp_cost = ctx->sellp_cost; o.sellp_rr = ctx->sellp_rr;
  o.lattice_segments = ctx->lattice_segments; o.lattice_max_blocks = ctx->lattice_max_blocks;
  o.debug = ctx->debug_upload;
  return o;
}

static_assert(sizeof(WaveRR) == sizeof(int4) && alignof(WaveRR) <= alignof(int4),
              "the round-robin descriptors are read as int4 by spmv_sellp_kernel");

void set_tiles(DevCSR &m, const TilePlan &T) { m.n_tiles = T.n_tiles; m.tiles_per_xcd = T.tiles_per_xcd; m.grid = T.grid; }

// Host CSR -> device: upload_csr plans the layouts (gmg_layout.hpp) and the copy_* functions below enqueue the plan's
// vectors as they are; they wait for nothing, so every plan has to outlive the stream's copies.

// the CSR copy, with a zeroed 8-entry pad behind col and val, and the row-window tiles
int copy_csr(gmg_context *ctx, DevCSR &m, const CsrView &A, const std::vector<int32_t> &rp, const TilePlan &T) {
  const size_t nnz = (size_t)A.nnz(), pad = 8;
  HIPC(upload(m.rowptr, rp, ctx->stream));
  HIPC(upload(m.col, A.col, nnz, ctx->stream, nnz + pad));
  HIPC(upload(m.val, A.val, nnz, ctx->stream, nnz + pad));
  HIPC(hipMemsetAsync(m.col.get() + nnz, 0, sizeof(int32_t) * pad, ctx->stream));
  HIPC(hipMemsetAsync(m.val.get() + nnz, 0, sizeof(double) * pad, ctx->stream));
  HIPC(upload(m.tile_row, T.tile_row, ctx->stream));
  set_tiles(m, T);
  return GMG_OK;
}

// value and column streams, with 64 bytes of slack behind each (the kernels' 16-byte loads past the last quad)
int copy_streams(gmg_context *ctx, const SellStreams &s, DevPtr<void> &vals, DevPtr<void> &cols) {
  HIPC(vals.alloc_bytes(s.val_bytes() + 64));
  HIPC(cols.alloc_bytes(s.col_bytes() + 64));
  HIPC(hipMemcpyAsync(vals.get(), s.vals(), s.val_bytes(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(cols.get(), s.cols(), s.col_bytes(), hipMemcpyHostToDevice, ctx->stream));
  return GMG_OK;
}

int copy_sell(gmg_context *ctx, DevCSR &m, const StreamPlan &P) {
  const SellPlan &s = P.sell;
  const SellpPlan &w = P.sellp;
  const LatticePlan &L = P.lat;
  hipStream_t st = ctx->stream;
  HIPC(upload(m.slice_ptr, s.slice_ptr, st));
  HIPC(upload(m.slice_base, s.slice_base, st));
  HIPC(upload(m.sell_dict, s.vd.dict, st));
  CHK(copy_streams(ctx, s.s, m.sell_vals, m.sell_cols));
  m.sell = true; m.val8 = s.s.val8; m.col16 = s.s.col16;
  m.n_slices = (int)s.n_slices; m.sell_quads = s.quads; m.sell_grid = s.sell_grid;
  if (s.pat.n_pattern_slices > 0) {
    HIPC(upload(m.sell_spat, s.pat.spat, st));
    HIPC(upload(m.sell_pat, s.pat.table, st));
    m.n_patterns = (int)s.pat.list.size(); m.n_pattern_slices = s.pat.n_pattern_slices;
    m.sellp_pid = s.sellp_pid; m.use_sellp = s.use_sellp;
    std::copy(s.sellp_centre, s.sellp_centre + 9, m.sellp_centre);
  }
  if (!w.wave_ptr.empty()) HIPC(upload(m.sellp_wave_ptr, w.wave_ptr, st));
  if (w.rowclass) {
    HIPC(upload(m.sellp_rowcls, w.rowcls, st));
    HIPC(upload(m.sellp_ctab, w.ctab, st));
    if (!w.wave_rr.empty()) HIPC(upload(m.sellp_wave_rr, reinterpret_cast<const int4 *>(w.wave_rr.data()), w.wave_rr.size(), st));
    m.rowclass = true; m.n_classes = w.n_classes;
  }
  m.lat_classes = L.classes;
  if (L.planned) {
    m.lat_nx = (int)L.nx; m.lat_nxy = (int)L.nxy; m.lat_R0 = (int)L.R0; m.lat_R1 = (int)L.R1; m.lat_W = (int)L.W;
    m.lat_C = L.C; m.lat_K = L.K; m.lat_S = L.S; m.lat_fast_blocks = L.fast_blocks; m.lat_grid = L.grid;
    m.lat_fast_rows = L.fast_rows; m.lat_n_gen = (int)L.gen.size(); m.lat_gen_bytes = L.gen_bytes;
  }
  if (L.built) {
    HIPC(upload(m.lat_rowcls, L.rowcls, st, L.rowcls.size() + 64));
    HIPC(upload(m.lat_ctab, L.ctab, st));
    HIPC(upload(m.lat_gen, L.gen, st));
    m.lattice = true;
  }
  return GMG_OK;
}

int copy_hybrid(gmg_context *ctx, DevCSR &m, const HybridPlan &H) {
  hipStream_t st = ctx->stream;
  HIPC(upload(m.hyb_qptr, H.qptr, st));
  HIPC(upload(m.hyb_spat, H.pat.spat, st));
  HIPC(upload(m.hyb_pat, H.pat.table, st));
  HIPC(upload(m.hyb_tiles, H.tiles, st));
  HIPC(upload(m.hyb_reg, H.reg, st));
  HIPC(upload(m.hyb_dict, H.vd.dict, st));
  CHK(copy_streams(ctx, H.s, m.hyb_vals, m.hyb_cols));
  m.hyb = true; m.hyb_val8 = H.vd.val8;
  m.hyb_n_slices = H.n_slices; m.hyb_n_reg = (int)H.reg.size(); m.hyb_n_pattern_slices = H.pat.n_pattern_slices;
  m.hyb_n_tiles = H.n_tiles; m.hyb_tile_blocks = H.tile_blocks; m.hyb_grid = H.grid;
  m.hyb_stream_bytes = H.stream_bytes; m.hyb_csr_bytes = H.csr_bytes;
  return GMG_OK;
}

// keep_csr: the CSR copy of a SELL operator is only kept where the SGS sweeps need it (levels >= 1).  allow_hybrid: see plan_streams
int upload_csr(gmg_context *ctx, DevCSR &m, int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col,
               const double *val, bool keep_csr = false, bool allow_hybrid = false) {
  if (n_rows < 0 || n_cols < 0 || !rowptr) return fail(ctx, GMG_ERR_INVALID, "upload_csr: bad arguments");
  const int64_t nnz = rowptr[n_rows];
  if (nnz >= (int64_t)1 << 31 || n_rows >= (int64_t)1 << 31 || n_cols >= (int64_t)1 << 31)
    return fail(ctx, GMG_ERR_UNSUPPORTED, "operator needs 64-bit device indices (nnz >= 2^31)");
  reset_keep_halo(m);
  m.n_rows = n_rows; m.n_cols = n_cols; m.nnz = nnz;
  const LayoutOptions opt = layout_options(ctx);
  PhaseLog phase{opt.debug};
  const CsrView A{n_rows, n_cols, rowptr, col, val};
  if (const char *wrong = check_csr(A)) return fail(ctx, GMG_ERR_INVALID, wrong);
  const std::vector<int32_t> rp(rowptr, rowptr + n_rows + 1);
  const TilePlan T = plan_tiles(rowptr, n_rows);
  StreamPlan P;
  int rc = copy_csr(ctx, m, A, rp, T);
  phase("csr copy");
  if (rc == GMG_OK) {
    // (whether m carries a halo plan says nothing here: the plan of these rows is set after them, what m holds is the one of
    // the operator before -- none after gmg_reset, so every partitioned system matrix of the host driver has taken the hybrid layout)
    P = plan_streams(A, opt, allow_hybrid, phase);
    rc = P.sell.built ? copy_sell(ctx, m, P) : P.hyb.built ? copy_hybrid(ctx, m, P.hyb) : GMG_OK;
  }
  const hipError_t waited = hipStreamSynchronize(ctx->stream);  // rp, T and P are read by the copies until here
  if (rc != GMG_OK) return rc;
  HIPC(waited);
  m.valid = true;
  if (m.sell && !keep_csr) { m.col.reset(); m.val.reset(); m.tile_row.reset(); }
  phase("finish");
  if (opt.debug)
    std::fprintf(stderr, "[gmg] operator %lld x %lld nnz %lld: tiles %d grid %d sell %d val8 %d col16 %d sell_grid %d patterns %d pattern_slices %d/%d\n", (long long)n_rows,
                 (long long)n_cols, (long long)nnz, m.n_tiles, m.grid, (int)m.sell, (int)m.val8, (int)m.col16, m.sell_grid, m.n_patterns, m.n_pattern_slices, m.n_slices);
  if (opt.debug && m.rowclass) std::fprintf(stderr, "[gmg]   row classes of the run-pattern slices: %d\n", m.n_classes);
  if (opt.debug && !m.hyb) std::fprintf(stderr, "[gmg]   layout %s\n", m.sell ? "sell" : "csr");
  return GMG_OK;
}

int alloc_vec(gmg_context *ctx, DevPtr<double> &p, int64_t n) {
  HIPC(p.alloc((size_t)std::max<int64_t>(n + 2, 2)));
  HIPC(hipMemsetAsync(p.get(), 0, sizeof(double) * (size_t)std::max<int64_t>(n + 2, 2), ctx->stream));
  return GMG_OK;
}

// ---- SpMV launcher ---------------------------------------------------------------------

// one launcher for both layouts; returns the grid (= number of reduction partials when CG != 0)
// Launch on the context's stream.  When the caller armed ctx->timed_start / timed_stop the events are
// attached to the dispatch itself (hipExtLaunchKernelGGL): hipEventElapsedTime then gives the kernel's own
// begin-to-end time -- what rocprofv3 --kernel-trace reports -- instead of event-record to event-record,
// which includes the launch gap.
template <typename K, typename... A>
inline void launch_timed(gmg_context *ctx, K kernel, dim3 grid, dim3 block, size_t lds, const A &...args) {
  if (ctx->timed_start) {
    hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, ctx->stream, ctx->timed_start, ctx->timed_stop, 0u, args...);
    ctx->timed_start = ctx->timed_stop = nullptr;
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, args...);
  }
}

template <int MODE, int CG>
int launch_op(gmg_context *ctx, const DevCSR &m, const SpmvArgs &a) {
  if (m.sell || m.lat_only) {
    SellArgs sa{m.slice_ptr.get(), m.slice_base.get(), m.sell_vals.get(), m.sell_cols.get(), m.sell_dict.get(), m.sell_spat.get(), m.sell_pat.get(), m.n_slices, (int)m.n_rows, a};
    if constexpr (MODE == kStore && (CG == 0 || CG == 2)) {
      if (m.lattice && !a.init) {
        LatArgs la{};
        la.pa.sa = sa; la.pa.col16 = m.col16 ? 1 : 0;
        la.rowcls = m.lat_rowcls.get(); la.ctab = m.lat_ctab.get(); la.n_classes = m.lat_classes;
        la.nx = m.lat_nx; la.nxy = m.lat_nxy; la.W = m.lat_W; la.R0 = m.lat_R0; la.R1 = m.lat_R1; la.C = m.lat_C; la.K = m.lat_K; la.S = m.lat_S;
        la.fast_blocks = m.lat_fast_blocks; la.gen_slices = m.lat_gen.get(); la.n_gen = m.lat_n_gen;
        la.edge_mode = m.lat_only ? 1 : 0; la.n_rows = (int)m.n_rows;
        if (m.lat_S * m.lat_C > (m.lat_fast_blocks / 8) * 4) launch_timed(ctx, spmv_lattice_kernel<CG, true>, dim3(m.lat_grid), dim3(kThreads), 0, la);
        else launch_timed(ctx, spmv_lattice_kernel<CG, false>, dim3(m.lat_grid), dim3(kThreads), 0, la);
        return m.lat_grid;
      }
    }
    if (m.lat_only) {  // (an operator that exists as a class table only: plain products and the coarse CG's three-kernel iteration)
      ctx->err = "operator set by gmg_set_level_matrix_lattice: only y = A x and the three-kernel coarse CG are available";
      ctx->launch_refused = true;
      return 1;
    }
    if (m.use_sellp) {
      SellPatArgs pa{};
      pa.sa = sa; pa.wave_ptr = m.sellp_wave_ptr.get(); pa.wave_rr = m.sellp_wave_rr.get(); pa.pid0 = m.sellp_pid; pa.col16 = m.col16 ? 1 : 0;
      for (int u = 0; u < 9; ++u) pa.centre[u] = m.sellp_centre[u];
      pa.rowcls = m.sellp_rowcls.get(); pa.ctab = m.sellp_ctab.get(); pa.n_classes = m.n_classes;
      if (m.rowclass) launch_timed(ctx, spmv_sellp_kernel<MODE, CG, true>, dim3(m.sell_grid), dim3(kThreads), 0, pa);
      else launch_timed(ctx, spmv_sellp_kernel<MODE, CG, false>, dim3(m.sell_grid), dim3(kThreads), 0, pa);
      return m.sell_grid;
    }
    if (m.val8 && m.col16) launch_timed(ctx, spmv_sell_kernel<MODE, CG, true, true>, dim3(m.sell_grid), dim3(kThreads), 0, sa);
    else if (m.val8) launch_timed(ctx, spmv_sell_kernel<MODE, CG, true, false>, dim3(m.sell_grid), dim3(kThreads), 0, sa);
    else if (m.col16) launch_timed(ctx, spmv_sell_kernel<MODE, CG, false, true>, dim3(m.sell_grid), dim3(kThreads), 0, sa);
    else launch_timed(ctx, spmv_sell_kernel<MODE, CG, false, false>, dim3(m.sell_grid), dim3(kThreads), 0, sa);
    return m.sell_grid;
  }
  if constexpr (MODE == kStore && CG == 0) {
    if (m.hyb && !a.init && !ctx->disable_hybrid) {
      HybArgs h{};
      h.sa = SellArgs{m.hyb_qptr.get(), nullptr, m.hyb_vals.get(), m.hyb_cols.get(), m.hyb_dict.get(), m.hyb_spat.get(), m.hyb_pat.get(), m.hyb_n_slices, (int)m.n_rows, a};
      h.tiles = m.hyb_tiles.get(); h.reg = m.hyb_reg.get(); h.n_tiles = m.hyb_n_tiles; h.n_reg = m.hyb_n_reg; h.tile_blocks = m.hyb_tile_blocks;
      if (ctx->hybrid_two_launches) {  // (measurement: the SELL workgroups without the row window's 32 KiB of LDS)
        HybArgs t = h, q = h;
        q.tile_blocks = 0;
        launch_timed(ctx, spmv_hybrid_kernel<true, 1>, dim3(m.hyb_tile_blocks), dim3(kThreads), 0, t);
        if (m.hyb_val8) hipLaunchKernelGGL((spmv_hybrid_kernel<true, 2>), dim3(m.hyb_grid - m.hyb_tile_blocks), dim3(kThreads), 0, ctx->stream, q);
        else hipLaunchKernelGGL((spmv_hybrid_kernel<false, 2>), dim3(m.hyb_grid - m.hyb_tile_blocks), dim3(kThreads), 0, ctx->stream, q);
        return m.hyb_grid;
      }
      if (m.hyb_val8) launch_timed(ctx, spmv_hybrid_kernel<true, 0>, dim3(m.hyb_grid), dim3(kThreads), 0, h);
      else launch_timed(ctx, spmv_hybrid_kernel<false, 0>, dim3(m.hyb_grid), dim3(kThreads), 0, h);
      return m.hyb_grid;
    }
  }
  launch_timed(ctx, spmv_tile_kernel<MODE, CG>, dim3(m.grid), dim3(kThreads), 0, a);
  return m.grid;
}
template <int MODE>
void launch_spmv_mode(gmg_context *ctx, const DevCSR &m, const SpmvArgs &a) {
  (void)launch_op<MODE, 0>(ctx, m, a);
}

SpmvArgs base_args(const DevCSR &m, const double *x, double *y) {
  SpmvArgs a{};
  a.rowptr = m.rowptr.get(); a.col = m.col.get(); a.val = m.val.get(); a.tile_row = m.tile_row.get();
  a.n_tiles = m.n_tiles; a.tiles_per_xcd = m.tiles_per_xcd;
  a.x = x; a.y = y;
  return a;
}

// ghost import of `x` for operator m (Epetra_Import inside every vmult); no-op on one rank
int import_ghosts(gmg_context *ctx, const DevCSR &m, double *x) {
  if (!m.halo.active) return GMG_OK;  // a replicated operator
  int rc = halo_exchange(ctx->comm, m.halo, x, m.n_rows, ctx->stream);
  if (rc) return fail(ctx, GMG_ERR_COMM, "halo exchange failed");
  return GMG_OK;
}

int spmv(gmg_context *ctx, const DevCSR &m, int mode, const double *x, double *y, const double *init = nullptr,
         const double *b = nullptr) {
  if (!m.valid) return fail(ctx, GMG_ERR_INVALID, "operator not set");
  if (m.n_rows == 0) return GMG_OK;
  SpmvArgs a = base_args(m, x, y);
  a.init = init; a.b = b;
  switch (mode) {
    case kStore: launch_spmv_mode<kStore>(ctx, m, a); break;
    case kResid: launch_spmv_mode<kResid>(ctx, m, a); break;
    case kAddTo: launch_spmv_mode<kAddTo>(ctx, m, a); break;
    default: return fail(ctx, GMG_ERR_INVALID, "bad spmv mode");
  }
  return launch_status(ctx);
}

// ---- reductions to the host -------------------------------------------------------------

int fetch_scalars(gmg_context *ctx, int n) {
  HIPC(hipMemcpyAsync(ctx->scal_host.get(), ctx->scal_dev.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(stream_wait(ctx->stream));
  if (*ctx->sgs_abort.get()) return fail(ctx, GMG_ERR_HIP, "SSOR sweep: a wave gave up waiting for its partner (internal protocol error)");
  if (comm_aborted(ctx->comm)) return fail(ctx, GMG_ERR_COMM, "peer transport: a rank gave up waiting for a message or an acknowledgement");
  if (ctx->comm.n_ranks > 1) {
    // sums: slots flagged by the caller; handled in the callers below
  }
  return GMG_OK;
}

int dot_host(gmg_context *ctx, const double *x, const double *y, int64_t n, double *out) {
  const int g = grid_for(n);
  hipLaunchKernelGGL(dot_partial_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, x, y, n, ctx->part_a.get());
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double *)ctx->part_a.get(), g, 1, 0u,
                     ctx->scal_dev.get());
  if (ctx->comm.n_ranks > 1) {
    if (allreduce_sum(ctx->comm, ctx->scal_dev.get(), 1, ctx->stream)) return fail(ctx, GMG_ERR_COMM, "all-reduce failed");
  }
  CHK(launch_status(ctx));
  CHK(fetch_scalars(ctx, 1));
  *out = ctx->scal_host.get()[0];
  return GMG_OK;
}

// ---- smoothers (A7) ---------------------------------------------------------------------

// event times of the SSOR sweep launches bracketed so far -> stats (waits for the stream)
void collect_sgs_samples(gmg_context *ctx) {
  if (ctx->ev3_used == 0) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (int i = 0; i < ctx->ev3_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev_e[(size_t)i].get(), ctx->ev_f[(size_t)i].get()) != hipSuccess) continue;
    ctx->stats.sgs_ms_total += ms;
    ctx->stats.sgs_samples++;
  }
  ctx->ev3_used = 0;
}

// option sgs_profile: the instrumented variant of the sweep; prints where each range of the first blocks spent its cycles
int sgs_profile_launch(gmg_context *ctx, Level &L, SgsWaveArgs p) {
  const size_t nr = (size_t)L.sgs.w_n_ranges;
  DevPtr<unsigned long long> d;
  std::vector<unsigned long long> h(4 * nr, 0);
  HIPC(d.alloc(4 * nr));
  p.prof = d.get();
  p.prof_mode = ctx->sgs_profile_mode;
  hipLaunchKernelGGL(sgs_wave_kernel<true>, dim3(L.sgs.n_blocks), dim3(kSwThreads), (size_t)L.sgs.w_lds_bytes, ctx->stream, p);
  HIPC(hipMemcpyAsync(h.data(), d.get(), sizeof(unsigned long long) * 4 * nr, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (L.sgs.w_steps > 1000) {
    std::fprintf(stderr, "[gmg] SGS sweep profile mode %d (%lld rows, %d ranges; shader cycles: sweep / of it waiting for the ring / load / write-back):", ctx->sgs_profile_mode, (long long)L.n, (int)nr);
    for (size_t i = 0; i < std::min<size_t>(nr, 10); ++i)
      std::fprintf(stderr, " [%llu %llu %llu %llu]", h[4 * i], h[4 * i + 1], h[4 * i + 2], h[4 * i + 3]);
    std::fprintf(stderr, "\n");
  }
  return GMG_OK;
}

// the pre-pass operands of a level's sweep for the epilogue of its residual product (spmv_tile_kernel<kResidPre, 0>)
SgsPreArgs sgs_pre_args(const gmg_context *ctx, const Level &L, double *y) {
  SgsPreArgs q{};
  q.row_ci = L.sgs.w_row_ci.get(); q.rpos_f = L.sgs.w_rpos_f.get(); q.rpos_b = L.sgs.w_rpos_b.get();
  q.iso_diag = L.sgs.w_iso_diag.get(); q.iso_invd = L.sgs.w_iso_invd.get();
  q.stream = reinterpret_cast<double *>(L.sgs.w_stream.get()); q.ycur = L.sgs.w_ycur.get(); q.y = y; q.omega = ctx->omega;
  return q;
}

// prepass_done: r was produced by the level's residual product with the pre-pass in its epilogue (smooth_level)
int sgs_apply(gmg_context *ctx, Level &L, double *y, const double *r, bool prepass_done = false) {
  if (L.sgs.wave) {
    SgsWaveArgs p{};
    p.ranges = L.sgs.w_ranges.get(); p.block_rng = L.sgs.w_block_rng.get(); p.stream = L.sgs.w_stream.get(); p.ws_ci = L.sgs.w_ws_ci.get();
    p.ci_row = L.sgs.w_ci_row.get(); p.ycur = L.sgs.w_ycur.get(); p.y = y; p.omega = ctx->omega; p.y_slots = L.sgs.w_y_slots;
    p.row_ci = L.sgs.w_row_ci.get(); p.rpos_f = L.sgs.w_rpos_f.get(); p.rpos_b = L.sgs.w_rpos_b.get(); p.iso_diag = L.sgs.w_iso_diag.get();
    p.iso_invd = L.sgs.w_iso_invd.get(); p.r = r; p.n_rows = L.n; p.abort_flag = ctx->sgs_abort.get();
    if (!prepass_done) hipLaunchKernelGGL(sgs_wave_prepass_kernel, dim3(grid_for(L.n)), dim3(256), 0, ctx->stream, p);
    // one process per GPU: the blocks are what the reference's ranks sweep -- each rank sweeps its share of them and
    // the pieces of y are all-gathered (levels >= 1 are replicated: every rank needs the whole vector)
    const int n_ranks = ctx->dist ? ctx->comm.n_ranks : 1;
    const bool split = n_ranks > 1 && L.sgs.n_blocks % n_ranks == 0 && !ctx->sgs_profile;
    const int nbl = split ? L.sgs.n_blocks / n_ranks : L.sgs.n_blocks;
    p.block0 = split ? ctx->comm.rank * nbl : 0;
    if (L.sgs.w_n_coupled > 0) {
      if (ctx->sgs_profile && !L.sgs.phased) return sgs_profile_launch(ctx, L, p);
      // sampled like the level-0 SpMV: every prof_every-th sweep launch carries start / stop events; a full pool stops
      // the sampling (no synchronisation ever enters the timed region); stats: launches counted, samples timed
      if (ctx->prof_every > 0 && !ctx->ev_e.empty()) {
        ctx->stats.sgs_launches++;
        if ((ctx->sgs_launch_no++ % (ctx->prof_every | 1)) == 0 && ctx->ev3_used < (int)ctx->ev_e.size()) {  // (odd stride: a V-cycle launches 4 sweeps per level, a stride of 8 would always hit the same one)
          ctx->timed_start = ctx->ev_e[(size_t)ctx->ev3_used].get(); ctx->timed_stop = ctx->ev_f[(size_t)ctx->ev3_used++].get();
          ctx->stats.sgs_substeps += L.sgs.w_steps;
          ctx->stats.sgs_stream_bytes += L.sgs.w_stream_bytes;
        }
      }
      const size_t lds = ctx->sgs_lds_bytes_override > 0 ? (size_t)ctx->sgs_lds_bytes_override : (size_t)L.sgs.w_lds_bytes;
      if (L.sgs.phased) {
        SgsPhaseArgs q{};
        q.ranges = L.sgs.p_ranges.get(); q.blk_tab = L.sgs.p_blk_tab.get(); q.block_rng = p.block_rng; q.block0 = p.block0; q.stream = p.stream; q.ws_ci = p.ws_ci; q.ci_row = p.ci_row;
        q.ycur = p.ycur; q.y = p.y; q.omega = p.omega; q.y_slots = p.y_slots; q.prof = nullptr;
        if (ctx->sgs_phase_profile > 0 && n_ranks == 1 && L.sgs.dep) {
          // diagnostics of the one-dependent-wave sweep: per range, cycles of every wave and how many of them it waited
          const size_t nr = (size_t)L.sgs.w_n_ranges;
          DevPtr<unsigned long long> d;
          std::vector<unsigned long long> h(12 * nr, 0);
          HIPC(d.alloc(12 * nr));
          q.prof = d.get();
          hipLaunchKernelGGL(sgs_dep_kernel, dim3(nbl), dim3(kDpThreads), lds, ctx->stream, q, ctx->sgs_abort.get());
          hipError_t e = hipMemcpyAsync(h.data(), d.get(), sizeof(unsigned long long) * 12 * nr, hipMemcpyDeviceToHost, ctx->stream);
          if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
          if (e != hipSuccess) { ctx->err = std::string("SSOR sweep profile: ") + hipGetErrorString(e); return GMG_ERR_HIP; }
          if (L.sgs.w_steps > 1000 && nbl == 1)
            for (size_t i = 0; i < nr; ++i) {
              const PhRange &P = L.sgs.host_pranges[i];
              std::fprintf(stderr, "[gmg]   %s steps %4d | cycles/step %7.1f | dependent wave waited %5.1f %% | prep waves waited %5.1f %% %5.1f %% %5.1f %%\n", P.backward ? "bwd" : "fwd",
                           P.n_steps, (double)h[12 * i] / std::max(1, P.n_steps), 100.0 * h[12 * i + 1] / std::max<double>(1, h[12 * i]),
                           100.0 * h[12 * i + 3] / std::max<double>(1, h[12 * i + 2]), 100.0 * h[12 * i + 5] / std::max<double>(1, h[12 * i + 4]),
                           100.0 * h[12 * i + 7] / std::max<double>(1, h[12 * i + 6]));
            }
        } else if (ctx->sgs_phase_profile > 0 && n_ranks == 1 && !L.sgs.dep) {  // (several ranks: the option is refused in gmg_set_option; the all-gather below must run)
          // the instrumented variant of the sweep (same arithmetic, same results, s_memtime around every phase); the
          // launch falls through to the common tail like the production one
          const size_t nr = (size_t)L.sgs.w_n_ranges;
          DevPtr<unsigned long long> d;
          std::vector<unsigned long long> h(12 * nr, 0);
          HIPC(d.alloc(12 * nr));
          q.prof = d.get();
#ifdef GMG_EXPERIMENTS
          if (ctx->sgs_chain) hipLaunchKernelGGL(sgs_chain_kernel, dim3(nbl), dim3(kPhThreads), lds, ctx->stream, q, ctx->sgs_abort.get());
          else
#endif
          if (L.sgs.reg) hipLaunchKernelGGL(sgs_regs_kernel, dim3(nbl), dim3(kPhThreads), lds, ctx->stream, q);
          else hipLaunchKernelGGL(sgs_phase_profile_kernel, dim3(nbl), dim3(kPhThreads), lds, ctx->stream, q);
          hipError_t e = hipMemcpyAsync(h.data(), d.get(), sizeof(unsigned long long) * 12 * nr, hipMemcpyDeviceToHost, ctx->stream);
          if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
          if (e != hipSuccess) { ctx->err = std::string("SSOR sweep profile: ") + hipGetErrorString(e); return GMG_ERR_HIP; }
          if (L.sgs.w_steps > 1000 && nbl == 1) {
            std::fprintf(stderr, "[gmg] four-wave sweep (%s), %lld rows: per range dir steps | cycles/step | load+write-back cycles\n",
                         L.sgs.reg ? "records global -> registers; 'reads' = issuing the loads, 'copy' = none" : ctx->sgs_chain ? "hand-over through an LDS word" : "s_barrier per phase", (long long)L.n);
            for (size_t i = 0; i < nr; ++i) {
              const PhRange &P = L.sgs.host_pranges[i];
              const double turns = std::max(1.0, P.n_steps / (double)kPhWaves);
              std::fprintf(stderr, "[gmg]   %s steps %4d | %7.1f | %llu | wave 0 per turn: wait %.0f reads %.0f copy %.0f P2 %.0f CRIT %.0f barriers / polls %.0f\n", P.backward ? "bwd" : "fwd", P.n_steps,
                           (double)h[12 * i] / std::max(1, P.n_steps), h[12 * i + 2] + h[12 * i + 3], h[12 * i + 4] / turns, h[12 * i + 5] / turns, h[12 * i + 6] / turns, h[12 * i + 7] / turns,
                           h[12 * i + 8] / turns, h[12 * i + 9] / turns);
            }
          }
          if (L.sgs.w_steps > 1000 && nbl > 1) {  // several blocks, one per CU: the cycles of each block's ranges
            double c_max = 0, c_sum = 0;
            for (int b = 0; b < nbl; ++b) {
              unsigned long long cyc = 0, xfer = 0;
              int steps = 0;
              for (int i = L.sgs.host_block_rng[(size_t)b]; i < L.sgs.host_block_rng[(size_t)b + 1]; ++i) {
                cyc += h[12 * (size_t)i]; xfer += h[12 * (size_t)i + 2] + h[12 * (size_t)i + 3]; steps += L.sgs.host_pranges[(size_t)i].n_steps;
              }
              std::fprintf(stderr, "[gmg]   block %3d: rows [%d, %d), %d ranges, %d steps, %llu cycles in the steps, %llu load + write-back\n", b, L.sgs.host_block_row[(size_t)b],
                           L.sgs.host_block_row[(size_t)b + 1], L.sgs.host_block_rng[(size_t)b + 1] - L.sgs.host_block_rng[(size_t)b], steps, cyc, xfer);
              c_max = std::max(c_max, (double)(cyc + xfer)); c_sum += (double)(cyc + xfer);
            }
            std::fprintf(stderr, "[gmg] four-wave sweep, %lld rows, %d blocks: longest / mean block (steps + transfers) %.2f\n", (long long)L.n, nbl, c_sum > 0 ? c_max * nbl / c_sum : 1.0);
          }
        } else
        if (L.sgs.dep) {
          if (ctx->timed_start) {  // (two kernel arguments: the one-argument launch_timed does not fit)
            hipExtLaunchKernelGGL(sgs_dep_kernel, dim3(nbl), dim3(kDpThreads), (std::uint32_t)lds, ctx->stream, ctx->timed_start, ctx->timed_stop, 0u, q, ctx->sgs_abort.get());
            ctx->timed_start = ctx->timed_stop = nullptr;
          } else {
            hipLaunchKernelGGL(sgs_dep_kernel, dim3(nbl), dim3(kDpThreads), lds, ctx->stream, q, ctx->sgs_abort.get());
          }
        } else
#ifdef GMG_EXPERIMENTS
        if (ctx->sgs_chain) hipLaunchKernelGGL(sgs_chain_kernel, dim3(nbl), dim3(kPhThreads), lds, ctx->stream, q, ctx->sgs_abort.get());
        else
#endif
        if (L.sgs.reg) launch_timed(ctx, sgs_regs_kernel, dim3(nbl), dim3(kPhThreads), lds, q);
        else launch_timed(ctx, sgs_phase_kernel, dim3(nbl), dim3(kPhThreads), lds, q);
      } else {
        launch_timed(ctx, sgs_wave_kernel<false>, dim3(nbl), dim3(kSwThreads), lds, p);
      }
    }
    if (split) {
      const std::vector<int32_t> &br = L.sgs.host_block_row;
      const int64_t len = L.sgs.w_stage_len;
      auto piece = [&](int r, int64_t *b, int64_t *e) { *b = br[(size_t)(r * nbl)]; *e = br[(size_t)((r + 1) * nbl)]; };
      int64_t b, e;
      piece(ctx->comm.rank, &b, &e);
      double *mine = L.sgs.w_stage.get() + (int64_t)ctx->comm.rank * len;
      if (e > b) HIPC(hipMemcpyAsync(mine, y + b, sizeof(double) * (size_t)(e - b), hipMemcpyDeviceToDevice, ctx->stream));
      if (allgather_chunks(ctx->comm, L.sgs.w_stage.get(), len, ctx->stream)) return fail(ctx, GMG_ERR_COMM, "SSOR: all-gather failed");
      for (int r = 0; r < n_ranks; ++r) {
        if (r == ctx->comm.rank) continue;
        piece(r, &b, &e);
        if (e > b) HIPC(hipMemcpyAsync(y + b, L.sgs.w_stage.get() + (int64_t)r * len, sizeof(double) * (size_t)(e - b), hipMemcpyDeviceToDevice, ctx->stream));
      }
    }
    HIPC(hipGetLastError());
    return GMG_OK;
  }
  HIPC(hipMemsetAsync(y, 0, sizeof(double) * (size_t)L.n, ctx->stream));
  SgsArgs a{};
  a.rowptr = L.A.rowptr.get(); a.col = L.A.col.get(); a.val = L.A.val.get(); a.invd = L.invd.get();
  a.block_row = L.sgs.block_row.get(); a.block_stage = L.sgs.block_stage.get();
  a.stage_ptr = L.sgs.stage_ptr.get(); a.stage_rows = L.sgs.stage_rows.get();
  a.omega = ctx->omega; a.r = r; a.y = y;
  hipLaunchKernelGGL(sgs_sweep_kernel<false>, dim3(L.sgs.n_blocks), dim3(1024), 0, ctx->stream, a);
  hipLaunchKernelGGL(sgs_sweep_kernel<true>, dim3(L.sgs.n_blocks), dim3(1024), 0, ctx->stream, a);
  HIPC(hipGetLastError());
  return GMG_OK;
}

// The Lanczos estimate of lambda_max(D^-1 A) of a level (gmg_lanczos.hpp): m steps enqueued without a host wait, then one
// download of the record.  Scratch: the level's w1 (r), w2 (p), t (A p) and the context's partials and record -- free between two
// smoother calls.  alpha / beta: m entries each or NULL.
int lanczos_estimate(gmg_context *ctx, Level &L, int level, int m, double *ritz, double *alpha, double *beta, int *steps_run) {
  if (!L.A.valid || !L.invd) return fail(ctx, GMG_ERR_INVALID, "Lanczos estimate: the level matrix has not been set");
  if (L.A.halo.active || (level == 0 && l0_partitioned(ctx)))
    return fail(ctx, GMG_ERR_UNSUPPORTED, "Lanczos estimate: a row-partitioned operator (the estimate has no communication)");
  if (m < 1 || m > lanczos::kMaxSteps) return fail(ctx, GMG_ERR_INVALID, "Lanczos estimate: 1 .. 64 steps");
  std::vector<double> rec(2 * (size_t)m + 2, 0.0);
  if (L.n > 0) {
    double *d_rec = ctx->lanczos_rec.get();
    HIPC(hipMemsetAsync(d_rec, 0, sizeof(double) * lanczos::record_len(m), ctx->stream));
    lanczos::Args a{};
    a.r = L.w1.get(); a.p = L.w2.get(); a.q = L.t.get(); a.invd = L.invd.get(); a.n = L.n;
    a.n_part = grid_for(L.n);
    a.part_pq = ctx->part_a.get(); a.part_rho = ctx->part_b.get(); a.rec = d_rec; a.m = m;
    const int g = ctx->lanczos_max_blocks > 0 ? std::min(a.n_part, ctx->lanczos_max_blocks) : a.n_part;
    hipLaunchKernelGGL(lanczos::lanczos_start_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, a);
    for (int j = 0; j < m; ++j) {
      a.j = j;
      CHK(spmv(ctx, L.A, kStore, L.w2.get(), L.t.get()));
      hipLaunchKernelGGL(lanczos::lanczos_pq_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, a);
      hipLaunchKernelGGL(lanczos::lanczos_r_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, a);
      hipLaunchKernelGGL(lanczos::lanczos_p_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, a);
    }
    CHK(launch_status(ctx));
    HIPC(hipMemcpyAsync(rec.data(), d_rec, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(stream_wait(ctx->stream));  // (the one host wait of the estimate)
  }
  const int run = std::min(m, std::max(0, (int)rec[0]));
  if (steps_run) *steps_run = run;
  if (ritz) *ritz = lanczos::ritz_value(rec.data() + 2, rec.data() + 2 + m, run);
  for (int j = 0; j < m; ++j) {
    if (alpha) alpha[j] = j < run ? rec[2 + (size_t)j] : 0.0;
    if (beta) beta[j] = j < run ? rec[2 + (size_t)m + (size_t)j] : 0.0;
  }
  return GMG_OK;
}

// the bound the Chebyshev smoother uses on a level: the user's, else min(safety ritz, Gershgorin) where the Lanczos bound is
// selected and has been formed (cheb_prepare), else Gershgorin
double cheb_lambda(const gmg_context *ctx, const Level &L) {
  if (ctx->cheb_lmax_user > 0) return ctx->cheb_lmax_user;
  if (ctx->cheb_lmax_source == GMG_CHEB_LMAX_LANCZOS && L.cheb_est.valid && L.cheb_est.steps_run > 0) {
    const double s = ctx->cheb_safety * L.cheb_est.ritz;
    return L.cheb_lmax > 0 ? std::min(s, L.cheb_lmax) : s;
  }
  return L.cheb_lmax;
}

// before a level's Chebyshev steps: form the Lanczos bound if it is wanted and the level has none yet (one host wait, once
// per level matrix)
int cheb_prepare(gmg_context *ctx, Level &L, int level) {
  if (ctx->cheb_lmax_source != GMG_CHEB_LMAX_LANCZOS || ctx->cheb_lmax_user > 0 || L.cheb_est.valid) return GMG_OK;
  Level::ChebEstimate e;
  CHK(lanczos_estimate(ctx, L, level, ctx->cheb_lanczos_steps, &e.ritz, nullptr, nullptr, &e.steps_run));
  e.valid = true;
  L.cheb_est = e;
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] level %d Chebyshev bound: Gershgorin %.6f, Ritz value %.6f after %d of %d Lanczos steps, lambda in use %.6f\n", level, L.cheb_lmax,
                 e.ritz, e.steps_run, ctx->cheb_lanczos_steps, cheb_lambda(ctx, L));
  return GMG_OK;
}

// y = S r for the Chebyshev "preconditioner" (Ifpack_Chebyshev recurrence, zero start).
// Result lands in *out (one of L.w1 / L.w3).
int cheb_apply(gmg_context *ctx, Level &L, const double *r, double **out) {
  const double lmax = cheb_lambda(ctx, L);
  const int degree = ctx->cheb_degree_opt > 0 ? ctx->cheb_degree_opt : ctx->cheb_degree;
  if (ctx->cheb_polynomial == GMG_CHEB_FOURTH_KIND) {
    // fourth-kind polynomial (Lottes 2022): d = (4 / (3 lmax)) B r, y = d; then for j = 1 .. k - 1
    //   d = ((2 j - 1) / (2 j + 3)) d + ((8 j + 4) / ((2 j + 3) lmax)) B (r - A y),  y += d
    // -- the first-kind recurrence's kernels with other scalars; cheb_ratio is not read
    double *y = L.w1.get(), *yn = L.w3.get(), *w = L.w2.get();
    hipLaunchKernelGGL(cheb_first_kernel, dim3(grid_for(L.n)), dim3(kThreads), 0, ctx->stream, y, w, r, (const double *)L.invd.get(),
                       0.75 * lmax, L.n);
    for (int j = 1; j < degree; ++j) {
      CHK(import_ghosts(ctx, L.A, y));
      SpmvArgs a = base_args(L.A, y, yn);
      a.b = r; a.invd = L.invd.get(); a.w = w;
      a.c1 = (2.0 * j - 1.0) / (2.0 * j + 3.0);
      a.omega = (8.0 * j + 4.0) / ((2.0 * j + 3.0) * lmax);
      launch_spmv_mode<kCheb>(ctx, L.A, a);
      std::swap(y, yn);
    }
    *out = y;
    return GMG_OK;
  }
  const double alpha = lmax / ctx->cheb_ratio, beta = lmax;
  const double delta = 2.0 / (beta - alpha), theta = 0.5 * (beta + alpha), s1 = theta * delta;
  double rhok = 1.0 / s1;
  double *y = L.w1.get(), *yn = L.w3.get(), *w = L.w2.get();
  hipLaunchKernelGGL(cheb_first_kernel, dim3(grid_for(L.n)), dim3(kThreads), 0, ctx->stream, y, w, r, (const double *)L.invd.get(),
                     theta, L.n);
  for (int deg = 1; deg < degree; ++deg) {
    const double rhokp1 = 1.0 / (2.0 * s1 - rhok);
    const double d1 = rhokp1 * rhok, d2 = 2.0 * rhokp1 * delta;
    rhok = rhokp1;
    CHK(import_ghosts(ctx, L.A, y));
    SpmvArgs a = base_args(L.A, y, yn);
    a.b = r; a.invd = L.invd.get(); a.w = w; a.omega = d2; a.c1 = d1;
    launch_spmv_mode<kCheb>(ctx, L.A, a);
    std::swap(y, yn);
  }
  *out = y;
  return GMG_OK;
}

// MGSmootherPrecondition::apply (from_zero) / ::smooth on level l; u and rhs are level vectors.
// Jacobi steps run out of place; u_io may come back holding the level's spare buffer (and spare_io what u_io held).
int smooth_level(gmg_context *ctx, int l, DevPtr<double> &u_io, const double *rhs, bool from_zero, DevPtr<double> &spare_io) {
  Level &L = ctx->lv[(size_t)l];
  double *u = u_io.get(), *spare = spare_io.get();
  const int g = grid_for(L.n);
  int first = 0;
  if (ctx->smoother == GMG_SMOOTHER_CHEBYSHEV && ctx->steps > 0) CHK(cheb_prepare(ctx, L, l));
  if (from_zero && ctx->steps > 0) {
    first = 1;
    if (ctx->smoother == GMG_SMOOTHER_JACOBI) {
      hipLaunchKernelGGL(vec_scale_mul_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, u, ctx->omega, rhs,
                         (const double *)L.invd.get(), L.n);
    } else if (ctx->smoother == GMG_SMOOTHER_SSOR) {
      CHK(sgs_apply(ctx, L, u, rhs));
    } else {
      double *y = nullptr;
      CHK(cheb_apply(ctx, L, rhs, &y));
      hipLaunchKernelGGL(vec_equ_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, u, 1.0, (const double *)y, L.n);
    }
  }
  for (int s = first; s < ctx->steps; ++s) {
    CHK(import_ghosts(ctx, L.A, u));
    if (ctx->smoother == GMG_SMOOTHER_JACOBI) {
      SpmvArgs a = base_args(L.A, u, spare);
      a.b = rhs; a.invd = L.invd.get(); a.omega = ctx->omega;
      launch_spmv_mode<kJacobi>(ctx, L.A, a);
      std::swap(u, spare);
    } else {
      // SSOR on the row-window kernel: the sweep's pre-pass (r into the record stream, the closed form of rows without
      // couplings) rides in the epilogue of the product that forms r
      const bool pre = ctx->smoother == GMG_SMOOTHER_SSOR && L.sgs.wave && !ctx->dist && !ctx->disable_vcycle_fused && L.A.valid && !L.A.sell &&
                       !L.A.lat_only && !L.A.halo.active && L.A.n_rows == L.n;
      if (pre) {
        SpmvArgs a = base_args(L.A, u, L.t.get());
        a.b = rhs; a.pre = sgs_pre_args(ctx, L, L.w1.get());
        launch_timed(ctx, spmv_tile_kernel<kResidPre, 0>, dim3(L.A.grid), dim3(kThreads), 0, a);
        CHK(launch_status(ctx));
      } else {
        CHK(spmv(ctx, L.A, kResid, u, L.t.get(), nullptr, rhs));  // r = rhs - A u
      }
      if (ctx->smoother == GMG_SMOOTHER_SSOR) {
        CHK(sgs_apply(ctx, L, L.w1.get(), L.t.get(), pre));
        hipLaunchKernelGGL(vec_add_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, u, 1.0, (const double *)L.w1.get(), L.n);
      } else {
        double *y = nullptr;
        CHK(cheb_apply(ctx, L, L.t.get(), &y));
        hipLaunchKernelGGL(vec_add_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, u, 1.0, (const double *)y, L.n);
      }
    }
  }
  if (u != u_io.get()) std::swap(u_io, spare_io);
  return launch_status(ctx);
}

// Sample i brackets iteration i * prof_every of the solve just finished.  Iterations at or beyond the
// converged count returned at once: their event time is the cost of the bracket itself (launch gap +
// an early-exit kernel) and is kept apart, so that bench.py can take it off the live launches.
void collect_profile_samples(gmg_context *ctx) {
  const int iters = ctx->st_final.iters;
  for (int i = 0; i < ctx->ev_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev_a[(size_t)i].get(), ctx->ev_b[(size_t)i].get()) != hipSuccess) continue;
    if (i * ctx->prof_every < iters) {
      ctx->stats.spmv0_ms_total += ms;
      ctx->stats.spmv0_samples++;
    } else {
      ctx->stats.spmv0_noop_ms_total += ms;
      ctx->stats.spmv0_noop_samples++;
    }
  }
  for (int i = 0; i < ctx->ev2_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev_c[(size_t)i].get(), ctx->ev_d[(size_t)i].get()) != hipSuccess) continue;
    if (i * ctx->prof_every < iters) {
      ctx->stats.cgupd_ms_total += ms;
      ctx->stats.cgupd_samples++;
    }
  }
}

constexpr int64_t kUnfusedMinRowsDecl = 200000;

// Enqueues coarse-CG iterations in chunks and watches the 64-byte device state.  The first
// chunk is sized from the previous solve (zero-start solves of one hierarchy need nearly the
// same number of iterations); while the host waits for a chunk's state, the NEXT chunk is
// already queued, so the GPU never idles on the host round trip -- iterations enqueued after
// convergence return at once (the `done` flag, ~1 us each).
// `later_default`: iterations per follow-up chunk; it only has to outlast the host's poll-and-enqueue
// round trip (~30 us), so long iterations (large level 0) take short chunks and waste fewer no-ops.
template <class EnqueueOne>
int run_cg_chunks(gmg_context *ctx, int later_default, EnqueueOne enqueue_one) {
  const int maxit = ctx->coarse_maxit;
  const int last = ctx->last_coarse_iters;
  const int first = ctx->coarse_chunk > 0 ? ctx->coarse_chunk : (last > 8 ? last - (later_default < 6 ? std::max(2, last / 4) : 2) : 16);
  const int later = ctx->coarse_chunk > 0 ? ctx->coarse_chunk : later_default;
  int launched = 0;
  auto launch_chunk = [&](int n, int slot) -> int {
    for (int q = 0; q < n; ++q) {
      const int rc = enqueue_one(launched++);
      if (rc != GMG_OK) return rc;
    }
    CHK(launch_status(ctx));
    HIPC(hipMemcpyAsync(&ctx->st_host.get()[slot], ctx->st.get(), sizeof(CGState), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipEventRecord(ctx->ev_chunk[slot].get(), ctx->stream));
    return GMG_OK;
  };
  int slot = 0;
  CHK(launch_chunk(std::min(first, maxit + 1), slot));
  // over RCCL the no-op iterations after convergence would still run their collectives: not worth it across ranks; over
  // the peer transport they return at once like on one GPU
  const bool speculate = !l0_partitioned(ctx) || ctx->comm.peer;
  for (;;) {
    if (speculate) CHK(launch_chunk(later, slot ^ 1));
    for (;;) {
      const hipError_t e = hipEventQuery(ctx->ev_chunk[slot].get());
      if (e == hipSuccess) break;
      if (e != hipErrorNotReady) { ctx->err = std::string("hipEventQuery: ") + hipGetErrorString(e); return GMG_ERR_HIP; }
    }
    if (ctx->st_host.get()[slot].done) { ctx->st_final = ctx->st_host.get()[slot]; ctx->stats.coarse_enqueued += launched; break; }
    if (launched > maxit + 2 * later + 2) return fail(ctx, GMG_ERR_HIP, "coarse CG state machine did not terminate");
    if (!speculate) CHK(launch_chunk(later, slot ^ 1));
    slot ^= 1;
  }
  return GMG_OK;
}  // == kUnfusedMinRows in gmg_dist.hpp

// ---- coarse solver (A9): device-resident classic CG on level 0 -----------------------------

int coarse_solve_unfused(gmg_context *ctx, double *x, const double *b, int *iters_out, double *res_out);
void collect_profile_samples(gmg_context *ctx);
int coarse_solve_direct(gmg_context *ctx, double *x, const double *b, int *iters_out, double *res_out, Event *pass_ev = nullptr);

int coarse_solve(gmg_context *ctx, double *x, const double *b, int *iters_out, double *res_out) {
  Level &L0 = ctx->lv[0];
  const DevCSR &A = L0.A;
  if (!A.valid) return fail(ctx, GMG_ERR_INVALID, "level-0 matrix not set");
  if (ctx->coarse_solver == GMG_COARSE_DIRECT) return coarse_solve_direct(ctx, x, b, iters_out, res_out);
  int variant = ctx->cg_variant;
  if (l0_partitioned(ctx) || (variant == 0 && L0.n >= kUnfusedMinRowsDecl) || variant == 2 || A.lat_only)
  {
    ctx->stats.coarse_variant = 2;
    ctx->stats.coarse_solver = GMG_COARSE_CG;
    return coarse_solve_unfused(ctx, x, b, iters_out, res_out);
  }
  ctx->stats.coarse_variant = 1;
  ctx->stats.coarse_solver = GMG_COARSE_CG;
  const int64_t n = L0.n;
  const int g_upd = grid_for((n / 2 + 0));
  const int g_init = grid_for(n);
  CGInitArgs ia{b, x, ctx->cg_g.get(), ctx->cg_d0.get(), ctx->cg_d1.get(), n, ctx->st.get(), ctx->part_b.get()};
  hipLaunchKernelGGL(cg_init_kernel, dim3(g_init), dim3(kThreads), 0, ctx->stream, ia);
  int n_part_gg = g_init;
  const int maxit = ctx->coarse_maxit;
  ctx->ev_used = 0; ctx->ev2_used = 0;
  CHK(run_cg_chunks(ctx, 6, [&](int launched) -> int {
    const bool odd = launched & 1;
    SpmvArgs a = base_args(A, odd ? ctx->cg_d1.get() : ctx->cg_d0.get(), ctx->cg_h.get());
    a.g = ctx->cg_g.get();
    a.dnew = odd ? ctx->cg_d0.get() : ctx->cg_d1.get();
    a.st = ctx->st.get();
    a.part_in = ctx->part_b.get(); a.n_part_in = n_part_gg;
    a.part_out = ctx->part_a.get();
    a.tol = ctx->coarse_tol; a.maxit = maxit;
    const bool sample = ctx->prof_every > 0 && (launched % ctx->prof_every) == 0 && ctx->ev_used < (int)ctx->ev_a.size();
    if (sample) { ctx->timed_start = ctx->ev_a[(size_t)ctx->ev_used].get(); ctx->timed_stop = ctx->ev_b[(size_t)ctx->ev_used++].get(); }
    const int n_part_dh = launch_op<kStore, 1>(ctx, A, a);
    CGUpdateArgs ua{x, ctx->cg_g.get(), a.dnew, ctx->cg_h.get(), n, ctx->st.get(), ctx->part_a.get(), n_part_dh, ctx->part_b.get()};
    const bool sample2 = sample && ctx->ev2_used < (int)ctx->ev_c.size();
    if (sample2) { ctx->timed_start = ctx->ev_c[(size_t)ctx->ev2_used].get(); ctx->timed_stop = ctx->ev_d[(size_t)ctx->ev2_used++].get(); }
    launch_timed(ctx, cg_update_kernel, dim3(g_upd), dim3(kThreads), 0, ua);
    n_part_gg = g_upd;
    return GMG_OK;
  }));
  collect_profile_samples(ctx);
  ctx->last_coarse_iters = ctx->st_final.iters;
  ctx->stats.coarse_solves++;
  ctx->stats.coarse_iterations += ctx->st_final.iters;
  if (iters_out) *iters_out = ctx->st_final.iters;
  if (res_out) *res_out = ctx->st_final.res;
  if (ctx->st_final.status != 0) return fail(ctx, GMG_ERR_COARSE_NOCONV, "coarse CG did not converge within max_it");
  return GMG_OK;
}


// ---- direct coarse solver (gmg_fastdiag.hpp): six transforms, one of them with the D^-1 scaling, and the boundary rows ----

void drop_coarse_direct(gmg_context *ctx) {
  ctx->fd = FastDiag();
  ctx->coarse_solver = GMG_COARSE_CG;
}

// GMG_COARSE_DIRECT if level 0 qualifies (tables uploaded, scratch allocated); otherwise GMG_ERR_UNSUPPORTED with the
// reason, and the context stays with the coarse CG
int select_coarse_direct(gmg_context *ctx) {
  drop_coarse_direct(ctx);
  Level &L0 = ctx->lv[0];
  const DevCSR &m = L0.A;
  if (!m.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_set_coarse_solver: level-0 matrix not set");
  if (l0_partitioned(ctx)) return fail(ctx, GMG_ERR_UNSUPPORTED, "level 0 is partitioned over the ranks");
  if (!m.lat_only) return fail(ctx, GMG_ERR_UNSUPPORTED, "level 0 was not formed by gmg_set_level_matrix_lattice");
  for (int d = 0; d < 3; ++d)  // (gmg_set_level_matrix_lattice takes no fewer than 5)
    if (m.lat_nv[d] > fastdiag::kMaxNv) return fail(ctx, GMG_ERR_UNSUPPORTED, "level 0 has more than 1024 vertices in a direction");
  double s = 0.0;
  if (!fastdiag::separable(m.lat_Ke, &s)) return fail(ctx, GMG_ERR_UNSUPPORTED, "the level-0 cell matrix is not the separable constant-coefficient Q1 Laplacian");
  (void)hipSetDevice(ctx->device);
  FastDiag fd;
  fd.s = s;
  std::vector<double> S, Sp, lam, mu;
  for (int d = 0; d < 3; ++d) {
    const int mm = m.lat_nv[d] - 2, ld = (mm + fastdiag::kPad - 1) / fastdiag::kPad * fastdiag::kPad;
    fd.m[d] = mm; fd.ld[d] = ld;
    S.assign((size_t)mm * mm, 0.0); lam.assign((size_t)mm, 0.0); mu.assign((size_t)mm, 0.0);
    fastdiag::tables(mm + 1, S.data(), lam.data(), mu.data());
    Sp.assign((size_t)ld * ld, 0.0);
    for (int j = 0; j < mm; ++j) std::copy(S.begin() + (size_t)j * mm, S.begin() + (size_t)(j + 1) * mm, Sp.begin() + (size_t)j * ld);
    HIPC(upload(fd.S[d], Sp, ctx->stream));
    HIPC(upload(fd.lam[d], lam, ctx->stream));
    HIPC(upload(fd.mu[d], mu, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));  // (the host tables are reused by the next axis)
  }
  CHK(alloc_vec(ctx, fd.t1, L0.n));
  CHK(alloc_vec(ctx, fd.t2, L0.n));
  HIPC(hipStreamSynchronize(ctx->stream));
  fd.ready = true;
  ctx->fd = std::move(fd);
  ctx->coarse_solver = GMG_COARSE_DIRECT;
  return GMG_OK;
}

// one pass: dst <- S_axis src on the interior (scale: divided by D_abc as well; axis 2 only)
void launch_fastdiag_pass(gmg_context *ctx, int axis, double *dst, const double *src, bool scale) {
  const FastDiag &fd = ctx->fd;
  const DevCSR &m = ctx->lv[0].A;
  fastdiag::PassArgs a{};
  a.src = src; a.dst = dst;
  for (int d = 0; d < 3; ++d) a.ax[d] = fastdiag::Axis{fd.S[d].get(), fd.lam[d].get(), fd.mu[d].get(), fd.m[d], fd.ld[d]};
  a.nx = m.lat_nx; a.nxy = m.lat_nxy; a.axis = axis; a.s = fd.s;
  // panels of 16 lines, one per wave
  const int64_t panels = axis == 0 ? (int64_t)((fd.m[1] + 15) / 16) * fd.m[2] : (int64_t)((fd.m[0] + 15) / 16) * fd.m[3 - axis];
  int64_t grid = std::min<int64_t>((panels + 3) / 4, 8192);
  if (ctx->coarse_direct_max_blocks > 0) grid = std::min<int64_t>(grid, ctx->coarse_direct_max_blocks);
  grid = std::max<int64_t>(grid, 1);
  if (axis == 0) launch_timed(ctx, fastdiag::fastdiag_pass_x_kernel, dim3((unsigned)grid), dim3(kThreads), 0, a);
  else if (scale) launch_timed(ctx, fastdiag::fastdiag_pass_yz_kernel<true>, dim3((unsigned)grid), dim3(kThreads), 0, a);
  else launch_timed(ctx, fastdiag::fastdiag_pass_yz_kernel<false>, dim3((unsigned)grid), dim3(kThreads), 0, a);
}

int coarse_solve_direct(gmg_context *ctx, double *x, const double *b, int *iters_out, double *res_out, Event *pass_ev) {
  Level &L0 = ctx->lv[0];
  const DevCSR &A = L0.A;
  FastDiag &fd = ctx->fd;
  if (!fd.ready || !A.lat_only || l0_partitioned(ctx)) return fail(ctx, GMG_ERR_INVALID, "direct coarse solver selected without its tables, or on a partitioned level 0");
  double *t1 = fd.t1.get(), *t2 = fd.t2.get();
  // launch k carries the events of pass_ev[k] when the caller asked for the passes' own times (gmg_coarse_direct_profile)
  int k = 0;
  auto arm = [&]() {
    if (pass_ev) { ctx->timed_start = pass_ev[2 * k].get(); ctx->timed_stop = pass_ev[2 * k + 1].get(); }
    ++k;
  };
  arm(); launch_fastdiag_pass(ctx, 0, t1, b, false);
  arm(); launch_fastdiag_pass(ctx, 1, t2, t1, false);
  arm(); launch_fastdiag_pass(ctx, 2, t1, t2, true);   // forward along z, then D^-1
  arm(); launch_fastdiag_pass(ctx, 2, t2, t1, false);
  arm(); launch_fastdiag_pass(ctx, 1, t1, t2, false);
  arm(); launch_fastdiag_pass(ctx, 0, x, t1, false);
  int grid = grid_for(L0.n);
  if (ctx->coarse_direct_max_blocks > 0) grid = std::min(grid, ctx->coarse_direct_max_blocks);
  arm();
  launch_timed(ctx, fastdiag::fastdiag_boundary_kernel, dim3(grid), dim3(kThreads), 0, x, b, (const uint8_t *)A.lat_rowcls.get(), (const double *)A.lat_ctab.get(), A.lat_nv[0],
               A.lat_nv[1], A.lat_nv[2]);
  ctx->stats.coarse_solves++;
  ctx->stats.coarse_solver = GMG_COARSE_DIRECT;
  ctx->last_coarse_iters = 0;
  if (iters_out) *iters_out = 0;
  if (res_out) {
    // the true |b - A x|_2: one lattice product and the norm kernels (level 0 is whole on this rank: no all-reduce)
    CHK(spmv(ctx, A, kStore, x, t1));
    const int g = grid_for(L0.n);
    hipLaunchKernelGGL(vec_sadd_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, t1, -1.0, 1.0, b, L0.n);
    hipLaunchKernelGGL(norms_partial_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, (const double *)t1, L0.n, ctx->part_a.get());
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double *)ctx->part_a.get(), g, 4, 4u, ctx->scal_dev.get());
    CHK(launch_status(ctx));
    CHK(fetch_scalars(ctx, 4));
    *res_out = std::sqrt(ctx->scal_host.get()[1]);
    return GMG_OK;
  }
  return launch_status(ctx);
}


// ---- canonical row partition of distributed runs: equal chunks, rank r owns
// [r*chunk, min((r+1)*chunk, n)); chosen so that ncclAllGather can rebuild a replica in place.
inline int64_t part_chunk(int64_t n, int n_ranks) { return (n + n_ranks - 1) / n_ranks; }
inline void part_range(int64_t n, int rank, int n_ranks, int64_t *b, int64_t *e) {
  const int64_t c = part_chunk(n, n_ranks);
  *b = std::min<int64_t>(n, (int64_t)rank * c);
  *e = std::min<int64_t>(n, (int64_t)(rank + 1) * c);
}

// full[0 .. n_global) <- concatenation of every rank's owned slice (local[0 .. n_owned))
int allgather_full(gmg_context *ctx, double *full, const double *local, int64_t n_global) {
  const int64_t c = part_chunk(n_global, ctx->comm.n_ranks);
  int64_t b, e;
  part_range(n_global, ctx->comm.rank, ctx->comm.n_ranks, &b, &e);
  // stage the owned slice at its place; the padded tail of the last chunks is never read
  if (e > b) HIPC(hipMemcpyAsync(full + b, local, sizeof(double) * (size_t)(e - b), hipMemcpyDeviceToDevice, ctx->stream));
  if (allgather_chunks(ctx->comm, full, c, ctx->stream)) return fail(ctx, GMG_ERR_COMM, "all-gather failed");
  return GMG_OK;
}

// MGCoarseGridBase::operator() as the V-cycle sees it: replicated defect in, replicated solution out
int coarse_level_solve(gmg_context *ctx) {
  Level &L0 = ctx->lv[0];
  if (!l0_partitioned(ctx)) return coarse_solve(ctx, L0.sol.get(), L0.def.get(), nullptr, nullptr);
  int64_t b, e;
  part_range(ctx->l0_global, ctx->comm.rank, ctx->comm.n_ranks, &b, &e);
  if (e > b) HIPC(hipMemcpyAsync(L0.def.get(), L0.def_full + b, sizeof(double) * (size_t)(e - b), hipMemcpyDeviceToDevice, ctx->stream));
  CHK(coarse_solve(ctx, L0.sol.get(), L0.def.get(), nullptr, nullptr));
  return allgather_full(ctx, L0.sol_full, L0.sol.get(), ctx->l0_global);
}

// ---- V-cycle (A5, A6, A8) -----------------------------------------------------------------

int level_v_step(gmg_context *ctx, int l) {
  Level &L = ctx->lv[(size_t)l];
  if (l == 0) return coarse_level_solve(ctx);
  Level &C = ctx->lv[(size_t)l - 1];
  double *c_def = (l == 1) ? C.def_full : C.def.get();
  const int g = grid_for(L.n);
  CHK(smooth_level(ctx, l, L.sol, L.def.get(), true, L.w1));  // pre_smooth->apply (Jacobi may swap sol <-> w1)
  if (L.has_I) {
    CHK(spmv(ctx, L.A, kStore, L.sol.get(), L.t.get()));                 // t = A u
    if (!ctx->dist && !ctx->disable_vcycle_fused) {
      // edge_out->vmult_add and t.sadd(-1, 1, defect) in the product's epilogue: row by row t = defect - (t + I u), the same
      // two additions in the same order (-t + defect and defect - t are the same IEEE operation)
      CHK(spmv(ctx, L.I, kResid, L.sol.get(), L.t.get(), L.t.get(), L.def.get()));
    } else {
      CHK(spmv(ctx, L.I, kStore, L.sol.get(), L.t.get(), L.t.get()));            // edge_out->vmult_add
      hipLaunchKernelGGL(vec_sadd_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, L.t.get(), -1.0, 1.0, (const double *)L.def.get(), L.n);
    }
  } else {
    CHK(spmv(ctx, L.A, kResid, L.sol.get(), L.t.get(), nullptr, L.def.get()));  // t = defect - A u
  }
  CHK(spmv(ctx, C.Pt, kStore, L.t.get(), c_def, c_def));            // restrict_and_add
  CHK(level_v_step(ctx, l - 1));
  const double *c_sol = (l == 1) ? C.sol_full : C.sol.get();        // read AFTER the recursion: Jacobi swaps C.sol
  CHK(spmv(ctx, C.P, kAddTo, c_sol, L.sol.get(), nullptr, L.sol.get()));  // u += P u_c
  if (L.has_I) {
    CHK(spmv(ctx, L.It, kResid, L.sol.get(), L.def.get(), nullptr, L.def.get()));  // defect -= I^T u
  }
  CHK(smooth_level(ctx, l, L.sol, L.def.get(), false, L.w1));     // post_smooth->smooth
  return GMG_OK;
}

// Inverse indices of the levels' copy lists for mg_copy_to_kernel / mg_copy_from_kernel, rebuilt when a list, a level size or
// the system size changed.  mgcopy_ok stays false (the V-cycle then copies list by list) when an index lies outside its
// vector or there are more than kMgMaxLevels levels.
int mg_copy_tables(gmg_context *ctx) {
  std::vector<int64_t> sig{ctx->S.n_rows};
  for (const Level &L : ctx->lv) { sig.push_back(L.n_vec); sig.push_back(L.n_copy); sig.push_back(L.copy_version); }
  if (sig == ctx->mgcopy_sig) return GMG_OK;
  ctx->mgcopy_sig = sig;
  ctx->mgcopy_ok = false;
  const int64_t n_sys = ctx->S.n_rows;
  if (ctx->n_levels > kMgMaxLevels) return GMG_OK;
  int64_t total = 0;
  for (const Level &L : ctx->lv) total += L.n_vec;
  std::vector<int32_t> to((size_t)std::max<int64_t>(total, 1), -1), from_level((size_t)std::max<int64_t>(n_sys, 1), -1), from_row((size_t)std::max<int64_t>(n_sys, 1), 0);
  int64_t off = 0;
  for (int l = 0; l < ctx->n_levels; ++l) {  // (ascending, as the loops of vcycle: a system DoF on two levels takes the later one)
    const Level &L = ctx->lv[(size_t)l];
    if ((int64_t)L.host_copy_g.size() != L.n_copy) return GMG_OK;
    for (int64_t k = 0; k < L.n_copy; ++k) {
      const int64_t g = L.host_copy_g[(size_t)k], r = L.host_copy_l[(size_t)k];
      if (g < 0 || g >= n_sys || r < 0 || r >= L.n_vec) return GMG_OK;
      to[(size_t)(off + r)] = (int32_t)g;
      from_level[(size_t)g] = l;
      from_row[(size_t)g] = (int32_t)r;
    }
    off += L.n_vec;
  }
  HIPC(ctx->mgcopy_to.alloc(to.size()));
  HIPC(ctx->mgcopy_from_level.alloc(from_level.size()));
  HIPC(ctx->mgcopy_from_row.alloc(from_row.size()));
  HIPC(hipMemcpyAsync(ctx->mgcopy_to.get(), to.data(), sizeof(int32_t) * to.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(ctx->mgcopy_from_level.get(), from_level.data(), sizeof(int32_t) * from_level.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(ctx->mgcopy_from_row.get(), from_row.data(), sizeof(int32_t) * from_row.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));  // (the host tables die here)
  ctx->mgcopy_ok = true;
  return GMG_OK;
}

int vcycle(gmg_context *ctx, double *dst, const double *src) {
  if (!ctx->S.valid) return fail(ctx, GMG_ERR_INVALID, "system matrix not set");
  const double *src_v = src;
  double *dst_v = dst;
  int64_t n_sys = ctx->S.n_rows;
  if (ctx->dist) {  // PreconditionMG sees replicas of the outer vectors; only level 0 stays partitioned
    CHK(allgather_full(ctx, ctx->sys_full_a.get(), src, ctx->sys_global));
    src_v = ctx->sys_full_a.get();
    dst_v = ctx->sys_full_b.get();
    n_sys = ctx->sys_global;
  }
  bool fused = !ctx->dist && !ctx->disable_vcycle_fused;
  if (fused) {
    CHK(mg_copy_tables(ctx));
    fused = ctx->mgcopy_ok;
  }
  MgCopyArgs mc{};
  if (fused) {
    mc.n_levels = ctx->n_levels; mc.to = ctx->mgcopy_to.get(); mc.src = src_v;
    mc.from_level = ctx->mgcopy_from_level.get(); mc.from_row = ctx->mgcopy_from_row.get(); mc.dst = dst_v; mc.n_sys = n_sys;
    for (int l = 0; l < ctx->n_levels; ++l) {
      Level &L = ctx->lv[(size_t)l];
      if (!L.A.valid) return fail(ctx, GMG_ERR_INVALID, "level matrix not set");
      mc.def[l] = (l == 0) ? L.def_full : L.def.get();
      mc.sol[l] = L.sol.get();
      mc.off[l + 1] = mc.off[l] + L.n_vec;
    }
    if (mc.off[ctx->n_levels] > 0) hipLaunchKernelGGL(mg_copy_to_kernel, dim3(grid_for(mc.off[ctx->n_levels])), dim3(kThreads), 0, ctx->stream, mc);
  }
  for (int l = 0; l < ctx->n_levels && !fused; ++l) {  // copy_to_mg
    Level &L = ctx->lv[(size_t)l];
    if (!L.A.valid) return fail(ctx, GMG_ERR_INVALID, "level matrix not set");
    double *def = (l == 0) ? L.def_full : L.def.get();
    const int64_t nl = (l == 0 && l0_partitioned(ctx)) ? ctx->l0_global : L.n_vec;
    HIPC(hipMemsetAsync(def, 0, sizeof(double) * (size_t)nl, ctx->stream));
    if (l > 0) HIPC(hipMemsetAsync(L.sol.get(), 0, sizeof(double) * (size_t)L.n_vec, ctx->stream));
    if (L.n_copy)
      hipLaunchKernelGGL(gather_scatter_kernel, dim3(grid_for(L.n_copy)), dim3(kThreads), 0, ctx->stream, def,
                         (const int32_t *)L.copy_l.get(), src_v, (const int32_t *)L.copy_g.get(), L.n_copy);
  }
  CHK(level_v_step(ctx, ctx->n_levels - 1));
  if (fused) {  // (the levels' solutions: read after the cycle, Jacobi swaps sol <-> w1)
    for (int l = 0; l < ctx->n_levels; ++l) mc.sol[l] = (l == 0) ? ctx->lv[0].sol_full : ctx->lv[(size_t)l].sol.get();
    if (n_sys > 0) hipLaunchKernelGGL(mg_copy_from_kernel, dim3(grid_for(n_sys)), dim3(kThreads), 0, ctx->stream, mc);
  } else {
    HIPC(hipMemsetAsync(dst_v, 0, sizeof(double) * (size_t)n_sys, ctx->stream));  // copy_from_mg: dst = 0
  }
  for (int l = 0; l < ctx->n_levels && !fused; ++l) {
    Level &L = ctx->lv[(size_t)l];
    const double *sol = (l == 0) ? L.sol_full : L.sol.get();
    if (L.n_copy)
      hipLaunchKernelGGL(gather_scatter_kernel, dim3(grid_for(L.n_copy)), dim3(kThreads), 0, ctx->stream, dst_v,
                         (const int32_t *)L.copy_g.get(), sol, (const int32_t *)L.copy_l.get(), L.n_copy);
  }
  if (ctx->dist) {
    int64_t b, e;
    part_range(ctx->sys_global, ctx->comm.rank, ctx->comm.n_ranks, &b, &e);
    if (e > b) HIPC(hipMemcpyAsync(dst, dst_v + b, sizeof(double) * (size_t)(e - b), hipMemcpyDeviceToDevice, ctx->stream));
  }
  ctx->stats.vcycles++;
  return launch_status(ctx);
}

// inverse diagonal + Gershgorin bound of D^-1 A (host), upload
int setup_diag(gmg_context *ctx, int64_t n, const int64_t *rp, const int32_t *col, const double *val, DevPtr<double> &invd_dev,
               double *lmax_out) {
  std::vector<double> invd((size_t)std::max<int64_t>(n, 1));
  double lmax = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    double aii = 0.0, rs = 0.0;
    for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
      if (col[k] == i) aii = val[k];
      rs += std::fabs(val[k]);
    }
    invd[(size_t)i] = 1.0 / aii;
    lmax = std::max(lmax, rs / std::fabs(aii));
  }
  if (lmax_out) *lmax_out = lmax;
  CHK(alloc_vec(ctx, invd_dev, n));
  if (n) HIPC(hipMemcpyAsync(invd_dev.get(), invd.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}


// What both plan builders end with: the sweep kernels may use the whole LDS, and, since the records carry absolute LDS
// addresses, their dynamic LDS must start at 0 (no static __shared__) -- else the level keeps the generic sweep (G.wave unset).
int sgs_wave_tail(gmg_context *ctx, SgsPlan &G, bool ph, bool dep, bool reg) {
  HIPC(hipFuncSetAttribute((const void *)sgs_wave_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPC(hipFuncSetAttribute((const void *)sgs_wave_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPC(hipFuncSetAttribute((const void *)sgs_phase_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPC(hipFuncSetAttribute((const void *)sgs_phase_profile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPC(hipFuncSetAttribute((const void *)sgs_dep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPC(hipFuncSetAttribute((const void *)sgs_regs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#ifdef GMG_EXPERIMENTS
  HIPC(hipFuncSetAttribute((const void *)sgs_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#endif
  // the sweep bakes absolute LDS addresses into its records: its dynamic LDS must start at 0 (no static __shared__)
  hipFuncAttributes fa{};
  HIPC(hipFuncGetAttributes(&fa, ph ? (const void *)sgs_phase_kernel : (const void *)sgs_wave_kernel<false>));
  G.wave = fa.sharedSizeBytes == 0;
  if (ph) {
    HIPC(hipFuncGetAttributes(&fa, (const void *)sgs_phase_profile_kernel));
    G.wave = G.wave && fa.sharedSizeBytes == 0;
  }
  if (dep) {
    HIPC(hipFuncGetAttributes(&fa, (const void *)sgs_dep_kernel));
    G.wave = G.wave && fa.sharedSizeBytes == 0;
  }
  if (reg) {
    HIPC(hipFuncGetAttributes(&fa, (const void *)sgs_regs_kernel));
    G.wave = G.wave && fa.sharedSizeBytes == 0;
  }
#ifdef GMG_EXPERIMENTS
  if (ph) {
    HIPC(hipFuncGetAttributes(&fa, (const void *)sgs_chain_kernel));
    G.wave = G.wave && fa.sharedSizeBytes == 0;
  }
#endif
  return GMG_OK;
}

// the options of the context that steer an SSOR plan
SsorPlanOptions ssor_plan_options(const gmg_context *ctx) {
  SsorPlanOptions o;
  o.disable_wave = ctx->sgs_disable_wave; o.disable_phase = ctx->sgs_disable_phase; o.profile = ctx->sgs_profile;
  o.dep = ctx->sgs_dep; o.reg = ctx->sgs_reg; o.chain = ctx->sgs_chain; o.sliding = ctx->sgs_sliding;
  o.y_slots = ctx->sgs_y_slots; o.groups = ctx->sgs_groups; o.phase_chunk = ctx->sgs_phase_chunk;
  o.phase_nosplit = ctx->sgs_phase_nosplit; o.phase_nocascade = ctx->sgs_phase_nocascade; o.pf_lead_kb = ctx->sgs_pf_lead_kb;
  o.debug = ctx->debug_upload; o.pack = ctx->sgs_pack;
  return o;
}

static_assert(sizeof(PhBlkEntry) == sizeof(uint4) && alignof(PhBlkEntry) <= alignof(uint4), "the block table is read as uint4 by the sweep kernels");

// The host-side members of a wavefront plan, as both builders leave them.  W: the host builder's plan, or the tallies and the
// host-side vectors of the device builder's (its tables stay on the device).
void sgs_set_host_members(SgsPlan &G, const SsorSweepPlan &W, const std::vector<int32_t> &block_row, int64_t n_coupled, int64_t stream_bytes) {
  G.host_bwd_rows = W.bwd_rows; G.host_pranges = W.pranges;
  G.host_block_row = block_row; G.host_block_rng = W.block_rng; G.host_block_steps = W.block_steps; G.host_block_bytes = W.block_bytes;
  G.n_self = W.n_self; G.live_max[0] = W.live_max[0]; G.live_max[1] = W.live_max[1];
  G.w_y_slots = W.y_slots; G.w_lds_bytes = W.lds_bytes; G.w_n_ranges = W.n_ranges(); G.n_bwd = W.n_bwd;
  G.phased = W.phased; G.dep = W.dep; G.reg = W.reg;
  G.w_n_coupled = n_coupled; G.w_stream_bytes = stream_bytes; G.w_steps = W.total_steps; G.w_stages = W.total_stages;
  G.n_packed = W.n_packed; G.w_fwd_steps = W.fwd_steps; G.w_stage_steps = W.stage_steps;
}

// debug_upload: the shapes of the steps and the plan's totals
void sgs_plan_log(const SgsPlan &G, const SsorSweepPlan &W, int64_t n) {
  const std::vector<int64_t> &hist_g = W.hist_g, &hist_l1 = W.hist_l1, &hist_l2 = W.hist_l2;
  if (W.phased)
    std::fprintf(stderr, "[gmg] SGS step shapes: G %lld %lld %lld %lld | L1/4 %lld %lld %lld %lld %lld %lld %lld %lld | L2/8 %lld %lld %lld %lld\n", (long long)hist_g[0], (long long)hist_g[1],
                 (long long)hist_g[2], (long long)hist_g[3], (long long)hist_l1[0], (long long)hist_l1[1], (long long)hist_l1[2], (long long)hist_l1[3], (long long)hist_l1[4],
                 (long long)hist_l1[5], (long long)hist_l1[6], (long long)hist_l1[7], (long long)hist_l2[0], (long long)hist_l2[1], (long long)hist_l2[2], (long long)hist_l2[3]);
  std::fprintf(stderr, "[gmg] SGS %s plan: %lld rows, %lld coupled, %d blocks, %lld stages, %lld sub-steps, %d ranges (%d forward + %d backward, %d self-contained), "
               "y slots %d (most live: forward %d, backward %d), stream %.1f MB; schedule: packed %d, levels %lld, steps per direction %lld, by stages %lld "
               "(blocks kept on their stages: %d for the y slots, %d for a step without a shape)\n",
               W.phased ? "four-wave" : "one-wave", (long long)n, (long long)G.w_n_coupled, (int)G.host_block_row.size() - 1, (long long)G.w_stages, (long long)G.w_steps, G.w_n_ranges,
               G.w_n_ranges - G.n_bwd, G.n_bwd, G.n_self, G.w_y_slots, G.live_max[0], G.live_max[1], (double)G.w_stream_bytes / 1e6,
               G.n_packed > 0 ? 1 : 0, (long long)G.w_stages, (long long)G.w_fwd_steps, (long long)G.w_stage_steps,
               W.n_pack_no_slots, W.n_pack_no_shape);
}

// debug_upload: the partition -- per block rows, sub-steps and stream of the plan, and the modelled cost (us) the balanced cuts equalise
void sgs_partition_log(gmg_context *ctx, Level &L, int64_t n, const int64_t *rp, const int32_t *col, const double *val, const std::vector<int32_t> &block_row,
                     bool explicit_rows) {
  const int n_blocks = (int)block_row.size() - 1;
  // the partition: per block rows, sub-steps and stream of the plan, and the modelled cost (us) the balanced cuts equalise
  const std::vector<double> cost = ssor_block_costs(SsorPattern(n, rp, col, val), block_row);
  double c_max = 0, c_sum = 0;
  int64_t s_max = 0, s_sum = 0;
  for (int b = 0; b < n_blocks; ++b) {
    std::fprintf(stderr, "[gmg]   SSOR block %3d: rows [%lld, %lld) %lld, sub-steps %lld, stream %.2f MB, model %.1f us\n", b, (long long)block_row[(size_t)b],
                 (long long)block_row[(size_t)b + 1], (long long)(block_row[(size_t)b + 1] - block_row[(size_t)b]), (long long)L.sgs.host_block_steps[(size_t)b],
                 (double)L.sgs.host_block_bytes[(size_t)b] / 1e6, cost[(size_t)b]);
    c_max = std::max(c_max, cost[(size_t)b]); c_sum += cost[(size_t)b];
    s_max = std::max(s_max, L.sgs.host_block_steps[(size_t)b]); s_sum += L.sgs.host_block_steps[(size_t)b];
  }
  std::fprintf(stderr, "[gmg]   SSOR partition (%s): %d blocks, longest / mean: model %.2f, sub-steps %.2f\n",
               explicit_rows ? "caller's" : ctx->ssor_partition == GMG_SSOR_PARTITION_BALANCED ? "balanced" : "equal rows", n_blocks,
               c_sum > 0 ? c_max * n_blocks / c_sum : 1.0, s_sum > 0 ? (double)s_max * n_blocks / (double)s_sum : 1.0);
  if (L.sgs.w_stage.get()) {
    const int n_ranks = ctx->comm.n_ranks;
    std::fprintf(stderr, "[gmg]   SSOR all-gather: %d ranks x %lld doubles (largest piece) = %.2f MB moved per sweep for %.2f MB of y\n", n_ranks,
                 (long long)L.sgs.w_stage_len, 8e-6 * (double)L.sgs.w_stage_len * n_ranks, 8e-6 * (double)n);
  }
}

// The SSOR plan of a level from its CSR on the host: gmg_sgs_layout.hpp plans, this copies.  Always the generic level schedule
// (the sweep of a level whose rows have unsorted columns); the wavefront plan where one can be made.
int setup_sgs(gmg_context *ctx, Level &L, int64_t n, const int64_t *rp, const int32_t *col, const double *val,
              const std::vector<int64_t> *explicit_rows) {
  const SsorPlanOptions opt = ssor_plan_options(ctx);
  const std::vector<int32_t> block_row = ssor_block_rows(n, rp, col, val, explicit_rows, ctx->ssor_partition == GMG_SSOR_PARTITION_BALANCED, ctx->ssor_blocks);
  const int n_blocks = (int)block_row.size() - 1;
  const SsorGenericPlan GP = ssor_generic_plan(n, rp, col, block_row);
  SsorSweepPlan W;
  ssor_sweep_plan(opt, n, rp, col, val, block_row, true, W);
  if (W.outcome == kSsorOneWave) ssor_sweep_plan(opt, n, rp, col, val, block_row, false, W);
  const auto t_planned = std::chrono::steady_clock::now();
  if (W.outcome == kSsorPlanned)
    if (const char *bad = check_sweep_plan(W, n)) { W.outcome = kSsorInvalid; W.message = bad; }
  const bool wave = W.outcome == kSsorPlanned;
  L.sgs = SgsPlan();
  SgsPlan &G = L.sgs;
  G.n_blocks = n_blocks; G.n_stages_max = GP.n_stages_max;
  HIPC(upload(G.stage_ptr, GP.stage_ptr, ctx->stream));
  HIPC(upload(G.stage_rows, GP.stage_rows, ctx->stream));
  HIPC(upload(G.block_row, block_row, ctx->stream));
  HIPC(upload(G.block_stage, GP.block_stage, ctx->stream));
  if (wave) {
    HIPC(upload(G.w_ranges, W.ranges, ctx->stream));
    HIPC(upload(G.p_ranges, W.pranges, ctx->stream));
    HIPC(upload(G.p_blk_tab, reinterpret_cast<const uint4 *>(W.blk_tab.data()), W.blk_tab.size(), ctx->stream));
    HIPC(upload(G.w_block_rng, W.block_rng, ctx->stream));
    HIPC(upload(G.w_ws_ci, W.ws_ci, ctx->stream));
    HIPC(upload(G.w_ci_row, W.ci_row, ctx->stream));
    HIPC(upload(G.w_row_ci, W.row_ci, ctx->stream));
    HIPC(upload(G.w_rpos_f, W.rpos_f, ctx->stream));
    HIPC(upload(G.w_rpos_b, W.rpos_b, ctx->stream));
    HIPC(upload(G.w_stream, W.stream, ctx->stream));
    HIPC(upload(G.w_iso_diag, W.iso_diag, ctx->stream));
    HIPC(upload(G.w_iso_invd, W.iso_invd, ctx->stream));
    // (every range self-contained: nobody reads or writes ycur -- it is not allocated and the pre-pass gets a null pointer)
    if (!(W.phased && W.n_self == (int)W.pranges.size())) HIPC(G.w_ycur.alloc(std::max<size_t>(W.ci_row.size(), 1)));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  // (the generic sweep: one step per stage and direction; the wavefront plan replaces these with its own counts)
  G.host_block_row = block_row;
  G.host_block_steps.assign((size_t)n_blocks, 0);
  for (int b = 0; b < n_blocks; ++b) G.host_block_steps[(size_t)b] = 2 * (int64_t)(GP.block_stage[(size_t)b + 1] - GP.block_stage[(size_t)b]);
  G.host_block_bytes.assign((size_t)n_blocks, 0);
  if (W.outcome == kSsorUnsupported || W.outcome == kSsorInvalid) return fail(ctx, W.outcome == kSsorUnsupported ? GMG_ERR_UNSUPPORTED : GMG_ERR_INVALID, W.message);
  if (wave) {
    if (ctx->debug_upload)
      std::fprintf(stderr, "[gmg] SGS plan laps (host, %lld rows): block graph %.4f s, steps + slots %.4f s, shapes %.4f s, record fill %.4f s, upload %.4f s\n", (long long)n,
                   W.laps[0], W.laps[1], W.laps[2], W.laps[3], std::chrono::duration<double>(std::chrono::steady_clock::now() - t_planned).count());
    sgs_set_host_members(G, W, block_row, (int64_t)W.ci_row.size(), (int64_t)W.stream.size());
    const int n_ranks = ctx->dist ? ctx->comm.n_ranks : 1;
    if (n_ranks > 1 && n_blocks % n_ranks == 0) {  // staging of the all-gather of the swept pieces
      const int nbl = n_blocks / n_ranks;
      int64_t len = 1;
      for (int r = 0; r < n_ranks; ++r) len = std::max<int64_t>(len, block_row[(size_t)((r + 1) * nbl)] - block_row[(size_t)(r * nbl)]);
      G.w_stage_len = len;
      HIPC(G.w_stage.alloc((size_t)(len * n_ranks)));
    }
    CHK(sgs_wave_tail(ctx, G, W.phased, W.dep, W.reg));
    if (ctx->debug_upload) sgs_plan_log(G, W, n);
  }
  if (ctx->debug_upload) sgs_partition_log(ctx, L, n, rp, col, val, block_row, explicit_rows != nullptr);
  return GMG_OK;
}

// grid of an assembly kernel: by size, at most `most` workgroups, capped by option assemble_max_blocks
dim3 asm_blocks(const gmg_context *ctx, int64_t n, int per_block, int most = 1 << 16) {
  int64_t g = std::max<int64_t>(1, std::min<int64_t>(most, (n + per_block - 1) / per_block));
  if (ctx->assemble_max_blocks > 0) g = std::min<int64_t>(g, ctx->assemble_max_blocks);
  return dim3((unsigned)g);
}

// ---- the same plan formed on the device (option ssor_plan_device; gmg_sgs_plan.hpp) ----------------------------------------
// Why the device builder does not apply to this context (nullptr: it may); one fixed text per cause.
const char *sgs_device_refusal(const gmg_context *ctx, bool explicit_rows, int64_t n) {
  if (ctx->dist) return "communicator";
  if (!explicit_rows && ctx->ssor_partition == GMG_SSOR_PARTITION_BALANCED) return "balanced partition";
  if (!ctx->sgs_sliding) return "option sgs_sliding unset";
  if (ctx->sgs_disable_wave) return "option sgs_disable_wave set";
  if (ctx->sgs_disable_phase) return "option sgs_disable_phase set";
  if (ctx->sgs_profile) return "option sgs_profile set";
  if (ctx->sgs_dep) return "option sgs_dep set";
  if (ctx->sgs_reg) return "option sgs_reg set";
  if (ctx->sgs_chain) return "option sgs_chain set";
  if (ctx->sgs_groups) return "option sgs_groups set";
  if (ctx->sgs_phase_chunk) return "option sgs_phase_chunk set";
  if (ctx->sgs_phase_nosplit) return "option sgs_phase_nosplit set";
  if (ctx->sgs_phase_nocascade) return "option sgs_phase_nocascade set";
  if (ctx->sgs_pf_lead_kb) return "option sgs_pf_lead_kb set";
  // (the kernels of gmg_sgs_plan.hpp form the stage-by-stage schedule; a level whose rows are scheduled by slack is the host's)
  if (ssor_pack_wanted(ssor_plan_options(ctx), n)) return "packed schedule";
  return nullptr;
}

// The plan of level L from its CSR on the device (rp: n + 1 row pointers, col, val).  *reason == nullptr on return: L.sgs holds
// the plan setup_sgs would have made, byte for byte.  Else nothing of L.sgs was touched and *reason says why the host builder
// has to run (decided after the kernels found the condition, before anything is kept).  A plan that fails its own checks is an
// error (GMG_ERR_INVALID): no sweep runs on it.
int setup_sgs_device(gmg_context *ctx, Level &L, int64_t n, const int32_t *rp, const int32_t *col, const double *val,
                     const std::vector<int64_t> *explicit_rows, const char **reason) {
  *reason = sgs_device_refusal(ctx, explicit_rows != nullptr, n);
  if (*reason) return GMG_OK;
  if (n <= 0) { *reason = "empty level"; return GMG_OK; }
  const std::vector<int32_t> block_row = ssor_block_rows(n, nullptr, nullptr, nullptr, explicit_rows, false, ctx->ssor_blocks);  // (the caller's or equal runs)
  const int n_blocks = (int)block_row.size() - 1;
  int y_cap = ctx->sgs_y_slots > 0 ? ctx->sgs_y_slots : kPhYSlots;
  y_cap = std::max(64, std::min(y_cap, kPhYSlots)) & ~1;
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)n, NB = (size_t)n_blocks;
  // debug_upload: wall time (seconds) up to each of the builder's host synchronisations: graph, stages, order .. offsets, records + check
  double laps[4] = {0, 0, 0, 0};
  auto lap_t = std::chrono::steady_clock::now();
  auto lap = [&](int k) {
    const auto t = std::chrono::steady_clock::now();
    laps[k] += std::chrono::duration<double>(t - lap_t).count();
    lap_t = t;
  };
  auto grid = [&](int64_t cnt) { return asm_blocks(ctx, cnt, 256); };
  auto scan = [&](int32_t *p, int64_t cnt) { hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, st, p, cnt); };
  sp::Args a{};
  a.n = n; a.n_blocks = n_blocks; a.y_cap = y_cap; a.rp = rp; a.col = col; a.val = val;
  // ---- 1. pruned graph
  DevPtr<int32_t> d_brow, d_prp, d_indeg, d_upptr, d_upfill, d_ccnt, d_stage, d_pcol, d_uplist, d_row_ci;
  DevPtr<uint8_t> d_coupled;
  DevPtr<uint32_t> d_flags;
  DevPtr<double> d_pval, d_iso_diag, d_iso_invd;
  DevPtr<sp::Block> d_blk;
  HIPC(upload(d_brow, block_row, st));
  HIPC(d_prp.alloc(N + 1)); HIPC(d_indeg.alloc(N)); HIPC(d_upptr.alloc(N + 1)); HIPC(d_upfill.alloc(N)); HIPC(d_ccnt.alloc(NB));
  HIPC(d_stage.alloc(N)); HIPC(d_coupled.alloc(N)); HIPC(d_flags.alloc(1)); HIPC(d_iso_diag.alloc(N)); HIPC(d_iso_invd.alloc(N)); HIPC(d_row_ci.alloc(N));
  HIPC(hipMemsetAsync(d_indeg.get(), 0, 4 * N, st)); HIPC(hipMemsetAsync(d_upptr.get(), 0, 4 * (N + 1), st)); HIPC(hipMemsetAsync(d_upfill.get(), 0, 4 * N, st));
  HIPC(hipMemsetAsync(d_ccnt.get(), 0, 4 * NB, st)); HIPC(hipMemsetAsync(d_coupled.get(), 0, N, st)); HIPC(hipMemsetAsync(d_flags.get(), 0, 4, st));
  HIPC(hipMemsetAsync(d_row_ci.get(), 0xff, 4 * N, st));
  a.brow = d_brow.get(); a.prp = d_prp.get(); a.indeg = d_indeg.get(); a.upptr = d_upptr.get(); a.upfill = d_upfill.get(); a.ccnt = d_ccnt.get();
  a.stage = d_stage.get(); a.coupled = d_coupled.get(); a.flags = d_flags.get(); a.iso_diag = d_iso_diag.get(); a.iso_invd = d_iso_invd.get(); a.row_ci = d_row_ci.get();
  hipLaunchKernelGGL(sp::graph_kernel<false>, grid(n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(sp::coupled_count_kernel, grid(n), dim3(256), 0, st, a);
  scan(d_prp.get(), n);
  scan(d_upptr.get(), n);
  uint32_t flags = 0;
  int32_t n_pruned = 0, n_up = 0;
  std::vector<int32_t> ccnt(NB, 0);
  HIPC(hipMemcpyAsync(&flags, d_flags.get(), 4, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(&n_pruned, d_prp.get() + n, 4, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(&n_up, d_upptr.get() + n, 4, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(ccnt.data(), d_ccnt.get(), 4 * NB, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  CHK(launch_status(ctx));
  lap(0);
  if (flags & sp::kUnsorted) { *reason = "unsorted columns"; return GMG_OK; }
  if (flags & sp::kWide) { *reason = "row too wide"; return GMG_OK; }
  std::vector<sp::Block> blk(NB);
  SsorSweepPlan W;  // the host-side part of the plan: ranges, tallies, what the logs print (the tables stay on the device)
  W.phased = true;
  std::vector<int32_t> &block_rng = W.block_rng;
  block_rng.assign(NB + 1, 0);
  int64_t nct = 0;
  for (int b = 0; b < n_blocks; ++b) {
    sp::Block &B = blk[(size_t)b];
    B = sp::Block{block_row[(size_t)b], block_row[(size_t)b + 1], (int32_t)nct, ccnt[(size_t)b], 0, 0, block_rng[(size_t)b], 0};
    nct += ccnt[(size_t)b];
    block_rng[(size_t)b + 1] = block_rng[(size_t)b] + (ccnt[(size_t)b] > 0 ? 2 : 0);
  }
  const int n_ranges = block_rng[NB];
  const size_t NC = (size_t)nct;
  a.n_coupled = (int32_t)nct;
  HIPC(upload(d_blk, blk, st));
  a.blk = d_blk.get();
  HIPC(d_pcol.alloc(std::max<size_t>((size_t)n_pruned, 1))); HIPC(d_pval.alloc(std::max<size_t>((size_t)n_pruned, 1))); HIPC(d_uplist.alloc(std::max<size_t>((size_t)n_up, 1)));
  a.pcol = d_pcol.get(); a.pval = d_pval.get(); a.uplist = d_uplist.get();
  hipLaunchKernelGGL(sp::graph_kernel<true>, grid(n), dim3(256), 0, st, a);
  // ---- 2. stages
  DevPtr<int32_t> d_queue, d_sptr, d_stepbase, d_nstages, d_nsteps, d_ci_row, d_spos;
  HIPC(d_queue.alloc(std::max<size_t>(NC, 1))); HIPC(d_ci_row.alloc(std::max<size_t>(NC, 1)));
  HIPC(d_sptr.alloc(NC + NB + 1)); HIPC(d_stepbase.alloc(NC + NB + 1)); HIPC(d_spos.alloc(NC + NB + 1)); HIPC(d_nstages.alloc(NB)); HIPC(d_nsteps.alloc(NB));
  a.queue = d_queue.get(); a.ci_row = d_ci_row.get(); a.sptr = d_sptr.get(); a.spos = d_spos.get(); a.stepbase = d_stepbase.get(); a.nstages = d_nstages.get(); a.nsteps = d_nsteps.get();
  hipLaunchKernelGGL(sp::stage_kernel, asm_blocks(ctx, n_blocks, 1), dim3(1024), 0, st, a);
  std::vector<int32_t> nstages(NB, 0), nsteps(NB, 0);
  HIPC(hipMemcpyAsync(nstages.data(), d_nstages.get(), 4 * NB, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(nsteps.data(), d_nsteps.get(), 4 * NB, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(&flags, d_flags.get(), 4, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  CHK(launch_status(ctx));
  lap(1);
  if (flags & sp::kInternal) return fail(ctx, GMG_ERR_INVALID, "SSOR plan on the device: the stage propagation did not reach every coupled row (internal error)");
  int64_t n_steps = 0, total_stages = 0;
  for (int b = 0; b < n_blocks; ++b) {
    blk[(size_t)b].S = nsteps[(size_t)b]; blk[(size_t)b].g0 = (int32_t)n_steps;
    n_steps += 2 * (int64_t)nsteps[(size_t)b];
    total_stages += nstages[(size_t)b];
  }
  if (n_steps >= INT32_MAX / kPhMaxRows) { *reason = "stream positions beyond 2^31"; return GMG_OK; }
  const size_t NS = (size_t)n_steps;
  a.n_steps = (int32_t)n_steps;
  HIPC(hipMemcpyAsync(d_blk.get(), blk.data(), sizeof(sp::Block) * NB, hipMemcpyHostToDevice, st));
  // ---- 3. - 6. order, steps, slots, shapes, offsets
  DevPtr<int32_t> d_su, d_st_bd, d_st_nrows, d_st_row, d_last, d_dueptr, d_duefill, d_duelist, d_slot, d_nslots, d_cut, d_shape, d_word, d_bytes, d_off16, d_rbytes;
  DevPtr<unsigned long long> d_mask;
  HIPC(d_su.alloc(2 * N)); HIPC(d_last.alloc(2 * N)); HIPC(d_slot.alloc(2 * N));
  HIPC(d_st_bd.alloc(NS + 1)); HIPC(d_st_nrows.alloc(NS + 1)); HIPC(d_st_row.alloc(NS * kPhMaxRows + 1)); HIPC(d_dueptr.alloc(NS + 1)); HIPC(d_duefill.alloc(NS + 1));
  HIPC(d_duelist.alloc(2 * NC + 1)); HIPC(d_nslots.alloc(2 * NB)); HIPC(d_cut.alloc(NS * kPhMaxRows + 1)); HIPC(d_shape.alloc(NS + 1)); HIPC(d_word.alloc(NS + 1));
  HIPC(d_bytes.alloc(NS + 1)); HIPC(d_off16.alloc(NS + 1)); HIPC(d_mask.alloc(2 * NS + 1)); HIPC(d_rbytes.alloc(2 * NB));
  HIPC(hipMemsetAsync(d_last.get(), 0xff, 8 * N, st)); HIPC(hipMemsetAsync(d_dueptr.get(), 0, 4 * (NS + 1), st)); HIPC(hipMemsetAsync(d_duefill.get(), 0, 4 * (NS + 1), st));
  HIPC(hipMemsetAsync(d_nslots.get(), 0, 8 * NB, st)); HIPC(hipMemsetAsync(d_off16.get(), 0, 4 * (NS + 1), st));
  a.su = d_su.get(); a.last = d_last.get(); a.slot = d_slot.get(); a.st_bd = d_st_bd.get(); a.st_nrows = d_st_nrows.get(); a.st_row = d_st_row.get();
  a.dueptr = d_dueptr.get(); a.duefill = d_duefill.get(); a.duelist = d_duelist.get(); a.nslots = d_nslots.get(); a.cut = d_cut.get(); a.shape = d_shape.get();
  a.word = d_word.get(); a.bytes = d_bytes.get(); a.off16 = d_off16.get(); a.mask = d_mask.get();
  if (nct > 0) {
    // (only now: the stage propagation was found complete above, so every coupled row has a stage and every stage its place)
    hipLaunchKernelGGL(sp::rank_kernel, asm_blocks(ctx, n_blocks, 1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(sp::order_kernel, grid(nct), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp::last_kernel, grid(2 * nct), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp::due_kernel<false>, grid(2 * nct), dim3(256), 0, st, a);
    scan(d_dueptr.get(), n_steps);
    hipLaunchKernelGGL(sp::due_kernel<true>, grid(2 * nct), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp::slot_kernel, asm_blocks(ctx, 2 * n_blocks, 1), dim3(sp::kSlotThreads), 0, st, a);
    hipLaunchKernelGGL(sp::cut_kernel, grid(n_steps), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp::chunk_kernel, grid(n_steps), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp::word_kernel, grid(n_steps), dim3(256), 0, st, a);
    scan(d_off16.get(), n_steps);
  }
  hipLaunchKernelGGL(sp::range_bytes_kernel, grid(2 * n_blocks), dim3(256), 0, st, a, d_rbytes.get());
  std::vector<int32_t> nslots(2 * NB, 0), rbytes(2 * NB, 0);
  HIPC(hipMemcpyAsync(nslots.data(), d_nslots.get(), 8 * NB, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(rbytes.data(), d_rbytes.get(), 8 * NB, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(&flags, d_flags.get(), 4, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  CHK(launch_status(ctx));
  lap(2);
  if (flags & sp::kNoFit) { *reason = "block does not fit"; return GMG_OK; }
  if (flags & sp::kNoShape) { *reason = "no shape"; return GMG_OK; }
  // ---- 7. the ranges: inside a block the backward one first in the stream, the forward one first in the table
  std::vector<PhRange> &pranges = W.pranges;
  pranges.resize((size_t)n_ranges);
  std::vector<int64_t> rbase((size_t)n_ranges + 1, 0);
  int64_t stream_size = 0;
  int *live_max = W.live_max, max_ws = 0;
  W.block_steps.assign(NB, 0); W.block_bytes.assign(NB, 0);
  for (int b = 0; b < n_blocks; ++b) {
    const sp::Block &B = blk[(size_t)b];
    if (B.nc == 0) continue;
    W.block_steps[(size_t)b] = 2 * (int64_t)B.S;
    const int64_t bytes0 = stream_size;
    for (int dir = 1; dir >= 0; --dir) {
      const int ns = nslots[2 * (size_t)b + dir];
      live_max[dir] = std::max(live_max[dir], ns);
      max_ws = std::max(max_ws, ns);
      PhRange P{};
      P.backward = dir; P.pad0[0] = 1; P.pad0[1] = ns;
      P.n_steps = B.S;
      const int64_t base = (stream_size + 1023) / 1024 * 1024, off = (int64_t)rbytes[2 * (size_t)b + dir] * 16;
      P.stream_off = base;
      P.blk_tab = (uint32_t)(B.g0 + (dir ? 0 : B.S));
      const int64_t padded = (off + 2048 + 1023) / 1024 * 1024;
      if (padded >= ((int64_t)1 << 31) || (base + padded) / 8 >= ((int64_t)1 << 31)) { *reason = "stream positions beyond 2^31"; return GMG_OK; }
      P.stream_bytes = (uint32_t)padded;
      stream_size = base + padded;
      pranges[(size_t)(B.rng + dir)] = P;
      rbase[(size_t)(B.rng + dir)] = base;
    }
    W.block_bytes[(size_t)b] = stream_size - bytes0;
  }
  const int y_slots = std::max(2, (max_ws + 1) & ~1);
  // ---- 8. records
  DevPtr<int64_t> d_rbase;
  DevPtr<char> d_stream;
  DevPtr<uint4> d_blk_tab;
  DevPtr<PhRange> d_pranges;
  DevPtr<int32_t> d_rpos, d_block_rng;
  DevPtr<unsigned long long> d_chk;
  HIPC(upload(d_rbase, rbase, st));
  HIPC(upload(d_pranges, pranges, st));
  HIPC(upload(d_block_rng, block_rng, st));
  HIPC(d_stream.alloc(std::max<size_t>((size_t)stream_size, 1))); HIPC(d_blk_tab.alloc(std::max<size_t>(NS, 1))); HIPC(d_rpos.alloc(std::max<size_t>(2 * NC, 1))); HIPC(d_chk.alloc(8));
  HIPC(hipMemsetAsync(d_stream.get(), 0, std::max<size_t>((size_t)stream_size, 1), st));
  HIPC(hipMemsetAsync(d_chk.get(), 0, 64, st));
  a.rbase = d_rbase.get(); a.stream = d_stream.get(); a.blk_tab = d_blk_tab.get(); a.rpos = d_rpos.get();
  if (nct > 0) {
    hipLaunchKernelGGL(sp::record_kernel, grid(2 * nct), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sp::header_kernel, grid(n_steps), dim3(256), 0, st, a);
  }
  // ---- the finished plan is checked from its own arrays before it is accepted
  sp::CheckArgs c{};
  c.ranges = d_pranges.get(); c.blk_tab = d_blk_tab.get(); c.stream = d_stream.get(); c.rpos_f = d_rpos.get(); c.rpos_b = d_rpos.get() + NC;
  c.n_ranges = n_ranges; c.n_coupled = (int32_t)nct; c.y_slots = y_slots; c.stream_bytes = stream_size; c.out = d_chk.get();
  hipLaunchKernelGGL(sp::check_kernel, asm_blocks(ctx, std::max(n_ranges, 1), 1, 1024), dim3(256), 0, st, c);
  unsigned long long chk[8] = {};
  std::vector<int32_t> ci_row(NC);
  std::vector<uint4> blk_tab_h;
  HIPC(hipMemcpyAsync(chk, d_chk.get(), 64, hipMemcpyDeviceToHost, st));
  if (NC) HIPC(hipMemcpyAsync(ci_row.data(), d_ci_row.get(), 4 * NC, hipMemcpyDeviceToHost, st));
  if (ctx->debug_upload && NS) {
    blk_tab_h.resize(NS);
    HIPC(hipMemcpyAsync(blk_tab_h.data(), d_blk_tab.get(), 16 * NS, hipMemcpyDeviceToHost, st));
  }
  HIPC(hipStreamSynchronize(st));
  CHK(launch_status(ctx));
  if (chk[0]) return fail(ctx, GMG_ERR_INVALID, "SSOR plan on the device: the block table, a header or a record fails the plan's checks (internal error)");
  if (stream_size > 0 && (chk[1] * 8 + 8 > (uint64_t)stream_size || chk[2] + 8 > (uint64_t)y_slots * 8))
    return fail(ctx, GMG_ERR_INVALID, "SSOR plan on the device: a record addresses memory outside the stream / the LDS slots (internal error)");
  if (chk[3] >= (uint64_t)n) return fail(ctx, GMG_ERR_INVALID, "SSOR plan on the device: a backward record stores outside the level vector (internal error)");
  if (NC && chk[4] * 8 + 8 > (uint64_t)stream_size) return fail(ctx, GMG_ERR_INVALID, "SSOR plan on the device: rhs position outside the stream (internal error)");
  // ---- 9. accepted: the plan and its host-side members, as setup_sgs leaves them
  L.sgs = SgsPlan();
  SgsPlan &G = L.sgs;
  G.n_blocks = n_blocks;
  HIPC(upload(G.w_ranges, std::vector<SwRange>(), st));
  HIPC(upload(G.w_ws_ci, std::vector<int32_t>(), st));
  G.p_ranges = std::move(d_pranges); G.p_blk_tab = std::move(d_blk_tab); G.w_block_rng = std::move(d_block_rng);
  G.w_ci_row = std::move(d_ci_row); G.w_row_ci = std::move(d_row_ci); G.w_stream = std::move(d_stream);
  G.w_iso_diag = std::move(d_iso_diag); G.w_iso_invd = std::move(d_iso_invd);
  HIPC(G.w_rpos_f.alloc(std::max<size_t>(NC, 1))); HIPC(G.w_rpos_b.alloc(std::max<size_t>(NC, 1)));
  if (NC) {
    HIPC(hipMemcpyAsync(G.w_rpos_f.get(), d_rpos.get(), 4 * NC, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(G.w_rpos_b.get(), d_rpos.get() + NC, 4 * NC, hipMemcpyDeviceToDevice, st));
  }
  HIPC(hipStreamSynchronize(st));
  for (int b = 0; b < n_blocks; ++b)  // (the aux words of the backward records in stream order: each block's coupled rows, last first)
    for (int q = blk[(size_t)b].nc - 1; q >= 0; --q) W.bwd_rows.push_back(ci_row[(size_t)(blk[(size_t)b].q0 + q)]);
  W.n_self = n_ranges; W.n_bwd = n_ranges / 2;
  W.y_slots = y_slots;
  W.lds_bytes = y_slots * 8 + kPhWaves * kPhRegion + kPhJunk;
  W.total_steps = n_steps; W.total_stages = total_stages;
  W.fwd_steps = W.stage_steps = n_steps / 2;  // (the stages, kPhMaxRows rows at a time: never packed)
  sgs_set_host_members(G, W, block_row, nct, stream_size);
  G.on_device = true;
  CHK(sgs_wave_tail(ctx, G, true, false, false));
  if (!G.wave) return fail(ctx, GMG_ERR_INVALID, "SSOR plan on the device: the sweep kernel has static LDS (internal error)");
  lap(3);
  if (ctx->debug_upload) {
    std::fprintf(stderr, "[gmg] SGS plan laps (device, %lld rows): graph %.4f s, stages %.4f s, order + slots + shapes + offsets %.4f s, records + check %.4f s\n", (long long)n,
                 laps[0], laps[1], laps[2], laps[3]);
    for (const uint4 &e : blk_tab_h) {
      int g, l1, l2;
      sp::key_shape((int)(e.z & 255u), &g, &l1, &l2);
      W.hist_l1[(size_t)std::min(7, l1 / 4)]++; W.hist_l2[(size_t)(l2 / 8)]++; W.hist_g[(size_t)g]++;
    }
    sgs_plan_log(G, W, n);
  }
  return GMG_OK;
}

// The SSOR plan of a level whose CSR lies on the device (d_*) -- and, for gmg_set_level_matrix, on the host as well (rp64 / col /
// val; col == nullptr: fetch() brings col and val back when the host builder needs them and returns the bytes it moved).
template <class Fetch>
int setup_sgs_any(gmg_context *ctx, Level &L, int64_t n, const int32_t *d_rp, const int32_t *d_col, const double *d_val, const int64_t *rp64,
                  const int32_t *col, const double *val, const std::vector<int64_t> *explicit_rows, Fetch fetch) {
  const char *reason = "";
  int64_t moved = 0;
  if (ctx->ssor_plan_device) {
    CHK(setup_sgs_device(ctx, L, n, d_rp, d_col, d_val, explicit_rows, &reason));
    if (!reason) {
      if (ctx->debug_upload) {  // (the log's modelled block costs come from the host's cost model: the CSR comes back for that line alone)
        if (!col) CHK(fetch(&col, &val, &moved));
        L.sgs.csr_bytes_down = moved;
        sgs_partition_log(ctx, L, n, rp64, col, val, L.sgs.host_block_row, explicit_rows != nullptr);
      }
      return GMG_OK;
    }
  }
  if (!col) CHK(fetch(&col, &val, &moved));
  CHK(setup_sgs(ctx, L, n, rp64, col, val, explicit_rows));
  L.sgs.csr_bytes_down = moved;
  L.sgs.host_reason = reason;
  return GMG_OK;
}

// frees every operator / work vector but keeps the stream, the reduction scratch and the communicator
void free_cg_ring(gmg_context *ctx) {
  // (collective: every rank frees its shared ring at the same point, gmg_set_level_matrix / gmg_reset / gmg_destroy)
  if (ctx->ring_shared[ctx->comm.rank]) comm_share_free(ctx->comm, ctx->ring_shared);
  for (int r = 0; r < kXRing; ++r) { ctx->cg_ring[r] = nullptr; ctx->cg_ring_own[r].reset(); }
  ctx->cg_ring_len = 0;
}

void free_locator(gmg_context *ctx) {
  ctx->loc_node.reset(); ctx->loc_dofs.reset();
  ctx->loc = gmg_forces::Locator{};
  ctx->loc_max_dof = -1;
}

void release_operators(gmg_context *ctx) {
  for (auto &L : ctx->lv) L = Level();
  ctx->S = DevCSR();
  for (DevPtr<double> *p : {&ctx->sys_full_a, &ctx->sys_full_b, &ctx->S_invd, &ctx->S_tmp, &ctx->cg_g, &ctx->cg_d0, &ctx->cg_d1, &ctx->cg_h}) p->reset();
  free_cg_ring(ctx);
  drop_coarse_direct(ctx);
}

// a CSR the device formed in place (rowptr / col / val of m): its sizes and the row-window tiling from the row pointers
int tile_device_csr(gmg_context *ctx, DevCSR &m, const std::vector<int32_t> &rp, int64_t n_rows, int64_t n_cols, int64_t nnz) {
  const TilePlan T = plan_tiles(rp.data(), n_rows);
  m.n_rows = n_rows; m.n_cols = n_cols; m.nnz = nnz;
  set_tiles(m, T);
  HIPC(upload(m.tile_row, T.tile_row, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  CHK(launch_status(ctx));
  m.valid = true;
  return GMG_OK;
}

struct AsmScratch {  // lives until the stream has run the kernels
  DevPtr<int32_t> iptr, ipos, islot;
  DevPtr<unsigned long long> total;
  DevPtr<int> over;
};

// What the two device assemblies share (gmg_assemble.hpp; LEVEL: the level-matrix form): the incidence lists, the pattern,
// and the FILL pass of the row kernel.  a holds the inputs and the outputs the caller owns (invd, ...); m receives rowptr /
// col / val, rp the row pointers on the host, n_inc the (row, slot) pairs.  before_fill(nnz) may point a at further outputs of
// the FILL pass once their size is known.  The FILL pass is enqueued, not waited for.
// The incidence lists (gmg_assemble.hpp, kernels 1 and 2): every row's (cell, vertex) slots in ascending order, from the inputs
// in a into a.inc_ptr / a.inc_slot (owned by w); n_inc receives the (row, slot) pairs.  The sort is enqueued, not waited for.
template <bool LEVEL>
int assemble_incidence(gmg_context *ctx, AsmArgs &a, AsmScratch &w, int32_t &n_inc) {
  const int64_t n_dofs = a.n_dofs, n_slots = a.n_slots;
  HIPC(w.iptr.alloc((size_t)n_dofs + 1));
  HIPC(w.ipos.alloc((size_t)n_dofs + 1));
  HIPC(hipMemsetAsync(w.iptr.get(), 0, sizeof(int32_t) * ((size_t)n_dofs + 1), ctx->stream));
  HIPC(hipMemsetAsync(w.ipos.get(), 0, sizeof(int32_t) * ((size_t)n_dofs + 1), ctx->stream));
  a.inc_ptr = w.iptr.get(); a.inc_pos = w.ipos.get();
  const dim3 g_slots = asm_blocks(ctx, n_slots, 256), g_dofs = asm_blocks(ctx, n_dofs, 256);
  if (n_slots) hipLaunchKernelGGL((asm_incidence_kernel<false, LEVEL>), g_slots, dim3(256), 0, ctx->stream, a);
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, w.iptr.get(), n_dofs);
  n_inc = 0;
  HIPC(hipMemcpyAsync(&n_inc, w.iptr.get() + n_dofs, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  HIPC(w.islot.alloc((size_t)std::max<int32_t>(n_inc, 1)));
  a.inc_slot = w.islot.get();
  if (n_slots) {
    hipLaunchKernelGGL((asm_incidence_kernel<true, LEVEL>), g_slots, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(asm_sort_incidence_kernel, g_dofs, dim3(256), 0, ctx->stream, a);
  }
  return GMG_OK;
}

template <bool LEVEL, class BeforeFill>
int assemble_rows(gmg_context *ctx, const char *who, AsmArgs &a, AsmScratch &w, DevCSR &m, std::vector<int32_t> &rp, int64_t &nnz, int32_t &n_inc,
                  BeforeFill before_fill) {
  const int64_t n_dofs = a.n_dofs;
  HIPC(m.rowptr.alloc((size_t)n_dofs + 1));
  HIPC(w.total.alloc(1));
  HIPC(w.over.alloc(1));
  HIPC(hipMemsetAsync(m.rowptr.get(), 0, sizeof(int32_t) * ((size_t)n_dofs + 1), ctx->stream));
  HIPC(hipMemsetAsync(w.total.get(), 0, sizeof(unsigned long long), ctx->stream));
  HIPC(hipMemsetAsync(w.over.get(), 0, sizeof(int), ctx->stream));
  a.rowptr = m.rowptr.get(); a.total = w.total.get(); a.overflow = w.over.get();
  const dim3 g_rows = asm_blocks(ctx, n_dofs, 1);
  CHK(assemble_incidence<LEVEL>(ctx, a, w, n_inc));
  if (n_dofs) hipLaunchKernelGGL((asm_row_kernel<false, LEVEL>), g_rows, dim3(64), 0, ctx->stream, a);
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, m.rowptr.get(), n_dofs);
  rp.assign((size_t)n_dofs + 1, 0);
  unsigned long long total = 0;
  int over = 0;
  HIPC(hipMemcpyAsync(rp.data(), m.rowptr.get(), sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&total, w.total.get(), sizeof total, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&over, w.over.get(), sizeof over, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (over) return fail(ctx, GMG_ERR_UNSUPPORTED, (std::string(who) + ": a row with more than 512 columns").c_str());
  if (total >= (1ull << 31)) return fail(ctx, GMG_ERR_UNSUPPORTED, (std::string(who) + ": operator needs 64-bit device indices (nnz >= 2^31)").c_str());
  nnz = (int64_t)total;
  const size_t pad = 8;
  HIPC(m.col.alloc((size_t)nnz + pad));
  HIPC(m.val.alloc((size_t)nnz + pad));
  HIPC(hipMemsetAsync(m.col.get() + nnz, 0, sizeof(int32_t) * pad, ctx->stream));
  HIPC(hipMemsetAsync(m.val.get() + nnz, 0, sizeof(double) * pad, ctx->stream));
  a.col = m.col.get(); a.val = m.val.get();
  CHK(before_fill(nnz));
  if (n_dofs && a.nq > 0) hipLaunchKernelGGL((asm_row_kernel<true, LEVEL, true>), g_rows, dim3(64), 0, ctx->stream, a);
  else if (n_dofs) hipLaunchKernelGGL((asm_row_kernel<true, LEVEL>), g_rows, dim3(64), 0, ctx->stream, a);
  return GMG_OK;
}

// The coefficient form of the two assemblies (gmg_assemble_*_matrix_coef): values at the quadrature points of every cell, the
// reference-cell products G, the weights and the scale(s) instead of cell matrices.
struct AsmCoef {
  int nq;
  const double *cell_coef, *G, *qw, *scale;
  int n_scale;  // 16 by cell level, or 1
};
struct AsmCoefDev {  // the uploaded tables; lives until the stream has run the kernels
  DevPtr<double> cc, G, qw, scale;
};

// the argument checks of the coefficient form, on the host before any launch (0: fine)
int check_coef(gmg_context *ctx, const char *who, const AsmCoef &k, int64_t n_cells) {
  const std::string w(who);
  if (k.nq < 1 || k.nq > kAsmMaxNq) return fail(ctx, GMG_ERR_INVALID, (w + ": nq must be in 1 .. 64").c_str());
  if ((n_cells > 0 && !k.cell_coef) || !k.G || !k.qw || !k.scale) return fail(ctx, GMG_ERR_INVALID, (w + ": cell_coef, G, qw or the scale is NULL").c_str());
  return GMG_OK;
}

int upload_coef(gmg_context *ctx, const AsmCoef &k, int64_t n_cells, int nv, AsmCoefDev &d, AsmArgs &a) {
  HIPC(upload(d.cc, k.cell_coef, (size_t)n_cells * (size_t)k.nq, ctx->stream));
  HIPC(upload(d.G, k.G, (size_t)k.nq * nv * nv, ctx->stream));
  HIPC(upload(d.qw, k.qw, (size_t)k.nq, ctx->stream));
  HIPC(upload(d.scale, k.scale, (size_t)k.n_scale, ctx->stream));
  a.nq = k.nq; a.cell_coef = d.cc.get(); a.G = d.G.get(); a.qw = d.qw.get(); a.scale = d.scale.get();
  return GMG_OK;
}

// device -> host copy of n elements on the context's stream (not waited for); a null destination is skipped
template <class T>
hipError_t mesh_fetch(gmg_context *ctx, T *dst, const DevPtr<T> &src, int64_t n) {
  if (!dst || n <= 0) return hipSuccess;
  return hipMemcpyAsync(dst, src.get(), sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
}

// The host-side checks of every entry that takes the forest, before anything is launched (gmg_build_mesh_tables in
// include/gmg_coulomb.h is the definition); level_of [cells of all levels]: the level of every cell
int check_forest(gmg_context *ctx, const char *who, int dim, const int32_t *n0, int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                 const int32_t *cell_first_child, std::vector<uint8_t> &level_of) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (dim != 2 && dim != 3) return bad(GMG_ERR_INVALID, "dim must be 2 or 3");
  if (n_levels < 0 || n_levels > kMtShift + 1) return bad(GMG_ERR_INVALID, "between 0 and 13 levels");
  if (!n0 || !level_ptr) return bad(GMG_ERR_INVALID, "n0 or level_ptr is NULL");
  for (int d = 0; d < dim; ++d)
    if (n0[d] < 1 || n0[d] > 511) return bad(GMG_ERR_INVALID, "n0 outside 1 .. 511");
  if (level_ptr[0] != 0) return bad(GMG_ERR_INVALID, "level_ptr does not start at 0");
  for (int l = 0; l < n_levels; ++l)
    if (level_ptr[l + 1] < level_ptr[l]) return bad(GMG_ERR_INVALID, "level_ptr decreases");
  const int nv = 1 << dim;
  const int64_t n_all = level_ptr[n_levels];
  if (n_all > 0 && (!cell_coord || !cell_first_child)) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_all * nv >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 slots");
  const int32_t lat[3] = {n0[0], n0[1], dim == 3 ? n0[2] : 1};
  level_of.assign((size_t)n_all, 0);
  for (int l = 0; l < n_levels; ++l) {
    const int64_t n_next = l + 1 < n_levels ? level_ptr[l + 2] - level_ptr[l + 1] : 0;
    for (int64_t c = level_ptr[l]; c < level_ptr[l + 1]; ++c) {
      level_of[(size_t)c] = (uint8_t)l;
      for (int d = 0; d < 3; ++d) {
        const int64_t x = cell_coord[3 * c + d], n = d < dim ? (int64_t)lat[d] << l : 1;
        if (x < 0 || x >= n) return bad(GMG_ERR_INVALID, "a cell outside its level's lattice");
      }
      const int64_t fc = cell_first_child[c];
      if (fc >= 0 && fc + nv > n_next) return bad(GMG_ERR_INVALID, "first_child points outside the next level");
    }
  }
  return GMG_OK;
}

DevCSR *which_matrix(gmg_context *ctx, int which) {
  if (which == GMG_SYSTEM) return &ctx->S;
  if (which < 0 || which >= ctx->n_levels) return nullptr;
  return &ctx->lv[(size_t)which].A;
}

}  // namespace

// The distributed coarse CG lives with the communicator code.
#include "gmg_dist.hpp"

// =============================================================================== C-ABI

extern "C" {

int gmg_create(gmg_context **out, int device_id, int n_levels) {
  if (!out || n_levels < 1) return GMG_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_id < 0 || device_id >= count) return GMG_ERR_HIP;
  if (hipSetDevice(device_id) != hipSuccess) return GMG_ERR_HIP;
  gmg_context *ctx = new gmg_context();
  ctx->device = device_id;
  ctx->n_levels = n_levels;
  ctx->lv.resize((size_t)n_levels);
  auto bail = [&](int code) { gmg_destroy(ctx); return code; };
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->st.alloc(1) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->st_host.alloc(2) != hipSuccess) return bail(GMG_ERR_HIP);
  for (auto &e : ctx->ev_chunk)
    if (e.create(hipEventDisableTiming) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->part_a.alloc(4 * kMaxPartials) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->part_b.alloc(4 * kMaxPartials) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->lanczos_rec.alloc(lanczos::record_len(lanczos::kMaxSteps)) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->scal_dev.alloc(8) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->scal_host.alloc(8) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->ocg_dev.alloc(4) != hipSuccess) return bail(GMG_ERR_HIP);
  if (ctx->sgs_abort.alloc(1) != hipSuccess) return bail(GMG_ERR_HIP);
  *ctx->sgs_abort.get() = 0;
  (void)hipMemsetAsync(ctx->st.get(), 0, sizeof(CGState), ctx->stream);
  // measurement scripts reach the diagnostic options of a context they do not create themselves through
  // GMG_OPTIONS="key=value,key=value" (same keys as gmg_set_option); unknown keys fail the creation
  if (const char *env = std::getenv("GMG_OPTIONS")) {
    std::string all(env);
    size_t pos = 0;
    while (pos < all.size()) {
      size_t end = all.find(',', pos);
      if (end == std::string::npos) end = all.size();
      const std::string item = all.substr(pos, end - pos);
      pos = end + 1;
      const size_t eq = item.find('=');
      if (item.empty()) continue;
      const std::string key = eq == std::string::npos ? item : item.substr(0, eq);
      const double v = eq == std::string::npos ? 1.0 : std::atof(item.c_str() + eq + 1);
      if (gmg_set_option(ctx, key.c_str(), v) != GMG_OK) return bail(GMG_ERR_INVALID);
    }
  }
  *out = ctx;
  return GMG_OK;
}

int gmg_destroy(gmg_context *ctx) {
  if (!ctx) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  release_operators(ctx);  // (before the communicator: the shared direction vectors are unmapped collectively)
  comm_destroy(ctx->comm);
  const hipStream_t stream = ctx->stream;
  delete ctx;  // every other allocation and event: by its owner
  if (stream) (void)hipStreamDestroy(stream);
  return GMG_OK;
}

int gmg_reset(gmg_context *ctx, int n_levels) {
  if (!ctx || n_levels < 1) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  HIPC(hipStreamSynchronize(ctx->stream));
  release_operators(ctx);
  free_locator(ctx);
  if (!ctx->reset_keeps_mesh_tables) ctx->mesh = MeshTables();
  ctx->refined = RefinedForest();
  ctx->n_levels = n_levels;
  ctx->lv.clear();
  ctx->lv.resize((size_t)n_levels);
  // the levels' copy_version restart at 0: a hierarchy of the same sizes would repeat the signature of the fused copies' tables
  ctx->mgcopy_sig.clear(); ctx->mgcopy_ok = false;
  ctx->last_coarse_iters = 0;
  ctx->stats = gmg_stats{};
  ctx->ev3_used = 0;
  return GMG_OK;
}

const char *gmg_last_error(const gmg_context *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int gmg_synchronize(gmg_context *ctx) {
  if (!ctx) return GMG_ERR_INVALID;
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

int gmg_set_system_matrix(gmg_context *ctx, int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col,
                          const double *val) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  CHK(upload_csr(ctx, ctx->S, n_rows, n_cols, rowptr, col, val, false, true));
  CHK(setup_diag(ctx, n_rows, rowptr, col, val, ctx->S_invd, nullptr));
  CHK(alloc_vec(ctx, ctx->S_tmp, n_cols));
  if (ctx->dist) {
    const int64_t padded = part_chunk(ctx->sys_global, ctx->comm.n_ranks) * ctx->comm.n_ranks;
    CHK(alloc_vec(ctx, ctx->sys_full_a, padded));
    CHK(alloc_vec(ctx, ctx->sys_full_b, padded));
    int64_t b, e;
    part_range(ctx->sys_global, ctx->comm.rank, ctx->comm.n_ranks, &b, &e);
    if (e - b != n_rows) return fail(ctx, GMG_ERR_INVALID, "system matrix rows do not match the canonical partition");
  }
  return GMG_OK;
}

// what a level needs besides its operator: work vectors and, on level 0, the coarse CG's vectors and the shape the bench reads
static int finish_level(gmg_context *ctx, int level, int64_t n_rows, int64_t n_cols, int64_t nnz) {
  Level &L = ctx->lv[(size_t)level];
  L.n = n_rows;
  L.n_vec = n_cols;
  for (DevPtr<double> *p : {&L.sol, &L.def, &L.t, &L.w1, &L.w2, &L.w3}) CHK(alloc_vec(ctx, *p, n_cols));
  if (level == 0) {
    if (l0_partitioned(ctx)) {
      const int64_t padded = part_chunk(ctx->l0_global, ctx->comm.n_ranks) * ctx->comm.n_ranks;
      CHK(alloc_vec(ctx, L.sol_full_own, padded));
      CHK(alloc_vec(ctx, L.def_full_own, padded));
      L.sol_full = L.sol_full_own.get();
      L.def_full = L.def_full_own.get();
    } else {
      L.sol_full_own.reset(); L.def_full_own.reset();
      L.sol_full = L.sol.get();
      L.def_full = L.def.get();
    }
    ctx->cg_n = n_cols;
    for (DevPtr<double> *p : {&ctx->cg_g, &ctx->cg_d0, &ctx->cg_d1, &ctx->cg_h}) CHK(alloc_vec(ctx, *p, n_cols));
    free_cg_ring(ctx);  // sized for the previous level 0
    ctx->stats.spmv0_rows = n_rows;
    ctx->stats.spmv0_nnz = nnz;
    ctx->stats.spmv0_layout = L.A.sell ? 1 + (L.A.val8 ? 2 : 0) + (L.A.col16 ? 4 : 0) + (L.A.use_sellp ? 8 : 0) : 0;
    if (L.A.sell) {
      const double frac_stream = L.A.n_slices ? 1.0 - (double)L.A.n_pattern_slices / L.A.n_slices : 1.0;
      const int64_t ent = L.A.sell_quads * 256;
      // row classes: the run-pattern slices stream one byte per row instead of one per entry
      const int64_t val_bytes = L.A.rowclass ? (int64_t)(frac_stream * (double)ent) + (int64_t)L.A.n_pattern_slices * 64 : ent * (L.A.val8 ? 1 : 8);
      ctx->stats.spmv0_matrix_bytes = val_bytes + (int64_t)(frac_stream * (double)ent * (L.A.col16 ? 2 : 4)) + 8 * (int64_t)L.A.n_slices;
      if (L.A.rowclass) ctx->stats.spmv0_layout += 16;
      if (L.A.lattice) {  // one class byte per interior row + the streams of the slices outside
        ctx->stats.spmv0_layout += 32;
        ctx->stats.spmv0_matrix_bytes = L.A.lat_fast_rows + L.A.lat_gen_bytes;
      }
    } else if (L.A.lat_only) {  // class table only: one class byte per row
      ctx->stats.spmv0_layout = 1 + 2 + 4 + 8 + 16 + 32 + 64;
      ctx->stats.spmv0_matrix_bytes = n_rows;
    } else {
      ctx->stats.spmv0_matrix_bytes = 12 * nnz + 4 * (n_rows + 1);
    }
    ctx->stats.spmv0_pattern_slices = L.A.n_pattern_slices;
    ctx->stats.spmv0_slices = L.A.n_slices;
    ctx->last_coarse_iters = 0;
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

int gmg_set_level_matrix(gmg_context *ctx, int level, int64_t n_rows, int64_t n_cols, const int64_t *rowptr,
                         const int32_t *col, const double *val) {
  if (!ctx || level < 0 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const auto ex = level > 0 ? ctx->ssor_block_rows.find(level) : ctx->ssor_block_rows.end();
  const std::vector<int64_t> *explicit_rows = ex == ctx->ssor_block_rows.end() ? nullptr : &ex->second;
  if (explicit_rows && explicit_rows->back() != n_rows)  // (before anything is uploaded)
    return fail(ctx, GMG_ERR_INVALID, "gmg_set_level_matrix: the SSOR block boundaries of this level (gmg_set_ssor_block_rows) do not end at n_rows");
  (void)hipSetDevice(ctx->device);
  Level &L = ctx->lv[(size_t)level];
  if (level == 0) drop_coarse_direct(ctx);  // (a new level 0: back to the coarse CG)
  L.cheb_est = Level::ChebEstimate();       // (a new matrix: its own bound)
  CHK(upload_csr(ctx, L.A, n_rows, n_cols, rowptr, col, val, level > 0));
  CHK(setup_diag(ctx, n_rows, rowptr, col, val, L.invd, &L.cheb_lmax));
  if (level > 0) {
    L.n = n_rows;  // (the SGS plan reads it)
    if (ctx->ssor_plan_device) {
      // the device builder reads an int32 CSR: a copy of this call's arrays (upload_csr may have kept another layout)
      DevPtr<int32_t> d_rp, d_col;
      DevPtr<double> d_val;
      if (!sgs_device_refusal(ctx, explicit_rows != nullptr, n_rows) && n_rows > 0) {
        if (rowptr[n_rows] > INT32_MAX) return fail(ctx, GMG_ERR_INVALID, "gmg_set_level_matrix: more than 2^31 entries");
        const std::vector<int32_t> rp32(rowptr, rowptr + n_rows + 1);
        HIPC(upload(d_rp, rp32, ctx->stream));
        HIPC(upload(d_col, col, (size_t)rowptr[n_rows], ctx->stream));
        HIPC(upload(d_val, val, (size_t)rowptr[n_rows], ctx->stream));
        HIPC(hipStreamSynchronize(ctx->stream));  // (rp32 leaves scope)
      }
      const int rc_plan = setup_sgs_any(ctx, L, n_rows, d_rp.get(), d_col.get(), d_val.get(), rowptr, col, val, explicit_rows,
                                        [](const int32_t **, const double **, int64_t *) { return (int)GMG_OK; });
      if (rc_plan != GMG_OK) {  // (a plan that failed its checks, or a HIP error on the way: the level is left without an operator, never a new matrix with an old plan)
        reset_keep_halo(L.A);
        L.invd.reset();
        L.cheb_lmax = 0.0;
        L.cheb_est = Level::ChebEstimate();
        L.sgs = SgsPlan();
        return rc_plan;
      }
    } else {
      CHK(setup_sgs(ctx, L, n_rows, rowptr, col, val, explicit_rows));
    }
  }
  return finish_level(ctx, level, n_rows, n_cols, rowptr[n_rows]);
}

// The level matrix of an UNDIVIDED lattice level formed on the device: what gmg_set_level_matrix would
// have received as CSR from assemble_multigrid (src/step-50.cc:869-889) for nv[0] x nv[1] x nv[2] vertices numbered
// lexicographically, every cell adding the same 8 x 8 matrix Ke, all faces Dirichlet (MGConstrainedDoFs, :704-706):
//   boundary vertex i:            a_ii = sum over its cells of |Ke[a][a]|, stored zeros elsewhere        (:877-879)
//   interior vertex i, column j:  sum over the cells holding both of Ke[a_i][a_j], 0 if j is on the boundary
// -- the sums in cell order (z, y, x ascending), from 0.0, exactly as CSRMatrix::add forms them: the same bits.  A vertex's
// 27 coefficients depend only on its position type per direction (on the low face / next to it / inside / next to the
// high face / on it): 125 classes.  The table is 125 x 27 numbers (host, microseconds); the per-row work -- class byte and
// 1 / a_ii of 10^6..10^7 rows -- is a kernel.  No CSR, no upload.
int gmg_set_level_matrix_lattice(gmg_context *ctx, int level, const int32_t nv[3], const double Ke[64]) {
  if (!ctx || !nv || !Ke || level < 0 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  if (level != 0) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_set_level_matrix_lattice: level 0 only (finer levels of an adaptive hierarchy are patches, and their smoothers need the rows)");
  if (l0_partitioned(ctx)) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_set_level_matrix_lattice: a row-partitioned level 0 takes its local rows as CSR (gmg_set_level_matrix)");
  const int64_t nx = nv[0], ny = nv[1], nz = nv[2];
  if (nx < 5 || ny < 5 || nz < 5) return fail(ctx, GMG_ERR_INVALID, "gmg_set_level_matrix_lattice: at least 5 vertices per direction");
  const int64_t n = nx * ny * nz, nxy = nx * ny, reach = nxy + nx + 1;
  if (n >= ((int64_t)1 << 28)) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_set_level_matrix_lattice: more than 2^28 rows");
  (void)hipSetDevice(ctx->device);
  Level &L = ctx->lv[0];
  DevCSR &m = L.A;
  drop_coarse_direct(ctx);  // (a new level 0: back to the coarse CG)
  reset_keep_halo(m);
  L.cheb_est = Level::ChebEstimate();
  for (int d = 0; d < 3; ++d) m.lat_nv[d] = nv[d];
  std::copy(Ke, Ke + 64, m.lat_Ke);
  // ---- class table
  const int64_t dims[3] = {nx, ny, nz};
  auto rep = [&](int t, int64_t mdim) -> int64_t { return t == 0 ? 0 : t == 1 ? 1 : t == 2 ? 2 : t == 3 ? mdim - 2 : mdim - 1; };
  std::vector<double> ctab((size_t)125 * 27, 0.0);
  double lmax = 0.0;
  for (int cls = 0; cls < 125; ++cls) {
    const int t[3] = {cls % 5, (cls / 5) % 5, cls / 25};
    int64_t v[3];
    bool v_bnd = false;
    for (int d = 0; d < 3; ++d) { v[d] = rep(t[d], dims[d]); v_bnd = v_bnd || v[d] == 0 || v[d] == dims[d] - 1; }
    double rowsum = 0.0;
    for (int j = 0; j < 27; ++j) {
      const int dd[3] = {j % 3 - 1, (j / 3) % 3 - 1, j / 9 - 1};
      int64_t u[3];
      bool exists = true, u_bnd = false;
      for (int d = 0; d < 3; ++d) {
        u[d] = v[d] + dd[d];
        exists = exists && u[d] >= 0 && u[d] < dims[d];
        u_bnd = u_bnd || u[d] == 0 || u[d] == dims[d] - 1;
      }
      double acc = 0.0;
      if (exists && ((v_bnd && j == 13) || (!v_bnd && !u_bnd))) {
        // the cells that hold both vertices, in cell order (z, y, x ascending)
        int64_t lo[3], hi[3];
        for (int d = 0; d < 3; ++d) { lo[d] = std::max<int64_t>(std::max(v[d], u[d]) - 1, 0); hi[d] = std::min<int64_t>(std::min(v[d], u[d]), dims[d] - 2); }
        for (int64_t cz = lo[2]; cz <= hi[2]; ++cz)
          for (int64_t cy = lo[1]; cy <= hi[1]; ++cy)
            for (int64_t cx = lo[0]; cx <= hi[0]; ++cx) {
              const int a = (int)((v[0] - cx) + 2 * (v[1] - cy) + 4 * (v[2] - cz)), b = (int)((u[0] - cx) + 2 * (u[1] - cy) + 4 * (u[2] - cz));
              acc += v_bnd ? std::fabs(Ke[a * 8 + a]) : Ke[a * 8 + b];
            }
      }
      ctab[(size_t)cls * 27 + (size_t)j] = acc;
      rowsum += std::fabs(acc);
    }
    lmax = std::max(lmax, rowsum / std::fabs(ctab[(size_t)cls * 27 + 13]));  // Gershgorin bound of D^-1 A (every class occurs for n >= 5)
  }
  // position types with the same 27 coefficients share a class (most of the 125 do: the table every workgroup copies into
  // its LDS shrinks to ~30 rows)
  LatticeClassMap cmap{};
  std::vector<double> utab;
  int n_unique = 0;
  for (int cls = 0; cls < 125; ++cls) {
    int found = -1;
    for (int q = 0; q < n_unique && found < 0; ++q)
      if (std::memcmp(&utab[(size_t)q * 27], &ctab[(size_t)cls * 27], sizeof(double) * 27) == 0) found = q;
    if (found < 0) {
      found = n_unique++;
      utab.insert(utab.end(), ctab.begin() + (std::ptrdiff_t)cls * 27, ctab.begin() + (std::ptrdiff_t)(cls + 1) * 27);
    }
    cmap.cls[cls] = (uint8_t)found;
  }
  HIPC(m.lat_rowcls.alloc_bytes((size_t)n + 64));
  HIPC(m.lat_ctab.alloc(utab.size()));
  HIPC(hipMemcpyAsync(m.lat_ctab.get(), utab.data(), sizeof(double) * utab.size(), hipMemcpyHostToDevice, ctx->stream));
  CHK(alloc_vec(ctx, L.invd, n));
  hipLaunchKernelGGL(lattice_rowclass_kernel, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, m.lat_rowcls.get(), L.invd.get(), (const double *)m.lat_ctab.get(), cmap, (int)nx, (int)ny, (int)nz);
  CHK(launch_status(ctx));
  HIPC(hipStreamSynchronize(ctx->stream));  // (utab dies with this scope)
  L.cheb_lmax = lmax;
  m.n_rows = m.n_cols = n;
  m.nnz = (3 * nx - 2) * (3 * ny - 2) * (3 * nz - 2);
  m.lat_classes = n_unique;
  m.lat_nx = (int)nx; m.lat_nxy = (int)nxy; m.lat_W = (int)nxy;
  m.lat_R0 = (int)(reach + 2); m.lat_R1 = (int)(n - reach);
  if (m.lat_R1 - m.lat_R0 < nxy) return fail(ctx, GMG_ERR_INVALID, "gmg_set_level_matrix_lattice: fewer than five planes");
  m.lat_C = (int)((nxy + kLatRowsPerUnit - 1) / kLatRowsPerUnit);
  m.lat_K = (int)((m.lat_R1 - m.lat_R0 + nxy - 1) / nxy);
  m.lat_fast_rows = m.lat_R1 - m.lat_R0;
  m.lat_n_gen = (m.lat_R0 + 63) / 64 + (int)((n - m.lat_R1 + 63) / 64);
  m.lat_gen_bytes = (int64_t)m.lat_n_gen * 64;
  LatticePlan grid;
  grid.C = m.lat_C; grid.K = m.lat_K;
  m.lat_grid = lattice_grid(layout_options(ctx), grid, (size_t)m.lat_n_gen);
  m.lat_S = grid.S; m.lat_fast_blocks = grid.fast_blocks;
  m.lat_grid += m.lat_fast_blocks;
  if (m.lat_grid > kMaxPartials) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_set_level_matrix_lattice: grid exceeds the reduction partials");
  m.valid = true;
  m.lattice = m.lat_only = true;
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] lattice operator %lld x %lld x %lld formed on the device: %d columns x %d steps, %d segments per XCD slab, grid %d, %d edge chunks\n", (long long)nx,
                 (long long)ny, (long long)nz, m.lat_C, m.lat_K, m.lat_S, m.lat_grid, m.lat_n_gen);
  CHK(finish_level(ctx, 0, n, n, m.nnz));
  if (ctx->coarse_direct_opt) {  // option coarse_direct: the direct coarse solver where this level 0 qualifies, the CG otherwise
    const int rc = select_coarse_direct(ctx);
    if (rc != GMG_OK && rc != GMG_ERR_UNSUPPORTED) return rc;
    if (rc == GMG_ERR_UNSUPPORTED) ctx->err.clear();
  }
  return GMG_OK;
}

int gmg_set_edge_matrix(gmg_context *ctx, int level, int64_t n_rows, int64_t n_cols, const int64_t *rowptr,
                        const int32_t *col, const double *val) {
  if (!ctx || level < 0 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  Level &L = ctx->lv[(size_t)level];
  // stored zeros contribute nothing to vmult_add / Tvmult: prune them (most of I_l is zero)
  std::vector<int64_t> rp((size_t)n_rows + 1, 0);
  std::vector<int32_t> c;
  std::vector<double> v;
  for (int64_t i = 0; i < n_rows; ++i) {
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      if (val[k] != 0.0) { c.push_back(col[k]); v.push_back(val[k]); }
    rp[(size_t)i + 1] = (int64_t)c.size();
  }
  L.has_I = !c.empty();
  if (!L.has_I) { L.I = DevCSR(); L.It = DevCSR(); return GMG_OK; }
  CHK(upload_csr(ctx, L.I, n_rows, n_cols, rp.data(), c.data(), v.data()));
  std::vector<int64_t> trp;
  std::vector<int32_t> tcol;
  std::vector<double> tval;
  transpose_host(n_rows, n_cols, rp.data(), c.data(), v.data(), trp, tcol, tval);
  CHK(upload_csr(ctx, L.It, n_cols, n_rows, trp.data(), tcol.data(), tval.data()));
  return GMG_OK;
}

int gmg_set_prolongation(gmg_context *ctx, int level, int64_t n_fine, int64_t n_coarse, const int64_t *rowptr,
                         const int32_t *col, const double *val) {
  if (!ctx || level < 0 || level >= ctx->n_levels - 1) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  Level &L = ctx->lv[(size_t)level];
  CHK(upload_csr(ctx, L.P, n_fine, n_coarse, rowptr, col, val));
  std::vector<int64_t> trp;
  std::vector<int32_t> tcol;
  std::vector<double> tval;
  transpose_host(n_fine, n_coarse, rowptr, col, val, trp, tcol, tval);
  CHK(upload_csr(ctx, L.Pt, n_coarse, n_fine, trp.data(), tcol.data(), tval.data()));
  L.has_P = true;
  return GMG_OK;
}

// MGTransferPrebuilt::build_matrices on the device (gmg_transfer.hpp): P_level and its transpose from the vertices of the
// DoFs of the two levels.  build_ms (may be null): device time of the build, the part the reference counts in its Solve timer.
int gmg_build_transfer(gmg_context *ctx, int level, int dim, int64_t n_coarse, const uint64_t *coarse_vertex, const uint8_t *coarse_boundary,
                       int64_t n_fine, const uint64_t *fine_vertex, uint64_t fine_spacing, double *build_ms) {
  if (!ctx || level < 0 || level >= ctx->n_levels - 1 || (dim != 2 && dim != 3) || n_coarse <= 0 || n_fine <= 0 || !coarse_vertex || !coarse_boundary ||
      !fine_vertex || fine_spacing == 0 || (fine_spacing & (fine_spacing - 1)) != 0)
    return GMG_ERR_INVALID;
  if (n_coarse >= ((int64_t)1 << 30) || n_fine >= ((int64_t)1 << 28)) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_build_transfer: level too large for 32-bit row pointers");
  (void)hipSetDevice(ctx->device);
  Level &L = ctx->lv[(size_t)level];
  for (DevCSR *m : {&L.P, &L.Pt}) reset_keep_halo(*m);
  DevPtr<unsigned long long> d_fv, d_cv, d_fk, d_ck;
  DevPtr<uint8_t> d_cb;
  DevPtr<int32_t> d_fd, d_cd;
  Event e0, e1;
  auto table_size = [](int64_t n) { unsigned long long t = 1024; while ((int64_t)t < 2 * n) t <<= 1; return t; };
  const unsigned long long ft = table_size(n_fine), ct = table_size(n_coarse);
  HIPC(d_fv.alloc((size_t)n_fine));
  HIPC(d_cv.alloc((size_t)n_coarse));
  HIPC(d_cb.alloc((size_t)n_coarse));
  HIPC(d_fk.alloc(ft));
  HIPC(d_ck.alloc(ct));
  HIPC(d_fd.alloc(ft));
  HIPC(d_cd.alloc(ct));
  HIPC(hipMemcpyAsync(d_fv.get(), fine_vertex, sizeof(uint64_t) * (size_t)n_fine, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_cv.get(), coarse_vertex, sizeof(uint64_t) * (size_t)n_coarse, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_cb.get(), coarse_boundary, (size_t)n_coarse, hipMemcpyHostToDevice, ctx->stream));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  HIPC(hipMemsetAsync(d_fk.get(), 0xff, sizeof(uint64_t) * ft, ctx->stream));
  HIPC(hipMemsetAsync(d_ck.get(), 0xff, sizeof(uint64_t) * ct, ctx->stream));
  hipLaunchKernelGGL(tr_table_build_kernel, dim3(grid_for(n_fine)), dim3(kThreads), 0, ctx->stream, (const unsigned long long *)d_fv.get(), n_fine, d_fk.get(), d_fd.get(), ft - 1);
  hipLaunchKernelGGL(tr_table_build_kernel, dim3(grid_for(n_coarse)), dim3(kThreads), 0, ctx->stream, (const unsigned long long *)d_cv.get(), n_coarse, d_ck.get(), d_cd.get(), ct - 1);
  TransferArgs a{};
  a.fine_vertex = d_fv.get(); a.coarse_vertex = d_cv.get(); a.coarse_boundary = d_cb.get(); a.n_fine = n_fine; a.n_coarse = n_coarse;
  a.fkeys = d_fk.get(); a.ckeys = d_ck.get(); a.fdof = d_fd.get(); a.cdof = d_cd.get(); a.fmask = ft - 1; a.cmask = ct - 1; a.dim = dim; a.half = fine_spacing;
  // one operator after the other: count, scan, allocate, fill
  auto build = [&](DevCSR &m, bool transposed) -> int {
    const int64_t nr = transposed ? n_coarse : n_fine, nc = transposed ? n_fine : n_coarse;
    HIPC(m.rowptr.alloc(((size_t)nr + 1)));
    a.rowptr = m.rowptr.get();
    if (transposed) hipLaunchKernelGGL(tr_restriction_kernel<false>, dim3(grid_for(nr)), dim3(kThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL(tr_prolongation_kernel<false>, dim3(grid_for(nr)), dim3(kThreads), 0, ctx->stream, a);
    hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, m.rowptr.get(), nr);
    int32_t nnz = 0;
    HIPC(hipMemcpyAsync(&nnz, m.rowptr.get() + nr, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    const size_t pad = 8;
    HIPC(m.col.alloc(((size_t)nnz + pad)));
    HIPC(m.val.alloc(((size_t)nnz + pad)));
    HIPC(hipMemsetAsync(m.col.get() + nnz, 0, sizeof(int32_t) * pad, ctx->stream));
    HIPC(hipMemsetAsync(m.val.get() + nnz, 0, sizeof(double) * pad, ctx->stream));
    a.col = m.col.get(); a.val = m.val.get();
    if (transposed) hipLaunchKernelGGL(tr_restriction_kernel<true>, dim3(grid_for(nr)), dim3(kThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL(tr_prolongation_kernel<true>, dim3(grid_for(nr)), dim3(kThreads), 0, ctx->stream, a);
    m.n_rows = nr; m.n_cols = nc; m.nnz = nnz;
    return launch_status(ctx);
  };
  int rc = build(L.P, false);
  if (rc == GMG_OK) rc = build(L.Pt, true);
  if (rc == GMG_OK && hipEventRecord(e1.get(), ctx->stream) != hipSuccess) rc = GMG_ERR_HIP;
  // the row-window tiling of the two operators (host: a pass over the row pointers)
  for (DevCSR *m : {&L.P, &L.Pt}) {
    if (rc != GMG_OK) break;
    std::vector<int32_t> rp((size_t)m->n_rows + 1);
    if (hipMemcpyAsync(rp.data(), m->rowptr.get(), sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = GMG_ERR_HIP; break; }
    const TilePlan T = plan_tiles(rp.data(), m->n_rows);
    set_tiles(*m, T);
    if (upload(m->tile_row, T.tile_row, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = GMG_ERR_HIP; break; }
    m->valid = true;
  }
  float ms = 0.f;
  if (rc == GMG_OK && hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (rc != GMG_OK) { if (ctx->err.empty()) ctx->err = "gmg_build_transfer failed"; return rc; }
  L.has_P = true;
  ctx->stats.build_matrices_ms += ms;
  if (build_ms) *build_ms = ms;
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] transfer %d -> %d built on the device: P %lld x %lld nnz %lld, P^T nnz %lld, %.3f ms\n", level, level + 1, (long long)n_fine, (long long)n_coarse,
                 (long long)L.P.nnz, (long long)L.Pt.nnz, ms);
  return GMG_OK;
}

// CSR of P_level (transposed = 0) or its transpose as the device holds it (tests): sizes first (arrays null), then the copy
int gmg_get_transfer(gmg_context *ctx, int level, int transposed, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int64_t *rowptr, int32_t *col, double *val) {
  if (!ctx || level < 0 || level >= ctx->n_levels - 1) return GMG_ERR_INVALID;
  const DevCSR &m = transposed ? ctx->lv[(size_t)level].Pt : ctx->lv[(size_t)level].P;
  if (!m.valid || !m.rowptr.get() || !m.col.get() || !m.val.get()) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_get_transfer: no CSR copy of this operator on the device");
  if (n_rows) *n_rows = m.n_rows;
  if (n_cols) *n_cols = m.n_cols;
  if (nnz) *nnz = m.nnz;
  if (!rowptr) return GMG_OK;
  std::vector<int32_t> rp((size_t)m.n_rows + 1);
  HIPC(hipMemcpyAsync(rp.data(), m.rowptr.get(), sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (m.nnz) {
    HIPC(hipMemcpyAsync(col, m.col.get(), sizeof(int32_t) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(val, m.val.get(), sizeof(double) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < rp.size(); ++i) rowptr[i] = rp[i];
  return GMG_OK;
}

int gmg_set_copy_indices(gmg_context *ctx, int level, int64_t n, const int32_t *global_idx, const int32_t *level_idx) {
  if (!ctx || level < 0 || level >= ctx->n_levels || n < 0) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  Level &L = ctx->lv[(size_t)level];
  L.copy_g.reset(); L.copy_l.reset();
  L.n_copy = n;
  L.copy_version++;
  L.host_copy_g.assign(global_idx, global_idx + (n ? n : 0));
  L.host_copy_l.assign(level_idx, level_idx + (n ? n : 0));
  if (n > 0) {
    HIPC(L.copy_g.alloc((size_t)n));
    HIPC(L.copy_l.alloc((size_t)n));
    HIPC(hipMemcpyAsync(L.copy_g.get(), global_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(L.copy_l.get(), level_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  // the inverse indices of the fused copies are part of the upload: built with the finest level's list, the last one a
  // hierarchy is given (any other order: the first V-cycle builds them)
  if (level == ctx->n_levels - 1 && ctx->S.valid && !ctx->dist) {
    bool complete = true;
    for (const Level &K : ctx->lv) complete = complete && K.A.valid;
    if (complete) CHK(mg_copy_tables(ctx));
  }
  return GMG_OK;
}

int gmg_set_smoother(gmg_context *ctx, int kind, double omega, int steps, int cheb_degree, double cheb_ratio,
                     double cheb_lmax) {
  if (!ctx || kind < 0 || kind > 2 || steps < 0) return GMG_ERR_INVALID;
  ctx->smoother = kind; ctx->omega = omega; ctx->steps = steps;
  if (cheb_degree > 0) ctx->cheb_degree = cheb_degree;
  if (cheb_ratio > 0) ctx->cheb_ratio = cheb_ratio;
  ctx->cheb_lmax_user = cheb_lmax;
  return GMG_OK;
}

// a bound formed with other steps or another safety factor is not the one asked for: every level estimates again
static void drop_cheb_estimates(gmg_context *ctx) {
  for (Level &L : ctx->lv) L.cheb_est = Level::ChebEstimate();
}

int gmg_set_chebyshev(gmg_context *ctx, int polynomial, int lmax_source, int lanczos_steps, double safety) {
  if (!ctx) return GMG_ERR_INVALID;
  if (polynomial != GMG_CHEB_FIRST_KIND && polynomial != GMG_CHEB_FOURTH_KIND) return fail(ctx, GMG_ERR_INVALID, "gmg_set_chebyshev: unknown polynomial");
  if (lmax_source != GMG_CHEB_LMAX_GERSHGORIN && lmax_source != GMG_CHEB_LMAX_LANCZOS) return fail(ctx, GMG_ERR_INVALID, "gmg_set_chebyshev: unknown lmax source");
  if (lanczos_steps < 0 || lanczos_steps > lanczos::kMaxSteps) return fail(ctx, GMG_ERR_INVALID, "gmg_set_chebyshev: 1 .. 64 Lanczos steps (0 keeps the value)");
  if (!(safety == 0.0 || (safety >= 1.0 && std::isfinite(safety)))) return fail(ctx, GMG_ERR_INVALID, "gmg_set_chebyshev: a safety factor >= 1 (0 keeps the value)");
  ctx->cheb_polynomial = polynomial;
  ctx->cheb_lmax_source = lmax_source;
  if (lanczos_steps > 0 && lanczos_steps != ctx->cheb_lanczos_steps) { ctx->cheb_lanczos_steps = lanczos_steps; drop_cheb_estimates(ctx); }
  if (safety > 0.0 && safety != ctx->cheb_safety) { ctx->cheb_safety = safety; drop_cheb_estimates(ctx); }
  return GMG_OK;
}

int gmg_estimate_lmax(gmg_context *ctx, int level, int steps, double *ritz, double *alpha, double *beta, int *steps_run) {
  if (!ctx) return GMG_ERR_INVALID;
  if (level < 0 || level >= ctx->n_levels) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_lmax: level outside the context");
  if (!ritz || !steps_run) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_lmax: ritz and steps_run expected");
  if (steps < 1 || steps > lanczos::kMaxSteps) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_lmax: 1 .. 64 steps");
  (void)hipSetDevice(ctx->device);
  return lanczos_estimate(ctx, ctx->lv[(size_t)level], level, steps, ritz, alpha, beta, steps_run);
}

int gmg_get_chebyshev(gmg_context *ctx, int level, double out[8]) {
  if (!ctx || !out || level < 0 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const Level &L = ctx->lv[(size_t)level];
  const bool lanczos_src = ctx->cheb_lmax_source == GMG_CHEB_LMAX_LANCZOS;
  out[0] = ctx->cheb_polynomial; out[1] = ctx->cheb_lmax_source; out[2] = ctx->cheb_lanczos_steps;
  out[3] = L.cheb_est.valid ? L.cheb_est.steps_run : 0;
  out[4] = L.A.valid ? L.cheb_lmax : 0.0;
  out[5] = L.cheb_est.valid ? L.cheb_est.ritz : 0.0;
  out[6] = ctx->cheb_safety;
  // (the Lanczos bound is formed at the level's first Chebyshev use: 0 until then)
  out[7] = !L.A.valid ? 0.0 : ctx->cheb_lmax_user > 0 ? ctx->cheb_lmax_user : (lanczos_src && !L.cheb_est.valid) ? 0.0 : cheb_lambda(ctx, L);
  return GMG_OK;
}

int gmg_set_coarse(gmg_context *ctx, double abs_tol, int max_it) {
  if (!ctx || max_it < 1) return GMG_ERR_INVALID;
  ctx->coarse_tol = abs_tol; ctx->coarse_maxit = max_it;
  return GMG_OK;
}

int gmg_set_coarse_solver(gmg_context *ctx, int kind) {
  if (!ctx) return GMG_ERR_INVALID;
  if (kind == GMG_COARSE_CG) {
    HIPC(hipStreamSynchronize(ctx->stream));  // (a solve still in flight uses the tables)
    drop_coarse_direct(ctx);
    return GMG_OK;
  }
  if (kind != GMG_COARSE_DIRECT) return fail(ctx, GMG_ERR_INVALID, "gmg_set_coarse_solver: GMG_COARSE_CG or GMG_COARSE_DIRECT");
  HIPC(hipStreamSynchronize(ctx->stream));
  return select_coarse_direct(ctx);
}

int gmg_coarse_direct_tables(int n_cells, double *S, double *lambda, double *mu) {
  if (n_cells < fastdiag::kMinNv - 1 || n_cells > fastdiag::kMaxNv - 1 || (!S && !lambda && !mu)) return GMG_ERR_INVALID;
  fastdiag::tables(n_cells, S, lambda, mu);
  return GMG_OK;
}

int gmg_coarse_direct_separable(const double Ke[64], double *s) {
  if (!Ke) return GMG_ERR_INVALID;
  return fastdiag::separable(Ke, s) ? GMG_OK : GMG_ERR_UNSUPPORTED;
}

int gmg_coarse_direct_profile(gmg_context *ctx, double *dst, const double *src, double pass_ms[7]) {
  if (!ctx || !dst || !src || !pass_ms) return GMG_ERR_INVALID;
  if (ctx->coarse_solver != GMG_COARSE_DIRECT || !ctx->fd.ready) return fail(ctx, GMG_ERR_INVALID, "gmg_coarse_direct_profile: the direct coarse solver is not selected");
  Level &L0 = ctx->lv[0];
  Event ev[14];
  for (auto &e : ev) HIPC(e.create());
  HIPC(hipMemcpyAsync(L0.def.get(), src, sizeof(double) * (size_t)L0.n, hipMemcpyDeviceToDevice, ctx->stream));
  CHK(coarse_solve_direct(ctx, L0.sol.get(), L0.def.get(), nullptr, nullptr, ev));
  HIPC(hipMemcpyAsync(dst, L0.sol.get(), sizeof(double) * (size_t)L0.n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 7; ++k) {
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, ev[2 * k].get(), ev[2 * k + 1].get()));
    pass_ms[k] = ms;
  }
  return GMG_OK;
}

int gmg_coarse_direct_transform(gmg_context *ctx, int axis, double *dst, const double *src) {
  if (!ctx || !dst || !src) return GMG_ERR_INVALID;
  if (axis < 0 || axis > 2) return fail(ctx, GMG_ERR_INVALID, "gmg_coarse_direct_transform: axis 0, 1 or 2");
  if (dst == src) return fail(ctx, GMG_ERR_INVALID, "gmg_coarse_direct_transform: dst and src must differ");
  if (ctx->coarse_solver != GMG_COARSE_DIRECT || !ctx->fd.ready) return fail(ctx, GMG_ERR_INVALID, "gmg_coarse_direct_transform: the direct coarse solver is not selected");
  launch_fastdiag_pass(ctx, axis, dst, src, false);
  RETURN_LAUNCHED(ctx);
}

// ---- vectors ----
// (gmg_vec_alloc hands the allocation to the caller over the C ABI, gmg_vec_free takes it back: no owner in between)

int gmg_vec_alloc(gmg_context *ctx, int64_t n, double **dptr) {
  if (!ctx || !dptr || n < 0) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  *dptr = nullptr;
  DevPtr<double> v;
  CHK(alloc_vec(ctx, v, n));
  *dptr = v.release();  // (the caller's from here on, until gmg_vec_free)
  return GMG_OK;
}
int gmg_vec_free(gmg_context *ctx, double *dptr) {
  if (!ctx) return GMG_ERR_INVALID;
  if (dptr) { HIPC(hipStreamSynchronize(ctx->stream)); HIPC(hipFree(dptr)); }
  return GMG_OK;
}
int gmg_vec_upload(gmg_context *ctx, double *dst, const double *src, int64_t n) {
  if (!ctx || n < 0) return GMG_ERR_INVALID;
  if (n) HIPC(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}
int gmg_vec_download(gmg_context *ctx, double *dst, const double *src, int64_t n) {
  if (!ctx || n < 0) return GMG_ERR_INVALID;
  if (n) HIPC(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}
int gmg_vec_set_zero(gmg_context *ctx, double *x, int64_t n) {
  if (!ctx || n < 0) return GMG_ERR_INVALID;
  if (n) HIPC(hipMemsetAsync(x, 0, sizeof(double) * (size_t)n, ctx->stream));
  return GMG_OK;
}
int gmg_vec_equ(gmg_context *ctx, double *y, double a, const double *x, int64_t n) {
  if (!ctx || n < 0) return GMG_ERR_INVALID;
  if (n) hipLaunchKernelGGL(vec_equ_kernel, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, y, a, x, n);
  RETURN_LAUNCHED(ctx);
}
int gmg_vec_add(gmg_context *ctx, double *y, double a, const double *x, int64_t n) {
  if (!ctx || n < 0) return GMG_ERR_INVALID;
  if (n) hipLaunchKernelGGL(vec_add_kernel, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, y, a, x, n);
  RETURN_LAUNCHED(ctx);
}
int gmg_vec_sadd(gmg_context *ctx, double *y, double s, double a, const double *x, int64_t n) {
  if (!ctx || n < 0) return GMG_ERR_INVALID;
  if (n) hipLaunchKernelGGL(vec_sadd_kernel, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, y, s, a, x, n);
  RETURN_LAUNCHED(ctx);
}
int gmg_vec_dot(gmg_context *ctx, const double *x, const double *y, int64_t n, double *out) {
  if (!ctx || !out || n < 0) return GMG_ERR_INVALID;
  return dot_host(ctx, x, y, n, out);
}
int gmg_vec_norms(gmg_context *ctx, const double *x, int64_t n, double *l1, double *l2, double *linf) {
  if (!ctx || n < 0) return GMG_ERR_INVALID;
  const int g = grid_for(n);
  hipLaunchKernelGGL(norms_partial_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, x, n, ctx->part_a.get());
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double *)ctx->part_a.get(), g, 4, 4u,
                     ctx->scal_dev.get());
  if (ctx->comm.n_ranks > 1) {
    if (allreduce_sum(ctx->comm, ctx->scal_dev.get(), 2, ctx->stream)) return fail(ctx, GMG_ERR_COMM, "all-reduce failed");
    if (allreduce_max(ctx->comm, ctx->scal_dev.get() + 2, 1, ctx->stream)) return fail(ctx, GMG_ERR_COMM, "all-reduce failed");
    if (allreduce_sum(ctx->comm, ctx->scal_dev.get() + 3, 1, ctx->stream)) return fail(ctx, GMG_ERR_COMM, "all-reduce failed");
  }
  CHK(launch_status(ctx));
  CHK(fetch_scalars(ctx, 4));
  if (l1) *l1 = ctx->scal_host.get()[0];
  if (l2) *l2 = std::sqrt(ctx->scal_host.get()[1]);
  if (linf) *linf = ctx->scal_host.get()[2];
  return GMG_OK;
}
int gmg_vec_all_zero(gmg_context *ctx, const double *x, int64_t n, int *out) {
  if (!ctx || !out) return GMG_ERR_INVALID;
  double a, b, c;
  CHK(gmg_vec_norms(ctx, x, n, &a, &b, &c));
  *out = (ctx->scal_host.get()[3] == 0.0) ? 1 : 0;
  return GMG_OK;
}

// ---- concepts ----

int gmg_spmv(gmg_context *ctx, int which, double *dst, const double *src) {
  if (!ctx) return GMG_ERR_INVALID;
  DevCSR *m = which_matrix(ctx, which);
  if (!m || !m->valid) return fail(ctx, GMG_ERR_INVALID, "gmg_spmv: operator not set");
  if (m->halo.active) {
    // the caller's src holds owned entries only: stage it in a buffer with a ghost tail
    double *tmp = (which == GMG_SYSTEM) ? ctx->S_tmp.get() : ctx->lv[(size_t)which].w3.get();
    HIPC(hipMemcpyAsync(tmp, src, sizeof(double) * (size_t)m->n_rows, hipMemcpyDeviceToDevice, ctx->stream));
    CHK(import_ghosts(ctx, *m, tmp));
    return spmv(ctx, *m, kStore, tmp, dst);
  }
  return spmv(ctx, *m, kStore, src, dst);
}

int gmg_precondition(gmg_context *ctx, double *dst, const double *src) {
  if (!ctx) return GMG_ERR_INVALID;
  return vcycle(ctx, dst, src);
}

int gmg_precondition_jacobi(gmg_context *ctx, double omega, double *dst, const double *src) {
  if (!ctx || !ctx->S.valid) return GMG_ERR_INVALID;
  hipLaunchKernelGGL(vec_scale_mul_kernel, dim3(grid_for(ctx->S.n_rows)), dim3(kThreads), 0, ctx->stream, dst, omega, src,
                     (const double *)ctx->S_invd.get(), ctx->S.n_rows);
  RETURN_LAUNCHED(ctx);
}

int gmg_coarse_solve(gmg_context *ctx, double *dst, const double *src, int *iterations, double *residual) {
  if (!ctx) return GMG_ERR_INVALID;
  Level &L0 = ctx->lv[0];
  if (!L0.A.valid) return fail(ctx, GMG_ERR_INVALID, "level-0 matrix not set");
  // run on the level's own vectors (ghost tails), then hand the owned part back
  HIPC(hipMemcpyAsync(L0.def.get(), src, sizeof(double) * (size_t)L0.n, hipMemcpyDeviceToDevice, ctx->stream));
  int rc = coarse_solve(ctx, L0.sol.get(), L0.def.get(), iterations, residual);
  HIPC(hipMemcpyAsync(dst, L0.sol.get(), sizeof(double) * (size_t)L0.n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return rc;
}

int gmg_smoother_step(gmg_context *ctx, int level, double *u, const double *rhs, int from_zero) {
  if (!ctx || level < 0 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  Level &L = ctx->lv[(size_t)level];
  if (!L.A.valid) return fail(ctx, GMG_ERR_INVALID, "level matrix not set");
  HIPC(hipMemcpyAsync(L.sol.get(), u, sizeof(double) * (size_t)L.n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(L.def.get(), rhs, sizeof(double) * (size_t)L.n, hipMemcpyDeviceToDevice, ctx->stream));
  CHK(smooth_level(ctx, level, L.sol, L.def.get(), from_zero != 0, L.w1));
  HIPC(hipMemcpyAsync(u, L.sol.get(), sizeof(double) * (size_t)L.n, hipMemcpyDeviceToDevice, ctx->stream));
  return GMG_OK;
}

int gmg_prolongate(gmg_context *ctx, int level, double *dst_fine, const double *src_coarse) {
  if (!ctx || level < 0 || level >= ctx->n_levels - 1) return GMG_ERR_INVALID;
  Level &L = ctx->lv[(size_t)level];
  if (!L.has_P) return fail(ctx, GMG_ERR_INVALID, "prolongation not set");
  if (L.P.halo.active) {
    HIPC(hipMemcpyAsync(L.w3.get(), src_coarse, sizeof(double) * (size_t)L.n, hipMemcpyDeviceToDevice, ctx->stream));
    CHK(import_ghosts(ctx, L.P, L.w3.get()));
    return spmv(ctx, L.P, kStore, L.w3.get(), dst_fine);
  }
  return spmv(ctx, L.P, kStore, src_coarse, dst_fine);
}

int gmg_restrict_and_add(gmg_context *ctx, int level, double *dst_coarse, const double *src_fine) {
  if (!ctx || level < 0 || level >= ctx->n_levels - 1) return GMG_ERR_INVALID;
  Level &L = ctx->lv[(size_t)level];
  if (!L.has_P) return fail(ctx, GMG_ERR_INVALID, "prolongation not set");
  if (L.Pt.halo.active) {
    Level &F = ctx->lv[(size_t)level + 1];
    HIPC(hipMemcpyAsync(F.w3.get(), src_fine, sizeof(double) * (size_t)F.n, hipMemcpyDeviceToDevice, ctx->stream));
    CHK(import_ghosts(ctx, L.Pt, F.w3.get()));
    return spmv(ctx, L.Pt, kStore, F.w3.get(), dst_coarse, dst_coarse);
  }
  return spmv(ctx, L.Pt, kStore, src_fine, dst_coarse, dst_coarse);
}

// ---- the two steps of one outer CG iteration around the preconditioner ----
// One rank, option disable_outer_cg_fused off: g.h lives in ocg_dev between the steps, alpha and beta are formed on the
// device, and only |g|^2 (SolverControl's check) comes back to the host.  Otherwise: the calls these steps replace.

int gmg_cg_direction_step(gmg_context *ctx, double *d, const double *g, const double *h, int64_t n, int first) {
  if (!ctx || !d || !g || !h || n < 0) return GMG_ERR_INVALID;
  const int gr = grid_for(n);
  if (ctx->dist || ctx->comm.n_ranks > 1 || ctx->disable_outer_cg_fused) {
    if (first) {
      hipLaunchKernelGGL(vec_equ_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, d, -1.0, h, n);
      return dot_host(ctx, g, h, n, &ctx->ocg_gh);
    }
    double beta = ctx->ocg_gh;
    CHK(dot_host(ctx, g, h, n, &ctx->ocg_gh));
    beta = ctx->ocg_gh / beta;
    hipLaunchKernelGGL(vec_sadd_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, d, beta, -1.0, h, n);
    RETURN_LAUNCHED(ctx);
  }
  double *const s = ctx->ocg_dev.get();
  if (first) {
    hipLaunchKernelGGL(vec_equ_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, d, -1.0, h, n);
    ctx->ocg_cur = 0;
  } else {
    ctx->ocg_cur ^= 1;
  }
  hipLaunchKernelGGL(dot_partial_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, g, h, n, ctx->part_a.get());
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double *)ctx->part_a.get(), gr, 1, 0u, s + ctx->ocg_cur);
  if (!first)
    hipLaunchKernelGGL(cg_outer_direction_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, d, h, n, (const double *)(s + ctx->ocg_cur),
                       (const double *)(s + (ctx->ocg_cur ^ 1)), -1.0);
  RETURN_LAUNCHED(ctx);
}

int gmg_cg_update_step(gmg_context *ctx, double *x, double *g, const double *d, const double *h, int64_t n, double *gg) {
  if (!ctx || !x || !g || !d || !h || !gg || n < 0) return GMG_ERR_INVALID;
  const int gr = grid_for(n);
  if (ctx->dist || ctx->comm.n_ranks > 1 || ctx->disable_outer_cg_fused) {
    double alpha = 0.0;
    CHK(dot_host(ctx, d, h, n, &alpha));
    alpha = ctx->ocg_gh / alpha;
    hipLaunchKernelGGL(vec_add_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, x, alpha, d, n);
    hipLaunchKernelGGL(vec_add_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, g, alpha, h, n);
    return dot_host(ctx, g, g, n, gg);
  }
  double *const s = ctx->ocg_dev.get();
  hipLaunchKernelGGL(dot_partial_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, d, h, n, ctx->part_a.get());
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double *)ctx->part_a.get(), gr, 1, 0u, s + 2);
  hipLaunchKernelGGL(cg_outer_update_kernel, dim3(gr), dim3(kThreads), 0, ctx->stream, x, g, d, h, n, (const double *)(s + ctx->ocg_cur),
                     (const double *)(s + 2), ctx->part_a.get());
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double *)ctx->part_a.get(), gr, 1, 0u, ctx->scal_dev.get());
  CHK(launch_status(ctx));
  CHK(fetch_scalars(ctx, 1));
  *gg = ctx->scal_host.get()[0];
  return GMG_OK;
}

// SolverCG<vector_t>::solve, deal.II operation order (see oracle/gmg_oracle.c:cg_solve).
int gmg_cg_solve(gmg_context *ctx, double *x, const double *b, double rel_tol, int max_it, int precond, int *iterations,
                 double *starting_value, double *convergence_value) {
  if (!ctx || !ctx->S.valid) return GMG_ERR_INVALID;
  const int64_t n = ctx->S.n_rows;
  DevPtr<double> g_own, d_own, h_own;
  CHK(alloc_vec(ctx, g_own, ctx->S.n_cols));
  CHK(alloc_vec(ctx, d_own, ctx->S.n_cols));
  CHK(alloc_vec(ctx, h_own, ctx->S.n_cols));
  double *const g = g_own.get(), *const d = d_own.get(), *const h = h_own.get();
  auto apply_precond = [&](double *dst, const double *src) -> int {
    if (precond == GMG_PRECOND_GMG) return vcycle(ctx, dst, src);
    if (precond == GMG_PRECOND_JACOBI) return gmg_precondition_jacobi(ctx, 0.6, dst, src);
    return GMG_ERR_INVALID;
  };
  int rc = GMG_OK;
  double bb = 0.0, res = 0.0, gh = 0.0, alpha = 0.0, beta = 0.0, tmp = 0.0;
  int it = 0, zero = 0;
  do {
    if ((rc = dot_host(ctx, b, b, n, &bb))) break;
    const double tol = rel_tol * std::sqrt(bb);
    if ((rc = gmg_vec_all_zero(ctx, x, n, &zero))) break;
    if (!zero) {
      if ((rc = gmg_spmv(ctx, GMG_SYSTEM, g, x))) break;
      gmg_vec_add(ctx, g, -1.0, b, n);
    } else {
      gmg_vec_equ(ctx, g, -1.0, b, n);
    }
    if ((rc = dot_host(ctx, g, g, n, &tmp))) break;
    res = std::sqrt(tmp);
    if (starting_value) *starting_value = res;
    if (res <= tol) break;
    if (precond != GMG_PRECOND_IDENTITY) {
      if ((rc = apply_precond(h, g))) break;
      if ((rc = gmg_cg_direction_step(ctx, d, g, h, n, 1))) break;  // d = -h, g.h
    } else {
      gmg_vec_equ(ctx, d, -1.0, g, n);
      gh = res * res;
    }
    for (;;) {
      ++it;
      if ((rc = gmg_spmv(ctx, GMG_SYSTEM, h, d))) break;
      if (precond != GMG_PRECOND_IDENTITY) {
        if ((rc = gmg_cg_update_step(ctx, x, g, d, h, n, &tmp))) break;  // alpha = g.h / d.h; x += alpha d; g += alpha h; |g|^2
      } else {  // (g.h is res * res on the host)
        if ((rc = dot_host(ctx, d, h, n, &alpha))) break;
        alpha = gh / alpha;
        gmg_vec_add(ctx, x, alpha, d, n);
        gmg_vec_add(ctx, g, alpha, h, n);
        if ((rc = dot_host(ctx, g, g, n, &tmp))) break;
      }
      res = std::sqrt(tmp);
      if (res <= tol) break;
      if (it >= max_it || res != res) { rc = GMG_ERR_OUTER_NOCONV; ctx->err = "outer CG did not converge within max_it"; break; }
      if (precond != GMG_PRECOND_IDENTITY) {
        if ((rc = apply_precond(h, g))) break;
        if ((rc = gmg_cg_direction_step(ctx, d, g, h, n, 0))) break;  // beta = g.h / (the previous g.h); d = beta d - h
      } else {
        beta = gh;
        gh = res * res;
        beta = gh / beta;
        gmg_vec_sadd(ctx, d, beta, -1.0, g, n);
      }
    }
  } while (0);
  if (iterations) *iterations = it;
  if (convergence_value) *convergence_value = res;
  (void)hipStreamSynchronize(ctx->stream);  // (the vectors are freed on return)
  return rc;
}

// ---- N1: charge density ----

int gmg_charge_density(gmg_context *ctx, int64_t n_cells, const double *cell_lo, const double *cell_h,
                       const double *root_lo, double root_h, int64_t n_atoms, const double *atom_xyz,
                       const double *atom_q, double r_c, double cutoff, int use_lists, int nq,
                       const double *quadrature_points, double *dens) {
  if (!ctx || n_cells < 0 || n_atoms < 0 || nq < 1 || n_cells >= ((int64_t)1 << 31)) return GMG_ERR_INVALID;
  if (n_cells == 0) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  // bins of edge `cutoff` over the atoms' bounding box (host; 64 k atoms: microseconds)
  DensityArgs a{};
  const double bs = std::max(cutoff, 1e-12);
  gmg_forces::Bins B;
  if (!gmg_forces::bin_atoms(n_atoms, atom_xyz, bs, (int64_t)1 << 28, B)) return fail(ctx, GMG_ERR_UNSUPPORTED, "atom bin grid too large");
  const double *lo = B.lo;
  const int *bn = B.n;
  const std::vector<int32_t> &bptr = B.ptr, &bitems = B.items;
  DevPtr<double> d_lo, d_h, d_root, d_xyz, d_q, d_qp, d_dens;
  DevPtr<int32_t> d_bptr, d_bitems;
  // (allocations of at least 8 bytes: two int32_t)
  if (upload(d_lo, cell_lo, 3 * (size_t)n_cells, ctx->stream) != hipSuccess || upload(d_h, cell_h, (size_t)n_cells, ctx->stream) != hipSuccess ||
      upload(d_root, root_lo, 3 * (size_t)n_cells, ctx->stream) != hipSuccess || upload(d_xyz, atom_xyz, 3 * (size_t)n_atoms, ctx->stream) != hipSuccess ||
      upload(d_q, atom_q, (size_t)n_atoms, ctx->stream) != hipSuccess || upload(d_qp, quadrature_points, 3 * (size_t)nq, ctx->stream) != hipSuccess ||
      upload(d_bptr, bptr, ctx->stream, 2) != hipSuccess || upload(d_bitems, bitems, ctx->stream, 2) != hipSuccess)
    return fail(ctx, GMG_ERR_HIP, "gmg_charge_density: upload failed");
  if (d_dens.alloc((size_t)n_cells * (size_t)nq) != hipSuccess) return fail(ctx, GMG_ERR_HIP, "gmg_charge_density: out of memory");
  ctx->dens_dev.reset(); ctx->dens_cells = 0; ctx->dens_nq = 0;
  a.cell_lo = d_lo.get(); a.cell_h = d_h.get(); a.root_lo = d_root.get(); a.root_h = root_h;
  a.atom_xyz = d_xyz.get(); a.atom_q = d_q.get(); a.n_atoms = (int)n_atoms;
  a.bin_lo0 = lo[0]; a.bin_lo1 = lo[1]; a.bin_lo2 = lo[2]; a.bin_size = bs;
  a.bin_n0 = bn[0]; a.bin_n1 = bn[1]; a.bin_n2 = bn[2];
  a.bin_ptr = d_bptr.get(); a.bin_items = d_bitems.get();
  a.cutoff = cutoff; a.r_c = r_c; a.use_lists = use_lists;
  a.qp = d_qp.get(); a.nq = nq; a.n_cells = (int)n_cells; a.dens = d_dens.get();
  hipLaunchKernelGGL(charge_density_kernel, dim3((unsigned)((n_cells + 3) / 4)), dim3(kThreads), 0, ctx->stream, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && dens) e = hipMemcpyAsync(dens, d_dens.get(), sizeof(double) * (size_t)n_cells * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && !dens) {  // the densities stay in HBM for gmg_rhs_assemble (gmg_get_charge_density copies them out on demand)
    ctx->dens_dev = std::move(d_dens); ctx->dens_cells = n_cells; ctx->dens_nq = nq;
  }
  if (e != hipSuccess) { ctx->err = std::string("gmg_charge_density: ") + hipGetErrorString(e); return GMG_ERR_HIP; }
  return GMG_OK;
}

int gmg_get_charge_density(gmg_context *ctx, int64_t n_cells, int nq, double *dens) {
  if (!ctx || !dens) return GMG_ERR_INVALID;
  if (!ctx->dens_dev.get() || ctx->dens_cells != n_cells || ctx->dens_nq != nq) return fail(ctx, GMG_ERR_INVALID, "gmg_get_charge_density: no densities of this shape on the device");
  HIPC(hipMemcpyAsync(dens, ctx->dens_dev.get(), sizeof(double) * (size_t)n_cells * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

// ---- charge densities from the resident mesh tables (gmg_density.hpp)

// what both entries check first: no communicator, 3D tables, a root lattice
static int density_resident_tables(gmg_context *ctx, const char *who, double h0) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  if (!ctx->mesh.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  if (ctx->mesh.dim != 3) return bad(GMG_ERR_UNSUPPORTED, "the mesh tables are not 3D");
  if (!(h0 > 0.0)) return bad(GMG_ERR_INVALID, "h0 must be positive");
  return GMG_OK;
}

int gmg_charge_density_resident(gmg_context *ctx, double origin, double h0, int64_t n_atoms, const double *atom_xyz, const double *atom_q, double r_c,
                                double cutoff, int use_lists, int nq, const double *quadrature_points, double *dens, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  const char *who = "gmg_charge_density_resident";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  ctx->dens_dev.reset(); ctx->dens_cells = 0; ctx->dens_nq = 0;  // after any failure the context holds no densities
  if (build_ms) *build_ms = 0.0;
  CHK(density_resident_tables(ctx, who, h0));
  if (nq < 1) return bad(GMG_ERR_INVALID, "nq must be at least 1");
  if (!(r_c > 0.0)) return bad(GMG_ERR_INVALID, "r_c must be positive");
  if (!(cutoff >= 0.0)) return bad(GMG_ERR_INVALID, "cutoff must not be negative");
  if (n_atoms < 0 || n_atoms >= ((int64_t)1 << 31)) return bad(GMG_ERR_INVALID, "n_atoms outside [0, 2^31)");
  if (!quadrature_points || (n_atoms > 0 && (!atom_xyz || !atom_q))) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  const MeshTables &m = ctx->mesh;
  const int64_t n_cells = m.n_cells;
  gmg_forces::Bins B;  // (host; 64 k atoms: microseconds)
  const double bs = std::max(cutoff, 1e-12);
  if (use_lists && !gmg_forces::bin_atoms(n_atoms, atom_xyz, bs, (int64_t)1 << 28, B)) return bad(GMG_ERR_UNSUPPORTED, "atom bin grid too large");
  if (n_cells == 0) return GMG_OK;
  DevPtr<double> d_xyz, d_q, d_qp, d_dens;
  DevPtr<int32_t> d_bptr, d_bitems;
  Event e0, e1;
  HIPC(upload(d_xyz, atom_xyz, 3 * (size_t)n_atoms, ctx->stream));
  HIPC(upload(d_q, atom_q, (size_t)n_atoms, ctx->stream));
  HIPC(upload(d_qp, quadrature_points, 3 * (size_t)nq, ctx->stream));
  HIPC(upload(d_bptr, B.ptr, ctx->stream, 2));
  HIPC(upload(d_bitems, B.items, ctx->stream, 2));
  HIPC(d_dens.alloc((size_t)n_cells * (size_t)nq));
  HIPC(e0.create());
  HIPC(e1.create());
  DensityResArgs a{};
  a.cell_dofs = m.cell_dofs.get(); a.cell_level = m.cell_level.get(); a.vertex_of_dof = m.vertex_of_dof.get(); a.n_cells = n_cells;
  a.origin = origin; a.h0 = h0;
  a.atom_xyz = d_xyz.get(); a.atom_q = d_q.get(); a.n_atoms = (int)n_atoms;
  a.bin_lo0 = B.lo[0]; a.bin_lo1 = B.lo[1]; a.bin_lo2 = B.lo[2]; a.bin_size = bs;
  a.bin_n0 = B.n[0]; a.bin_n1 = B.n[1]; a.bin_n2 = B.n[2];
  a.bin_ptr = d_bptr.get(); a.bin_items = d_bitems.get();
  a.cutoff = cutoff; a.r_c = r_c; a.use_lists = use_lists ? 1 : 0;
  a.qp = d_qp.get(); a.nq = nq; a.dens = d_dens.get();
  // a cell's lane group: the smallest power of two >= min(nq, 64); its LDS segment: 4 g - 1 atoms, at most 127 (32 KB per
  // workgroup: measured faster than 8 g - 1, which halves the workgroups a CU holds), or option
  // density_segment made odd, no shorter than the group and within 64 KB per workgroup
  while ((1 << a.lg_g) < std::min(nq, 64)) ++a.lg_g;
  const int g = 1 << a.lg_g, groups = kDrThreads / g;
  a.cap = std::max(std::min(4 * g - 1, 127), g | 1);
  if (ctx->density_segment > 0) a.cap = std::min(std::max(ctx->density_segment | 1, g | 1), ((int)(65536 / (32 * groups)) - 1) | 1);
  if (a.cap < g) a.cap = g | 1;
  const size_t lds = (size_t)groups * (size_t)a.cap * 4 * sizeof(double);
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  hipLaunchKernelGGL(density_resident_kernel, asm_blocks(ctx, n_cells, groups), dim3(kDrThreads), lds, ctx->stream, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(e1.get(), ctx->stream);
  if (e == hipSuccess && dens) e = hipMemcpyAsync(dens, d_dens.get(), sizeof(double) * (size_t)n_cells * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // (the uploads above live until the stream has run the kernel)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) { ctx->err = std::string(who) + ": " + hipGetErrorString(e); return GMG_ERR_HIP; }
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  if (!dens) {  // the densities stay in HBM, as gmg_charge_density leaves them
    ctx->dens_dev = std::move(d_dens); ctx->dens_cells = n_cells; ctx->dens_nq = nq;
  }
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] charge densities from resident tables: %lld cells x %d points, %lld atoms, groups of %d lanes, segments of %d atoms, %.3f ms\n",
                 (long long)n_cells, nq, (long long)n_atoms, g, a.cap, ms);
  return GMG_OK;
}

int gmg_get_resident_cell_geometry(gmg_context *ctx, double origin, double h0, double *cell_lo, double *cell_h, double *root_lo) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  CHK(density_resident_tables(ctx, "gmg_get_resident_cell_geometry", h0));
  const MeshTables &m = ctx->mesh;
  const int64_t n = m.n_cells;
  if (n == 0 || (!cell_lo && !cell_h && !root_lo)) return GMG_OK;
  DevPtr<double> d_lo, d_h, d_root;
  if (cell_lo) HIPC(d_lo.alloc(3 * (size_t)n));
  if (cell_h) HIPC(d_h.alloc((size_t)n));
  if (root_lo) HIPC(d_root.alloc(3 * (size_t)n));
  DensityResArgs a{};
  a.cell_dofs = m.cell_dofs.get(); a.cell_level = m.cell_level.get(); a.vertex_of_dof = m.vertex_of_dof.get(); a.n_cells = n;
  a.origin = origin; a.h0 = h0;
  a.cell_lo = d_lo.get(); a.cell_h = d_h.get(); a.root_lo = d_root.get();
  hipLaunchKernelGGL(dr_geometry_kernel, asm_blocks(ctx, n, kDrThreads), dim3(kDrThreads), 0, ctx->stream, a);
  HIPC(hipGetLastError());
  HIPC(mesh_fetch(ctx, cell_lo, d_lo, 3 * n));
  HIPC(mesh_fetch(ctx, cell_h, d_h, n));
  HIPC(mesh_fetch(ctx, root_lo, d_root, 3 * n));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

// ---- atom forces (gmg_forces.hpp) ----

}  // extern "C"

namespace {
bool atoms_ok(int64_t n_atoms, const double *xyz, const double *q) {
  return n_atoms >= 0 && n_atoms < ((int64_t)1 << 31) && (n_atoms == 0 || (xyz && q));
}
std::vector<double> pack_xq(int64_t n, const double *xyz, const double *q) {
  std::vector<double> xq((size_t)std::max<int64_t>(n, 1) * 4);
  for (int64_t i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) xq[(size_t)(4 * i + d)] = xyz[3 * i + d];
    xq[(size_t)(4 * i + 3)] = q[i];
  }
  return xq;
}
// per-atom (F, e) of a pair law into out_dev [n][4]: all pairs (rcut = inf, N-body tiles) or the pairs closer than rcut
// through the bins of gmg_forces::force_bins
template <class Law>
int launch_pairs(gmg_context *ctx, const Law &law, double rcut, int64_t n, const double *xyz, const double *xq_host,
                 const double *xq_dev, double *out_dev) {
  const int bs = ctx->force_block;
  const size_t lds = sizeof(double) * 4 * (size_t)bs;
  if (!(rcut < INFINITY)) {
    hipLaunchKernelGGL(gmg_forces::pair_all_kernel<Law>, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), lds, ctx->stream, law, rcut,
                       xq_dev, (int)n, out_dev);
    return GMG_OK;
  }
  gmg_forces::Bins B;
  gmg_forces::force_bins(n, xyz, rcut, B);
  std::vector<double> sorted((size_t)n * 4);
  for (int64_t k = 0; k < n; ++k)
    for (int c = 0; c < 4; ++c) sorted[(size_t)(4 * k + c)] = xq_host[4 * (size_t)B.items[(size_t)k] + c];
  std::vector<int32_t> ubin, ustart;
  for (size_t b = 0; b + 1 < B.ptr.size(); ++b)
    for (int32_t s = 0; s < B.ptr[b + 1] - B.ptr[b]; s += bs) { ubin.push_back((int32_t)b); ustart.push_back(s); }
  DevPtr<double> d_sorted;
  DevPtr<int32_t> d_items, d_ptr, d_ubin, d_ustart;
  if (d_sorted.alloc(std::max<size_t>(sorted.size(), 1)) != hipSuccess || d_items.alloc(std::max<size_t>(B.items.size(), 2)) != hipSuccess ||
      d_ptr.alloc(std::max<size_t>(B.ptr.size(), 2)) != hipSuccess || d_ubin.alloc(std::max<size_t>(ubin.size(), 2)) != hipSuccess ||
      d_ustart.alloc(std::max<size_t>(ustart.size(), 2)) != hipSuccess)
    return fail(ctx, GMG_ERR_HIP, "atom forces: out of memory");  // (sizes: at least 8 bytes each)
  HIPC(hipMemcpyAsync(d_sorted.get(), sorted.data(), sizeof(double) * sorted.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_items.get(), B.items.data(), sizeof(int32_t) * B.items.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_ptr.get(), B.ptr.data(), sizeof(int32_t) * B.ptr.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_ubin.get(), ubin.data(), sizeof(int32_t) * ubin.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_ustart.get(), ustart.data(), sizeof(int32_t) * ustart.size(), hipMemcpyHostToDevice, ctx->stream));
  gmg_forces::BinnedArgs a{d_sorted.get(), d_items.get(), d_ptr.get(), d_ubin.get(), d_ustart.get(), {B.n[0], B.n[1], B.n[2]}, out_dev};
  hipLaunchKernelGGL(gmg_forces::pair_binned_kernel<Law>, dim3((unsigned)ubin.size()), dim3(bs), lds, ctx->stream, law, rcut, a);
  HIPC(hipStreamSynchronize(ctx->stream));  // (the host arrays above are the sources of the copies, the buffers the kernel's inputs)
  return GMG_OK;
}
}  // namespace

extern "C" {

int gmg_set_point_locator(gmg_context *ctx, const int32_t n0[3], const double origin[3], double h0, int64_t n_nodes,
                          const int32_t *node, int64_t n_active, const int32_t *active_dofs) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  free_locator(ctx);
  if (!n0 || !origin || !node || !active_dofs || !(h0 > 0.0) || n_active < 1 || n_nodes < 1 || n_nodes >= ((int64_t)1 << 31) ||
      n_active >= ((int64_t)1 << 28))
    return fail(ctx, GMG_ERR_INVALID, "gmg_set_point_locator: bad sizes");
  int64_t n_roots = 1;
  for (int d = 0; d < 3; ++d) {
    if (n0[d] < 1) return fail(ctx, GMG_ERR_INVALID, "gmg_set_point_locator: bad root lattice");
    n_roots *= n0[d];
  }
  if (n_roots > n_nodes) return fail(ctx, GMG_ERR_INVALID, "gmg_set_point_locator: fewer nodes than roots");
  // every walk ends: children lie after their parent, inside the array, and at most 20 levels below a root
  std::vector<int8_t> depth((size_t)n_nodes, 0);
  for (int64_t k = 0; k < n_nodes; ++k) {
    const int32_t v = node[k];
    if (v >= 0) {
      if (v <= k || (int64_t)v + 7 >= n_nodes || depth[(size_t)k] >= 20) return fail(ctx, GMG_ERR_INVALID, "gmg_set_point_locator: node index out of range");
      for (int a = 0; a < 8; ++a) depth[(size_t)v + a] = (int8_t)std::max<int>(depth[(size_t)v + a], depth[(size_t)k] + 1);
    } else if (-(int64_t)v - 1 >= n_active) {
      return fail(ctx, GMG_ERR_INVALID, "gmg_set_point_locator: active cell index out of range");
    }
  }
  int64_t max_dof = -1;
  for (int64_t i = 0; i < 8 * n_active; ++i) {
    if (active_dofs[i] < 0) return fail(ctx, GMG_ERR_INVALID, "gmg_set_point_locator: negative DoF");
    max_dof = std::max<int64_t>(max_dof, active_dofs[i]);
  }
  DevPtr<int32_t> d_node, d_dofs;
  if (d_node.alloc((size_t)n_nodes) != hipSuccess || d_dofs.alloc(8 * (size_t)n_active) != hipSuccess)
    return fail(ctx, GMG_ERR_HIP, "gmg_set_point_locator: out of memory");
  HIPC(hipMemcpyAsync(d_node.get(), node, sizeof(int32_t) * (size_t)n_nodes, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_dofs.get(), active_dofs, sizeof(int32_t) * 8 * (size_t)n_active, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->loc = gmg_forces::Locator{{n0[0], n0[1], n0[2]}, {origin[0], origin[1], origin[2]}, h0, d_node.get(), d_dofs.get()};
  ctx->loc_node = std::move(d_node);  // (the context's only once the locator is complete)
  ctx->loc_dofs = std::move(d_dofs);
  ctx->loc_max_dof = max_dof;
  return GMG_OK;
}

// The two halves of gmg_atom_forces' front.  atom_forces_check_args: the arguments that are not the locator.
// atom_forces_device: the kernels on a locator whose arrays lie on the device (located == false: a mesh without cells, phi and
// the field are 0).
static int atom_forces_check_args(gmg_context *ctx, const char *who, int64_t n_atoms, const double *atom_xyz, const double *atom_q, double r_c, double cutoff) {
  if (!atoms_ok(n_atoms, atom_xyz, atom_q) || !(r_c > 0.0) || !(cutoff >= 0.0)) return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": bad arguments").c_str());
  return GMG_OK;
}

static int atom_forces_device(gmg_context *ctx, const char *who, const gmg_forces::Locator &L, bool located, int64_t n_atoms, const double *atom_xyz,
                              const double *atom_q, const double *u, double r_c, double cutoff, double *phi, double *field, double *force, double *force_short,
                              double *e_short) {
  (void)hipSetDevice(ctx->device);
  const int64_t n = n_atoms;
  const bool want_field = phi || field || force, want_pairs = force || force_short || e_short;
  const std::vector<double> xq = pack_xq(n, atom_xyz, atom_q);
  DevPtr<double> xq_own, phi_own, E_own, pair_own;
  if (xq_own.alloc((size_t)n * 4) != hipSuccess || phi_own.alloc((size_t)n) != hipSuccess || E_own.alloc((size_t)n * 3) != hipSuccess ||
      pair_own.alloc((size_t)n * 4) != hipSuccess)
    return fail(ctx, GMG_ERR_HIP, (std::string(who) + ": out of memory").c_str());
  double *const d_xq = xq_own.get(), *const d_phi = phi_own.get(), *const d_E = E_own.get(), *const d_pair = pair_own.get();
  HIPC(hipMemcpyAsync(d_xq, xq.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  const int bs = ctx->force_block;
  if (want_field && located)
    hipLaunchKernelGGL(gmg_forces::atom_field_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, ctx->stream, L, u, d_xq, (int)n,
                       d_phi, d_E);
  if (want_field && !located) {
    HIPC(hipMemsetAsync(d_phi, 0, sizeof(double) * (size_t)n, ctx->stream));
    HIPC(hipMemsetAsync(d_E, 0, sizeof(double) * 3 * (size_t)n, ctx->stream));
  }
  if (want_pairs) CHK(launch_pairs(ctx, gmg_forces::ShortLaw::make(r_c), cutoff > 0.0 ? cutoff * r_c : INFINITY, n, atom_xyz,
                                   xq.data(), d_xq, d_pair));
  HIPC(hipGetLastError());
  std::vector<double> E((size_t)n * 3), pair((size_t)n * 4);
  if (phi) HIPC(hipMemcpyAsync(phi, d_phi, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (want_field) HIPC(hipMemcpyAsync(E.data(), d_E, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  if (want_pairs) HIPC(hipMemcpyAsync(pair.data(), d_pair, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) {
      if (field) field[3 * i + d] = E[(size_t)(3 * i + d)];
      if (force_short) force_short[3 * i + d] = pair[(size_t)(4 * i + d)];
      if (force) force[3 * i + d] = atom_q[i] * E[(size_t)(3 * i + d)] + pair[(size_t)(4 * i + d)];
    }
    if (e_short) e_short[i] = pair[(size_t)(4 * i + 3)];
  }
  return GMG_OK;
}

int gmg_atom_forces(gmg_context *ctx, int64_t n_atoms, const double *atom_xyz, const double *atom_q, const double *u, int64_t n_u,
                    double r_c, double cutoff, double *phi, double *field, double *force, double *force_short, double *e_short) {
  if (!ctx) return GMG_ERR_INVALID;
  CHK(atom_forces_check_args(ctx, "gmg_atom_forces", n_atoms, atom_xyz, atom_q, r_c, cutoff));
  if (ctx->loc_max_dof < 0) return fail(ctx, GMG_ERR_INVALID, "gmg_atom_forces: call gmg_set_point_locator first");
  if (!u || n_u <= ctx->loc_max_dof) return fail(ctx, GMG_ERR_INVALID, "gmg_atom_forces: u is shorter than the locator's DoFs");
  if (n_atoms == 0) return GMG_OK;
  return atom_forces_device(ctx, "gmg_atom_forces", ctx->loc, true, n_atoms, atom_xyz, atom_q, u, r_c, cutoff, phi, field, force, force_short, e_short);
}

// ---- energy and forces at the atoms from the resident mesh tables

// what the entries on the resident locator check first: no communicator, tables, 3D
static int locator_resident_tables(gmg_context *ctx, const char *who) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  if (!ctx->mesh.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  if (ctx->mesh.dim != 3) return bad(GMG_ERR_UNSUPPORTED, "the mesh tables are not 3D");
  return GMG_OK;
}

// the resident locator as locate() takes it, after the checks both consumers share
static int resident_locator(gmg_context *ctx, const char *who, double origin, double h0, const double *u, int64_t n_u, gmg_forces::Locator &L) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  CHK(locator_resident_tables(ctx, who));
  const MeshTables &m = ctx->mesh;
  if (!m.locator.valid) return bad(GMG_ERR_INVALID, "the context holds no point locator (gmg_build_point_locator_resident)");
  if (!(h0 > 0.0)) return bad(GMG_ERR_INVALID, "h0 must be positive");
  if (n_u != m.n_dofs || (n_u > 0 && !u)) return bad(GMG_ERR_INVALID, "u does not have the mesh tables' n_dofs entries");
  L = gmg_forces::Locator{{m.locator.n0[0], m.locator.n0[1], m.locator.n0[2]}, {origin, origin, origin}, h0, m.locator.node.get(), m.cell_dofs.get()};
  return GMG_OK;
}

int gmg_build_point_locator_resident(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                                     const int32_t *cell_first_child, int64_t *n_nodes, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  const char *who = "gmg_build_point_locator_resident";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  ctx->mesh.locator = MeshTables::PointLocator();  // after any failure the context holds no resident locator
  if (build_ms) *build_ms = 0.0;
  CHK(locator_resident_tables(ctx, who));
  std::vector<uint8_t> level_of;
  CHK(check_forest(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of));
  if (dim != ctx->mesh.dim) return bad(GMG_ERR_INVALID, "dim differs from the mesh tables'");
  const int64_t n_all = level_ptr[n_levels];
  int64_t na = 0;
  for (int64_t c = 0; c < n_all; ++c) na += cell_first_child[c] < 0;
  if (na != ctx->mesh.n_cells) return bad(GMG_ERR_INVALID, "the forest's active cells are not as many as the mesh tables' n_cells");
  if (n_all > 0) {  // locate() indexes the roots by coordinate: level 0 must be the full lattice, x fastest
    if (level_ptr[1] != (int64_t)n0[0] * n0[1] * n0[2]) return bad(GMG_ERR_INVALID, "level 0 is not the full lattice");
    for (int64_t c = 0; c < level_ptr[1]; ++c)
      if (cell_coord[3 * c] != c % n0[0] || cell_coord[3 * c + 1] != (c / n0[0]) % n0[1] || cell_coord[3 * c + 2] != c / ((int64_t)n0[0] * n0[1]))
        return bad(GMG_ERR_INVALID, "level 0 is not in lexicographic cell order");
  }
  MeshTables::PointLocator loc;
  loc.n_nodes = n_all;
  for (int d = 0; d < 3; ++d) loc.n0[d] = n0[d];
  DevPtr<int32_t> d_fc, d_apos;  // the scratch lives until the stream has run the kernels
  Event e0, e1;
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  HIPC(upload(d_fc, cell_first_child, (size_t)n_all, ctx->stream));
  HIPC(d_apos.alloc((size_t)n_all + 1));
  HIPC(loc.node.alloc((size_t)std::max<int64_t>(n_all, 1)));
  gmg_forces::LocLevels lv{};
  lv.n_levels = n_levels;
  for (int l = 0; l < 14; ++l) lv.ptr[l] = level_ptr[std::min(l, n_levels)];
  const dim3 blk(kMtThreads);
  if (n_all) hipLaunchKernelGGL(mt_active_flag_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const int32_t *)d_fc.get(), n_all, d_apos.get());
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_apos.get(), n_all);
  if (n_all)
    hipLaunchKernelGGL(gmg_forces::loc_node_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const int32_t *)d_fc.get(), (const int32_t *)d_apos.get(), lv,
                       n_all, loc.node.get());
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  CHK(launch_status(ctx));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  loc.valid = true;
  ctx->mesh.locator = std::move(loc);  // (nothing after this can fail)
  if (n_nodes) *n_nodes = n_all;
  if (build_ms) *build_ms = ms;
  return GMG_OK;
}

int gmg_get_point_locator(gmg_context *ctx, int64_t *n_nodes, int32_t *node) {
  if (!ctx) return GMG_ERR_INVALID;
  CHK(locator_resident_tables(ctx, "gmg_get_point_locator"));
  const MeshTables &m = ctx->mesh;
  if (!m.locator.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_point_locator: the context holds no point locator (gmg_build_point_locator_resident)");
  (void)hipSetDevice(ctx->device);
  if (n_nodes) *n_nodes = m.locator.n_nodes;
  HIPC(mesh_fetch(ctx, node, m.locator.node, m.locator.n_nodes));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

int gmg_atom_forces_resident(gmg_context *ctx, double origin, double h0, int64_t n_atoms, const double *atom_xyz, const double *atom_q, const double *u,
                             int64_t n_u, double r_c, double cutoff, double *phi, double *field, double *force, double *force_short, double *e_short) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_atom_forces_resident";
  gmg_forces::Locator L{};
  CHK(resident_locator(ctx, who, origin, h0, u, n_u, L));
  CHK(atom_forces_check_args(ctx, who, n_atoms, atom_xyz, atom_q, r_c, cutoff));
  if (n_atoms == 0) return GMG_OK;
  return atom_forces_device(ctx, who, L, ctx->mesh.n_cells > 0, n_atoms, atom_xyz, atom_q, u, r_c, cutoff, phi, field, force, force_short, e_short);
}

int gmg_electrostatic_energy_resident(gmg_context *ctx, double origin, double h0, int64_t n_atoms, const double *atom_xyz, const double *atom_q, const double *u,
                                      int64_t n_u, double r_c, double cutoff, double out[3], double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_electrostatic_energy_resident";
  if (build_ms) *build_ms = 0.0;
  gmg_forces::Locator L{};
  CHK(resident_locator(ctx, who, origin, h0, u, n_u, L));
  CHK(atom_forces_check_args(ctx, who, n_atoms, atom_xyz, atom_q, r_c, cutoff));
  if (!out) return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": out is NULL").c_str());
  out[0] = out[1] = out[2] = 0.0;
  if (n_atoms == 0) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  const int64_t n = n_atoms;
  const std::vector<double> xq = pack_xq(n, atom_xyz, atom_q);
  DevPtr<double> d_xq, d_pair, d_fe, d_self, d_out;
  Event e0, e1;
  if (d_xq.alloc((size_t)n * 4) != hipSuccess || d_pair.alloc((size_t)n * 4) != hipSuccess || d_fe.alloc((size_t)n) != hipSuccess ||
      d_self.alloc((size_t)n) != hipSuccess || d_out.alloc(3) != hipSuccess)
    return fail(ctx, GMG_ERR_HIP, (std::string(who) + ": out of memory").c_str());
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipMemcpyAsync(d_xq.get(), xq.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  const int bs = ctx->force_block;
  hipLaunchKernelGGL(gmg_forces::atom_energy_terms_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, ctx->stream, L, ctx->mesh.n_cells > 0 ? 1 : 0, u,
                     (const double *)d_xq.get(), (int)n, std::sqrt(M_PI) * r_c, d_fe.get(), d_self.get());
  CHK(launch_pairs(ctx, gmg_forces::ShortLaw::make(r_c), cutoff > 0.0 ? cutoff * r_c : INFINITY, n, atom_xyz, xq.data(), d_xq.get(), d_pair.get()));
  gmg_forces::EnergySumArgs a{{d_pair.get() + 3, d_fe.get(), d_self.get()}, {4, 1, 1}, (int)n, d_out.get()};
  hipLaunchKernelGGL(gmg_forces::energy_sum_kernel, dim3(3), dim3(256), 0, ctx->stream, a);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  HIPC(hipMemcpyAsync(out, d_out.get(), sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  return GMG_OK;
}

int gmg_direct_coulomb(gmg_context *ctx, int64_t n_atoms, const double *atom_xyz, const double *atom_q, double *force, double *energy) {
  if (!ctx) return GMG_ERR_INVALID;
  if (!atoms_ok(n_atoms, atom_xyz, atom_q)) return fail(ctx, GMG_ERR_INVALID, "gmg_direct_coulomb: bad arguments");
  if (n_atoms == 0 || (!force && !energy)) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  const int64_t n = n_atoms;
  const std::vector<double> xq = pack_xq(n, atom_xyz, atom_q);
  DevPtr<double> xq_own, pair_own;
  if (xq_own.alloc((size_t)n * 4) != hipSuccess || pair_own.alloc((size_t)n * 4) != hipSuccess) return fail(ctx, GMG_ERR_HIP, "gmg_direct_coulomb: out of memory");
  double *const d_xq = xq_own.get(), *const d_pair = pair_own.get();
  HIPC(hipMemcpyAsync(d_xq, xq.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  CHK(launch_pairs(ctx, gmg_forces::DirectLaw{}, INFINITY, n, atom_xyz, xq.data(), d_xq, d_pair));
  HIPC(hipGetLastError());
  std::vector<double> pair((size_t)n * 4);
  HIPC(hipMemcpyAsync(pair.data(), d_pair, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < n; ++i) {
    if (force)
      for (int d = 0; d < 3; ++d) force[3 * i + d] = pair[(size_t)(4 * i + d)];
    if (energy) energy[i] = pair[(size_t)(4 * i + 3)];
  }
  return GMG_OK;
}

// ---- exact free-space potential of the Gaussian charges (gmg_exact.hpp) ----
// Both calls cut their points into launches of at most 2^exact_chunk_log2 point-atom evaluations (at least one point or cell
// per launch): a launch stays short whatever the sizes.  Every value is one lane's sequential sum, so the cuts change no bit.

int gmg_gaussian_potential(gmg_context *ctx, int64_t n_atoms, const double *atom_xyz, const double *atom_q, double r_c, int64_t n_points,
                           const double *point_xyz, double *phi, double *grad) {
  if (!ctx) return GMG_ERR_INVALID;
  if (!atoms_ok(n_atoms, atom_xyz, atom_q) || !(r_c > 0.0) || n_points < 0 || (n_points > 0 && !point_xyz))
    return fail(ctx, GMG_ERR_INVALID, "gmg_gaussian_potential: bad arguments");
  if (n_points == 0 || (!phi && !grad)) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  const std::vector<double> xq = pack_xq(n_atoms, atom_xyz, atom_q);
  DevPtr<double> xq_own, pts_own, phi_own, grad_own;
  if (xq_own.alloc(xq.size()) != hipSuccess || pts_own.alloc(3 * (size_t)n_points) != hipSuccess || (phi && phi_own.alloc((size_t)n_points) != hipSuccess) ||
      (grad && grad_own.alloc(3 * (size_t)n_points) != hipSuccess))
    return fail(ctx, GMG_ERR_HIP, "gmg_gaussian_potential: out of memory");
  double *const d_xq = xq_own.get(), *const d_pts = pts_own.get(), *const d_phi = phi_own.get(), *const d_grad = grad_own.get();
  HIPC(hipMemcpyAsync(d_xq, xq.data(), sizeof(double) * xq.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_pts, point_xyz, sizeof(double) * 3 * (size_t)n_points, hipMemcpyHostToDevice, ctx->stream));
  const int bs = ctx->force_block;
  const size_t lds = sizeof(double) * 4 * (size_t)bs;
  const gmg_exact::Gauss g = gmg_exact::Gauss::make(r_c);
  const int64_t per_launch = std::max<int64_t>(1, ((int64_t)1 << ctx->exact_chunk_log2) / std::max<int64_t>(n_atoms, 1));
  for (int64_t p0 = 0; p0 < n_points; p0 += per_launch) {
    const int64_t p1 = std::min(n_points, p0 + per_launch);
    const dim3 grid((unsigned)((p1 - p0 + bs - 1) / bs));
    if (phi && grad)
      hipLaunchKernelGGL((gmg_exact::gauss_potential_kernel<true, true>), grid, dim3(bs), lds, ctx->stream, g, d_xq, (int)n_atoms, d_pts, p0, p1, d_phi, d_grad);
    else if (phi)
      hipLaunchKernelGGL((gmg_exact::gauss_potential_kernel<true, false>), grid, dim3(bs), lds, ctx->stream, g, d_xq, (int)n_atoms, d_pts, p0, p1, d_phi, d_grad);
    else
      hipLaunchKernelGGL((gmg_exact::gauss_potential_kernel<false, true>), grid, dim3(bs), lds, ctx->stream, g, d_xq, (int)n_atoms, d_pts, p0, p1, d_phi, d_grad);
  }
  HIPC(hipGetLastError());
  if (phi) HIPC(hipMemcpyAsync(phi, d_phi, sizeof(double) * (size_t)n_points, hipMemcpyDeviceToHost, ctx->stream));
  if (grad) HIPC(hipMemcpyAsync(grad, d_grad, sizeof(double) * 3 * (size_t)n_points, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

// The two halves of gmg_energy_norm_error's front.  energy_error_check_args: the arguments that are not mesh arrays.
// energy_error_device: the kernels on cell_lo, cell_h and cell_dofs that lie on the device.
static int energy_error_check_args(gmg_context *ctx, const char *who, int64_t n_cells, const double *u, int64_t n_u, int64_t n_atoms, const double *atom_xyz,
                                   const double *atom_q, double r_c, int nq, const double *quadrature_points, const double *weights, const double *shape_grad,
                                   bool mesh_null = false) {
  if (n_cells < 0 || n_cells >= ((int64_t)1 << 28) || n_u < 0 || !atoms_ok(n_atoms, atom_xyz, atom_q) || !(r_c > 0.0) || nq < 1 ||
      (n_cells > 0 && (mesh_null || !u || !quadrature_points || !weights || !shape_grad)))
    return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": bad arguments").c_str());
  if (nq > 64) return fail(ctx, GMG_ERR_UNSUPPORTED, (std::string(who) + ": more than 64 quadrature points per cell").c_str());
  return GMG_OK;
}

static int energy_error_device(gmg_context *ctx, const char *who, int64_t n_cells, const double *d_lo, const double *d_h, const int32_t *d_dofs, const double *u,
                               int64_t n_atoms, const double *atom_xyz, const double *atom_q, double r_c, int nq, const double *quadrature_points,
                               const double *weights, const double *shape_grad, double *error, double *cell_err2) {
  const std::vector<double> xq = pack_xq(n_atoms, atom_xyz, atom_q);
  const size_t nc = (size_t)n_cells;
  DevPtr<double> xq_own, err_own, qp_own, w_own, sg_own;
  if (xq_own.alloc(xq.size()) != hipSuccess || err_own.alloc(nc) != hipSuccess || qp_own.alloc(3 * (size_t)nq) != hipSuccess ||
      w_own.alloc((size_t)nq) != hipSuccess || sg_own.alloc(24 * (size_t)nq) != hipSuccess)
    return fail(ctx, GMG_ERR_HIP, (std::string(who) + ": out of memory").c_str());
  double *const d_xq = xq_own.get(), *const d_err = err_own.get();
  double *const d_qp = qp_own.get(), *const d_w = w_own.get(), *const d_sg = sg_own.get();
  HIPC(hipMemcpyAsync(d_xq, xq.data(), sizeof(double) * xq.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_qp, quadrature_points, sizeof(double) * 3 * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_w, weights, sizeof(double) * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(d_sg, shape_grad, sizeof(double) * 24 * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
  const int bs = ctx->force_block, per_block = bs / nq;
  const size_t lds = sizeof(double) * 5 * (size_t)bs;  // the atom tile and one value per lane
  gmg_exact::ErrorArgs a{gmg_exact::Gauss::make(r_c), d_xq, (int)n_atoms, nq, d_lo, d_h, d_dofs, u, d_qp, d_w, d_sg, 0, 0, d_err};
  const int64_t points = std::max<int64_t>(1, ((int64_t)1 << ctx->exact_chunk_log2) / std::max<int64_t>(n_atoms, 1));
  const int64_t per_launch = std::max<int64_t>(1, points / nq);
  for (int64_t c0 = 0; c0 < n_cells; c0 += per_launch) {
    a.c0 = c0;
    a.c1 = std::min(n_cells, c0 + per_launch);
    hipLaunchKernelGGL(gmg_exact::energy_error_kernel, dim3((unsigned)((a.c1 - a.c0 + per_block - 1) / per_block)), dim3(bs), lds, ctx->stream, a);
  }
  // sum over the cells: partials per workgroup, then one workgroup (the grid depends on n_cells alone)
  const int grid = grid_for(n_cells);
  hipLaunchKernelGGL(sum_partial_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, (const double *)d_err, n_cells, ctx->part_a.get());
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double *)ctx->part_a.get(), grid, 1, 0u, ctx->scal_dev.get());
  HIPC(hipGetLastError());
  if (cell_err2) HIPC(hipMemcpyAsync(cell_err2, d_err, sizeof(double) * nc, hipMemcpyDeviceToHost, ctx->stream));
  CHK(fetch_scalars(ctx, 1));
  if (error) *error = std::sqrt(ctx->scal_host.get()[0]);
  return GMG_OK;
}

int gmg_energy_norm_error(gmg_context *ctx, int64_t n_cells, const double *cell_lo, const double *cell_h, const int32_t *cell_dofs,
                          const double *u, int64_t n_u, int64_t n_atoms, const double *atom_xyz, const double *atom_q, double r_c, int nq,
                          const double *quadrature_points, const double *weights, const double *shape_grad, double *error,
                          double *cell_err2) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_energy_norm_error";
  CHK(energy_error_check_args(ctx, who, n_cells, u, n_u, n_atoms, atom_xyz, atom_q, r_c, nq, quadrature_points, weights, shape_grad,
                              !cell_lo || !cell_h || !cell_dofs));
  for (int64_t i = 0; i < 8 * n_cells; ++i)
    if (cell_dofs[i] < 0 || cell_dofs[i] >= n_u) return fail(ctx, GMG_ERR_INVALID, "gmg_energy_norm_error: a DoF of a cell lies beyond the end of u");
  if (n_cells == 0) {
    if (error) *error = 0.0;
    return GMG_OK;
  }
  (void)hipSetDevice(ctx->device);
  const size_t nc = (size_t)n_cells;
  DevPtr<double> lo_own, h_own;
  DevPtr<int32_t> dofs_own;
  if (lo_own.alloc(3 * nc) != hipSuccess || h_own.alloc(nc) != hipSuccess || dofs_own.alloc(8 * nc) != hipSuccess)
    return fail(ctx, GMG_ERR_HIP, "gmg_energy_norm_error: out of memory");
  HIPC(hipMemcpyAsync(lo_own.get(), cell_lo, sizeof(double) * 3 * nc, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(h_own.get(), cell_h, sizeof(double) * nc, hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dofs_own.get(), cell_dofs, sizeof(int32_t) * 8 * nc, hipMemcpyHostToDevice, ctx->stream));
  return energy_error_device(ctx, who, n_cells, lo_own.get(), h_own.get(), dofs_own.get(), u, n_atoms, atom_xyz, atom_q, r_c, nq, quadrature_points, weights,
                             shape_grad, error, cell_err2);
}

// assemble_system's right-hand side (src/step-50.cc:813-828) from densities that never left the device: per cell
// F_i = sum_q phi_i(x_q) rho(x_q) w_q JxW (:813-820), the Dirichlet terms -K_ij g_j (:825-828) as a list of subtractions, and
// the scatter into the DoFs as a per-DoF gather over the (cell, vertex) slots in the reference's cell order with the
// hanging-node weights -- sequential per DoF: deterministic, no fp64 atomics, the same bits as the host loop.
int gmg_rhs_assemble(gmg_context *ctx, int64_t n_cells, int nq, int dim, const double *shape, const double *weight, const uint8_t *cell_level,
                     const double *jxw_of_level, int64_t n_terms, const int32_t *term_slot, const double *term_value, int64_t n_dofs,
                     const int64_t *dof_ptr, const int32_t *entry_slot, const uint8_t *entry_coef, const double *coef_table, double *rhs) {
  if (!ctx || n_cells < 0 || nq < 1 || nq > 512 || (dim != 2 && dim != 3) || !shape || !weight || !cell_level || !jxw_of_level || n_terms < 0 || n_dofs < 0 ||
      !dof_ptr || !coef_table || !rhs)
    return GMG_ERR_INVALID;
  if (!ctx->dens_dev.get() || ctx->dens_cells != n_cells || ctx->dens_nq != nq)
    return fail(ctx, GMG_ERR_INVALID, "gmg_rhs_assemble: call gmg_charge_density(..., dens = NULL) for these cells first");
  const int nv = 1 << dim;
  const int64_t n_slots = n_cells * nv, n_ent = dof_ptr[n_dofs];
  if (dof_ptr[0] < 0) return fail(ctx, GMG_ERR_INVALID, "gmg_rhs_assemble: dof_ptr starts below 0");
  if ((n_ent > 0 && (!entry_slot || !entry_coef)) || (n_terms > 0 && (!term_slot || !term_value)))
    return fail(ctx, GMG_ERR_INVALID, "gmg_rhs_assemble: a list of nonzero length is NULL");
  if (n_slots >= ((int64_t)1 << 31) || n_ent >= ((int64_t)1 << 31)) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_rhs_assemble: more than 2^31 slots");
  (void)hipSetDevice(ctx->device);
  DevPtr<double> d_F, d_tv;
  DevPtr<uint8_t> d_lv, d_ec;
  DevPtr<int32_t> d_ts, d_es, d_ptr;
  DevPtr<RhsArgs> d_a;  // (the argument block is 39 KB: it travels through memory, not through the kernel-argument segment)
  RhsArgs a{};
  std::vector<int32_t> ptr32((size_t)n_dofs + 1);
  for (int64_t i = 0; i <= n_dofs; ++i) {
    if (i && dof_ptr[i] < dof_ptr[i - 1]) return fail(ctx, GMG_ERR_INVALID, "gmg_rhs_assemble: dof_ptr not monotone");
    ptr32[(size_t)i] = (int32_t)dof_ptr[i];
  }
  for (int64_t c = 0; c < n_cells; ++c)
    if (cell_level[c] > 15) return fail(ctx, GMG_ERR_INVALID, "gmg_rhs_assemble: cell level above 15");
  for (int64_t e = 0; e < n_ent; ++e)
    if (entry_slot[e] < 0 || entry_slot[e] >= n_slots) return fail(ctx, GMG_ERR_INVALID, "gmg_rhs_assemble: slot out of range");
  for (int64_t t = 0; t < n_terms; ++t)
    if (term_slot[t] < 0 || term_slot[t] >= n_slots || (t && term_slot[t] < term_slot[t - 1])) return fail(ctx, GMG_ERR_INVALID, "gmg_rhs_assemble: term slots must ascend inside the slot range");
  HIPC(d_F.alloc((size_t)std::max<int64_t>(n_slots, 1)));
  HIPC(upload(d_lv, cell_level, (size_t)n_cells, ctx->stream));
  HIPC(upload(d_ptr, ptr32, ctx->stream));
  HIPC(upload(d_es, entry_slot, (size_t)n_ent, ctx->stream));
  HIPC(upload(d_ec, entry_coef, (size_t)n_ent, ctx->stream));
  HIPC(upload(d_ts, term_slot, (size_t)n_terms, ctx->stream));
  HIPC(upload(d_tv, term_value, (size_t)n_terms, ctx->stream));
  a.dens = ctx->dens_dev.get(); a.n_cells = n_cells; a.nq = nq; a.nv = nv; a.cell_level = d_lv.get(); a.F = d_F.get();
  for (int q = 0; q < nq; ++q) {
    a.weight[q] = weight[q];
    for (int i = 0; i < nv; ++i) a.shape[q * 8 + i] = shape[q * nv + i];
  }
  for (int l = 0; l < 16; ++l) a.jxw[l] = jxw_of_level[l];
  a.n_terms = n_terms; a.term_slot = d_ts.get(); a.term_value = d_tv.get();
  a.n_dofs = n_dofs; a.dof_ptr = d_ptr.get(); a.entry_slot = d_es.get(); a.entry_coef = d_ec.get(); a.rhs = rhs;
  for (int c = 0; c < 256; ++c) a.coef[c] = coef_table[c];
  HIPC(d_a.alloc(1));
  hipError_t e = hipMemcpyAsync(d_a.get(), &a, sizeof(RhsArgs), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    if (n_cells) hipLaunchKernelGGL(rhs_cell_kernel, dim3(grid_for(n_cells)), dim3(kThreads), 0, ctx->stream, (const RhsArgs *)d_a.get());
    if (n_terms) hipLaunchKernelGGL(rhs_terms_kernel, dim3(grid_for(n_terms)), dim3(kThreads), 0, ctx->stream, (const RhsArgs *)d_a.get());
    if (n_dofs) hipLaunchKernelGGL(rhs_gather_kernel, dim3(grid_for(n_dofs)), dim3(kThreads), 0, ctx->stream, (const RhsArgs *)d_a.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { ctx->err = std::string("gmg_rhs_assemble: ") + hipGetErrorString(e); return GMG_ERR_HIP; }
  return GMG_OK;
}

// ---- the active-mesh system matrix formed on the device (gmg_assemble.hpp) ----

// The argument checks of everything that takes the cell tables and the constraint lines (gmg_assemble_system_matrix[_coef],
// gmg_assemble_rhs), on the host before any launch: the communicator, dim, sizes, NULL arrays (other_null: one of the caller's
// own arrays of nonzero length is NULL), 32-bit device indices, line_ptr, masters, line indices, DoFs and levels.  lp32
// receives line_ptr in 32 bits, max_line the longest line.
static int check_cell_tables(gmg_context *ctx, const char *who, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level,
                             bool other_null, const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr, const int32_t *line_master,
                             const double *line_weight, std::vector<int32_t> &lp32, int64_t &max_line) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator (rank-local assembly does not exist yet)");
  if (dim != 2 && dim != 3) return bad(GMG_ERR_INVALID, "dim must be 2 or 3");
  if (n_dofs < 0 || n_cells < 0 || n_lines < 0) return bad(GMG_ERR_INVALID, "negative size");
  const int nv = 1 << dim;
  if ((n_cells > 0 && (!cell_dofs || !cell_level)) || other_null || (n_dofs > 0 && !constraint_of_dof) || (n_lines > 0 && !line_ptr))
    return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_dofs >= ((int64_t)1 << 31) || n_cells * nv >= ((int64_t)1 << 31) || n_lines >= ((int64_t)1 << 31))
    return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 DoFs, slots or lines");
  lp32.assign((size_t)n_lines + 1, 0);
  max_line = 0;
  if (n_lines > 0) {
    if (line_ptr[0] < 0) return bad(GMG_ERR_INVALID, "line_ptr starts below 0");
    for (int64_t l = 0; l < n_lines; ++l) {
      if (line_ptr[l + 1] < line_ptr[l]) return bad(GMG_ERR_INVALID, "line_ptr decreases");
      max_line = std::max(max_line, line_ptr[l + 1] - line_ptr[l]);
    }
    if (line_ptr[n_lines] >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 line entries");
    for (int64_t l = 0; l <= n_lines; ++l) lp32[(size_t)l] = (int32_t)line_ptr[l];
  }
  const int64_t n_ent = n_lines > 0 ? line_ptr[n_lines] : 0, n_slots = n_cells * nv;
  if (n_ent > 0 && (!line_master || !line_weight)) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  for (int64_t e = line_ptr && n_lines > 0 ? line_ptr[0] : 0; e < n_ent; ++e)
    if (line_master[e] < 0 || line_master[e] >= n_dofs) return bad(GMG_ERR_INVALID, "master outside [0, n_dofs)");
  for (int64_t d = 0; d < n_dofs; ++d)
    if (constraint_of_dof[d] < -1 || constraint_of_dof[d] >= n_lines) return bad(GMG_ERR_INVALID, "line index outside [0, n_lines)");
  for (int64_t s = 0; s < n_slots; ++s)
    if (cell_dofs[s] < 0 || cell_dofs[s] >= n_dofs) return bad(GMG_ERR_INVALID, "DoF outside [0, n_dofs)");
  for (int64_t c = 0; c < n_cells; ++c)
    if (cell_level[c] > 15) return bad(GMG_ERR_INVALID, "cell level of 16 or more");
  // (32-bit slot lists: every slot goes to its DoF and to at most max_line masters)
  if (n_slots * (1 + max_line) >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 (row, slot) pairs");
  return GMG_OK;
}

// The mesh arrays of the assemblies on the device: uploaded by the host-array entries (which own the copies until the stream
// has run the kernels), or the context's resident tables (the _resident entries)
struct CellTablesDev {
  const int32_t *cell_dofs = nullptr;  // [n_cells * 2^dim]
  const uint8_t *cell_level = nullptr;  // [n_cells]
  const int32_t *cons = nullptr, *line_ptr = nullptr, *line_master = nullptr;
  const double *line_weight = nullptr, *line_inhom = nullptr;
  int max_line = 0;
};

static void drop_system(gmg_context *ctx) { reset_keep_halo(ctx->S); ctx->S_invd.reset(); ctx->S_tmp.reset(); }

// the second half of both forms and both sources of the tables: everything after the argument checks and the uploads of the
// mesh arrays.  coef == nullptr takes the per-level cell matrices K_of_level, otherwise K_of_level is unused
static int assemble_system_device(gmg_context *ctx, const char *who, int dim, int64_t n_dofs, int64_t n_cells, const CellTablesDev &t, const double *K_of_level,
                                  const AsmCoef *coef, double *build_ms) {
  auto drop = [&] { drop_system(ctx); };
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  const int nv = 1 << dim;
  const int64_t n_slots = n_cells * nv;
  DevCSR &m = ctx->S;
  drop();
  AsmCoefDev d_coef;
  DevPtr<double> d_K;
  AsmScratch w;
  Event e0, e1;
  if (!coef) HIPC(upload(d_K, K_of_level, n_cells > 0 ? (size_t)16 * nv * nv : 0, ctx->stream));
  CHK(alloc_vec(ctx, ctx->S_invd, n_dofs));
  CHK(alloc_vec(ctx, ctx->S_tmp, n_dofs));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  AsmArgs a{};
  a.nv = nv; a.lg_nv = dim; a.max_line = t.max_line; a.n_dofs = n_dofs; a.n_slots = n_slots;
  a.cell_dofs = t.cell_dofs; a.cell_level = t.cell_level; a.K = d_K.get(); a.cons = t.cons;
  a.line_ptr = t.line_ptr; a.line_master = t.line_master; a.line_weight = t.line_weight;
  a.invd = ctx->S_invd.get();
  if (coef) CHK(upload_coef(ctx, *coef, n_cells, nv, d_coef, a));
  std::vector<int32_t> rp;
  int64_t nnz = 0;
  int32_t n_inc = 0;
  int rc = assemble_rows<false>(ctx, who, a, w, m, rp, nnz, n_inc, [](int64_t) { return (int)GMG_OK; });
  if (rc == GMG_OK) {
    rc = hipEventRecord(e1.get(), ctx->stream) == hipSuccess ? GMG_OK : bad(GMG_ERR_HIP, "hipEventRecord");
    if (rc == GMG_OK) rc = tile_device_csr(ctx, m, rp, n_dofs, n_dofs, nnz);
  }
  if (rc != GMG_OK) {  // (nothing half-built stays behind)
    (void)hipStreamSynchronize(ctx->stream);
    drop();
    return rc;
  }
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] system matrix assembled on the device: %lld rows nnz %lld, %lld (row, slot) pairs, %.3f ms\n", (long long)n_dofs, (long long)nnz, (long long)n_inc, ms);
  return GMG_OK;  // (tile_device_csr has asked hipGetLastError after the last launch)
}

// the first half of the host-array entries: the argument checks, then the mesh arrays go up into copies of this call
static int assemble_system(gmg_context *ctx, const char *who, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level,
                           const double *K_of_level, const AsmCoef *coef, const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr,
                           const int32_t *line_master, const double *line_weight, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  // the coefficient form: whatever the context held goes first, so that after any failure it holds no system matrix (the
  // cell-matrix form leaves the context untouched by arguments it refuses as invalid)
  if (coef) drop_system(ctx);
  std::vector<int32_t> lp32;
  int64_t max_line = 0;
  CHK(check_cell_tables(ctx, who, dim, n_dofs, n_cells, cell_dofs, cell_level, n_cells > 0 && !coef && !K_of_level, constraint_of_dof, n_lines, line_ptr,
                        line_master, line_weight, lp32, max_line));
  const int nv = 1 << dim;
  const int64_t n_ent = n_lines > 0 ? line_ptr[n_lines] : 0, n_slots = n_cells * nv;
  if (coef) CHK(check_coef(ctx, who, *coef, n_cells));
  drop_system(ctx);
  DevPtr<int32_t> d_cd, d_cons, d_lp, d_lm;
  DevPtr<uint8_t> d_lv;
  DevPtr<double> d_lw;
  HIPC(upload(d_cd, cell_dofs, (size_t)n_slots, ctx->stream));
  HIPC(upload(d_lv, cell_level, (size_t)n_cells, ctx->stream));
  HIPC(upload(d_cons, constraint_of_dof, (size_t)n_dofs, ctx->stream));
  HIPC(upload(d_lp, lp32, ctx->stream));
  HIPC(upload(d_lm, line_master, (size_t)n_ent, ctx->stream));
  HIPC(upload(d_lw, line_weight, (size_t)n_ent, ctx->stream));
  CellTablesDev t;
  t.cell_dofs = d_cd.get(); t.cell_level = d_lv.get(); t.cons = d_cons.get(); t.line_ptr = d_lp.get(); t.line_master = d_lm.get(); t.line_weight = d_lw.get();
  t.max_line = (int)max_line;
  // (the copies are released when this returns, as they were: hipFree waits for the kernels that read them)
  return assemble_system_device(ctx, who, dim, n_dofs, n_cells, t, K_of_level, coef, build_ms);
}

int gmg_assemble_system_matrix(gmg_context *ctx, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level,
                               const double *K_of_level, const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr,
                               const int32_t *line_master, const double *line_weight, double *build_ms) {
  return assemble_system(ctx, "gmg_assemble_system_matrix", dim, n_dofs, n_cells, cell_dofs, cell_level, K_of_level, nullptr, constraint_of_dof, n_lines,
                         line_ptr, line_master, line_weight, build_ms);
}

int gmg_assemble_system_matrix_coef(gmg_context *ctx, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level, int nq,
                                    const double *cell_coef, const double *G, const double *qw, const double *scale_of_level,
                                    const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr, const int32_t *line_master,
                                    const double *line_weight, double *build_ms) {
  const AsmCoef coef{nq, cell_coef, G, qw, scale_of_level, 16};
  return assemble_system(ctx, "gmg_assemble_system_matrix_coef", dim, n_dofs, n_cells, cell_dofs, cell_level, nullptr, &coef, constraint_of_dof, n_lines,
                         line_ptr, line_master, line_weight, build_ms);
}

// ---- DoF numbering, constraints and level flags from the forest (gmg_mesh_tables.hpp)

int gmg_build_mesh_tables(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                          const int32_t *cell_first_child, int level0_lexicographic, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  ctx->mesh = MeshTables();  // after any failure the context holds no mesh tables
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string("gmg_build_mesh_tables: ") + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  std::vector<uint8_t> level_of;
  CHK(check_forest(ctx, "gmg_build_mesh_tables", dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of));
  const int nv = 1 << dim, nf = 2 * dim;
  const int64_t n_all = level_ptr[n_levels];
  const int32_t lat[3] = {n0[0], n0[1], dim == 3 ? n0[2] : 1};
  const int64_t n_l0 = n_levels > 0 ? level_ptr[1] : 0;
  const bool lattice0 = level0_lexicographic != 0 && n_all > 0;
  if (lattice0) {  // level 0 must be the full lattice, x fastest
    if (n_l0 != (int64_t)lat[0] * lat[1] * lat[2]) return bad(GMG_ERR_INVALID, "level0_lexicographic: level 0 is not the full lattice");
    for (int64_t c = 0; c < n_l0; ++c)
      if (cell_coord[3 * c] != c % lat[0] || cell_coord[3 * c + 1] != (c / lat[0]) % lat[1] || cell_coord[3 * c + 2] != c / ((int64_t)lat[0] * lat[1]))
        return bad(GMG_ERR_INVALID, "level0_lexicographic: level 0 is not in lexicographic cell order");
  }
  // the scratch lives until the stream has run the kernels
  DevPtr<int32_t> d_coord, d_fc, d_apos, d_active, d_rank, d_tdof, d_cidx, d_lbase, d_ebase, d_drank;
  DevPtr<uint8_t> d_lvl, d_hangs, d_edge;
  DevPtr<unsigned long long> d_akeys, d_vkeys, d_ckeys, d_visit;
  DevPtr<unsigned int> d_afirst, d_vfirst, d_hpos;
  DevPtr<int> d_err;
  Event e0, e1;
  MeshTables mt;
  mt.dim = dim;
  mt.level.resize((size_t)n_levels);
  auto table_size = [](int64_t n) { unsigned long long t = 1024; while ((int64_t)t < 2 * n) t <<= 1; return t; };
  HIPC(upload(d_coord, cell_coord, (size_t)n_all * 3, ctx->stream));
  HIPC(upload(d_fc, cell_first_child, (size_t)n_all, ctx->stream));
  HIPC(upload(d_lvl, level_of, ctx->stream));
  HIPC(d_err.alloc(1));
  HIPC(hipMemsetAsync(d_err.get(), 0, sizeof(int), ctx->stream));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  MtForest f{};
  f.coord = d_coord.get(); f.first_child = d_fc.get(); f.level = d_lvl.get(); f.dim = dim; f.nv = nv; f.nf = nf;
  for (int d = 0; d < 3; ++d) { f.n0[d] = lat[d]; f.hi[d] = (unsigned long long)lat[d] << kMtShift; }
  const dim3 blk(kMtThreads);
  // the flag word, and what it means once the stream has been waited for
  auto flagged = [&](int &rc) -> int {
    int err = 0;
    HIPC(hipMemcpyAsync(&err, d_err.get(), sizeof err, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    rc = err & kMtErrDuplicate    ? bad(GMG_ERR_INVALID, "the same cell appears twice")
         : err & kMtErrUnbalanced ? bad(GMG_ERR_INVALID, "hanging node without a DoF: the mesh is not 2:1 balanced")
         : err & kMtErrFull       ? bad(GMG_ERR_HIP, "a hash table filled up")
                                  : (int)GMG_OK;
    return GMG_OK;
  };
  // 1. the active cells, by (level, index)
  HIPC(d_apos.alloc((size_t)n_all + 1));
  if (n_all) hipLaunchKernelGGL(mt_active_flag_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const int32_t *)d_fc.get(), n_all, d_apos.get());
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_apos.get(), n_all);
  int32_t n_active32 = 0;
  HIPC(hipMemcpyAsync(&n_active32, d_apos.get() + n_all, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  const int64_t n_active = n_active32;
  mt.n_cells = n_active;
  HIPC(d_active.alloc((size_t)std::max<int64_t>(n_active, 1)));
  HIPC(mt.cell_level.alloc((size_t)std::max<int64_t>(n_active, 1)));
  HIPC(mt.cell_dofs.alloc((size_t)std::max<int64_t>(n_active * nv, 1)));
  if (n_all) hipLaunchKernelGGL(mt_active_list_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, f, n_all, (const int32_t *)d_apos.get(), d_active.get(), mt.cell_level.get());
  // first-touch numbering of a cell list (gmg_mesh_tables.hpp, kernels 1 - 3); keys / first: a table of `size` entries
  int64_t max_slots = n_active * nv;
  for (int l = 0; l < n_levels; ++l) max_slots = std::max(max_slots, (level_ptr[l + 1] - level_ptr[l]) * nv);
  HIPC(d_rank.alloc((size_t)max_slots + 1));
  HIPC(d_hpos.alloc((size_t)std::max<int64_t>(max_slots, 1)));
  auto number = [&](const int32_t *cells, int64_t begin, int64_t n_slots, unsigned long long *keys, unsigned int *first, unsigned long long size, int32_t *tdof,
                    DevPtr<int32_t> &cell_dofs, DevPtr<unsigned long long> &vertex_of_dof, int64_t &n_dofs, int &rc) -> int {
    HIPC(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * size, ctx->stream));
    HIPC(hipMemsetAsync(first, 0xff, sizeof(unsigned int) * size, ctx->stream));
    const dim3 g = asm_blocks(ctx, n_slots, kMtThreads);
    if (n_slots) {
      hipLaunchKernelGGL(mt_vertex_insert_kernel, g, blk, 0, ctx->stream, f, cells, begin, n_slots, keys, first, d_hpos.get(), size - 1, d_err.get());
      hipLaunchKernelGGL(mt_first_flag_kernel, g, blk, 0, ctx->stream, (const unsigned int *)first, (const unsigned int *)d_hpos.get(), n_slots, d_rank.get());
    }
    hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_rank.get(), n_slots);
    int32_t n32 = 0;
    HIPC(hipMemcpyAsync(&n32, d_rank.get() + n_slots, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    CHK(flagged(rc));  // (a full table leaves first slots unset: nothing may index through them)
    if (rc != GMG_OK) return GMG_OK;
    n_dofs = n32;
    HIPC(vertex_of_dof.alloc((size_t)std::max<int64_t>(n_dofs, 1)));
    if (n_slots)
      hipLaunchKernelGGL(mt_number_kernel, g, blk, 0, ctx->stream, (const unsigned long long *)keys, (const unsigned int *)first, (const unsigned int *)d_hpos.get(),
                         (const int32_t *)d_rank.get(), n_slots, cell_dofs.get(), vertex_of_dof.get(), tdof);
    return GMG_OK;
  };
  int rc = GMG_OK;
  // 2. the active numbering; its table stays for the hanging nodes
  const unsigned long long a_size = table_size(n_active * nv);
  HIPC(d_akeys.alloc(a_size));
  HIPC(d_afirst.alloc(a_size));
  HIPC(d_tdof.alloc(a_size));
  CHK(number(d_active.get(), 0, n_active * nv, d_akeys.get(), d_afirst.get(), a_size, d_tdof.get(), mt.cell_dofs, mt.vertex_of_dof, mt.n_dofs, rc));
  if (rc != GMG_OK) return rc;
  // 3. level by level: the cells by coordinates, the level numbering, the faces (hanging faces of the active cells, the
  // refinement edge), the flags
  int64_t max_level_cells = 0;
  for (int l = 0; l < n_levels; ++l) max_level_cells = std::max(max_level_cells, level_ptr[l + 1] - level_ptr[l]);
  const unsigned long long v_size_max = table_size(max_level_cells * nv), c_size_max = table_size(max_level_cells);
  HIPC(d_vkeys.alloc(v_size_max));
  HIPC(d_vfirst.alloc(v_size_max));
  HIPC(d_ckeys.alloc(c_size_max));
  HIPC(d_cidx.alloc(c_size_max));
  HIPC(d_hangs.alloc((size_t)std::max<int64_t>(n_active * nf, 1)));
  HIPC(hipMemsetAsync(d_hangs.get(), 0, (size_t)std::max<int64_t>(n_active * nf, 1), ctx->stream));
  for (int l = 0; l < n_levels; ++l) {
    MeshTables::PerLevel &L = mt.level[(size_t)l];
    const int64_t begin = level_ptr[l], n_cells = level_ptr[l + 1] - begin;
    L.n_cells = n_cells;
    HIPC(L.cell_dofs.alloc((size_t)std::max<int64_t>(n_cells * nv, 1)));
    if (l == 0 && lattice0) {
      L.n_dofs = (int64_t)(lat[0] + 1) * (lat[1] + 1) * (dim == 3 ? lat[2] + 1 : 1);
      HIPC(L.vertex_of_dof.alloc((size_t)L.n_dofs));
      hipLaunchKernelGGL(mt_lattice_kernel, asm_blocks(ctx, std::max(n_cells * nv, L.n_dofs), kMtThreads), blk, 0, ctx->stream, f, n_cells, L.n_dofs, L.cell_dofs.get(),
                         L.vertex_of_dof.get());
    } else {
      CHK(number(nullptr, begin, n_cells * nv, d_vkeys.get(), d_vfirst.get(), table_size(n_cells * nv), nullptr, L.cell_dofs, L.vertex_of_dof, L.n_dofs, rc));
      if (rc != GMG_OK) return rc;
    }
    const unsigned long long c_size = table_size(n_cells);
    HIPC(hipMemsetAsync(d_ckeys.get(), 0xff, sizeof(unsigned long long) * c_size, ctx->stream));
    HIPC(d_edge.alloc((size_t)std::max<int64_t>(L.n_dofs, 1)));
    HIPC(hipMemsetAsync(d_edge.get(), 0, (size_t)std::max<int64_t>(L.n_dofs, 1), ctx->stream));
    HIPC(L.dof_flags.alloc((size_t)std::max<int64_t>(L.n_dofs, 1)));
    if (n_cells) {
      hipLaunchKernelGGL(mt_cell_insert_kernel, asm_blocks(ctx, n_cells, kMtThreads), blk, 0, ctx->stream, f, begin, n_cells, d_ckeys.get(), d_cidx.get(), c_size - 1, d_err.get());
      CHK(flagged(rc));  // (a cell met twice or a full table leaves positions without an index)
      if (rc != GMG_OK) return rc;
      hipLaunchKernelGGL(mt_level_face_kernel, asm_blocks(ctx, n_cells * nf, kMtThreads), blk, 0, ctx->stream, f, l, begin, n_cells, (const unsigned long long *)d_ckeys.get(),
                         (const int32_t *)d_cidx.get(), c_size - 1, (const int32_t *)d_apos.get(), (const int32_t *)L.cell_dofs.get(), d_hangs.get(), d_edge.get());
    }
    if (L.n_dofs)
      hipLaunchKernelGGL(mt_level_flags_kernel, asm_blocks(ctx, L.n_dofs, kMtThreads), blk, 0, ctx->stream, f, (const unsigned long long *)L.vertex_of_dof.get(),
                         (const uint8_t *)d_edge.get(), L.n_dofs, L.dof_flags.get());
    HIPC(hipStreamSynchronize(ctx->stream));  // (d_edge is allocated anew for the next level)
  }
  // 4. the hanging-node lines, then the Dirichlet lines behind them
  const int64_t n_dofs = mt.n_dofs;
  HIPC(d_visit.alloc((size_t)std::max<int64_t>(n_dofs, 1)));
  HIPC(hipMemsetAsync(d_visit.get(), 0xff, sizeof(unsigned long long) * (size_t)std::max<int64_t>(n_dofs, 1), ctx->stream));
  HIPC(d_lbase.alloc((size_t)n_active + 1));
  HIPC(d_ebase.alloc((size_t)n_active + 1));
  HIPC(d_drank.alloc((size_t)n_dofs + 1));
  HIPC(mt.constraint_of_dof.alloc((size_t)std::max<int64_t>(n_dofs, 1)));
  HIPC(hipMemsetAsync(mt.constraint_of_dof.get(), 0xff, sizeof(int32_t) * (size_t)std::max<int64_t>(n_dofs, 1), ctx->stream));
  MtHang a{};
  a.active_cell = d_active.get(); a.face_hangs = d_hangs.get(); a.cell_dofs = mt.cell_dofs.get(); a.keys = d_akeys.get(); a.tdof = d_tdof.get(); a.mask = a_size - 1;
  a.visit = d_visit.get(); a.n_active = n_active; a.err = d_err.get(); a.line_base = d_lbase.get(); a.entry_base = d_ebase.get();
  const dim3 g_cells = asm_blocks(ctx, n_active, kMtThreads), g_dofs = asm_blocks(ctx, n_dofs, kMtThreads);
  if (n_active) {
    hipLaunchKernelGGL(mt_hang_visit_kernel, asm_blocks(ctx, n_active * nf, kMtThreads), blk, 0, ctx->stream, f, a);
    hipLaunchKernelGGL(mt_hang_lines_kernel<false>, g_cells, blk, 0, ctx->stream, f, a);
  }
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_lbase.get(), n_active);
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_ebase.get(), n_active);
  if (n_dofs)
    hipLaunchKernelGGL(mt_dirichlet_flag_kernel, g_dofs, blk, 0, ctx->stream, f, (const unsigned long long *)mt.vertex_of_dof.get(), (const unsigned long long *)d_visit.get(), n_dofs,
                       d_drank.get());
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_drank.get(), n_dofs);
  int32_t n_hanging = 0, n_entries = 0, n_dirichlet = 0;
  HIPC(hipMemcpyAsync(&n_hanging, d_lbase.get() + n_active, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&n_entries, d_ebase.get() + n_active, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&n_dirichlet, d_drank.get() + n_dofs, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  CHK(flagged(rc));
  if (rc != GMG_OK) return rc;
  mt.n_hanging = n_hanging; mt.n_entries = n_entries; mt.n_lines = (int64_t)n_hanging + n_dirichlet;
  HIPC(mt.line_ptr.alloc((size_t)mt.n_lines + 1));
  HIPC(mt.line_dof.alloc((size_t)std::max<int64_t>(mt.n_lines, 1)));
  HIPC(mt.line_master.alloc((size_t)std::max<int64_t>(mt.n_entries, 1)));
  HIPC(mt.line_weight.alloc((size_t)std::max<int64_t>(mt.n_entries, 1)));
  a.constraint_of_dof = mt.constraint_of_dof.get(); a.line_dof = mt.line_dof.get(); a.line_ptr = mt.line_ptr.get(); a.line_master = mt.line_master.get();
  a.line_weight = mt.line_weight.get();
  if (n_active) hipLaunchKernelGGL(mt_hang_lines_kernel<true>, g_cells, blk, 0, ctx->stream, f, a);
  hipLaunchKernelGGL(mt_dirichlet_lines_kernel, g_dofs, blk, 0, ctx->stream, f, (const unsigned long long *)mt.vertex_of_dof.get(), (const unsigned long long *)d_visit.get(),
                     (const int32_t *)d_drank.get(), n_dofs, n_hanging, (int32_t)mt.n_lines, n_entries, mt.constraint_of_dof.get(), mt.line_dof.get(), mt.line_ptr.get());
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  CHK(launch_status(ctx));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  mt.valid = true;
  ctx->mesh = std::move(mt);
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] mesh tables built on the device: %lld active cells, %lld DoFs, %lld hanging + %lld Dirichlet lines, %.3f ms\n", (long long)n_active,
                 (long long)n_dofs, (long long)n_hanging, (long long)n_dirichlet, ms);
  return GMG_OK;
}

int gmg_get_mesh_tables(gmg_context *ctx, int64_t *n_cells, int64_t *n_dofs, int64_t *n_hanging, int64_t *n_lines, int64_t *n_entries, int32_t *cell_dofs,
                        uint8_t *cell_level, uint64_t *vertex_of_dof, int32_t *constraint_of_dof, int64_t *line_ptr, int32_t *line_master, double *line_weight,
                        int32_t *line_dof) {
  if (!ctx) return GMG_ERR_INVALID;
  const MeshTables &m = ctx->mesh;
  if (!m.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_mesh_tables: the context holds no mesh tables");
  (void)hipSetDevice(ctx->device);
  if (n_cells) *n_cells = m.n_cells;
  if (n_dofs) *n_dofs = m.n_dofs;
  if (n_hanging) *n_hanging = m.n_hanging;
  if (n_lines) *n_lines = m.n_lines;
  if (n_entries) *n_entries = m.n_entries;
  std::vector<int32_t> lp(line_ptr ? (size_t)m.n_lines + 1 : 0);
  HIPC(mesh_fetch(ctx, cell_dofs, m.cell_dofs, m.n_cells << m.dim));
  HIPC(mesh_fetch(ctx, cell_level, m.cell_level, m.n_cells));
  HIPC(mesh_fetch(ctx, (unsigned long long *)vertex_of_dof, m.vertex_of_dof, m.n_dofs));
  HIPC(mesh_fetch(ctx, constraint_of_dof, m.constraint_of_dof, m.n_dofs));
  HIPC(mesh_fetch(ctx, line_ptr ? lp.data() : nullptr, m.line_ptr, m.n_lines + 1));
  HIPC(mesh_fetch(ctx, line_master, m.line_master, m.n_entries));
  HIPC(mesh_fetch(ctx, line_weight, m.line_weight, m.n_entries));
  HIPC(mesh_fetch(ctx, line_dof, m.line_dof, m.n_lines));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < lp.size(); ++i) line_ptr[i] = lp[i];
  return GMG_OK;
}

int gmg_get_mesh_level_tables(gmg_context *ctx, int level, int64_t *n_cells, int64_t *n_dofs, int32_t *cell_dofs, uint64_t *vertex_of_dof, uint8_t *dof_flags) {
  if (!ctx) return GMG_ERR_INVALID;
  const MeshTables &m = ctx->mesh;
  if (!m.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_mesh_level_tables: the context holds no mesh tables");
  if (level < 0 || level >= (int)m.level.size()) return fail(ctx, GMG_ERR_INVALID, "gmg_get_mesh_level_tables: no such level in the mesh tables");
  (void)hipSetDevice(ctx->device);
  const MeshTables::PerLevel &L = m.level[(size_t)level];
  if (n_cells) *n_cells = L.n_cells;
  if (n_dofs) *n_dofs = L.n_dofs;
  HIPC(mesh_fetch(ctx, cell_dofs, L.cell_dofs, L.n_cells << m.dim));
  HIPC(mesh_fetch(ctx, (unsigned long long *)vertex_of_dof, L.vertex_of_dof, L.n_dofs));
  HIPC(mesh_fetch(ctx, dof_flags, L.dof_flags, L.n_dofs));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

// ---- the step between two cycles from the forest alone (gmg_refine.hpp)

namespace {

// the forest on the device with every level's cells by coordinates (mt_cell_insert_kernel); level[l] for l = 0 .. n_levels - 1
struct ForestDev {
  DevPtr<int32_t> coord, fc, cidx;
  DevPtr<uint8_t> lvl;
  DevPtr<unsigned long long> ckeys;
  DevPtr<int> err;
  std::vector<RfLevel> level;
  MtForest f{};
  int64_t n_all = 0;
};

unsigned long long rf_table_size(int64_t n) { unsigned long long t = 1024; while ((int64_t)t < 2 * n) t <<= 1; return t; }

// the flag word once the stream has been waited for; rc: what it means
int rf_flagged(gmg_context *ctx, const char *who, const DevPtr<int> &d_err, int &rc) {
  int err = 0;
  HIPC(hipMemcpyAsync(&err, d_err.get(), sizeof err, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  const char *msg = err & kMtErrDuplicate    ? "the same cell or vertex appears twice"
                    : err & kMtErrUnbalanced ? "a neighbour position without a cell on the level below: the forest is not vertex-balanced"
                    : err & kRfErrOrphan     ? "a cell without a parent"
                    : err & kRfErrMissing    ? "a vertex without a value: the old vertices do not cover the parents of the new ones"
                    : err & kRfErrFace       ? "mesh not 2:1 balanced across a face"
                    : err & kMtErrFull       ? "a hash table filled up"
                                             : nullptr;
  rc = msg ? fail(ctx, err & ~(kMtErrFull) ? GMG_ERR_INVALID : GMG_ERR_HIP, (std::string(who) + ": " + msg).c_str()) : (int)GMG_OK;
  return GMG_OK;
}

int forest_to_device(gmg_context *ctx, const char *who, int dim, const int32_t *n0, int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                     const int32_t *cell_first_child, const std::vector<uint8_t> &level_of, ForestDev &d, int &rc) {
  const int64_t n_all = level_ptr[n_levels];
  d.n_all = n_all;
  HIPC(upload(d.coord, cell_coord, (size_t)n_all * 3, ctx->stream));
  HIPC(upload(d.fc, cell_first_child, (size_t)n_all, ctx->stream));
  HIPC(upload(d.lvl, level_of, ctx->stream));
  HIPC(d.err.alloc(1));
  HIPC(hipMemsetAsync(d.err.get(), 0, sizeof(int), ctx->stream));
  MtForest &f = d.f;
  f.coord = d.coord.get(); f.first_child = d.fc.get(); f.level = d.lvl.get(); f.dim = dim; f.nv = 1 << dim; f.nf = 2 * dim;
  for (int e = 0; e < 3; ++e) { f.n0[e] = e < dim ? n0[e] : 1; f.hi[e] = (unsigned long long)f.n0[e] << kMtShift; }
  std::vector<unsigned long long> off((size_t)n_levels + 1, 0);
  for (int l = 0; l < n_levels; ++l) off[(size_t)l + 1] = off[(size_t)l] + rf_table_size(level_ptr[l + 1] - level_ptr[l]);
  const size_t total = (size_t)std::max<unsigned long long>(off[(size_t)n_levels], 1);
  HIPC(d.ckeys.alloc(total));
  HIPC(d.cidx.alloc(total));
  HIPC(hipMemsetAsync(d.ckeys.get(), 0xff, sizeof(unsigned long long) * total, ctx->stream));
  d.level.resize((size_t)n_levels);
  for (int l = 0; l < n_levels; ++l) {
    RfLevel &L = d.level[(size_t)l];
    L.keys = d.ckeys.get() + off[(size_t)l]; L.index = d.cidx.get() + off[(size_t)l]; L.mask = off[(size_t)l + 1] - off[(size_t)l] - 1;
    L.begin = level_ptr[l]; L.n = level_ptr[l + 1] - level_ptr[l];
    if (L.n)
      hipLaunchKernelGGL(mt_cell_insert_kernel, asm_blocks(ctx, L.n, kMtThreads), dim3(kMtThreads), 0, ctx->stream, f, L.begin, L.n, d.ckeys.get() + off[(size_t)l],
                         d.cidx.get() + off[(size_t)l], L.mask, d.err.get());
  }
  CHK(rf_flagged(ctx, who, d.err, rc));  // (a cell met twice or a full table leaves positions without an index)
  return GMG_OK;
}

float rf_elapsed(Event &e0, Event &e1) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  return ms;
}

}  // namespace

// Both refinement entries.  marked = false: flag [cells of all levels] is the host's; marked = true (gmg_refine_forest_marked):
// the flags are formed on the device from the marks gmg_estimate_error_resident left in the context, by the active numbers
// (the scan gmg_build_face_table forms).  Everything after the flags is the same code.
static int refine_forest(gmg_context *ctx, const char *who, bool marked, int dim, const int32_t *n0, int n_levels, const int64_t *level_ptr,
                         const int32_t *cell_coord, const int32_t *cell_first_child, const uint8_t *flag, int *new_n_levels, int64_t *new_n_cells,
                         int64_t *n_split, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  if (marked && !ctx->mesh.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  std::vector<uint8_t> level_of;
  CHK(check_forest(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of));
  const int nv = 1 << dim;
  const int64_t n_all = level_ptr[n_levels];
  if (!marked && n_all > 0 && !flag) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (marked) {
    if (!ctx->mesh.marks.valid) return bad(GMG_ERR_INVALID, "the context holds no marks (gmg_estimate_error_resident)");
    int64_t na = 0;
    for (int64_t c = 0; c < n_all; ++c) na += cell_first_child[c] < 0;
    if (na != ctx->mesh.n_cells) return bad(GMG_ERR_INVALID, "the forest's active cells are not as many as the marks");
  }
  ForestDev d;
  DevPtr<uint8_t> d_flag, d_F;
  DevPtr<int32_t> d_rank, d_apos;
  Event e0, e1;
  RefinedForest out;
  int rc = GMG_OK;
  if (!marked) HIPC(upload(d_flag, flag, (size_t)n_all, ctx->stream));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  CHK(forest_to_device(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of, d, rc));
  if (rc != GMG_OK) return rc;
  const dim3 blk(kMtThreads);
  if (marked) {  // flag[c] = the mark of c's active number (every active number is below n_cells: counted above)
    HIPC(d_flag.alloc((size_t)std::max<int64_t>(n_all, 1)));
    HIPC(d_apos.alloc((size_t)n_all + 1));
    if (n_all) hipLaunchKernelGGL(mt_active_flag_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const int32_t *)d.fc.get(), n_all, d_apos.get());
    hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_apos.get(), n_all);
    if (n_all)
      hipLaunchKernelGGL(rf_mark_flag_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const int32_t *)d.fc.get(), (const int32_t *)d_apos.get(),
                         (const uint8_t *)ctx->mesh.marks.mark.get(), n_all, d_flag.get());
  }
  // 1. the closure, from the finest level down to level 1
  HIPC(d_F.alloc((size_t)std::max<int64_t>(n_all, 1)));
  HIPC(d_rank.alloc((size_t)n_all + 1));
  if (n_all) hipLaunchKernelGGL(rf_flag_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const int32_t *)d.fc.get(), (const uint8_t *)d_flag.get(), n_all, d_F.get());
  for (int l = n_levels - 1; l >= 1; --l) {
    const RfLevel &cur = d.level[(size_t)l];
    if (cur.n)
      hipLaunchKernelGGL(rf_closure_kernel, asm_blocks(ctx, cur.n * (dim == 3 ? 27 : 9), kMtThreads), blk, 0, ctx->stream, d.f, l, cur, d.level[(size_t)l - 1], d_F.get(), d.err.get());
  }
  // 2. the rank of every split cell, and with it the sizes
  if (n_all) hipLaunchKernelGGL(rf_split_flag_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const uint8_t *)d_F.get(), n_all, d_rank.get());
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_rank.get(), n_all);
  std::vector<int32_t> rank_at((size_t)n_levels + 1, 0);
  for (int l = 0; l <= n_levels; ++l)
    HIPC(hipMemcpyAsync(&rank_at[(size_t)l], d_rank.get() + level_ptr[l], sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  CHK(rf_flagged(ctx, who, d.err, rc));  // (before anything is sized by the ranks)
  if (rc != GMG_OK) return rc;
  const int64_t split_last = n_levels > 0 ? rank_at[(size_t)n_levels] - rank_at[(size_t)n_levels - 1] : 0;
  out.n_levels = n_levels + (split_last > 0 ? 1 : 0);
  if (out.n_levels > kMtShift + 1) return bad(GMG_ERR_UNSUPPORTED, "a split on level 12: no level beyond 12");
  out.n_flags = n_all;
  out.n_split = rank_at[(size_t)n_levels];
  out.n_cells = n_all + (int64_t)nv * out.n_split;
  if (out.n_cells * nv >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 slots");
  out.level_ptr.assign((size_t)out.n_levels + 1, 0);
  std::vector<int64_t> old_size((size_t)out.n_levels + 1, 0);
  for (int l = 0; l < n_levels; ++l) old_size[(size_t)l] = level_ptr[l + 1] - level_ptr[l];
  for (int l = 0; l < out.n_levels; ++l)
    out.level_ptr[(size_t)l + 1] = out.level_ptr[(size_t)l] + old_size[(size_t)l] + (l > 0 ? (int64_t)nv * (rank_at[(size_t)l] - rank_at[(size_t)l - 1]) : 0);
  // 3. the new forest
  HIPC(out.coord.alloc((size_t)std::max<int64_t>(out.n_cells * 3, 1)));
  HIPC(out.first_child.alloc((size_t)std::max<int64_t>(out.n_cells, 1)));
  HIPC(out.parent.alloc((size_t)std::max<int64_t>(out.n_cells, 1)));
  for (int l = 0; l < n_levels; ++l) {
    const RfLevel &cur = d.level[(size_t)l];
    if (!cur.n) continue;
    RfSplit s{};
    s.F = d_F.get(); s.rank = d_rank.get(); s.rank_base = rank_at[(size_t)l];
    s.new_begin = out.level_ptr[(size_t)l];
    s.new_begin_next = l + 1 < out.n_levels ? out.level_ptr[(size_t)l + 1] : out.n_cells;  // (no next level: nothing of this one is split)
    s.old_size_next = old_size[(size_t)l + 1];
    s.coord = out.coord.get(); s.first_child = out.first_child.get(); s.parent = out.parent.get();
    hipLaunchKernelGGL(rf_split_kernel, asm_blocks(ctx, cur.n, kMtThreads), blk, 0, ctx->stream, d.f, l, cur, l > 0 ? d.level[(size_t)l - 1] : RfLevel{}, s, d.err.get());
  }
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  CHK(rf_flagged(ctx, who, d.err, rc));
  if (rc != GMG_OK) return rc;
  CHK(launch_status(ctx));
  out.closed = std::move(d_F);
  out.valid = true;
  if (new_n_levels) *new_n_levels = out.n_levels;
  if (new_n_cells) *new_n_cells = out.n_cells;
  if (n_split) *n_split = out.n_split;
  if (build_ms) *build_ms = rf_elapsed(e0, e1);
  ctx->refined = std::move(out);
  return GMG_OK;
}

int gmg_refine_forest(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                      const int32_t *cell_first_child, const uint8_t *flag, int *new_n_levels, int64_t *new_n_cells, int64_t *n_split, double *build_ms) {
  return refine_forest(ctx, "gmg_refine_forest", false, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, flag, new_n_levels, new_n_cells, n_split,
                       build_ms);
}

int gmg_refine_forest_marked(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                             const int32_t *cell_first_child, int *new_n_levels, int64_t *new_n_cells, int64_t *n_split, double *build_ms) {
  return refine_forest(ctx, "gmg_refine_forest_marked", true, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, nullptr, new_n_levels, new_n_cells,
                       n_split, build_ms);
}

int gmg_get_refined_forest(gmg_context *ctx, int *n_levels, int64_t *n_cells, int64_t *n_flags, int64_t *n_split, int64_t *level_ptr, int32_t *cell_coord,
                           int32_t *cell_first_child, int32_t *cell_parent, uint8_t *closed_flag) {
  if (!ctx) return GMG_ERR_INVALID;
  const RefinedForest &r = ctx->refined;
  if (!r.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_refined_forest: the context holds no refined forest");
  (void)hipSetDevice(ctx->device);
  if (n_levels) *n_levels = r.n_levels;
  if (n_cells) *n_cells = r.n_cells;
  if (n_flags) *n_flags = r.n_flags;
  if (n_split) *n_split = r.n_split;
  if (level_ptr) std::copy(r.level_ptr.begin(), r.level_ptr.end(), level_ptr);
  HIPC(mesh_fetch(ctx, cell_coord, r.coord, r.n_cells * 3));
  HIPC(mesh_fetch(ctx, cell_first_child, r.first_child, r.n_cells));
  HIPC(mesh_fetch(ctx, cell_parent, r.parent, r.n_cells));
  HIPC(mesh_fetch(ctx, closed_flag, r.closed, r.n_flags));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

int gmg_transfer_solution(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                          const int32_t *cell_first_child, int64_t n_old, const uint64_t *old_vertex_of_dof, const double *u_old, int64_t n_new,
                          const uint64_t *new_vertex_of_dof, const int32_t *constraint_of_dof, double *u_new, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  const char *who = "gmg_transfer_solution";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  std::vector<uint8_t> level_of;
  CHK(check_forest(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of));
  if (n_old < 0 || n_new < 0) return bad(GMG_ERR_INVALID, "a negative number of DoFs");
  if ((n_old > 0 && (!old_vertex_of_dof || !u_old)) || (n_new > 0 && (!new_vertex_of_dof || !u_new))) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_old >= ((int64_t)1 << 31) || n_new >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 DoFs");
  const int nv = 1 << dim;
  const int64_t n_all = level_ptr[n_levels], begin1 = n_levels > 0 ? level_ptr[1] : 0;
  DevPtr<int32_t> d_coord, d_fc, d_oidx, d_nidx, d_cons;
  DevPtr<uint8_t> d_lvl, d_have;
  DevPtr<unsigned long long> d_overt, d_nvert, d_okeys, d_nkeys;
  DevPtr<double> d_u;
  DevPtr<int> d_err;
  Event e0, e1;
  int rc = GMG_OK;
  HIPC(upload(d_coord, cell_coord, (size_t)n_all * 3, ctx->stream));
  HIPC(upload(d_fc, cell_first_child, (size_t)n_all, ctx->stream));
  HIPC(upload(d_lvl, level_of, ctx->stream));
  HIPC(upload(d_overt, (const unsigned long long *)old_vertex_of_dof, (size_t)n_old, ctx->stream));
  HIPC(upload(d_nvert, (const unsigned long long *)new_vertex_of_dof, (size_t)n_new, ctx->stream));
  if (constraint_of_dof) HIPC(upload(d_cons, constraint_of_dof, (size_t)n_new, ctx->stream));
  HIPC(d_err.alloc(1));
  HIPC(hipMemsetAsync(d_err.get(), 0, sizeof(int), ctx->stream));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  MtForest f{};
  f.coord = d_coord.get(); f.first_child = d_fc.get(); f.level = d_lvl.get(); f.dim = dim; f.nv = nv; f.nf = 2 * dim;
  for (int e = 0; e < 3; ++e) { f.n0[e] = e < dim ? n0[e] : 1; f.hi[e] = (unsigned long long)f.n0[e] << kMtShift; }
  const unsigned long long o_size = rf_table_size(n_old), n_size = rf_table_size(n_new);
  HIPC(d_okeys.alloc(o_size));
  HIPC(d_oidx.alloc(o_size));
  HIPC(d_nkeys.alloc(n_size));
  HIPC(d_nidx.alloc(n_size));
  HIPC(d_have.alloc((size_t)std::max<int64_t>(n_new, 1)));
  HIPC(d_u.alloc((size_t)std::max<int64_t>(n_new, 1)));
  HIPC(hipMemsetAsync(d_okeys.get(), 0xff, sizeof(unsigned long long) * o_size, ctx->stream));
  HIPC(hipMemsetAsync(d_nkeys.get(), 0xff, sizeof(unsigned long long) * n_size, ctx->stream));
  const dim3 blk(kMtThreads);
  if (n_old) hipLaunchKernelGGL(rf_vertex_insert_kernel, asm_blocks(ctx, n_old, kMtThreads), blk, 0, ctx->stream, (const unsigned long long *)d_overt.get(), n_old, d_okeys.get(), d_oidx.get(), o_size - 1, d_err.get());
  if (n_new) hipLaunchKernelGGL(rf_vertex_insert_kernel, asm_blocks(ctx, n_new, kMtThreads), blk, 0, ctx->stream, (const unsigned long long *)d_nvert.get(), n_new, d_nkeys.get(), d_nidx.get(), n_size - 1, d_err.get());
  CHK(rf_flagged(ctx, who, d_err, rc));  // (a vertex met twice or a full table leaves positions without an index)
  if (rc != GMG_OK) return rc;
  RfTransfer t{};
  t.okeys = d_okeys.get(); t.nkeys = d_nkeys.get(); t.oidx = d_oidx.get(); t.nidx = d_nidx.get(); t.omask = o_size - 1; t.nmask = n_size - 1;
  t.u_old = u_old; t.u_new = d_u.get(); t.have = d_have.get(); t.err = d_err.get();
  const int64_t n_slots = (n_all - begin1) * nv;
  if (n_new) hipLaunchKernelGGL(rf_transfer_old_kernel, asm_blocks(ctx, n_new, kMtThreads), blk, 0, ctx->stream, t, (const unsigned long long *)d_nvert.get(), n_new);
  if (n_slots) hipLaunchKernelGGL(rf_transfer_interp_kernel, asm_blocks(ctx, n_slots, kMtThreads), blk, 0, ctx->stream, f, begin1, n_slots, t);
  if (n_new) hipLaunchKernelGGL(rf_transfer_finish_kernel, asm_blocks(ctx, n_new, kMtThreads), blk, 0, ctx->stream, t, (const int32_t *)d_cons.get(), n_new);
  CHK(rf_flagged(ctx, who, d_err, rc));
  if (rc != GMG_OK) return rc;
  CHK(launch_status(ctx));
  if (n_new) HIPC(hipMemcpyAsync(u_new, d_u.get(), sizeof(double) * (size_t)n_new, hipMemcpyDeviceToDevice, ctx->stream));
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (build_ms) *build_ms = rf_elapsed(e0, e1);
  return GMG_OK;
}

// the device half of both face-table entries: the forest's faces by kind for its na active cells, left in d_kind / d_cell
static int face_table_device(gmg_context *ctx, const char *who, int dim, const int32_t *n0, int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                             const int32_t *cell_first_child, const std::vector<uint8_t> &level_of, int64_t na, DevPtr<uint8_t> &d_kind, DevPtr<int32_t> &d_cell,
                             float &ms) {
  const int nv = 1 << dim, nf = 2 * dim, nfc = nv / 2;
  const int64_t n_all = level_ptr[n_levels];
  ForestDev d;
  DevPtr<int32_t> d_apos;
  Event e0, e1;
  int rc = GMG_OK;
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  CHK(forest_to_device(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of, d, rc));
  if (rc != GMG_OK) return rc;
  const dim3 blk(kMtThreads);
  const size_t nk = (size_t)std::max<int64_t>(na * nf, 1), ncell = nk * (size_t)nfc;
  HIPC(d_apos.alloc((size_t)n_all + 1));
  HIPC(d_kind.alloc(nk));
  HIPC(d_cell.alloc(ncell));
  HIPC(hipMemsetAsync(d_kind.get(), 0, nk, ctx->stream));
  HIPC(hipMemsetAsync(d_cell.get(), 0, sizeof(int32_t) * ncell, ctx->stream));
  if (n_all) hipLaunchKernelGGL(mt_active_flag_kernel, asm_blocks(ctx, n_all, kMtThreads), blk, 0, ctx->stream, (const int32_t *)d.fc.get(), n_all, d_apos.get());
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_apos.get(), n_all);
  for (int l = 0; l < n_levels; ++l) {
    const RfLevel &cur = d.level[(size_t)l];
    if (cur.n)
      hipLaunchKernelGGL(rf_face_kernel, asm_blocks(ctx, cur.n * nf, kMtThreads), blk, 0, ctx->stream, d.f, l, cur, l > 0 ? d.level[(size_t)l - 1] : RfLevel{}, level_ptr[l + 1],
                         (const int32_t *)d_apos.get(), d_kind.get(), d_cell.get(), d.err.get());
  }
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  CHK(rf_flagged(ctx, who, d.err, rc));
  if (rc != GMG_OK) return rc;
  CHK(launch_status(ctx));
  ms = rf_elapsed(e0, e1);
  return GMG_OK;
}

int gmg_build_face_table(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                         const int32_t *cell_first_child, int64_t *n_active, uint8_t *face_kind, int32_t *face_cell, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  const char *who = "gmg_build_face_table";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  std::vector<uint8_t> level_of;
  CHK(check_forest(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of));
  const int nv = 1 << dim, nf = 2 * dim, nfc = nv / 2;
  const int64_t n_all = level_ptr[n_levels];
  int64_t na = 0;
  for (int64_t c = 0; c < n_all; ++c) na += cell_first_child[c] < 0;
  if (!face_kind && !face_cell) {  // the size alone
    if (n_active) *n_active = na;
    return GMG_OK;
  }
  if (na > 0 && (!face_kind || !face_cell)) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  DevPtr<int32_t> d_cell;
  DevPtr<uint8_t> d_kind;
  float ms = 0.f;
  CHK(face_table_device(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of, na, d_kind, d_cell, ms));
  HIPC(mesh_fetch(ctx, face_kind, d_kind, na * nf));
  HIPC(mesh_fetch(ctx, face_cell, d_cell, na * nf * nfc));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (n_active) *n_active = na;
  if (build_ms) *build_ms = ms;
  return GMG_OK;
}

// gmg_build_face_table with the table left in the context, next to the mesh tables whose active cells it numbers (DESIGN.md
// section 24).  The marks of an earlier estimate belong to the table they were formed with and leave with it.
int gmg_build_face_table_resident(gmg_context *ctx, int dim, const int32_t n0[3], int n_levels, const int64_t *level_ptr, const int32_t *cell_coord,
                                  const int32_t *cell_first_child, int64_t *n_active, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  const char *who = "gmg_build_face_table_resident";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  ctx->mesh.faces = MeshTables::Faces();  // after any failure the context holds no face table
  ctx->mesh.marks = MeshTables::Marks();
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  if (!ctx->mesh.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  std::vector<uint8_t> level_of;
  CHK(check_forest(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of));
  if (dim != ctx->mesh.dim) return bad(GMG_ERR_INVALID, "dim differs from the mesh tables'");
  const int64_t n_all = level_ptr[n_levels];
  int64_t na = 0;
  for (int64_t c = 0; c < n_all; ++c) na += cell_first_child[c] < 0;
  if (na != ctx->mesh.n_cells) return bad(GMG_ERR_INVALID, "the forest's active cells are not as many as the mesh tables' n_cells");
  MeshTables::Faces faces;
  float ms = 0.f;
  CHK(face_table_device(ctx, who, dim, n0, n_levels, level_ptr, cell_coord, cell_first_child, level_of, na, faces.kind, faces.cell, ms));
  faces.valid = true;
  ctx->mesh.faces = std::move(faces);  // (nothing after this can fail)
  if (n_active) *n_active = na;
  if (build_ms) *build_ms = ms;
  return GMG_OK;
}

int gmg_get_face_table(gmg_context *ctx, int64_t *n_active, uint8_t *face_kind, int32_t *face_cell) {
  if (!ctx) return GMG_ERR_INVALID;
  if (ctx->dist) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_get_face_table: not on a communicator");
  const MeshTables &m = ctx->mesh;
  if (!m.valid || !m.faces.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_face_table: the context holds no face table (gmg_build_face_table_resident)");
  (void)hipSetDevice(ctx->device);
  const int64_t nf = 2 * m.dim, nfc = (int64_t)1 << (m.dim - 1);
  if (n_active) *n_active = m.n_cells;
  HIPC(mesh_fetch(ctx, face_kind, m.faces.kind, m.n_cells * nf));
  HIPC(mesh_fetch(ctx, face_cell, m.faces.cell, m.n_cells * nf * nfc));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

// ---- the right-hand side from the cell tables, and constraints.distribute on the same tables (gmg_rhs_cells.hpp, DESIGN.md
// section 19)

// the checks of the right-hand side's own arguments, shared by both entries (after the checks of the mesh arrays)
static int check_rhs_args(gmg_context *ctx, const char *who, int64_t n_cells, bool any_inhom, const double *K_of_level, int nq, const double *source) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (nq < 1 || nq > 512) return bad(GMG_ERR_INVALID, "nq must be in 1 .. 512");
  if (!source && n_cells > 0 && (!ctx->dens_dev.get() || ctx->dens_cells != n_cells || ctx->dens_nq != nq))
    return bad(GMG_ERR_INVALID, "source is NULL and the device holds no densities of n_cells x nq (gmg_charge_density with dens = NULL)");
  if (any_inhom && !K_of_level) return bad(GMG_ERR_INVALID, "K_of_level is NULL while a line_inhomogeneity is not 0");
  return GMG_OK;
}

// the second half of gmg_assemble_rhs and gmg_assemble_rhs_resident: everything after the argument checks and the uploads of
// the mesh arrays
static int assemble_rhs_device(gmg_context *ctx, const char *who, int dim, int64_t n_dofs, int64_t n_cells, const CellTablesDev &t, bool any_inhom,
                               const double *K_of_level, int nq, const double *shape, const double *weight, const double *jxw_of_level, const double *source,
                               double *rhs, double *build_ms) {
  (void)hipSetDevice(ctx->device);
  const int nv = 1 << dim;
  const int64_t n_slots = n_cells * nv;
  DevPtr<double> d_K, d_src, d_F;
  DevPtr<RhsArgs> d_ra;  // (the argument block of rhs_cell_kernel is 39 KB: it travels through memory)
  AsmScratch w;
  Event e0, e1;
  if (any_inhom) HIPC(upload(d_K, K_of_level, (size_t)16 * nv * nv, ctx->stream));
  if (source) HIPC(upload(d_src, source, (size_t)n_cells * (size_t)nq, ctx->stream));
  HIPC(d_F.alloc((size_t)std::max<int64_t>(n_slots, 1)));
  RhsArgs ra{};
  ra.dens = source ? d_src.get() : ctx->dens_dev.get(); ra.n_cells = n_cells; ra.nq = nq; ra.nv = nv; ra.cell_level = t.cell_level; ra.F = d_F.get();
  for (int q = 0; q < nq; ++q) {
    ra.weight[q] = weight[q];
    for (int i = 0; i < nv; ++i) ra.shape[q * 8 + i] = shape[q * nv + i];
  }
  for (int l = 0; l < 16; ++l) ra.jxw[l] = jxw_of_level[l];
  HIPC(d_ra.alloc(1));
  HIPC(hipMemcpyAsync(d_ra.get(), &ra, sizeof(RhsArgs), hipMemcpyHostToDevice, ctx->stream));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  AsmArgs a{};
  a.nv = nv; a.lg_nv = dim; a.max_line = t.max_line; a.n_dofs = n_dofs; a.n_slots = n_slots;
  a.cell_dofs = t.cell_dofs; a.cell_level = t.cell_level; a.cons = t.cons;
  a.line_ptr = t.line_ptr; a.line_master = t.line_master; a.line_weight = t.line_weight;
  int32_t n_inc = 0;
  int rc = assemble_incidence<false>(ctx, a, w, n_inc);
  if (rc != GMG_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  RhsCellsArgs r{};
  r.nv = nv; r.lg_nv = dim; r.n_dofs = n_dofs; r.n_slots = n_slots; r.cell_dofs = t.cell_dofs; r.cell_level = t.cell_level; r.K = d_K.get();
  r.cons = t.cons; r.line_ptr = t.line_ptr; r.line_master = t.line_master; r.line_weight = t.line_weight; r.line_inhom = t.line_inhom;
  r.inc_ptr = a.inc_ptr; r.inc_slot = a.inc_slot; r.F = d_F.get(); r.rhs = rhs;
  if (n_cells) hipLaunchKernelGGL(rhs_cell_kernel, asm_blocks(ctx, n_cells, kThreads), dim3(kThreads), 0, ctx->stream, (const RhsArgs *)d_ra.get());
  if (n_slots && any_inhom) hipLaunchKernelGGL(rhs_cells_dirichlet_kernel, asm_blocks(ctx, n_slots, 256), dim3(256), 0, ctx->stream, r);
  if (n_dofs) hipLaunchKernelGGL(rhs_cells_gather_kernel, asm_blocks(ctx, n_dofs, 256), dim3(256), 0, ctx->stream, r);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(e1.get(), ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // (the tables above live until the stream has run the kernels)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) { ctx->err = std::string(who) + ": " + hipGetErrorString(e); return GMG_ERR_HIP; }
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] right-hand side from cell tables: %lld DoFs, %lld cells x %d points, %lld (row, slot) pairs, %.3f ms\n", (long long)n_dofs,
                 (long long)n_cells, nq, (long long)n_inc, ms);
  return GMG_OK;
}

int gmg_assemble_rhs(gmg_context *ctx, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level,
                     const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr, const int32_t *line_master, const double *line_weight,
                     const double *line_inhomogeneity, const double *K_of_level, int nq, const double *shape, const double *weight,
                     const double *jxw_of_level, const double *source, double *rhs, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_assemble_rhs";
  std::vector<int32_t> lp32;
  int64_t max_line = 0;
  CHK(check_cell_tables(ctx, who, dim, n_dofs, n_cells, cell_dofs, cell_level,
                        !shape || !weight || !jxw_of_level || (n_dofs > 0 && !rhs) || (n_lines > 0 && !line_inhomogeneity), constraint_of_dof, n_lines,
                        line_ptr, line_master, line_weight, lp32, max_line));
  bool any_inhom = false;
  for (int64_t l = 0; l < n_lines; ++l) any_inhom = any_inhom || line_inhomogeneity[l] != 0.0;
  CHK(check_rhs_args(ctx, who, n_cells, any_inhom, K_of_level, nq, source));
  (void)hipSetDevice(ctx->device);
  const int nv = 1 << dim;
  const int64_t n_ent = n_lines > 0 ? line_ptr[n_lines] : 0, n_slots = n_cells * nv;
  DevPtr<int32_t> d_cd, d_cons, d_lp, d_lm;
  DevPtr<uint8_t> d_lv;
  DevPtr<double> d_lw, d_li;
  HIPC(upload(d_cd, cell_dofs, (size_t)n_slots, ctx->stream));
  HIPC(upload(d_lv, cell_level, (size_t)n_cells, ctx->stream));
  HIPC(upload(d_cons, constraint_of_dof, (size_t)n_dofs, ctx->stream));
  HIPC(upload(d_lp, lp32, ctx->stream));
  HIPC(upload(d_lm, line_master, (size_t)n_ent, ctx->stream));
  HIPC(upload(d_lw, line_weight, (size_t)n_ent, ctx->stream));
  HIPC(upload(d_li, line_inhomogeneity, (size_t)n_lines, ctx->stream));
  CellTablesDev t;
  t.cell_dofs = d_cd.get(); t.cell_level = d_lv.get(); t.cons = d_cons.get(); t.line_ptr = d_lp.get(); t.line_master = d_lm.get(); t.line_weight = d_lw.get();
  t.line_inhom = d_li.get(); t.max_line = (int)max_line;
  return assemble_rhs_device(ctx, who, dim, n_dofs, n_cells, t, any_inhom, K_of_level, nq, shape, weight, jxw_of_level, source, rhs, build_ms);
}

// the launch of constraints.distribute, shared by gmg_distribute_constraints and gmg_distribute_constraints_resident
static int distribute_device(gmg_context *ctx, const char *who, int64_t n_dofs, double *u, const CellTablesDev &t) {
  hipLaunchKernelGGL(distribute_constraints_kernel, asm_blocks(ctx, n_dofs, 256), dim3(256), 0, ctx->stream, n_dofs, t.cons, t.line_ptr, t.line_master, t.line_weight,
                     t.line_inhom, u);
  hipError_t e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) { ctx->err = std::string(who) + ": " + hipGetErrorString(e); return GMG_ERR_HIP; }
  return GMG_OK;
}

int gmg_distribute_constraints(gmg_context *ctx, int64_t n_dofs, double *u, const int32_t *constraint_of_dof, int64_t n_lines, const int64_t *line_ptr,
                               const int32_t *line_master, const double *line_weight, const double *line_inhomogeneity) {
  if (!ctx) return GMG_ERR_INVALID;
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string("gmg_distribute_constraints: ") + msg).c_str()); };
  if (n_dofs < 0 || n_lines < 0) return bad(GMG_ERR_INVALID, "negative size");
  if ((n_dofs > 0 && (!u || !constraint_of_dof)) || (n_lines > 0 && (!line_ptr || !line_inhomogeneity))) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_dofs >= ((int64_t)1 << 31) || n_lines >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 DoFs or lines");
  std::vector<int32_t> lp32((size_t)n_lines + 1, 0);
  if (n_lines > 0) {
    if (line_ptr[0] < 0) return bad(GMG_ERR_INVALID, "line_ptr starts below 0");
    for (int64_t l = 0; l < n_lines; ++l)
      if (line_ptr[l + 1] < line_ptr[l]) return bad(GMG_ERR_INVALID, "line_ptr decreases");
    if (line_ptr[n_lines] >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 line entries");
    for (int64_t l = 0; l <= n_lines; ++l) lp32[(size_t)l] = (int32_t)line_ptr[l];
  }
  const int64_t n_ent = n_lines > 0 ? line_ptr[n_lines] : 0;
  if (n_ent > 0 && (!line_master || !line_weight)) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  for (int64_t d = 0; d < n_dofs; ++d)
    if (constraint_of_dof[d] < -1 || constraint_of_dof[d] >= n_lines) return bad(GMG_ERR_INVALID, "line index outside [0, n_lines)");
  for (int64_t e = n_lines > 0 ? line_ptr[0] : 0; e < n_ent; ++e) {
    if (line_master[e] < 0 || line_master[e] >= n_dofs) return bad(GMG_ERR_INVALID, "master outside [0, n_dofs)");
    // (the host loop runs in place and ascending: one thread per constrained DoF agrees with it only when no master is constrained)
    if (constraint_of_dof[line_master[e]] >= 0) return bad(GMG_ERR_INVALID, "a master is itself constrained");
  }
  if (n_dofs == 0) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  DevPtr<int32_t> d_cons, d_lp, d_lm;
  DevPtr<double> d_lw, d_li;
  HIPC(upload(d_cons, constraint_of_dof, (size_t)n_dofs, ctx->stream));
  HIPC(upload(d_lp, lp32, ctx->stream));
  HIPC(upload(d_lm, line_master, (size_t)n_ent, ctx->stream));
  HIPC(upload(d_lw, line_weight, (size_t)n_ent, ctx->stream));
  HIPC(upload(d_li, line_inhomogeneity, (size_t)n_lines, ctx->stream));
  CellTablesDev t;
  t.cons = d_cons.get(); t.line_ptr = d_lp.get(); t.line_master = d_lm.get(); t.line_weight = d_lw.get(); t.line_inhom = d_li.get();
  return distribute_device(ctx, "gmg_distribute_constraints", n_dofs, u, t);
}

int gmg_get_system_matrix(gmg_context *ctx, int64_t *n_rows, int64_t *nnz, int64_t *rowptr, int32_t *col, double *val) {
  if (!ctx) return GMG_ERR_INVALID;
  const DevCSR &m = ctx->S;
  if (!m.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_system_matrix: system matrix not set");
  if (!m.rowptr.get() || !m.col.get() || !m.val.get()) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_get_system_matrix: no CSR copy of the system matrix on the device");
  if (n_rows) *n_rows = m.n_rows;
  if (nnz) *nnz = m.nnz;
  if (!rowptr) return GMG_OK;
  if (m.nnz && (!col || !val)) return fail(ctx, GMG_ERR_INVALID, "gmg_get_system_matrix: col / val are NULL");
  (void)hipSetDevice(ctx->device);
  std::vector<int32_t> rp((size_t)m.n_rows + 1);
  HIPC(hipMemcpyAsync(rp.data(), m.rowptr.get(), sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (m.nnz) {
    HIPC(hipMemcpyAsync(col, m.col.get(), sizeof(int32_t) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(val, m.val.get(), sizeof(double) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < rp.size(); ++i) rowptr[i] = rp[i];
  return GMG_OK;
}

int gmg_system_matrix_norms(gmg_context *ctx, double *l1, double *linf, double *frobenius) {
  if (!ctx) return GMG_ERR_INVALID;
  const DevCSR &m = ctx->S;
  if (!m.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_system_matrix_norms: system matrix not set");
  if (ctx->dist) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_system_matrix_norms: not on a communicator");
  if (!m.rowptr.get() || !m.col.get() || !m.val.get() || m.n_rows != m.n_cols)
    return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_system_matrix_norms: no CSR copy of the system matrix on the device");
  (void)hipSetDevice(ctx->device);
  DevPtr<double> rs, cs;
  CHK(alloc_vec(ctx, rs, m.n_rows));
  CHK(alloc_vec(ctx, cs, m.n_rows));
  int64_t g = std::max<int64_t>(1, std::min<int64_t>(1 << 16, (m.n_rows + 255) / 256));
  if (ctx->assemble_max_blocks > 0) g = std::min<int64_t>(g, ctx->assemble_max_blocks);
  if (m.n_rows)
    hipLaunchKernelGGL(asm_norm_sums_kernel, dim3((unsigned)g), dim3(256), 0, ctx->stream, (const int32_t *)m.rowptr.get(), (const int32_t *)m.col.get(),
                       (const double *)m.val.get(), m.n_rows, rs.get(), cs.get());
  double s1, s2, mx;
  CHK(gmg_vec_norms(ctx, rs.get(), m.n_rows, &s1, &s2, &mx));
  if (linf) *linf = mx;
  CHK(gmg_vec_norms(ctx, cs.get(), m.n_rows, &s1, &s2, &mx));
  if (l1) *l1 = mx;
  CHK(gmg_vec_norms(ctx, m.val.get(), m.nnz, &s1, &s2, &mx));
  if (frobenius) *frobenius = s2;
  return GMG_OK;
}

// ---- the multigrid level and interface matrices formed on the device (gmg_assemble.hpp) ----

// the checks of a level assembly that do not read the mesh arrays (both forms, both sources of the tables)
static int check_level_args(gmg_context *ctx, const char *who, int level, int dim, int64_t n_dofs, int64_t n_cells, bool mesh_null, const double *K,
                            const AsmCoef *coef) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator (rank-local assembly does not exist yet)");
  if (level == 0 && l0_partitioned(ctx)) return bad(GMG_ERR_UNSUPPORTED, "a row-partitioned level 0 takes its local rows as CSR (gmg_set_level_matrix)");
  if (dim != 2 && dim != 3) return bad(GMG_ERR_INVALID, "dim must be 2 or 3");
  if (n_dofs < 0 || n_cells < 0) return bad(GMG_ERR_INVALID, "negative size");
  const int nv = 1 << dim;
  if (mesh_null || (n_cells > 0 && !coef && !K)) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_dofs >= ((int64_t)1 << 31) || n_cells >= ((int64_t)1 << 31) / nv) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 DoFs or slots");
  if (coef) CHK(check_coef(ctx, who, *coef, n_cells));
  return GMG_OK;
}

// the second half of a level assembly: d_cell_dofs [n_cells * 2^dim] and d_flags [n_dofs] are on the device, uploaded by the
// host-array entries or resident (the _resident entries).  coef == nullptr takes the level's cell matrix K, otherwise K is unused
static int assemble_level_device(gmg_context *ctx, const char *who, int level, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *d_cell_dofs,
                                 const double *K, const AsmCoef *coef, const uint8_t *d_flags, double *build_ms) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  const int nv = 1 << dim;
  const int64_t n_slots = n_cells * nv;
  const auto ex = level > 0 ? ctx->ssor_block_rows.find(level) : ctx->ssor_block_rows.end();
  const std::vector<int64_t> *explicit_rows = ex == ctx->ssor_block_rows.end() ? nullptr : &ex->second;
  if (explicit_rows && explicit_rows->back() != n_dofs)
    return bad(GMG_ERR_INVALID, "the SSOR block boundaries of this level (gmg_set_ssor_block_rows) do not end at n_dofs");
  Level &L = ctx->lv[(size_t)level];
  DevCSR &m = L.A;
  DevPtr<double> d_K, d_eval;
  AsmCoefDev d_coef;
  DevPtr<unsigned long long> d_lmax;
  AsmScratch w;
  Event e0, e1;
  if (!coef) HIPC(upload(d_K, K, n_cells > 0 ? (size_t)nv * nv : 0, ctx->stream));
  HIPC(L.I.rowptr.alloc((size_t)n_dofs + 1));  // (the row kernel counts I_l's entries into it)
  HIPC(d_lmax.alloc(1));
  CHK(alloc_vec(ctx, L.invd, n_dofs));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  HIPC(hipMemsetAsync(L.I.rowptr.get(), 0, sizeof(int32_t) * ((size_t)n_dofs + 1), ctx->stream));
  HIPC(hipMemsetAsync(d_lmax.get(), 0, sizeof(unsigned long long), ctx->stream));
  AsmArgs a{};
  a.nv = nv; a.lg_nv = dim; a.max_line = 0; a.n_dofs = n_dofs; a.n_slots = n_slots;
  a.cell_dofs = d_cell_dofs; a.K = d_K.get(); a.flags = d_flags; a.invd = L.invd.get(); a.edge_cnt = L.I.rowptr.get();
  if (coef) CHK(upload_coef(ctx, *coef, n_cells, nv, d_coef, a));
  std::vector<int32_t> rp;
  int64_t nnz = 0;
  int32_t n_inc = 0;
  CHK(assemble_rows<true>(ctx, who, a, w, m, rp, nnz, n_inc, [&](int64_t nz) {
    HIPC(d_eval.alloc((size_t)std::max<int64_t>(nz, 1)));
    a.edge_val = d_eval.get();
    return (int)GMG_OK;
  }));
  const dim3 g_dofs = asm_blocks(ctx, n_dofs, 256);
  const int32_t *c_rp = m.rowptr.get(), *c_col = m.col.get();
  if (n_dofs) hipLaunchKernelGGL(asm_gershgorin_kernel, g_dofs, dim3(256), 0, ctx->stream, c_rp, c_col, (const double *)m.val.get(), n_dofs, d_lmax.get());
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, L.I.rowptr.get(), n_dofs);
  // the host needs the row pointers for the tilings and, unless the SSOR plan is formed on the device (option ssor_plan_device),
  // the CSR for setup_sgs
  std::vector<int32_t> col_h, irp((size_t)n_dofs + 1), trp;
  std::vector<double> val_h;
  const bool plan_on_host = level > 0 && !ctx->ssor_plan_device;
  if (plan_on_host) { col_h.resize((size_t)nnz); val_h.resize((size_t)nnz); }
  unsigned long long lmax_bits = 0;
  HIPC(hipMemcpyAsync(irp.data(), L.I.rowptr.get(), sizeof(int32_t) * irp.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&lmax_bits, d_lmax.get(), sizeof lmax_bits, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  const int64_t n_edge = irp[(size_t)n_dofs];
  if (n_edge > 0) {
    const size_t pad = 8;
    for (DevCSR *x : {&L.I, &L.It}) {
      HIPC(x->col.alloc((size_t)n_edge + pad));
      HIPC(x->val.alloc((size_t)n_edge + pad));
      HIPC(hipMemsetAsync(x->col.get() + n_edge, 0, sizeof(int32_t) * pad, ctx->stream));
      HIPC(hipMemsetAsync(x->val.get() + n_edge, 0, sizeof(double) * pad, ctx->stream));
    }
    HIPC(L.It.rowptr.alloc((size_t)n_dofs + 1));
    const int32_t *c_irp = L.I.rowptr.get(), *c_icol = L.I.col.get();
    const double *c_ival = L.I.val.get();
    hipLaunchKernelGGL(asm_edge_fill_kernel, g_dofs, dim3(256), 0, ctx->stream, c_rp, c_col, (const double *)d_eval.get(), n_dofs, c_irp, L.I.col.get(), L.I.val.get());
    hipLaunchKernelGGL(asm_edge_transpose_kernel<false>, g_dofs, dim3(256), 0, ctx->stream, c_rp, c_col, n_dofs, c_irp, c_icol, c_ival, L.It.rowptr.get(), L.It.col.get(), L.It.val.get());
    hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, L.It.rowptr.get(), n_dofs);
    hipLaunchKernelGGL(asm_edge_transpose_kernel<true>, g_dofs, dim3(256), 0, ctx->stream, c_rp, c_col, n_dofs, c_irp, c_icol, c_ival, L.It.rowptr.get(), L.It.col.get(), L.It.val.get());
    trp.resize((size_t)n_dofs + 1);
    HIPC(hipMemcpyAsync(trp.data(), L.It.rowptr.get(), sizeof(int32_t) * trp.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  if (plan_on_host && nnz) {
    HIPC(hipMemcpyAsync(col_h.data(), m.col.get(), sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(val_h.data(), m.val.get(), sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  CHK(tile_device_csr(ctx, m, rp, n_dofs, n_dofs, nnz));
  if (n_edge > 0) {
    if (trp[(size_t)n_dofs] != n_edge) return bad(GMG_ERR_HIP, "the transposed interface matrix lost entries");
    CHK(tile_device_csr(ctx, L.I, irp, n_dofs, n_dofs, n_edge));
    CHK(tile_device_csr(ctx, L.It, trp, n_dofs, n_dofs, n_edge));
    L.has_I = true;
  } else {
    L.I = DevCSR(); L.It = DevCSR();
  }
  std::memcpy(&L.cheb_lmax, &lmax_bits, sizeof(double));
  if (level > 0) {
    L.n = n_dofs;  // (the SGS plan reads it)
    const std::vector<int64_t> rp64(rp.begin(), rp.end());
    if (plan_on_host) {
      CHK(setup_sgs(ctx, L, n_dofs, rp64.data(), col_h.data(), val_h.data(), explicit_rows));
      L.sgs.csr_bytes_down = 12 * nnz;
    } else {
      CHK(setup_sgs_any(ctx, L, n_dofs, m.rowptr.get(), m.col.get(), m.val.get(), rp64.data(), nullptr, nullptr, explicit_rows,
                        [&](const int32_t **c, const double **v, int64_t *moved) {
                          col_h.resize((size_t)nnz); val_h.resize((size_t)nnz);
                          if (nnz) {
                            HIPC(hipMemcpyAsync(col_h.data(), m.col.get(), sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
                            HIPC(hipMemcpyAsync(val_h.data(), m.val.get(), sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
                            HIPC(hipStreamSynchronize(ctx->stream));
                          }
                          *c = col_h.data(); *v = val_h.data(); *moved = 12 * nnz;
                          return (int)GMG_OK;
                        }));
    }
  }
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] level %d matrix assembled on the device: %lld rows nnz %lld, %lld (row, slot) pairs, interface matrix nnz %lld, %.3f ms\n", level,
                 (long long)n_dofs, (long long)nnz, (long long)n_inc, (long long)n_edge, ms);
  return finish_level(ctx, level, n_dofs, n_dofs, nnz);
}

// the first half of the host-array entries: the argument checks, then the mesh arrays go up into copies of this call
static int assemble_level_checked(gmg_context *ctx, const char *who, int level, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs,
                                  const double *K, const AsmCoef *coef, const uint8_t *dof_flags, double *build_ms) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  CHK(check_level_args(ctx, who, level, dim, n_dofs, n_cells, (n_cells > 0 && !cell_dofs) || (n_dofs > 0 && !dof_flags), K, coef));
  const int64_t n_slots = n_cells << dim;
  for (int64_t s = 0; s < n_slots; ++s)
    if (cell_dofs[s] < 0 || cell_dofs[s] >= n_dofs) return bad(GMG_ERR_INVALID, "DoF outside [0, n_dofs)");
  for (int64_t d = 0; d < n_dofs; ++d)
    if (dof_flags[d] > 3) return bad(GMG_ERR_INVALID, "flag bits above 1");
  DevPtr<int32_t> d_cd;
  DevPtr<uint8_t> d_fl;
  HIPC(upload(d_cd, cell_dofs, (size_t)n_slots, ctx->stream));
  HIPC(upload(d_fl, dof_flags, (size_t)n_dofs, ctx->stream));
  return assemble_level_device(ctx, who, level, dim, n_dofs, n_cells, d_cd.get(), K, coef, d_fl.get(), build_ms);
}

// The resident form's first half (gmg_assemble_level_matrix[_coef]_resident): the level's cell table and
// flags are the ones gmg_build_mesh_tables left on the device, in range by construction, so only their presence is checked.
static int assemble_level_resident(gmg_context *ctx, const char *who, int level, const double *K, const AsmCoef *coef, double *build_ms) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator (rank-local assembly does not exist yet)");
  const MeshTables &mt = ctx->mesh;
  if (!mt.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  if (level >= (int)mt.level.size()) return bad(GMG_ERR_INVALID, "no such level in the mesh tables");
  const MeshTables::PerLevel &T = mt.level[(size_t)level];
  CHK(check_level_args(ctx, who, level, mt.dim, T.n_dofs, T.n_cells, false, K, coef));
  return assemble_level_device(ctx, who, level, mt.dim, T.n_dofs, T.n_cells, T.cell_dofs.get(), K, coef, T.dof_flags.get(), build_ms);
}

// the host-array entries (resident = false: the mesh arguments are used) and the resident ones (they are ignored)
static int assemble_level(gmg_context *ctx, const char *who, int level, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, const double *K,
                          const AsmCoef *coef, const uint8_t *dof_flags, double *build_ms, bool resident = false) {
  if (!ctx) return GMG_ERR_INVALID;
  if (level < 0 || level >= ctx->n_levels) return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": level outside the context").c_str());
  (void)hipSetDevice(ctx->device);
  Level &L = ctx->lv[(size_t)level];
  // whatever the level held goes first: after a failure it holds no operator
  auto clear = [&] {
    reset_keep_halo(L.A);
    L.I = DevCSR(); L.It = DevCSR();
    L.has_I = false;
    L.invd.reset();
    L.cheb_lmax = 0.0;
    L.cheb_est = Level::ChebEstimate();
    L.sgs = SgsPlan();
  };
  clear();
  if (level == 0) drop_coarse_direct(ctx);  // (a new level 0: back to the coarse CG)
  const int rc = resident ? assemble_level_resident(ctx, who, level, K, coef, build_ms)
                          : assemble_level_checked(ctx, who, level, dim, n_dofs, n_cells, cell_dofs, K, coef, dof_flags, build_ms);
  if (rc != GMG_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    clear();
  }
  return rc;
}

int gmg_assemble_level_matrix(gmg_context *ctx, int level, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, const double *K,
                              const uint8_t *dof_flags, double *build_ms) {
  return assemble_level(ctx, "gmg_assemble_level_matrix", level, dim, n_dofs, n_cells, cell_dofs, K, nullptr, dof_flags, build_ms);
}

int gmg_assemble_level_matrix_coef(gmg_context *ctx, int level, int dim, int64_t n_dofs, int64_t n_cells, const int32_t *cell_dofs, int nq,
                                   const double *cell_coef, const double *G, const double *qw, double scale, const uint8_t *dof_flags, double *build_ms) {
  const AsmCoef coef{nq, cell_coef, G, qw, &scale, 1};
  return assemble_level(ctx, "gmg_assemble_level_matrix_coef", level, dim, n_dofs, n_cells, cell_dofs, nullptr, &coef, dof_flags, build_ms);
}

// ---- boundary values and close() on the resident mesh tables, and the consumers that read the tables where they lie
// (gmg_close.hpp)

int gmg_close_constraints(gmg_context *ctx, int64_t n_values, const double *dirichlet_value, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  ctx->mesh.closed = MeshTables::Closed();  // after any failure the context holds no closed constraints
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string("gmg_close_constraints: ") + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  const MeshTables &mt = ctx->mesh;
  if (!mt.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  const int64_t H = mt.n_hanging, L = mt.n_lines;
  if (n_values != L - H) return bad(GMG_ERR_INVALID, "n_values is not the number of Dirichlet lines (n_lines - n_hanging)");
  MeshTables::Closed c;
  DevPtr<int> d_flag;
  Event e0, e1;
  HIPC(c.line_ptr.alloc((size_t)L + 1));
  HIPC(c.line_inhom.alloc((size_t)std::max<int64_t>(L, 1)));
  HIPC(d_flag.alloc(1));
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  HIPC(hipMemsetAsync(c.line_ptr.get(), 0, sizeof(int32_t) * ((size_t)L + 1), ctx->stream));
  HIPC(hipMemsetAsync(d_flag.get(), 0, sizeof(int), ctx->stream));
  // the Dirichlet lines' values (NULL: +0.0, which is all bits 0)
  if (n_values > 0 && dirichlet_value) {
    HIPC(hipMemcpyAsync(c.line_inhom.get() + H, dirichlet_value, sizeof(double) * (size_t)n_values, hipMemcpyHostToDevice, ctx->stream));
    for (int64_t i = 0; i < n_values; ++i) c.any_inhom = c.any_inhom || dirichlet_value[i] != 0.0;  // (a hanging line's sum is 0 unless one of these is not)
  } else if (n_values > 0) {
    HIPC(hipMemsetAsync(c.line_inhom.get() + H, 0, sizeof(double) * (size_t)n_values, ctx->stream));
  }
  ClArgs a{};
  a.cons = mt.constraint_of_dof.get(); a.line_ptr = mt.line_ptr.get(); a.line_master = mt.line_master.get(); a.line_weight = mt.line_weight.get();
  a.n_hanging = H; a.ptr = c.line_ptr.get(); a.inhom = c.line_inhom.get(); a.flag = d_flag.get();
  const dim3 g = asm_blocks(ctx, H, kClThreads);
  if (H) hipLaunchKernelGGL(cl_close_kernel<false>, g, dim3(kClThreads), 0, ctx->stream, a);
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, c.line_ptr.get(), L);
  int flag = 0;
  int32_t total = 0;
  HIPC(hipMemcpyAsync(&flag, d_flag.get(), sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&total, c.line_ptr.get() + L, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (flag & kClErrHanging) return bad(GMG_ERR_INVALID, "hanging node constrained to a hanging node");
  c.n_entries = total;
  for (int k = 0; k <= kClKeptMax; ++k)
    if (flag & (1 << (kClKeptShift + k))) c.max_line = k;
  if (c.max_line >= kClKeptMax) return bad(GMG_ERR_UNSUPPORTED, "a line with 16 or more entries");
  HIPC(c.line_master.alloc((size_t)std::max<int64_t>(c.n_entries, 1)));
  HIPC(c.line_weight.alloc((size_t)std::max<int64_t>(c.n_entries, 1)));
  a.master = c.line_master.get(); a.weight = c.line_weight.get();
  if (H) hipLaunchKernelGGL(cl_close_kernel<true>, g, dim3(kClThreads), 0, ctx->stream, a);
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  CHK(launch_status(ctx));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  c.valid = true;
  ctx->mesh.closed = std::move(c);
  if (ctx->debug_upload)
    std::fprintf(stderr, "[gmg] constraints closed on the device: %lld hanging + %lld Dirichlet lines, %lld of %lld entries kept, %.3f ms\n", (long long)H,
                 (long long)(L - H), (long long)total, (long long)mt.n_entries, ms);
  return GMG_OK;
}

int gmg_get_closed_constraints(gmg_context *ctx, int64_t *n_lines, int64_t *n_entries, int64_t *line_ptr, int32_t *line_master, double *line_weight,
                               double *line_inhomogeneity) {
  if (!ctx) return GMG_ERR_INVALID;
  const MeshTables &m = ctx->mesh;
  if (!m.valid || !m.closed.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_closed_constraints: the context holds no closed constraints");
  (void)hipSetDevice(ctx->device);
  if (n_lines) *n_lines = m.n_lines;
  if (n_entries) *n_entries = m.closed.n_entries;
  std::vector<int32_t> lp(line_ptr ? (size_t)m.n_lines + 1 : 0);
  HIPC(mesh_fetch(ctx, line_ptr ? lp.data() : nullptr, m.closed.line_ptr, m.n_lines + 1));
  HIPC(mesh_fetch(ctx, line_master, m.closed.line_master, m.closed.n_entries));
  HIPC(mesh_fetch(ctx, line_weight, m.closed.line_weight, m.closed.n_entries));
  HIPC(mesh_fetch(ctx, line_inhomogeneity, m.closed.line_inhom, m.n_lines));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < lp.size(); ++i) line_ptr[i] = lp[i];
  return GMG_OK;
}

// What the resident entries check instead of the siblings' host loops over the mesh arrays (the tables were produced by the
// library and are in range by construction): no communicator, tables, and (need_closed) their closed lines.  t receives the
// device pointers.
static int resident_tables(gmg_context *ctx, const char *who, bool need_closed, CellTablesDev &t) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator (rank-local assembly does not exist yet)");
  const MeshTables &m = ctx->mesh;
  if (!m.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  if (need_closed && !m.closed.valid) return bad(GMG_ERR_INVALID, "the context holds no closed constraints (gmg_close_constraints)");
  t.cell_dofs = m.cell_dofs.get(); t.cell_level = m.cell_level.get(); t.cons = m.constraint_of_dof.get();
  t.line_ptr = m.closed.line_ptr.get(); t.line_master = m.closed.line_master.get(); t.line_weight = m.closed.line_weight.get();
  t.line_inhom = m.closed.line_inhom.get(); t.max_line = m.closed.max_line;
  // (32-bit slot lists: every slot goes to its DoF and to at most max_line masters)
  if ((m.n_cells << m.dim) * (1 + (int64_t)t.max_line) >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 (row, slot) pairs");
  return GMG_OK;
}

static int assemble_system_resident(gmg_context *ctx, const char *who, const double *K_of_level, const AsmCoef *coef, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  if (coef) drop_system(ctx);  // (as the sibling: after any failure of the coefficient form the context holds no system matrix)
  CellTablesDev t;
  CHK(resident_tables(ctx, who, true, t));
  const MeshTables &m = ctx->mesh;
  if (m.n_cells > 0 && !coef && !K_of_level) return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": an array of nonzero length is NULL").c_str());
  if (coef) CHK(check_coef(ctx, who, *coef, m.n_cells));
  return assemble_system_device(ctx, who, m.dim, m.n_dofs, m.n_cells, t, K_of_level, coef, build_ms);
}

int gmg_assemble_system_matrix_resident(gmg_context *ctx, const double *K_of_level, double *build_ms) {
  return assemble_system_resident(ctx, "gmg_assemble_system_matrix_resident", K_of_level, nullptr, build_ms);
}

int gmg_assemble_system_matrix_coef_resident(gmg_context *ctx, int nq, const double *cell_coef, const double *G, const double *qw, const double *scale_of_level,
                                             double *build_ms) {
  const AsmCoef coef{nq, cell_coef, G, qw, scale_of_level, 16};
  return assemble_system_resident(ctx, "gmg_assemble_system_matrix_coef_resident", nullptr, &coef, build_ms);
}

int gmg_assemble_level_matrix_resident(gmg_context *ctx, int level, const double *K, double *build_ms) {
  return assemble_level(ctx, "gmg_assemble_level_matrix_resident", level, 0, 0, 0, nullptr, K, nullptr, nullptr, build_ms, true);
}

int gmg_assemble_level_matrix_coef_resident(gmg_context *ctx, int level, int nq, const double *cell_coef, const double *G, const double *qw, double scale,
                                            double *build_ms) {
  const AsmCoef coef{nq, cell_coef, G, qw, &scale, 1};
  return assemble_level(ctx, "gmg_assemble_level_matrix_coef_resident", level, 0, 0, 0, nullptr, nullptr, &coef, nullptr, build_ms, true);
}

int gmg_assemble_rhs_resident(gmg_context *ctx, const double *K_of_level, int nq, const double *shape, const double *weight, const double *jxw_of_level,
                              const double *source, double *rhs, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_assemble_rhs_resident";
  CellTablesDev t;
  CHK(resident_tables(ctx, who, true, t));
  const MeshTables &m = ctx->mesh;
  if (!shape || !weight || !jxw_of_level || (m.n_dofs > 0 && !rhs)) return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": an array of nonzero length is NULL").c_str());
  CHK(check_rhs_args(ctx, who, m.n_cells, m.closed.any_inhom, K_of_level, nq, source));
  return assemble_rhs_device(ctx, who, m.dim, m.n_dofs, m.n_cells, t, m.closed.any_inhom, K_of_level, nq, shape, weight, jxw_of_level, source, rhs, build_ms);
}

// (the closed lines never have a constrained master -- gmg_close_constraints drops or refuses every such entry -- so what
// gmg_distribute_constraints checks on the host, "no master is itself constrained", holds by construction)
int gmg_distribute_constraints_resident(gmg_context *ctx, int64_t n_dofs, double *u) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_distribute_constraints_resident";
  CellTablesDev t;
  CHK(resident_tables(ctx, who, true, t));
  if (n_dofs != ctx->mesh.n_dofs) return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": n_dofs differs from the mesh tables'").c_str());
  if (n_dofs > 0 && !u) return fail(ctx, GMG_ERR_INVALID, (std::string(who) + ": an array of nonzero length is NULL").c_str());
  if (n_dofs == 0) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  return distribute_device(ctx, who, n_dofs, u, t);
}

int gmg_get_level_matrix(gmg_context *ctx, int level, int which, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int64_t *rowptr, int32_t *col, double *val) {
  if (!ctx) return GMG_ERR_INVALID;
  if (level < 0 || level >= ctx->n_levels) return fail(ctx, GMG_ERR_INVALID, "gmg_get_level_matrix: level outside the context");
  if (which != GMG_LEVEL_A && which != GMG_LEVEL_EDGE && which != GMG_LEVEL_EDGE_T) return fail(ctx, GMG_ERR_INVALID, "gmg_get_level_matrix: which must be GMG_LEVEL_A, GMG_LEVEL_EDGE or GMG_LEVEL_EDGE_T");
  const Level &L = ctx->lv[(size_t)level];
  if (!L.A.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_level_matrix: level matrix not set");
  if (which != GMG_LEVEL_A && !L.has_I) {  // no interface matrix on this level
    if (n_rows) *n_rows = L.A.n_rows;
    if (n_cols) *n_cols = L.A.n_rows;
    if (nnz) *nnz = 0;
    if (rowptr) std::fill(rowptr, rowptr + L.A.n_rows + 1, (int64_t)0);
    return GMG_OK;
  }
  const DevCSR &m = which == GMG_LEVEL_A ? L.A : which == GMG_LEVEL_EDGE ? L.I : L.It;
  if (!m.rowptr.get() || !m.col.get() || !m.val.get()) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_get_level_matrix: no CSR copy of this operator on the device");
  if (n_rows) *n_rows = m.n_rows;
  if (n_cols) *n_cols = m.n_cols;
  if (nnz) *nnz = m.nnz;
  if (!rowptr) return GMG_OK;
  if (m.nnz && (!col || !val)) return fail(ctx, GMG_ERR_INVALID, "gmg_get_level_matrix: col / val are NULL");
  (void)hipSetDevice(ctx->device);
  std::vector<int32_t> rp((size_t)m.n_rows + 1);
  HIPC(hipMemcpyAsync(rp.data(), m.rowptr.get(), sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (m.nnz) {
    HIPC(hipMemcpyAsync(col, m.col.get(), sizeof(int32_t) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipMemcpyAsync(val, m.val.get(), sizeof(double) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < rp.size(); ++i) rowptr[i] = rp[i];
  return GMG_OK;
}

// ---- error estimator and refinement marks formed on the device (gmg_estimate.hpp) ----

// The two halves of the estimator's front (as section 22 split the assemblies).  estimate_check_args: what both entries check of
// the small arguments, before anything is launched.  estimate_device: the three kernels on cell and face tables that lie on the
// device, and the downloads.  keep (may be NULL) receives the marks and their number instead of leaving them to the call.
static int estimate_check_args(gmg_context *ctx, const char *who, int dim, int64_t n_cells, int64_t n_u, bool mesh_null, const double *h_of_level,
                               const double *face_measure_of_level, const double *diameter_of_level, int ng, const double *gauss_x, const double *gauss_w,
                               const double *u, int residual, int nq, const double *weight, const double *jxw_of_level, const double *dens, double fraction) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (dim != 2 && dim != 3) return bad(GMG_ERR_INVALID, "dim must be 2 or 3");
  if (n_cells < 0 || n_u < 0) return bad(GMG_ERR_INVALID, "negative size");
  if (ng < 1 || ng > kEstMaxGauss) return bad(GMG_ERR_INVALID, "ng must be in 1 .. 8");
  if (residual < 0 || residual > 2) return bad(GMG_ERR_INVALID, "residual must be 0, 1 or 2");
  if (residual && (nq < 1 || nq > 512)) return bad(GMG_ERR_INVALID, "nq must be in 1 .. 512");
  if (!std::isfinite(fraction) || fraction < 0.0) return bad(GMG_ERR_INVALID, "fraction must be finite and not negative");
  const int nfc = 1 << (dim - 1), nf = 2 * dim;
  if (!gauss_x || !gauss_w || !h_of_level || !face_measure_of_level || !diameter_of_level || (residual && (!weight || !jxw_of_level)) || mesh_null || (n_u > 0 && !u))
    return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_cells * nf * nfc >= ((int64_t)1 << 31) || n_cells * (residual ? nq : 1) >= ((int64_t)1 << 40)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 face entries");
  if (residual && !dens && n_cells > 0 && (!ctx->dens_dev.get() || ctx->dens_cells != n_cells || ctx->dens_nq != nq))
    return bad(GMG_ERR_INVALID, "no densities of this shape on the device (gmg_charge_density(..., dens = NULL))");
  return GMG_OK;
}

static int estimate_device(gmg_context *ctx, int dim, int64_t n_cells, const int32_t *d_cell_dofs, const uint8_t *d_cell_level, const uint8_t *d_face_kind,
                           const int32_t *d_face_cell, const double *h_of_level, const double *face_measure_of_level, const double *diameter_of_level, int ng,
                           const double *gauss_x, const double *gauss_w, const double *u, int residual, int nq, const double *weight,
                           const double *jxw_of_level, const double *dens, double fraction, float *eta, double *kelly_sq, double *residual_sq, double *face_int,
                           double *threshold, uint8_t *mark, int64_t *n_marked, double *build_ms, MeshTables::Marks *keep) {
  const int nv = 1 << dim, nfc = 1 << (dim - 1), nf = 2 * dim;
  if (n_cells == 0) {  // as the host: the maximum over nothing is 0
    if (threshold) *threshold = fraction * 0.0;
    if (n_marked) *n_marked = 0;
    if (build_ms) *build_ms = 0.0;
    if (keep) { keep->n_marked = 0; keep->valid = true; }
    return GMG_OK;
  }
  (void)hipSetDevice(ctx->device);
  const size_t nc = (size_t)n_cells;
  DevPtr<uint8_t> d_mark;
  DevPtr<double> d_dens, d_w, d_fi, d_k, d_r, d_thr;
  DevPtr<float> d_eta, d_part;
  DevPtr<unsigned long long> d_count;
  Event e0, e1;
  if (residual) {
    HIPC(upload(d_w, weight, (size_t)nq, ctx->stream));
    if (dens) HIPC(upload(d_dens, dens, nc * (size_t)nq, ctx->stream));
  }
  HIPC(d_fi.alloc(nc * nf));
  HIPC(d_k.alloc(nc));
  HIPC(d_r.alloc(nc));
  HIPC(d_eta.alloc(nc));
  HIPC(d_mark.alloc(nc));
  HIPC(d_thr.alloc(1));
  HIPC(d_count.alloc(1));
  const int cap = ctx->estimate_max_blocks;
  auto blocks = [&](int64_t n, int most) {
    int64_t g = std::max<int64_t>(1, std::min<int64_t>(most, (n + kEstThreads - 1) / kEstThreads));
    if (cap > 0) g = std::min<int64_t>(g, cap);
    return (unsigned)g;
  };
  const unsigned g_slots = blocks(n_cells * nf, 1 << 16), g_cells = blocks(n_cells, kEstMaxBlocks);
  HIPC(d_part.alloc(g_cells));
  EstArgs a{};
  a.dim = dim; a.nv = nv; a.nfc = nfc; a.nf = nf; a.ng = ng; a.nq = residual ? nq : 0; a.residual = residual; a.n_cells = n_cells;
  a.cell_dofs = d_cell_dofs; a.cell_level = d_cell_level; a.face_kind = d_face_kind; a.face_cell = d_face_cell; a.u = u;
  a.dens = !residual ? nullptr : dens ? d_dens.get() : ctx->dens_dev.get();
  a.weight = d_w.get();
  for (int l = 0; l < 16; ++l) {
    a.h[l] = h_of_level[l]; a.measure[l] = face_measure_of_level[l]; a.diameter[l] = diameter_of_level[l];
    a.jxw[l] = residual ? jxw_of_level[l] : 0.0;
  }
  for (int q = 0; q < ng; ++q) { a.gx[q] = gauss_x[q]; a.gw[q] = gauss_w[q]; }
  a.fraction = fraction;
  a.face_int = d_fi.get(); a.kelly_sq = d_k.get(); a.residual_sq = d_r.get(); a.eta = d_eta.get(); a.partial = d_part.get();
  a.n_partial = (int)g_cells; a.threshold = d_thr.get(); a.mark = d_mark.get(); a.n_marked = d_count.get();
  HIPC(e0.create());
  HIPC(e1.create());
  HIPC(hipEventRecord(e0.get(), ctx->stream));
  HIPC(hipMemsetAsync(d_count.get(), 0, sizeof(unsigned long long), ctx->stream));
  if (dim == 2) hipLaunchKernelGGL(est_face_kernel<2>, dim3(g_slots), dim3(kEstThreads), 0, ctx->stream, a);
  else hipLaunchKernelGGL(est_face_kernel<3>, dim3(g_slots), dim3(kEstThreads), 0, ctx->stream, a);
  hipLaunchKernelGGL(est_cell_kernel, dim3(g_cells), dim3(kEstThreads), 0, ctx->stream, a);
  hipLaunchKernelGGL(est_mark_kernel, dim3(g_cells), dim3(kEstThreads), 0, ctx->stream, a);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e1.get(), ctx->stream));
  double thr = 0.0;
  unsigned long long count = 0;
  if (eta) HIPC(hipMemcpyAsync(eta, d_eta.get(), sizeof(float) * nc, hipMemcpyDeviceToHost, ctx->stream));
  if (kelly_sq) HIPC(hipMemcpyAsync(kelly_sq, d_k.get(), sizeof(double) * nc, hipMemcpyDeviceToHost, ctx->stream));
  if (residual_sq) HIPC(hipMemcpyAsync(residual_sq, d_r.get(), sizeof(double) * nc, hipMemcpyDeviceToHost, ctx->stream));
  if (face_int) HIPC(hipMemcpyAsync(face_int, d_fi.get(), sizeof(double) * nc * nf, hipMemcpyDeviceToHost, ctx->stream));
  if (mark) HIPC(hipMemcpyAsync(mark, d_mark.get(), nc, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&thr, d_thr.get(), sizeof thr, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(&count, d_count.get(), sizeof count, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  if (threshold) *threshold = thr;
  if (n_marked) *n_marked = (int64_t)count;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) ms = 0.f;
  if (build_ms) *build_ms = ms;
  if (keep) { keep->mark = std::move(d_mark); keep->n_marked = (int64_t)count; keep->valid = true; }  // (the caller installs them on GMG_OK alone)
  RETURN_LAUNCHED(ctx);
}

int gmg_estimate_error(gmg_context *ctx, int dim, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level, const uint8_t *face_kind,
                       const int32_t *face_cell, const double *h_of_level, const double *face_measure_of_level, const double *diameter_of_level,
                       int ng, const double *gauss_x, const double *gauss_w, const double *u, int64_t n_u, int residual, int nq,
                       const double *weight, const double *jxw_of_level, const double *dens, double fraction, float *eta, double *kelly_sq,
                       double *residual_sq, double *face_int, double *threshold, uint8_t *mark, int64_t *n_marked, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_estimate_error";
  CHK(estimate_check_args(ctx, who, dim, n_cells, n_u, n_cells > 0 && (!cell_dofs || !cell_level || !face_kind || !face_cell), h_of_level, face_measure_of_level,
                          diameter_of_level, ng, gauss_x, gauss_w, u, residual, nq, weight, jxw_of_level, dens, fraction));
  const int nv = 1 << dim, nfc = 1 << (dim - 1), nf = 2 * dim;
  for (int64_t c = 0; c < n_cells; ++c)
    if (cell_level[c] > 15) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_error: cell level of 16 or more");
  for (int64_t s = 0; s < n_cells * nv; ++s)
    if (cell_dofs[s] < 0 || cell_dofs[s] >= n_u) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_error: DoF outside [0, n_u)");
  for (int64_t c = 0; c < n_cells; ++c)
    for (int f = 0; f < nf; ++f) {
      const int64_t slot = c * nf + f;
      const int kind = face_kind[slot], l = cell_level[c];
      const int32_t *fc = face_cell + slot * nfc;
      if (kind > 3) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_error: face kind above 3");
      const int n_idx = kind == 0 ? 0 : kind == 2 ? nfc : 1, want = kind == 1 ? l : kind == 2 ? l + 1 : l - 1;
      for (int k = 0; k < n_idx; ++k) {
        if (fc[k] < 0 || fc[k] >= n_cells) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_error: face_cell index outside [0, n_cells)");
        if ((int)cell_level[fc[k]] != want) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_error: the level of a face neighbour does not fit the kind of its face");
      }
      if (kind == 3 && (fc[1] < 0 || fc[1] >= nfc)) return fail(ctx, GMG_ERR_INVALID, "gmg_estimate_error: quadrant outside [0, 2^(dim-1))");
    }
  DevPtr<int32_t> d_cd, d_fc;
  DevPtr<uint8_t> d_lv, d_fk;
  if (n_cells > 0) {
    (void)hipSetDevice(ctx->device);
    const size_t nc = (size_t)n_cells;
    HIPC(upload(d_cd, cell_dofs, nc * nv, ctx->stream));
    HIPC(upload(d_lv, cell_level, nc, ctx->stream));
    HIPC(upload(d_fk, face_kind, nc * nf, ctx->stream));
    HIPC(upload(d_fc, face_cell, nc * nf * nfc, ctx->stream));
  }
  return estimate_device(ctx, dim, n_cells, d_cd.get(), d_lv.get(), d_fk.get(), d_fc.get(), h_of_level, face_measure_of_level, diameter_of_level, ng, gauss_x,
                         gauss_w, u, residual, nq, weight, jxw_of_level, dens, fraction, eta, kelly_sq, residual_sq, face_int, threshold, mark, n_marked,
                         build_ms, nullptr);
}

// gmg_estimate_error on the resident tables and the kept face table; the marks stay in the context
int gmg_estimate_error_resident(gmg_context *ctx, const double *h_of_level, const double *face_measure_of_level, const double *diameter_of_level, int ng,
                                const double *gauss_x, const double *gauss_w, const double *u, int64_t n_u, int residual, int nq, const double *weight,
                                const double *jxw_of_level, const double *dens, double fraction, float *eta, double *kelly_sq, double *residual_sq,
                                double *face_int, double *threshold, uint8_t *mark, int64_t *n_marked, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_estimate_error_resident";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  ctx->mesh.marks = MeshTables::Marks();  // after any failure the context holds no marks
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  MeshTables &m = ctx->mesh;
  if (!m.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  if (!m.faces.valid) return bad(GMG_ERR_INVALID, "the context holds no face table (gmg_build_face_table_resident)");
  if (n_u != m.n_dofs) return bad(GMG_ERR_INVALID, "n_u differs from the mesh tables' n_dofs");
  CHK(estimate_check_args(ctx, who, m.dim, m.n_cells, n_u, false, h_of_level, face_measure_of_level, diameter_of_level, ng, gauss_x, gauss_w, u, residual, nq, weight,
                          jxw_of_level, dens, fraction));
  MeshTables::Marks keep;
  CHK(estimate_device(ctx, m.dim, m.n_cells, m.cell_dofs.get(), m.cell_level.get(), m.faces.kind.get(), m.faces.cell.get(), h_of_level, face_measure_of_level,
                      diameter_of_level, ng, gauss_x, gauss_w, u, residual, nq, weight, jxw_of_level, dens, fraction, eta, kelly_sq, residual_sq, face_int,
                      threshold, mark, n_marked, build_ms, &keep));
  m.marks = std::move(keep);
  return GMG_OK;
}

int gmg_get_marks(gmg_context *ctx, int64_t *n_cells, uint8_t *mark, int64_t *n_marked) {
  if (!ctx) return GMG_ERR_INVALID;
  if (ctx->dist) return fail(ctx, GMG_ERR_UNSUPPORTED, "gmg_get_marks: not on a communicator");
  const MeshTables &m = ctx->mesh;
  if (!m.valid || !m.marks.valid) return fail(ctx, GMG_ERR_INVALID, "gmg_get_marks: the context holds no marks (gmg_estimate_error_resident)");
  (void)hipSetDevice(ctx->device);
  if (n_cells) *n_cells = m.n_cells;
  if (n_marked) *n_marked = m.marks.n_marked;
  HIPC(mesh_fetch(ctx, mark, m.marks.mark, m.n_cells));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

// ---- the patches of the graphical output (gmg_output.hpp) ----

// What both entries check of the small arguments, before anything is launched; then output_device: the kernel on cell tables
// that lie on the device, cut into launches of at most 2^output_chunk_log2 cells whose results are copied out one by one.
static int output_check_args(gmg_context *ctx, const char *who, int dim, int64_t n_cells, int64_t n_dofs, double h0, const double *u, int64_t n_u,
                             int n_fields, const double *const *dof_field) {
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (dim != 2 && dim != 3) return bad(GMG_ERR_INVALID, "dim must be 2 or 3");
  if (n_cells < 0 || n_dofs < 0 || n_u < 0) return bad(GMG_ERR_INVALID, "negative size");
  if (!(h0 > 0.0) || !std::isfinite(h0)) return bad(GMG_ERR_INVALID, "h0 must be positive");
  if (n_fields < 0 || n_fields > gmg_output::kMaxFields) return bad(GMG_ERR_INVALID, "n_fields must be in 0 .. 8");
  if (n_u != n_dofs) return bad(GMG_ERR_INVALID, "n_u differs from n_dofs");
  if (n_u > 0 && !u) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_fields > 0 && !dof_field) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  for (int j = 0; j < n_fields; ++j)
    if (n_dofs > 0 && !dof_field[j]) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  if (n_cells >= ((int64_t)1 << 31) >> dim || n_dofs >= ((int64_t)1 << 31)) return bad(GMG_ERR_UNSUPPORTED, "more than 2^31 DoFs or slots");
  return GMG_OK;
}

static int output_device(gmg_context *ctx, int dim, int64_t n_cells, int64_t n_dofs, const int32_t *d_cell_dofs, const uint8_t *d_cell_level,
                         const unsigned long long *d_vertex_of_dof, double origin, double h0, const double *u, int n_fields,
                         const double *const *dof_field, double *point, double *solution, double *grad_phi, double *const *patch_field, double *build_ms) {
  if (build_ms) *build_ms = 0.0;
  if (n_cells == 0) return GMG_OK;
  (void)hipSetDevice(ctx->device);
  const int nv = 1 << dim;
  const int64_t chunk = std::min<int64_t>(n_cells, (int64_t)1 << ctx->output_chunk_log2);
  const size_t cs = (size_t)chunk * (size_t)nv;  // slots of a launch: what the temporaries hold
  DevPtr<double> d_point, d_sol, d_grad, d_field[gmg_output::kMaxFields], d_out[gmg_output::kMaxFields];
  Event e0, e1;
  gmg_output::PatchArgs a{};
  a.cell_dofs = d_cell_dofs; a.cell_level = d_cell_level; a.vertex_of_dof = d_vertex_of_dof; a.u = u;
  a.origin = origin; a.h0 = h0; a.hf = h0 / 4096.0; a.n_fields = n_fields;
  if (point) { HIPC(d_point.alloc(3 * cs)); a.point = d_point.get(); }
  if (solution) { HIPC(d_sol.alloc(cs)); a.solution = d_sol.get(); }
  if (grad_phi) { HIPC(d_grad.alloc(3 * cs)); a.grad_phi = d_grad.get(); }
  for (int j = 0; j < n_fields; ++j) {
    if (!patch_field || !patch_field[j]) continue;  // (a field nobody asks for is not uploaded either)
    HIPC(upload(d_field[j], dof_field[j], (size_t)n_dofs, ctx->stream));
    HIPC(d_out[j].alloc(cs));
    a.dof_field[j] = d_field[j].get(); a.patch_field[j] = d_out[j].get();
  }
  HIPC(e0.create());
  HIPC(e1.create());
  double total_ms = 0.0;
  for (int64_t c0 = 0; c0 < n_cells; c0 += chunk) {
    const int64_t c1 = std::min(n_cells, c0 + chunk);
    const size_t ns = (size_t)(c1 - c0) * (size_t)nv, s0 = (size_t)c0 * (size_t)nv;
    a.c0 = c0; a.c1 = c1;
    const dim3 grid = asm_blocks(ctx, (int64_t)ns, gmg_output::kPatchThreads);
    HIPC(hipEventRecord(e0.get(), ctx->stream));
    if (dim == 2) hipLaunchKernelGGL(gmg_output::patch_kernel<2>, grid, dim3(gmg_output::kPatchThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL(gmg_output::patch_kernel<3>, grid, dim3(gmg_output::kPatchThreads), 0, ctx->stream, a);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(e1.get(), ctx->stream));
    if (point) HIPC(hipMemcpyAsync(point + 3 * s0, d_point.get(), sizeof(double) * 3 * ns, hipMemcpyDeviceToHost, ctx->stream));
    if (solution) HIPC(hipMemcpyAsync(solution + s0, d_sol.get(), sizeof(double) * ns, hipMemcpyDeviceToHost, ctx->stream));
    if (grad_phi) HIPC(hipMemcpyAsync(grad_phi + 3 * s0, d_grad.get(), sizeof(double) * 3 * ns, hipMemcpyDeviceToHost, ctx->stream));
    for (int j = 0; j < n_fields; ++j)
      if (a.patch_field[j]) HIPC(hipMemcpyAsync(patch_field[j] + s0, d_out[j].get(), sizeof(double) * ns, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));  // (the temporaries are the next launch's)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0.get(), e1.get()) == hipSuccess) total_ms += ms;
  }
  if (build_ms) *build_ms = total_ms;
  RETURN_LAUNCHED(ctx);
}

int gmg_output_patches(gmg_context *ctx, int dim, int64_t n_cells, const int32_t *cell_dofs, const uint8_t *cell_level, const uint64_t *vertex_of_dof,
                       int64_t n_dofs, double origin, double h0, const double *u, int64_t n_u, int n_fields, const double *const *dof_field, double *point,
                       double *solution, double *grad_phi, double *const *patch_field, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_output_patches";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  CHK(output_check_args(ctx, who, dim, n_cells, n_dofs, h0, u, n_u, n_fields, dof_field));
  if (n_cells > 0 && (!cell_dofs || !cell_level || !vertex_of_dof)) return bad(GMG_ERR_INVALID, "an array of nonzero length is NULL");
  const int nv = 1 << dim;
  for (int64_t c = 0; c < n_cells; ++c)
    if (cell_level[c] > gmg_output::kMaxLevel) return bad(GMG_ERR_INVALID, "cell level above 13");
  for (int64_t s = 0; s < n_cells * nv; ++s)
    if (cell_dofs[s] < 0 || cell_dofs[s] >= n_dofs) return bad(GMG_ERR_INVALID, "DoF outside [0, n_dofs)");
  DevPtr<int32_t> d_cd;
  DevPtr<uint8_t> d_lv;
  DevPtr<unsigned long long> d_vk;
  if (n_cells > 0) {
    (void)hipSetDevice(ctx->device);
    HIPC(upload(d_cd, cell_dofs, (size_t)n_cells * nv, ctx->stream));
    HIPC(upload(d_lv, cell_level, (size_t)n_cells, ctx->stream));
    HIPC(upload(d_vk, (const unsigned long long *)vertex_of_dof, (size_t)n_dofs, ctx->stream));
  }
  return output_device(ctx, dim, n_cells, n_dofs, d_cd.get(), d_lv.get(), d_vk.get(), origin, h0, u, n_fields, dof_field, point, solution, grad_phi,
                       patch_field, build_ms);
}

// gmg_output_patches on the resident tables: no mesh array crosses the bus
int gmg_output_patches_resident(gmg_context *ctx, double origin, double h0, const double *u, int64_t n_u, int n_fields, const double *const *dof_field,
                                double *point, double *solution, double *grad_phi, double *const *patch_field, double *build_ms) {
  if (!ctx) return GMG_ERR_INVALID;
  const char *who = "gmg_output_patches_resident";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  if (ctx->dist) return bad(GMG_ERR_UNSUPPORTED, "not on a communicator");
  const MeshTables &m = ctx->mesh;
  if (!m.valid) return bad(GMG_ERR_INVALID, "the context holds no mesh tables (gmg_build_mesh_tables)");
  CHK(output_check_args(ctx, who, m.dim, m.n_cells, m.n_dofs, h0, u, n_u, n_fields, dof_field));
  return output_device(ctx, m.dim, m.n_cells, m.n_dofs, m.cell_dofs.get(), m.cell_level.get(), m.vertex_of_dof.get(), origin, h0, u, n_fields, dof_field,
                       point, solution, grad_phi, patch_field, build_ms);
}

// gmg_energy_norm_error on the resident cell_dofs and on the geometry dr_geometry_kernel forms (DESIGN.md sections 23, 24)
int gmg_energy_norm_error_resident(gmg_context *ctx, double origin, double h0, const double *u, int64_t n_u, int64_t n_atoms, const double *atom_xyz,
                                   const double *atom_q, double r_c, int nq, const double *quadrature_points, const double *weights,
                                   const double *shape_grad, double *error, double *cell_err2) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  const char *who = "gmg_energy_norm_error_resident";
  auto bad = [&](int code, const char *msg) { return fail(ctx, code, (std::string(who) + ": " + msg).c_str()); };
  CHK(density_resident_tables(ctx, who, h0));  // no communicator, 3D tables, h0 > 0
  const MeshTables &m = ctx->mesh;
  const int64_t n_cells = m.n_cells;
  if (n_u != m.n_dofs) return bad(GMG_ERR_INVALID, "n_u differs from the mesh tables' n_dofs");
  CHK(energy_error_check_args(ctx, who, n_cells, u, n_u, n_atoms, atom_xyz, atom_q, r_c, nq, quadrature_points, weights, shape_grad));
  if (n_cells == 0) {
    if (error) *error = 0.0;
    return GMG_OK;
  }
  DevPtr<double> d_lo, d_h;
  HIPC(d_lo.alloc(3 * (size_t)n_cells));
  HIPC(d_h.alloc((size_t)n_cells));
  DensityResArgs a{};
  a.cell_dofs = m.cell_dofs.get(); a.cell_level = m.cell_level.get(); a.vertex_of_dof = m.vertex_of_dof.get(); a.n_cells = n_cells;
  a.origin = origin; a.h0 = h0;
  a.cell_lo = d_lo.get(); a.cell_h = d_h.get(); a.root_lo = nullptr;
  hipLaunchKernelGGL(dr_geometry_kernel, asm_blocks(ctx, n_cells, kDrThreads), dim3(kDrThreads), 0, ctx->stream, a);
  HIPC(hipGetLastError());
  return energy_error_device(ctx, who, n_cells, d_lo.get(), d_h.get(), m.cell_dofs.get(), u, n_atoms, atom_xyz, atom_q, r_c, nq, quadrature_points, weights,
                             shape_grad, error, cell_err2);
}

// ---- distributed ----

int gmg_comm_unique_id(void *out_id) { return comm_unique_id(out_id) ? GMG_ERR_COMM : GMG_OK; }

int gmg_comm_init(gmg_context *ctx, int rank, int n_ranks, const void *id) {
  if (!ctx || rank < 0 || n_ranks < 1 || rank >= n_ranks) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  if (comm_init(ctx->comm, rank, n_ranks, id)) {
    ctx->err = ctx->comm.why[0] ? std::string(ctx->comm.why) : std::string("communicator start-up failed (ncclCommInitRank / peer mailbox mapping)");
    return GMG_ERR_COMM;
  }
  ctx->dist = true;
  return GMG_OK;
}

int gmg_comm_info(gmg_context *ctx, int64_t out[8]) {
  if (!ctx || !out) return GMG_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = ctx->dist ? ctx->comm.n_ranks : 1;
  out[1] = !ctx->dist ? 0 : (ctx->comm.peer ? 2 : 1);
  out[2] = ctx->comm.peer && ctx->comm.box_fine ? 1 : 0;
  out[3] = ctx->comm.peer ? ctx->comm.ring_fine : -1;
  out[4] = ctx->dist ? ctx->comm.n_devices : 1;
  out[5] = l0_partitioned(ctx) ? 1 : 0;
  return GMG_OK;
}

int gmg_comm_barrier(gmg_context *ctx) {
  if (!ctx) return GMG_ERR_INVALID;
  if (!ctx->dist) return GMG_OK;
  HIPC(hipStreamSynchronize(ctx->stream));
  if (comm_host_barrier(ctx->comm)) return fail(ctx, GMG_ERR_COMM, "host barrier: a rank did not arrive");
  return GMG_OK;
}

int gmg_set_global_sizes(gmg_context *ctx, int64_t n_system_global, int64_t n_level0_global) {
  if (!ctx || n_system_global < 0 || n_level0_global < 0) return GMG_ERR_INVALID;
  if (!ctx->dist) return fail(ctx, GMG_ERR_INVALID, "gmg_set_global_sizes: call gmg_comm_init first");
  ctx->sys_global = n_system_global;
  ctx->l0_global = n_level0_global;
  if (l0_partitioned(ctx) && ctx->coarse_solver == GMG_COARSE_DIRECT) {  // (the direct solver needs level 0 whole: back to the CG)
    HIPC(hipStreamSynchronize(ctx->stream));
    drop_coarse_direct(ctx);
  }
  return GMG_OK;
}

int gmg_partition_range(int64_t n_global, int rank, int n_ranks, int64_t *begin, int64_t *end) {
  if (n_global < 0 || n_ranks < 1 || rank < 0 || rank >= n_ranks || !begin || !end) return GMG_ERR_INVALID;
  part_range(n_global, rank, n_ranks, begin, end);
  return GMG_OK;
}

int gmg_vec_allgather(gmg_context *ctx, int64_t n_global, double *dst_full, const double *src_local) {
  if (!ctx || n_global < 0) return GMG_ERR_INVALID;
  if (!ctx->dist) {
    if (n_global) HIPC(hipMemcpyAsync(dst_full, src_local, sizeof(double) * (size_t)n_global, hipMemcpyDeviceToDevice, ctx->stream));
    return GMG_OK;
  }
  return allgather_full(ctx, dst_full, src_local, n_global);
}

int gmg_set_halo_plan(gmg_context *ctx, int which, int n_neighbors, const int32_t *neighbor_rank,
                      const int32_t *send_count, const int32_t *send_idx, const int32_t *recv_count) {
  if (!ctx) return GMG_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  // `which`: GMG_SYSTEM, level l (A_l, I_l share it), 1000+l (P_l), 2000+l (P_l^T), 3000+l (I_l^T)
  std::vector<DevCSR *> targets;
  if (which == GMG_SYSTEM) targets = {&ctx->S};
  else if (which >= 0 && which < ctx->n_levels) targets = {&ctx->lv[(size_t)which].A, &ctx->lv[(size_t)which].I};
  else if (which >= 1000 && which < 1000 + ctx->n_levels) targets = {&ctx->lv[(size_t)which - 1000].P};
  else if (which >= 2000 && which < 2000 + ctx->n_levels) targets = {&ctx->lv[(size_t)which - 2000].Pt};
  else if (which >= 3000 && which < 3000 + ctx->n_levels) targets = {&ctx->lv[(size_t)which - 3000].It};
  else return fail(ctx, GMG_ERR_INVALID, "gmg_set_halo_plan: bad operator id");
  for (DevCSR *m : targets) {
    m->halo = HaloPlan();
    if (build_halo(m->halo, n_neighbors, neighbor_rank, send_count, send_idx, recv_count, ctx->stream))
      return fail(ctx, GMG_ERR_HIP, "halo plan upload failed");
  }
  return GMG_OK;
}

// ---- measurement ----

int gmg_stats_reset(gmg_context *ctx) {
  if (!ctx) return GMG_ERR_INVALID;
  collect_sgs_samples(ctx);
  const gmg_stats keep = ctx->stats;
  ctx->stats = gmg_stats{};
  ctx->stats.spmv0_rows = keep.spmv0_rows; ctx->stats.spmv0_nnz = keep.spmv0_nnz; ctx->stats.coarse_variant = keep.coarse_variant;
  ctx->stats.spmv0_layout = keep.spmv0_layout; ctx->stats.spmv0_matrix_bytes = keep.spmv0_matrix_bytes;
  ctx->stats.spmv0_pattern_slices = keep.spmv0_pattern_slices; ctx->stats.spmv0_slices = keep.spmv0_slices;
  ctx->stats.coarse_solver = keep.coarse_solver;
  return GMG_OK;
}
int gmg_stats_get(gmg_context *ctx, gmg_stats *out) {
  if (!ctx || !out) return GMG_ERR_INVALID;
  collect_sgs_samples(ctx);
  *out = ctx->stats;
  return GMG_OK;
}
int gmg_set_profiling(gmg_context *ctx, int sample_every) {
  if (!ctx || sample_every < 0) return GMG_ERR_INVALID;
  ctx->prof_every = sample_every;
  if (sample_every > 0 && ctx->ev_a.empty()) {
    for (auto *v : {&ctx->ev_a, &ctx->ev_b, &ctx->ev_c, &ctx->ev_d, &ctx->ev_e, &ctx->ev_f}) {
      v->resize(256);
      for (auto &e : *v) HIPC(e.create());
    }
  }
  return GMG_OK;
}
int gmg_calibrate_hbm(gmg_context *ctx, int64_t n_bytes, int reps, double *read_gbps, double *copy_gbps) {
  if (!ctx || n_bytes < (1 << 20) || reps < 1) return GMG_ERR_INVALID;
  const int64_t n2 = n_bytes / 16;
  DevPtr<double2> a_own, b_own;
  Event e0_own, e1_own;
  HIPC(a_own.alloc((size_t)n2));
  HIPC(b_own.alloc((size_t)n2));
  double2 *const a = a_own.get(), *const b = b_own.get();
  HIPC(hipMemsetAsync(a, 0, (size_t)n2 * 16, ctx->stream));
  HIPC(hipMemsetAsync(b, 0, (size_t)n2 * 16, ctx->stream));
  HIPC(e0_own.create());
  HIPC(e1_own.create());
  const hipEvent_t e0 = e0_own.get(), e1 = e1_own.get();
  float ms = 0.f;
  for (int pass = 0; pass < 2; ++pass) {  // pass 0 warms up
    HIPC(hipEventRecord(e0, ctx->stream));
    for (int r = 0; r < reps; ++r)
      hipLaunchKernelGGL(stream_read_kernel, dim3(kMaxPartials), dim3(kThreads), 0, ctx->stream, (const double2 *)a, n2, ctx->part_a.get());
    HIPC(hipEventRecord(e1, ctx->stream));
    HIPC(hipEventSynchronize(e1));
    HIPC(hipEventElapsedTime(&ms, e0, e1));
  }
  if (read_gbps) *read_gbps = (double)n2 * 16 * reps / (ms * 1e-3) / 1e9;
  for (int pass = 0; pass < 2; ++pass) {
    HIPC(hipEventRecord(e0, ctx->stream));
    for (int r = 0; r < reps; ++r)
      hipLaunchKernelGGL(stream_copy_kernel, dim3(kMaxPartials * 2), dim3(kThreads), 0, ctx->stream, (const double2 *)a, b, n2);
    HIPC(hipEventRecord(e1, ctx->stream));
    HIPC(hipEventSynchronize(e1));
    HIPC(hipEventElapsedTime(&ms, e0, e1));
  }
  if (copy_gbps) *copy_gbps = (double)n2 * 32 * reps / (ms * 1e-3) / 1e9;
  return GMG_OK;
}

int gmg_set_option(gmg_context *ctx, const char *key, double value) {
  if (!ctx || !key) return GMG_ERR_INVALID;
  const std::string k(key);
  const bool on = value != 0.0;
  if (k == "host_threads") g_host_threads = (int)value;
  else if (k == "debug_upload") ctx->debug_upload = on;
  else if (k == "disable_sell") ctx->disable_sell = on;
  else if (k == "disable_outer_cg_fused") ctx->disable_outer_cg_fused = on;
  else if (k == "disable_hybrid") ctx->disable_hybrid = on;
  else if (k == "hybrid_two_launches") ctx->hybrid_two_launches = on;
  else if (k == "disable_vcycle_fused") ctx->disable_vcycle_fused = on;
  else if (k == "disable_patterns") ctx->disable_patterns = on;
  else if (k == "disable_compression") ctx->disable_compression = on;
  else if (k == "disable_sellp") ctx->disable_sellp = on;
  else if (k == "disable_rowclass") ctx->disable_rowclass = on;
  else if (k == "disable_lattice") ctx->disable_lattice = on;
  else if (k == "lattice_segments") ctx->lattice_segments = (int)value;
  else if (k == "lattice_max_blocks") ctx->lattice_max_blocks = (int)value;
  else if (k == "sell_grid") ctx->sell_grid = (int)value;
  else if (k == "sellp_cost") ctx->sellp_cost = value;
  else if (k == "sellp_rr") ctx->sellp_rr = (int)value;
  else if (k == "cg_variant") ctx->cg_variant = (int)value;
  else if (k == "coarse_chunk") ctx->coarse_chunk = (int)value;
  else if (k == "coarse_direct") ctx->coarse_direct_opt = on;
  else if (k == "coarse_direct_max_blocks") {
    if (!(value >= 0 && value <= 65536) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "coarse_direct_max_blocks: an integer in 0 .. 65536");
    ctx->coarse_direct_max_blocks = (int)value;
  }
  else if (k == "ssor_balanced") ctx->ssor_partition = on ? GMG_SSOR_PARTITION_BALANCED : GMG_SSOR_PARTITION_ROWS;
  else if (k == "sgs_y_slots") ctx->sgs_y_slots = (int)value;
  else if (k == "sgs_sliding") ctx->sgs_sliding = on;
  else if (k == "sgs_pack") ctx->sgs_pack = value < 0 ? -1 : on ? 1 : 0;
  else if (k == "ssor_plan_device") ctx->ssor_plan_device = on;
  else if (k == "sgs_disable_wave") ctx->sgs_disable_wave = on;
  else if (k == "sgs_disable_phase") ctx->sgs_disable_phase = on;
  else if (k == "sgs_dep") ctx->sgs_dep = on;
  else if (k == "sgs_reg") ctx->sgs_reg = on;
  else if (k == "sgs_pf_lead_kb") ctx->sgs_pf_lead_kb = (int)value;
  else if (k == "sgs_chain") {
#ifndef GMG_EXPERIMENTS
    if (on) return fail(ctx, GMG_ERR_UNSUPPORTED, "sgs_chain needs a -DGMG_EXPERIMENTS build (tools/build_experiments.sh)");
#endif
    ctx->sgs_chain = on;
  }
  else if (k == "sgs_phase_profile") {
    if (on && ctx->dist && ctx->comm.n_ranks > 1) return fail(ctx, GMG_ERR_INVALID, "sgs_phase_profile: one rank only (the instrumented sweep is a single-GPU measurement)");
    ctx->sgs_phase_profile = (int)value;
  }
  else if (k == "sgs_phase_nosplit") ctx->sgs_phase_nosplit = on;
  else if (k == "sgs_phase_nocascade") ctx->sgs_phase_nocascade = on;
  else if (k == "sgs_phase_chunk") ctx->sgs_phase_chunk = (int)value;
  else if (k == "force_block") {
    if (value != 64 && value != 128 && value != 256) return fail(ctx, GMG_ERR_INVALID, "force_block: 64, 128 or 256");
    ctx->force_block = (int)value;
  }
  else if (k == "reset_keeps_mesh_tables") ctx->reset_keeps_mesh_tables = on;
  else if (k == "density_segment") {
    if (!(value >= 0 && value <= 2047) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "density_segment: an integer in 0 .. 2047");
    ctx->density_segment = (int)value;
  } else if (k == "assemble_max_blocks") {
    if (!(value >= 0 && value <= 65536) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "assemble_max_blocks: an integer in 0 .. 65536");
    ctx->assemble_max_blocks = (int)value;
  }
  else if (k == "estimate_max_blocks") {
    if (!(value >= 0 && value <= 65536) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "estimate_max_blocks: an integer in 0 .. 65536");
    ctx->estimate_max_blocks = (int)value;
  }
  else if (k == "exact_chunk_log2") {
    if (!(value >= 0 && value <= 35) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "exact_chunk_log2: an integer in 0 .. 35");
    ctx->exact_chunk_log2 = (int)value;
  }
  else if (k == "output_chunk_log2") {
    if (!(value >= 0 && value <= 30) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "output_chunk_log2: an integer in 0 .. 30");
    ctx->output_chunk_log2 = (int)value;
  }
  else if (k == "cheb_polynomial") {
    if (value != GMG_CHEB_FIRST_KIND && value != GMG_CHEB_FOURTH_KIND) return fail(ctx, GMG_ERR_INVALID, "cheb_polynomial: 0 (first kind) or 1 (fourth kind)");
    return gmg_set_chebyshev(ctx, (int)value, ctx->cheb_lmax_source, 0, 0.0);
  }
  else if (k == "cheb_lmax_source") {
    if (value != GMG_CHEB_LMAX_GERSHGORIN && value != GMG_CHEB_LMAX_LANCZOS) return fail(ctx, GMG_ERR_INVALID, "cheb_lmax_source: 0 (Gershgorin) or 1 (Lanczos)");
    return gmg_set_chebyshev(ctx, ctx->cheb_polynomial, (int)value, 0, 0.0);
  }
  else if (k == "cheb_lanczos_steps") {
    if (!(value >= 1 && value <= lanczos::kMaxSteps) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "cheb_lanczos_steps: an integer in 1 .. 64");
    return gmg_set_chebyshev(ctx, ctx->cheb_polynomial, ctx->cheb_lmax_source, (int)value, 0.0);
  }
  else if (k == "cheb_safety") {
    if (!(value >= 1.0)) return fail(ctx, GMG_ERR_INVALID, "cheb_safety: a factor >= 1");
    return gmg_set_chebyshev(ctx, ctx->cheb_polynomial, ctx->cheb_lmax_source, 0, value);
  }
  else if (k == "cheb_degree") {
    if (!(value >= 0 && value <= 64) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "cheb_degree: an integer in 0 .. 64 (0: the degree of gmg_set_smoother)");
    ctx->cheb_degree_opt = (int)value;
  }
  else if (k == "lanczos_max_blocks") {
    if (!(value >= 0 && value <= 65536) || value != (double)(int)value) return fail(ctx, GMG_ERR_INVALID, "lanczos_max_blocks: an integer in 0 .. 65536");
    ctx->lanczos_max_blocks = (int)value;
  }
  else if (k == "sgs_groups") ctx->sgs_groups = (int)value;
  else if (k == "sgs_lds_bytes_override") ctx->sgs_lds_bytes_override = (int)value;
  else if (k == "sgs_profile") {
    if (on && ctx->dist && ctx->comm.n_ranks > 1) return fail(ctx, GMG_ERR_INVALID, "sgs_profile: one rank only");
    ctx->sgs_profile = on;
    ctx->sgs_profile_mode = (int)value - 1;
#ifndef GMG_EXPERIMENTS
    // the timing modes that skip work (and give wrong results) are not in this library: tools/build_experiments.sh
    if (ctx->sgs_profile_mode > 0) return fail(ctx, GMG_ERR_UNSUPPORTED, "sgs_profile modes > 1 need a -DGMG_EXPERIMENTS build (tools/build_experiments.sh)");
#endif
  }
  else return fail(ctx, GMG_ERR_INVALID, "gmg_set_option: unknown key");
  return GMG_OK;
}

int gmg_set_tuning(gmg_context *ctx, int coarse_chunk, int cg_variant) {
  if (!ctx || coarse_chunk < 0 || cg_variant < 0 || cg_variant > 2) return GMG_ERR_INVALID;
  ctx->coarse_chunk = coarse_chunk;
  ctx->cg_variant = cg_variant;
  return GMG_OK;
}

int gmg_set_ssor_blocks(gmg_context *ctx, int n_blocks) {
  if (!ctx || n_blocks < 1) return GMG_ERR_INVALID;
  ctx->ssor_blocks = n_blocks;
  return GMG_OK;
}

int gmg_set_ssor_block_rows(gmg_context *ctx, int level, int n_blocks, const int64_t *block_row) {
  if (!ctx) return GMG_ERR_INVALID;
  if (level < 1 || level >= ctx->n_levels) return fail(ctx, GMG_ERR_INVALID, "gmg_set_ssor_block_rows: levels 1 .. n_levels - 1 (level 0 is the coarse CG)");
  if (n_blocks < 0 || (n_blocks > 0 && !block_row)) return fail(ctx, GMG_ERR_INVALID, "gmg_set_ssor_block_rows: n_blocks >= 0 boundaries expected");
  if (n_blocks == 0) {
    ctx->ssor_block_rows.erase(level);
    return GMG_OK;
  }
  if (block_row[0] != 0) return fail(ctx, GMG_ERR_INVALID, "gmg_set_ssor_block_rows: the first boundary must be 0");
  for (int b = 0; b < n_blocks; ++b)
    if (block_row[b + 1] < block_row[b]) return fail(ctx, GMG_ERR_INVALID, "gmg_set_ssor_block_rows: boundaries must not decrease");
  if (block_row[n_blocks] > INT32_MAX) return fail(ctx, GMG_ERR_INVALID, "gmg_set_ssor_block_rows: rows beyond the 32-bit range");
  ctx->ssor_block_rows[level].assign(block_row, block_row + n_blocks + 1);
  return GMG_OK;
}

int gmg_set_ssor_partition(gmg_context *ctx, int kind) {
  if (!ctx) return GMG_ERR_INVALID;
  if (kind != GMG_SSOR_PARTITION_ROWS && kind != GMG_SSOR_PARTITION_BALANCED) return fail(ctx, GMG_ERR_INVALID, "gmg_set_ssor_partition: unknown kind");
  ctx->ssor_partition = kind;
  return GMG_OK;
}

int gmg_get_ssor_partition(gmg_context *ctx, int level, int *n_blocks, int64_t *block_row, int64_t *block_steps) {
  if (!ctx || !n_blocks || level < 1 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const SgsPlan &G = ctx->lv[(size_t)level].sgs;
  if (G.host_block_row.empty()) return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_partition: the level matrix has not been set");
  *n_blocks = (int)G.host_block_row.size() - 1;
  if (block_row) std::copy(G.host_block_row.begin(), G.host_block_row.end(), block_row);
  if (block_steps) std::copy(G.host_block_steps.begin(), G.host_block_steps.end(), block_steps);
  return GMG_OK;
}

int gmg_ssor_balance_rows(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int n_blocks, int64_t *block_row,
                          double *block_cost) {
  if (n < 0 || n > INT32_MAX || n_blocks < 1 || !block_row || (n > 0 && (!rowptr || !col)) || (n > 0 && rowptr[0] != 0)) return GMG_ERR_INVALID;
  for (int64_t i = 0; i < n; ++i) {
    if (rowptr[i + 1] < rowptr[i]) return GMG_ERR_INVALID;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      if (col[k] < 0 || col[k] >= n) return GMG_ERR_INVALID;
  }
  std::vector<int64_t> br;
  std::vector<double> cost;
  if (n == 0) {
    br.assign((size_t)n_blocks + 1, 0);
    cost.assign((size_t)n_blocks, 0.0);
  } else {
    ssor_balance(SsorPattern(n, rowptr, col, val), n_blocks, br, cost);
  }
  std::copy(br.begin(), br.end(), block_row);
  if (block_cost) std::copy(cost.begin(), cost.end(), block_cost);
  return GMG_OK;
}

int gmg_get_ssor_plan(gmg_context *ctx, int level, int64_t out[8]) {
  if (!ctx || !out || level < 1 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const SgsPlan &G = ctx->lv[(size_t)level].sgs;
  if (G.host_block_row.empty()) return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_plan: the level matrix has not been set");
  std::fill(out, out + 8, (int64_t)0);
  if (!G.wave) return GMG_OK;  // the generic CSR sweep has no plan
  out[0] = G.w_n_ranges - G.n_bwd; out[1] = G.n_bwd; out[2] = G.n_self; out[3] = G.w_y_slots;
  out[4] = G.live_max[0]; out[5] = G.live_max[1]; out[6] = G.w_steps; out[7] = G.w_stream_bytes;
  return GMG_OK;
}

int gmg_get_ssor_schedule(gmg_context *ctx, int level, int64_t out[4]) {
  if (!ctx || !out || level < 1 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const SgsPlan &G = ctx->lv[(size_t)level].sgs;
  if (G.host_block_row.empty()) return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_schedule: the level matrix has not been set");
  std::fill(out, out + 4, (int64_t)0);
  if (!G.wave) return GMG_OK;  // the generic CSR sweep has no plan
  out[0] = G.n_packed > 0 ? 1 : 0; out[1] = G.w_stages; out[2] = G.w_fwd_steps; out[3] = G.w_stage_steps;
  return GMG_OK;
}

int gmg_get_ssor_backward_rows(gmg_context *ctx, int level, int64_t *count, int32_t *rows) {
  if (!ctx || !count || level < 1 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const SgsPlan &G = ctx->lv[(size_t)level].sgs;
  if (G.host_block_row.empty()) return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_backward_rows: the level matrix has not been set");
  *count = G.wave ? (int64_t)G.host_bwd_rows.size() : 0;
  if (rows && G.wave) std::copy(G.host_bwd_rows.begin(), G.host_bwd_rows.end(), rows);
  return GMG_OK;
}

int gmg_get_ssor_plan_array(gmg_context *ctx, int level, int which, int64_t *bytes, void *out) {
  if (!ctx || !bytes || level < 1 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const Level &L = ctx->lv[(size_t)level];
  const SgsPlan &G = L.sgs;
  if (G.host_block_row.empty() || !G.wave || !G.phased) return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_plan_array: the level has no four-wave plan");
  const void *src = nullptr;
  int64_t len = 0;
  switch (which) {
    case GMG_SSOR_PLAN_STREAM: src = G.w_stream.get(); len = G.w_stream_bytes; break;
    case GMG_SSOR_PLAN_RANGES: src = G.p_ranges.get(); len = (int64_t)sizeof(PhRange) * G.w_n_ranges; break;
    case GMG_SSOR_PLAN_BLK_TAB: src = G.p_blk_tab.get(); len = 16 * G.w_steps; break;
    case GMG_SSOR_PLAN_BLOCK_RNG: src = G.w_block_rng.get(); len = 4 * (int64_t)G.host_block_row.size(); break;
    case GMG_SSOR_PLAN_ROW_CI: src = G.w_row_ci.get(); len = 4 * L.n; break;
    case GMG_SSOR_PLAN_CI_ROW: src = G.w_ci_row.get(); len = 4 * G.w_n_coupled; break;
    case GMG_SSOR_PLAN_RPOS_F: src = G.w_rpos_f.get(); len = 4 * G.w_n_coupled; break;
    case GMG_SSOR_PLAN_RPOS_B: src = G.w_rpos_b.get(); len = 4 * G.w_n_coupled; break;
    case GMG_SSOR_PLAN_ISO_DIAG: src = G.w_iso_diag.get(); len = 8 * L.n; break;
    case GMG_SSOR_PLAN_ISO_INVD: src = G.w_iso_invd.get(); len = 8 * L.n; break;
    default: return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_plan_array: unknown array");
  }
  if (!out) { *bytes = len; return GMG_OK; }
  if (*bytes < len) return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_plan_array: the buffer is too small");
  *bytes = len;
  (void)hipSetDevice(ctx->device);
  if (len) HIPC(hipMemcpyAsync(out, src, (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return GMG_OK;
}

int gmg_get_ssor_plan_origin(gmg_context *ctx, int level, int *on_device, int64_t *csr_bytes_downloaded, const char **reason) {
  if (!ctx || level < 1 || level >= ctx->n_levels) return GMG_ERR_INVALID;
  const SgsPlan &G = ctx->lv[(size_t)level].sgs;
  if (G.host_block_row.empty()) return fail(ctx, GMG_ERR_INVALID, "gmg_get_ssor_plan_origin: the level matrix has not been set");
  if (on_device) *on_device = G.on_device ? 1 : 0;
  if (csr_bytes_downloaded) *csr_bytes_downloaded = G.csr_bytes_down;
  if (reason) *reason = G.host_reason;
  return GMG_OK;
}

int gmg_ssor_slot_plan(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t row_begin, int64_t row_end, int backward,
                       int32_t *step, int32_t *last_reader, int32_t *slot, int64_t *n_steps, int64_t *n_slots) {
  if (n < 0 || n > INT32_MAX || row_begin < 0 || row_end < row_begin || row_end > n || (n > 0 && (!rowptr || !col || !val)) || (n > 0 && rowptr[0] != 0)) return GMG_ERR_INVALID;
  for (int64_t i = 0; i < n; ++i) {
    if (rowptr[i + 1] < rowptr[i]) return GMG_ERR_INVALID;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      if (col[k] < 0 || col[k] >= n) return GMG_ERR_INVALID;
  }
  const int m = (int)(row_end - row_begin), dir = backward ? 1 : 0;
  SsorBlockGraph B;
  SsorSlotPlan S;
  std::vector<int32_t> seq;
  std::vector<SsorStep> steps;
  if (m > 0) {
    if (!ssor_block_graph(row_begin, row_end, rowptr, col, val, B)) return GMG_ERR_INVALID;  // (ascending columns expected)
    ssor_build_steps(dir, B.n_stages, B.sptr, B.by_stage, B.prp, B.pcol, kPhMaxRows, true, 0, kPhYSlots, seq, steps);
    ssor_slot_alloc(m, B.prp, B.pcol, dir, seq, steps, S);
  }
  if (step) std::copy(S.step.begin(), S.step.end(), step);
  if (last_reader) std::copy(S.last.begin(), S.last.end(), last_reader);
  if (slot) std::copy(S.slot.begin(), S.slot.end(), slot);
  if (n_steps) *n_steps = (int64_t)steps.size();
  if (n_slots) *n_slots = S.n_slots;
  return GMG_OK;
}

// a host CSR and a block of its rows as the two routines below take them: sizes, row pointers, columns in range
static bool ssor_host_csr_ok(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t row_begin, int64_t row_end) {
  if (n < 0 || n > INT32_MAX || row_begin < 0 || row_end < row_begin || row_end > n || (n > 0 && (!rowptr || !col || !val)) || (n > 0 && rowptr[0] != 0)) return false;
  for (int64_t i = 0; i < n; ++i) {
    if (rowptr[i + 1] < rowptr[i]) return false;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      if (col[k] < 0 || col[k] >= n) return false;
  }
  return true;
}

int gmg_ssor_pack_levels(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t row_begin, int64_t row_end, int32_t *level,
                         int64_t *n_levels, int64_t *n_stage_steps) {
  if (!ssor_host_csr_ok(n, rowptr, col, val, row_begin, row_end)) return GMG_ERR_INVALID;
  SsorBlockGraph B;
  SsorLevels Lv;
  if (row_end > row_begin) {
    if (!ssor_block_graph(row_begin, row_end, rowptr, col, val, B)) return GMG_ERR_INVALID;  // (ascending columns expected)
    ssor_pack_levels(B, Lv);
    for (size_t i = 0; i < Lv.level.size(); ++i)
      if (!B.coupled[i]) Lv.level[i] = -1;  // a row without couplings has no level
  }
  if (level) std::copy(Lv.level.begin(), Lv.level.end(), level);
  if (n_levels) *n_levels = Lv.n_levels;
  if (n_stage_steps) *n_stage_steps = Lv.stage_steps;
  return GMG_OK;
}

int gmg_ssor_slot_plan_packed(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int64_t row_begin, int64_t row_end, int backward,
                              int32_t *step, int32_t *last_reader, int32_t *slot, int64_t *n_steps, int64_t *n_slots) {
  if (!ssor_host_csr_ok(n, rowptr, col, val, row_begin, row_end)) return GMG_ERR_INVALID;
  const int m = (int)(row_end - row_begin), dir = backward ? 1 : 0;
  SsorBlockGraph B;
  SsorLevels Lv;
  SsorSlotPlan S;
  std::vector<int32_t> seq;
  std::vector<SsorStep> steps;
  if (m > 0) {
    if (!ssor_block_graph(row_begin, row_end, rowptr, col, val, B)) return GMG_ERR_INVALID;  // (ascending columns expected)
    ssor_pack_levels(B, Lv);
    ssor_build_steps(dir, Lv.n_levels, Lv.sptr, Lv.by_level, B.prp, B.pcol, kPhMaxRows, true, 0, kPhYSlots, seq, steps);
    ssor_slot_alloc(m, B.prp, B.pcol, dir, seq, steps, S);
  }
  if (step) std::copy(S.step.begin(), S.step.end(), step);
  if (last_reader) std::copy(S.last.begin(), S.last.end(), last_reader);
  if (slot) std::copy(S.slot.begin(), S.slot.end(), slot);
  if (n_steps) *n_steps = (int64_t)steps.size();
  if (n_slots) *n_slots = S.n_slots;
  return GMG_OK;
}

}  // extern "C"
