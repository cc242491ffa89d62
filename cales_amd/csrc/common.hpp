// Internal definitions shared by the HIP translation units of libcales_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/cales.h"
#include "lmf_pack.hpp"

// The working precision rp of the reference (src/precision.f90:11-20): FP64, or FP32 when the library is built with -DCALES_SINGLE
// (the reference's -D_SINGLE_PRECISION; libcales_hip_sp.so). `real` is cales_real of include/cales.h.
typedef cales_real real;
#ifdef CALES_SINGLE
typedef float2 real2;
#define CALES_EPS 1.1920929e-07f            /* epsilon(1._rp), reference src/param.f90:20 */
#define CALES_BIG 3.4028235e38f             /* huge(1._rp), src/param.f90:25 */
#else
typedef double2 real2;
#define CALES_EPS 2.220446049250313e-16     /* epsilon(1._rp), reference src/param.f90:20 */
#define CALES_BIG 1.7976931348623157e308    /* huge(1._rp), src/param.f90:25 */
#endif
constexpr int RSZ = (int)sizeof(real);          // bytes per element: the byte offsets of ldb/stb
constexpr int LINE_REALS = 128 / RSZ;           // elements per 128-B cache line (16 / 32): row pitch and field offset are laid out in lines
__host__ __device__ inline real2 make_real2(real x, real y) { real2 r; r.x = x; r.y = y; return r; }

struct Geom {              // passed by value to kernels
  int n1, n2, n3;          // local interior sizes
  int s1;                  // row pitch >= n1+3, a multiple of 16 doubles
  long s12;                // s1*(n2+2)
  int jlo;                 // global index offset of local row j=1 is jlo+1 (y-slab)
  int ng2;                 // global n2

  __host__ __device__ inline size_t ix(int i, int j, int k) const { return (size_t)i + (size_t)s1 * (size_t)j + (size_t)s12 * (size_t)k; }
};

struct DBound { real *x = nullptr, *y = nullptr, *z = nullptr; };
// Boundary term of an inhomogeneous z condition in the r.h.s. of a velocity Helmholtz solve (cmpt_rhs_b / bc_rhs, bound.f90:447-560, times alpha, main.f90:432):
// one side of one component; `at` evaluates it for column (i, j) with the operations of the reference in their order. Used by k_rhs_b_velz (the term as a
// pass of its own / as a plane) and by the in-LDS Helmholtz sweep, which adds it while it loads plane 1 / n.
struct RhsBz {
  const real *bc; char ctype, cf; real dlc, dlf, sgn, alpha;
  __host__ __device__ inline real at(int i, int j, int n1) const {
    const real bcv = bc[i + (size_t)(n1 + 2) * j];
    real r = 0.;
    if (cf == 'c') { if (ctype == 'D') r = -2. * bcv / dlc / dlf; else if (ctype == 'N') r = sgn * bcv / dlf; }
    else           { if (ctype == 'D') r = -bcv / dlc / dlf;      else if (ctype == 'N') r = sgn * bcv / dlc; }
    return r * alpha;
  }
};   // device BC planes (0:na+1,0:nb+1,0:1), reference src/typedef.f90:10-14

// Communication hooks (include/cales.h): y-slab neighbours, slab<->mode-block all-to-all, all-reduce.
struct Comm {
  cales_halo_cb halo = nullptr; cales_alltoall_cb a2a = nullptr; cales_allreduce_cb allred = nullptr; void *user = nullptr;
  real *A = nullptr, *B = nullptr; int64_t nbuf = 0;   // two device staging buffers owned by the host (doubles)
  bool on = false;
  cales_halo_s_cb halo_s = nullptr; cales_alltoall_part_cb a2a_part = nullptr;   // exchanges on the second stream (cales_set_comm_overlap)
  // What the registered hooks imply, fixed by comm_changed (api.hip) at the end of cales_set_comm / cales_set_comm_overlap and only read after: which
  // exchanges go on the second stream (its hook and the stream both exist), and which y neighbours this slab has (MPI_PROC_NULL at a non-periodic
  // end, src/initmpi.f90:201-204)
  bool halo_second_stream = false, a2a_second_stream = false, has_lo = false, has_hi = false;
};

// Where the spectral (after the x transform) data of the Poisson solve lives.
//  blocked = 0: in place in the haloed array: complex (m, j, k) at (ix(0,j,k)>>1) + m
//  blocked = 1: staging buffer laid out [peer][k][jl][mm] (complex), peer block = n3*n2l*cw:
//               on the slab side peer = m/cw, on the mode-block side peer = (j-1)/n2l.
struct Spec {
  int blocked, cw, n2l, n3;
  int nyq = 0;      // periodic x (periodic or Neumann y): the two REAL modes 0 and n1/2 of a row share complex slot 0 (re, im) and the row has n1/2 complex slots -- whole 128-B lines (k_solver.hip, "Nyquist packing")
  // slab side: global mode m, LOCAL row jl (1-based), plane k (1-based)
  __host__ __device__ inline size_t at_slab(const Geom &g, int m, int jl, int k) const {
    if (!blocked) return (g.ix(0, jl, k) >> 1) + (size_t)m;
    const int peer = m / cw, mm = m - peer * cw;
    return (size_t)mm + (size_t)cw * ((size_t)(jl - 1) + (size_t)n2l * ((size_t)(k - 1) + (size_t)n3 * peer));
  }
  // mode-block side: LOCAL mode mm, GLOBAL row j (1-based), plane k (1-based)
  __host__ __device__ inline size_t at_mode(const Geom &g, int mm, int j, int k) const {
    if (!blocked) return (g.ix(0, j, k) >> 1) + (size_t)mm;
    const int peer = (j - 1) / n2l, jl = (j - 1) - peer * n2l;
    return (size_t)mm + (size_t)cw * ((size_t)jl + (size_t)n2l * ((size_t)(k - 1) + (size_t)n3 * peer));
  }
};

// Run-time switches: read from the environment ONCE, by cales_create; the launch path only looks at these fields.
struct Flags {
  bool unfolded_correc = false, unfolded_mom = false, eager_projection = false, lazy_projection = false, helmholtz_z_per_column = false, unfused_imp_rhs = false, unfused_correc = false, unfused_forcing = false, unfused_fillps = false, unfused_mean = false, keep_last_rhs = false, wide_offsets = false, dsmag_reference_sequence = false, dsmag_xghosts = false, smag_reference_sequence = false, gaussel_march = false, fft_generic = false, fft_no_odd_radix = false, keep_null_mode = false, unfused_rk = false, overlap = false, xghosts_in_step = false, unmerged_bc = false, no_nyquist_packing = false, sgs_six_components = false, lmf_unpacked_remainder = false, lmf_main_bands = false, derived_points = false;
  int kchunk = 0; long tile_min_blocks = 2048;
  std::string test_bad_launch;      // CALES_TEST_BAD_LAUNCH: test hook of the launch check (LAUNCH below)
  void read_env() {
    test_bad_launch = getenv("CALES_TEST_BAD_LAUNCH") ? getenv("CALES_TEST_BAD_LAUNCH") : "";
    unfolded_mom = getenv("CALES_UNFOLDED_MOM") != nullptr;      // no subgrid model in cales_step: the projection as a pass of its own (k_correc_cell) in every substep instead of inside the next momentum pass
    lazy_projection = getenv("CALES_LAZY_PROJECTION") != nullptr;      // ... the third substep's projection left to the next step on grids of any size (default: one rank with 4M cells or more -- measured: 1024^3 166.0 -> 161.5 ms/step, 64^3 0.235 -> 0.242)
    eager_projection = getenv("CALES_EAGER_PROJECTION") != nullptr;      // ... folded, but the third substep's projection done before cales_step returns instead of by the next step's first momentum pass (or the first call that looks at the fields)
    unfolded_correc = getenv("CALES_UNFOLDED_CORREC") != nullptr;      // dynamic model in cales_step: the projection as a pass of its own (k_correc_cell) instead of inside the strain-rate pass
    helmholtz_z_per_column = getenv("CALES_HELMHOLTZ_Z_PER_COLUMN") != nullptr;
    unfused_imp_rhs = getenv("CALES_UNFUSED_IMP_RHS") != nullptr;
    unfused_correc = getenv("CALES_UNFUSED_CORREC") != nullptr;
    unfused_forcing = getenv("CALES_UNFUSED_FORCING") != nullptr;
    unfused_fillps = getenv("CALES_UNFUSED_FILLPS") != nullptr;
    unfused_mean = getenv("CALES_UNFUSED_MEAN") != nullptr;
    keep_last_rhs = getenv("CALES_KEEP_LAST_RHS") != nullptr;
    wide_offsets = getenv("CALES_WIDE_OFFSETS") != nullptr;
    dsmag_reference_sequence = getenv("CALES_DSMAG_REFERENCE_SEQUENCE") != nullptr;
    dsmag_xghosts = getenv("CALES_DSMAG_XGHOSTS") != nullptr;
    sgs_six_components = getenv("CALES_SGS_SIX_COMPONENTS") != nullptr;      // dynamic model in cales_step on one rank: all six |S|Sij travel between the strain-rate pass and the last pass (default: five, the third from the trace -- SgsPath::five)
    lmf_unpacked_remainder = getenv("CALES_LMF_UNPACKED_REMAINDER") != nullptr;      // dynamic model's last pass on one rank, pair fields: the remainder x tile as one more tile column of the one launch (default: packed into full waves, a launch of its own -- SgsPath::lmf_packed)
    lmf_main_bands = getenv("CALES_LMF_MAIN_BANDS") != nullptr;      // ... packed: the launch of the full tiles through the band map even where band_wanted says no (experiments)
    smag_reference_sequence = getenv("CALES_SMAG_REFERENCE_SEQUENCE") != nullptr;
    gaussel_march = getenv("CALES_GAUSSEL_MARCH") != nullptr;
    no_nyquist_packing = getenv("CALES_NO_NYQUIST_PACKING") != nullptr;      // periodic x, periodic or Neumann y: the real modes 0 and n1/2 in columns of their own (n1/2 + 1 mode columns) instead of sharing column 0
    fft_generic = getenv("CALES_FFT_GENERIC") != nullptr;
    fft_no_odd_radix = getenv("CALES_FFT_NO_ODD_RADIX") != nullptr;      // x / y lines of 3, 5, 9 times 2^p on the Stockham kernels instead of the radix-8 register kernels
    xghosts_in_step = getenv("CALES_XGHOSTS_IN_STEP") != nullptr;      // keep the x ghost columns up to date after every operator of cales_step
    keep_null_mode = getenv("CALES_KEEP_NULL_MODE") != nullptr;
    unfused_rk = getenv("CALES_UNFUSED_RK") != nullptr;
    // exchanges beside the kernels on a second stream: opt-in (CALES_OVERLAP=1) until a run with real peers has confirmed it -- the emulated
    // ranks of the tests cannot show a gain, and the in-order exchanges are the form with the fewest assumptions (CALES_NO_OVERLAP wins)
    overlap = getenv("CALES_OVERLAP") != nullptr && atoi(getenv("CALES_OVERLAP")) != 0 && getenv("CALES_NO_OVERLAP") == nullptr;
    unmerged_bc = getenv("CALES_UNMERGED_BC") != nullptr;
    derived_points = getenv("CALES_DERIVED_POINTS") != nullptr && atoi(getenv("CALES_DERIVED_POINTS")) != 0;      // derived fields (include/cales_derived.h): dense boxes too by the one-thread-per-point kernel instead of the LDS-tile form (k_derived.hip)
    kchunk = getenv("CALES_KCHUNK") ? atoi(getenv("CALES_KCHUNK")) : 0;
    tile_min_blocks = getenv("CALES_TILE_MIN_BLOCKS") ? atol(getenv("CALES_TILE_MIN_BLOCKS")) : 2048;
  }
};

// The path ONE cales_step takes through the fused / folded forms of its operators (reference sequence src/main.f90:417-508): decided once by
// make_plan (api.hip) from the case, the switches (Flags) and the few pieces of state listed under `in_*`, re-made only when one of those changes, and
// READ -- never re-derived -- by step_body. cales_describe_plan (include/cales.h) prints it: bench.py puts the string into its line (config.path), the
// golden tests assert it next to the profile counters.
struct StepPlan {
  bool valid = false;
  bool in_visct_zero = false, in_sgs_first = false;      // the state the plan was made from (a change of the hooks invalidates it: comm_changed)
  bool xskip = false;            // periodic x: the step's kernels wrap around, the x ghost columns are left alone until somebody else reads them
  bool fold_correc = false;      // dynamic model: projection + pressure update inside the strain-rate pass of the substep's cmpt_sgs (k_corr_strain_tile)
  bool fold_rows2 = false;       // ... on several slabs with TWO ghost rows of the prediction (three of pp): the pass also forms the ghost rows of everything it writes,
                                 // so no row of u, v, w, p, |S|, |S|Sij, the filtered velocity or v_c travels after it (27 field planes per step instead of 48)
  bool fold_mom = false;         // no subgrid model: projection of substeps 1, 2 (and 3: lazy_last) inside the NEXT momentum pass (k_momrk<CORR>)
  bool lazy_last = false;        // ... the third substep's projection stays pending across the return of cales_step (one rank only)
  bool defer_imp_rhs = false;    // z-implicit: the Helmholtz sweeps form their r.h.s. (implicit part of rk, forcing, boundary terms) while loading
  bool any_wm = false, skip_first_wm = false;   // wall model: the update between bulk_forcing and fillps is dead work (main.f90:492-501) and skipped
  bool fuse_cu = false;          // correc + updatep in one pass
  bool defer_force = false;      // bulk-forcing increment added by the correction pass (means summed by the forward x transform: mean_mask)
  bool fuse_fill = false;        // fillps inside the forward x transform of the pressure solve
  bool visct_ghosts = false;     // the eddy viscosity's ghost cells are updated after cmpt_sgs (not needed while the field is identically zero)
  bool keep_last_rhs = false;
  int mean_mask = 0, force_mask = 0;
};

// Block -> tile map of the plane-marching tile kernels (band_map below), and the launch geometry of a tile pass (grid: 1-D through bm where bm.gx != 0)
struct BandMap { int gx, gy, gz, sub; };
struct TileGeom { dim3 block, grid; int kchunk = 0; BandMap bm{0, 0, 0, 0}; };

// A kernel held by a path record: the instantiation a set-up function chose and its name AS THAT FUNCTION SPELLS IT -- what the launch check reports and the
// test hook matches (LAUNCH_REC below). KERNEL_REC(k_tile<unsigned, 0, 1>) fills one: variadic, so the commas of a template argument list survive.
template <typename Fn> struct KernelRec { Fn *fn = nullptr; const char *name = ""; };
#define KERNEL_REC(...) {__VA_ARGS__, #__VA_ARGS__}
// a tile pass: the kernel and its launch geometry (k.fn == nullptr: the path has no such pass)
template <typename Args> struct TilePass { KernelRec<void(Geom, Args)> k; TileGeom geo; };

// The path of cmpt_sgs (k_sgs.hip), decided once by cales_create (sgs_setup; sgs_setup_launches once the CU count is known) and only read after:
// op_cmpt_sgs launches it, sgs_path_name prints it, cales_create allocates its scratch fields, make_plan folds the projection only into pair fields.
enum class SgsForm { none, smag_rows, smag_reference, dsmag_tiles, dsmag_reference };
// the directions <Mij Lij>, <Mij Mij> of the dynamic model are averaged over (sgs.f90:359-370): _CHANNEL (hard-wired there) | -D_DIT | _DUCT | _CAVITY (none)
enum class SgsAve { planes, volume, xlines, local };
struct StrainTileArgs; struct LmfArgs;      // the kernels' arguments (k_sgs.hip)
struct SgsPath {
  SgsForm form = SgsForm::none;
  bool pair = false, lazy = false, ucf = false;      // |S|Sij as pair fields (ss2); lazy: |S| straight into visct (homogeneous sgs BCs); ucf: the last pass forms the cell-centred velocity
  // five: inside cales_step with the projection folded into the strain-rate pass on ONE rank, five |S|Sij travel (two pair fields and S12 plain) and the last
  // pass takes |S|S33 = -(|S|S11 + |S|S22): the trace of the strain rate of a velocity that pass has just projected is the divergence the solve left. Calls
  // without the fold (start-up, operator level, CALES_UNFOLDED_CORREC), slabs and every other form keep six (CALES_SGS_SIX_COMPONENTS: everywhere)
  bool five = false;
  bool filter2d = false;    // the reference's -D_FILTER_2D (cales_case.sgstype = CALES_SGS_DSMAG_FILTER2D): test filter in the x-y planes only, alph2 = 2.52 everywhere
  SgsAve ave = SgsAve::planes;      // cales_case.sgstype & CALES_SGS_AVE_*: volume folds the plane sums into one (k_volume_fold), xlines takes the sequence (k_contract_lines),
                                    // local (CALES_SGS_AVE_LOCAL) averages nothing: k_lmf_tile<.., LOCAL> / k_contract_local write visct cell by cell -- no lazy form, six components
  bool wraps_x = true;      // reads wrapped interior columns where x is periodic (cales_step may leave the x ghost columns stale)
  // static kernel arguments (y walls: dsmag those this rank owns, smag_rows those of the case -- global distances, the shear reaches every slab)
  int zlo = 0, zhi = 0, wmlo = 0, wmhi = 0, wylo = 0, wyhi = 0, wmylo = 0, wmyhi = 0; real flo = 0., fhi = 0.;
  int perz = 0, perx = 0, skipz = 0, lmf_ty = 0;
  // The passes: kernel records from sgs_setup -- the one place every instantiation is named, from the properties that select it (32- or 64-bit byte offsets,
  // walls or wall-model faces in y, ucf, pair fields, the plane filter, the averaging) --, geometries from sgs_setup_launches. What a call may choose between is
  // a separate entry, and the call only indexes: strain without the projection folded in, corr[rows2][five] with it (rows2: SgsFold::rows2, from two ghost rows
  // of the prediction; five components on one rank only, so corr[1][1] stays empty); lmf[five] the last pass and lmf_rem[five] its packed remainder pass. An
  // entry the path does not have stays empty (pair fields only: corr, lmf_rem; five only: the [1] entries).
  TilePass<StrainTileArgs> smag, strain, corr[2][2];
  TilePass<LmfArgs> lmf[2], lmf_rem[2];      // (lmf's geometry unbanded: the overlap of cmpt_sgs splits it per call)
  // lmf_packed (pair fields on one rank, lmf_pack(n1).on, not CALES_LMF_UNPACKED_REMAINDER): lmf covers the full x tiles only and lmf_rem, a launch of the
  // packed instantiation with a chunk length of its own, the remainder tile of every row (lmf_pack.hpp); lmf_gx: x tiles of a row, the remainder one
  // included -- the block sums of a plane keep the slots of the one launch
  bool lmf_packed = false; int lmf_gx = 0;
};
// op_cmpt_sgs inside cales_step: the projection folded into the strain-rate pass (StepPlan::fold_correc; rows2: fold_rows2; fmask: deferred forcing)
struct SgsFold { real dtrk; bool rows2; int fmask; };

// What the momentum + RK pass is (k_momrk.hip, op_rk_par), decided once by cales_create (mom_setup, once the CU count is known) and only read after. No field
// pointers here either: MomRkArgs is filled per call, and so is what a call decides (NOS from visct_zero, RD / WR from the substep, CORR from RkOpts::pending)
struct MomPath {
  bool fused = true;      // k_momrk; false (CALES_UNFUSED_RK): k_mom + k_rk_update
  int imp = 0;            // the IMP form of the kernels (impdiff)
  bool small = false;     // 32-bit byte offsets (ldb/stb)
  TileGeom geo;           // tiles of 64 x TYM
  // some face of the case has a wall model: the ghost layers of u, v, w travel to the second buffers with every operator-level call, inside cales_step
  // only where something reads them before the next bounduvw rewrites them (a wall model that samples the ghost cell itself; CALES_UNMERGED_BC)
  bool wm = false, wm_ghosts_in_step = false;
};
// A projection u = (u* + f) - dtrk grad(pp), p += pp that cales_step has left to the next momentum pass (StepPlan::fold_mom); due when dtrk != 0. fmask: the
// components whose bulk-forcing increment it adds. p_done: z-implicit diffusion, the pressure update ran as a pass of its own (its z Laplacian of pp cannot
// be formed in ghost cells), only the velocity is pending. xskip: the step that left it left the x ghost columns alone (step_xskip)
struct PendingProjection { real dtrk = 0.; int fmask = 0; bool p_done = false, xskip = false; };

// One direction of one field in the ghost-cell operators (k_bound.hip): the type of each end ('P' at both: periodic, one copy serves both; 'D'; 'N'; 0: this
// end is left alone), cen = 0: face-centred along this direction, and per end the spacing of the Neumann rule and the plane of boundary values. k_bc_all
// takes it as it stands.
struct BcRule { char t0, t1, cen; real dr0, dr1; const real *bc0, *bc1; };
// ... the three directions of one field. wm[d]: bit 0 / 1 -- the lower / upper end of direction d is a wall-model face of this rank and the field a
// tangential velocity component: bounduvw leaves that end to the update that follows the wall model
struct BcRules { BcRule d[3]; unsigned char wm[3]; };
enum class VelSet { state = 0, filtered = 1 };      // u, v, w with bcu/bcv/bcw | the dynamic model's filtered velocity uf, vf, wf with bcuf/bcvf/bcwf
// What the case fixes about the ghost-cell operators (k_bound.hip), worked out once by cales_create (bc_setup) from the BC types, is_bound, the wall-model
// faces, the grid and Flags, and only read after: the kernel form of every BC set and the rules of every (field kind, direction, end) as this rank applies
// them -- 'P' where the direction is periodic, 0 at an end the slab does not own and for a periodic y on several slabs (the rows are exchanged). The
// tables hold everything about the case and nothing about a call: no field pointers (the f / f2 swaps change them), and the plane pointers are stable
// (the wall model rewrites what the planes hold). What a call changes is bc_rule's business.
enum class BcForm { merged, all, by_direction };      // k_bc_merged (x, y periodic) | k_bc_all (any pointwise set) | one k_set_bc launch per direction
struct BcPath {
  BcForm vel = BcForm::by_direction, wm = BcForm::by_direction, cell[2] = {BcForm::by_direction, BcForm::by_direction};      // velocity set; tangential set of the wall-model faces; pressure [0] / sgs [1] set
  BcRules rules_vel[2][3] = {}, rules_cell[2] = {};      // [VelSet][component]; pressure [0] / sgs [1] set
  // the one thing a call decides about the form: k_bc_all does not serve a Neumann condition on face-centred data. Bit d-1: the normal component has one in direction d
  // on this rank (never with is_correc, which leaves a non-periodic normal direction alone) -- the velocity set takes `all` in calls that skip every such direction
  int vel_fcn = 0;
  bool ride[2] = {false, false};      // cell-centred fields with the pressure / sgs set can join the velocity's launch (BcCall::ride)
};
// What travels between y slabs for one field: its rows 1 / n2 into the neighbours' ghost rows (a field; a pair field, rows twice as long), or its rows
// 2 / n2-1 (3 / n2-2) into the ghost rows of the neighbours' first (second) companion field (cales_ctx::vel_comp)
enum class HaloRows : unsigned char { field, pair, second_rows, third_rows };
struct HaloBatch;      // (below, with StageLayout)
// What a caller inside cales_step asks of ONE call of a ghost-cell operator; default-constructed: the operator as the C-ABI entry runs it. The operator
// turns it, with BcPath's tables, into the rules of the call (bc_rule) and the exchange that goes with them
struct BcCall {
  int skip = 0;                  // bit d-1: leave direction d alone (the call's consumers do not read it)
  // bounduvw leaves the wall-model update and the tangential ghost cells of wall-model faces alone: those of the first bounduvw of a substep are rewritten
  // by the bounduvw that follows the correction before anything reads them (fillps, the solver and correc do not) -- StepPlan::skip_first_wm
  bool skip_wm = false;
  // the ghost rows already hold the neighbours' rows, no slab exchange (end-of-step refresh: only the x ghost columns are stale, the rows the neighbours
  // sent are complete but for their two ends, which the local copies fill; folded strain-rate pass: it formed the ghost rows itself)
  bool rows_current = false;
  HaloBatch *collect = nullptr;  // the y-halo rows are collected here instead of exchanged (the caller flushes: halo_flush)
  // corrected view (StepPlan::fold_mom): the fields hold the prediction, sources that are interior cells are read as (u* + f) - dtrk grad(pp); fmask: the
  // components whose bulk-forcing increment the pending projection adds
  real view_dtrk = 0.; int view_fmask = 0;
  // bounduvw: cell-centred riders (which: 0 pressure, 1 sgs set). They join the velocity's launch and slab exchange where BcPath::ride allows and z is
  // not skipped; otherwise bounduvw gives them their ghost cells itself right after the velocity's (boundp, this call minus the riders)
  int nride = 0; real *ride[3] = {nullptr, nullptr, nullptr}; int ride_which[3] = {0, 0, 0};
  void rider(real *p, int which) { ride[nride] = p; ride_which[nride++] = which; }
};
// rk inside cales_step. mean_mask: the bulk means of these forced components are summed by the forward x transform of the pressure solve (FusedFill);
// rhs_in_sweep: z-implicit, u -= hf12*dudtd is applied inside the Helmholtz sweep (StepPlan::defer_imp_rhs); store_rhs = false: third substep, nobody reads
// the new r.h.s. (MomRkArgs::wr_new); pending: the projection of the substep before, which the fused pass applies while it loads (k_momrk<.., CORR>)
struct RkOpts { int mean_mask = 0; bool rhs_in_sweep = false, store_rhs = true; const PendingProjection *pending = nullptr; };
// dtrki != 0: the forward x transform of the pressure solve forms pp = div(u*)/dtrk itself and sums the bulk means of the components in mean_mask
struct FusedFill { real dtrki = 0.; int mean_mask = 0; };

// Where the scalar reductions live (bulk means and forcing, chkdt, chkdiv, the dynamic model's plane sums), the same with and without communication:
// result slots, then the plane sums p1d, then the per-block partial sums. Results and p1d are what the slabs all-reduce: views into the tail of staging buffer A
// once hooks are registered, into the head of the context's own d_red (which always holds the partials) otherwise -- red_place (api.hip) places both
struct RedLayout {
  enum Slot { CHECK = 0, FORCE = 8, BULK_MEAN = 16, NSLOT = 64 };      // res[]: chkdt's two maxima | chkdiv's sum and maximum; FORCE + component: its bulk mean (rk.f90:197-222); cales_bulk_mean
  enum Host { H_CHECK = 0, H_BULK_MEAN = 16, H_FORCE = 32, H_DPDL = 35, NHOST = 64 };      // h_red[]: H_FORCE and H_DPDL are d_force's f(3) and dpdl(3), back to back
  int64_t p1d = NSLOT, np1d = 0, part = 0, npart = 0, total = 0;      // offset and length of p1d (2 n3 and two to spare) and of the partials (sixteen blocks per plane, or two arrays of eight); reals of d_red
  int64_t comm_tail = 0;      // reals at the end of the staging buffers that no exchange uses: results and p1d live there, with room to spare
  static RedLayout of(int n3) {
    RedLayout L; L.np1d = 2 * (int64_t)n3 + 2; L.part = L.p1d + L.np1d; L.npart = 16 * (int64_t)(n3 + 2); L.total = L.part + L.npart; L.comm_tail = 4096 + L.np1d + 2;
    return L;
  }
};
// Where the regions of the two staging buffers live (Comm::A and Comm::B: the host's memory, `total` reals each), worked out once by cales_create
// and only read after. Halo exchange: the lo | hi rows that leave at the head of A, those that arrive at the head of B, n planes each (blocks). All-to-all: P peer
// blocks from the head of both, slabs in A, mode blocks in B. Between two exchanges a caller may borrow the head of A (stage_borrow). The tail of A holds the
// reductions' results and plane sums (RedLayout::comm_tail), and no exchange or borrower reaches it.
struct StageLayout {
  static constexpr int MAXPLANES = 16;      // row planes of one block (lo or hi) of one halo exchange; a pair field takes two
  // the total counts FOUR blocks of MAXPLANES planes per buffer where the offsets use two (send and receive sit in different buffers): twice the room the
  // halo region needs, kept because the hosts size their memory by the total
  static constexpr int HALO_SIZED_FOR = 2;
  int64_t plane = 0;       // reals of one row plane, x and z ghost cells included: s1 (n3 + 2)
  int64_t halo = 0;        // the halo region [0, halo) of A (send) and of B (receive): two blocks of MAXPLANES planes
  int64_t a2a = 0;         // all-to-all capacity: reals of the P peer blocks of n3 n2l cw complex values
  int64_t borrow = 0;      // [0, borrow) of A may be borrowed between two exchanges: everything below the tail
  int64_t tail = 0, total = 0;      // offset of the tail (RedLayout::comm_tail reals) | reals of each buffer (cales_comm_buffer_doubles)
  struct Blocks { int64_t lo, hi, count; };      // offsets of the lo | hi block of an exchange of n planes (the same in A and B) and the reals of each
  Blocks blocks(int n) const { return Blocks{0, n * plane, n * plane}; }
  static StageLayout of(int s1, int n3, int n2l, int cw, int P, const RedLayout &red) {
    StageLayout L; L.plane = (int64_t)s1 * (n3 + 2); L.halo = 2 * MAXPLANES * L.plane; L.a2a = 2 * (int64_t)P * n3 * n2l * cw;
    L.tail = L.borrow = L.a2a > HALO_SIZED_FOR * L.halo ? L.a2a : HALO_SIZED_FOR * L.halo; L.total = L.tail + red.comm_tail;
    return L;
  }
};
// y-halo rows collected over several ghost-cell calls and exchanged in ONE message by halo_flush: a local of the caller
struct HaloBatch { int n = 0; real *p[StageLayout::MAXPLANES]; HaloRows kind[StageLayout::MAXPLANES]; };
constexpr real RKPAR[3][2] = {{32. / 60., 0.}, {25. / 60., -17. / 60.}, {45. / 60., -25. / 60.}};      // the three substeps' coefficients, param.f90:27-29
struct KernelStat { std::string name; int64_t calls = 0; real ms = 0.; };
struct Solver;      // k_solver.hip
struct MemBlock { void *base; size_t bytes; bool pinned; };      // one allocation of a context ("who owns device memory")

struct cales_ctx {
  cales_case C{};
  Flags fl;
  StepPlan plan;      // see StepPlan above
  Geom g{};
  int n[3] = {0, 0, 0}, lo[3] = {1, 1, 1};
  real dl[3] = {0., 0., 0.}, dli[3] = {0., 0., 0.}, visc = 0.;
  hipStream_t stream = nullptr; bool own_stream = false;
  hipStream_t comm_stream = nullptr;      // exchanges that overlap kernels (created by cales_set_comm_overlap)
  std::vector<hipEvent_t> sync_ev; size_t sync_next = 0;      // ordering events between the two streams (no timing), reused round-robin
  std::string err;
  std::string launch_err;      // first failed kernel launch / attribute call (LAUNCH below): the context is failed from then on
  // host copies of the grid
  std::vector<real> dzc, dzf, zc, zf, dzci, dzfi, gvr_c, gvr_f;
  char cbcvel[18] = {};
  int is_bound[6] = {}, index_wm[6] = {};
  std::vector<MemBlock> mem; int64_t mem_bytes = 0;      // every device and pinned-host allocation of the context, temporaries of a call included (ctx_alloc)
  // device grid (0:n3+1)
  real *d_dzc = nullptr, *d_dzf = nullptr, *d_zc = nullptr, *d_zf = nullptr, *d_dzci = nullptr, *d_dzfi = nullptr, *d_gvr_c = nullptr, *d_gvr_f = nullptr;
  // fields
  real *f[CALES_NFIELDS] = {};
  real *f2[3] = {nullptr, nullptr, nullptr};   // second velocity buffers of the fused mom+RK kernel (pointers are swapped with f[U..W])
  size_t ntot = 0;
  // BC planes
  DBound bcu, bcv, bcw, bcp, bcs, bcuf, bcvf, bcwf, bcu_mag, bcv_mag, bcw_mag;
  real *rhsbp[3] = {nullptr, nullptr, nullptr};        // (na,nb,0:1)
  // solver
  // k_solver.hip: plans, tables and the path of every solved field; the z solves' coefficients, chunked tables and scratch (solver_setup; the device tables are the context's memory)
  Solver *solver = nullptr;
  real *scr1 = nullptr, *scr2 = nullptr;         // solver scratch (haloed size)
  RedLayout red;      // reductions (RedLayout above)
  real *d_red = nullptr; real *h_red = nullptr;       // the context's own buffer of red.total reals | results on the host (pinned, RedLayout::Host)
  real *res = nullptr, *d_p1d = nullptr;              // views placed by red_place: result slots and plane sums, in d_red or in the tail of comm.A
  real step_dt = 0.;                                  // dt of the last cales_step (cales_get_dpdl divides by it)
  real *d_force = nullptr;                    // f(3) + dpdl(3) accumulators on device
  // sgs scratch
  real *ss2[3] = {nullptr, nullptr, nullptr};      // |S|Sij as three pair fields (2 ntot reals each; SgsPath::pair) instead of sij / mij
  real *s0 = nullptr, *wk[6] = {}, *sij[6] = {}, *mij[6] = {}, *uc = nullptr, *vc = nullptr, *wc = nullptr, *uf = nullptr, *vf = nullptr, *wf = nullptr, *alph2 = nullptr;
  real is_wall[6] = {};
  SgsPath sgs;      // see SgsPath above
  BcPath bc;        // see BcPath above
  MomPath mom;      // see MomPath above
  bool sgs_first = true;
  // decomposition
  int P = 1, rank = 0; bool per_y = true; int cw = 0;      // cw: complex mode columns per rank (padded)
  Comm comm;
  StageLayout stage;      // the regions of comm.A / comm.B (StageLayout above)
  // profiling
  bool prof = false;
  std::vector<KernelStat> stats;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evpool;
  real *d_del = nullptr;   // Smagorinsky filter width per plane (fast path)
  void *native_comm = nullptr;   // RCCL communicator when the library does the exchanges itself (comm_rccl.cpp)
  bool visct_zero = true;  // CALES_VISCT still holds the zeros it was created / reset with (no SGS model: lets kernels skip it)
  // dynamic model, fast path: the eddy-viscosity field holds |S| and d_cs(0:n3+1) the clipped plane coefficients <LM>/<MM> until somebody
  // other than the fused momentum kernel reads it (materialize_visct); visct = |S| * cs(k) is the same product either way
  bool visct_lazy = false; real *d_cs = nullptr;
  // The mode of the step in progress, read by the host side of nearly every operator. Everything else a step decides reaches the operators as
  // arguments (BcCall, RkOpts, FusedFill, SgsFold, ...)
  bool in_step = false;             // inside cales_step: the operator order is known, dead ghost work can be dropped
  bool force_zeroed = false;
  int ncu = 0;      // compute units of the device (balanced_kchunk)
  // cales_step with periodic x: the x ghost columns are not maintained between the operators of a step -- every kernel of the step reads the wrapped
  // interior column instead (a ghost-column update touches two cache lines per row and field for two values: 1.2 of 45 ms per step at 512^3) -- and
  // are brought up to date once, when the step returns
  bool step_xskip = false;
  // What outlives a call of cales_step, written by step_body as it returns and taken off by the next step or by finish_pending (api.hip), which every other
  // entry of the C-ABI that reads or writes a field calls first (cales_sync included: a caller never sees the prediction). pend: the third substep's
  // projection (StepPlan::lazy_last) -- the next step's first momentum pass applies it. pend_xrefresh: only the x ghost columns are due (a step with
  // step_xskip; local copies, no exchange: safe on several slabs) -- the next cales_step does not read them, the refresh is 0.2 ms of strided accesses at 512^3
  PendingProjection pend;
  bool pend_xrefresh = false;
  size_t pp_companion_bytes = 0;      // scr2 sits this many bytes behind CALES_PP in one allocation (api.hip field_alloc_multi)
  // several slabs with the dynamic model: u, v, w (both buffer sets) and pp carry COMPANION fields right behind them in their allocations (the same
  // distance for all: comp_one reals) -- the second ghost rows of the folded strain-rate pass (rows -1 and n2+2 in the companion's ghost rows 0 and
  // n2+1; pp a second companion for row n2+3), exchanged from the rows 2 / n2-1 (3) of the neighbours (k_bound.hip, halo kinds 2 and 3)
  bool vel_comp = false; size_t comp_one = 0; real *scr3 = nullptr;
  int field_ofs = 0;       // doubles between a field's allocation and its element (0,0,0)
};

#define CBV(c, side, dir, vel) ((c)->cbcvel[(side) + 2 * ((dir) - 1) + 6 * ((vel) - 1)])
#define CBP(c, side, dir) ((c)->C.cbcpre[(side) + 2 * ((dir) - 1)])
#define CBS(c, side, dir) ((c)->C.cbcsgs[(side) + 2 * ((dir) - 1)])
#define LWM(c, side, dir) ((c)->C.lwm[(side) + 2 * ((dir) - 1)])
#define ISB(c, side, dir) ((c)->is_bound[(side) + 2 * ((dir) - 1)])
#define IWM(c, side, dir) ((c)->index_wm[(side) + 2 * ((dir) - 1)])

#define HIPCHK(ctx, call)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
      return 1;                                                                                    \
    }                                                                                              \
  } while (0)

// ---- every kernel launch is checked (the reference ignores its istat everywhere, src/solver_gpu.f90:80).
// LAUNCH = hipLaunchKernelGGL + hipGetLastError: an invalid configuration (block size, LDS size, too many registers for the block) is caught at the
// launch site. The FIRST failure is recorded in c->launch_err with the kernel's name and stays there: the context is failed, LAUNCHCHK at the end
// of every operator and cales_* entry returns non-zero with that message (cales_last_error), and every later call on the context refuses to run --
// never a silently wrong field. Void helpers and lambdas record through the same path (HIPSOFT for other HIP calls whose status must not be lost).
// Test hook: CALES_TEST_BAD_LAUNCH=<substring of a kernel name> gives the matching launches a block of 4096 threads (invalid on every device).
void launch_failed(cales_ctx *c, const char *what, hipError_t e);
#define LAUNCH_NAMED(c, kernel, name, grid, block, lds, stream, ...)                               \
  do {                                                                                             \
    dim3 blk_ = (block);                                                                           \
    if (!(c)->fl.test_bad_launch.empty() && strstr(name, (c)->fl.test_bad_launch.c_str())) blk_ = dim3(4096, 1, 1); \
    hipLaunchKernelGGL(kernel, grid, blk_, lds, stream, __VA_ARGS__);                              \
    const hipError_t le_ = hipGetLastError();                                                      \
    if (le_ != hipSuccess) launch_failed(c, name, le_);                                            \
  } while (0)
#define LAUNCH(c, kernel, ...) LAUNCH_NAMED(c, kernel, #kernel, __VA_ARGS__)
// ... of a kernel record (KernelRec above): the kernel a set-up function chose, under the name that function spelled
#define LAUNCH_REC(c, rec, ...) LAUNCH_NAMED(c, (rec).fn, (rec).name, __VA_ARGS__)
#define LAUNCHCHK(c)                                                                               \
  do {                                                                                             \
    if (!(c)->launch_err.empty()) { (c)->err = (c)->launch_err; return 1; }                        \
  } while (0)
#define HIPSOFT(c, call)                                                                           \
  do {                                                                                             \
    const hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) launch_failed(c, #call, e_);                                             \
  } while (0)

// profiling bracket: PROF_BEGIN(ctx,"name"); launch...; PROF_END(ctx)
int  prof_begin(cales_ctx *c, const char *name, hipStream_t s = nullptr);
void prof_end(cales_ctx *c, int slot, hipStream_t s = nullptr);
// the next ordering event of the context's pool (cales_ctx::sync_ev, round robin), recorded on `s`
int  mark_stream(cales_ctx *c, hipStream_t s, hipEvent_t *e);
// `later` waits for everything queued on `earlier` so far
int  stream_after(cales_ctx *c, hipStream_t later, hipStream_t earlier);
void prof_flush(cales_ctx *c);
struct ProfScope {
  cales_ctx *c; int slot;
  hipStream_t s;
  ProfScope(cales_ctx *c_, const char *name, hipStream_t s_ = nullptr) : c(c_), slot(c_->prof ? prof_begin(c_, name, s_) : -1), s(s_) {}
  ~ProfScope() { if (slot >= 0) prof_end(c, slot, s); }
};

// ---- device memory (api.hip): n reals (at least one) until cales_destroy (ctx_release_all), zeroed on request; ctx_free gives one allocation back early
int  ctx_alloc(cales_ctx *c, real **p, size_t n, bool zero = true);
int  ctx_alloc_pinned(cales_ctx *c, real **p, size_t n);
int  ctx_upload(cales_ctx *c, real **p, const std::vector<real> &v);      // ... holding a copy of a host table
void ctx_free(cales_ctx *c, real *p);
void ctx_release_all(cales_ctx *c);
struct CtxTemp {      // n reals for the length of a scope, released on every return (p null: the allocation failed, c->err says why)
  cales_ctx *c; real *p = nullptr;
  CtxTemp(cales_ctx *c_, size_t n) : c(c_) { ctx_alloc(c, &p, n, false); }
  CtxTemp(const CtxTemp &) = delete;
  ~CtxTemp() { ctx_free(c, p); }
};
// ---- host-side set-up (host_setup.cpp)
void   hs_initgrid(int gtype, int n, real gr, real lz, real *dzc, real *dzf, real *zc, real *zf);
void   hs_initbc(cales_ctx *c, std::vector<real> hb[11][3]);
void   hs_eigenvalues(int n, const char *cbc2, char c_or_f, real *lambda);
void   hs_tridmatrix(const char *cbc2, int n, const real *dzci, const real *dzfi, char c_or_f, real *a, real *b, real *c);
int    hs_initflow(const cales_case *cs, const char *inivel, int is_wallturb, real *u, real *v, real *w, real *p, int rank, int nranks);
int    hs_check_case(const cales_case *cs, std::string &msg);
void   hs_bc_rhs(const char *cbc2, const real *bc, int na, int nb, const real *dlc, const real *dlf, char c_or_f, real *rhs);

// ---- device operators (k_*.hip); all asynchronous on c->stream
void bc_setup(cales_ctx *c);                // BcPath (needs is_bound, cbcvel, the grid and the BC planes)
int op_bounduvw(cales_ctx *c, VelSet set, int is_updt_wm, int is_correc, const BcCall &b = BcCall());      // the set's fields are read at call time (the f / f2 swaps)
int op_boundp(cales_ctx *c, real *p, int which, const BcCall &b = BcCall());
int op_boundp_multi(cales_ctx *c, int nf, real **p, int which, const BcCall &b = BcCall());
// the two entries of the slab exchange of rows (k_bound.hip): the rows of nf fields of one kind into the caller's batch (BcCall::collect) or exchanged now --
// vcomp: the corrected-view components of a call that carries a view, with the "now" case only --, and a batch flushed in order or on the second stream
int halo_rows(cales_ctx *c, int nf, real **flds, HaloRows kind, const BcCall &b, const unsigned char *vcomp = nullptr);
int halo_flush(cales_ctx *c, HaloBatch &rows, bool second_stream);
int op_mom(cales_ctx *c);
int op_rk(cales_ctx *c, int irk, real dt, const RkOpts &o = RkOpts());
int op_rk_par(cales_ctx *c, real rkpar1, real rkpar2, real dt, const RkOpts &o = RkOpts());
int op_momrk(cales_ctx *c, real f1, real f2, real f12, const RkOpts &o = RkOpts());
void mom_setup(cales_ctx *c);               // MomPath (needs ncu)
int op_bulk_forcing(cales_ctx *c);
int op_bulk_mean_dev(cales_ctx *c, const real *p, int c_or_f);   // result to res[RedLayout::BULK_MEAN]
real *red_partials(cales_ctx *c, size_t need);      // room for `need` partial sums (RedLayout); nullptr and c->err where the layout has less
int allreduce_dev(cales_ctx *c, real *p, int64_t count, int op);      // [p, p + count) over the slabs, in place (op: 0 sum, 1 max): nothing on one rank; the range must lie in the tail of staging buffer A or in its borrowed head
real *stage_borrow(cales_ctx *c, int64_t n);      // n reals at the head of staging buffer A, free of every exchange queued so far (StageLayout::borrow); nullptr and c->err otherwise
int read_back(cales_ctx *c, real *host, const real *dev, size_t n);      // n reals to the host on the context's stream, complete on return
// ... n elements of any type, queued on the context's stream and NOT waited for: the caller syncs once behind its last copy
template <class T> int read_back_queued(cales_ctx *c, T *host, const void *dev, size_t n) {
  HIPCHK(c, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return 0;
}
int op_zero_force(cales_ctx *c, int first, int last);      // d_force[first, last) = 0 (f(3), dpdl(3))
int op_fillps(cales_ctx *c, real dtrki);
int op_updt_rhs_b(cales_ctx *c);
int op_solver(cales_ctx *c, const FusedFill &fill = FusedFill());
int op_helmholtz_z(cales_ctx *c, int ivel, real alpha, bool fused_rhs = false, real hf12 = 0.);      // fused_rhs: the sweep forms (u - hf12*dudtd) + f + rhs_b while loading
extern "C" void cales_comm_release_native(cales_ctx *c);
int op_helmholtz(cales_ctx *c, int ivel, real alpha);
int op_correc(cales_ctx *c, real dtrk, int fmask = 0);      // fmask: see op_correc_updatep
int materialize_visct(cales_ctx *c);
// THE check of a field id of the C-ABI (api.hip): the device pointer of field `id` (enum cales_field), or nullptr and c->err = "<who>: bad field id" for an
// id out of range or a field this context did not allocate. `use`: FIELD_READ -- the caller reads the field: a lazy eddy viscosity is materialized first |
// FIELD_ROWS16 -- its kernels load 16 bytes per lane from element 1 of a row (readout.hpp): refused unless that is a 16-byte boundary. An entry that refuses
// other arguments checks the id first WITHOUT FIELD_READ and asks again with it last: nothing is materialized or launched for a call that is refused
enum FieldUse { FIELD_WRITE = 0, FIELD_READ = 1, FIELD_ROWS16 = 2 };
real *field_ptr(cales_ctx *c, int id, const char *who, int use);
int op_stats_chan(cales_ctx *c, real *buf);
int op_stats_chan_budget(cales_ctx *c, real *budget, real *leak);
int op_out1d(cales_ctx *c, int field, int idir, int use_dzc, real *buf);
int op_out1d_chan(cales_ctx *c, real *buf);
int op_out2d_duct(cales_ctx *c, real *buf);
// include/cales_pdf.h (k_pdf.hip): per-plane histograms of a field, joint histograms of two fields on chosen planes; synchronous
int op_pdf_planes(cales_ctx *c, int field, int nbins, real lo, real hi, int64_t *counts, int64_t *outside);
int op_jpdf_planes(cales_ctx *c, int field_a, int field_b, int nbins, real lo_a, real hi_a, real lo_b, real hi_b, int nplanes, const int32_t *kplanes,
                   int64_t *counts, int64_t *outside);
// include/cales_spectra.h (k_spectra.hip): power spectra of a field along x or y on every plane, and in chosen x-y planes; synchronous
int op_spectra_lines(cales_ctx *c, int field, int idir, real *power, real *lsum);
int op_spectra_planes(cales_ctx *c, int field, int nplanes, const int32_t *kplanes, real *power2);
// include/cales_cospectra.h (k_spectra.hip, the two-field form of the above): cross-spectra of two fields sampled at the same index, along x or y on every plane and in chosen x-y planes; synchronous
int op_cospectra_lines(cales_ctx *c, int field_a, int field_b, int idir, real *cross, real *lsum_a, real *lsum_b);
int op_cospectra_planes(cales_ctx *c, int field_a, int field_b, int nplanes, const int32_t *kplanes, real *cross2);
// include/cales_derived.h (k_derived.hip): vorticity, SijSij, WijWij and Q of the stored velocity, as a strided box for the host or into the interior of pp; synchronous
// (first, count: the rank's share of the box as cales_box_share gives it, checked by the entry -- interior cells only, first in GLOBAL indices)
int op_derived_box(cales_ctx *c, int quantity, const int32_t *first, const int32_t *count, const int32_t *nskip, real *buf);
int op_derived_to_pp(cales_ctx *c, int quantity);
bool solver_can_fuse_fillps(cales_ctx *c);
int solver_mode_columns(cales_ctx *c);      // complex mode columns per rank of the pressure solve
std::string solver_path_name(cales_ctx *c);      // which transform / tridiagonal kernels the pressure solve of this context takes (cales_describe_plan)
std::string helmholtz_path_name(cales_ctx *c, int iv);      // ... and the Helmholtz solve of velocity component iv (0..2) of the 3-D implicit step
const char *sgs_path_name(const cales_ctx *c);      // likewise for cmpt_sgs (SgsPath)
void sgs_setup(cales_ctx *c);               // SgsPath: form, flags, static kernel arguments and kernel records (needs is_wall)
int sgs_setup_launches(cales_ctx *c);       // ... and the launch geometry of its tile passes (needs ncu)
int op_force_from_partials(cales_ctx *c, int mask, const real *part, int nblk);
int op_correc_updatep(cales_ctx *c, real dtrk, real alpha, int upd, int fmask = 0);      // fmask: the components whose deferred bulk-forcing increment the pass adds (StepPlan::defer_force)
int op_updatep(cales_ctx *c, real alpha);
// fold: the projection folded into the strain-rate pass (cales_step), nullptr: not folded; visct_ghosts_done (cales_step): set where the pass has updated the
// ghost cells of the eddy viscosity itself (dsmag, lazy form on several slabs: with the scratch fields' exchange)
int op_cmpt_sgs(cales_ctx *c, const SgsFold *fold, bool *visct_ghosts_done = nullptr);
int op_boundp_wide(cales_ctx *c, int nf, real **p2, int which, const BcCall &b = BcCall());      // ghost cells of pair fields (y, z; x periodic and wrapped by the consumers)
int op_xwrap_zghost(cales_ctx *c, int nf, real **f);      // periodic copy of the x ghost columns on the planes k = 0 and n3+1
int op_chkdt(cales_ctx *c, real *dtmax);
int op_chkdiv(cales_ctx *c, real *divtot, real *divmax);
int solver_setup(cales_ctx *c);
int solver_comm_changed(cales_ctx *c);      // comm_changed (api.hip): the staging buffers and the exchange form of the solves' schedules
void solver_teardown(cales_ctx *c);      // (the host-side struct; its tables go with the context's memory)

// XCD-aware block order for the one-plane-per-block stencil kernels (grid = x tiles, y tiles, z planes).
// Workgroups are dealt round-robin to the 8 XCDs, each with its private 4 MiB L2 (MI355X_MICROARCH.md, "Workgroup
// dispatch"). The remap lets every XCD walk a fixed (x tile, group of 8 y-adjacent tiles) column through k, so the k+-1
// planes and j+-1 rows a block needs were fetched moments earlier by blocks of the SAME XCD and are L2 hits instead
// of HBM re-reads. Only the order changes (a bijection on block ids); results are identical.
#ifdef __HIPCC__

// ---- global accesses as base pointer (kernel argument, scalar registers) + BYTE offset. With OFF = unsigned the compiler
// emits the saddr + 32-bit voffset form: one VGPR per access stream instead of a 64-bit address per field (tile kernels
// stream up to 17 fields). Hosts pick OFF = unsigned when a field is smaller than 4 GB, size_t otherwise.
// element k of a small read-only coefficient array (grid spacings, zc, ...) through the scalar cache: the constant address space makes the
// load an s_load (lgkmcnt) whatever stores the kernel makes, so waiting for it never drains the vector loads in flight (a global_load of the
// same value costs an s_waitcnt vmcnt(0) in the middle of a prefetch)
// (in the LDS-heavy last dsmag pass the same change measured 7 % slower -- scalar loads share lgkmcnt with the LDS reads and return
// out of order, so waiting for one drains the LDS queue -- and that kernel keeps its vector loads)
// ONLY for data no kernel writes while a kernel reads it through here: the scalar cache is not coherent with vector stores inside a launch (it is
// invalidated at kernel boundaries). The grid tables never change; the plane coefficients d_cs of the dynamic model are written by k_dsmag_coef and
// read through ldc by LATER launches only (k_momrk) -- a kernel that both wrote and read them would see stale values.
__device__ inline real ldc(const real *p, int k) { return ((const __attribute__((address_space(4))) real *)p)[k]; }
template <typename OFF> __device__ inline real ldb(const real *b, OFF o) { return *(const real *)((const char *)b + o); }
template <typename OFF> __device__ inline void stb(real *b, OFF o, real v) { *(real *)((char *)b + o) = v; }

// ---- cross-lane moves on the vector ALU (DPP) instead of ds_bpermute: no LDS-pipe traffic, short latency ----
template <int CTRL, int ROWMASK = 0xf>
__device__ inline real dpp_f64(real v) {       // lanes without a source receive 0 (bound_ctrl); rows masked out keep v itself
#ifdef CALES_SINGLE
  const int w = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(w, w, CTRL, ROWMASK, 0xf, true));
#else
  int lo = __double2loint(v), hi = __double2hiint(v);
  // old = the source register and bound_ctrl: no register has to be zeroed before every move (the old form cost one v_mov per dpp move)
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROWMASK, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROWMASK, 0xf, true);
  return __hiloint2double(hi, lo);
#endif
}
// the value of one lane (a compile-time lane number) in all lanes: v_readlane_b32 through a scalar register
template <int LANE>
__device__ inline real lane_bcast(real v) {
#ifdef CALES_SINGLE
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), LANE));
#else
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), LANE), __builtin_amdgcn_readlane(__double2loint(v), LANE));
#endif
}
__device__ inline real lane_prev(real v) { return dpp_f64<0x138>(v); }   // wave_shr:1, lane i <- lane i-1 (lane 0 <- 0)
__device__ inline real lane_next(real v) { return dpp_f64<0x130>(v); }   // wave_shl:1, lane i <- lane i+1 (lane 63 <- 0)
// sum over the 64 lanes, valid in lane 63 ONLY (row_shr 1,2,4,8 then row_bcast 15 and 31; the rows the two broadcasts mask out
// add their own value to themselves, so every other lane ends with garbage -- callers must consume the result in lane 63 and nowhere else)
__device__ inline real wave_sum_lane63(real s) {
  s += dpp_f64<0x111>(s); s += dpp_f64<0x112>(s); s += dpp_f64<0x114>(s); s += dpp_f64<0x118>(s);
  s += dpp_f64<0x142, 0xa>(s); s += dpp_f64<0x143, 0xc>(s);
  return s;
}

// Block -> tile map of the plane-marching tile kernels, launched as a 1-D grid: consecutive blocks go to the eight XCDs in turn, and each XCD
// takes bands of `sub` consecutive y tiles with all their x tiles and k chunks (x fastest, then y inside the band, then k), so that the halo
// rows and columns two neighbouring tiles both read meet in one XCD's L2 instead of being fetched over the fabric twice. With the plain 3-D
// grid every y neighbour sits on another XCD. The grid is padded to whole bands; blocks of the padding return at once (false).
static inline BandMap band_map(int gx, int gy, int gz) { BandMap m{gx, gy, gz, 1}; m.sub = gy >= 64 ? 8 : (gy + 7) / 8; if (m.sub < 1) m.sub = 1; return m; }
// The plain 3-D grid already gives every XCD fixed x-tile columns (y neighbours in one L2) when the number of x tiles divides 8 or is a multiple
// of it -- the 64-wide tiles of power-of-two grids: there the bands bring nothing (momentum pass 8.0 -> 8.6 ms/step at 512^3, measured) and
// are not used; the 62-wide tiles (9 per 512 cells: the XCD of a tile then runs along diagonals) and odd sizes take the bands.
static inline bool band_wanted(int gx) { return !(gx % 8 == 0 || 8 % gx == 0); }
static inline unsigned band_blocks(const BandMap &m) { return 8u * m.gx * m.sub * m.gz * ((m.gy + 8 * m.sub - 1) / (8 * m.sub)); }
// a tile launch through the band map where that helps (band_wanted): the grid becomes the padded 1-D grid of the bands
static inline TileGeom with_bands(TileGeom t) {
  if (band_wanted(t.grid.x)) { t.bm = band_map(t.grid.x, t.grid.y, t.grid.z); t.grid = dim3(band_blocks(t.bm), 1, 1); }
  return t;
}
__device__ inline bool band_block(const BandMap &m, int &bx, int &by, int &bz) {
  unsigned s = blockIdx.x >> 3; const unsigned xcd = blockIdx.x & 7u;
  bx = s % m.gx; s /= m.gx; const unsigned sb = s % m.sub; s /= m.sub; bz = s % m.gz; s /= m.gz;
  by = (s * 8 + xcd) * m.sub + sb;
  return by < m.gy;
}
__device__ inline void stencil_block(int &bx, int &by, int &bz) {
  const unsigned gx = gridDim.x, gy = gridDim.y, gz = gridDim.z, SUB = 8;
  if (gy % SUB != 0 || (gx * (gy / SUB)) % 8 != 0) { bx = blockIdx.x; by = blockIdx.y; bz = blockIdx.z; return; }
  const unsigned L = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  const unsigned xcd = L & 7u, s = L >> 3;
  const unsigned sub = s % SUB, k = (s / SUB) % gz, T = (s / (SUB * gz)) * 8 + xcd;
  bx = (int)(T % gx); by = (int)((T / gx) * SUB + sub); bz = (int)k;
}
#endif

// shortest chunk of a grid with fewer blocks than CUs: every block runs at once, a launch lasts (chunk + 3-plane prologue) planes -- 64^3 Taylor-Green:
// momentum pass 77 -> 54 us per step with chunks of 4 planes instead of 8 (192 blocks of 7 planes against 48 of 11), the step 0.223 -> 0.200 ms
constexpr int SMALL_KCH = 4;
// Few rounds of blocks (a y slab of a decomposed grid, a mid-size grid): the marching tile kernels hold ONE block per CU, a launch then runs in
// ceil(blocks / CUs) rounds of (chunk length + prologue) planes each, and half-empty last rounds show -- one rank of eight of the 512^3 channel:
// strain-rate pass 1.48 -> 1.32 ms/step with 9 chunks of 57 planes (504 blocks, 1.97 rounds) instead of 16 of 32 (896 blocks, 3.5 rounds), the
// dynamic model's last pass 1.39 -> 1.27 with 7 chunks instead of 16; the measured order of eight chunk lengths follows rounds x (planes + 3).
// With many rounds (the 512^3 grid on one GPU: 6.5) the passes are bound by bandwidth, idle CUs of the last round leave theirs to the others and
// the rule does not hold (measured: 13 full rounds 3 % SLOWER than 6.5) -- so: only below seven rounds, chunk lengths from 16 planes. (6.5 rounds, end of
// round 6: one rank of four -- 16 chunks of 32 planes against 12 of 43 -- strain-rate pass 2.94 -> 2.74, last pass 2.60 -> 2.56, momentum 2.03 -> 1.91 ms/step,
// every chunk length tried in the order of the product; the 512 x 256 x 256 duct momentum 2.52 -> 2.44; one rank of two -- 8 chunks of 64 against 6 of 86 -- equal.)
static inline int balanced_kchunk(const cales_ctx *c, long nxy_blocks, int n3, int kch0, int kmax = 1 << 30) {
  const long ncu = c->ncu > 0 ? c->ncu : 256;
  const int nch0 = (n3 + kch0 - 1) / kch0;
  if (nxy_blocks * nch0 >= 7 * ncu || c->fl.kchunk > 0 || c->fl.tile_min_blocks != 2048) return kch0;      // (switches that force chunking: the tests' business)
  long best = -1; int bk = kch0;
  for (int nch = 1; nch <= 4 * nch0 + 4; ++nch) {
    const int kch = (n3 + nch - 1) / nch;
    if (kch < 16 && kch < kch0) break;
    if (kch > kmax) continue;
    const long nb = nxy_blocks * ((n3 + kch - 1) / kch), cost = ((nb + ncu - 1) / ncu) * (kch + 3);
    if (best < 0 || cost < best) { best = cost; bk = kch; }
  }
  return bk;
}
// Geometry of a marching tile kernel (plain 3-D grid): blocks of 64 x (ty + 2), tiles ty x wx over n2 + rows_more rows, k chunks halved until the grid has
// tile_min_blocks blocks, on small grids one per CU (SMALL_KCH), then balanced over the rounds (balanced_kchunk); CALES_KCHUNK overrides.
static inline void tile_chunks(const cales_ctx *c, TileGeom &t, int kmax = 1 << 30) {      // the k chunks of t.grid.x x t.grid.y tiles: t.kchunk, t.grid.z
  const int *n = c->n;
  const long nxy = (long)t.grid.x * t.grid.y;
  int kch = n[2];
  while (nxy * ((n[2] + kch - 1) / kch) < c->fl.tile_min_blocks && kch > 32) kch = (kch + 1) / 2;
  while (nxy * ((n[2] + kch - 1) / kch) < 256 && kch > SMALL_KCH) kch = (kch + 1) / 2;
  kch = balanced_kchunk(c, nxy, n[2], kch, kmax);
  if (c->fl.kchunk > 0) kch = c->fl.kchunk < n[2] ? c->fl.kchunk : n[2];      // (experiments)
  t.kchunk = kch; t.grid.z = (n[2] + kch - 1) / kch;
}
static inline TileGeom tile_geom(const cales_ctx *c, int ty, int wx, int rows_more = 0, int kmax = 1 << 30) {
  const int *n = c->n;
  TileGeom t; t.block = dim3(64, ty + 2, 1); t.grid = dim3((n[0] + wx - 1) / wx, (n[1] + rows_more + ty - 1) / ty, 1);
  tile_chunks(c, t, kmax);
  return t;
}
static inline bool any_wm(const cales_ctx *c) { for (int q = 0; q < 6; ++q) if (c->C.lwm[q] != 0) return true; return false; }      // some face of the CASE has a wall model (a face owned by another slab counts)
// some wall-model face of the CASE (on whichever rank) has its sampling height inside the first cell: its interpolation reaches the ghost cell (index_wm = 1 / n,
// wmodel.f90:120-131; the conditions of host_setup.cpp's index search, from global quantities only -- every rank must answer alike: what hangs on the answer
// moves an all-reduce from one place of the substep to another)
static inline bool wm_samples_ghost(const cales_ctx *c) {
  const real h = c->C.hwm;
  for (int d = 1; d <= 3; ++d) for (int sd = 0; sd <= 1; ++sd) if (c->C.lwm[sd + 2 * (d - 1)] != 0) {
    const real first = d < 3 ? 0.5 * c->dl[d - 1] : (sd == 0 ? c->zc[1] : c->C.l[2] - c->zc[c->n[2]]);      // distance of the first cell centre from the wall
    if (!(first < h)) return true;
  }
  return false;
}
// several slabs need the hooks: THE sentence of every call that finds none (who: the caller's prefix)
static inline int require_hooks(cales_ctx *c, const char *who = "") {
  if (!c->comm.on) c->err = std::string(who) + "nranks > 1 but no communication hooks registered (cales_set_comm)";
  return c->comm.on ? 0 : 1;
}
static inline int bc_skipped(const cales_ctx *c, const BcCall &b) { return b.skip | (c->step_xskip ? 1 : 0); }
static inline dim3 grid3(int nx, int ny, int nz, dim3 b) { return dim3((nx + b.x - 1) / b.x, (ny + b.y - 1) / b.y, (nz + b.z - 1) / b.z); }
