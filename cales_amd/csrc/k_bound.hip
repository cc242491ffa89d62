// Ghost-cell operators: bounduvw / boundp / set_bc (reference src/bound.f90:18-399), the single-rank image of updthalo (src/bound.f90:619-696),
// updt_rhs_b (src/bound.f90:562-617) and the log-law / laminar wall model (src/wmodel.f90:19-335).
//
// The reference issues one tiny `!$acc kernels` region per face and field (39 regions), x, then y, then z: corner ghosts depend on that order. Here a
// ghost-cell update is a list of entries {field, rules, view} (BcEntry) that takes one of three kernel forms (BcForm, chosen per BC set by bc_setup):
//   k_bc_merged   x and y periodic, any pointwise z condition: all directions of up to eight fields in one launch;
//   k_bc_all      any set of pointwise conditions but Neumann on face-centred data: all directions of up to six fields in one launch;
//   k_set_bc      one launch per direction in the reference's order, up to six (field, end) jobs each: what the others do not serve, CALES_UNMERGED_BC.
// What the case fixes about every (field kind, direction, end) sits in BcPath's tables (bc_setup), what a call changes is applied by bc_rule, and every
// operator -- bounduvw with its riders and wall-model faces, boundp of one or several fields, pair fields -- goes through bc_update: the slab exchange,
// one builder per form, one launch site per kernel.
#include "common.hpp"

// Corrected view (cales_step, projection folded into the next momentum pass): a source cell that is an INTERIOR cell (1..n in all three directions) is
// read as the projected velocity (u* + f) - dtrk grad(pp) of component comp = 1..3 (the expressions of k_correc_cell), every other cell as stored --
// ghost cells written by an earlier direction of the same update are final already. comp = 0: plain reads.
struct CorrView { const real *pp, *dzci, *force; real cfi, cfj, dt; int fmask, perx; };      // force: the bulk-forcing increments of the substep (device), fmask: the forced components
__device__ inline real view_rd(const Geom &g, const CorrView &V, int comp, const real *p, int i, int j, int k) {
  const size_t c = g.ix(i, j, k);
  const real v = p[c];
  if (!comp || i < 1 || i > g.n1 || j < 1 || j > g.n2 || k < 1 || k > g.n3) return v;
  const real pc = V.pp[c];
  const real pb = comp == 1 ? V.pp[(V.perx && i == g.n1) ? g.ix(1, j, k) : c + 1] : comp == 2 ? V.pp[c + g.s1] : V.pp[c + g.s12];
  const real cf = comp == 1 ? V.cfi : comp == 2 ? V.cfj : V.dt * V.dzci[k];
  return ((V.fmask >> (comp - 1) & 1) ? v + V.force[comp - 1] : v) - cf * (pb - pc);
}
static CorrView corr_view(const cales_ctx *c, const BcCall &b) {
  CorrView V{};
  V.pp = c->f[CALES_PP]; V.dzci = c->d_dzci; V.force = c->d_force; V.cfi = b.view_dtrk * c->dli[0]; V.cfj = b.view_dtrk * c->dli[1]; V.dt = b.view_dtrk;
  V.fmask = b.view_fmask; V.perx = c->step_xskip ? 1 : 0;
  return V;
}
struct BcJob {
  real *p;          // field
  const real *bc;   // plane of side `ibound` (already offset), (0:na+1,0:nb+1)
  real dr;
  char ctype;         // 'P','D','N'
  char centered;
  char ibound;
  char vcomp = 0;     // != 0: sources through the corrected view of this velocity component
};
struct BcJobs { int njobs, idir; BcJob job[6]; CorrView V; };

__global__ __launch_bounds__(256) void k_set_bc(Geom g, BcJobs J) {
  const BcJob jb = J.job[blockIdx.z];
  const int idir = J.idir;
  const int na = idir == 1 ? g.n2 : g.n1, nb = idir == 3 ? g.n2 : g.n3, n = idir == 1 ? g.n1 : idir == 2 ? g.n2 : g.n3;
  const int a = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y * 4 + threadIdx.y;
  if (a > na + 1 || b > nb + 1) return;
  const long st = idir == 1 ? 1 : idir == 2 ? (long)g.s1 : g.s12;
  const size_t base = idir == 1 ? g.ix(0, a, b) : idir == 2 ? g.ix(a, 0, b) : g.ix(a, b, 0);
  real *p = jb.p + base;
#define P(m) p[(long)(m)*st]
  // sources (cells 1, n-1, n of the line): through the corrected view when the job asks for it
  auto R = [&](int m) -> real {
    if (!jb.vcomp) return P(m);
    return idir == 1 ? view_rd(g, J.V, jb.vcomp, jb.p, m, a, b) : idir == 2 ? view_rd(g, J.V, jb.vcomp, jb.p, a, m, b) : view_rd(g, J.V, jb.vcomp, jb.p, a, b, m);
  };
  const real bcv = jb.bc ? jb.bc[a + (size_t)(na + 2) * b] : 0.;
  const real sgn = (jb.ctype == 'D' && jb.centered) ? -1. : 1.;
  switch (jb.ctype) {
  case 'P':   // bound.f90:220-248 (one job handles both ends)
    { const real lo = R(n), hi = R(1); P(0) = lo; P(n + 1) = hi; } break;
  case 'D':   // bound.f90:249-319
    if (jb.centered) { if (jb.ibound == 0) P(0) = 2. * bcv + sgn * R(1); else P(n + 1) = 2. * bcv + sgn * R(n); }
    else { if (jb.ibound == 0) P(0) = bcv; else { P(n + 1) = R(n - 1); P(n) = bcv; } }
    break;
  case 'N':   // bound.f90:320-396
    if (jb.centered) { if (jb.ibound == 0) P(0) = -jb.dr * bcv + sgn * R(1); else P(n + 1) = jb.dr * bcv + sgn * R(n); }
    else { if (jb.ibound == 0) P(0) = -jb.dr * bcv + R(1); else { P(n + 1) = R(n); P(n) = jb.dr * bcv + R(n - 1); } }
    break;
  }
#undef P
}

static int launch_jobs(cales_ctx *c, BcJobs &J) {
  if (J.njobs == 0) return 0;
  const int na = J.idir == 1 ? c->n[1] : c->n[0], nb = J.idir == 3 ? c->n[1] : c->n[2];
  dim3 b(64, 4, 1), gr((na + 2 + 63) / 64, (nb + 2 + 3) / 4, J.njobs);
  LAUNCH(c, k_set_bc, gr, b, 0, c->stream, c->g, J);
  LAUNCHCHK(c);
  return 0;
}
static inline const real *plane(const DBound &b, int idir, int ibound, const int *n) {
  const size_t pl = idir == 1 ? (size_t)(n[1] + 2) * (n[2] + 2) : idir == 2 ? (size_t)(n[0] + 2) * (n[2] + 2) : (size_t)(n[0] + 2) * (n[1] + 2);
  const real *base = idir == 1 ? b.x : idir == 2 ? b.y : b.z;
  return base + (size_t)ibound * pl;
}

// ---- all three directions in ONE launch, for the common BC sets: x periodic, y periodic (or exchanged between slabs), any
// pointwise z condition. The reference applies x, then y, then z, and later directions also fill the corner ghosts of earlier ones
// (bound.f90:158-199). With periodic x and y that sequence is a composition with a closed form -- every ghost cell is the z
// operation applied to the periodically wrapped interior cell -- so each thread computes its ghost cell from interior cells only
// and no ordering between the directions is left. Saves two of the three launches of every bounduvw / boundp (19 -> 7 per substep
// for a channel), which is what small grids are bound by.
struct MField { real *p; const real *bc0, *bc1; real dr0, dr1; char t0, t1, centered, vcomp = 0; };      // vcomp != 0: sources through the corrected view (CorrView) of this velocity component      // z sides: 'P','D','N' or 0 (leave z alone)
struct MJobs { int nf, do_x, wrap_y, do_z; MField f[8]; CorrView V; };
__global__ __launch_bounds__(256) void k_bc_merged(Geom g, MJobs J) {
  const int region = blockIdx.z % 3; const MField F = J.f[blockIdx.z / 3];
  const int n1 = g.n1, n2 = g.n2, n3 = g.n3;
  const int a = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y * 4 + threadIdx.y;
  auto wx = [&](int i) { return !J.do_x ? i : i == 0 ? n1 : i == n1 + 1 ? 1 : i; };
  auto wy = [&](int j) { return !J.wrap_y ? j : j == 0 ? n2 : j == n2 + 1 ? 1 : j; };
  const bool top_face = J.do_z && F.t1 == 'D' && !F.centered;      // plane n3 itself is boundary data (face-centred normal component)
  const bool zset0 = J.do_z && F.t0 != 0, zset1 = J.do_z && F.t1 != 0;      // the z condition sets the ghost plane below / above
  real *p = F.p;
  auto S = [&](int i, int j, int k) -> real { return F.vcomp ? view_rd(g, J.V, F.vcomp, F.p, i, j, k) : F.p[g.ix(i, j, k)]; };      // sources
  if (region == 0) {               // z ghost planes of the column (a, b), ghost columns included
    if (!J.do_z || a > n1 + 1 || b > n2 + 1) return;
    const int ia = wx(a), jb = wy(b);
    const size_t q2 = (size_t)a + (size_t)(n1 + 2) * b;
    if (F.t0 == 'P') { p[g.ix(a, b, 0)] = S(ia, jb, n3); p[g.ix(a, b, n3 + 1)] = S(ia, jb, 1); return; }
    if (F.t0 == 'D') p[g.ix(a, b, 0)] = F.centered ? 2. * F.bc0[q2] - S(ia, jb, 1) : F.bc0[q2];
    else if (F.t0 == 'N') p[g.ix(a, b, 0)] = -F.dr0 * F.bc0[q2] + S(ia, jb, 1);
    if (F.t1 == 'D') {
      if (F.centered) p[g.ix(a, b, n3 + 1)] = 2. * F.bc1[q2] - S(ia, jb, n3);
      else { p[g.ix(a, b, n3 + 1)] = S(ia, jb, n3 - 1); p[g.ix(a, b, n3)] = F.bc1[q2]; }
    } else if (F.t1 == 'N') p[g.ix(a, b, n3 + 1)] = F.dr1 * F.bc1[q2] + S(ia, jb, n3);
  } else if (region == 1) {        // x ghost columns of the rows (b, k) (ghost rows included), in every plane the z condition does not set -- the ghost planes too
    // where z is left alone (the corrected normal velocity, skipped directions): the reference's x and y copies run over whole planes (bound.f90:158-199)
    const int bb = a, k = b;       // lanes along y (rows 4 KB apart share DRAM pages; along z they would be a plane apart), blocks along z
    if (!J.do_x || k > n3 + 1 || bb > n2 + 1 || (top_face && k == n3) || (k == 0 && zset0) || (k == n3 + 1 && zset1)) return;
    const int jb = wy(bb);
    p[g.ix(0, bb, k)] = S(n1, jb, k); p[g.ix(n1 + 1, bb, k)] = S(1, jb, k);
  } else {                         // y ghost rows, i = 1..n1, the same planes
    const int i = a + 1, k = b;
    if (!J.wrap_y || i > n1 || k > n3 + 1 || (top_face && k == n3) || (k == 0 && zset0) || (k == n3 + 1 && zset1)) return;
    p[g.ix(i, 0, k)] = S(i, n2, k); p[g.ix(i, n2 + 1, k)] = S(i, 1, k);
  }
}
static int launch_merged(cales_ctx *c, MJobs &J, const Geom &G) {      // (G: the context's geometry or its doubled-width view, wide_geom)
  if (!J.nf) return 0;
  const int n[3] = {G.n1, G.n2, G.n3};
  // one grid for the three regions: region 0 needs (n1+2) x (n2+2), region 1 (n2+2) x n3, region 2 n1 x n3 threads
  const int ex = std::max(n[0] + 2, n[1] + 2), ey = std::max(n[1] + 2, n[2] + 2);
  LAUNCH(c, k_bc_merged, dim3((ex + 63) / 64, (ey + 3) / 4, 3 * J.nf), dim3(64, 4, 1), 0, c->stream, G, J);
  LAUNCHCHK(c);
  return 0;
}
// ---- ANY set of pointwise conditions (periodic, Dirichlet, Neumann on cell-centred data, Dirichlet on face-centred data) in all three directions in ONE
// launch: ducts, cavities, half channels -- the cases k_bc_merged (periodic x and y) leaves to one k_set_bc launch per direction. The reference applies
// x, then y, then z over WHOLE planes (bound.f90:158-199, set_bc: ghost rows and planes of the other directions included), so a later direction also
// rewrites the edge and corner cells of an earlier one from the values that one left. Every rule is "target = c bc + s source" with ONE source cell
// (set_bc, bound.f90:202-399), so that sequence has a closed form: the value of a cell the z rule sets is the z rule applied to the value the x and y
// rules leave in its source cell, and so on down to a cell no rule sets -- Z(Y(X(stored))) with each rule's boundary value taken where the reference
// takes it (the plane entry of the cell being set, ghost positions included). A thread computes its cell from stored cells no thread writes: no
// ordering between the directions is left. Not served: Neumann on face-centred data (outflow: set_bc copies the OLD boundary value into the ghost
// cell while it rewrites the boundary value itself) -- such sets keep the launch per direction.
using ADir = BcRule;      // (common.hpp; t = 0: this end is left alone; 'P': both ends; cen = 0: face-centred along this direction)
struct AField { real *p; ADir d[3]; char vcomp; };      // vcomp != 0: stored cells through the corrected view of this velocity component
struct AJobs { int nf; AField f[6]; CorrView V; };
__device__ inline bool a_set(const ADir &R, int idx, int n) {
  if (idx == 0) return R.t0 != 0;
  if (idx == n + 1) return R.t1 != 0;
  return idx == n && !R.cen && R.t1 == 'D';
}
// the rule of direction R for the cell at index idx (in 0, n, n+1): value = c * bc(side) + s * value(src)
__device__ inline void a_rule(const ADir &R, int idx, int n, real &c, real &s, int &src, int &side) {
  if (idx == 0) {
    side = 0; src = 1;
    if (R.t0 == 'P') { c = 0.; s = 1.; src = n; }
    else if (R.t0 == 'D') { if (R.cen) { c = 2.; s = -1.; } else { c = 1.; s = 0.; } }
    else { c = -R.dr0; s = 1.; }                                              // 'N', cell-centred: bound.f90:320-348
  } else {
    side = 1; src = n;
    if (R.t1 == 'P') { c = 0.; s = 1.; src = 1; }
    else if (R.t1 == 'D') { if (R.cen) { c = 2.; s = -1.; } else if (idx == n) { c = 1.; s = 0.; } else { c = 0.; s = 1.; src = n - 1; } }
    else { c = R.dr1; s = 1.; }
  }
}
__global__ __launch_bounds__(256) void k_bc_all(Geom g, AJobs J) {
  const int region = blockIdx.z % 3; const AField F = J.f[blockIdx.z / 3];
  const int n1 = g.n1, n2 = g.n2, n3 = g.n3;
  const int a = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y * 4 + threadIdx.y;
  real *p = F.p;
  auto S = [&](int i, int j, int k) -> real { return F.vcomp ? view_rd(g, J.V, F.vcomp, F.p, i, j, k) : F.p[g.ix(i, j, k)]; };      // stored cells
  auto VX = [&](int i, int j, int k) -> real {      // what the x rules leave at (i, j, k)
    const ADir &R = F.d[0];
    if (!a_set(R, i, n1)) return S(i, j, k);
    real c, s_; int src, side; a_rule(R, i, n1, c, s_, src, side);
    const real *bc = side ? R.bc1 : R.bc0;
    real v = (c != 0. && bc) ? c * bc[j + (size_t)(n2 + 2) * k] : 0.;
    if (s_ != 0.) v += s_ * S(src, j, k);
    return v;
  };
  auto VY = [&](int i, int j, int k) -> real {      // ... the x and y rules
    const ADir &R = F.d[1];
    if (!a_set(R, j, n2)) return VX(i, j, k);
    real c, s_; int src, side; a_rule(R, j, n2, c, s_, src, side);
    const real *bc = side ? R.bc1 : R.bc0;
    real v = (c != 0. && bc) ? c * bc[i + (size_t)(n1 + 2) * k] : 0.;
    if (s_ != 0.) v += s_ * VX(i, src, k);
    return v;
  };
  auto VZ = [&](int i, int j, int k) -> real {      // ... all three
    const ADir &R = F.d[2];
    if (!a_set(R, k, n3)) return VY(i, j, k);
    real c, s_; int src, side; a_rule(R, k, n3, c, s_, src, side);
    const real *bc = side ? R.bc1 : R.bc0;
    real v = (c != 0. && bc) ? c * bc[i + (size_t)(n1 + 2) * j] : 0.;
    if (s_ != 0.) v += s_ * VY(i, j, src);
    return v;
  };
  // the (up to three) indices a direction sets: 0, n+1 and, for face-centred Dirichlet data, n
  if (region == 0) {               // planes the z rules set, every (i, j) of the plane
    if (a > n1 + 1 || b > n2 + 1) return;
    const int ks[3] = {0, n3 + 1, n3};
#pragma unroll
    for (int q = 0; q < 3; ++q) if (a_set(F.d[2], ks[q], n3)) p[g.ix(a, b, ks[q])] = VZ(a, b, ks[q]);
  } else if (region == 1) {        // rows the y rules set, in the planes the z rules leave alone
    if (a > n1 + 1 || b > n3 + 1 || a_set(F.d[2], b, n3)) return;
    const int js[3] = {0, n2 + 1, n2};
#pragma unroll
    for (int q = 0; q < 3; ++q) if (a_set(F.d[1], js[q], n2)) p[g.ix(a, js[q], b)] = VY(a, js[q], b);
  } else {                         // columns the x rules set, in the rows and planes the others leave alone
    if (a > n2 + 1 || b > n3 + 1 || a_set(F.d[1], a, n2) || a_set(F.d[2], b, n3)) return;
    const int is_[3] = {0, n1 + 1, n1};
#pragma unroll
    for (int q = 0; q < 3; ++q) if (a_set(F.d[0], is_[q], n1)) p[g.ix(is_[q], a, b)] = VX(is_[q], a, b);
  }
}
static int launch_all(cales_ctx *c, AJobs &J) {
  if (!J.nf) return 0;
  const int *n = c->n;
  const int ex = std::max(n[0] + 2, n[1] + 2), ey = std::max(n[1] + 2, n[2] + 2);
  LAUNCH(c, k_bc_all, dim3((ex + 63) / 64, (ey + 3) / 4, 3 * J.nf), dim3(64, 4, 1), 0, c->stream, c->g, J);
  LAUNCHCHK(c);
  return 0;
}
// BcPath's entry for one direction of one field: the types of its two ends as the reference's loops over idir / ibound apply them on this rank
static BcRule table_rule(const cales_ctx *c, int idir, char c0, char c1, int cen, const DBound &bc) {
  const int n3 = c->n[2];
  BcRule R{};
  R.cen = (char)cen;
  R.dr0 = idir < 3 ? c->dl[idir - 1] : cen ? c->dzc[0] : c->dzf[0]; R.dr1 = idir < 3 ? c->dl[idir - 1] : cen ? c->dzc[n3] : c->dzf[n3];
  R.bc0 = plane(bc, idir, 0, c->n); R.bc1 = plane(bc, idir, 1, c->n);
  if (c0 == 'P' && c1 == 'P') { if (!(idir == 2 && c->P > 1)) R.t0 = R.t1 = 'P'; }      // (y on several slabs: the rows are exchanged; x and z are never decomposed: a local copy)
  else { if (ISB(c, 0, idir)) R.t0 = c0; if (ISB(c, 1, idir)) R.t1 = c1; }
  return R;
}
// x periodic, y periodic on one rank or exchanged between slabs, z pointwise
static bool merged_ok(const cales_ctx *c, const char *cbx, const char *cby) {
  if (c->fl.unmerged_bc) return false;
  if (!(cbx[0] == 'P' && cbx[1] == 'P')) return false;
  if (!(cby[0] == 'P' && cby[1] == 'P')) return false;
  return true;
}
// BcPath: the form of every BC set of the case and the rules of every field kind (cales_create)
void bc_setup(cales_ctx *c) {
  BcPath &B = c->bc;
  const BcForm other = c->fl.unmerged_bc ? BcForm::by_direction : BcForm::all;
  for (int w = 0; w < 2; ++w) { const char *cb = w ? c->C.cbcsgs : c->C.cbcpre; B.cell[w] = merged_ok(c, cb, cb + 2) ? BcForm::merged : other; }
  bool merged = B.cell[0] == BcForm::merged;       // velocity and pressure are periodic together (sanity.f90:163-175)
  for (int ivel = 1; ivel <= 3 && merged; ++ivel) {
    for (int d = 1; d <= 2; ++d) merged = merged && CBV(c, 0, d, ivel) == 'P' && CBV(c, 1, d, ivel) == 'P';
    if (ivel == 3 && (CBV(c, 0, 3, 3) == 'N' || CBV(c, 1, 3, 3) == 'N')) merged = false;      // face-centred Neumann reads the plane it rewrites
  }
  B.vel = merged ? BcForm::merged : other;
  B.wm = other;      // (tangential components only: cell-centred along the wall normal, always served)
  B.vel_fcn = 0;
  for (int d = 1; d <= 3; ++d) for (int sd = 0; sd <= 1; ++sd) if (ISB(c, sd, d) && CBV(c, sd, d, d) == 'N') B.vel_fcn |= 1 << (d - 1);
  // the periodic kernel takes riders whose own set is periodic in x and y, the all-directions kernel any cell-centred set
  for (int w = 0; w < 2; ++w) B.ride[w] = merged ? B.cell[w] == BcForm::merged : B.vel == BcForm::all;
  const DBound *bvel[2][3] = {{&c->bcu, &c->bcv, &c->bcw}, {&c->bcuf, &c->bcvf, &c->bcwf}};
  for (int d = 1; d <= 3; ++d) {
    const int wm = (ISB(c, 0, d) && LWM(c, 0, d) != 0 ? 1 : 0) | (ISB(c, 1, d) && LWM(c, 1, d) != 0 ? 2 : 0);
    for (int s = 0; s < 2; ++s) for (int iv = 1; iv <= 3; ++iv) {
      B.rules_vel[s][iv - 1].d[d - 1] = table_rule(c, d, CBV(c, 0, d, iv), CBV(c, 1, d, iv), iv != d, *bvel[s][iv - 1]);
      B.rules_vel[s][iv - 1].wm[d - 1] = iv != d ? (unsigned char)wm : 0;
    }
    for (int w = 0; w < 2; ++w) B.rules_cell[w].d[d - 1] = w ? table_rule(c, d, CBS(c, 0, d), CBS(c, 1, d), 1, c->bcs) : table_rule(c, d, CBP(c, 0, d), CBP(c, 1, d), 1, c->bcp);
  }
}

// y-slab neighbours (bound.f90:619-696 for idir = 2): pack the first/last interior rows of nf fields into the
// staging buffer A, let the host exchange them, unpack into the ghost rows. Planes include the x/z ghosts.
constexpr int HP = StageLayout::MAXPLANES;
struct HaloFields { int nf; real *p[HP]; unsigned char wide[HP]; int off[HP]; unsigned char vcomp[HP]; unsigned char rofs[HP]; real *dst[HP]; CorrView V; };      // rofs / dst: rows 1 + rofs and n2 - rofs leave, into the ghost rows of dst (a companion field; rofs = 0: the field itself)      // vcomp != 0: the rows that leave are read through the corrected view      // wide: a pair field (rows twice as long); off: first staging plane of the field, in planes of s1 (n3+2) values
// x ghost columns of the two z ghost planes, rows 0..n2+1: the corners the velocity update after the projection leaves alone (bounduvw with
// is_correc does not touch the z ghost planes of w, and the periodic copies of the step's earlier calls were skipped: cales_step, step_xskip)
__global__ __launch_bounds__(256) void k_xwrap_zghost(Geom g, HaloFields H) {
  const int j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y ? g.n3 + 1 : 0;
  if (j > g.n2 + 1) return;
  real *p = H.p[blockIdx.z];
  p[g.ix(0, j, k)] = p[g.ix(g.n1, j, k)]; p[g.ix(g.n1 + 1, j, k)] = p[g.ix(1, j, k)];
}
__global__ __launch_bounds__(256) void k_pack_y(Geom g, HaloFields H, real *__restrict__ lo, real *__restrict__ hi) {
  const int i = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z, w = H.wide[f];
  if (i >= (g.n1 + 2) << w || k > g.n3 + 1) return;
  const size_t s1 = (size_t)g.s1 << w, s12 = (size_t)g.s12 << w;
  const size_t q = (size_t)i + s1 * k + (size_t)g.s1 * (g.n3 + 2) * H.off[f];
  if (H.vcomp[f]) { lo[q] = view_rd(g, H.V, H.vcomp[f], H.p[f], i, 1, k); hi[q] = view_rd(g, H.V, H.vcomp[f], H.p[f], i, g.n2, k); return; }      // (never a pair field)
  lo[q] = H.p[f][i + s1 * (1 + H.rofs[f]) + s12 * k]; hi[q] = H.p[f][i + s1 * (g.n2 - H.rofs[f]) + s12 * k];
}
__global__ __launch_bounds__(256) void k_unpack_y(Geom g, HaloFields H, const real *__restrict__ lo, const real *__restrict__ hi, int has_lo, int has_hi) {
  const int i = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z, w = H.wide[f];
  if (i >= (g.n1 + 2) << w || k > g.n3 + 1) return;
  const size_t s1 = (size_t)g.s1 << w, s12 = (size_t)g.s12 << w;
  const size_t q = (size_t)i + s1 * k + (size_t)g.s1 * (g.n3 + 2) * H.off[f];
  if (has_lo) H.dst[f][i + s12 * k] = lo[q];
  if (has_hi) H.dst[f][i + s1 * (g.n2 + 1) + s12 * k] = hi[q];
}
// A field of PAIRS (two values per cell, SgsPath::pair) is, for every operation that copies whole rows or planes, a field of twice the width:
// 2 (n1 + 2) values per row, pitches doubled. Its x ghost "columns" mean nothing in that view -- the callers skip direction x.
static Geom wide_geom(const cales_ctx *c) { Geom g = c->g; g.n1 = 2 * c->g.n1 + 2; g.s1 = 2 * c->g.s1; g.s12 = 2 * c->g.s12; return g; }
// the staging planes a field of this kind takes in each block, and the companion whose ghost rows its rows arrive in (0: the field's own)
static int halo_planes(HaloRows k) { return k == HaloRows::pair ? 2 : 1; }
static int halo_companion(HaloRows k) { return k == HaloRows::second_rows ? 1 : k == HaloRows::third_rows ? 2 : 0; }
// ONE exchange of the rows of nf entries: pack into the lo | hi blocks of A, the hook -- in order on the context's stream, or its second-stream form on the
// second stream --, unpack the blocks of B into the ghost rows (StageLayout::blocks). vcomp[q] != 0 in a call that carries a corrected view: the rows of field q
// that leave are those of this component of the projected velocity (nullptr: none)
static int halo_exchange(cales_ctx *c, int nf, real *const *flds, const HaloRows *kinds, bool second_stream, const BcCall &b = BcCall(), const unsigned char *vcomp = nullptr) {
  const Geom &G = c->g; const Comm &m = c->comm;
  HaloFields H; H.nf = nf; int planes = 0, anyw = 0;
  for (int q = 0; q < nf; ++q) planes += halo_planes(kinds[q]);
  if (planes > StageLayout::MAXPLANES) { c->err = "halo staging buffer too small"; return 1; }      // (the arrays of HaloFields and the blocks of the layout)
  for (int q = 0, at = 0; q < nf; at += halo_planes(kinds[q++])) {
    const int comp = halo_companion(kinds[q]);
    H.p[q] = flds[q]; H.wide[q] = kinds[q] == HaloRows::pair; H.off[q] = at; anyw |= H.wide[q]; H.vcomp[q] = 0;
    H.rofs[q] = (unsigned char)comp; H.dst[q] = flds[q] + (size_t)comp * c->comp_one;
  }
  if (b.view_dtrk != 0. && vcomp) {      // op_bounduvw through the corrected view
    H.V = corr_view(c, b);
    for (int q = 0; q < nf; ++q) if (!H.rofs[q]) H.vcomp[q] = vcomp[q];
  }
  const StageLayout::Blocks S = c->stage.blocks(planes);
  const hipStream_t st = second_stream ? c->comm_stream : c->stream;
  dim3 blk(64, 4, 1), gr(((G.s1 << anyw) + 63) / 64, (c->n[2] + 2 + 3) / 4, nf);
  LAUNCH(c, k_pack_y, gr, blk, 0, st, G, H, m.A + S.lo, m.A + S.hi);
  { ProfScope ps(c, "halo_exchange", st);
    const int rc = second_stream ? m.halo_s(m.user, S.lo, S.hi, S.lo, S.hi, S.count, (void *)st) : m.halo(m.user, S.lo, S.hi, S.lo, S.hi, S.count);
    if (rc) { c->err = "halo callback failed"; return 1; } }
  LAUNCH(c, k_unpack_y, gr, blk, 0, st, G, H, m.B + S.lo, m.B + S.hi, m.has_lo ? 1 : 0, m.has_hi ? 1 : 0);
  LAUNCHCHK(c);
  return 0;
}
// The rows of nf fields of one kind: nothing where the ghost rows already hold them (BcCall::rows_current), into the caller's batch (BcCall::collect, exchanged
// later by halo_flush -- without a view: vcomp goes with an exchange made now), or exchanged now, in order
int halo_rows(cales_ctx *c, int nf, real **flds, HaloRows kind, const BcCall &b, const unsigned char *vcomp) {
  if (int e = require_hooks(c)) return e;
  if (halo_companion(kind) && !c->comp_one) { c->err = "halo_rows: no companion fields"; return 1; }
  if (b.rows_current) return 0;
  if ((b.collect ? b.collect->n : 0) + nf > StageLayout::MAXPLANES) { c->err = "halo batch full"; return 1; }
  if (b.collect) {
    HaloBatch &R = *b.collect;
    for (int q = 0; q < nf; ++q) { R.p[R.n] = flds[q]; R.kind[R.n++] = kind; }
    return 0;
  }
  HaloRows k[StageLayout::MAXPLANES]; for (int q = 0; q < nf; ++q) k[q] = kind;
  return halo_exchange(c, nf, flds, k, false, b, vcomp);
}
// The rows collected in `rows` (BcCall::collect), as many fields per exchange as the staging buffers hold. second_stream: they travel on the second stream,
// after everything queued on the context's stream so far (their ghost-cell kernels included: what those wrote into the ghost rows is overwritten by the rows
// that arrive, whose own x/z ghost cells the neighbour has already set -- the same values the in-order sequence produces), and the caller makes the
// context's stream wait (stream_after) before the first kernel that reads those ghost rows. Otherwise the same batching in order on the context's stream
int halo_flush(cales_ctx *c, HaloBatch &rows, bool second_stream) {
  if (!rows.n) return 0;
  if (second_stream) { if (int e = stream_after(c, c->comm_stream, c->stream)) return e; }
  for (int q0 = 0; q0 < rows.n;) {
    int nf = 0, planes = 0;
    while (q0 + nf < rows.n && planes + halo_planes(rows.kind[q0 + nf]) <= StageLayout::MAXPLANES) planes += halo_planes(rows.kind[q0 + nf++]);
    if (int e = halo_exchange(c, nf, rows.p + q0, rows.kind + q0, second_stream)) return e;
    q0 += nf;
  }
  rows.n = 0;
  return 0;
}
// ------------------------------------------------------------------------------------------ one ghost-cell update
// An entry of an update: the field, its rules in BcPath's tables and, in a call that carries a corrected view, the velocity component the field holds
// the prediction of (0: plain reads) -- stated by whoever lists the entry, never inferred from the pointer
struct BcEntry { real *p; const BcRules *r; char vcomp; };
// What one update takes from its call: the skipped directions (bc_skipped), bounduvw's is_correc, the update of the wall-model faces that follows the
// wall model instead of the main one, a pair field in the doubled-width view
struct BcUse { int skipped = 0; bool is_correc = false, wm_faces = false, wide = false; };
// does the update serve direction d (0..2) at all? A periodic z is copied even where z is "skipped": the skip is for wall planes nobody reads. Pair fields:
// direction x is the consumers' business (they wrap around) and pointwise z conditions would need the BC planes in the doubled view (the callers skip z at walls)
static bool dir_on(const BcUse &u, int d, bool periodic) {
  if (u.wide && (d == 0 || (d == 2 && !periodic))) return false;
  return !(u.skipped >> d & 1) || (d == 2 && periodic);
}
// THE place where a call changes a rule of the tables: direction d of field T as this update applies it
static BcRule bc_rule(const BcRules &T, int d, const BcUse &u) {
  BcRule R = T.d[d];
  const bool periodic = R.t0 == 'P';
  int off = T.wm[d];                                                              // main update: the wall-model ends are set afterwards, from the wall-model stress
  if (u.wm_faces) off = ~T.wm[d];                                                 // ... by this update: those ends and nothing else (bound.f90:125-148)
  else if (!dir_on(u, d, periodic) || (u.is_correc && !R.cen && !periodic)) off = 3;      // the corrected normal velocity keeps its wall value (bound.f90:60-75)
  if (off & 1) R.t0 = 0;
  if (off & 2) R.t1 = 0;
  return R;
}
// x, y periodic: every entry in one launch (k_bc_merged). The three flags are what the call leaves on of each direction
static int update_merged(cales_ctx *c, int ne, const BcEntry *e, const BcUse &u, const CorrView &V) {
  MJobs J; J.nf = ne; J.V = V;
  J.do_x = dir_on(u, 0, true); J.wrap_y = c->P == 1 && dir_on(u, 1, true); J.do_z = dir_on(u, 2, e[0].r->d[2].t0 == 'P');
  if (u.wide && !J.wrap_y && !J.do_z) return 0;
  for (int q = 0; q < ne; ++q) {
    const BcRule z = bc_rule(*e[q].r, 2, u);
    MField &F = J.f[q]; F.p = e[q].p; F.bc0 = z.bc0; F.bc1 = z.bc1; F.dr0 = z.dr0; F.dr1 = z.dr1; F.t0 = z.t0; F.t1 = z.t1; F.centered = z.cen; F.vcomp = e[q].vcomp;
  }
  return launch_merged(c, J, u.wide ? wide_geom(c) : c->g);
}
// any pointwise set: six entries per launch (k_bc_all); the update of the wall-model faces only where some end is on
static int update_all(cales_ctx *c, int ne, const BcEntry *e, const BcUse &u, const CorrView &V) {
  for (int q0 = 0; q0 < ne; q0 += 6) {
    AJobs J; J.nf = std::min(6, ne - q0); J.V = V; bool any = false;
    for (int q = 0; q < J.nf; ++q) {
      AField &F = J.f[q]; F.p = e[q0 + q].p; F.vcomp = e[q0 + q].vcomp;
      for (int d = 0; d < 3; ++d) { F.d[d] = bc_rule(*e[q0 + q].r, d, u); any = any || F.d[d].t0 || F.d[d].t1; }
    }
    if (u.wm_faces && !any) continue;
    if (int er = launch_all(c, J)) return er;
  }
  return 0;
}
// the reference's order, one k_set_bc launch per direction and at most six jobs per launch: first the periodic copies of y (one rank) and z, the image of
// updthalo (bound.f90:619-696: neighbours of the non-pencil directions), then x -> y -> z for everything else. A 'P' is one job for both ends; the
// two ends of an entry stay in one launch
static int update_by_direction(cales_ctx *c, int ne, const BcEntry *e, const BcUse &u, const CorrView &V) {
  for (int pass = 0; pass < 2; ++pass)
    for (int d = pass ? 0 : 1; d < 3; ++d) {
      BcJobs J; J.njobs = 0; J.idir = d + 1; J.V = V;
      for (int q = 0; q < ne; ++q) {
        const BcRule R = bc_rule(*e[q].r, d, u);
        const bool copy = d > 0 && R.t0 == 'P';
        if (copy != (pass == 0)) continue;
        if (J.njobs + (copy ? 1 : 2) > 6) { if (int er = launch_jobs(c, J)) return er; J.njobs = 0; }
        auto add = [&](char t, int ib, const real *bc, real dr) {
          BcJob &j = J.job[J.njobs++];
          j.p = e[q].p; j.bc = bc; j.dr = dr; j.ctype = t; j.centered = R.cen; j.ibound = (char)ib; j.vcomp = e[q].vcomp;
        };
        if (R.t0 == 'P') { add('P', 0, nullptr, 0.); continue; }
        if (R.t0) add(R.t0, 0, R.bc0, R.dr0);
        if (R.t1) add(R.t1, 1, R.bc1, R.dr1);
      }
      if (int er = launch_jobs(c, J)) return er;
    }
  return 0;
}
// ne <= 8 entries in the form `form`: the rows of the slab neighbours (in one exchange; not for the wall-model faces, which follow an update that had
// it), then the ghost cells in as few launches as the form's job table allows
static int bc_update(cales_ctx *c, int ne, const BcEntry *e, BcForm form, const BcUse &u, const BcCall &b) {
  if (ne > 8) { c->err = "a ghost-cell update takes at most eight fields"; return 1; }
  if (c->P > 1 && !u.wm_faces) {
    real *p[8]; unsigned char vc[8];
    for (int q = 0; q < ne; ++q) { p[q] = e[q].p; vc[q] = (unsigned char)e[q].vcomp; }
    if (int er = halo_rows(c, ne, p, u.wide ? HaloRows::pair : HaloRows::field, b, vc)) return er;
  }
  // corrected view (cales_step, fold_mom): the fields hold the prediction, the ghost cells receive the values of the projected velocity
  const CorrView V = b.view_dtrk != 0. ? corr_view(c, b) : CorrView{};
  return form == BcForm::merged ? update_merged(c, ne, e, u, V) : form == BcForm::all ? update_all(c, ne, e, u, V) : update_by_direction(c, ne, e, u, V);
}

// ------------------------------------------------------------------------------------------ boundp (bound.f90:156-200)
static int cell_update(cales_ctx *c, int nf, real **p, int which, const BcCall &b, bool wide) {
  BcEntry e[8];
  for (int q = 0; q < nf && q < 8; ++q) e[q] = BcEntry{p[q], &c->bc.rules_cell[which], 0};
  BcUse u; u.skipped = bc_skipped(c, b); u.wide = wide;
  return bc_update(c, nf, e, c->bc.cell[which], u, b);
}
// pair fields (x and y periodic only: SgsPath::pair): the y rows (wrapped on one rank, exchanged between slabs) and the z ghost planes where z is periodic,
// through the one-launch kernel in the doubled-width view
int op_boundp_wide(cales_ctx *c, int nf, real **p2, int which, const BcCall &b) {
  ProfScope ps(c, "boundp");
  if (c->bc.cell[which] != BcForm::merged || nf > 8 || !(bc_skipped(c, b) & 1)) { c->err = "pair fields need periodic x and y and a caller that skips direction x"; return 1; }
  return cell_update(c, nf, p2, which, b, true);
}
// nf <= 8 fields with the same BC set (which: 0 pressure, 1 sgs) in one halo exchange and as few launches as the job table allows
int op_boundp_multi(cales_ctx *c, int nf, real **p, int which, const BcCall &b) {
  ProfScope ps(c, "boundp");
  return cell_update(c, nf, p, which, b, false);
}
int op_boundp(cales_ctx *c, real *p, int which, const BcCall &b) { real *fl[1] = {p}; return op_boundp_multi(c, 1, fl, which, b); }

// ------------------------------------------------------------------------------------------ wall model (wmodel.f90:65-335)
__device__ inline real vel_relative(real v1, real v2, real coef, real mag) {
  real r = (1. - coef) * v1 + coef * v2;
  return r - mag;
}
__device__ inline void wallmodel(int mtype, real uh, real vh, real h, real l1d, real visc, real &t1, real &t2) {
  const real kap = 0.41, blog = 5.20;
  real upar = sqrt(uh * uh + vh * vh), tauw_tot = 0.;      // (mtype: 1 or -1, hs_check_case; the reference's select has no other branch)
  if (mtype == 1) {
    real conv = 1., utau = fmax(sqrt(upar / h * visc), visc / h * exp(-kap * blog));
    while (conv > 0.5e-4) {
      const real utau_old = utau;
      const real f = upar / utau - 1. / kap * log(h * utau / visc) - blog;
      const real fp = -1. / utau * (upar / utau + 1. / kap);
      utau = fabs(utau - f / fp);
      conv = fabs(utau / utau_old - 1.);
    }
    tauw_tot = utau * utau;
  } else if (mtype == -1) {      // WM_LAM, wmodel.f90:303
    const real del = 0.5 * l1d, umax = upar / (h / del * (2. - h / del));
    tauw_tot = 2. / del * umax * visc;
  }
  t1 = tauw_tot * uh / (upar + CALES_EPS); t2 = tauw_tot * vh / (upar + CALES_EPS);
}

struct WmArgs {
  int idir, ibound, mtype, i1, i2;   // i1/i2: near / far interpolation index along idir
  real coef, sgn, h, l1d, visc;
  const real *u, *v, *w;           // velocity fields
  real *bc_a, *bc_b;               // planes (side ibound) receiving the first / second tangential component
  const real *mag_a, *mag_b;       // *_mag planes (side ibound)
  const real *zc, *zf, *dzc;
};
// All wall-model faces of a bounduvw in one launch (a channel has two, a duct four): blockIdx.z = 2 face + component; the grid spans the
// largest face and the blocks beyond a smaller one return.
// component 0: first tangential component loop, 1: second (wmodel.f90:138-153/154-170, 189-204/205-221, 240-255/256-271)
struct WmJobs { WmArgs a[6]; int n; };
__global__ __launch_bounds__(256) void k_wallmodel(Geom g, WmJobs J) {
  const WmArgs &A = J.a[blockIdx.z >> 1];
  const int na = A.idir == 1 ? g.n2 : g.n1, nb = A.idir == 3 ? g.n2 : g.n3;
  const int a = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y * 4 + threadIdx.y, comp = blockIdx.z & 1;
  if (a > na + 1 || b > nb + 1) return;
  const size_t ld = na + 2;
  const real visci = 1. / A.visc;
  real t1, t2;
#define M(pl, a_, b_) pl[(a_) + ld * (b_)]
  if (A.idir == 1) {          // wall normal x; a = j, b = k; tangential: v (first), w (second)
    const int i1 = A.i1, i2 = A.i2;
    if (comp == 0) {
      if (a > na || b < 1 || b > nb) return;           // j = 0..n2, k = 1..n3
      const int j = a, k = b;
      const real v1 = A.v[g.ix(i1, j, k)], v2 = A.v[g.ix(i2, j, k)];
      const real w1 = 0.25 * (A.w[g.ix(i1, j, k)] + A.w[g.ix(i1, j + 1, k)] + A.w[g.ix(i1, j, k - 1)] + A.w[g.ix(i1, j + 1, k - 1)]);
      const real w2 = 0.25 * (A.w[g.ix(i2, j, k)] + A.w[g.ix(i2, j + 1, k)] + A.w[g.ix(i2, j, k - 1)] + A.w[g.ix(i2, j + 1, k - 1)]);
      const real v_mag = M(A.mag_a, j, k), w_mag = 0.25 * (M(A.mag_b, j, k) + M(A.mag_b, j + 1, k) + M(A.mag_b, j, k - 1) + M(A.mag_b, j + 1, k - 1));
      wallmodel(A.mtype, vel_relative(v1, v2, A.coef, v_mag), vel_relative(w1, w2, A.coef, w_mag), A.h, A.l1d, A.visc, t1, t2);
      M(A.bc_a, j, k) = A.sgn * visci * t1;
    } else {
      if (a < 1 || a > na || b > nb) return;           // j = 1..n2, k = 0..n3
      const int j = a, k = b;
      const real wei = (A.zf[k] - A.zc[k]) / A.dzc[k];
      const real v1 = 0.5 * ((1. - wei) * (A.v[g.ix(i1, j - 1, k)] + A.v[g.ix(i1, j, k)]) + wei * (A.v[g.ix(i1, j - 1, k + 1)] + A.v[g.ix(i1, j, k + 1)]));
      const real v2 = 0.5 * ((1. - wei) * (A.v[g.ix(i2, j - 1, k)] + A.v[g.ix(i2, j, k)]) + wei * (A.v[g.ix(i2, j - 1, k + 1)] + A.v[g.ix(i2, j, k + 1)]));
      const real w1 = A.w[g.ix(i1, j, k)], w2 = A.w[g.ix(i2, j, k)];
      const real v_mag = 0.5 * ((1. - wei) * (M(A.mag_a, j - 1, k) + M(A.mag_a, j, k)) + wei * (M(A.mag_a, j - 1, k + 1) + M(A.mag_a, j, k + 1)));
      const real w_mag = M(A.mag_b, j, k);
      wallmodel(A.mtype, vel_relative(v1, v2, A.coef, v_mag), vel_relative(w1, w2, A.coef, w_mag), A.h, A.l1d, A.visc, t1, t2);
      M(A.bc_b, j, k) = A.sgn * visci * t2;
    }
  } else if (A.idir == 2) {   // wall normal y; a = i, b = k; tangential: u (first), w (second)
    const int j1 = A.i1, j2 = A.i2;
    if (comp == 0) {
      if (a > na || b < 1 || b > nb) return;           // i = 0..n1, k = 1..n3
      const int i = a, k = b;
      const real u1 = A.u[g.ix(i, j1, k)], u2 = A.u[g.ix(i, j2, k)];
      const real w1 = 0.25 * (A.w[g.ix(i, j1, k)] + A.w[g.ix(i + 1, j1, k)] + A.w[g.ix(i, j1, k - 1)] + A.w[g.ix(i + 1, j1, k - 1)]);
      const real w2 = 0.25 * (A.w[g.ix(i, j2, k)] + A.w[g.ix(i + 1, j2, k)] + A.w[g.ix(i, j2, k - 1)] + A.w[g.ix(i + 1, j2, k - 1)]);
      const real u_mag = M(A.mag_a, i, k), w_mag = 0.25 * (M(A.mag_b, i, k) + M(A.mag_b, i + 1, k) + M(A.mag_b, i, k - 1) + M(A.mag_b, i + 1, k - 1));
      wallmodel(A.mtype, vel_relative(u1, u2, A.coef, u_mag), vel_relative(w1, w2, A.coef, w_mag), A.h, A.l1d, A.visc, t1, t2);
      M(A.bc_a, i, k) = A.sgn * visci * t1;
    } else {
      if (a < 1 || a > na || b > nb) return;           // i = 1..n1, k = 0..n3
      const int i = a, k = b;
      const real wei = (A.zf[k] - A.zc[k]) / A.dzc[k];
      const real u1 = 0.5 * ((1. - wei) * (A.u[g.ix(i - 1, j1, k)] + A.u[g.ix(i, j1, k)]) + wei * (A.u[g.ix(i - 1, j1, k + 1)] + A.u[g.ix(i, j1, k + 1)]));
      const real u2 = 0.5 * ((1. - wei) * (A.u[g.ix(i - 1, j2, k)] + A.u[g.ix(i, j2, k)]) + wei * (A.u[g.ix(i - 1, j2, k + 1)] + A.u[g.ix(i, j2, k + 1)]));
      const real w1 = A.w[g.ix(i, j1, k)], w2 = A.w[g.ix(i, j2, k)];
      const real u_mag = 0.5 * ((1. - wei) * (M(A.mag_a, i - 1, k) + M(A.mag_a, i, k)) + wei * (M(A.mag_a, i - 1, k + 1) + M(A.mag_a, i, k + 1)));
      const real w_mag = M(A.mag_b, i, k);
      wallmodel(A.mtype, vel_relative(u1, u2, A.coef, u_mag), vel_relative(w1, w2, A.coef, w_mag), A.h, A.l1d, A.visc, t1, t2);
      M(A.bc_b, i, k) = A.sgn * visci * t2;
    }
  } else {                    // wall normal z; a = i, b = j; tangential: u (first), v (second)
    const int k1 = A.i1, k2 = A.i2;
    if (comp == 0) {
      if (a > na || b < 1 || b > nb) return;           // i = 0..n1, j = 1..n2
      const int i = a, j = b;
      const real u1 = A.u[g.ix(i, j, k1)], u2 = A.u[g.ix(i, j, k2)];
      const real v1 = 0.25 * (A.v[g.ix(i, j, k1)] + A.v[g.ix(i + 1, j, k1)] + A.v[g.ix(i, j - 1, k1)] + A.v[g.ix(i + 1, j - 1, k1)]);
      const real v2 = 0.25 * (A.v[g.ix(i, j, k2)] + A.v[g.ix(i + 1, j, k2)] + A.v[g.ix(i, j - 1, k2)] + A.v[g.ix(i + 1, j - 1, k2)]);
      const real u_mag = M(A.mag_a, i, j), v_mag = 0.25 * (M(A.mag_b, i, j) + M(A.mag_b, i + 1, j) + M(A.mag_b, i, j - 1) + M(A.mag_b, i + 1, j - 1));
      wallmodel(A.mtype, vel_relative(u1, u2, A.coef, u_mag), vel_relative(v1, v2, A.coef, v_mag), A.h, A.l1d, A.visc, t1, t2);
      M(A.bc_a, i, j) = A.sgn * visci * t1;
    } else {
      if (a < 1 || a > na || b > nb) return;           // i = 1..n1, j = 0..n2
      const int i = a, j = b;
      const real u1 = 0.25 * (A.u[g.ix(i - 1, j, k1)] + A.u[g.ix(i, j, k1)] + A.u[g.ix(i - 1, j + 1, k1)] + A.u[g.ix(i, j + 1, k1)]);
      const real u2 = 0.25 * (A.u[g.ix(i - 1, j, k2)] + A.u[g.ix(i, j, k2)] + A.u[g.ix(i - 1, j + 1, k2)] + A.u[g.ix(i, j + 1, k2)]);
      const real v1 = A.v[g.ix(i, j, k1)], v2 = A.v[g.ix(i, j, k2)];
      const real u_mag = 0.25 * (M(A.mag_a, i - 1, j) + M(A.mag_a, i, j) + M(A.mag_a, i - 1, j + 1) + M(A.mag_a, i, j + 1));
      const real v_mag = M(A.mag_b, i, j);
      wallmodel(A.mtype, vel_relative(u1, u2, A.coef, u_mag), vel_relative(v1, v2, A.coef, v_mag), A.h, A.l1d, A.visc, t1, t2);
      M(A.bc_b, i, j) = A.sgn * visci * t2;
    }
  }
#undef M
}

static int updt_wallmodelbc(cales_ctx *c, DBound &bu, DBound &bv, DBound &bw, const real *u, const real *v, const real *w) {
  const int *n = c->n; const real h = c->C.hwm; const real *dl = c->dl;
  WmJobs J; J.n = 0; int gx = 0, gy = 0;
  for (int idir = 1; idir <= 3; ++idir) for (int ib = 0; ib <= 1; ++ib) {
    if (!(ISB(c, ib, idir) && LWM(c, ib, idir) != 0)) continue;
    WmArgs &A = J.a[J.n++]; A.idir = idir; A.ibound = ib; A.mtype = LWM(c, ib, idir); A.h = h; A.visc = c->visc; A.l1d = c->C.l[idir - 1];
    A.u = u; A.v = v; A.w = w; A.zc = c->d_zc; A.zf = c->d_zf; A.dzc = c->d_dzc;
    const int index = IWM(c, ib, idir);
    A.i2 = index; A.i1 = ib == 0 ? index - 1 : index + 1; A.sgn = ib == 0 ? 1. : -1.;
    if (idir == 1) { A.coef = ib == 0 ? (h - (A.i1 - 0.5) * dl[0]) / dl[0] : (h - (n[0] - A.i1 + 0.5) * dl[0]) / dl[0]; }
    else if (idir == 2) { A.coef = ib == 0 ? (h - (A.i1 - 0.5) * dl[1]) / dl[1] : (h - (n[1] - A.i1 + 0.5) * dl[1]) / dl[1]; }
    else { A.coef = ib == 0 ? (h - c->zc[A.i1]) / c->dzc[A.i1] : (h - (c->C.l[2] - c->zc[A.i1])) / (c->dzc[A.i2]); }
    DBound *ba = idir == 1 ? &bv : &bu, *bb = idir == 3 ? &bv : &bw;
    const DBound *ma = idir == 1 ? &c->bcv_mag : &c->bcu_mag, *mb = idir == 3 ? &c->bcv_mag : &c->bcw_mag;
    A.bc_a = const_cast<real *>(plane(*ba, idir, ib, n)); A.bc_b = const_cast<real *>(plane(*bb, idir, ib, n));
    A.mag_a = plane(*ma, idir, ib, n); A.mag_b = plane(*mb, idir, ib, n);
    const int na = idir == 1 ? n[1] : n[0], nb = idir == 3 ? n[1] : n[2];
    gx = std::max(gx, (na + 2 + 63) / 64); gy = std::max(gy, (nb + 2 + 3) / 4);
  }
  if (J.n) LAUNCH(c, k_wallmodel, dim3(gx, gy, 2 * J.n), dim3(64, 4, 1), 0, c->stream, c->g, J);
  LAUNCHCHK(c);
  return 0;
}

// ------------------------------------------------------------------------------------------ bounduvw (bound.f90:18-154)
// The three components of a velocity set, face-centred along their own direction, plus the call's riders; then, unless the call leaves the wall model
// alone, the wall-model stress (is_updt_wm) and the tangential ghost cells of the wall-model faces from it. Riders that cannot join (BcPath::ride, a
// skipped z, the per-direction form) get their own update right after.
int op_bounduvw(cales_ctx *c, VelSet set, int is_updt_wm, int is_correc, const BcCall &b) {
  const BcPath &B = c->bc;
  const bool state = set == VelSet::state, view = b.view_dtrk != 0.;
  real *fl[3] = {state ? c->f[CALES_U] : c->uf, state ? c->f[CALES_V] : c->vf, state ? c->f[CALES_W] : c->wf};
  BcEntry e[6];
  for (int iv = 0; iv < 3; ++iv) e[iv] = BcEntry{fl[iv], &B.rules_vel[(int)set][iv], (char)(state && view ? iv + 1 : 0)};
  BcUse u; u.skipped = bc_skipped(c, b); u.is_correc = is_correc != 0;
  // the form of the velocity set (BcPath): k_bc_all only while no direction of this call holds a Neumann condition on the normal component
  BcForm form = B.vel;
  if (form == BcForm::all && !is_correc && (B.vel_fcn & ~u.skipped)) form = BcForm::by_direction;
  // riders: cell-centred fields join the velocity's launch -- and its slab exchange
  int nr = 0;
  if (b.nride > 0 && form != BcForm::by_direction && !(u.skipped & 4)) {
    nr = b.nride;
    for (int q = 0; q < b.nride; ++q) if (!B.ride[b.ride_which[q]]) nr = 0;
  }
  for (int q = 0; q < nr; ++q) e[3 + q] = BcEntry{b.ride[q], &B.rules_cell[b.ride_which[q]], 0};
  { ProfScope ps(c, "bounduvw");
    if (int er = bc_update(c, 3 + nr, e, form, u, b)) return er;
    if (!b.skip_wm) {
      if (is_updt_wm) { if (int er = state ? updt_wallmodelbc(c, c->bcu, c->bcv, c->bcw, fl[0], fl[1], fl[2]) : updt_wallmodelbc(c, c->bcuf, c->bcvf, c->bcwf, fl[0], fl[1], fl[2])) return er; }
      BcUse w; w.wm_faces = true;      // tangential Neumann BCs carrying the wall-model stress (bound.f90:125-148)
      if (int er = bc_update(c, 3, e, B.wm, w, b)) return er;
    } }
  if (!b.nride || nr) return 0;
  // the riders could not join: their ghost cells now, consecutive riders of one BC set together
  BcCall alone = b; alone.nride = 0;
  for (int q0 = 0, q1; q0 < b.nride; q0 = q1) {
    real *p[3];
    for (q1 = q0; q1 < b.nride && b.ride_which[q1] == b.ride_which[q0]; ++q1) p[q1 - q0] = b.ride[q1];
    if (int er = op_boundp_multi(c, q1 - q0, p, b.ride_which[q0], alone)) return er;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ updt_rhs_b (bound.f90:562-617)
struct RhsJob { real *p; const real *rhs; int idir, pos, na, nb; };
__global__ __launch_bounds__(256) void k_updt_rhs_b(Geom g, RhsJob J) {
  const int a = blockIdx.x * 64 + threadIdx.x + 1, b = blockIdx.y * 4 + threadIdx.y + 1;
  if (a > J.na || b > J.nb) return;
  const size_t q = J.idir == 1 ? g.ix(J.pos, a, b) : J.idir == 2 ? g.ix(a, J.pos, b) : g.ix(a, b, J.pos);
  J.p[q] += J.rhs[(a - 1) + (size_t)J.na * (b - 1)];
}
static int rhs_b_dir(cales_ctx *c, real *p, int idir, const char *cbc6, const char *cf, const real *rhs) {
  const int *n = c->n;
  const int na = idir == 1 ? n[1] : n[0], nb = idir == 3 ? n[1] : n[2];
  const int q = (cf[idir - 1] == 'f' && cbc6[1 + 2 * (idir - 1)] == 'D') ? 1 : 0;
  for (int ib = 0; ib <= 1; ++ib) {
    if (!ISB(c, ib, idir)) continue;
    RhsJob J; J.p = p; J.rhs = rhs + (size_t)ib * na * nb; J.idir = idir; J.pos = ib ? n[idir - 1] - q : 1; J.na = na; J.nb = nb;
    LAUNCH(c, k_updt_rhs_b, dim3((na + 63) / 64, (nb + 3) / 4), dim3(64, 4), 0, c->stream, c->g, J);
  }
  LAUNCHCHK(c);
  return 0;
}

int op_updt_rhs_b(cales_ctx *c) {
  ProfScope ps(c, "updt_rhs_b");
  // the planes are zero for periodic and homogeneous BCs; skip those launches (adding 0. is the identity)
  for (int idir = 1; idir <= 3; ++idir) {
    const bool zero = (c->C.bcpre[0 + 2 * (idir - 1)] == 0. && c->C.bcpre[1 + 2 * (idir - 1)] == 0.) ||
                      (CBP(c, 0, idir) == 'P');
    if (zero) continue;
    if (int e = rhs_b_dir(c, c->f[CALES_PP], idir, c->C.cbcpre, "ccc", c->rhsbp[idir - 1])) return e;
  }
  return 0;
}

// z part of the Helmholtz boundary r.h.s. for one velocity component (main.f90:425-433): rhsbz computed on the
// host from the CURRENT bc planes would need a download; the planes of wall-model faces change every substep,
// so the term is evaluated on the device from the plane directly.
__global__ __launch_bounds__(256) void k_rhs_b_velz(Geom g, real *p, const real *bcplane, int ib, char ctype, char c_or_f, real dlc,
                                                    real dlf, real alpha, int pos, real *plane_out) {
  const int i = blockIdx.x * 64 + threadIdx.x + 1, j = blockIdx.y * 4 + threadIdx.y + 1;
  if (i > g.n1 || j > g.n2) return;
  const RhsBz R{bcplane, ctype, c_or_f, dlc, dlf, ib == 0 ? (real)1. : (real)-1., alpha};
  const real r = R.at(i, j, g.n1);
  if (plane_out) plane_out[(size_t)(i - 1) + (size_t)g.n1 * (j - 1)] = r;      // added by the column form of the fused Helmholtz sweep, in the reference's order
  else p[g.ix(i, j, pos)] += r;
}
// The same term on the x (idir = 1) and y (idir = 2) faces for the 3-D implicit step (main.f90:424-431: rhsbx, rhsby times alpha, added by
// updt_rhs_b to the first and the last unknown plane of the direction, bound.f90:578-603): inflow profiles, moving side walls.
__global__ __launch_bounds__(256) void k_rhs_b_velxy(Geom g, real *p, const real *bcplane, int idir, int ib, char ctype, char c_or_f, real dl,
                                                     real alpha, int pos) {
  const int a = blockIdx.x * 64 + threadIdx.x + 1, k = blockIdx.y * 4 + threadIdx.y + 1;      // a = j (x faces) or i (y faces)
  const int na = idir == 1 ? g.n2 : g.n1;
  if (a > na || k > g.n3) return;
  const real bcv = bcplane[a + (size_t)(na + 2) * k];
  const real sgn = ib == 0 ? 1. : -1.;
  real r = 0.;
  if (c_or_f == 'c') { if (ctype == 'D') r = -2. * bcv / dl / dl; else if (ctype == 'N') r = sgn * bcv / dl; }
  else               { if (ctype == 'D') r = -bcv / dl / dl;      else if (ctype == 'N') r = sgn * bcv / dl; }
  p[idir == 1 ? g.ix(pos, a, k) : g.ix(a, pos, k)] += r * alpha;
}
int op_rhs_b_velxy(cales_ctx *c, int ivel, real alpha) {
  const int *n = c->n;
  const DBound &bc = ivel == 1 ? c->bcu : ivel == 2 ? c->bcv : c->bcw;
  for (int idir = 1; idir <= 2; ++idir) {
    const char cf = ivel == idir ? 'f' : 'c';
    const char *cbc = &c->cbcvel[6 * (ivel - 1) + 2 * (idir - 1)];
    const int q = (cf == 'f' && cbc[1] == 'D') ? 1 : 0;
    const int na = idir == 1 ? n[1] : n[0];
    for (int ib = 0; ib <= 1; ++ib) {
      if (!ISB(c, ib, idir) || cbc[ib] == 'P') continue;
      LAUNCH(c, k_rhs_b_velxy, dim3((na + 63) / 64, (n[2] + 3) / 4), dim3(64, 4), 0, c->stream, c->g, c->f[CALES_U + ivel - 1],
                         plane(bc, idir, ib, n), idir, ib, cbc[ib], cf, c->dl[idir - 1], alpha, ib ? n[idir - 1] - q : 1);
    }
  }
  LAUNCHCHK(c);
  return 0;
}
// the two sides as arguments of the in-LDS sweep (no launch); has[ib]: the side exists on this rank and is not periodic
// (bound.f90:479-482: dzc01_c=[dzc(0),dzc(n)], dzf01_c=[dzf(1),dzf(n)]; dzc01_f=[dzc(1),dzc(n-1)], dzf01_f=[dzf(1),dzf(n)])
void rhs_b_velz_args(cales_ctx *c, int ivel, real alpha, RhsBz *R, int *has) {
  const int *n = c->n; const int n3 = n[2];
  const char cf = ivel == 3 ? 'f' : 'c';
  const DBound &bc = ivel == 1 ? c->bcu : ivel == 2 ? c->bcv : c->bcw;
  const char *cbc = &c->cbcvel[6 * (ivel - 1) + 4];
  has[0] = has[1] = 0;
  for (int ib = 0; ib <= 1; ++ib) {
    R[ib] = RhsBz{nullptr, 0, cf, 1., 1., 1., 0.};
    if (!ISB(c, ib, 3) || cbc[ib] == 'P') continue;
    has[ib] = 1;
    const real dlc = cf == 'c' ? (ib ? c->dzc[n3] : c->dzc[0]) : (ib ? c->dzc[n3 - 1] : c->dzc[1]);
    const real dlf = ib ? c->dzf[n3] : c->dzf[1];
    R[ib] = RhsBz{plane(bc, 3, ib, n), cbc[ib], cf, dlc, dlf, ib == 0 ? (real)1. : (real)-1., alpha};
  }
}
// ... as a pass of its own. planes != nullptr: the two contributions go to planes[0 / n1*n2] instead of being added to the field; has[ib] tells which exist
int op_rhs_b_velz(cales_ctx *c, int ivel, real alpha, real *planes, int *has) {
  const int *n = c->n;
  RhsBz R[2]; int on[2];
  rhs_b_velz_args(c, ivel, alpha, R, on);
  if (has) { has[0] = on[0]; has[1] = on[1]; }
  for (int ib = 0; ib <= 1; ++ib) {
    if (!on[ib]) continue;
    const int pos = ib ? n[2] - ((R[ib].cf == 'f' && R[ib].ctype == 'D') ? 1 : 0) : 1;      // face-centred Dirichlet data: the last unknown plane is n3 - 1
    LAUNCH(c, k_rhs_b_velz, dim3((n[0] + 63) / 64, (n[1] + 3) / 4), dim3(64, 4), 0, c->stream, c->g, c->f[CALES_U + ivel - 1],
                       R[ib].bc, ib, R[ib].ctype, R[ib].cf, R[ib].dlc, R[ib].dlf, alpha, pos, planes ? planes + (size_t)ib * n[0] * n[1] : nullptr);
  }
  LAUNCHCHK(c);
  return 0;
}

int op_xwrap_zghost(cales_ctx *c, int nf, real **f) {
  HaloFields H; H.nf = nf; for (int q = 0; q < nf; ++q) H.p[q] = f[q];
  LAUNCH(c, k_xwrap_zghost, dim3((c->n[1] + 2 + 255) / 256, 2, nf), dim3(256), 0, c->stream, c->g, H);
  LAUNCHCHK(c);
  return 0;
}
