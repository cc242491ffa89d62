// extern "C" entry points of libcales_hip.so (include/cales.h): context life cycle, host<->device copies,
// one entry per reference operator, the fused time step (reference src/main.f90:417-508) and the
// HIP-event kernel timers used by bench.py's roofline line.
#include "common.hpp"
#include "../../include/cales_post.h"
#include "../../include/cales_pdf.h"
#include "../../include/cales_spectra.h"
#include "../../include/cales_cospectra.h"
#include "../../include/cales_derived.h"
#include <algorithm>
#include <atomic>

static thread_local std::string g_create_err;

// ------------------------------------------------------------------------------------------ launch check (common.hpp, LAUNCH)
void launch_failed(cales_ctx *c, const char *what, hipError_t e) {
  if (c->launch_err.empty()) c->launch_err = std::string("kernel launch failed: ") + what + ": " + hipGetErrorString(e) + " (the context is unusable from here on)";
}
// every operator entry: refuse a failed context, run, and report a launch that failed on the way
static int finish_pending(cales_ctx *c);
// ... and first of all completes a projection that cales_step left to its successor (common.hpp, cales_ctx::pend)
#define ENTER(c) do { LAUNCHCHK(c); if (const int pe_ = finish_pending(c)) return pe_; } while (0)
#define ENTRY(c, expr) do { ENTER(c); const int e_ = (expr); if (e_) return e_; LAUNCHCHK(c); return 0; } while (0)

// ------------------------------------------------------------------------------------------ profiling
int mark_stream(cales_ctx *c, hipStream_t s, hipEvent_t *e) {
  if (c->sync_ev.size() < 64) { hipEvent_t ne; HIPCHK(c, hipEventCreateWithFlags(&ne, hipEventDisableTiming)); c->sync_ev.push_back(ne); c->sync_next = c->sync_ev.size() - 1; }
  *e = c->sync_ev[c->sync_next]; c->sync_next = (c->sync_next + 1) % c->sync_ev.size();
  HIPCHK(c, hipEventRecord(*e, s));
  return 0;
}
int stream_after(cales_ctx *c, hipStream_t later, hipStream_t earlier) {
  hipEvent_t e;
  if (int err = mark_stream(c, earlier, &e)) return err;
  HIPCHK(c, hipStreamWaitEvent(later, e, 0));
  return 0;
}
int prof_begin(cales_ctx *c, const char *name, hipStream_t s) {
  int slot = -1;
  for (size_t q = 0; q < c->stats.size(); ++q) if (c->stats[q].name == name) { slot = (int)q; break; }
  if (slot < 0) { KernelStat s; s.name = name; c->stats.push_back(s); slot = (int)c->stats.size() - 1; }
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!c->evpool.empty()) { ev = c->evpool.back(); c->evpool.pop_back(); }
  else { hipEventCreate(&ev.first); hipEventCreate(&ev.second); }
  hipEventRecord(ev.first, s ? s : c->stream);
  c->pending.push_back({slot, ev});
  return (int)c->pending.size() - 1;
}
void prof_end(cales_ctx *c, int idx, hipStream_t s) { hipEventRecord(c->pending[idx].second.second, s ? s : c->stream); }
void prof_flush(cales_ctx *c) {
  if (c->pending.empty()) return;
  hipStreamSynchronize(c->stream);
  if (c->comm_stream) hipStreamSynchronize(c->comm_stream);
  for (auto &pe : c->pending) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, pe.second.first, pe.second.second);
    c->stats[pe.first].calls += 1; c->stats[pe.first].ms += ms;
    c->evpool.push_back(pe.second);
  }
  c->pending.clear();
}

// ------------------------------------------------------------------------------------------ device memory (common.hpp)
static std::atomic<int64_t> g_mem_bytes{0}, g_mem_allocs{0};      // over every context of the process: cales_memory_in_use(NULL)
static void mem_record(cales_ctx *c, void *base, size_t bytes, bool pinned) {
  c->mem.push_back({base, bytes, pinned}); c->mem_bytes += (int64_t)bytes; g_mem_bytes += (int64_t)bytes; g_mem_allocs += 1;
}
int ctx_alloc(cales_ctx *c, real **p, size_t n, bool zero) {
  HIPCHK(c, hipMalloc(p, (n ? n : 1) * sizeof(real)));
  mem_record(c, *p, (n ? n : 1) * sizeof(real), false);
  if (zero) HIPCHK(c, hipMemset(*p, 0, (n ? n : 1) * sizeof(real)));
  return 0;
}
int ctx_alloc_pinned(cales_ctx *c, real **p, size_t n) {
  if (hipHostMalloc((void **)p, n * sizeof(real)) != hipSuccess) { c->err = "hipHostMalloc failed"; return 1; }
  mem_record(c, *p, n * sizeof(real), true);
  return 0;
}
void ctx_free(cales_ctx *c, real *p) {
  for (size_t q = c->mem.size(); p && q-- > 0;) if (c->mem[q].base == p) {
    const MemBlock b = c->mem[q]; c->mem.erase(c->mem.begin() + q);
    if (b.pinned) hipHostFree(b.base); else hipFree(b.base);
    c->mem_bytes -= (int64_t)b.bytes; g_mem_bytes -= (int64_t)b.bytes; g_mem_allocs -= 1;
    return;
  }
}
void ctx_release_all(cales_ctx *c) { while (!c->mem.empty()) ctx_free(c, (real *)c->mem.back().base); }
// ------------------------------------------------------------------------------------------ helpers
// 3-D fields: pitch-padded rows, shifted so that element (1,j,k) sits on a 128-B boundary (see cales_create). (Skewing the start of
// every field by a different number of cache lines, so that the same cell of different fields does not fall on the same L2 set,
// was measured at 512^3 with six strides and changed no kernel by more than the run-to-run noise.) width = 2: a field of PAIRS (|S|Sij of the
// dynamic model, SgsPath::pair), pair (1,j,k) on a 128-B boundary
static int field_alloc(cales_ctx *c, real **p, int width = 1) {
  real *base = nullptr;
  if (ctx_alloc(c, &base, width * (c->ntot + LINE_REALS))) return 1;
  *p = base + width * c->field_ofs;
  return 0;
}
// k fields in ONE allocation, each right behind the one before: a kernel that addresses the first with 32-bit byte offsets reaches the others with
// multiples of the constant c->pp_companion_bytes added (the correction pressure and its companions, the velocity and its companion: the second /
// third ghost rows of k_corr_strain_tile on several slabs).
static int field_alloc_multi(cales_ctx *c, int k, real **p) {
  real *base = nullptr;
  const size_t one = c->ntot + LINE_REALS;
  if (ctx_alloc(c, &base, (size_t)k * one)) return 1;
  for (int q = 0; q < k; ++q) p[q] = base + (size_t)q * one + c->field_ofs;
  c->pp_companion_bytes = one * sizeof(real); c->comp_one = one;
  return 0;
}
// host layout (0:n1+1,0:n2+1,0:n3+1), x contiguous  <->  device layout with row pitch s1
__global__ __launch_bounds__(256) void k_repack(Geom g, int to_device, real *__restrict__ dev, real *__restrict__ packed) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
  if (i > g.n1 + 1 || j > g.n2 + 1) return;
  const size_t h = (size_t)i + (size_t)(g.n1 + 2) * ((size_t)j + (size_t)(g.n2 + 2) * k);
  if (to_device) dev[g.ix(i, j, k)] = packed[h]; else packed[h] = dev[g.ix(i, j, k)];
}
// A strided box of a field (include/cales_post.h), packed in Fortran order: one thread per OUTPUT element, numbered as the packed array is stored, so the
// stores of a wave are contiguous whatever the box -- its lanes run along the fastest direction of the output that has more than one point. The loads are
// what the box makes them: row segments with nskip(1) = 1, one element per row (one 128-B line per lane) for a y-z plane. The points are first + m * skip
// in LOCAL haloed indices; the host has checked them against the field (box_share below).
struct BoxRead { int first[3], skip[3], count[3]; };
__global__ __launch_bounds__(256) void k_box_read(Geom g, BoxRead b, size_t total, const real *__restrict__ dev, real *__restrict__ packed) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t r = t / (size_t)b.count[0];
  const int m0 = (int)(t - r * (size_t)b.count[0]), m2 = (int)(r / (size_t)b.count[1]), m1 = (int)(r - (size_t)m2 * (size_t)b.count[1]);
  packed[t] = dev[g.ix(b.first[0] + m0 * b.skip[0], b.first[1] + m1 * b.skip[1], b.first[2] + m2 * b.skip[2])];
}
// Same-box calibration (bench.py "calibration"): three streams over the rows of the context's own fields in the library's layout
// (padded rows, element 1 of every row on a 128-B boundary, 8 B per lane -- what the FP64 passes do), timed with HIP events on the context's stream.
// MODE 0: read-only, 1: write-only, 2: copy. Rows are dealt to the blocks round-robin (the order of tools/micro/calib.hip's calib_copy8_rows).
template <int MODE>
__global__ __launch_bounds__(256) void k_calib_rows(Geom g, long nrows, const real *__restrict__ a, real *__restrict__ b, real *__restrict__ sink) {
  real acc = 0.;
  for (long r = blockIdx.x; r < nrows; r += gridDim.x) {
    const size_t o = (size_t)r * g.s1 + 1;
    for (int i = threadIdx.x; i < g.n1; i += 256) {
      if (MODE == 0) acc += a[o + i];
      else if (MODE == 1) b[o + i] = (real)1.5;
      else b[o + i] = a[o + i];
    }
  }
  if (MODE == 0 && acc == (real)1.2345e30) sink[blockIdx.x] = acc;      // never true: no write traffic
}
int ctx_upload(cales_ctx *c, real **p, const std::vector<real> &v) {
  if (ctx_alloc(c, p, v.size(), false)) return 1;
  HIPCHK(c, hipMemcpy(*p, v.data(), v.size() * sizeof(real), hipMemcpyHostToDevice));
  return 0;
}
// the views of RedLayout: result slots and plane sums in the tail of staging buffer A once hooks are registered (the host all-reduces them in place), in d_red otherwise
static void red_place(cales_ctx *c) {
  c->res = c->comm.on ? c->comm.A + c->stage.tail : c->d_red;
  c->d_p1d = c->res + c->red.p1d;
}
// THE place where a change of the hooks reaches everything that depends on them (cales_create, cales_set_comm, cales_set_comm_overlap): Comm's record of what
// they imply, the views of the reductions, the plan of a step (re-made by the next reader) and the schedules of the solves
static int comm_changed(cales_ctx *c) {
  Comm &m = c->comm;
  const bool second = c->P > 1 && m.on && c->comm_stream;
  m.halo_second_stream = second && m.halo_s; m.a2a_second_stream = second && m.a2a_part;
  m.has_lo = c->per_y || c->rank > 0; m.has_hi = c->per_y || c->rank < c->P - 1;
  red_place(c);
  c->plan.valid = false;
  return solver_comm_changed(c);
}
// n reals at the head of staging buffer A for a caller between two exchanges: below the tail, and after whatever the second stream still does with the buffer
real *stage_borrow(cales_ctx *c, int64_t n) {
  if (require_hooks(c)) return nullptr;
  if (n > c->stage.borrow) { c->err = "staging buffer too small for the " + std::to_string(n) + " reals a caller borrows"; return nullptr; }
  if (c->comm_stream && stream_after(c, c->stream, c->comm_stream)) return nullptr;
  return c->comm.A;
}
real *field_ptr(cales_ctx *c, int id, const char *who, int use) {
  if (id < 0 || id >= CALES_NFIELDS || !c->f[id]) { c->err = std::string(who) + ": bad field id"; return nullptr; }
  // (element 1 of a row: every field of a context has it on a 128-B boundary, field_alloc above)
  if ((use & FIELD_ROWS16) && ((uintptr_t)(c->f[id] + 1) & 15u) != 0) { c->err = std::string(who) + ": the field's rows are not 16-byte aligned"; return nullptr; }
  if ((use & FIELD_READ) && id == CALES_VISCT && materialize_visct(c)) return nullptr;
  return c->f[id];
}
static int upload_bound(cales_ctx *c, DBound &b, std::vector<real> h[3]) {
  return ctx_upload(c, &b.x, h[0]) || ctx_upload(c, &b.y, h[1]) || ctx_upload(c, &b.z, h[2]);
}

extern "C" {

// ------------------------------------------------------------------------------------------ host-only helpers
int cales_initgrid(int gtype, int n, real gr, real lz, real *dzc, real *dzf, real *zc, real *zf) {
  if (n < 1 || !dzc || !dzf || !zc || !zf) return 1;
  hs_initgrid(gtype, n, gr, lz, dzc, dzf, zc, zf);
  return 0;
}
int cales_initflow(const cales_case *cs, const char *inivel, int is_wallturb, real *u, real *v, real *w, real *p) {
  if (!cs || !inivel || !u || !v || !w || !p) return 1;
  return hs_initflow(cs, inivel, is_wallturb, u, v, w, p, 0, 1);
}
int cales_check_case(const cales_case *cs, char *msg, int msglen) {
  std::string m;
  const int rc = hs_check_case(cs, m);
  if (msg && msglen > 0) { std::snprintf(msg, msglen, "%s", m.c_str()); }
  return rc;
}

int cales_real_size(void) { return (int)sizeof(real); }
int cales_device_count(int *ndev) { if (!ndev) return 1; *ndev = 0; return hipGetDeviceCount(ndev) == hipSuccess ? 0 : 2; }
int cales_set_device(int dev) { return hipSetDevice(dev) == hipSuccess ? 0 : 1; }

// ------------------------------------------------------------------------------------------ context
const char *cales_last_error(const cales_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int cales_memory_in_use(const cales_ctx *c, int64_t *bytes, int64_t *allocations) {
  if (bytes) *bytes = c ? c->mem_bytes : g_mem_bytes.load();
  if (allocations) *allocations = c ? (int64_t)c->mem.size() : g_mem_allocs.load();
  return 0;
}

void cales_destroy(cales_ctx *c) {
  if (!c) return;
  hipStreamSynchronize(c->stream);
  prof_flush(c);
  for (auto &ev : c->evpool) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
  for (auto &e : c->sync_ev) hipEventDestroy(e);
  if (c->comm_stream) { hipStreamSynchronize(c->comm_stream); hipStreamDestroy(c->comm_stream); }
  if (c->own_stream) hipStreamDestroy(c->stream);
  cales_comm_release_native(c);
  solver_teardown(c);
  ctx_release_all(c);
  delete c;
}

static bool fold_correc_possible(const cales_ctx *c);      // (with make_plan below)
int cales_create(const cales_case *cs, void *stream, cales_ctx **out) {
  if (!cs || !out) { g_create_err = "null argument"; return 1; }
  *out = nullptr;
  std::string msg;
  if (hs_check_case(cs, msg)) { g_create_err = msg; return 2; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_err = "no HIP device: the CaLES hot path has no CPU fallback"; return 3; }
  cales_ctx *c = new cales_ctx();
  c->C = *cs;
  // 'dsmag' of a -D_FILTER_2D build: normalised once -- the model is 'dsmag' everywhere, the plane filter is a property of its path (SgsPath)
  // ... and so are the directions the Germano identity is averaged over (enum cales_sgs_average; cales_check_case has refused every other combination)
  if (cs->sgstype & CALES_SGS_AVE_VOLUME) c->sgs.ave = SgsAve::volume;
  if (cs->sgstype & CALES_SGS_AVE_XLINES) c->sgs.ave = SgsAve::xlines;
  if (cs->sgstype & CALES_SGS_AVE_LOCAL) c->sgs.ave = SgsAve::local;
  c->C.sgstype = cs->sgstype & ~(CALES_SGS_AVE_VOLUME | CALES_SGS_AVE_XLINES | CALES_SGS_AVE_LOCAL);
  if (c->C.sgstype == CALES_SGS_DSMAG_FILTER2D) { c->C.sgstype = CALES_SGS_DSMAG; c->sgs.filter2d = true; }
  c->fl.read_env();      // the CALES_* switches are fixed for the life of the context
  // (a context is whole at every stage: its members start out null, what it has allocated is in c->mem -- cales_destroy takes it as it is)
  auto fail = [&](int rc) { g_create_err = c->err; cales_destroy(c); return rc; };
  if (stream) c->stream = (hipStream_t)stream;
  else if (hipStreamCreate(&c->stream) != hipSuccess) { c->stream = nullptr; c->err = "hipStreamCreate failed"; return fail(4); }
  else c->own_stream = true;
  // geometry: y-slab of rank `rank`
  const int P = cs->nranks, r = cs->rank;
  c->P = P; c->rank = r; c->per_y = cs->cbcpre[2] == 'P' && cs->cbcpre[3] == 'P';
  c->n[0] = cs->ng[0]; c->n[1] = cs->ng[1] / P; c->n[2] = cs->ng[2];
  c->lo[0] = 1; c->lo[1] = r * c->n[1] + 1; c->lo[2] = 1;
  for (int d = 0; d < 3; ++d) { c->dl[d] = cs->l[d] / (real)(1.f * (float)cs->ng[d]); c->dli[d] = 1. / c->dl[d]; }   // param.f90:153-154
  c->visc = 1. / cs->visci;
  Geom &g = c->g;
  g.n1 = c->n[0]; g.n2 = c->n[1]; g.n3 = c->n[2];
  // Row pitch: a multiple of one cache line (128 B = 16 doubles / 32 floats) with room for the n1/2+1 complex modes of a row stored from i = 1; with the
  // one-line-minus-one-element offset of field_alloc, element i = 1 of every row is 128-B aligned, so kernels whose waves handle 64 consecutive
  // cells from i = 1 read and write whole cache lines (partial-line writes cost ~1.5x, tools/micro/wrtile.hip).
  g.s1 = (g.n1 + 3 + LINE_REALS - 1) / LINE_REALS * LINE_REALS;
  c->field_ofs = LINE_REALS - 1;
  g.s12 = (long)g.s1 * (g.n2 + 2); g.jlo = c->lo[1] - 1; g.ng2 = cs->ng[1];
  c->ntot = (size_t)g.s12 * (g.n3 + 2);
  const int n3 = c->n[2];
  // z grid and metrics (main.f90:246-285)
  c->dzc.resize(n3 + 2); c->dzf.resize(n3 + 2); c->zc.resize(n3 + 2); c->zf.resize(n3 + 2);
  c->dzci.resize(n3 + 2); c->dzfi.resize(n3 + 2); c->gvr_c.resize(n3 + 2); c->gvr_f.resize(n3 + 2);
  hs_initgrid(cs->gtype, n3, cs->gr, cs->l[2], c->dzc.data(), c->dzf.data(), c->zc.data(), c->zf.data());
  for (int k = 0; k <= n3 + 1; ++k) {
    c->dzci[k] = 1. / c->dzc[k]; c->dzfi[k] = 1. / c->dzf[k];
    c->gvr_c[k] = c->dl[0] * c->dl[1] * c->dzc[k] / (cs->l[0] * cs->l[1] * cs->l[2]);
    c->gvr_f[k] = c->dl[0] * c->dl[1] * c->dzf[k] / (cs->l[0] * cs->l[1] * cs->l[2]);
  }
  if (ctx_upload(c, &c->d_dzc, c->dzc) || ctx_upload(c, &c->d_dzf, c->dzf) || ctx_upload(c, &c->d_zc, c->zc) || ctx_upload(c, &c->d_zf, c->zf) ||
      ctx_upload(c, &c->d_dzci, c->dzci) || ctx_upload(c, &c->d_dzfi, c->dzfi) || ctx_upload(c, &c->d_gvr_c, c->gvr_c) || ctx_upload(c, &c->d_gvr_f, c->gvr_f))
    return fail(5);
  // which faces are physical boundaries of this slab (initmpi.f90:201-204 for x-pencils; y is the decomposed direction)
  c->is_bound[0] = c->is_bound[1] = 1;
  { c->is_bound[2] = (!c->per_y && r == 0) ? 1 : 0; c->is_bound[3] = (!c->per_y && r == P - 1) ? 1 : 0;
    const bool per_z = cs->cbcpre[4] == 'P' && cs->cbcpre[5] == 'P';
    c->is_bound[4] = c->is_bound[5] = per_z ? 0 : 1; }
  // boundary-condition tables (bound.f90:726-867)
  std::vector<real> hb[11][3];
  hs_initbc(c, hb);
  DBound *bs[11] = {&c->bcu, &c->bcv, &c->bcw, &c->bcp, &c->bcs, &c->bcuf, &c->bcvf, &c->bcwf, &c->bcu_mag, &c->bcv_mag, &c->bcw_mag};
  for (int q = 0; q < 11; ++q) if (upload_bound(c, *bs[q], hb[q])) return fail(6);
  // walls (sgs.f90:70-83,154-171); those in y are global properties of the case, not of the slab (distances use global indices)
  for (int d = 1; d <= 3; ++d) for (int s = 0; s <= 1; ++s) c->is_wall[s + 2 * (d - 1)] = (ISB(c, s, d) && CBV(c, s, d, d) == 'D') ? 1. : 0.;
  for (int s = 0; s <= 1; ++s) c->is_wall[s + 2] = (!c->per_y && CBV(c, s, 2, 2) == 'D') ? 1. : 0.;
  sgs_setup(c);      // the form of cmpt_sgs: which scratch fields it needs, whether the projection can fold into it
  bc_setup(c);       // the form of every BC set in the ghost-cell operators
  // pressure boundary r.h.s. (main.f90:317, bound.f90:447-499)
  { const int *n = c->n;
    const real dx01[2] = {c->dl[0], c->dl[0]}, dy01[2] = {c->dl[1], c->dl[1]};
    const real dzc01[2] = {c->dzc[0], c->dzc[n3]}, dzf01[2] = {c->dzf[1], c->dzf[n3]};
    std::vector<real> rx((size_t)n[1] * n[2] * 2), ry((size_t)n[0] * n[2] * 2), rz((size_t)n[0] * n[1] * 2);
    hs_bc_rhs(&cs->cbcpre[0], hb[3][0].data(), n[1], n[2], dx01, dx01, 'c', rx.data());
    hs_bc_rhs(&cs->cbcpre[2], hb[3][1].data(), n[0], n[2], dy01, dy01, 'c', ry.data());
    hs_bc_rhs(&cs->cbcpre[4], hb[3][2].data(), n[0], n[1], dzc01, dzf01, 'c', rz.data());
    if (ctx_upload(c, &c->rhsbp[0], rx) || ctx_upload(c, &c->rhsbp[1], ry) || ctx_upload(c, &c->rhsbp[2], rz)) return fail(7); }
  // fields (haloed); r.h.s. buffers use the same layout so every kernel shares one index
  const int nfields = cs->impdiff ? CALES_NFIELDS : CALES_DUDTD;
  // several slabs where some plan can take StepPlan::fold_rows2 (three fields under 4 GB, four rows per slab, the one-launch ghost-cell kernel):
  // companions behind u, v, w (both buffer sets) and two behind pp (common.hpp, vel_comp)
  c->vel_comp = P > 1 && fold_correc_possible(c) && c->n[1] >= 4 && 3 * (c->ntot + 2 * LINE_REALS) * sizeof(real) < (1ull << 32) && !c->fl.unmerged_bc;
  auto vel_field = [&](real **p) { real *two[2] = {nullptr, nullptr}; const int e = field_alloc_multi(c, c->vel_comp ? 2 : 1, two); *p = two[0]; return e; };
  for (int q = 0; q < nfields; ++q) if (q != CALES_PP && (q <= CALES_W ? vel_field(&c->f[q]) : field_alloc(c, &c->f[q]))) return fail(8);
  { real *three[3]; if (field_alloc(c, &c->scr1) || field_alloc_multi(c, c->vel_comp ? 3 : 2, three)) return fail(9);      // (scr2, scr3: pp's companions)
    c->f[CALES_PP] = three[0]; c->scr2 = three[1]; c->scr3 = c->vel_comp ? three[2] : nullptr; }
  for (int q = 0; q < 3; ++q) if (vel_field(&c->f2[q])) return fail(9);
  c->red = RedLayout::of(n3);
  if (ctx_alloc(c, &c->d_red, (size_t)c->red.total) || ctx_alloc(c, &c->d_force, 8)) return fail(10);
  if (ctx_alloc_pinned(c, &c->h_red, RedLayout::NHOST)) return fail(11);
  // sgs scratch (sgs.f90:70-83,154-171)
  if (c->C.sgstype >= 1) {
    if (field_alloc(c, &c->s0)) return fail(12);
    const int nw = c->C.sgstype == 1 ? 3 : 6;
    for (int m = 0; m < nw; ++m) if (field_alloc(c, &c->wk[m])) return fail(12);
  }
  if (c->C.sgstype == 2) {
    if (field_alloc(c, &c->uc) || field_alloc(c, &c->vc) || field_alloc(c, &c->wc) || field_alloc(c, &c->uf) ||
        field_alloc(c, &c->vf) || field_alloc(c, &c->wf) || (!c->sgs.filter2d && field_alloc(c, &c->alph2)))
      return fail(13);
    if (c->sgs.pair) {      // |S|Sij as three fields of pairs between K_AC and the fused last pass: the twelve scalar scratch fields of the other forms are not needed
      for (int m = 0; m < 3; ++m) if (field_alloc(c, &c->ss2[m], 2)) return fail(13);
    } else
    for (int m = 0; m < 6; ++m) if (field_alloc(c, &c->sij[m]) || field_alloc(c, &c->mij[m])) return fail(13);
  }
  { hipDeviceProp_t pr; int dev = 0; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) c->ncu = pr.multiProcessorCount; }      // (before solver_setup: its schedule counts on it)
  if (solver_setup(c)) return fail(14);
  c->stage = StageLayout::of(c->g.s1, n3, c->n[1], c->cw, P, c->red);      // (the mode columns per rank are the solver's)
  if (comm_changed(c)) return fail(14);      // no hooks yet: the reductions in d_red, the solves' schedules without staging buffers
  if (sgs_setup_launches(c)) return fail(14);
  mom_setup(c);
  if (hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "sync failed"; return fail(15); }
  if (!c->launch_err.empty()) { c->err = c->launch_err; return fail(16); }      // a set-up kernel (twiddles, tables) or attribute call failed
  *out = c;
  return 0;
}

int cales_sync(cales_ctx *c) { ENTER(c); HIPCHK(c, hipStreamSynchronize(c->stream)); return 0; }      // (what has been asked for is done when this returns: a pending projection too)
int cales_local_size(const cales_ctx *c, int32_t n[3], int32_t lo[3]) { for (int d = 0; d < 3; ++d) { n[d] = c->n[d]; lo[d] = c->lo[d]; } return 0; }

// ------------------------------------------------------------------------------------------ copies
int cales_set_field(cales_ctx *c, int field, const real *host) {
  ENTER(c);
  real *f = field_ptr(c, field, "cales_set_field", FIELD_WRITE); if (!f) return 1;
  if (field == CALES_VISCT) { c->visct_zero = false; c->visct_lazy = false; }
  const size_t nh = (size_t)(c->n[0] + 2) * (c->n[1] + 2) * (c->n[2] + 2);
  const dim3 b(64, 4, 1), gr((c->n[0] + 2 + 63) / 64, (c->n[1] + 2 + 3) / 4, c->n[2] + 2);
  HIPCHK(c, hipMemcpyAsync(c->scr1, host, nh * sizeof(real), hipMemcpyHostToDevice, c->stream));     // scr1: scratch between operators
  LAUNCH(c, k_repack, gr, b, 0, c->stream, c->g, 1, f, c->scr1);
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int cales_get_field(cales_ctx *c, int field, real *host) {
  ENTER(c);
  real *f = field_ptr(c, field, "cales_get_field", FIELD_READ); if (!f) return 1;
  const size_t nh = (size_t)(c->n[0] + 2) * (c->n[1] + 2) * (c->n[2] + 2);
  const dim3 b(64, 4, 1), gr((c->n[0] + 2 + 63) / 64, (c->n[1] + 2 + 3) / 4, c->n[2] + 2);
  LAUNCH(c, k_repack, gr, b, 0, c->stream, c->g, 0, f, c->scr1);
  LAUNCHCHK(c);
  return read_back(c, host, c->scr1, nh);
}
int cales_upload_state(cales_ctx *c, const real *u, const real *v, const real *w, const real *p) {
  return cales_set_field(c, CALES_U, u) || cales_set_field(c, CALES_V, v) || cales_set_field(c, CALES_W, w) || cales_set_field(c, CALES_P, p);
}
int cales_download_state(cales_ctx *c, real *u, real *v, real *w, real *p, real *visct) {
  if (u && cales_get_field(c, CALES_U, u)) return 1;
  if (v && cales_get_field(c, CALES_V, v)) return 1;
  if (w && cales_get_field(c, CALES_W, w)) return 1;
  if (p && cales_get_field(c, CALES_P, p)) return 1;
  if (visct && cales_get_field(c, CALES_VISCT, visct)) return 1;
  return 0;
}
int cales_get_bcvel(cales_ctx *c, int ivel, real *x, real *y, real *z) {
  const DBound &b = ivel == 1 ? c->bcu : ivel == 2 ? c->bcv : c->bcw; const int *n = c->n;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(x, b.x, sizeof(real) * (size_t)(n[1] + 2) * (n[2] + 2) * 2, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(y, b.y, sizeof(real) * (size_t)(n[0] + 2) * (n[2] + 2) * 2, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(z, b.z, sizeof(real) * (size_t)(n[0] + 2) * (n[1] + 2) * 2, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------------------------------ parts of a field (include/cales_post.h: out2d / out3d)
// the share of rank cs->rank in the box lo : hi : nskip of global haloed indices: first point and number of points per direction
static int box_share(const cales_case *cs, const int32_t *lo, const int32_t *hi, const int32_t *nskip, int32_t *first, int32_t *count, std::string &err) {
  if (!cs || !lo || !hi || !nskip || !first || !count) { err = "box: null argument"; return 1; }
  if (cs->nranks < 1 || cs->rank < 0 || cs->rank >= cs->nranks || cs->ng[1] % cs->nranks) { err = "box: bad rank / number of ranks"; return 1; }
  for (int d = 0; d < 3; ++d) {
    const char x = "xyz"[d];
    if (nskip[d] < 1) { err = std::string("box: nskip < 1 in ") + x; return 1; }
    if (lo[d] < 0) { err = std::string("box: lo < 0 in ") + x; return 1; }
    if (hi[d] > cs->ng[d] + 1) { err = std::string("box: hi > ng+1 in ") + x; return 1; }
    if (lo[d] > hi[d]) { err = std::string("box: lo > hi in ") + x; return 1; }
    first[d] = lo[d]; count[d] = (hi[d] - lo[d]) / nskip[d] + 1;
  }
  // y: the rows the rank owns, with the global ghost row 0 on the first rank and ng2+1 on the last
  const int n2 = cs->ng[1] / cs->nranks;
  const int a = cs->rank == 0 ? 0 : cs->rank * n2 + 1, b = std::min((int)hi[1], cs->rank == cs->nranks - 1 ? cs->ng[1] + 1 : (cs->rank + 1) * n2);
  const int m0 = a > lo[1] ? (a - lo[1] + nskip[1] - 1) / nskip[1] : 0;      // first point at or above a
  first[1] = lo[1] + m0 * nskip[1];
  count[1] = first[1] <= b ? (b - first[1]) / nskip[1] + 1 : 0;
  return 0;
}
int cales_box_share(const cales_case *cs, const int32_t lo[3], const int32_t hi[3], const int32_t nskip[3], int32_t first[3], int32_t count[3]) {
  return box_share(cs, lo, hi, nskip, first, count, g_create_err);
}
int cales_read_box(cales_ctx *c, int field, const int32_t lo[3], const int32_t hi[3], const int32_t nskip[3], real *buf, int32_t count[3]) {
  ENTER(c);
  const char *who = "cales_read_box";
  if (!field_ptr(c, field, who, FIELD_WRITE)) return 1;      // (the id first; nothing is read yet)
  int32_t first[3], cnt[3];
  if (int e = box_share(&c->C, lo, hi, nskip, first, cnt, c->err)) return e;
  if (count) for (int d = 0; d < 3; ++d) count[d] = cnt[d];
  const size_t total = (size_t)cnt[0] * (size_t)cnt[1] * (size_t)cnt[2];      // (never more than a field: the points of a share are distinct cells of the slab)
  if (total == 0) return 0;
  if (!buf) { c->err = "box: buf is NULL"; return 1; }
  const real *f = field_ptr(c, field, who, FIELD_READ); if (!f) return 1;
  BoxRead b;
  for (int d = 0; d < 3; ++d) { b.first[d] = first[d]; b.skip[d] = nskip[d]; b.count[d] = cnt[d]; }
  b.first[1] -= c->g.jlo;      // global row -> row of the slab
  { ProfScope ps(c, "box_read");
    LAUNCH(c, k_box_read, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->g, b, total, f, c->scr1); }     // scr1: scratch between operators
  LAUNCHCHK(c);
  return read_back(c, buf, c->scr1, total);
}
int cales_out2d(cales_ctx *c, int field, int inorm, int islice, real *buf, int32_t count[3]) {
  ENTER(c);
  if (inorm < 1 || inorm > 3) { c->err = "out2d: inorm must be 1..3"; return 1; }
  if (islice < 1 || islice > c->C.ng[inorm - 1]) { c->err = "out2d: islice outside 1..ng"; return 1; }
  int32_t lo[3] = {1, 1, 1}, hi[3] = {c->C.ng[0], c->C.ng[1], c->C.ng[2]};
  const int32_t one[3] = {1, 1, 1};
  lo[inorm - 1] = hi[inorm - 1] = islice;
  return cales_read_box(c, field, lo, hi, one, buf, count);
}
int cales_out3d(cales_ctx *c, int field, const int32_t nskip[3], real *buf, int32_t count[3]) {
  const int32_t lo[3] = {1, 1, 1};
  return cales_read_box(c, field, lo, c->C.ng, nskip, buf, count);
}

// ------------------------------------------------------------------------------------------ operators
int cales_bounduvw(cales_ctx *c, int is_updt_wm, int is_correc) {
  ENTRY(c, op_bounduvw(c, VelSet::state, is_updt_wm, is_correc));
}
int cales_boundp(cales_ctx *c, int field, int which) {
  if (!field_ptr(c, field, "cales_boundp", FIELD_WRITE)) return 1;
  ENTRY(c, op_boundp(c, c->f[field], which));
}
int cales_get_forcing(cales_ctx *c, real f[3]);
int cales_mom(cales_ctx *c) { ENTRY(c, op_mom(c)); }
int cales_rk(cales_ctx *c, int irk, real dt) { if (irk < 1 || irk > 3) { c->err = "irk must be 1..3"; return 1; } ENTRY(c, op_rk(c, irk, dt)); }
int cales_rk_par(cales_ctx *c, const real rkpar[2], real dt, real f_out[3]) {
  if (!rkpar) { c->err = "cales_rk_par: rkpar is NULL"; return 1; }
  ENTER(c);
  if (int e = op_rk_par(c, rkpar[0], rkpar[1], dt)) return e;
  LAUNCHCHK(c);
  return f_out ? cales_get_forcing(c, f_out) : 0;
}
int cales_bulk_forcing(cales_ctx *c) { ENTRY(c, op_bulk_forcing(c)); }
int cales_get_forcing(cales_ctx *c, real f[3]) {
  if (int e = read_back(c, c->h_red + RedLayout::H_FORCE, c->d_force, 3)) return e;
  for (int q = 0; q < 3; ++q) f[q] = c->h_red[RedLayout::H_FORCE + q];
  return 0;
}
int cales_bulk_mean(cales_ctx *c, int field, int c_or_f, real *mean) {
  if (!field_ptr(c, field, "cales_bulk_mean", FIELD_WRITE)) return 1;      // (the mean of the field as it is stored: nothing is materialized)
  ENTER(c);
  if (int e = op_bulk_mean_dev(c, c->f[field], c_or_f)) return e;
  LAUNCHCHK(c);
  if (int e = read_back(c, c->h_red + RedLayout::H_BULK_MEAN, c->res + RedLayout::BULK_MEAN, 1)) return e;
  *mean = c->h_red[RedLayout::H_BULK_MEAN];
  return 0;
}
int cales_fillps(cales_ctx *c, real dtrki) { ENTRY(c, op_fillps(c, dtrki)); }
int cales_updt_rhs_b(cales_ctx *c) { ENTRY(c, op_updt_rhs_b(c)); }
int cales_solver(cales_ctx *c) { ENTRY(c, op_solver(c)); }
int cales_helmholtz(cales_ctx *c, int ivel, real alpha) { ENTRY(c, op_helmholtz(c, ivel, alpha)); }
int cales_helmholtz_z(cales_ctx *c, int ivel, real alpha) { if (ivel < 1 || ivel > 3) { c->err = "ivel must be 1..3"; return 1; } ENTRY(c, op_helmholtz_z(c, ivel, alpha)); }
int cales_correc(cales_ctx *c, real dtrk) { ENTRY(c, op_correc(c, dtrk)); }
int cales_updatep(cales_ctx *c, real alpha) { ENTRY(c, op_updatep(c, alpha)); }
int cales_cmpt_sgs(cales_ctx *c) { ENTRY(c, op_cmpt_sgs(c, nullptr)); }
int cales_chkdt(cales_ctx *c, real *dtmax) { ENTRY(c, op_chkdt(c, dtmax)); }
int cales_chkdiv(cales_ctx *c, real *divtot, real *divmax) { ENTRY(c, op_chkdiv(c, divtot, divmax)); }
int cales_out1d_single_point_chan(cales_ctx *c, real *buf) { if (!c || !buf) return 1; ENTRY(c, op_stats_chan(c, buf)); }
int cales_out1d_chan_budgets(cales_ctx *c, real *budget, real *leakage) { if (!c) return 1; ENTRY(c, op_stats_chan_budget(c, budget, leakage)); }
int cales_out1d(cales_ctx *c, int field, int idir, int use_dzc, real *buf) { if (!c || !buf) return 1; ENTRY(c, op_out1d(c, field, idir, use_dzc, buf)); }
int cales_out1d_chan(cales_ctx *c, real *buf) { if (!c || !buf) return 1; ENTRY(c, op_out1d_chan(c, buf)); }
int cales_out2d_duct(cales_ctx *c, real *buf) { if (!c || !buf) return 1; ENTRY(c, op_out2d_duct(c, buf)); }
// include/cales_pdf.h (k_pdf.hip)
int cales_pdf_planes(cales_ctx *c, int field, int nbins, real lo, real hi, int64_t *counts, int64_t *outside) {
  if (!c) return 1;
  ENTRY(c, op_pdf_planes(c, field, nbins, lo, hi, counts, outside));
}
int cales_jpdf_planes(cales_ctx *c, int field_a, int field_b, int nbins, real lo_a, real hi_a, real lo_b, real hi_b, int nplanes, const int32_t *kplanes,
                      int64_t *counts, int64_t *outside) {
  if (!c) return 1;
  ENTRY(c, op_jpdf_planes(c, field_a, field_b, nbins, lo_a, hi_a, lo_b, hi_b, nplanes, kplanes, counts, outside));
}
// include/cales_spectra.h (k_spectra.hip)
int cales_spectra_lines(cales_ctx *c, int field, int idir, real *power, real *lsum) {
  if (!c) return 1;
  ENTRY(c, op_spectra_lines(c, field, idir, power, lsum));
}
int cales_spectra_planes(cales_ctx *c, int field, int nplanes, const int32_t *kplanes, real *power2) {
  if (!c) return 1;
  ENTRY(c, op_spectra_planes(c, field, nplanes, kplanes, power2));
}
// include/cales_cospectra.h (k_spectra.hip)
int cales_cospectra_lines(cales_ctx *c, int field_a, int field_b, int idir, real *cross, real *lsum_a, real *lsum_b) {
  if (!c) return 1;
  ENTRY(c, op_cospectra_lines(c, field_a, field_b, idir, cross, lsum_a, lsum_b));
}
int cales_cospectra_planes(cales_ctx *c, int field_a, int field_b, int nplanes, const int32_t *kplanes, real *cross2) {
  if (!c) return 1;
  ENTRY(c, op_cospectra_planes(c, field_a, field_b, nplanes, kplanes, cross2));
}
// include/cales_derived.h (k_derived.hip)
static int derived_quantity_ok(cales_ctx *c, int quantity, const char *who) {
  if (quantity >= 0 && quantity < CALES_NDERIVED) return 1;
  c->err = std::string(who) + ": unknown quantity";
  return 0;
}
int cales_derived_box(cales_ctx *c, int quantity, const int32_t lo[3], const int32_t hi[3], const int32_t nskip[3], real *buf, int32_t count[3]) {
  if (!c) return 1;
  ENTER(c);
  if (!derived_quantity_ok(c, quantity, "cales_derived_box")) return 1;
  int32_t first[3], cnt[3];
  if (int e = box_share(&c->C, lo, hi, nskip, first, cnt, c->err)) return e;
  for (int d = 0; d < 3; ++d) if (lo[d] < 1 || hi[d] > c->C.ng[d]) {      // (the quantities are those of interior cells)
    c->err = std::string("derived box: ") + (lo[d] < 1 ? "lo < 1 in " : "hi > ng in ") + "xyz"[d]; return 1;
  }
  if (count) for (int d = 0; d < 3; ++d) count[d] = cnt[d];
  if ((size_t)cnt[0] * (size_t)cnt[1] * (size_t)cnt[2] == 0) return 0;
  if (!buf) { c->err = "derived box: buf is NULL"; return 1; }
  if (int e = op_derived_box(c, quantity, first, cnt, nskip, buf)) return e;
  LAUNCHCHK(c);
  return 0;
}
int cales_derived_out2d(cales_ctx *c, int quantity, int inorm, int islice, real *buf, int32_t count[3]) {
  if (!c) return 1;
  ENTER(c);
  if (inorm < 1 || inorm > 3) { c->err = "derived out2d: inorm must be 1..3"; return 1; }
  if (islice < 1 || islice > c->C.ng[inorm - 1]) { c->err = "derived out2d: islice outside 1..ng"; return 1; }
  int32_t lo[3] = {1, 1, 1}, hi[3] = {c->C.ng[0], c->C.ng[1], c->C.ng[2]};
  const int32_t one[3] = {1, 1, 1};
  lo[inorm - 1] = hi[inorm - 1] = islice;
  return cales_derived_box(c, quantity, lo, hi, one, buf, count);
}
int cales_derived_out3d(cales_ctx *c, int quantity, const int32_t nskip[3], real *buf, int32_t count[3]) {
  if (!c) return 1;
  const int32_t lo[3] = {1, 1, 1};
  return cales_derived_box(c, quantity, lo, c->C.ng, nskip, buf, count);
}
int cales_derived_to_pp(cales_ctx *c, int quantity) {
  if (!c) return 1;
  ENTER(c);
  if (!derived_quantity_ok(c, quantity, "cales_derived_to_pp")) return 1;
  ENTRY(c, op_derived_to_pp(c, quantity));
}

// ------------------------------------------------------------------------------------------ time step (main.f90:412-508)
__global__ __launch_bounds__(256) void k_row2_to_companion(Geom g, const real *__restrict__ pp, real *__restrict__ comp) {
  const int i = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y * 4 + threadIdx.y;
  if (i > g.n1 + 1 || k > g.n3 + 1) return;
  comp[g.ix(i, 1, k)] = pp[g.ix(i, 2, k)];
}

// the projection of a substep may be left to the next momentum pass (step_body): static conditions of the case and the switches
static bool fold_mom_ok(const cales_ctx *c) {
  bool ok = !c->fl.unfolded_mom && c->C.sgstype == 0 && c->visct_zero && !c->sgs_first && (c->C.impdiff == 0 || c->C.impdiff == 2) && (c->P == 1 || c->comm.on) && c->n[2] >= 3 &&
            !c->fl.unfused_rk && !c->fl.unfused_correc && !any_wm(c);
  for (int d = 1; d <= 3 && ok; ++d) {
    bool per = CBP(c, 0, d) == 'P' && CBP(c, 1, d) == 'P', walls = CBP(c, 0, d) == 'N' && CBP(c, 1, d) == 'N' && c->C.bcpre[2 * (d - 1)] == 0. && c->C.bcpre[2 * (d - 1) + 1] == 0.;
    // (walls: the normal component is prescribed -- with the homogeneous Neumann pressure its face values do not change in the projection --, the tangential
    //  ones no-slip or free-slip: either rule is an affine map of the mirrored interior cell, which the corrected view reads projected)
    for (int iv = 1; iv <= 3; ++iv) for (int sd = 0; sd <= 1; ++sd) { per = per && CBV(c, sd, d, iv) == 'P'; walls = walls && (CBV(c, sd, d, iv) == 'D' || (iv != d && CBV(c, sd, d, iv) == 'N')); }
    ok = per || walls;
  }
  return ok;
}
static bool fuse_cu_possible(const cales_ctx *c) { return !c->fl.unfused_correc && c->C.impdiff != 1; }     // updatep only needs pp: one pass with correc
// correction + pressure update of a substep as passes of their own, and the ghost cells of what they produced (main.f90:498-504)
static int project_now(cales_ctx *c, real dtrk, real alpha, int fmask) {
  const bool fuse_cu = fuse_cu_possible(c);
  if (int e = fuse_cu ? op_correc_updatep(c, dtrk, alpha, 1, fmask) : op_correc(c, dtrk, fmask)) return e;
  // the pressure is final once the fused correction has run: its ghost cells ride along with those of the velocity (one launch, one slab exchange)
  BcCall b;
  if (fuse_cu) b.rider(c->f[CALES_P], 0);
  if (int e = op_bounduvw(c, VelSet::state, 1, 1, b)) return e;
  if (!fuse_cu) { if (int e = op_updatep(c, alpha)) return e; if (int e = op_boundp(c, c->f[CALES_P], 0)) return e; }
  return 0;
}
// the ghost cells of everything a caller may look at, all directions (the corners of the x ghost columns with the z ghost planes included), when the
// step left the x ghost columns alone (step_xskip)
static int end_of_step_refresh(cales_ctx *c) {
  if (!c->step_xskip) return 0;
  c->step_xskip = false;
  BcCall b; b.rows_current = true;      // (only the x ghost columns are stale)
  b.rider(c->f[CALES_P], 0); b.rider(c->f[CALES_PP], 0); b.rider(c->f[CALES_VISCT], 1);
  if (int e = op_bounduvw(c, VelSet::state, 0, 1, b)) return e;
  if (!(CBV(c, 0, 3, 3) == 'P' && CBV(c, 1, 3, 3) == 'P')) { if (int e = op_xwrap_zghost(c, 3, c->f + CALES_U)) return e; }      // (periodic z: the z copies of the launch above cover the corners)
  return 0;
}
// the mode of a step in progress ends with the scope, on the error returns too
struct StepMode { cales_ctx *c; ~StepMode() { c->in_step = false; c->step_xskip = false; } };
// A projection that cales_step left to its successor (fold_mom, third substep) is completed here -- correction pass, ghost cells, and the refresh of
// the x ghost columns -- before anything else looks at the fields. Collective over the ranks like every entry of the C-ABI.
static int finish_pending(cales_ctx *c) {
  if (c->in_step || (c->pend.dtrk == 0. && !c->pend_xrefresh)) return 0;
  const PendingProjection pj = c->pend; const bool due = pj.dtrk != 0.;      // (not due: only the refresh of the x ghost columns is, cales_step with step_xskip)
  c->pend = PendingProjection(); c->pend_xrefresh = false;
  c->in_step = true; c->step_xskip = due ? pj.xskip : true;
  StepMode mode{c};
  int e = 0;
  if (due && pj.p_done) {      // (z-implicit diffusion: the pressure is up to date, ghost cells included)
    e = op_correc(c, pj.dtrk, pj.fmask);
    if (!e) e = op_bounduvw(c, VelSet::state, 1, 1);
  } else if (due) e = project_now(c, pj.dtrk, 0., pj.fmask);
  if (!e) e = end_of_step_refresh(c);      // (the completion ends with the refresh)
  if (e) { c->launch_err = std::string(due ? "completing a pending projection" : "refreshing the x ghost columns") + " failed (" + c->err + "): the context is unusable"; return e; }
  LAUNCHCHK(c);
  return 0;
}
// ---- the plan of a step (StepPlan, common.hpp): every decision about WHICH form of an operator a substep takes is made here, from the case, the
// switches and the state recorded in the plan's in_* fields -- step_body below only reads the result.
// The conditions of the plan known when the context is created (all but comm.on and the solver's radix-8 x plan -- ng(1)/2 a power of two or 3, 5, 9 times
// one, solver_setup; a row of whole 64-cell tiles that misses it, 448 cells say, gets companions it never uses): cales_create allocates the companion
// fields of fold_rows2 from them too (vel_comp). fillps inside the forward x transform: homogeneous pressure BCs (no boundary r.h.s.)
static bool fuse_fill_possible(const cales_ctx *c) {
  bool ok = !c->fl.unfused_fillps;
  for (int d = 0; d < 3; ++d) ok = ok && ((c->C.bcpre[2 * d] == 0. && c->C.bcpre[2 * d + 1] == 0.) || c->C.cbcpre[2 * d] == 'P');
  return ok;
}
// xskip: periodic x, explicit diffusion, no wall model, the fused passes everywhere -- every kernel of the step wraps around instead of reading x ghost
// columns, which are then left alone until the step returns (common.hpp, step_xskip). (The switches here and in fold_mom_ok, not MomPath::fused: cales_create
// asks through fold_correc_possible before mom_setup has run)
static bool xskip_possible(const cales_ctx *c) {
  const Flags &fl = c->fl;
  return !fl.xghosts_in_step && CBP(c, 0, 1) == 'P' && CBP(c, 1, 1) == 'P' && c->C.impdiff == 0 && !fl.unfused_rk && !fl.unfused_correc && c->sgs.wraps_x && !any_wm(c);
}
// fold_correc: dynamic model with |S|Sij as pair fields (SgsPath::pair: x and y periodic), z periodic or two no-slip walls, xskip: the projection
// u = u* - dtrk grad(pp) (+ the deferred forcing) and p += pp are folded into the strain-rate pass of cmpt_sgs, which reads the velocity anyway --
// the correction pass (9 words per cell) disappears (dsmag_fast, k_corr_strain_tile)
static bool fold_correc_possible(const cales_ctx *c) {
  bool ok = fuse_fill_possible(c) && xskip_possible(c) && c->sgs.pair && !c->fl.unfolded_correc && c->n[0] % 64 == 0;      // (whole 64-cell tiles in x)
  const bool perz = CBV(c, 0, 3, 3) == 'P' && CBV(c, 1, 3, 3) == 'P';
  bool walls = CBP(c, 0, 3) == 'N' && CBP(c, 1, 3) == 'N';
  for (int iv = 1; iv <= 3; ++iv) for (int sd = 0; sd <= 1; ++sd) walls = walls && CBV(c, sd, 3, iv) == 'D';
  // several slabs: the pass reaches the companion field of pp with 32-bit offsets (two fields under 4 GB)
  // (at least two rows per slab: row 2 goes to the companion field BEFORE the exchange, and with one row per slab "row 2" is the stale ghost row n2+1)
  return ok && (perz || walls) && (c->P == 1 || (c->n[1] >= 2 && 2 * (c->ntot + 2 * LINE_REALS) * sizeof(real) < (1ull << 32)));
}
static void make_plan(cales_ctx *c) {
  StepPlan pl;
  pl.valid = true;
  pl.in_visct_zero = c->visct_zero; pl.in_sgs_first = c->sgs_first;
  const Flags &fl = c->fl;
  pl.any_wm = any_wm(c);
  // (fuse_fill: the transform then also sums the bulk means of the forced components, whose increment only the correction kernel needs)
  pl.fuse_fill = fuse_fill_possible(c) && solver_can_fuse_fillps(c);
  pl.xskip = pl.fuse_fill && xskip_possible(c);
  pl.fold_correc = pl.xskip && fold_correc_possible(c) && (c->P == 1 || c->comm.on);      // (several slabs: through the slab hooks)
  // ... with a second ghost row of the prediction and a third of pp (the companion fields: vel_comp) the pass forms the ghost rows of all its outputs itself
  pl.fold_rows2 = pl.fold_correc && c->vel_comp;
  // no subgrid model, explicit or z-implicit diffusion, no wall model, every direction periodic or between walls with homogeneous Neumann pressure
  // (Taylor-Green, channels, cavities without a model): the projection and pressure update of substeps 1 and 2 are applied by the momentum pass of the
  // NEXT substep while it loads its planes (k_momrk<.., CORR = 1>) -- between the two the fields hold the prediction, whose ghost cells receive the
  // projected values through the corrected view of the ghost-cell kernels. The correction pass (9 words per cell) runs once per step instead of three times.
  pl.fold_mom = !pl.fold_correc && fold_mom_ok(c);
  // ... and the THIRD substep's projection may be left to the next step's first momentum pass (finish_pending for every other entry of the C-ABI). One rank
  // only: on several slabs completing it moves slab rows, which would turn every rank-local entry of the C-ABI into a hidden collective
  pl.lazy_last = pl.fold_mom && !fl.eager_projection && c->P == 1 && (fl.lazy_projection || (size_t)c->n[0] * c->n[1] * c->n[2] >= ((size_t)1 << 22));
  // z-implicit diffusion: the Helmholtz sweeps form their r.h.s. themselves (k_gaussel_cols_rhs); needs the shared-pivot form
  { const char *bz = &c->cbcvel[4];
    pl.defer_imp_rhs = c->C.impdiff == 2 && !fl.helmholtz_z_per_column && !fl.unfused_imp_rhs &&
                       !(bz[0] == 'P' && bz[1] == 'P') && !(bz[6] == 'P' && bz[7] == 'P') && !(bz[12] == 'P' && bz[13] == 'P'); }
  // Wall models: the bounduvw between bulk_forcing and fillps (main.f90:492-494) updates the wall-model planes and sets the tangential ghost cells of the
  // wall-model faces from them -- and nothing reads either before the bounduvw after correc (main.f90:500-501) has rewritten both: fillps differences the
  // normal components, the solver and boundp see pp, correc only adds to the cells. The one exception is a sampling height inside the first cell
  // (index_wm = 1 / n): that second wall-model update then interpolates with the ghost cell the first one left. Everywhere else the first update is
  // skipped (two launches per substep), with results identical to the last bit.
  { bool dead = !wm_samples_ghost(c);
    for (int sd = 0; sd <= 1; ++sd) if (LWM(c, sd, 1) != 0) dead = false;      // (wall-model faces in x: no reference-made vector holds this shortcut to account there)
    // (from the case alone, the same on every rank: the deferred forcing moves the all-reduce of the bulk means; CALES_UNMERGED_BC keeps the reference's
    //  full sequence: the A/B of the tests)
    pl.skip_first_wm = dead && pl.any_wm && !fl.unmerged_bc; }
  // explicit step, forced directions periodic: the velocity between the forcing and the correction is only differenced along the forced direction
  // (fillps) -- the increment is added by the correction kernel, one pass less. With a wall model only where its first update is skipped (above):
  // k_wallmodel would otherwise sample the velocity without the increment
  pl.fuse_cu = fuse_cu_possible(c);
  { bool ok = c->C.impdiff == 0 && pl.fuse_cu && !fl.unfused_forcing && (!pl.any_wm || pl.skip_first_wm);
    for (int d = 0; d < 3; ++d) if (c->C.is_forced[d]) ok = ok && c->cbcvel[6 * d + 2 * d] == 'P' && c->cbcvel[6 * d + 2 * d + 1] == 'P';
    pl.force_mask = (c->C.is_forced[0] ? 1 : 0) | (c->C.is_forced[1] ? 2 : 0) | (c->C.is_forced[2] ? 4 : 0);
    pl.defer_force = ok && pl.force_mask != 0; }
  pl.mean_mask = (pl.fuse_fill && pl.defer_force && !fl.unfused_mean) ? pl.force_mask : 0;
  pl.keep_last_rhs = fl.keep_last_rhs;
  // no subgrid model and homogeneous sgs BC values: the eddy viscosity is zero, ghost cells included, since start-up (sgs.f90:62-68; the first
  // cmpt_sgs of a context zeroes the whole field)
  pl.visct_ghosts = !(c->C.sgstype == 0 && (c->visct_zero || c->sgs_first));
  for (int q = 0; q < 6; ++q) if (c->C.bcsgs[q] != 0.) pl.visct_ghosts = true;
  c->plan = pl;
}
static const StepPlan &current_plan(cales_ctx *c) {
  const StepPlan &pl = c->plan;
  if (!pl.valid || pl.in_visct_zero != c->visct_zero || pl.in_sgs_first != c->sgs_first) make_plan(c);
  return c->plan;
}
int cales_describe_plan(cales_ctx *c, char *buf, int buflen) {
  if (!c || !buf || buflen < 1) return 1;
  const StepPlan &pl = current_plan(c);      // (reads no field: a pending projection stays pending)
  std::string s;
  s += std::string("projection=") + (pl.fold_rows2 ? "in_strain_rate_pass(ghost_rows_local)" : pl.fold_correc ? "in_strain_rate_pass" : pl.fold_mom ? (pl.lazy_last ? "in_next_momentum_pass(all_substeps)" : "in_next_momentum_pass(substeps_1_2)") : (pl.fuse_cu ? "own_pass(correc+updatep)" : "own_passes"));
  s += std::string(";x_ghost_columns=") + (pl.xskip ? "wrapped" : "maintained");
  s += std::string(";fillps=") + (pl.fuse_fill ? "in_x_transform" : "own_pass");
  s += std::string(";bulk_forcing=") + (pl.force_mask == 0 ? "none" : pl.defer_imp_rhs ? "in_helmholtz_sweep" : pl.defer_force ? (pl.mean_mask ? "in_correction(means_in_x_transform)" : "in_correction(means_own_pass)") : "own_pass");
  if (c->C.impdiff == 2) s += std::string(";implicit_rhs=") + (pl.defer_imp_rhs ? "in_helmholtz_sweep" : "own_pass");
  if (pl.any_wm) s += std::string(";first_wall_model_update=") + (pl.skip_first_wm ? "skipped" : "kept");
  s += std::string(";ghost_cells=") + (c->fl.unmerged_bc ? "by_direction" : "one_launch");
  s += std::string(";visct_ghost_cells=") + (pl.visct_ghosts ? "updated" : "zero_field");
  s += std::string(";momentum=") + (c->mom.fused ? "fused_mom_rk" : "mom+rk_update");
  s += std::string(";sgs=") + sgs_path_name(c);
  if (c->sgs.ave != SgsAve::planes) s += std::string(";sgs_average=") + (c->sgs.ave == SgsAve::volume ? "volume" : c->sgs.ave == SgsAve::xlines ? "x_lines" : "local");
  s += std::string(";solver=") + solver_path_name(c);
  if (c->C.impdiff == 1) for (int iv = 0; iv < 3; ++iv) s += std::string(";helmholtz_") + "uvw"[iv] + "=" + helmholtz_path_name(c, iv);
  if (c->P > 1) s += ";mode_columns_per_rank=" + std::to_string(solver_mode_columns(c));      // of the pressure solve (padded to whole 128-B lines where that costs 6 % or less: solver_setup)
  s += ";ranks=" + std::to_string(c->P) + ";exchanges=" + (c->P == 1 ? "none" : !c->comm.on ? "unset" : (c->comm.halo_second_stream || c->comm.a2a_second_stream) ? "second_stream" : "in_order");
  std::snprintf(buf, buflen, "%s", s.c_str());
  return (int)s.size() < buflen ? 0 : 2;      // 2: truncated
}

static int step_body(cales_ctx *c, real dt);
int cales_step(cales_ctx *c, real dt) {
  LAUNCHCHK(c);
  const int e = step_body(c, dt);
  LAUNCHCHK(c);
  // an error in the middle of a step leaves the fields between two operators (x ghost columns stale with step_xskip, a half-applied substep): the
  // context is marked failed so that operator-level calls cannot read that state as if it were a finished step
  if (e) { c->launch_err = "an earlier cales_step failed (" + c->err + "): the fields are in an intermediate state, the context is unusable"; return e; }
  return 0;
}
// One time step, src/main.f90:417-508. WHICH form every operator takes is the plan's (make_plan); what is left here is the sequence, and the plan's
// decisions go to the operators as arguments of each call.
static int step_body(cales_ctx *c, real dt) {
  const StepPlan pl = current_plan(c);      // (a copy: the plan of THIS step, whatever the step does to the state it was made from)
  if (c->pend.dtrk != 0. && !pl.fold_mom) { if (int e = finish_pending(c)) return e; }      // (the conditions changed between two steps: a field was set by hand)
  // The pending projection is this step's from here on: the one the step before left to this step's first momentum pass, then that of every substep that
  // folds. It goes back to the context in one place, at the end of a step that succeeded -- an error return leaves none behind
  PendingProjection pend = c->pend;
  c->pend = PendingProjection();
  op_zero_force(c, pend.dtrk != 0. ? 3 : 0, 6);     // dpdl(:) = 0, and f(:) unless a pending projection still needs its increments
  c->in_step = true;
  StepMode mode{c};
  if (c->pend_xrefresh && !pl.xskip) {      // the step before left the x ghost columns stale and this one reads them
    c->pend_xrefresh = false; c->step_xskip = true;
    if (int e = end_of_step_refresh(c)) return e;
  }
  c->step_xskip = pl.xskip;
  const int fmask = pl.defer_force ? pl.force_mask : 0;      // the components whose bulk-forcing increment the projection adds
  SgsFold fold{0., pl.fold_rows2, fmask};      // (pl.fold_correc: the projection each substep leaves to cmpt_sgs)
  for (int irk = 1; irk <= 3; ++irk) {
    const real dtrk = (RKPAR[irk - 1][0] + RKPAR[irk - 1][1]) * dt, dtrki = 1. / dtrk;
    real alpha = 0.;
    const bool p_ghosts_due = pend.dtrk != 0. && !pend.p_done;      // the momentum pass below stores p + pp of the interior cells: its ghost cells ride along with those of the prediction
    { RkOpts o; o.mean_mask = pl.mean_mask; o.rhs_in_sweep = pl.defer_imp_rhs; o.store_rhs = irk < 3 || pl.keep_last_rhs; o.pending = pend.dtrk != 0. ? &pend : nullptr;
      if (int e = op_rk(c, irk, dt, o)) return e;
      pend = PendingProjection(); }
    if (!pl.defer_force && !pl.defer_imp_rhs) { if (int e = op_bulk_forcing(c)) return e; }
    if (c->C.impdiff == 2) {
      alpha = -.5 * c->visc * dtrk;
      const real hf12 = .5 * (RKPAR[irk - 1][0] * dt + RKPAR[irk - 1][1] * dt);      // (rounded as rk rounds the factor of its own implicit part)
      for (int iv = 1; iv <= 3; ++iv) if (int e = op_helmholtz_z(c, iv, alpha, pl.defer_imp_rhs, hf12)) return e;
    } else if (c->C.impdiff == 1) {
      alpha = -.5 * c->visc * dtrk;
      for (int iv = 1; iv <= 3; ++iv) if (int e = op_helmholtz(c, iv, alpha)) return e;
    }
    { BcCall b; b.skip_wm = pl.skip_first_wm;
      if (p_ghosts_due) b.rider(c->f[CALES_P], 0);
      // (two ghost rows of the prediction, fold_rows2: the rows 2 / n2-1 travel to the neighbours' companion fields in the same message as the rows 1 / n2)
      HaloBatch rows; if (pl.fold_rows2) b.collect = &rows;
      if (int e = op_bounduvw(c, VelSet::state, 1, 0, b)) return e;
      if (pl.fold_rows2) {
        if (int e = halo_rows(c, 3, c->f + CALES_U, HaloRows::second_rows, b)) return e;
        if (int e = halo_flush(c, rows, false)) return e;
      } }
    if (!pl.fuse_fill) { if (int e = op_fillps(c, dtrki)) return e; if (int e = op_updt_rhs_b(c)) return e; }
    if (int e = op_solver(c, pl.fuse_fill ? FusedFill{dtrki, pl.mean_mask} : FusedFill())) return e;
    if (pl.fold_rows2) {
      // three ghost rows of pp above (n2+1, and n2+2, n2+3 in the ghost rows n2+1 of its two companions), two below (0, and -1 in the first companion's row 0):
      // ONE exchange, behind the ghost-cell kernel (whole rows travel: the x and z ghost cells the kernel gave them included)
      HaloBatch rows; BcCall b; b.collect = &rows;
      real *one[1] = {c->f[CALES_PP]};
      if (int e = op_boundp(c, c->f[CALES_PP], 0, b)) return e;
      if (int e = halo_rows(c, 1, one, HaloRows::second_rows, b)) return e;
      if (int e = halo_rows(c, 1, one, HaloRows::third_rows, b)) return e;
      if (int e = halo_flush(c, rows, false)) return e;
    } else
    if (pl.fold_correc && c->P > 1) {
      // the folded projection corrects v in the ghost row n2+1 too and needs pp one row further out: row 2 of every slab goes to row 1 of pp's companion
      // field and both fields take the ghost-cell update -- ONE exchange; the upper neighbour's row 2 arrives in the companion's ghost row n2+1
      LAUNCH(c, k_row2_to_companion, dim3((c->n[0] + 2 + 63) / 64, (c->n[2] + 2 + 3) / 4), dim3(64, 4), 0, c->stream, c->g, c->f[CALES_PP], c->scr2);
      real *two[2] = {c->f[CALES_PP], c->scr2};
      if (int e = op_boundp_multi(c, 2, two, 0)) return e;
    } else
    if (int e = op_boundp(c, c->f[CALES_PP], 0)) return e;
    if (pl.fold_correc) {      // correc, bounduvw, updatep, boundp(p): inside the cmpt_sgs below (dsmag_fast)
      fold.dtrk = dtrk;
    } else if (pl.fold_mom && (irk < 3 || pl.lazy_last)) {
      // the ghost cells of the projected velocity now (through the corrected view), its interior cells and p + pp in the next momentum pass -- the next
      // substep's, or after the third substep the next step's (finish_pending for every other entry of the C-ABI)
      pend.dtrk = dtrk; pend.fmask = fmask; pend.xskip = pl.xskip;
      if (c->C.impdiff == 2) {      // z-implicit diffusion: the pressure update keeps its own pass (updatep.f90:40-46) -- the z Laplacian of pp has no values in ghost cells
        if (int e = op_updatep(c, alpha)) return e;
        if (int e = op_boundp(c, c->f[CALES_P], 0)) return e;
        pend.p_done = true;
      }
      BcCall b; b.view_dtrk = pend.dtrk; b.view_fmask = pend.fmask;
      if (int e = op_bounduvw(c, VelSet::state, 1, 1, b)) return e;
    } else if (int e = project_now(c, dtrk, alpha, fmask)) return e;
    bool visct_ghosts_done = false;
    if (int e = op_cmpt_sgs(c, pl.fold_correc ? &fold : nullptr, &visct_ghosts_done)) return e;
    if (pl.visct_ghosts && !visct_ghosts_done) { if (int e = op_boundp(c, c->f[CALES_VISCT], 1)) return e; }
  }
  if (pend.dtrk != 0.) c->pend = pend;      // (lazy_last) the last projection is the next step's (or finish_pending's), the refresh with it
  else if (c->step_xskip && !c->fl.eager_projection) c->pend_xrefresh = true;      // the x ghost columns wait for the first caller that is not the next step (finish_pending)
  else if (int e = end_of_step_refresh(c)) return e;
  c->step_dt = dt;
  return 0;
}
int cales_get_dpdl(cales_ctx *c, real dpdl[3]) {
  if (int e = read_back(c, c->h_red + RedLayout::H_FORCE, c->d_force, 6)) return e;      // (f and dpdl, back to back)
  const real dti = 1. / c->step_dt;
  for (int q = 0; q < 3; ++q) dpdl[q] = -c->h_red[RedLayout::H_DPDL + q] * dti;
  return 0;
}

// ------------------------------------------------------------------------------------------ multi-GPU hooks
int cales_comm_buffer_doubles(const cales_ctx *c, int64_t *n) {
  *n = c->stage.total;      // (StageLayout, common.hpp)
  return 0;
}
int cales_set_comm(cales_ctx *c, cales_halo_cb halo, cales_alltoall_cb a2a, cales_allreduce_cb allred, void *user,
                   real *bufA, real *bufB, int64_t nbuf) {
  if (!halo || !a2a || !allred || !bufA || !bufB || nbuf < c->stage.total) { c->err = "cales_set_comm: missing callback/buffer or buffers too small"; return 1; }
  c->comm.halo = halo; c->comm.a2a = a2a; c->comm.allred = allred; c->comm.user = user;
  c->comm.A = bufA; c->comm.B = bufB; c->comm.nbuf = nbuf; c->comm.on = true;
  HIPCHK(c, hipMemsetAsync(bufA, 0, nbuf * sizeof(real), c->stream));
  HIPCHK(c, hipMemsetAsync(bufB, 0, nbuf * sizeof(real), c->stream));
  return comm_changed(c);      // (the reduction results move into the tail of A, where the host can all-reduce them in place)
}
int cales_set_comm_overlap(cales_ctx *c, cales_halo_s_cb halo_s, cales_alltoall_part_cb a2a_part) {
  if (!c->comm.on) { c->err = "cales_set_comm_overlap: call cales_set_comm first"; return 1; }
  if (!c->fl.overlap) return 0;      // default: every exchange in order on the one stream; CALES_OVERLAP=1 opts into the second stream (Flags::read_env)
  if (!c->comm_stream) {      // highest priority: the send/receive kernels of an exchange should get their few workgroups at once, beside a full grid
    int least = 0, greatest = 0;
    HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(c, hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, greatest));
  }
  c->comm.halo_s = halo_s; c->comm.a2a_part = a2a_part;
  return comm_changed(c);
}
int cales_initflow_slab(const cales_case *cs, const char *inivel, int is_wallturb, real *u, real *v, real *w, real *p) {
  if (!cs || !inivel || !u || !v || !w || !p) return 1;
  return hs_initflow(cs, inivel, is_wallturb, u, v, w, p, cs->rank, cs->nranks);
}

// ------------------------------------------------------------------------------------------ measurement
int cales_profile_enable(cales_ctx *c, int on) { prof_flush(c); c->prof = on != 0; return 0; }
int cales_profile_reset(cales_ctx *c) { prof_flush(c); c->stats.clear(); return 0; }
int cales_profile_count(cales_ctx *c) { prof_flush(c); return (int)c->stats.size(); }
int cales_profile_get(cales_ctx *c, int idx, char *name, int namelen, int64_t *calls, real *total_ms) {
  prof_flush(c);
  if (idx < 0 || idx >= (int)c->stats.size()) return 1;
  if (name && namelen > 0) std::snprintf(name, namelen, "%s", c->stats[idx].name.c_str());
  if (calls) *calls = c->stats[idx].calls;
  if (total_ms) *total_ms = c->stats[idx].ms;
  return 0;
}
int cales_calibrate(cales_ctx *c, int reps, real gbps[3], int64_t *bytes_per_stream) {
  if (!c || !gbps || reps < 1) return 1;
  ENTER(c);      // (completes a pending projection: the scratch field written below is then dead)
  const long nrows = (long)(c->n[1] + 2) * (c->n[2] + 2);
  const double bytes = (double)nrows * c->n[0] * sizeof(real);
  if (bytes_per_stream) *bytes_per_stream = (int64_t)bytes;
  struct Event { hipEvent_t e = nullptr; ~Event() { if (e) hipEventDestroy(e); } } ev0, ev1;      // destroyed on every return
  HIPCHK(c, hipEventCreate(&ev0.e)); HIPCHK(c, hipEventCreate(&ev1.e));
  const hipEvent_t e0 = ev0.e, e1 = ev1.e;
  const dim3 gr(256 * 16), bl(256);
  const real *a = c->f[CALES_U]; real *b = c->scr1;      // scr1: scratch between operators
  auto run = [&](int mode) {
    const auto k_calib_rows_mode = mode == 0 ? k_calib_rows<0> : mode == 1 ? k_calib_rows<1> : k_calib_rows<2>;
    LAUNCH(c, k_calib_rows_mode, gr, bl, 0, c->stream, c->g, nrows, a, b, c->d_red + c->red.part);      // (sink: the reductions' partials, never written)
  };
  int rc = 0;
  for (int mode = 0; mode < 3 && !rc; ++mode) {
    run(mode);
    if (hipEventRecord(e0, c->stream) != hipSuccess) { rc = 1; break; }
    for (int r = 0; r < reps; ++r) run(mode);
    if (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) { rc = 1; break; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || !(ms > 0.f)) { rc = 1; break; }
    gbps[mode] = (real)((mode == 2 ? 2. : 1.) * bytes * reps / (ms * 1e-3) / 1e9);
  }
  if (rc) { c->err = "cales_calibrate: event timing failed"; return rc; }
  LAUNCHCHK(c);
  return 0;
}
int cales_device_info(cales_ctx *c, char *name, int namelen, int64_t *hbm_bytes) {
  hipDeviceProp_t p; int dev = 0;
  HIPCHK(c, hipGetDevice(&dev)); HIPCHK(c, hipGetDeviceProperties(&p, dev));
  if (name && namelen > 0) std::snprintf(name, namelen, "%s (%s)", p.name, p.gcnArchName);
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return 0;
}

}  // extern "C"
