// Per-plane histograms of a field and joint histograms of two fields (include/cales_pdf.h): the kernels and their host side. The only kernels of the
// library that scatter: every block counts its samples into 32-bit counters in LDS (atomicAdd on __shared__ memory), keeps the samples that fall
// outside the range in registers, and adds its non-zero counters to the 64-bit counts in global memory with one atomicAdd each. The sums are integers:
// exact, independent of the order in which the blocks arrive, the same bits from run to run.
#include "common.hpp"
#include "../../include/cales_pdf.h"
#include <algorithm>

typedef unsigned long long u64;
#ifdef CALES_SINGLE
typedef float4 realv;      // 16 bytes per lane
#else
typedef double2 realv;
#endif
constexpr int PDF_VEC = 16 / RSZ;

// The bin rule of include/cales_pdf.h to the letter: t = (x - lo) * s, that subtraction then that multiplication (no contraction: there is no sum
// after the product, and the pragma says so); -1: below, nb: above (x >= hi, +inf, NaN, a t rounded up to nb), otherwise the bin
__device__ inline int pdf_bin(real x, real lo, real s, int nb) {
#pragma clang fp contract(off)
  const real d = x - lo;
  const real t = d * s;
  if (t < (real)0.) return -1;
  if (!(t < (real)nb)) return nb;
  return (int)t;
}
// sum over the 64 lanes of a wave (every lane takes part), the total in lane 0
__device__ inline unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}
// What a launch of either kernel walks: blocks of 256 threads, blockIdx.y the plane, blockIdx.x a run of `rows` rows of it (the last run of a plane
// may be shorter). A row is read in chunks of PDF_VEC elements from element 1, which sits on a 128-B boundary in every row (Geom); the last chunk of
// a row may reach past n1 into the pitch padding or the next row's first element -- inside the field's allocation, and masked out.
struct PdfGeom { int rows, chunks; };

__global__ __launch_bounds__(256) void k_pdf_planes(Geom g, PdfGeom pg, int nb, real lo, real s, const real *__restrict__ f, u64 *__restrict__ counts, u64 *__restrict__ outside) {
  extern __shared__ unsigned cnt[];      // nb counters
  const int k = blockIdx.y + 1, j0 = blockIdx.x * pg.rows + 1, nrows = min(pg.rows, g.n2 - j0 + 1);
  for (int b = threadIdx.x; b < nb; b += 256) cnt[b] = 0u;
  __syncthreads();
  unsigned below = 0u, above = 0u;
  auto tally = [&](real x) {
    const int b = pdf_bin(x, lo, s, nb);
    if (b < 0) ++below; else if (b >= nb) ++above; else atomicAdd(&cnt[b], 1u);
  };
  const int nq = nrows * pg.chunks;
  for (int q = threadIdx.x; q < nq; q += 256) {
    const int r = q / pg.chunks, i = 1 + PDF_VEC * (q - r * pg.chunks);
    const realv v = *(const realv *)(f + g.ix(i, j0 + r, k));
    tally(v.x);
    if (i + 1 <= g.n1) tally(v.y);
#ifdef CALES_SINGLE
    if (i + 2 <= g.n1) tally(v.z);
    if (i + 3 <= g.n1) tally(v.w);
#endif
  }
  __syncthreads();
  u64 *out = counts + (size_t)nb * (size_t)(k - 1);
  for (int b = threadIdx.x; b < nb; b += 256) { const unsigned v = cnt[b]; if (v) atomicAdd(&out[b], (u64)v); }
  below = wave_sum_u32(below); above = wave_sum_u32(above);
  if ((threadIdx.x & 63) == 0) {
    if (below) atomicAdd(&outside[2 * (size_t)(k - 1)], (u64)below);
    if (above) atomicAdd(&outside[2 * (size_t)(k - 1) + 1], (u64)above);
  }
}
// the joint form: blockIdx.y the entry of kplanes, nb x nb counters (first axis: field a), one tally of the samples with either variable outside
__global__ __launch_bounds__(256) void k_jpdf_planes(Geom g, PdfGeom pg, int nb, real lo_a, real s_a, real lo_b, real s_b, const int32_t *__restrict__ kplanes,
                                                     const real *__restrict__ fa, const real *__restrict__ fb, u64 *__restrict__ counts, u64 *__restrict__ outside) {
  extern __shared__ unsigned cnt[];      // nb * nb counters
  const int k = kplanes[blockIdx.y], j0 = blockIdx.x * pg.rows + 1, nrows = min(pg.rows, g.n2 - j0 + 1), nc = nb * nb;
  for (int b = threadIdx.x; b < nc; b += 256) cnt[b] = 0u;
  __syncthreads();
  unsigned out = 0u;
  auto tally = [&](real xa, real xb) {
    const int a = pdf_bin(xa, lo_a, s_a, nb), b = pdf_bin(xb, lo_b, s_b, nb);
    if (a < 0 || a >= nb || b < 0 || b >= nb) ++out; else atomicAdd(&cnt[a + nb * b], 1u);
  };
  const int nq = nrows * pg.chunks;
  for (int q = threadIdx.x; q < nq; q += 256) {
    const int r = q / pg.chunks, i = 1 + PDF_VEC * (q - r * pg.chunks);
    const size_t c = g.ix(i, j0 + r, k);
    const realv va = *(const realv *)(fa + c), vb = *(const realv *)(fb + c);
    tally(va.x, vb.x);
    if (i + 1 <= g.n1) tally(va.y, vb.y);
#ifdef CALES_SINGLE
    if (i + 2 <= g.n1) tally(va.z, vb.z);
    if (i + 3 <= g.n1) tally(va.w, vb.w);
#endif
  }
  __syncthreads();
  u64 *dst = counts + (size_t)nc * (size_t)blockIdx.y;
  for (int b = threadIdx.x; b < nc; b += 256) { const unsigned v = cnt[b]; if (v) atomicAdd(&dst[b], (u64)v); }
  out = wave_sum_u32(out);
  if ((threadIdx.x & 63) == 0 && out) atomicAdd(&outside[blockIdx.y], (u64)out);
}

// ------------------------------------------------------------------------------------------ host side
// Rows per block: enough blocks to fill the device (about 2048 over the planes), but no block with fewer samples than it has counters to clear and
// flush, or fewer than 4096; *nbx: the blocks of a plane
static PdfGeom pdf_geom(const cales_ctx *c, int nplanes, int ncounters, unsigned *nbx) {
  const int n1 = c->n[0], n2 = c->n[1];
  const int want = (2048 + nplanes - 1) / nplanes, least = std::max(4096, ncounters);
  int rows = std::max((n2 + want - 1) / want, (least + n1 - 1) / n1);
  rows = std::min(std::max(rows, 1), n2);
  *nbx = (unsigned)((n2 + rows - 1) / rows);
  return PdfGeom{rows, (n1 + PDF_VEC - 1) / PDF_VEC};
}
static int pdf_field(cales_ctx *c, int field, const char *who) {
  if (field < 0 || field >= CALES_NFIELDS || !c->f[field]) { c->err = std::string(who) + ": bad field id"; return 1; }
  // the kernels load 16 bytes per lane from element 1 of a row, which every field of a context has on a 128-B boundary (field_alloc, api.hip)
  if (((uintptr_t)(c->f[field] + 1) & 15u) != 0) { c->err = std::string(who) + ": the field's rows are not 16-byte aligned"; return 1; }
  return 0;
}
// s of the bin rule; refuses a range that is not one
static int pdf_scale(cales_ctx *c, int nbins, real lo, real hi, const char *who, real *s) {
  if (!std::isfinite(lo) || !std::isfinite(hi)) { c->err = std::string(who) + ": lo and hi must be finite"; return 1; }
  if (!(hi > lo)) { c->err = std::string(who) + ": hi <= lo"; return 1; }
  *s = (real)nbins / (hi - lo);
  return 0;
}
// n 64-bit integers in a temporary of reals
static size_t reals_for_i64(size_t n) { return (n * sizeof(int64_t) + sizeof(real) - 1) / sizeof(real); }
static int read_back_i64(cales_ctx *c, int64_t *host, const u64 *dev, size_t n) {
  HIPCHK(c, hipMemcpyAsync(host, dev, n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int op_pdf_planes(cales_ctx *c, int field, int nbins, real lo, real hi, int64_t *counts, int64_t *outside) {
  const char *who = "cales_pdf_planes";
  if (pdf_field(c, field, who)) return 1;
  if (nbins < 1 || nbins > CALES_PDF_MAX_BINS) { c->err = std::string(who) + ": nbins must be 1 ... " + std::to_string(CALES_PDF_MAX_BINS); return 1; }
  real s;
  if (pdf_scale(c, nbins, lo, hi, who, &s)) return 1;
  if (!counts) { c->err = std::string(who) + ": counts is NULL"; return 1; }
  if (field == CALES_VISCT) if (int e = materialize_visct(c)) return e;
  const int n3 = c->n[2];
  const size_t ncnt = (size_t)nbins * n3, nall = ncnt + 2 * (size_t)n3;
  CtxTemp tmp(c, reals_for_i64(nall)); if (!tmp.p) return 1;
  u64 *d_counts = (u64 *)tmp.p, *d_out = d_counts + ncnt;
  unsigned nbx; const PdfGeom pg = pdf_geom(c, n3, nbins, &nbx);
  { ProfScope ps(c, "pdf_planes");
    HIPCHK(c, hipMemsetAsync(d_counts, 0, nall * sizeof(u64), c->stream));
    const dim3 grid(nbx, n3), block(256); const size_t lds = (size_t)nbins * sizeof(unsigned);
    LAUNCH(c, k_pdf_planes, grid, block, lds, c->stream, c->g, pg, nbins, lo, s, c->f[field], d_counts, d_out); }
  LAUNCHCHK(c);
  if (int e = read_back_i64(c, counts, d_counts, ncnt)) return e;
  if (outside) if (int e = read_back_i64(c, outside, d_out, 2 * (size_t)n3)) return e;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int op_jpdf_planes(cales_ctx *c, int field_a, int field_b, int nbins, real lo_a, real hi_a, real lo_b, real hi_b, int nplanes, const int32_t *kplanes,
                   int64_t *counts, int64_t *outside) {
  const char *who = "cales_jpdf_planes";
  if (pdf_field(c, field_a, who) || pdf_field(c, field_b, who)) return 1;
  if (nbins < 1 || nbins > CALES_JPDF_MAX_BINS) { c->err = std::string(who) + ": nbins must be 1 ... " + std::to_string(CALES_JPDF_MAX_BINS); return 1; }
  real s_a, s_b;
  if (pdf_scale(c, nbins, lo_a, hi_a, who, &s_a) || pdf_scale(c, nbins, lo_b, hi_b, who, &s_b)) return 1;
  if (!counts) { c->err = std::string(who) + ": counts is NULL"; return 1; }
  if (nplanes < 1) { c->err = std::string(who) + ": nplanes < 1"; return 1; }
  if (!kplanes) { c->err = std::string(who) + ": kplanes is NULL"; return 1; }
  for (int p = 0; p < nplanes; ++p) if (kplanes[p] < 1 || kplanes[p] > c->C.ng[2]) { c->err = std::string(who) + ": plane outside 1 ... ng(3)"; return 1; }
  if (field_a == CALES_VISCT || field_b == CALES_VISCT) if (int e = materialize_visct(c)) return e;
  const size_t nc = (size_t)nbins * nbins, ncnt = nc * (size_t)nplanes, nall = ncnt + (size_t)nplanes;
  // counts | outside | the planes (32-bit, behind the 64-bit integers)
  CtxTemp tmp(c, reals_for_i64(nall + ((size_t)nplanes + 1) / 2)); if (!tmp.p) return 1;
  u64 *d_counts = (u64 *)tmp.p, *d_out = d_counts + ncnt; int32_t *d_k = (int32_t *)(d_out + nplanes);
  unsigned nbx; const PdfGeom pg = pdf_geom(c, nplanes, (int)nc, &nbx);
  HIPCHK(c, hipMemcpyAsync(d_k, kplanes, (size_t)nplanes * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  { ProfScope ps(c, "jpdf_planes");
    HIPCHK(c, hipMemsetAsync(d_counts, 0, nall * sizeof(u64), c->stream));
    const dim3 grid(nbx, nplanes), block(256); const size_t lds = nc * sizeof(unsigned);
    LAUNCH(c, k_jpdf_planes, grid, block, lds, c->stream, c->g, pg, nbins, lo_a, s_a, lo_b, s_b, d_k, c->f[field_a], c->f[field_b], d_counts, d_out); }
  LAUNCHCHK(c);
  if (int e = read_back_i64(c, counts, d_counts, ncnt)) return e;
  if (outside) if (int e = read_back_i64(c, outside, d_out, (size_t)nplanes)) return e;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
