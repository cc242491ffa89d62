// Per-plane histograms of a field and joint histograms of two fields (include/cales_pdf.h): the kernels and their host side. The only kernels of the
// library that scatter: every block counts its samples into 32-bit counters in LDS (atomicAdd on __shared__ memory), keeps the samples that fall
// outside the range in registers, and adds its non-zero counters to the 64-bit counts in global memory with one atomicAdd each. The sums are integers:
// exact, independent of the order in which the blocks arrive, the same bits from run to run.
#include "readout.hpp"
#include "../../include/cales_pdf.h"

typedef unsigned long long u64;

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
// may be shorter), read in `chunks` 16-byte chunks per row (read_rows16, readout.hpp)
struct PdfGeom { int rows, chunks; };

__global__ __launch_bounds__(256) void k_pdf_planes(Geom g, PdfGeom pg, int nb, real lo, real s, const real *__restrict__ f, u64 *__restrict__ counts, u64 *__restrict__ outside) {
  extern __shared__ unsigned cnt[];      // nb counters
  const int k = blockIdx.y + 1, j0 = blockIdx.x * pg.rows + 1, nrows = min(pg.rows, g.n2 - j0 + 1);
  for (int b = threadIdx.x; b < nb; b += 256) cnt[b] = 0u;
  __syncthreads();
  unsigned below = 0u, above = 0u;
  read_rows16<1>(g, pg.chunks, j0, nrows, k, f, nullptr, [&](int, int, real x) {
    const int b = pdf_bin(x, lo, s, nb);
    if (b < 0) ++below; else if (b >= nb) ++above; else atomicAdd(&cnt[b], 1u);
  });
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
  read_rows16<2>(g, pg.chunks, j0, nrows, k, fa, fb, [&](int, int, real xa, real xb) {
    const int a = pdf_bin(xa, lo_a, s_a, nb), b = pdf_bin(xb, lo_b, s_b, nb);
    if (a < 0 || a >= nb || b < 0 || b >= nb) ++out; else atomicAdd(&cnt[a + nb * b], 1u);
  });
  __syncthreads();
  u64 *dst = counts + (size_t)nc * (size_t)blockIdx.y;
  for (int b = threadIdx.x; b < nc; b += 256) { const unsigned v = cnt[b]; if (v) atomicAdd(&dst[b], (u64)v); }
  out = wave_sum_u32(out);
  if ((threadIdx.x & 63) == 0 && out) atomicAdd(&outside[blockIdx.y], (u64)out);
}

// ------------------------------------------------------------------------------------------ host side
// Rows per block (row_runs, readout.hpp): no block with fewer samples than it has counters to clear and flush, or fewer than 4096; *nbx: the blocks of a plane
static PdfGeom pdf_geom(const cales_ctx *c, int nplanes, int ncounters, unsigned *nbx) {
  const int n1 = c->n[0], least = std::max(4096, ncounters);
  const RowRuns rr = row_runs(c->n[1], nplanes, (least + n1 - 1) / n1, 1);
  *nbx = (unsigned)rr.per_plane;
  return PdfGeom{rr.rows, (n1 + REALV - 1) / REALV};
}
// s of the bin rule; refuses a range that is not one
static int pdf_scale(cales_ctx *c, int nbins, real lo, real hi, const char *who, real *s) {
  if (!std::isfinite(lo) || !std::isfinite(hi)) { c->err = std::string(who) + ": lo and hi must be finite"; return 1; }
  if (!(hi > lo)) { c->err = std::string(who) + ": hi <= lo"; return 1; }
  *s = (real)nbins / (hi - lo);
  return 0;
}

int op_pdf_planes(cales_ctx *c, int field, int nbins, real lo, real hi, int64_t *counts, int64_t *outside) {
  const char *who = "cales_pdf_planes";
  if (!field_ptr(c, field, who, FIELD_ROWS16)) return 1;
  if (nbins < 1 || nbins > CALES_PDF_MAX_BINS) { c->err = std::string(who) + ": nbins must be 1 ... " + std::to_string(CALES_PDF_MAX_BINS); return 1; }
  real s;
  if (pdf_scale(c, nbins, lo, hi, who, &s)) return 1;
  if (!counts) { c->err = std::string(who) + ": counts is NULL"; return 1; }
  const real *f = field_ptr(c, field, who, FIELD_READ); if (!f) return 1;
  const int n3 = c->n[2];
  const size_t ncnt = (size_t)nbins * n3;
  TempCarver tc; const auto p_counts = tc.part<u64>(ncnt), p_out = tc.part<u64>(2 * (size_t)n3);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  u64 *d_counts = p_counts.in(tmp.p), *d_out = p_out.in(tmp.p);
  unsigned nbx; const PdfGeom pg = pdf_geom(c, n3, nbins, &nbx);
  { ProfScope ps(c, "pdf_planes");
    HIPCHK(c, hipMemsetAsync(tmp.p, 0, tc.bytes, c->stream));
    const dim3 grid(nbx, n3), block(256); const size_t lds = (size_t)nbins * sizeof(unsigned);
    LAUNCH(c, k_pdf_planes, grid, block, lds, c->stream, c->g, pg, nbins, lo, s, f, d_counts, d_out); }
  LAUNCHCHK(c);
  if (int e = read_back_queued(c, counts, d_counts, ncnt)) return e;
  if (outside) if (int e = read_back_queued(c, outside, d_out, 2 * (size_t)n3)) return e;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int op_jpdf_planes(cales_ctx *c, int field_a, int field_b, int nbins, real lo_a, real hi_a, real lo_b, real hi_b, int nplanes, const int32_t *kplanes,
                   int64_t *counts, int64_t *outside) {
  const char *who = "cales_jpdf_planes";
  if (!field_ptr(c, field_a, who, FIELD_ROWS16) || !field_ptr(c, field_b, who, FIELD_ROWS16)) return 1;
  if (nbins < 1 || nbins > CALES_JPDF_MAX_BINS) { c->err = std::string(who) + ": nbins must be 1 ... " + std::to_string(CALES_JPDF_MAX_BINS); return 1; }
  real s_a, s_b;
  if (pdf_scale(c, nbins, lo_a, hi_a, who, &s_a) || pdf_scale(c, nbins, lo_b, hi_b, who, &s_b)) return 1;
  if (!counts) { c->err = std::string(who) + ": counts is NULL"; return 1; }
  if (plane_list_check(who, nplanes, kplanes, c->C.ng[2], c->err)) return 1;
  const real *fa = field_ptr(c, field_a, who, FIELD_READ), *fb = field_ptr(c, field_b, who, FIELD_READ); if (!fa || !fb) return 1;
  const size_t nc = (size_t)nbins * nbins, ncnt = nc * (size_t)nplanes;
  TempCarver tc; const auto p_counts = tc.part<u64>(ncnt), p_out = tc.part<u64>(nplanes); const auto p_k = tc.part<int32_t>(nplanes);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  u64 *d_counts = p_counts.in(tmp.p), *d_out = p_out.in(tmp.p); int32_t *d_k = p_k.in(tmp.p);
  unsigned nbx; const PdfGeom pg = pdf_geom(c, nplanes, (int)nc, &nbx);
  if (int e = plane_list_upload(c, d_k, kplanes, nplanes)) return e;
  { ProfScope ps(c, "jpdf_planes");
    HIPCHK(c, hipMemsetAsync(tmp.p, 0, p_k.at, c->stream));      // the counters: everything in front of the planes
    const dim3 grid(nbx, nplanes), block(256); const size_t lds = nc * sizeof(unsigned);
    LAUNCH(c, k_jpdf_planes, grid, block, lds, c->stream, c->g, pg, nbins, lo_a, s_a, lo_b, s_b, d_k, fa, fb, d_counts, d_out); }
  LAUNCHCHK(c);
  if (int e = read_back_queued(c, counts, d_counts, ncnt)) return e;
  if (outside) if (int e = read_back_queued(c, outside, d_out, (size_t)nplanes)) return e;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
