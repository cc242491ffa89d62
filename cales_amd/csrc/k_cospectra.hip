// Cross-spectra of two fields along x, along y and in x-y planes (include/cales_cospectra.h): the kernels and their host side. The line transform, its plan,
// the twiddle table and the LDS sizing are those of the power spectra (spectral_line.hpp); what is new here is that a block keeps lines of TWO fields.
//
// Pairing: two real lines ride in one complex transform, and both come from the SAME field -- rows (columns) r and r+1 of field a form one complex line,
// rows r and r+1 of field b another. A row of a with a row of b in one transform would leave in F^b, after the Hermitian split (spec_pair), a rounding
// error proportional to the norm of a: with u and its mean of tens of u_tau against w the cross-spectrum would lose its relative accuracy.
//
// LDS: the nl complex lines of spec_nl (spectral_line.hpp: 64 KB soft, 128 KB at the cap) are split half and half, nl / 2 complex lines = nl real lines of
// either field; in a batch of nc <= nl / 2 complex lines per field those of a are lines 0 ... nc-1 and those of b lines nc ... 2 nc - 1, so that one
// spec_transform of 2 nc lines serves both. At the cap (N = 2048 in double) that is one complex line per field: a batch is two rows of each field.
// Sums over lines are formed in a fixed order and without atomics, as in k_spectra.hip: a thread owns its modes, adds the lines of its block in line
// order and writes ONE partial per block; k_cospec_fold adds the blocks of a plane in block order. The same bits from run to run.
#include "spectral_line.hpp"
#include "../../include/cales_cospectra.h"

// a conj(b)
__host__ __device__ inline real2 cmulc(real2 a, real2 b) { return make_real2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }

// a thread's sums over the lines of its block: the modes m = threadIdx.x + 256 u
struct CospecAcc {
  real2 cr[SPEC_MPT], sa[SPEC_MPT], sb[SPEC_MPT];      // F^a conj(F^b) | F^a | F^b
  __device__ inline void clear() {
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) cr[u] = sa[u] = sb[u] = make_real2((real)0., (real)0.);
  }
  // the real lines 2c and 2c+1 of either field, from the transformed complex lines c (of a) and nc + c (of b), c = 0 ... nc - 1, in that order
  __device__ inline void add(const real2 *__restrict__ Z, int N, int nh, int nreal) {
    const int nc = (nreal + 1) / 2;
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) {
      const int m = threadIdx.x + 256 * u;
      if (m >= nh) continue;
      for (int c = 0; c < nc; ++c) {
        real2 a0, a1, b0, b1;
        spec_pair(Z + c * N, N, m, &a0, &a1); spec_pair(Z + (nc + c) * N, N, m, &b0, &b1);
        cr[u] = cadd(cr[u], cmulc(a0, b0)); sa[u] = cadd(sa[u], a0); sb[u] = cadd(sb[u], b0);
        if (2 * c + 1 < nreal) { cr[u] = cadd(cr[u], cmulc(a1, b1)); sa[u] = cadd(sa[u], a1); sb[u] = cadd(sb[u], b1); }
      }
    }
  }
  // one partial per block: cross (nh complex) | sum of a (nh complex) | sum of b (nh complex)
  __device__ inline void store(real2 *__restrict__ dst, int nh) const {
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) {
      const int m = threadIdx.x + 256 * u;
      if (m < nh) { dst[m] = cr[u]; dst[nh + m] = sa[u]; dst[2 * nh + m] = sb[u]; }
    }
  }
};

// x lines. blockIdx.y: the plane (k = blockIdx.y + 1, or the entry of kplanes), blockIdx.x: a run of sg.rows consecutive rows of it (the last run may be
// shorter), taken sg.nl rows at a time: rows r and r+1 of a batch of nr rows are real and imaginary part of complex line r/2 (field a) and nc + r/2
// (field b), nc = ceil(nr / 2); both fields are read at the same index in sg.chunks 16-byte chunks per row (read_rows16<2>, readout.hpp).
// PLANES = false: F^a conj(F^b), F^a and F^b summed over the rows of the block in row order, one partial per block (CospecAcc::store) at
//                 part[(blockIdx.y nb + blockIdx.x) 3 nh]
// PLANES = true:  the rows' transforms F(0 ... n1/2) go to rows_out[((2 blockIdx.y + field) n2 + j - 1) nh + m], field = 0 (a), 1 (b)
template <bool PLANES>
__global__ __launch_bounds__(256) void k_cospec_x(Geom g, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const int32_t *__restrict__ kplanes,
                                                  const real *__restrict__ fa, const real *__restrict__ fb, real2 *__restrict__ part, real2 *__restrict__ rows_out) {
  extern __shared__ real2 spec_lds[];      // 2 nl N
  const int N = pl.n, nh = sg.nh;
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int k = kplanes ? kplanes[blockIdx.y] : (int)blockIdx.y + 1, j0 = blockIdx.x * sg.rows + 1, nrows = min(sg.rows, g.n2 - j0 + 1);
  CospecAcc acc; acc.clear();
  for (int r0 = 0; r0 < nrows; r0 += sg.nl) {
    const int nr = min(sg.nl, nrows - r0), nc = (nr + 1) / 2;
    read_rows16<2>(g, sg.chunks, j0 + r0, nr, k, fa, fb, [&](int r, int i, real xa, real xb) {
      ((real *)(A + (r >> 1) * N + (i - 1)))[r & 1] = xa; ((real *)(A + (nc + (r >> 1)) * N + (i - 1)))[r & 1] = xb; });
    if (nr & 1) for (int i = threadIdx.x; i < N; i += 256) A[(nc - 1) * N + i].y = A[(2 * nc - 1) * N + i].y = (real)0.;      // the odd last row rides alone
    __syncthreads();
    const real2 *Z = spec_transform(pl, tw, 2 * nc, A, B);
    if (PLANES) {
      for (int w = threadIdx.x; w < 2 * nr * nh; w += 256) {
        const int fr = w / nh, m = w - fr * nh, fld = fr / nr, r = fr - fld * nr;
        real2 f0, f1; spec_pair(Z + (fld * nc + (r >> 1)) * N, N, m, &f0, &f1);
        rows_out[((size_t)(2 * blockIdx.y + fld) * g.n2 + (size_t)(j0 - 1 + r0 + r)) * nh + m] = (r & 1) ? f1 : f0;
      }
    } else acc.add(Z, N, nh, nr);
    __syncthreads();      // the next batch overwrites both buffers
  }
  if (!PLANES) acc.store(part + ((size_t)blockIdx.y * sg.nb + blockIdx.x) * 3 * (size_t)nh, nh);
}

// y lines of plane k = blockIdx.y + 1. blockIdx.x: a tile of sg.nl adjacent columns from i0 = 1 + nl blockIdx.x (the last tile may hold fewer), read from
// both fields; columns c and c+1 of the tile are real and imaginary part of complex line c/2 (field a) and nc + c/2 (field b). Every row of the tile is
// sg.chunks 16-byte chunks per field, masked past n1 as read_rows16 masks them; a tile narrower than a chunk (sg.chunks = 0: nl = 2 in single
// precision) is read element by element. The sums over the columns of the tile in column order, one partial per tile at part[(blockIdx.y nb + blockIdx.x) 3 nh]
__global__ __launch_bounds__(256) void k_cospec_y(Geom g, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const real *__restrict__ fa, const real *__restrict__ fb,
                                                  real2 *__restrict__ part) {
  extern __shared__ real2 spec_lds[];
  const int N = pl.n, nh = sg.nh;      // N = n2
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int k = blockIdx.y + 1, i0 = 1 + sg.nl * blockIdx.x, ncols = min(sg.nl, g.n1 - i0 + 1), nc = (ncols + 1) / 2;
  if (sg.chunks > 0) {
    for (int q = threadIdx.x; q < N * sg.chunks; q += 256) {
      const int j = q / sg.chunks, col = REALV * (q - j * sg.chunks), i = i0 + col;
      if (i > g.n1) continue;
      const size_t at = g.ix(i, j + 1, k);
      real ea[REALV], eb[REALV]; realv_unpack(*(const realv *)(fa + at), ea); realv_unpack(*(const realv *)(fb + at), eb);
#pragma unroll
      for (int t = 0; t < REALV; ++t) if (i + t <= g.n1) {
        ((real *)(A + ((col + t) >> 1) * N + j))[(col + t) & 1] = ea[t]; ((real *)(A + (nc + ((col + t) >> 1)) * N + j))[(col + t) & 1] = eb[t];
      }
    }
  } else {
    for (int q = threadIdx.x; q < N * ncols; q += 256) {
      const int j = q / ncols, col = q - j * ncols;
      const size_t at = g.ix(i0 + col, j + 1, k);
      ((real *)(A + (col >> 1) * N + j))[col & 1] = fa[at]; ((real *)(A + (nc + (col >> 1)) * N + j))[col & 1] = fb[at];
    }
  }
  if (ncols & 1) for (int j = threadIdx.x; j < N; j += 256) A[(nc - 1) * N + j].y = A[(2 * nc - 1) * N + j].y = (real)0.;      // the odd last column rides alone
  __syncthreads();
  const real2 *Z = spec_transform(pl, tw, 2 * nc, A, B);
  CospecAcc acc; acc.clear();
  acc.add(Z, N, nh, ncols);
  acc.store(part + ((size_t)blockIdx.y * sg.nb + blockIdx.x) * 3 * (size_t)nh, nh);
}

// the y pass of the plane cross-spectra: blockIdx.y a plane of the chunk, blockIdx.x a tile of nl / 2 adjacent columns m of the complex rows of BOTH
// fields (nhx = n1/2+1 per row, what k_cospec_x<true> wrote): the columns of a are lines 0 ... ncol-1, the same columns of b lines ncol ... 2 ncol - 1.
// Transforms every column along y (N = n2 points), forms H^a conj(H^b) at (m, ky), adds ky and n2 - ky where the two differ and writes
// cross2(0:1, m, q, plane), q = 0 ... n2/2: no sum across blocks
__global__ __launch_bounds__(256) void k_cospec_y2(int nhx, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const real2 *__restrict__ rows, real2 *__restrict__ cross2) {
  extern __shared__ real2 spec_lds[];
  const int N = pl.n, nhy = sg.nh, nlh = sg.nl / 2;
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int m0 = nlh * blockIdx.x, ncol = min(nlh, nhx - m0);
  const real2 *src = rows + (size_t)2 * blockIdx.y * N * nhx + m0;
  for (int q = threadIdx.x; q < 2 * N * ncol; q += 256) {
    const int fj = q / ncol, c = q - fj * ncol, fld = fj / N, j = fj - fld * N;
    A[(fld * ncol + c) * N + j] = src[(size_t)fj * nhx + c];      // (the rows of b follow the n2 rows of a)
  }
  __syncthreads();
  const real2 *Z = spec_transform(pl, tw, 2 * ncol, A, B);
  real2 *dst = cross2 + (size_t)blockIdx.y * nhx * nhy + m0;
  for (int w = threadIdx.x; w < ncol * nhy; w += 256) {
    const int q = w / ncol, c = w - q * ncol, ky2 = q ? N - q : 0;
    real2 v = cmulc(Z[c * N + q], Z[(ncol + c) * N + q]);
    if (ky2 != q) v = cadd(v, cmulc(Z[c * N + ky2], Z[(ncol + c) * N + ky2]));
    dst[(size_t)q * nhx + c] = v;
  }
}

// the partials of the nb blocks of every plane, added in block order: cross, lsum_a, lsum_b, each (2, nh, nplanes)
__global__ __launch_bounds__(256) void k_cospec_fold(int nh, int nb, int nplanes, const real2 *__restrict__ part, real2 *__restrict__ cross, real2 *__restrict__ lsa, real2 *__restrict__ lsb) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nh * nplanes) return;
  const int k = t / nh, m = t - k * nh;
  const real2 *p = part + (size_t)k * nb * 3 * nh + m;
  real2 cr = make_real2((real)0., (real)0.), sa = cr, sb = cr;
  for (int b = 0; b < nb; ++b, p += 3 * nh) { cr = cadd(cr, p[0]); sa = cadd(sa, p[nh]); sb = cadd(sb, p[2 * nh]); }
  cross[t] = cr; lsa[t] = sa; lsb[t] = sb;
}

// ------------------------------------------------------------------------------------------ host side
// runs of rows per block of the x kernel (row_runs, readout.hpp): whole batches of nl rows -- nl / 2 complex lines of either field
static void cospec_x_geom(const cales_ctx *c, int nplanes, SpecGeom *sg) {
  const int n1 = c->n[0];
  sg->nl = spec_nl(n1); sg->nh = n1 / 2 + 1; sg->chunks = (n1 + REALV - 1) / REALV;
  const RowRuns rr = row_runs(c->n[1], nplanes, 1, sg->nl);
  sg->rows = rr.rows; sg->nb = rr.per_plane;
}
// the two field ids of a call, before anything else is looked at (nothing is materialised yet)
static int cospec_fields_ok(cales_ctx *c, int field_a, int field_b, const char *who) {
  return field_ptr(c, field_a, who, FIELD_ROWS16) && field_ptr(c, field_b, who, FIELD_ROWS16);
}

int op_cospectra_lines(cales_ctx *c, int field_a, int field_b, int idir, real *cross, real *lsum_a, real *lsum_b) {
  const char *who = "cales_cospectra_lines";
  if (!cospec_fields_ok(c, field_a, field_b, who)) return 1;
  if (idir != 1 && idir != 2) { c->err = std::string(who) + ": idir must be 1 or 2"; return 1; }
  if (idir == 2 && c->P > 1) { c->err = std::string(who) + ": idir = 2 on one rank only (a slab holds no whole y line)"; return 1; }
  const int n1 = c->n[0], n2 = c->n[1], n3 = c->n[2], N = idir == 1 ? n1 : n2;
  if (spec_line_ok(c, N, who)) return 1;
  if (!cross) { c->err = std::string(who) + ": cross is NULL"; return 1; }
  const real *fa = field_ptr(c, field_a, who, FIELD_READ), *fb = field_ptr(c, field_b, who, FIELD_READ); if (!fa || !fb) return 1;
  const SpecPlan pl = spec_plan(N);
  SpecGeom sg;
  if (idir == 1) cospec_x_geom(c, n3, &sg);
  else { sg.nl = spec_nl(N); sg.nh = N / 2 + 1; sg.rows = 0; sg.chunks = sg.nl / REALV; sg.nb = (n1 + sg.nl - 1) / sg.nl; }
  const int nh = sg.nh;
  const size_t lds = spec_lds_bytes(sg.nl, N);
  if (idir == 1 ? spec_lds_attr(c, k_cospec_x<false>, lds) : spec_lds_attr(c, k_cospec_y, lds)) return 1;
  const size_t n_out = (size_t)nh * n3;      // complex values of each result
  TempCarver tc; const auto p_tw = tc.part<real2>(N), p_part = tc.part<real2>((size_t)n3 * sg.nb * 3 * nh), p_cr = tc.part<real2>(n_out), p_la = tc.part<real2>(n_out), p_lb = tc.part<real2>(n_out);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  real2 *d_tw = p_tw.in(tmp.p), *d_part = p_part.in(tmp.p), *d_cr = p_cr.in(tmp.p), *d_la = p_la.in(tmp.p), *d_lb = p_lb.in(tmp.p);
  { ProfScope ps(c, pl.direct ? "cospectra_lines_direct" : "cospectra_lines");
    LAUNCH(c, k_spec_twiddle, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, d_tw);
    const dim3 grid(sg.nb, n3), block(256);
    if (idir == 1) LAUNCH(c, k_cospec_x<false>, grid, block, lds, c->stream, c->g, sg, pl, d_tw, (const int32_t *)nullptr, fa, fb, d_part, (real2 *)nullptr);
    else LAUNCH(c, k_cospec_y, grid, block, lds, c->stream, c->g, sg, pl, d_tw, fa, fb, d_part);
    LAUNCH(c, k_cospec_fold, dim3((nh * n3 + 255) / 256), block, 0, c->stream, nh, sg.nb, n3, d_part, d_cr, d_la, d_lb); }
  LAUNCHCHK(c);
  if (int e = read_back_queued(c, cross, d_cr, 2 * n_out)) return e;
  if (lsum_a) if (int e = read_back_queued(c, lsum_a, d_la, 2 * n_out)) return e;
  if (lsum_b) if (int e = read_back_queued(c, lsum_b, d_lb, 2 * n_out)) return e;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int op_cospectra_planes(cales_ctx *c, int field_a, int field_b, int nplanes, const int32_t *kplanes, real *cross2) {
  const char *who = "cales_cospectra_planes";
  if (!cospec_fields_ok(c, field_a, field_b, who)) return 1;
  if (c->P > 1) { c->err = std::string(who) + ": one rank only (a slab holds no whole y line)"; return 1; }
  const int n1 = c->n[0], n2 = c->n[1];
  if (spec_line_ok(c, n1, who) || spec_line_ok(c, n2, who)) return 1;
  if (!cross2) { c->err = std::string(who) + ": cross2 is NULL"; return 1; }
  if (plane_list_check(who, nplanes, kplanes, c->C.ng[2], c->err)) return 1;
  const real *fa = field_ptr(c, field_a, who, FIELD_READ), *fb = field_ptr(c, field_b, who, FIELD_READ); if (!fa || !fb) return 1;
  const SpecPlan plx = spec_plan(n1), ply = spec_plan(n2);
  const int nhx = n1 / 2 + 1, nhy = n2 / 2 + 1;
  // the complex rows of a plane of BOTH fields take about as much as two planes of a field: as many planes at a time as 32 MB of scratch hold, one at least
  const size_t plane_rows = 2 * (size_t)nhx * n2, plane_out = (size_t)nhx * nhy;
  const int chunk = (int)std::min<size_t>((size_t)nplanes, std::max<size_t>(1, ((size_t)32 << 20) / (plane_rows * sizeof(real2))));
  SpecGeom sx; cospec_x_geom(c, chunk, &sx);
  SpecGeom sy; sy.nl = spec_nl(n2); sy.nh = nhy; sy.rows = 0; sy.chunks = 0; sy.nb = (nhx + sy.nl / 2 - 1) / (sy.nl / 2);
  const size_t ldsx = spec_lds_bytes(sx.nl, n1), ldsy = spec_lds_bytes(sy.nl, n2);
  if (spec_lds_attr(c, k_cospec_x<true>, ldsx) || spec_lds_attr(c, k_cospec_y2, ldsy)) return 1;
  // twiddles of x | of y | the complex rows of a chunk, both fields | its cross2 | the planes
  TempCarver tc; const auto p_twx = tc.part<real2>(n1), p_twy = tc.part<real2>(n2), p_rows = tc.part<real2>(plane_rows * chunk), p_out = tc.part<real2>(plane_out * chunk);
  const auto p_k = tc.part<int32_t>(nplanes);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  real2 *d_twx = p_twx.in(tmp.p), *d_twy = p_twy.in(tmp.p), *d_rows = p_rows.in(tmp.p), *d_out = p_out.in(tmp.p); int32_t *d_k = p_k.in(tmp.p);
  if (int e = plane_list_upload(c, d_k, kplanes, nplanes)) return e;
  { ProfScope ps(c, (plx.direct || ply.direct) ? "cospectra_planes_direct" : "cospectra_planes");
    const dim3 block(256);
    LAUNCH(c, k_spec_twiddle, dim3((n1 + 255) / 256), block, 0, c->stream, n1, d_twx);
    LAUNCH(c, k_spec_twiddle, dim3((n2 + 255) / 256), block, 0, c->stream, n2, d_twy);
    for (int p0 = 0; p0 < nplanes; p0 += chunk) {
      const int np = std::min(chunk, nplanes - p0);
      LAUNCH(c, k_cospec_x<true>, dim3(sx.nb, np), block, ldsx, c->stream, c->g, sx, plx, d_twx, (const int32_t *)(d_k + p0), fa, fb, (real2 *)nullptr, d_rows);
      LAUNCH(c, k_cospec_y2, dim3(sy.nb, np), block, ldsy, c->stream, nhx, sy, ply, d_twy, d_rows, d_out);
      if (int e = read_back_queued(c, cross2 + 2 * plane_out * p0, d_out, 2 * plane_out * np)) return e;
    } }
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
