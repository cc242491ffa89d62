// Power spectra of a field along x, along y and in x-y planes (include/cales_spectra.h): the kernels and their host side. A translation unit of its own
// with a line transform of its own -- the transforms of the pressure solve (k_solver.hip) are neither called nor touched. The transform, its plan and the
// LDS sizing are in spectral_line.hpp, which the cross-spectra (k_cospectra.hip) include as well.
//
// The line lives in LDS: up to `nl` complex lines of N points in buffer A, a second buffer B of the same size, and a complex Stockham transform that
// goes back and forth between the two, one stage per factor 4, 2, 3 or 5 of N (spec_stage). Twiddles exp(-2 pi I t / N), t = 0 ... N-1, come from a
// table in global memory that a small kernel fills once per call (evaluated in double, rounded once). A line whose length has another prime factor
// takes the plain sum over its points (spec_direct): correct, O(N^2), the profile scope then carries the suffix _direct. Two REAL lines ride in one
// complex transform as real and imaginary part and are told apart by the Hermitian symmetry (spec_pair); an odd last line rides alone.
//
// LDS per block = 2 buffers x nl lines x N x sizeof(real2), nl = 8 halved until that fits 64 KB, but not below 2 (spec_nl):
//   double: N <= 256: nl = 8, at most 64 KB | N <= 512: nl = 4, 64 KB | N <= 1024: nl = 2, 64 KB | N <= 2048 (the cap): nl = 2, 128 KB
//   float:  N <= 512: nl = 8, at most 64 KB | N <= 1024: nl = 4, 64 KB | N <= 2048: nl = 2, 64 KB
//   the smallest lines (N = 1, 2): nl = 8, 256 B / 512 B.
// Sums over lines are formed in a fixed order and without atomics: a thread owns its modes, adds the lines of its block in line order and writes ONE
// partial per block; k_spec_fold adds the blocks of a plane in block order. The same bits from run to run.
#include "spectral_line.hpp"

// a thread's sums over the lines of its block: the modes m = threadIdx.x + 256 u
struct SpecAcc {
  real pw[SPEC_MPT], sr[SPEC_MPT], si[SPEC_MPT];
  __device__ inline void clear() {
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) pw[u] = sr[u] = si[u] = (real)0.;
  }
  // the real lines 2c and 2c+1 of the transformed complex lines c = 0 ... (nreal+1)/2 - 1, in that order
  __device__ inline void add(const real2 *__restrict__ Z, int N, int nh, int nreal) {
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) {
      const int m = threadIdx.x + 256 * u;
      if (m >= nh) continue;
      for (int c = 0; 2 * c < nreal; ++c) {
        real2 fa, fb; spec_pair(Z + c * N, N, m, &fa, &fb);
        pw[u] += cabs2(fa); sr[u] += fa.x; si[u] += fa.y;
        if (2 * c + 1 < nreal) { pw[u] += cabs2(fb); sr[u] += fb.x; si[u] += fb.y; }
      }
    }
  }
  // one partial per block: power(nh) | real part (nh) | imaginary part (nh)
  __device__ inline void store(real *__restrict__ dst, int nh) const {
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) {
      const int m = threadIdx.x + 256 * u;
      if (m < nh) { dst[m] = pw[u]; dst[nh + m] = sr[u]; dst[2 * nh + m] = si[u]; }
    }
  }
};

// x lines. blockIdx.y: the plane (k = blockIdx.y + 1, or the entry of kplanes), blockIdx.x: a run of sg.rows consecutive rows of it (the last run may be
// shorter), taken 2 nl rows at a time: rows r and r+1 of a batch are real and imaginary part of complex line r/2, read in sg.chunks 16-byte chunks per row
// (read_rows16, readout.hpp).
// PLANES = false: |F|^2 and F summed over the rows of the block in row order, one partial per block (SpecAcc::store) at part[(blockIdx.y nb + blockIdx.x) 3 nh]
// PLANES = true:  the rows' transforms F(0 ... n1/2) go to rows_out[(blockIdx.y n2 + j - 1) nh + m]
template <bool PLANES>
__global__ __launch_bounds__(256) void k_spec_x(Geom g, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const int32_t *__restrict__ kplanes,
                                                const real *__restrict__ f, real *__restrict__ part, real2 *__restrict__ rows_out) {
  extern __shared__ real2 spec_lds[];      // 2 nl N
  const int N = pl.n, nh = sg.nh;
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int k = kplanes ? kplanes[blockIdx.y] : (int)blockIdx.y + 1, j0 = blockIdx.x * sg.rows + 1, nrows = min(sg.rows, g.n2 - j0 + 1);
  SpecAcc acc; acc.clear();
  for (int r0 = 0; r0 < nrows; r0 += 2 * sg.nl) {
    const int nr = min(2 * sg.nl, nrows - r0), nc = (nr + 1) / 2;
    read_rows16<1>(g, sg.chunks, j0 + r0, nr, k, f, nullptr, [&](int r, int i, real x) { ((real *)(A + (r >> 1) * N + (i - 1)))[r & 1] = x; });
    if (nr & 1) for (int i = threadIdx.x; i < N; i += 256) A[(nc - 1) * N + i].y = (real)0.;      // the odd last row rides alone
    __syncthreads();
    const real2 *Z = spec_transform(pl, tw, nc, A, B);
    if (PLANES) {
      for (int w = threadIdx.x; w < nr * nh; w += 256) {
        const int r = w / nh, m = w - r * nh;
        real2 fa, fb; spec_pair(Z + (r >> 1) * N, N, m, &fa, &fb);
        const bool odd = r & 1;
        rows_out[((size_t)blockIdx.y * g.n2 + (size_t)(j0 - 1 + r0 + r)) * nh + m] = make_real2(odd ? fb.x : fa.x, odd ? fb.y : fa.y);
      }
    } else acc.add(Z, N, nh, nr);
    __syncthreads();      // the next batch overwrites both buffers
  }
  if (!PLANES) acc.store(part + ((size_t)blockIdx.y * sg.nb + blockIdx.x) * 3 * (size_t)nh, nh);
}

// y lines of plane k = blockIdx.y + 1. blockIdx.x: a tile of 2 nl adjacent columns from i0 = 1 + 2 nl blockIdx.x (the last tile may hold fewer), columns
// c and c+1 of the tile real and imaginary part of complex line c/2. Every row of the tile is sg.chunks 16-byte chunks (with nl = 8 in double one whole
// 128-B segment); a chunk that starts past n1 is not read, one that reaches past n1 is masked as read_rows16 masks it. |G|^2 and G summed over the columns of the tile
// in column order, one partial per tile at part[(blockIdx.y nb + blockIdx.x) 3 nh]
__global__ __launch_bounds__(256) void k_spec_y(Geom g, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const real *__restrict__ f, real *__restrict__ part) {
  extern __shared__ real2 spec_lds[];
  const int N = pl.n, nh = sg.nh;      // N = n2
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int k = blockIdx.y + 1, i0 = 1 + 2 * sg.nl * blockIdx.x, ncols = min(2 * sg.nl, g.n1 - i0 + 1), nc = (ncols + 1) / 2;
  for (int q = threadIdx.x; q < N * sg.chunks; q += 256) {
    const int j = q / sg.chunks, col = REALV * (q - j * sg.chunks), i = i0 + col;
    if (i > g.n1) continue;
    real e[REALV]; realv_unpack(*(const realv *)(f + g.ix(i, j + 1, k)), e);
#pragma unroll
    for (int t = 0; t < REALV; ++t) if (i + t <= g.n1) ((real *)(A + ((col + t) >> 1) * N + j))[(col + t) & 1] = e[t];
  }
  if (ncols & 1) for (int j = threadIdx.x; j < N; j += 256) A[(nc - 1) * N + j].y = (real)0.;      // the odd last column rides alone
  __syncthreads();
  const real2 *Z = spec_transform(pl, tw, nc, A, B);
  SpecAcc acc; acc.clear();
  acc.add(Z, N, nh, ncols);
  acc.store(part + ((size_t)blockIdx.y * sg.nb + blockIdx.x) * 3 * (size_t)nh, nh);
}

// the y pass of the plane spectra: blockIdx.y a plane of the chunk, blockIdx.x a tile of nl adjacent columns m of its complex rows (nhx = n1/2+1 per row,
// what k_spec_x<true> wrote). Transforms every column along y (N = n2 points), forms |H(m, ky)|^2, adds ky and n2 - ky where the two differ and writes
// power2(m, q, plane), q = 0 ... n2/2: no sum across blocks
__global__ __launch_bounds__(256) void k_spec_y2(int nhx, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const real2 *__restrict__ rows, real *__restrict__ power2) {
  extern __shared__ real2 spec_lds[];
  const int N = pl.n, nhy = sg.nh;
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int m0 = sg.nl * blockIdx.x, ncol = min(sg.nl, nhx - m0);
  const real2 *src = rows + (size_t)blockIdx.y * N * nhx + m0;
  for (int q = threadIdx.x; q < N * ncol; q += 256) {
    const int j = q / ncol, c = q - j * ncol;
    A[c * N + j] = src[(size_t)j * nhx + c];
  }
  __syncthreads();
  const real2 *Z = spec_transform(pl, tw, ncol, A, B);
  real *dst = power2 + (size_t)blockIdx.y * nhx * nhy + m0;
  for (int w = threadIdx.x; w < ncol * nhy; w += 256) {
    const int q = w / ncol, c = w - q * ncol, ky2 = q ? N - q : 0;
    real v = cabs2(Z[c * N + q]);
    if (ky2 != q) v += cabs2(Z[c * N + ky2]);
    dst[(size_t)q * nhx + c] = v;
  }
}

// the partials of the nb blocks of every plane, added in block order: power(nh, nplanes), lsum(2, nh, nplanes)
__global__ __launch_bounds__(256) void k_spec_fold(int nh, int nb, int nplanes, const real *__restrict__ part, real *__restrict__ power, real *__restrict__ lsum) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nh * nplanes) return;
  const int k = t / nh, m = t - k * nh;
  const real *p = part + (size_t)k * nb * 3 * nh + m;
  real pw = 0., sr = 0., si = 0.;
  for (int b = 0; b < nb; ++b, p += 3 * nh) { pw += p[0]; sr += p[nh]; si += p[2 * nh]; }
  power[t] = pw; lsum[2 * (size_t)t] = sr; lsum[2 * (size_t)t + 1] = si;
}

// ------------------------------------------------------------------------------------------ host side (plan, LDS sizing, row runs: spectral_line.hpp)
int op_spectra_lines(cales_ctx *c, int field, int idir, real *power, real *lsum) {
  const char *who = "cales_spectra_lines";
  if (!field_ptr(c, field, who, FIELD_ROWS16)) return 1;
  if (idir != 1 && idir != 2) { c->err = std::string(who) + ": idir must be 1 or 2"; return 1; }
  if (idir == 2 && c->P > 1) { c->err = std::string(who) + ": idir = 2 on one rank only (a slab holds no whole y line)"; return 1; }
  const int n1 = c->n[0], n2 = c->n[1], n3 = c->n[2], N = idir == 1 ? n1 : n2;
  if (spec_line_ok(c, N, who)) return 1;
  if (!power) { c->err = std::string(who) + ": power is NULL"; return 1; }
  const real *f = field_ptr(c, field, who, FIELD_READ); if (!f) return 1;
  const SpecPlan pl = spec_plan(N);
  SpecGeom sg;
  if (idir == 1) spec_x_geom(c, n3, &sg);
  else { sg.nl = spec_nl(N); sg.nh = N / 2 + 1; sg.rows = 0; sg.chunks = 2 * sg.nl / REALV; sg.nb = (n1 + 2 * sg.nl - 1) / (2 * sg.nl); }
  const int nh = sg.nh;
  const size_t lds = spec_lds_bytes(sg.nl, N);
  if (idir == 1 ? spec_lds_attr(c, k_spec_x<false>, lds) : spec_lds_attr(c, k_spec_y, lds)) return 1;
  const size_t n_pow = (size_t)nh * n3, n_ls = 2 * n_pow;
  TempCarver tc; const auto p_tw = tc.part<real2>(N); const auto p_part = tc.part<real>((size_t)n3 * sg.nb * 3 * nh), p_pow = tc.part<real>(n_pow), p_ls = tc.part<real>(n_ls);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  real2 *d_tw = p_tw.in(tmp.p); real *d_part = p_part.in(tmp.p), *d_pow = p_pow.in(tmp.p), *d_ls = p_ls.in(tmp.p);
  { ProfScope ps(c, pl.direct ? "spectra_lines_direct" : "spectra_lines");
    LAUNCH(c, k_spec_twiddle, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, d_tw);
    const dim3 grid(sg.nb, n3), block(256);
    if (idir == 1) LAUNCH(c, k_spec_x<false>, grid, block, lds, c->stream, c->g, sg, pl, d_tw, (const int32_t *)nullptr, f, d_part, (real2 *)nullptr);
    else LAUNCH(c, k_spec_y, grid, block, lds, c->stream, c->g, sg, pl, d_tw, f, d_part);
    LAUNCH(c, k_spec_fold, dim3((nh * n3 + 255) / 256), block, 0, c->stream, nh, sg.nb, n3, d_part, d_pow, d_ls); }
  LAUNCHCHK(c);
  if (int e = read_back_queued(c, power, d_pow, n_pow)) return e;
  if (lsum) if (int e = read_back_queued(c, lsum, d_ls, n_ls)) return e;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int op_spectra_planes(cales_ctx *c, int field, int nplanes, const int32_t *kplanes, real *power2) {
  const char *who = "cales_spectra_planes";
  if (!field_ptr(c, field, who, FIELD_ROWS16)) return 1;
  if (c->P > 1) { c->err = std::string(who) + ": one rank only (a slab holds no whole y line)"; return 1; }
  const int n1 = c->n[0], n2 = c->n[1];
  if (spec_line_ok(c, n1, who) || spec_line_ok(c, n2, who)) return 1;
  if (!power2) { c->err = std::string(who) + ": power2 is NULL"; return 1; }
  if (plane_list_check(who, nplanes, kplanes, c->C.ng[2], c->err)) return 1;
  const real *f = field_ptr(c, field, who, FIELD_READ); if (!f) return 1;
  const SpecPlan plx = spec_plan(n1), ply = spec_plan(n2);
  const int nhx = n1 / 2 + 1, nhy = n2 / 2 + 1;
  // the complex rows of a plane take about as much as a plane of the field: as many planes at a time as 32 MB of scratch hold, one at least
  const size_t plane_rows = (size_t)nhx * n2, plane_out = (size_t)nhx * nhy;
  const int chunk = (int)std::min<size_t>((size_t)nplanes, std::max<size_t>(1, ((size_t)32 << 20) / (plane_rows * sizeof(real2))));
  SpecGeom sx; spec_x_geom(c, chunk, &sx);
  SpecGeom sy; sy.nl = spec_nl(n2); sy.nh = nhy; sy.rows = 0; sy.chunks = 0; sy.nb = (nhx + sy.nl - 1) / sy.nl;
  const size_t ldsx = spec_lds_bytes(sx.nl, n1), ldsy = spec_lds_bytes(sy.nl, n2);
  if (spec_lds_attr(c, k_spec_x<true>, ldsx) || spec_lds_attr(c, k_spec_y2, ldsy)) return 1;
  // twiddles of x | of y | the complex rows of a chunk | its power2 | the planes
  TempCarver tc; const auto p_twx = tc.part<real2>(n1), p_twy = tc.part<real2>(n2), p_rows = tc.part<real2>(plane_rows * chunk);
  const auto p_out = tc.part<real>(plane_out * chunk); const auto p_k = tc.part<int32_t>(nplanes);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  real2 *d_twx = p_twx.in(tmp.p), *d_twy = p_twy.in(tmp.p), *d_rows = p_rows.in(tmp.p);
  real *d_out = p_out.in(tmp.p); int32_t *d_k = p_k.in(tmp.p);
  if (int e = plane_list_upload(c, d_k, kplanes, nplanes)) return e;
  { ProfScope ps(c, (plx.direct || ply.direct) ? "spectra_planes_direct" : "spectra_planes");
    const dim3 block(256);
    LAUNCH(c, k_spec_twiddle, dim3((n1 + 255) / 256), block, 0, c->stream, n1, d_twx);
    LAUNCH(c, k_spec_twiddle, dim3((n2 + 255) / 256), block, 0, c->stream, n2, d_twy);
    for (int p0 = 0; p0 < nplanes; p0 += chunk) {
      const int np = std::min(chunk, nplanes - p0);
      LAUNCH(c, k_spec_x<true>, dim3(sx.nb, np), block, ldsx, c->stream, c->g, sx, plx, d_twx, (const int32_t *)(d_k + p0), f, (real *)nullptr, d_rows);
      LAUNCH(c, k_spec_y2, dim3(sy.nb, np), block, ldsy, c->stream, nhx, sy, ply, d_twy, d_rows, d_out);
      if (int e = read_back_queued(c, power2 + plane_out * p0, d_out, plane_out * np)) return e;
    } }
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
