// Power spectra of a field (include/cales_spectra.h) and cross-spectra of two fields (include/cales_cospectra.h) along x, along y and in x-y planes: the
// kernels and their host side, both templated on NF = 1 or 2, the number of fields. A translation unit of its own with a line transform of its own --
// the transforms of the pressure solve (k_solver.hip) are neither called nor touched. The transform, its plan, the LDS sizing and the launch geometry
// are in spectral_line.hpp.
//
// The line lives in LDS: up to `nl` complex lines of N points in buffer A, a second buffer B of the same size, and a complex Stockham transform that
// goes back and forth between the two, one stage per factor 4, 2, 3 or 5 of N (spec_stage). Twiddles exp(-2 pi I t / N), t = 0 ... N-1, come from a
// table in global memory that a small kernel fills once per call (evaluated in double, rounded once). A line whose length has another prime factor
// takes the plain sum over its points (spec_direct): correct, O(N^2), the profile scope then carries the suffix _direct. Two REAL lines ride in one
// complex transform as real and imaginary part and are told apart by the Hermitian symmetry (spec_pair); an odd last line rides alone.
//
// Pairing: the two real lines of a transform come from the SAME field -- rows (columns) r and r+1 of field a form one complex line, rows r and r+1 of
// field b another. A row of a with a row of b in one transform would leave in F^b, after the Hermitian split, a rounding error proportional to the
// norm of a: with u and its mean of tens of u_tau against w the cross-spectrum would lose its relative accuracy.
//
// LDS per block = 2 buffers x nl lines x N x sizeof(real2), nl = 8 halved until that fits 64 KB, but not below 2 (spec_nl):
//   double: N <= 256: nl = 8, at most 64 KB | N <= 512: nl = 4, 64 KB | N <= 1024: nl = 2, 64 KB | N <= 2048 (the cap): nl = 2, 128 KB
//   float:  N <= 512: nl = 8, at most 64 KB | N <= 1024: nl = 4, 64 KB | N <= 2048: nl = 2, 64 KB
//   the smallest lines (N = 1, 2): nl = 8, 256 B / 512 B.
// The NF fields share the nl lines, nl / NF complex = 2 nl / NF real lines each; in a batch of nc <= nl / NF complex lines per field those of a are
// lines 0 ... nc-1 and those of b lines nc ... 2 nc - 1, so that one spec_transform of NF nc lines serves both. At the cap in double NF = 2 has one
// complex line per field: a batch is two rows of each.
// Sums over lines are formed in a fixed order and without atomics: a thread owns its modes, adds the lines of its block in line order and writes ONE
// partial per block; k_spec_fold adds the blocks of a plane in block order. The same bits from run to run.
#include "spectral_line.hpp"
#include "../../include/cales_cospectra.h"

// a conj(b)
__host__ __device__ inline real2 cmulc(real2 a, real2 b) { return make_real2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
__host__ __device__ inline real spec_plus(real a, real b) { return a + b; }
__host__ __device__ inline real2 spec_plus(real2 a, real2 b) { return cadd(a, b); }

// What NF decides beyond the share of the lines: the per-mode sums of a thread over the lines of its block (modes m = threadIdx.x + 256 u), the three
// slots of nh values of T a block's partial holds, and the product of the plane spectra. The fields of a kernel are a pack by value.
template <int NF> struct SpecFields { const real *p[NF]; };
template <int NF> struct SpecSums;
// power spectra: |F|^2 | Re sum F | Im sum F, in reals
template <> struct SpecSums<1> {
  typedef real T;
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
  __device__ inline void store(real *__restrict__ dst, int nh) const {
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) {
      const int m = threadIdx.x + 256 * u;
      if (m < nh) { dst[m] = pw[u]; dst[nh + m] = sr[u]; dst[2 * nh + m] = si[u]; }
    }
  }
  // |H|^2 of mode column c of `ncol` at point q
  static __device__ inline real product(const real2 *__restrict__ Z, int N, int ncol, int c, int q) { return cabs2(Z[c * N + q]); }
};
// cross-spectra: F^a conj(F^b) | sum F^a | sum F^b, complex
template <> struct SpecSums<2> {
  typedef real2 T;
  real2 cr[SPEC_MPT], sa[SPEC_MPT], sb[SPEC_MPT];
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
  __device__ inline void store(real2 *__restrict__ dst, int nh) const {
#pragma unroll
    for (int u = 0; u < SPEC_MPT; ++u) {
      const int m = threadIdx.x + 256 * u;
      if (m < nh) { dst[m] = cr[u]; dst[nh + m] = sa[u]; dst[2 * nh + m] = sb[u]; }
    }
  }
  // H^a conj(H^b) of mode column c at point q: the columns of b follow the `ncol` of a
  static __device__ inline real2 product(const real2 *__restrict__ Z, int N, int ncol, int c, int q) { return cmulc(Z[c * N + q], Z[(ncol + c) * N + q]); }
};

// real line `l` of field `fld` of a batch of nc complex lines per field: the part (l & 1) of point `at` of complex line fld nc + l / 2
__device__ inline real &spec_real_line(real2 *A, int N, int nc, int fld, int l, int at) { return ((real *)(A + (fld * nc + (l >> 1)) * N + at))[l & 1]; }
// an odd last real line rides alone: the imaginary part of the last complex line of every field is zero
template <int NF> __device__ inline void spec_zero_odd(real2 *A, int N, int nc) {
  for (int i = threadIdx.x; i < N; i += 256)
#pragma unroll
    for (int fld = NF; fld-- > 0;) A[((fld + 1) * nc - 1) * N + i].y = (real)0.;      // (b's line first: the other way round k_spec_x<2, ...> takes 2 to 4 more VGPRs)
}

// x lines. blockIdx.y: the plane (k = blockIdx.y + 1, or the entry of kplanes), blockIdx.x: a run of sg.rows consecutive rows of it (the last run may be
// shorter), taken 2 nl / NF rows at a time: rows r and r+1 of a batch of nr rows are real and imaginary part of complex line fld nc + r/2 of field fld,
// nc = ceil(nr / 2); every field is read at the same index in sg.chunks 16-byte chunks per row (read_rows16, readout.hpp).
// PLANES = false: the sums of SpecSums<NF> over the rows of the block in row order, one partial per block at part[(blockIdx.y nb + blockIdx.x) 3 nh]
// PLANES = true:  the rows' transforms F(0 ... n1/2) go to rows_out[((NF blockIdx.y + fld) n2 + j - 1) nh + m]
template <int NF, bool PLANES>
__global__ __launch_bounds__(256) void k_spec_x(Geom g, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const int32_t *__restrict__ kplanes, SpecFields<NF> f,
                                                typename SpecSums<NF>::T *__restrict__ part, real2 *__restrict__ rows_out) {
  extern __shared__ real2 spec_lds[];      // 2 nl N
  const int N = pl.n, nh = sg.nh, batch = 2 * sg.nl / NF;
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int k = kplanes ? kplanes[blockIdx.y] : (int)blockIdx.y + 1, j0 = blockIdx.x * sg.rows + 1, nrows = min(sg.rows, g.n2 - j0 + 1);
  SpecSums<NF> acc; acc.clear();
  for (int r0 = 0; r0 < nrows; r0 += batch) {
    const int nr = min(batch, nrows - r0), nc = (nr + 1) / 2;
    read_rows16<NF>(g, sg.chunks, j0 + r0, nr, k, f.p[0], f.p[NF - 1], [&](int r, int i, real xa, real xb = (real)0.) {
      spec_real_line(A, N, nc, 0, r, i - 1) = xa;
      if constexpr (NF == 2) spec_real_line(A, N, nc, 1, r, i - 1) = xb; });
    if (nr & 1) spec_zero_odd<NF>(A, N, nc);
    __syncthreads();
    const real2 *Z = spec_transform(pl, tw, NF * nc, A, B);
    if (PLANES) {
      for (int w = threadIdx.x; w < NF * nr * nh; w += 256) {
        const int fr = w / nh, m = w - fr * nh, fld = NF == 1 ? 0 : fr / nr, r = fr - fld * nr;
        real2 fa, fb; spec_pair(Z + (fld * nc + (r >> 1)) * N, N, m, &fa, &fb);
        const bool odd = r & 1;      // (by component: a select between the two real2, filled through pointers, keeps both in scratch)
        rows_out[((size_t)(NF * blockIdx.y + fld) * g.n2 + (size_t)(j0 - 1 + r0 + r)) * nh + m] = make_real2(odd ? fb.x : fa.x, odd ? fb.y : fa.y);
      }
    } else acc.add(Z, N, nh, nr);
    __syncthreads();      // the next batch overwrites both buffers
  }
  if (!PLANES) acc.store(part + ((size_t)blockIdx.y * sg.nb + blockIdx.x) * 3 * (size_t)nh, nh);
}

// y lines of plane k = blockIdx.y + 1. blockIdx.x: a tile of 2 nl / NF adjacent columns from i0 = 1 + tile blockIdx.x (the last tile may hold fewer), read
// from every field; columns c and c+1 of the tile are real and imaginary part of complex line fld nc + c/2. Every row of the tile is sg.chunks 16-byte
// chunks per field (with nl = 8 in double and one field one whole 128-B segment); a chunk that starts past n1 is not read, one that reaches past n1 is
// masked as read_rows16 masks it; a tile narrower than a chunk (sg.chunks = 0: two fields, nl = 2 in single precision) is read element by element. The
// sums over the columns of the tile in column order, one partial per tile at part[(blockIdx.y nb + blockIdx.x) 3 nh]
template <int NF>
__global__ __launch_bounds__(256) void k_spec_y(Geom g, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, SpecFields<NF> f, typename SpecSums<NF>::T *__restrict__ part) {
  extern __shared__ real2 spec_lds[];
  const int N = pl.n, nh = sg.nh, tile = 2 * sg.nl / NF;      // N = n2
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int k = blockIdx.y + 1, i0 = 1 + tile * blockIdx.x, ncols = min(tile, g.n1 - i0 + 1), nc = (ncols + 1) / 2;
  if (NF == 1 || sg.chunks > 0) {
    for (int q = threadIdx.x; q < N * sg.chunks; q += 256) {
      const int j = q / sg.chunks, col = REALV * (q - j * sg.chunks), i = i0 + col;
      if (i > g.n1) continue;
      const size_t at = g.ix(i, j + 1, k);
      real e[NF][REALV];
#pragma unroll
      for (int fld = 0; fld < NF; ++fld) realv_unpack(*(const realv *)(f.p[fld] + at), e[fld]);
#pragma unroll
      for (int t = 0; t < REALV; ++t) if (i + t <= g.n1) {
#pragma unroll
        for (int fld = 0; fld < NF; ++fld) spec_real_line(A, N, nc, fld, col + t, j) = e[fld][t];
      }
    }
  } else {
    for (int q = threadIdx.x; q < N * ncols; q += 256) {
      const int j = q / ncols, col = q - j * ncols;
      const size_t at = g.ix(i0 + col, j + 1, k);
#pragma unroll
      for (int fld = 0; fld < NF; ++fld) spec_real_line(A, N, nc, fld, col, j) = f.p[fld][at];
    }
  }
  if (ncols & 1) spec_zero_odd<NF>(A, N, nc);
  __syncthreads();
  const real2 *Z = spec_transform(pl, tw, NF * nc, A, B);
  SpecSums<NF> acc; acc.clear();
  acc.add(Z, N, nh, ncols);
  acc.store(part + ((size_t)blockIdx.y * sg.nb + blockIdx.x) * 3 * (size_t)nh, nh);
}

// the y pass of the plane spectra: blockIdx.y a plane of the chunk, blockIdx.x a tile of nl / NF adjacent columns m of the complex rows of every field
// (nhx = n1/2+1 per row, what k_spec_x<NF, true> wrote: the n2 rows of b follow those of a): the columns of a are lines 0 ... ncol-1, the same columns
// of b lines ncol ... 2 ncol - 1. Transforms every column along y (N = n2 points), forms SpecSums<NF>::product at (m, ky), adds ky and n2 - ky where the
// two differ and writes out(m, q, plane), q = 0 ... n2/2, power2 in reals or cross2 complex: no sum across blocks
template <int NF>
__global__ __launch_bounds__(256) void k_spec_y2(int nhx, SpecGeom sg, SpecPlan pl, const real2 *__restrict__ tw, const real2 *__restrict__ rows, typename SpecSums<NF>::T *__restrict__ out) {
  extern __shared__ real2 spec_lds[];
  const int N = pl.n, nhy = sg.nh, cols = sg.nl / NF;
  real2 *A = spec_lds, *B = spec_lds + sg.nl * N;
  const int m0 = cols * blockIdx.x, ncol = min(cols, nhx - m0);
  const real2 *src = rows + (size_t)NF * blockIdx.y * N * nhx + m0;
  for (int q = threadIdx.x; q < NF * N * ncol; q += 256) {
    const int fj = q / ncol, c = q - fj * ncol, fld = NF == 1 ? 0 : fj / N, j = fj - fld * N;
    A[(fld * ncol + c) * N + j] = src[(size_t)fj * nhx + c];
  }
  __syncthreads();
  const real2 *Z = spec_transform(pl, tw, NF * ncol, A, B);
  typename SpecSums<NF>::T *dst = out + (size_t)blockIdx.y * nhx * nhy + m0;
  for (int w = threadIdx.x; w < ncol * nhy; w += 256) {
    const int q = w / ncol, c = w - q * ncol, ky2 = q ? N - q : 0;
    typename SpecSums<NF>::T v = SpecSums<NF>::product(Z, N, ncol, c, q);
    if (ky2 != q) v = spec_plus(v, SpecSums<NF>::product(Z, N, ncol, c, ky2));
    dst[(size_t)q * nhx + c] = v;
  }
}

// the three slots of the partials of the nb blocks of every plane, added in block order: power(nh, nplanes) and lsum(2, nh, nplanes) in reals, or cross,
// lsum_a and lsum_b, each (2, nh, nplanes)
__device__ inline void spec_fold_store(int t, real pw, real sr, real si, real *power, real *lsum) { power[t] = pw; lsum[2 * (size_t)t] = sr; lsum[2 * (size_t)t + 1] = si; }
__device__ inline void spec_fold_store(int t, real2 cr, real2 sa, real2 sb, real2 *cross, real2 *lsa, real2 *lsb) { cross[t] = cr; lsa[t] = sa; lsb[t] = sb; }
template <class T, class... L>
__global__ __launch_bounds__(256) void k_spec_fold(int nh, int nb, int nplanes, const T *__restrict__ part, T *__restrict__ out, L *__restrict__... ls) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nh * nplanes) return;
  const int k = t / nh, m = t - k * nh;
  const T *p = part + (size_t)k * nb * 3 * nh + m;
  T s0 = T(), s1 = T(), s2 = T();
  for (int b = 0; b < nb; ++b, p += 3 * nh) { s0 = spec_plus(s0, p[0]); s1 = spec_plus(s1, p[nh]); s2 = spec_plus(s2, p[2 * nh]); }
  spec_fold_store(t, s0, s1, s2, out, ls...);
}

// ------------------------------------------------------------------------------------------ host side (plan, LDS sizing, geometry: spectral_line.hpp)
// The entries of one NF differ from those of the other in their names and in the outputs: out[0] power (nh, n3) in reals or cross (2, nh, n3), then the
// optional line sums of the NF fields, (2, nh, n3) each.
template <int NF> struct SpecNames;      // (the profile scopes: [1] of a call that takes the direct sum)
template <> struct SpecNames<1> { static constexpr const char *lines = "cales_spectra_lines", *planes = "cales_spectra_planes", *out = "power",
  *scope_lines[2] = {"spectra_lines", "spectra_lines_direct"}, *scope_planes[2] = {"spectra_planes", "spectra_planes_direct"}; };
template <> struct SpecNames<2> { static constexpr const char *lines = "cales_cospectra_lines", *planes = "cales_cospectra_planes", *out = "cross",
  *scope_lines[2] = {"cospectra_lines", "cospectra_lines_direct"}, *scope_planes[2] = {"cospectra_planes", "cospectra_planes_direct"}; };
// the field ids of a call, before anything else is looked at (nothing is materialised yet) ...
template <int NF> static int spec_fields_ok(cales_ctx *c, const int (&field)[NF], const char *who) {
  for (int id : field) if (!field_ptr(c, id, who, FIELD_ROWS16)) return 0;
  return 1;
}
// ... and after everything else: the fields to read
template <int NF> static int spec_fields_read(cales_ctx *c, const int (&field)[NF], const char *who, SpecFields<NF> *f) {
  int bad = 0;
  for (int fld = 0; fld < NF; ++fld) bad |= !(f->p[fld] = field_ptr(c, field[fld], who, FIELD_READ));
  return bad;
}

template <int NF> static int spec_lines(cales_ctx *c, const int (&field)[NF], int idir, real *const (&out)[NF + 1]) {
  typedef typename SpecSums<NF>::T T;
  const char *who = SpecNames<NF>::lines;
  if (!spec_fields_ok(c, field, who)) return 1;
  if (idir != 1 && idir != 2) { c->err = std::string(who) + ": idir must be 1 or 2"; return 1; }
  if (idir == 2 && c->P > 1) { c->err = std::string(who) + ": idir = 2 on one rank only (a slab holds no whole y line)"; return 1; }
  const int n1 = c->n[0], n2 = c->n[1], n3 = c->n[2], N = idir == 1 ? n1 : n2;
  if (spec_line_ok(c, N, who)) return 1;
  if (!out[0]) { c->err = std::string(who) + ": " + SpecNames<NF>::out + " is NULL"; return 1; }
  SpecFields<NF> f; if (spec_fields_read(c, field, who, &f)) return 1;
  const SpecPlan pl = spec_plan(N);
  const SpecGeom sg = idir == 1 ? spec_geom_x(n1, n2, n3, NF, sizeof(real)) : spec_geom_y(n1, n2, NF, sizeof(real));
  const int nh = sg.nh;
  const size_t lds = spec_lds_bytes(sg.nl, N);
  if (idir == 1 ? spec_lds_attr(c, k_spec_x<NF, false>, lds) : spec_lds_attr(c, k_spec_y<NF>, lds)) return 1;
  const size_t n_out = (size_t)nh * n3;      // values of each result: T of out[0], complex of the line sums
  TempCarver tc; const auto p_tw = tc.part<real2>(N); const auto p_part = tc.part<T>((size_t)n3 * sg.nb * 3 * nh), p_out = tc.part<T>(n_out);
  TempPart<real2> p_ls[NF]; for (auto &p : p_ls) p = tc.part<real2>(n_out);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  real2 *d_tw = p_tw.in(tmp.p), *d_ls[NF]; T *d_part = p_part.in(tmp.p), *d_out = p_out.in(tmp.p);
  for (int fld = 0; fld < NF; ++fld) d_ls[fld] = p_ls[fld].in(tmp.p);
  { ProfScope ps(c, SpecNames<NF>::scope_lines[pl.direct]);
    LAUNCH(c, k_spec_twiddle, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, d_tw);
    const dim3 grid(sg.nb, n3), block(256);
    if (idir == 1) LAUNCH(c, (k_spec_x<NF, false>), grid, block, lds, c->stream, c->g, sg, pl, d_tw, (const int32_t *)nullptr, f, d_part, (real2 *)nullptr);
    else LAUNCH(c, k_spec_y<NF>, grid, block, lds, c->stream, c->g, sg, pl, d_tw, f, d_part);
    const dim3 fold((nh * n3 + 255) / 256);
    if constexpr (NF == 1) LAUNCH(c, (k_spec_fold<real, real>), fold, block, 0, c->stream, nh, sg.nb, n3, d_part, d_out, (real *)d_ls[0]);
    else LAUNCH(c, (k_spec_fold<real2, real2, real2>), fold, block, 0, c->stream, nh, sg.nb, n3, d_part, d_out, d_ls[0], d_ls[1]); }
  LAUNCHCHK(c);
  if (int e = read_back_queued(c, out[0], (real *)d_out, NF * n_out)) return e;
  for (int fld = 0; fld < NF; ++fld) if (out[1 + fld]) if (int e = read_back_queued(c, out[1 + fld], (real *)d_ls[fld], 2 * n_out)) return e;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

template <int NF> static int spec_planes(cales_ctx *c, const int (&field)[NF], int nplanes, const int32_t *kplanes, real *out2) {
  typedef typename SpecSums<NF>::T T;
  const char *who = SpecNames<NF>::planes;
  if (!spec_fields_ok(c, field, who)) return 1;
  if (c->P > 1) { c->err = std::string(who) + ": one rank only (a slab holds no whole y line)"; return 1; }
  const int n1 = c->n[0], n2 = c->n[1];
  if (spec_line_ok(c, n1, who) || spec_line_ok(c, n2, who)) return 1;
  if (!out2) { c->err = std::string(who) + ": " + SpecNames<NF>::out + "2 is NULL"; return 1; }
  if (plane_list_check(who, nplanes, kplanes, c->C.ng[2], c->err)) return 1;
  SpecFields<NF> f; if (spec_fields_read(c, field, who, &f)) return 1;
  const SpecPlan plx = spec_plan(n1), ply = spec_plan(n2);
  const int nhx = n1 / 2 + 1, nhy = n2 / 2 + 1;
  // the complex rows of a plane of NF fields take about as much as NF planes of a field: as many planes at a time as 32 MB of scratch hold, one at least
  const size_t plane_rows = NF * (size_t)nhx * n2, plane_out = (size_t)nhx * nhy;
  const int chunk = (int)std::min<size_t>((size_t)nplanes, std::max<size_t>(1, ((size_t)32 << 20) / (plane_rows * sizeof(real2))));
  const SpecGeom sx = spec_geom_x(n1, n2, chunk, NF, sizeof(real)), sy = spec_geom_y2(n1, n2, NF, sizeof(real));
  const size_t ldsx = spec_lds_bytes(sx.nl, n1), ldsy = spec_lds_bytes(sy.nl, n2);
  if (spec_lds_attr(c, k_spec_x<NF, true>, ldsx) || spec_lds_attr(c, k_spec_y2<NF>, ldsy)) return 1;
  // twiddles of x | of y | the complex rows of a chunk, every field | its power2 or cross2 | the planes
  TempCarver tc; const auto p_twx = tc.part<real2>(n1), p_twy = tc.part<real2>(n2), p_rows = tc.part<real2>(plane_rows * chunk);
  const auto p_out = tc.part<T>(plane_out * chunk); const auto p_k = tc.part<int32_t>(nplanes);
  CtxTemp tmp(c, tc.reals(sizeof(real))); if (!tmp.p) return 1;
  real2 *d_twx = p_twx.in(tmp.p), *d_twy = p_twy.in(tmp.p), *d_rows = p_rows.in(tmp.p);
  T *d_out = p_out.in(tmp.p); int32_t *d_k = p_k.in(tmp.p);
  if (int e = plane_list_upload(c, d_k, kplanes, nplanes)) return e;
  { ProfScope ps(c, SpecNames<NF>::scope_planes[plx.direct || ply.direct]);
    const dim3 block(256);
    LAUNCH(c, k_spec_twiddle, dim3((n1 + 255) / 256), block, 0, c->stream, n1, d_twx);
    LAUNCH(c, k_spec_twiddle, dim3((n2 + 255) / 256), block, 0, c->stream, n2, d_twy);
    for (int p0 = 0; p0 < nplanes; p0 += chunk) {
      const int np = std::min(chunk, nplanes - p0);
      LAUNCH(c, (k_spec_x<NF, true>), dim3(sx.nb, np), block, ldsx, c->stream, c->g, sx, plx, d_twx, (const int32_t *)(d_k + p0), f, (T *)nullptr, d_rows);
      LAUNCH(c, k_spec_y2<NF>, dim3(sy.nb, np), block, ldsy, c->stream, nhx, sy, ply, d_twy, d_rows, d_out);
      if (int e = read_back_queued(c, out2 + NF * plane_out * p0, (real *)d_out, NF * plane_out * np)) return e;
    } }
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int op_spectra_lines(cales_ctx *c, int field, int idir, real *power, real *lsum) { return spec_lines<1>(c, {field}, idir, {power, lsum}); }
int op_spectra_planes(cales_ctx *c, int field, int nplanes, const int32_t *kplanes, real *power2) { return spec_planes<1>(c, {field}, nplanes, kplanes, power2); }
int op_cospectra_lines(cales_ctx *c, int field_a, int field_b, int idir, real *cross, real *lsum_a, real *lsum_b) { return spec_lines<2>(c, {field_a, field_b}, idir, {cross, lsum_a, lsum_b}); }
int op_cospectra_planes(cales_ctx *c, int field_a, int field_b, int nplanes, const int32_t *kplanes, real *cross2) { return spec_planes<2>(c, {field_a, field_b}, nplanes, kplanes, cross2); }
