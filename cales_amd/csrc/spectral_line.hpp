// The line transform of the spectra and cross-spectra (k_spectra.hip): the launch geometry of its kernels, the plan of a line, the Stockham stages that take
// it back and forth between two LDS buffers, the compensated plain sum for a length with another prime factor, the Hermitian split of two real lines that
// rode in one complex transform, the twiddle table, and the host's sizing of LDS. k_spectra.hip's head says how the pieces go together.
#pragma once
#include "readout.hpp"
#include "../../include/cales_spectra.h"

// ------------------------------------------------------------------------------------------ launch geometry: plain integers, no HIP type -- a plain host
// compiler includes this part (tests/readout_host.cpp). nf = 1 (power spectra) or 2 (cross-spectra) fields share the nl complex lines of a block;
// real_size = sizeof(real)
constexpr size_t SPEC_LDS_SOFT = 64 * 1024, SPEC_LDS_MAX = 128 * 1024;
// rows: rows of a plane per block (x) | chunks: 16-byte chunks per row (x) or per tile row (y) | nl: complex lines in LDS | nh: n/2+1 | nb: blocks per plane
struct SpecGeom { int rows, chunks, nl, nh, nb; };
// complex lines of N points a block keeps in LDS (see the head of k_spectra.hip)
inline int spec_nl(int N, size_t real_size) {
  int nl = 8;
  while (nl > 2 && 2 * (size_t)nl * N * 2 * real_size > SPEC_LDS_SOFT) nl /= 2;
  return nl;
}
// k_spec_x: runs of rows per block (row_runs, readout.hpp) in whole batches of 2 nl / nf rows -- nl / nf complex lines of every field
inline SpecGeom spec_geom_x(int n1, int n2, int nplanes, int nf, size_t real_size) {
  const int nl = spec_nl(n1, real_size), realv = 16 / (int)real_size;
  const RowRuns rr = row_runs(n2, nplanes, 1, 2 * nl / nf);
  return SpecGeom{rr.rows, (n1 + realv - 1) / realv, nl, n1 / 2 + 1, rr.per_plane};
}
// k_spec_y: tiles of 2 nl / nf adjacent columns; a tile narrower than a chunk (nf = 2, nl = 2 in single precision) has none and is read by element
inline SpecGeom spec_geom_y(int n1, int n2, int nf, size_t real_size) {
  const int nl = spec_nl(n2, real_size), tile = 2 * nl / nf;
  return SpecGeom{0, tile / (16 / (int)real_size), nl, n2 / 2 + 1, (n1 + tile - 1) / tile};
}
// k_spec_y2: nl / nf of the n1/2+1 mode columns per block
inline SpecGeom spec_geom_y2(int n1, int n2, int nf, size_t real_size) {
  const int nl = spec_nl(n2, real_size), cols = nl / nf;
  return SpecGeom{0, 0, nl, n2 / 2 + 1, (n1 / 2 + 1 + cols - 1) / cols};
}

#ifdef __HIPCC__
constexpr int SPEC_MAX_STAGES = 12;                                     // 2048 = 4^5 2: 6 stages; 2 3^6 = 1458: 7
constexpr int SPEC_MPT = (CALES_SPECTRA_MAX_LINE / 2 + 1 + 255) / 256;  // modes a thread of a block of 256 owns at the cap: 5

// n = radix(0) ... radix(nst-1), or direct. The radices are packed four bits each: a kernel argument indexed by the stage would be copied to scratch
struct SpecPlan {
  int n, nst, direct; unsigned long long radices;
  __host__ __device__ inline int radix(int st) const { return (int)((radices >> (4 * st)) & 15ull); }
};

__host__ __device__ inline real2 cadd(real2 a, real2 b) { return make_real2(a.x + b.x, a.y + b.y); }
__host__ __device__ inline real2 csub(real2 a, real2 b) { return make_real2(a.x - b.x, a.y - b.y); }
__host__ __device__ inline real2 cmul(real2 a, real2 b) { return make_real2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline real cabs2(real2 a) { return a.x * a.x + a.y * a.y; }

// One butterfly of a Stockham stage of radix R on one line: x -> y, N points, s = the product of the radices of the stages before, M = N / R butterflies
// numbered item = q + s p (q < s, p < N / (R s)). With n' = N / s the length of the sub-transforms of this stage:
//   y[q + s (R p + u)] = w^(p u) sum_t x[q + s (p + t n'/R)] W_R^(t u),   w = exp(-2 pi I / n') = tw[s],   u = 0 ... R-1
// and s (p + t n'/R) + q = item + t M. The last stage leaves the transform in natural order.
template <int R>
__host__ __device__ inline void spec_bfly(const real2 *__restrict__ x, real2 *__restrict__ y, const real2 *__restrict__ tw, int N, int s, int item) {
  const int M = N / R, p = item / s, q = item - p * s;
  real2 a[R], b[R];
#pragma unroll
  for (int t = 0; t < R; ++t) a[t] = x[item + t * M];
  if constexpr (R == 2) { b[0] = cadd(a[0], a[1]); b[1] = csub(a[0], a[1]); }
  else if constexpr (R == 4) {
    const real2 e0 = cadd(a[0], a[2]), e1 = csub(a[0], a[2]), o0 = cadd(a[1], a[3]), o1 = csub(a[1], a[3]);
    b[0] = cadd(e0, o0); b[2] = csub(e0, o0);
    b[1] = make_real2(e1.x + o1.y, e1.y - o1.x);      // e1 - I o1
    b[3] = make_real2(e1.x - o1.y, e1.y + o1.x);      // e1 + I o1
  } else if constexpr (R == 3) {      // W_3 = -1/2 - I sin(2 pi / 3)
    const real s3 = (real)0.86602540378443864676;
    const real2 t1 = cadd(a[1], a[2]), t3 = csub(a[1], a[2]);
    const real2 m = make_real2(a[0].x - (real)0.5 * t1.x, a[0].y - (real)0.5 * t1.y), n = make_real2(s3 * t3.x, s3 * t3.y);
    b[0] = cadd(a[0], t1);
    b[1] = make_real2(m.x + n.y, m.y - n.x);      // m - I n
    b[2] = make_real2(m.x - n.y, m.y + n.x);      // m + I n
  } else {                  // R == 5: W_5^t = c_t - I s_t, c = cos, s = sin of 2 pi / 5 and 4 pi / 5
    const real c1 = (real)0.30901699437494742410, c2 = (real)-0.80901699437494742410, s1 = (real)0.95105651629515357212, s2 = (real)0.58778525229247312917;
    const real2 t1 = cadd(a[1], a[4]), t2 = cadd(a[2], a[3]), t3 = csub(a[1], a[4]), t4 = csub(a[2], a[3]);
    const real2 m1 = make_real2(a[0].x + c1 * t1.x + c2 * t2.x, a[0].y + c1 * t1.y + c2 * t2.y), m2 = make_real2(a[0].x + c2 * t1.x + c1 * t2.x, a[0].y + c2 * t1.y + c1 * t2.y);
    const real2 n1 = make_real2(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y), n2 = make_real2(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y);
    b[0] = cadd(a[0], cadd(t1, t2));
    b[1] = make_real2(m1.x + n1.y, m1.y - n1.x); b[4] = make_real2(m1.x - n1.y, m1.y + n1.x);      // m1 -/+ I n1
    b[2] = make_real2(m2.x + n2.y, m2.y - n2.x); b[3] = make_real2(m2.x - n2.y, m2.y + n2.x);      // m2 -/+ I n2
  }
  real2 *out = y + q + s * R * p;
  out[0] = b[0];
#pragma unroll
  for (int u = 1; u < R; ++u) out[s * u] = cmul(b[u], tw[p * u * s]);      // p u s < N
}
// stage `st` of the plan on `nl` lines of N points, x -> y: the work of thread tid of nthr
__host__ __device__ inline void spec_stage(const SpecPlan &pl, int st, int s, const real2 *__restrict__ tw, int nl, const real2 *__restrict__ x, real2 *__restrict__ y, int tid, int nthr) {
  const int N = pl.n, r = pl.radix(st), M = N / r;
  for (int w = tid; w < nl * M; w += nthr) {
    const int line = w / M, item = w - line * M;
    const real2 *xi = x + line * N; real2 *yo = y + line * N;
    if (r == 4) spec_bfly<4>(xi, yo, tw, N, s, item);
    else if (r == 2) spec_bfly<2>(xi, yo, tw, N, s, item);
    else if (r == 3) spec_bfly<3>(xi, yo, tw, N, s, item);
    else spec_bfly<5>(xi, yo, tw, N, s, item);
  }
}
// the plain sum, one output point per item: y[m] = sum_i x[i] tw[i m mod N], added in the order of i. The sum is compensated (Kahan): the rounding error
// of a plain running sum grows with N -- on a constant line of 2046 points it was measured at 200 eps |F|, past what a staged transform of that
// length is held to (16 log2 N eps) -- and the compensated one does not
__host__ __device__ inline void spec_direct(int N, const real2 *__restrict__ tw, int nl, const real2 *__restrict__ x, real2 *__restrict__ y, int tid, int nthr) {
  for (int w = tid; w < nl * N; w += nthr) {
    const int line = w / N, m = w - line * N;
    const real2 *xi = x + line * N;
    real2 acc = make_real2((real)0., (real)0.), lost = acc;
    for (int i = 0, e = 0; i < N; ++i) {
      const real2 term = csub(cmul(xi[i], tw[e]), lost), t = cadd(acc, term);
      lost = csub(csub(t, acc), term); acc = t;
      e += m; if (e >= N) e -= N;
    }
    y[w] = acc;
  }
}
// Z = DFT(a + I b) of two real lines a, b: F_a(m) and F_b(m), m = 0 ... N/2, from Z(m) and Z(N - m)
__host__ __device__ inline void spec_pair(const real2 *__restrict__ Z, int N, int m, real2 *fa, real2 *fb) {
  const real2 zm = Z[m], zn = Z[m ? N - m : 0];
  *fa = make_real2((real)0.5 * (zm.x + zn.x), (real)0.5 * (zm.y - zn.y));
  *fb = make_real2((real)0.5 * (zm.y + zn.y), (real)0.5 * (zn.x - zm.x));
}
// The block transforms the `nl` lines it has put into A (every thread past the barrier that ends the loading); returns the buffer that holds the
// result, behind a barrier
__device__ inline real2 *spec_transform(const SpecPlan &pl, const real2 *__restrict__ tw, int nl, real2 *A, real2 *B) {
  if (pl.direct) { spec_direct(pl.n, tw, nl, A, B, threadIdx.x, 256); __syncthreads(); return B; }
  int s = 1;
  for (int st = 0; st < pl.nst; ++st) {
    spec_stage(pl, st, s, tw, nl, A, B, threadIdx.x, 256);
    __syncthreads();
    real2 *t = A; A = B; B = t;
    s *= pl.radix(st);
  }
  return A;
}

// (inline: the kernel is part of every unit that includes this header, and the units' copies are one at link time -- as those of a template are)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
inline __global__ __launch_bounds__(256) void k_spec_twiddle(int N, real2 *__restrict__ tw) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  const double a = 2. * (double)t / (double)N;
  tw[t] = make_real2((real)cospi(a), (real)(-sinpi(a)));
}
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------ host side
// N as factors 4 (first), 2, 3, 5; anything else: the direct sum
static SpecPlan spec_plan(int n) {
  SpecPlan pl; pl.n = n; pl.nst = 0; pl.direct = 0; pl.radices = 0ull;
  int m = n;
  const int rs[4] = {4, 2, 3, 5};
  for (int r : rs) while (m % r == 0 && pl.nst < SPEC_MAX_STAGES) { pl.radices |= (unsigned long long)r << (4 * pl.nst++); m /= r; }
  if (m != 1) { pl.nst = 0; pl.direct = 1; pl.radices = 0ull; }
  return pl;
}
static size_t spec_lds_bytes(int nl, int N) { return 2 * (size_t)nl * N * sizeof(real2); }
// a kernel that asks for more than 64 KB of dynamic LDS has to say so once
template <class K> static int spec_lds_attr(cales_ctx *c, K kernel, size_t lds) {
  if (lds > SPEC_LDS_MAX) { c->err = "spectra: the line does not fit the LDS budget"; return 1; }
  if (lds > SPEC_LDS_SOFT) HIPCHK(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPEC_LDS_MAX));
  return 0;
}
static int spec_line_ok(cales_ctx *c, int n, const char *who) {
  if (n > CALES_SPECTRA_MAX_LINE) { c->err = std::string(who) + ": a line of " + std::to_string(n) + " points is longer than CALES_SPECTRA_MAX_LINE = " + std::to_string(CALES_SPECTRA_MAX_LINE); return 1; }
  return 0;
}
#endif
