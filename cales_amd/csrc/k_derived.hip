// Derived fields of the stored velocity (include/cales_derived.h): vorticity, SijSij, WijWij and Q of the reference's src/post.f90, formed on the device for
// the cells a caller asks for. The arithmetic is derived_math.hpp's, one function per quantity with contraction off: what a kernel here adds is where the
// samples come from and where the result goes, so every form gives the bits the host restatement gives (tests/test_derived_host.py). Two forms: one thread per
// point of any strided box, the neighbours through the caches (k_derived_points), and for dense boxes of whole rows tiles that march along z with the
// planes of the stencil in LDS (k_derived_rows); CALES_DERIVED_POINTS=1 sends every box to the first.
#include "readout.hpp"
#include "derived_math.hpp"
#include "../../include/cales_derived.h"

static_assert(CALES_NDERIVED == DQ_N && CALES_DERIVED_VOX == DQ_VOX && CALES_DERIVED_VOY == DQ_VOY && CALES_DERIVED_VOZ == DQ_VOZ && CALES_DERIVED_STR == DQ_STR &&
              CALES_DERIVED_ENS == DQ_ENS && CALES_DERIVED_QCR == DQ_QCR && CALES_DERIVED_VOX_EDGE == DQ_VOX_EDGE && CALES_DERIVED_VOY_EDGE == DQ_VOY_EDGE &&
              CALES_DERIVED_VOZ_EDGE == DQ_VOZ_EDGE, "derived_math.hpp numbers the quantities as enum cales_derived does");

// The points of a strided box, first + m * skip in LOCAL haloed indices, all of them interior cells (the entry has checked the box: api.hip)
struct DerivedBox { int first[3], skip[3], count[3]; };
// dli(1), dli(2) and the tables dzci, dzfi (0:n3+1) of the context
struct DerivedGrid { real dxi, dyi; const real *dzci, *dzfi; };
// the accessor of derived_math.hpp straight on the fields: cell c = g.ix(i, j, k), the neighbours through the caches
struct GlobalCell {
  const real *__restrict__ pu, *__restrict__ pv, *__restrict__ pw; size_t c; long s1, s12;
  __device__ __forceinline__ size_t at(int di, int dj, int dk) const { return (size_t)((long)c + di + dj * s1 + dk * s12); }
  __device__ __forceinline__ real u(int di, int dj, int dk) const { return pu[at(di, dj, dk)]; }
  __device__ __forceinline__ real v(int di, int dj, int dk) const { return pv[at(di, dj, dk)]; }
  __device__ __forceinline__ real w(int di, int dj, int dk) const { return pw[at(di, dj, dk)]; }
};
enum DerivedOut { TO_PACKED = 0, TO_FIELD = 1 };      // the packed box (the host's buffer) | the same cell of a field in the library's layout

// One thread per OUTPUT element of the box, numbered as the packed array is stored (the scheme of k_box_read, api.hip): the stores of a wave are contiguous
// whatever the box, its lanes run along the fastest direction of the output that has more than one point. Geom::ix gives size_t offsets: fields beyond 4 GB need
// nothing special. A cell reads up to 27 samples of the three components; with nskip(1) = 1 a wave reads row segments, and the rows j+-1 and the planes k+-1
// of its neighbours in the grid are the same lines moments later -- L2 hits. Every box that is not dense takes this form.
template <int Q, int OUT>
__global__ __launch_bounds__(256) void k_derived_points(Geom g, DerivedBox b, size_t total, DerivedGrid gr, const real *__restrict__ u, const real *__restrict__ v,
                                                        const real *__restrict__ w, real *__restrict__ dst) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t r = t / (size_t)b.count[0];
  const int m0 = (int)(t - r * (size_t)b.count[0]), m2 = (int)(r / (size_t)b.count[1]), m1 = (int)(r - (size_t)m2 * (size_t)b.count[1]);
  const int i = b.first[0] + m0 * b.skip[0], j = b.first[1] + m1 * b.skip[1], k = b.first[2] + m2 * b.skip[2];
  const size_t c = g.ix(i, j, k);
  const DerivedMetrics<real> m{gr.dxi, gr.dyi, gr.dzci[k - 1], gr.dzci[k], gr.dzfi[k]};
  const real q = derived_eval<Q, real>(GlobalCell{u, v, w, c, (long)g.s1, g.s12}, m);
  dst[OUT == TO_PACKED ? t : c] = q;
}

// The dense form: whole rows of at least 64 cells, nskip = 1. A block of 256 threads owns a tile of DTX x DTY cells -- lanes along x, wave w the rows w and
// w + 4 -- and marches along z over a run of planes. The three planes k-1, k, k+1 of u, v, w the stencil needs sit in a ring of three slots in LDS, each the
// tile with its one-cell halo (DLX x DLY): every velocity sample is loaded from global memory once per tile (plus the halo, 660 / 512), the up to 40
// reads of a cell are LDS reads with the lanes on consecutive words. Ring: 3 slots x 3 fields x 10 x 66 reals = 47.5 KB in FP64 -- three blocks per CU of
// 160 KB. Per plane: the block loads plane k+1 into the slot plane k-2 left, barrier, computes plane k from the three slots, barrier. The cells call the
// functions of derived_math.hpp the points form calls, on the same values: the same bits.
constexpr int DTX = 64, DTY = 8, DLX = DTX + 2, DLY = DTY + 2, DFIELD = DLX * DLY, DSLOT = 3 * DFIELD;
// the box in LOCAL indices: rows j0 ... j0 + nj - 1 (all of x), planes k0 ... k0 + nk - 1; klen planes per block (blockIdx.z the run)
struct DerivedRows { int j0, nj, k0, nk, klen; };
// the accessor of derived_math.hpp on the ring: the thread's cell in the slots of the planes k-1, k, k+1 (u; v and w one and two DFIELD behind)
struct LdsCell {
  const real *km, *kc, *kp;
  __device__ __forceinline__ const real *plane(int dk) const { return dk < 0 ? km : dk > 0 ? kp : kc; }
  __device__ __forceinline__ real u(int di, int dj, int dk) const { return plane(dk)[di + dj * DLX]; }
  __device__ __forceinline__ real v(int di, int dj, int dk) const { return plane(dk)[DFIELD + di + dj * DLX]; }
  __device__ __forceinline__ real w(int di, int dj, int dk) const { return plane(dk)[2 * DFIELD + di + dj * DLX]; }
};
template <int Q, int OUT>
__global__ __launch_bounds__(256) void k_derived_rows(Geom g, DerivedRows b, DerivedGrid gr, const real *__restrict__ u, const real *__restrict__ v,
                                                      const real *__restrict__ w, real *__restrict__ dst) {
  __shared__ real ring[3 * DSLOT];
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int i0 = 1 + blockIdx.x * DTX, ilast = min(i0 + DTX - 1, g.n1);
  const int j0 = b.j0 + blockIdx.y * DTY, jlast = min(j0 + DTY - 1, b.j0 + b.nj - 1);
  const int ka = b.k0 + blockIdx.z * b.klen, kb = min(ka + b.klen - 1, b.k0 + b.nk - 1);
  // plane k of the tile and its halo into slot k mod 3: columns i0-1 ... ilast+1 <= n1+1, rows j0-1 ... jlast+1 <= n2+1, 0 <= k <= n3+1 -- inside the fields. What a
  // shorter tile leaves unwritten no cell of the box reads
  auto load_plane = [&](int k) {
    real *s = ring + (k % 3) * DSLOT;
    for (int e = threadIdx.x; e < DFIELD; e += 256) {
      const int r = e / DLX, col = e - r * DLX, i = i0 - 1 + col, j = j0 - 1 + r;
      if (i <= ilast + 1 && j <= jlast + 1) {
        const size_t o = g.ix(i, j, k);
        s[e] = u[o]; s[DFIELD + e] = v[o]; s[2 * DFIELD + e] = w[o];
      }
    }
  };
  load_plane(ka - 1); load_plane(ka);
  const int i = i0 + lx;
  for (int k = ka; k <= kb; ++k) {
    load_plane(k + 1);
    __syncthreads();
    const DerivedMetrics<real> m{gr.dxi, gr.dyi, ldc(gr.dzci, k - 1), ldc(gr.dzci, k), ldc(gr.dzfi, k)};
    const real *km = ring + ((k + 2) % 3) * DSLOT, *kc = ring + (k % 3) * DSLOT, *kp = ring + ((k + 1) % 3) * DSLOT;
#pragma unroll
    for (int rr = 0; rr < DTY / 4; ++rr) {
      const int r = ly + 4 * rr, j = j0 + r;
      if (i <= g.n1 && j <= jlast) {
        const int at = (r + 1) * DLX + lx + 1;
        const real q = derived_eval<Q, real>(LdsCell{km + at, kc + at, kp + at}, m);
        if (OUT == TO_PACKED) dst[(size_t)(i - 1) + (size_t)g.n1 * ((size_t)(j - b.j0) + (size_t)b.nj * (size_t)(k - b.k0))] = q;
        else dst[g.ix(i, j, k)] = q;
      }
    }
    __syncthreads();      // (the next plane's load overwrites the slot of plane k-1)
  }
}

// ------------------------------------------------------------------------------------------ host side
typedef void (*DerivedRowsKernel)(Geom, DerivedRows, DerivedGrid, const real *, const real *, const real *, real *);
#define DERIVED_Q(Q) {k_derived_rows<Q, TO_PACKED>, k_derived_rows<Q, TO_FIELD>}
static const DerivedRowsKernel derived_rows_tab[DQ_N][2] = {DERIVED_Q(0), DERIVED_Q(1), DERIVED_Q(2), DERIVED_Q(3), DERIVED_Q(4),
                                                            DERIVED_Q(5), DERIVED_Q(6), DERIVED_Q(7), DERIVED_Q(8)};
#undef DERIVED_Q
typedef void (*DerivedKernel)(Geom, DerivedBox, size_t, DerivedGrid, const real *, const real *, const real *, real *);
#define DERIVED_Q(Q) {k_derived_points<Q, TO_PACKED>, k_derived_points<Q, TO_FIELD>}
static const DerivedKernel derived_points_tab[DQ_N][2] = {DERIVED_Q(0), DERIVED_Q(1), DERIVED_Q(2), DERIVED_Q(3), DERIVED_Q(4),
                                                          DERIVED_Q(5), DERIVED_Q(6), DERIVED_Q(7), DERIVED_Q(8)};
#undef DERIVED_Q

// the launch of a call, under its profile scope: the box's points (local indices) into dst
static int derived_launch(cales_ctx *c, int quantity, DerivedOut out, const DerivedBox &b, real *dst) {
  const size_t total = (size_t)b.count[0] * (size_t)b.count[1] * (size_t)b.count[2];      // (never more than a field: the points of a box are distinct interior cells)
  const DerivedGrid gr{c->dli[0], c->dli[1], c->d_dzci, c->d_dzfi};
  const int n1 = c->n[0];
  const bool dense = b.skip[0] == 1 && b.skip[1] == 1 && b.skip[2] == 1 && b.first[0] == 1 && b.count[0] == n1 && n1 >= DTX;
  if (dense && !c->fl.derived_points) {
    // runs of planes: about 2048 blocks where the box has them, no run shorter than 8 planes (every run loads two planes more than it forms)
    const int xt = (n1 + DTX - 1) / DTX, yt = (b.count[1] + DTY - 1) / DTY, nk = b.count[2];
    const int want = std::max(1, 2048 / (xt * yt)), klen = std::min(nk, std::max((nk + want - 1) / want, 8));
    const DerivedRows rw{b.first[1], b.count[1], b.first[2], nk, klen};
    ProfScope ps(c, "derived_rows");
    LAUNCH_NAMED(c, derived_rows_tab[quantity][out], "k_derived_rows", dim3(xt, yt, (nk + klen - 1) / klen), dim3(256), 0, c->stream, c->g, rw, gr,
                 c->f[CALES_U], c->f[CALES_V], c->f[CALES_W], dst);
    return 0;
  }
  ProfScope ps(c, "derived_points");
  LAUNCH_NAMED(c, derived_points_tab[quantity][out], "k_derived_points", dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->g, b, total, gr,
               c->f[CALES_U], c->f[CALES_V], c->f[CALES_W], dst);
  return 0;
}

int op_derived_box(cales_ctx *c, int quantity, const int32_t *first, const int32_t *count, const int32_t *nskip, real *buf) {
  DerivedBox b;
  for (int d = 0; d < 3; ++d) { b.first[d] = first[d]; b.skip[d] = nskip[d]; b.count[d] = count[d]; }
  b.first[1] -= c->g.jlo;      // global row -> row of the slab
  const size_t total = (size_t)count[0] * (size_t)count[1] * (size_t)count[2];
  if (int e = derived_launch(c, quantity, TO_PACKED, b, c->scr1)) return e;      // scr1: scratch between operators
  LAUNCHCHK(c);
  return read_back(c, buf, c->scr1, total);
}

int op_derived_to_pp(cales_ctx *c, int quantity) {
  DerivedBox b;
  for (int d = 0; d < 3; ++d) { b.first[d] = 1; b.skip[d] = 1; b.count[d] = c->n[d]; }
  if (int e = derived_launch(c, quantity, TO_FIELD, b, c->f[CALES_PP])) return e;
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
