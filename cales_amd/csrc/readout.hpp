// What the field read-outs share (api.hip: box reads; k_pdf.hip: histograms; k_spectra.hip: spectra and cross-spectra): the host side of a call -- its temporary, the plane
// list, the rows a block takes -- and, for the kernels, the 16-byte reader of a run of rows. The host part uses no HIP type: a plain host compiler
// includes it (tests/readout_host.cpp), as it does lmf_pack.hpp. The field id of a call goes through field_ptr (common.hpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#ifdef __HIPCC__
#include "common.hpp"
#endif

// ---- the temporary of a call: parts of n elements of T, declared in order, every part on a 16-byte boundary of an allocation that starts on one (CtxTemp).
// part() before the allocation, reals() its size for CtxTemp, TempPart::in() the part inside it
template <class T> struct TempPart {
  size_t at;      // bytes from the start
  T *in(void *base) const { return (T *)((char *)base + at); }
};
struct TempCarver {
  size_t bytes = 0;      // a multiple of 16
  template <class T> TempPart<T> part(size_t n) { const TempPart<T> p{bytes}; bytes += (n * sizeof(T) + 15) & ~(size_t)15; return p; }
  size_t reals(size_t real_size) const { return bytes / real_size; }      // (4 or 8 divides 16)
};

// ---- the plane list of cales_jpdf_planes / cales_spectra_planes: global k, 1 ... ng(3), any order, repeats allowed. 0: fine; 1 and err otherwise
inline int plane_list_check(const char *who, int nplanes, const int32_t *kplanes, int ng3, std::string &err) {
  const char *what = nullptr;
  if (nplanes < 1) what = ": nplanes < 1";
  else if (!kplanes) what = ": kplanes is NULL";
  else for (int p = 0; p < nplanes && !what; ++p) if (kplanes[p] < 1 || kplanes[p] > ng3) what = ": plane outside 1 ... ng(3)";
  if (what) err = std::string(who) + what;
  return what ? 1 : 0;
}

// ---- rows per block of a kernel whose blocks take runs of rows of a plane (blockIdx.y the plane, blockIdx.x the run): enough blocks to fill the device,
// about 2048 over the planes, but no run shorter than least_rows (or than the plane), then whole multiples of `multiple` rows
struct RowRuns { int rows, per_plane; };      // rows of a run (the last of a plane may be shorter) | runs = blocks of a plane
inline RowRuns row_runs(int n2, int nplanes, int least_rows, int multiple) {
  const int want = (2048 + nplanes - 1) / nplanes;
  int rows = std::min(std::max((n2 + want - 1) / want, least_rows), n2);
  rows = (rows + multiple - 1) / multiple * multiple;
  return RowRuns{rows, (n2 + rows - 1) / rows};
}

#ifdef __HIPCC__
// ---- host side with the context
inline int plane_list_upload(cales_ctx *c, int32_t *d_k, const int32_t *kplanes, int nplanes) {
  HIPCHK(c, hipMemcpyAsync(d_k, kplanes, (size_t)nplanes * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// ---- device side: 16 bytes per lane
#ifdef CALES_SINGLE
typedef float4 realv;
#else
typedef double2 realv;
#endif
constexpr int REALV = 16 / RSZ;      // elements of a realv
__device__ inline void realv_unpack(const realv &v, real (&e)[REALV]) {
  e[0] = v.x; e[1] = v.y;
#ifdef CALES_SINGLE
  e[2] = v.z; e[3] = v.w;
#endif
}
// The block reads rows j0 ... j0 + nrows - 1 of plane k of one field (NF = 1) or of two at the same index (NF = 2): thread q of 256 takes chunk q of
// nrows x chunks, chunks = ceil(n1 / REALV) chunks of REALV elements per row from element 1, which sits on a 128-B boundary in every row (Geom), and hands
// every sample to body(r, i, x) / body(r, i, xa, xb): r the row of the run, i = 1 ... n1 the column. The last chunk of a row may reach past n1 into the
// pitch padding or the next row's first element -- inside the field's allocation (the host has checked the 16-byte alignment: FIELD_ROWS16), and masked out here.
template <int NF, class Body>
__device__ __forceinline__ void read_rows16(const Geom &g, int chunks, int j0, int nrows, int k, const real *__restrict__ fa, const real *__restrict__ fb, Body body) {
  const int nq = nrows * chunks;
  for (int q = threadIdx.x; q < nq; q += 256) {
    const int r = q / chunks, i = 1 + REALV * (q - r * chunks);
    const size_t c = g.ix(i, j0 + r, k);
    real a[REALV], b[REALV];
    realv_unpack(*(const realv *)(fa + c), a);
    if constexpr (NF == 2) realv_unpack(*(const realv *)(fb + c), b);
#pragma unroll
    for (int t = 0; t < REALV; ++t) if (t == 0 || i + t <= g.n1) {
      if constexpr (NF == 2) body(r, i + t, a[t], b[t]); else body(r, i + t, a[t]);
    }
  }
}
#endif
