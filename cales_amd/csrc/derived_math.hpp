// The arithmetic of the derived fields (include/cales_derived.h), written once: vorticity, SijSij, WijWij and Q of the reference's src/post.f90, one function
// template per quantity, for one cell. Both kernel forms of k_derived.hip call these, and so does a plain host compiler (tests/derived_host.cpp): like
// readout.hpp the file holds no HIP type.
//
// Every function evaluates the expression of post.f90 in the order it is written there, as Fortran and C parse it -- left to right within one precedence
// level, x**2 as x * x --, with contraction off: each operation is one IEEE rounding, no fused multiply-add is formed (a host compiler other than clang gets
// -ffp-contract=off on its command line). A restatement in the same order in any IEEE arithmetic of the same precision gives the same bits
// (tests/test_derived_host.py: derived_ref).
//
// A: the accessor of the cell, a.u(di, dj, dk) / a.v(...) / a.w(...) = ux / uy / uz at (i + di, j + dj, k + dk), offsets -1, 0, 1. No function asks for an offset
// with three non-zero entries: an interior cell never reads a cell with three ghost indices.
#pragma once

#if defined(__HIPCC__)
#define DERIVED_HD __host__ __device__ inline
#else
#define DERIVED_HD inline
#endif
#if defined(__clang__)
#define DERIVED_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DERIVED_NO_CONTRACT
#endif

// enum cales_derived of include/cales_derived.h (the values are part of the ABI)
enum { DQ_VOX = 0, DQ_VOY = 1, DQ_VOZ = 2, DQ_STR = 3, DQ_ENS = 4, DQ_QCR = 5, DQ_VOX_EDGE = 6, DQ_VOY_EDGE = 7, DQ_VOZ_EDGE = 8, DQ_N = 9 };

// the metrics of a cell of plane k: dli(1), dli(2), dzci(k-1), dzci(k), dzfi(k)
template <class T> struct DerivedMetrics { T dxi, dyi, dzci_m, dzci, dzfi; };

// ---- vorticity at the cell centre (post.f90:14-56)
template <class T, class A> DERIVED_HD T derived_vox(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T dyi = m.dyi, dzc = m.dzci, dzm = m.dzci_m;
  return (T)0.25 * (
      (a.w(0, 1, 0) - a.w(0, 0, 0)) * dyi - (a.v(0, 0, 1) - a.v(0, 0, 0)) * dzc +
      (a.w(0, 1, -1) - a.w(0, 0, -1)) * dyi - (a.v(0, 0, 0) - a.v(0, 0, -1)) * dzm +
      (a.w(0, 0, 0) - a.w(0, -1, 0)) * dyi - (a.v(0, -1, 1) - a.v(0, -1, 0)) * dzc +
      (a.w(0, 0, -1) - a.w(0, -1, -1)) * dyi - (a.v(0, -1, 0) - a.v(0, -1, -1)) * dzm);
}
template <class T, class A> DERIVED_HD T derived_voy(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T dxi = m.dxi, dzc = m.dzci, dzm = m.dzci_m;
  return (T)0.25 * (
      (a.u(0, 0, 1) - a.u(0, 0, 0)) * dzc - (a.w(1, 0, 0) - a.w(0, 0, 0)) * dxi +
      (a.u(0, 0, 0) - a.u(0, 0, -1)) * dzm - (a.w(1, 0, -1) - a.w(0, 0, -1)) * dxi +
      (a.u(-1, 0, 1) - a.u(-1, 0, 0)) * dzc - (a.w(0, 0, 0) - a.w(-1, 0, 0)) * dxi +
      (a.u(-1, 0, 0) - a.u(-1, 0, -1)) * dzm - (a.w(0, 0, -1) - a.w(-1, 0, -1)) * dxi);
}
template <class T, class A> DERIVED_HD T derived_voz(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T dxi = m.dxi, dyi = m.dyi;
  return (T)0.25 * (
      (a.v(1, 0, 0) - a.v(0, 0, 0)) * dxi - (a.u(0, 1, 0) - a.u(0, 0, 0)) * dyi +
      (a.v(1, -1, 0) - a.v(0, -1, 0)) * dxi - (a.u(0, 0, 0) - a.u(0, -1, 0)) * dyi +
      (a.v(0, 0, 0) - a.v(-1, 0, 0)) * dxi - (a.u(-1, 1, 0) - a.u(-1, 0, 0)) * dyi +
      (a.v(0, -1, 0) - a.v(-1, -1, 0)) * dxi - (a.u(-1, 0, 0) - a.u(-1, -1, 0)) * dyi);
}

// ---- vorticity at the cell edge (vorticity_one_component, post.f90:104-151)
template <class T, class A> DERIVED_HD T derived_vox_edge(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  return (a.w(0, 1, 0) - a.w(0, 0, 0)) * m.dyi - (a.v(0, 0, 1) - a.v(0, 0, 0)) * m.dzci;
}
template <class T, class A> DERIVED_HD T derived_voy_edge(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  return (a.u(0, 0, 1) - a.u(0, 0, 0)) * m.dzci - (a.w(1, 0, 0) - a.w(0, 0, 0)) * m.dxi;
}
template <class T, class A> DERIVED_HD T derived_voz_edge(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  return (a.v(1, 0, 0) - a.v(0, 0, 0)) * m.dxi - (a.u(0, 1, 0) - a.u(0, 0, 0)) * m.dyi;
}

// ---- the off-diagonal sums shared by strain_rate (SGN = +1, post.f90:80-97) and rotation_rate (SGN = -1, :172-189): .25*(t1**2 + t2**2 + t3**2 + t4**2)*.25,
// t = a +- b with the sign of the quantity (x - y is x + (-y) to the bit)
template <int SGN, class T> DERIVED_HD T derived_pm(T x, T y) {
  DERIVED_NO_CONTRACT
  return SGN > 0 ? x + y : x - y;
}
template <class T> DERIVED_HD T derived_mean_sq(T t1, T t2, T t3, T t4) {
  DERIVED_NO_CONTRACT
  return (T)0.25 * (t1 * t1 + t2 * t2 + t3 * t3 + t4 * t4) * (T)0.25;
}
template <int SGN, class T, class A> DERIVED_HD T derived_x12(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T dxi = m.dxi, dyi = m.dyi;
  const T t1 = derived_pm<SGN>((a.u(0, 1, 0) - a.u(0, 0, 0)) * dyi, (a.v(1, 0, 0) - a.v(0, 0, 0)) * dxi);
  const T t2 = derived_pm<SGN>((a.u(0, 0, 0) - a.u(0, -1, 0)) * dyi, (a.v(1, -1, 0) - a.v(0, -1, 0)) * dxi);
  const T t3 = derived_pm<SGN>((a.u(-1, 1, 0) - a.u(-1, 0, 0)) * dyi, (a.v(0, 0, 0) - a.v(-1, 0, 0)) * dxi);
  const T t4 = derived_pm<SGN>((a.u(-1, 0, 0) - a.u(-1, -1, 0)) * dyi, (a.v(0, -1, 0) - a.v(-1, -1, 0)) * dxi);
  return derived_mean_sq(t1, t2, t3, t4);
}
template <int SGN, class T, class A> DERIVED_HD T derived_x13(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T dxi = m.dxi, dzc = m.dzci, dzm = m.dzci_m;
  const T t1 = derived_pm<SGN>((a.u(0, 0, 1) - a.u(0, 0, 0)) * dzc, (a.w(1, 0, 0) - a.w(0, 0, 0)) * dxi);
  const T t2 = derived_pm<SGN>((a.u(0, 0, 0) - a.u(0, 0, -1)) * dzm, (a.w(1, 0, -1) - a.w(0, 0, -1)) * dxi);
  const T t3 = derived_pm<SGN>((a.u(-1, 0, 1) - a.u(-1, 0, 0)) * dzc, (a.w(0, 0, 0) - a.w(-1, 0, 0)) * dxi);
  const T t4 = derived_pm<SGN>((a.u(-1, 0, 0) - a.u(-1, 0, -1)) * dzm, (a.w(0, 0, -1) - a.w(-1, 0, -1)) * dxi);
  return derived_mean_sq(t1, t2, t3, t4);
}
template <int SGN, class T, class A> DERIVED_HD T derived_x23(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T dyi = m.dyi, dzc = m.dzci, dzm = m.dzci_m;
  const T t1 = derived_pm<SGN>((a.v(0, 0, 1) - a.v(0, 0, 0)) * dzc, (a.w(0, 1, 0) - a.w(0, 0, 0)) * dyi);
  const T t2 = derived_pm<SGN>((a.v(0, 0, 0) - a.v(0, 0, -1)) * dzm, (a.w(0, 1, -1) - a.w(0, 0, -1)) * dyi);
  const T t3 = derived_pm<SGN>((a.v(0, -1, 1) - a.v(0, -1, 0)) * dzc, (a.w(0, 0, 0) - a.w(0, -1, 0)) * dyi);
  const T t4 = derived_pm<SGN>((a.v(0, -1, 0) - a.v(0, -1, -1)) * dzm, (a.w(0, 0, -1) - a.w(0, -1, -1)) * dyi);
  return derived_mean_sq(t1, t2, t3, t4);
}
// ---- SijSij (strain_rate, post.f90:58-102)
template <class T, class A> DERIVED_HD T derived_str(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T d11 = (a.u(0, 0, 0) - a.u(-1, 0, 0)) * m.dxi, d22 = (a.v(0, 0, 0) - a.v(0, -1, 0)) * m.dyi, d33 = (a.w(0, 0, 0) - a.w(0, 0, -1)) * m.dzfi;
  const T s11 = d11 * d11, s22 = d22 * d22, s33 = d33 * d33;
  const T s12 = derived_x12<1>(a, m), s13 = derived_x13<1>(a, m), s23 = derived_x23<1>(a, m);
  return s11 + s22 + s33 + (T)2 * (s12 + s13 + s23);
}
// ---- WijWij (rotation_rate, post.f90:153-194)
template <class T, class A> DERIVED_HD T derived_ens(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T e12 = derived_x12<-1>(a, m), e13 = derived_x13<-1>(a, m), e23 = derived_x23<-1>(a, m);
  return (T)2 * (e12 + e13 + e23);
}
// ---- Q (q_criterion, post.f90:196-211)
template <class T, class A> DERIVED_HD T derived_qcr(const A &a, const DerivedMetrics<T> &m) {
  DERIVED_NO_CONTRACT
  const T ens = derived_ens(a, m), str = derived_str(a, m);
  return (T)0.5 * (ens - str);
}

// quantity Q of enum cales_derived
template <int Q, class T, class A> DERIVED_HD T derived_eval(const A &a, const DerivedMetrics<T> &m) {
  static_assert(Q >= 0 && Q < DQ_N, "enum cales_derived");
  if constexpr (Q == DQ_VOX) return derived_vox(a, m);
  else if constexpr (Q == DQ_VOY) return derived_voy(a, m);
  else if constexpr (Q == DQ_VOZ) return derived_voz(a, m);
  else if constexpr (Q == DQ_STR) return derived_str(a, m);
  else if constexpr (Q == DQ_ENS) return derived_ens(a, m);
  else if constexpr (Q == DQ_QCR) return derived_qcr(a, m);
  else if constexpr (Q == DQ_VOX_EDGE) return derived_vox_edge(a, m);
  else if constexpr (Q == DQ_VOY_EDGE) return derived_voy_edge(a, m);
  else return derived_voz_edge(a, m);
}
// ... chosen at run time (a host that loops over the quantities)
template <class T, class A> DERIVED_HD T derived_eval_rt(int q, const A &a, const DerivedMetrics<T> &m) {
  switch (q) {
    case DQ_VOX: return derived_vox(a, m);
    case DQ_VOY: return derived_voy(a, m);
    case DQ_VOZ: return derived_voz(a, m);
    case DQ_STR: return derived_str(a, m);
    case DQ_ENS: return derived_ens(a, m);
    case DQ_QCR: return derived_qcr(a, m);
    case DQ_VOX_EDGE: return derived_vox_edge(a, m);
    case DQ_VOY_EDGE: return derived_voy_edge(a, m);
    default: return derived_voz_edge(a, m);
  }
}
