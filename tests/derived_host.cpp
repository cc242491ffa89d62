// The arithmetic of the derived fields (cales_amd/csrc/derived_math.hpp) on the CPU: a stand-alone program (its own main, nothing loaded into Python) that
// evaluates all nine quantities of include/cales_derived.h in double and in float at every interior cell of a haloed field read from a file, and writes the
// results back. tests/test_derived_host.py writes the field, builds this file with the host compiler under -fsanitize=address,undefined -ffp-contract=off, runs
// it once and demands the bits of its numpy restatement.
//
//   derived_host IN OUT
// IN  (doubles): n1 n2 n3 dxi dyi | dzci(0:n3+1) | dzfi(0:n3+1) | u, v, w (0:n1+1, 0:n2+1, 0:n3+1), Fortran order
// OUT (doubles): the nine quantities (n1, n2, n3) each, Fortran order, evaluated in double | the same evaluated in float from the inputs rounded to float
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "derived_math.hpp"

template <class T> struct HostCell {
  const T *pu, *pv, *pw; long c, s1, s12;
  T u(int di, int dj, int dk) const { return pu[c + di + dj * s1 + dk * s12]; }
  T v(int di, int dj, int dk) const { return pv[c + di + dj * s1 + dk * s12]; }
  T w(int di, int dj, int dk) const { return pw[c + di + dj * s1 + dk * s12]; }
};

template <class T>
static void evaluate(int n1, int n2, int n3, const std::vector<double> &in, std::vector<double> &out) {
  const size_t nh = (size_t)(n1 + 2) * (n2 + 2) * (n3 + 2);
  std::vector<T> a(in.size());
  for (size_t q = 0; q < in.size(); ++q) a[q] = (T)in[q];
  const T dxi = a[3], dyi = a[4];
  const T *dzci = a.data() + 5, *dzfi = dzci + n3 + 2, *u = dzfi + n3 + 2, *v = u + nh, *w = v + nh;
  const long s1 = n1 + 2, s12 = (long)(n1 + 2) * (n2 + 2);
  for (int q = 0; q < DQ_N; ++q)
    for (int k = 1; k <= n3; ++k) for (int j = 1; j <= n2; ++j) for (int i = 1; i <= n1; ++i) {
      const DerivedMetrics<T> m{dxi, dyi, dzci[k - 1], dzci[k], dzfi[k]};
      const HostCell<T> cell{u, v, w, i + j * s1 + k * s12, s1, s12};
      out.push_back((double)derived_eval_rt<T>(q, cell, m));
    }
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: derived_host IN OUT\n"); return 2; }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  double head[3];
  if (std::fread(head, sizeof(double), 3, f) != 3) { std::fprintf(stderr, "short input\n"); return 2; }
  const int n1 = (int)head[0], n2 = (int)head[1], n3 = (int)head[2];
  if (n1 < 1 || n2 < 1 || n3 < 1 || n1 > 64 || n2 > 64 || n3 > 64) { std::fprintf(stderr, "bad sizes\n"); return 2; }
  const size_t n = 5 + 2 * (size_t)(n3 + 2) + 3 * (size_t)(n1 + 2) * (n2 + 2) * (n3 + 2);
  std::vector<double> in(n);
  in[0] = head[0]; in[1] = head[1]; in[2] = head[2];
  if (std::fread(in.data() + 3, sizeof(double), n - 3, f) != n - 3) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  std::vector<double> out;
  evaluate<double>(n1, n2, n3, in, out);
  evaluate<float>(n1, n2, n3, in, out);
  FILE *g = std::fopen(argv[2], "wb");
  if (!g) { std::perror(argv[2]); return 2; }
  if (std::fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) { std::fprintf(stderr, "short write\n"); return 2; }
  std::fclose(g);
  std::printf("%zu values of %d quantities in double and float written\n", out.size(), (int)DQ_N);
  return 0;
}
