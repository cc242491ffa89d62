// Stand-alone check of the host parts of cales_amd/csrc/readout.hpp and spectral_line.hpp, built and run by tests/test_readout_host.py with the host
// compiler and -fsanitize=address,undefined:
//   1. row_runs gives, for every input, the rows per block and the blocks per plane that the two functions it replaced gave -- pdf_geom (k_pdf.hip) and
//      spec_x_geom (k_spectra.hip) as they stood before, restated below to the letter. n1, n2 = 1..2048, nplanes = 1..64, counters 1, 256, 4096, 16384 for
//      the histograms; the three line counts of spec_nl (8, 4, 2) for the spectra. The histogram sweep is thinned: every n1 and n2 up to 64, and above
//      that the values beside a step of one of the roundings (multiples of `want` for n2; powers of two and the divisors of the sample floor for n1);
//   1b. the launch geometry of the spectra kernels (spectral_line.hpp: spec_geom_x, spec_geom_y, spec_geom_y2 of nf = 1, 2 fields) against the rules of
//      the power spectra and of the cross-spectra as they stood when each had kernels of its own (k_spectra.hip, k_cospectra.hip), restated below to the
//      letter: rows, chunks, nl, nh and nb for reals of 4 and 8 bytes; x over the thinned n1, n2 and every nplanes of 1, y and y2 over the thinned n1 and every n2;
//   2. TempCarver: for every sequence of up to four parts of 4-, 8- and 16-byte elements with counts 0, 1, 3 and 7, every part starts on a 16-byte boundary, the
//      parts do not overlap (each is filled with a tag of its own and read again) and the last ends inside the total, in reals of 4 and of 8 bytes;
//   3. plane_list_check: the three refusals with `who` in front, and a list with repeats in any order accepted.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "spectral_line.hpp"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ---- 1. the two rules as they stood (their context's sizes as arguments; spec_x_geom's nl = spec_nl(n1))
static void pdf_geom_was(int n1, int n2, int nplanes, int ncounters, int *rows_out, int *nbx) {
  const int want = (2048 + nplanes - 1) / nplanes, least = std::max(4096, ncounters);
  int rows = std::max((n2 + want - 1) / want, (least + n1 - 1) / n1);
  rows = std::min(std::max(rows, 1), n2);
  *nbx = (n2 + rows - 1) / rows; *rows_out = rows;
}
static void spec_x_geom_was(int n2, int nplanes, int nl, int *rows_out, int *nb) {
  const int want = (2048 + nplanes - 1) / nplanes, batch = 2 * nl;
  int rows = (n2 + want - 1) / want;
  rows = (rows + batch - 1) / batch * batch;
  *rows_out = rows; *nb = (n2 + rows - 1) / rows;
}
static bool near_step(int n, int step) { const int r = n % step; return r <= 1 || r == step - 1; }
static long check_row_runs() {
  long n = 0;
  const int counters[4] = {1, 256, 4096, 16384};
  std::vector<int> n1s;
  for (int n1 = 1; n1 <= 2048; ++n1)
    if (n1 <= 64 || (n1 & (n1 - 1)) == 0 || (n1 & (n1 + 1)) == 0 || ((n1 - 1) & (n1 - 2)) == 0 || 4096 % n1 <= 1 || 16384 % n1 <= 1 || n1 % 97 == 0) n1s.push_back(n1);
  for (int nplanes = 1; nplanes <= 64; ++nplanes) {
    const int want = (2048 + nplanes - 1) / nplanes;
    for (int n2 = 1; n2 <= 2048; ++n2) {
      if (n2 > 64 && !near_step(n2, want) && n2 % 101) continue;
      for (int n1 : n1s) for (int nc : counters) {
        int rows, nbx; pdf_geom_was(n1, n2, nplanes, nc, &rows, &nbx);
        const RowRuns rr = row_runs(n2, nplanes, (std::max(4096, nc) + n1 - 1) / n1, 1);      // as pdf_geom calls it
        CHECK(rr.rows == rows && rr.per_plane == nbx, "pdf n1 %d n2 %d nplanes %d counters %d: %d x %d, was %d x %d", n1, n2, nplanes, nc, rr.rows, rr.per_plane, rows, nbx);
        ++n;
      }
    }
    for (int n2 = 1; n2 <= 2048; ++n2) for (int nl = 8; nl >= 2; nl /= 2) {
      int rows, nb; spec_x_geom_was(n2, nplanes, nl, &rows, &nb);
      const RowRuns rr = row_runs(n2, nplanes, 1, 2 * nl);      // as spec_x_geom calls it
      CHECK(rr.rows == rows && rr.per_plane == nb, "spectra n2 %d nplanes %d nl %d: %d x %d, was %d x %d", n2, nplanes, nl, rr.rows, rr.per_plane, rows, nb);
      ++n;
    }
  }
  return n;
}

// ---- 1b. the geometry of the spectra kernels as the two units had it: `real` a type of `rsz` bytes, REALV = 16 / rsz, sizeof(real2) = 2 rsz
static int spec_nl_was(int N, size_t rsz) {
  int nl = 8;
  while (nl > 2 && 2 * (size_t)nl * N * (2 * rsz) > 64 * 1024) nl /= 2;
  return nl;
}
static void spec_x_geom_was(int n1, int n2, int nplanes, size_t rsz, SpecGeom *sg) {
  const int REALV = 16 / (int)rsz;
  sg->nl = spec_nl_was(n1, rsz); sg->nh = n1 / 2 + 1; sg->chunks = (n1 + REALV - 1) / REALV;
  const RowRuns rr = row_runs(n2, nplanes, 1, 2 * sg->nl);
  sg->rows = rr.rows; sg->nb = rr.per_plane;
}
static void cospec_x_geom_was(int n1, int n2, int nplanes, size_t rsz, SpecGeom *sg) {
  const int REALV = 16 / (int)rsz;
  sg->nl = spec_nl_was(n1, rsz); sg->nh = n1 / 2 + 1; sg->chunks = (n1 + REALV - 1) / REALV;
  const RowRuns rr = row_runs(n2, nplanes, 1, sg->nl);
  sg->rows = rr.rows; sg->nb = rr.per_plane;
}
static SpecGeom spec_y_geom_was(int n1, int N, size_t rsz) {
  const int REALV = 16 / (int)rsz;
  SpecGeom sg; sg.nl = spec_nl_was(N, rsz); sg.nh = N / 2 + 1; sg.rows = 0; sg.chunks = 2 * sg.nl / REALV; sg.nb = (n1 + 2 * sg.nl - 1) / (2 * sg.nl);
  return sg;
}
static SpecGeom cospec_y_geom_was(int n1, int N, size_t rsz) {
  const int REALV = 16 / (int)rsz;
  SpecGeom sg; sg.nl = spec_nl_was(N, rsz); sg.nh = N / 2 + 1; sg.rows = 0; sg.chunks = sg.nl / REALV; sg.nb = (n1 + sg.nl - 1) / sg.nl;
  return sg;
}
static SpecGeom spec_y2_geom_was(int n1, int n2, size_t rsz) {
  const int nhx = n1 / 2 + 1, nhy = n2 / 2 + 1;
  SpecGeom sy; sy.nl = spec_nl_was(n2, rsz); sy.nh = nhy; sy.rows = 0; sy.chunks = 0; sy.nb = (nhx + sy.nl - 1) / sy.nl;
  return sy;
}
static SpecGeom cospec_y2_geom_was(int n1, int n2, size_t rsz) {
  const int nhx = n1 / 2 + 1, nhy = n2 / 2 + 1;
  SpecGeom sy; sy.nl = spec_nl_was(n2, rsz); sy.nh = nhy; sy.rows = 0; sy.chunks = 0; sy.nb = (nhx + sy.nl / 2 - 1) / (sy.nl / 2);
  return sy;
}
static void same_geom(const char *what, const SpecGeom &g, const SpecGeom &w, int n1, int n2, int nplanes, int nf, size_t rsz) {
  CHECK(g.rows == w.rows && g.chunks == w.chunks && g.nl == w.nl && g.nh == w.nh && g.nb == w.nb, "%s n1 %d n2 %d nplanes %d nf %d reals of %zu: %d %d %d %d %d, was %d %d %d %d %d",
        what, n1, n2, nplanes, nf, rsz, g.rows, g.chunks, g.nl, g.nh, g.nb, w.rows, w.chunks, w.nl, w.nh, w.nb);
}
static long check_spec_geom() {
  long n = 0;
  std::vector<int> n1s;      // every n1 up to 64, and above that the values beside a step of spec_nl (powers of two) and a few others
  for (int n1 = 1; n1 <= 2048; ++n1) if (n1 <= 64 || (n1 & (n1 - 1)) == 0 || (n1 & (n1 + 1)) == 0 || ((n1 - 1) & (n1 - 2)) == 0 || n1 % 97 == 0) n1s.push_back(n1);
  for (size_t rsz = 4; rsz <= 8; rsz += 4) for (int nf = 1; nf <= 2; ++nf) for (int n1 : n1s) {
    for (int nplanes = 1; nplanes <= 64; ++nplanes) {
      const int want = (2048 + nplanes - 1) / nplanes;
      for (int n2 = 1; n2 <= 2048; ++n2) {
        if (n2 > 64 && !near_step(n2, want) && n2 % 101) continue;
        SpecGeom was; if (nf == 1) spec_x_geom_was(n1, n2, nplanes, rsz, &was); else cospec_x_geom_was(n1, n2, nplanes, rsz, &was);
        same_geom("x", spec_geom_x(n1, n2, nplanes, nf, rsz), was, n1, n2, nplanes, nf, rsz);
        ++n;
      }
    }
    for (int n2 = 1; n2 <= 2048; ++n2) {
      same_geom("y", spec_geom_y(n1, n2, nf, rsz), nf == 1 ? spec_y_geom_was(n1, n2, rsz) : cospec_y_geom_was(n1, n2, rsz), n1, n2, 0, nf, rsz);
      same_geom("y2", spec_geom_y2(n1, n2, nf, rsz), nf == 1 ? spec_y2_geom_was(n1, n2, rsz) : cospec_y2_geom_was(n1, n2, rsz), n1, n2, 0, nf, rsz);
      n += 2;
    }
  }
  // the one geometry without chunks: two fields in single precision at nl = 2
  CHECK(spec_geom_y(64, 2048, 2, 4).chunks == 0 && spec_geom_y(64, 1024, 2, 4).chunks == 1 && spec_geom_y(64, 2048, 1, 4).chunks == 1 && spec_geom_y(64, 2048, 2, 8).chunks == 1, "chunks of a y tile");
  return n;
}

// ---- 2. the carver
struct Elem16 { double x, y; };
static long check_carver() {
  long n = 0;
  const size_t counts[4] = {0, 1, 3, 7};
  for (int len = 1; len <= 4; ++len) {
    int total = 1; for (int q = 0; q < len; ++q) total *= 12;
    for (int code = 0; code < total; ++code) {
      TempCarver tc;
      size_t at[4], bytes[4];
      for (int q = 0, c = code; q < len; ++q, c /= 12) {
        const int type = c % 3; const size_t cnt = counts[(c % 12) / 3];
        if (type == 0) { at[q] = tc.part<int32_t>(cnt).at; bytes[q] = cnt * 4; }
        else if (type == 1) { at[q] = tc.part<uint64_t>(cnt).at; bytes[q] = cnt * 8; }
        else { at[q] = tc.part<Elem16>(cnt).at; bytes[q] = cnt * 16; }
      }
      for (size_t rsz = 4; rsz <= 8; rsz += 4) {
        const size_t size = tc.reals(rsz) * rsz;      // what CtxTemp allocates
        char *base = (char *)std::aligned_alloc(256, (size + 255) / 256 * 256 + 256);      // (device allocations are aligned to 256 bytes)
        CHECK(at[len - 1] + bytes[len - 1] <= size, "sequence %d of %d, reals of %zu: the last part ends at %zu of %zu", code, len, rsz, at[len - 1] + bytes[len - 1], size);
        for (int q = 0; q < len; ++q) {
          const TempPart<char> p{at[q]};
          CHECK(((uintptr_t)p.in(base) & 15u) == 0, "sequence %d of %d: part %d at %zu", code, len, q, at[q]);
          if (at[q] + bytes[q] <= size) std::memset(p.in(base), q + 1, bytes[q]);      // (past the allocation the sanitizer would stop the run)
        }
        for (int q = 0; q < len; ++q) for (size_t b = 0; b < bytes[q] && at[q] + b < size; ++b)
          if (base[at[q] + b] != q + 1) { CHECK(false, "sequence %d of %d: part %d overlaps part %d", code, len, q, base[at[q] + b] - 1); break; }
        std::free(base);
        ++n;
      }
    }
  }
  // typed pointers land where the offsets say
  TempCarver tc; const auto a = tc.part<int32_t>(3); const auto b = tc.part<Elem16>(1); const auto c = tc.part<uint64_t>(5);
  char *base = (char *)std::aligned_alloc(256, 256);
  CHECK((char *)a.in(base) == base && (char *)b.in(base) == base + 16 && (char *)c.in(base) == base + 32 && tc.bytes == 80 && tc.reals(4) == 20 && tc.reals(8) == 10, "bytes %zu", tc.bytes);
  std::free(base);
  return n;
}

// ---- 3. the plane list
static int check_planes() {
  std::string err;
  const int32_t ok[6] = {3, 1, 3, 12, 1, 12}, low[3] = {1, 0, 2}, high[2] = {13, 1}, neg[1] = {-4};
  CHECK(plane_list_check("who", 6, ok, 12, err) == 0 && err.empty(), "%s", err.c_str());
  CHECK(plane_list_check("who", 1, ok, 3, err) == 0 && err.empty(), "%s", err.c_str());
  CHECK(plane_list_check("who", 0, ok, 12, err) == 1 && err == "who: nplanes < 1", "%s", err.c_str());
  CHECK(plane_list_check("who", -2, ok, 12, err) == 1 && err == "who: nplanes < 1", "%s", err.c_str());
  CHECK(plane_list_check("cales_x", 2, nullptr, 12, err) == 1 && err == "cales_x: kplanes is NULL", "%s", err.c_str());
  CHECK(plane_list_check("who", 0, nullptr, 12, err) == 1 && err == "who: nplanes < 1", "%s", err.c_str());      // (the order of the checks)
  CHECK(plane_list_check("who", 3, low, 12, err) == 1 && err == "who: plane outside 1 ... ng(3)", "%s", err.c_str());
  CHECK(plane_list_check("who", 2, high, 12, err) == 1 && err == "who: plane outside 1 ... ng(3)", "%s", err.c_str());
  CHECK(plane_list_check("who", 1, neg, 12, err) == 1 && err == "who: plane outside 1 ... ng(3)", "%s", err.c_str());
  CHECK(plane_list_check("who", 6, ok, 11, err) == 1, "%s", err.c_str());
  return 10;
}

int main() {
  const long nr = check_row_runs(), ng = check_spec_geom(), nc = check_carver();
  const int np = check_planes();
  std::printf("%ld row rules, %ld spectra geometries, %ld carved temporaries, %d plane lists checked, %d failures\n", nr, ng, nc, np, fails);
  return fails ? 1 : 0;
}
