// Stand-alone check of the lane map of the packed remainder tile (cales_amd/csrc/lmf_pack.hpp), built and run by tests/test_lmf_packing_host.py with the
// host compiler and -fsanitize=address,undefined. For every row length n1 = 1..1100 and row count n2 = 1..40, with the tile height of the packed
// instantiations (8 rows, blocks of 64 x 10 threads):
//   1. the full tiles (62 output columns each, as k_lmf_tile maps them) plus the packed remainder blocks put out every cell (i, j) exactly once;
//   2. every output lane of a packed block has its two x neighbours in the lanes beside it, inside its own segment and on its own row, and the halo lanes
//      at the row's end hold the wrapped column (n1 + 1 -> 1);
//   3. every thread of a packed block, dead segments and dead lanes included, sits on a column in 0..n1+1 and on rows (j clamped as the kernel clamps it,
//      and jo +- 1) in 0..n2+1;
//   4. packing is chosen exactly when full >= 1, rem >= 1 and S >= 2.
#include <cstdio>
#include <vector>
#include "lmf_pack.hpp"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int wrap(int i, int n1) { return i == 0 ? n1 : (i == n1 + 1 ? 1 : i); }      // the kernel's perx

int main() {
  const int TL = 8;
  long packed_shapes = 0;
  for (int n1 = 1; n1 <= 1100; ++n1) {
    const LmfPack p = lmf_pack(n1);
    // a stretch needs rem + 2 lanes and starts on a multiple of four lanes (the kernel's sums of four then meet the same partners as in the unpacked tile):
    // S counts pitches of rem + 2 rounded up to four. Whether a row length is packed does not hang on the rounding: 64 / (rem + 2) >= 2 exactly when S >= 2
    const int full = n1 / 62, rem = n1 - 62 * full, pitch = (rem + 2 + 3) / 4 * 4, S = 64 / pitch;
    CHECK(p.full == full && p.rem == rem && p.W == rem + 2 && p.P == pitch && p.P % 4 == 0 && p.S == S, "n1 %d", n1);
    CHECK((64 / (rem + 2) >= 2) == (S >= 2), "n1 %d", n1);
    CHECK(p.on == (full >= 1 && rem >= 1 && S >= 2), "n1 %d", n1);
    if (!p.on) continue;
    CHECK(p.S * p.P <= 64, "n1 %d", n1);
    for (int n2 = 1; n2 <= 40; ++n2) {
      ++packed_shapes;
      const int gy = (n2 + TL - 1) / TL, gyp = lmf_pack_blocks(p, gy);
      CHECK(gyp * p.S >= gy && (gyp - 1) * p.S < gy, "n1 %d n2 %d", n1, n2);
      // the launch of the full tiles: grid.x = full, the unpacked kernel's map. Its output predicate is a product of one in (bx, tx) and one in (by, ty), so
      // a cell is put out cx[i] * cy[j] times: both counted along their own axis (the columns left of the last full tile's end are done with that), then
      // laid out over the columns i0 = 62 full .. n1 + 1 the packed blocks sit on
      const int i0 = 62 * full, nc = n1 + 2 - i0;
      std::vector<int> cx(n1 + 2, 0), cy(n2 + 2, 0), hits((size_t)nc * (n2 + 2), 0);
      for (int bx = 0; bx < full; ++bx) for (int tx = 1; tx <= 62; ++tx) { const int i = bx * 62 + tx; if (i <= n1) ++cx[i]; }
      for (int by = 0; by < gy; ++by) for (int ty = 1; ty <= TL; ++ty) { const int j = by * TL + ty; if (j <= n2) ++cy[j]; }
      for (int i = 0; i < i0; ++i) CHECK(cx[i] == (i >= 1), "n1 %d: column %d put out %d times by the full tiles", n1, i, cx[i]);
      for (int j = 0; j <= n2 + 1; ++j) CHECK(cy[j] == (j >= 1 && j <= n2), "n2 %d: row %d put out %d times by the full tiles", n2, j, cy[j]);
      for (int j = 0; j <= n2 + 1; ++j) for (int i = i0; i <= n1 + 1; ++i) hits[(size_t)j * nc + i - i0] = cx[i] * cy[j];
      for (int by = 0; by < gyp; ++by) for (int ty = 0; ty < TL + 2; ++ty) for (int tx = 0; tx < 64; ++tx) {
        const LmfLane m = lmf_pack_lane(p, tx, ty, by, 0, TL, n2);
        const int jc = m.j < n2 + 1 ? m.j : n2 + 1;      // the kernel's clamp of the thread's own row
        CHECK(m.i >= 0 && m.i <= n1 + 1 && m.lx >= 0 && m.lx < p.P && (tx - m.lx) % 4 == 0, "n1 %d n2 %d by %d tx %d ty %d: i %d", n1, n2, by, tx, ty, m.i);
        CHECK(jc >= 0 && jc <= n2 + 1, "n1 %d n2 %d by %d tx %d ty %d: jc %d", n1, n2, by, tx, ty, jc);
        CHECK(m.jo - 1 >= 0 && m.jo + 1 <= n2 + 1, "n1 %d n2 %d by %d tx %d ty %d: jo %d", n1, n2, by, tx, ty, m.jo);
        CHECK(m.tile >= 0 && m.tile < gy, "n1 %d n2 %d by %d tx %d: tile %d", n1, n2, by, tx, m.tile);
        CHECK(m.live || !m.out, "n1 %d n2 %d by %d tx %d ty %d", n1, n2, by, tx, ty);
        if (!m.out) continue;
        CHECK(m.i >= 1 && m.i <= n1 && m.j >= 1 && m.j <= n2 && m.jo == m.j, "n1 %d n2 %d by %d tx %d ty %d: (%d, %d) jo %d", n1, n2, by, tx, ty, m.i, m.j, m.jo);
        CHECK(m.i >= i0, "n1 %d tx %d: i %d", n1, tx, m.i);
        ++hits[(size_t)m.j * nc + m.i - i0];
        CHECK(tx >= 1 && tx <= 62, "n1 %d tx %d", n1, tx);
        const LmfLane l = lmf_pack_lane(p, tx - 1, ty, by, 0, TL, n2), r = lmf_pack_lane(p, tx + 1, ty, by, 0, TL, n2);
        CHECK(l.seg == m.seg && r.seg == m.seg && l.j == m.j && r.j == m.j && l.jo == m.jo && r.jo == m.jo, "n1 %d n2 %d by %d tx %d ty %d", n1, n2, by, tx, ty);
        CHECK(wrap(l.i, n1) == (m.i == 1 ? n1 : m.i - 1) && wrap(r.i, n1) == (m.i == n1 ? 1 : m.i + 1), "n1 %d tx %d: %d %d %d", n1, tx, l.i, m.i, r.i);
        // the rows above and below (LDS neighbours [ty +- 1][tx]) belong to the same segment and the same column
        const LmfLane d = lmf_pack_lane(p, tx, ty - 1, by, 0, TL, n2), u = lmf_pack_lane(p, tx, ty + 1, by, 0, TL, n2);
        CHECK(d.i == m.i && u.i == m.i && d.j == m.j - 1 && u.j == m.j + 1, "n1 %d n2 %d by %d tx %d ty %d", n1, n2, by, tx, ty);
      }
      for (int j = 0; j <= n2 + 1; ++j) for (int i = i0; i <= n1 + 1; ++i) {
        const int want = (i >= 1 && i <= n1 && j >= 1 && j <= n2) ? 1 : 0;
        CHECK(hits[(size_t)j * nc + i - i0] == want, "n1 %d n2 %d: cell (%d, %d) put out %d times", n1, n2, i, j, hits[(size_t)j * nc + i - i0]);
      }
    }
  }
  // the row lengths of the table in DESIGN.md
  const int tab[][3] = {{64, 2, 16}, {128, 4, 8}, {192, 6, 8}, {256, 8, 5}, {384, 12, 4}, {512, 16, 3}, {768, 24, 2}, {1024, 32, 1}};
  for (const auto &t : tab) { const LmfPack p = lmf_pack(t[0]); CHECK(p.rem == t[1] && p.S == t[2] && p.on == (t[2] >= 2), "n1 %d", t[0]); }
  std::printf("%ld packed shapes checked, %d failures\n", packed_shapes, fails);
  return fails ? 1 : 0;
}
