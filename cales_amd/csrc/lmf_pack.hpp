// The remainder x tile of the dynamic model's last pass (k_lmf_tile, k_sgs.hip), packed: the pass works on tiles of 62 output columns with the x halo
// inside the wave, so a row of n1 cells takes n1 / 62 full tiles and one tile of rem = n1 - 62 (n1 / 62) live columns -- 16 of 64 lanes at 512 cells. A live
// stretch of that tile needs W = rem + 2 lanes; stretches start every P lanes, P = W rounded up to a multiple of four, and S = 64 / P of them fit into one
// wave, each with its own two halo lanes and each on another y tile: the remainder column of the tile grid then takes ceil(gy / S) blocks per k chunk
// instead of gy. (Four: the kernel adds its lanes in aligned fours before anything else; with stretches that start on a multiple of four every cell meets
// the same partners in the same order as in the unpacked tile, and the block sums of a y tile come out equal to the bit.) This header is the lane map of
// that form and nothing else; it compiles without HIP (tests/test_lmf_packing_host.py runs it on the CPU over every row length).
#pragma once
#if defined(__HIPCC__)
#define LMF_HD __host__ __device__
#else
#define LMF_HD
#endif

constexpr int LMF_WX = 62;      // output columns of a full tile (64 lanes less the two halo lanes)

struct LmfPack { int full, rem, W, P, S; bool on; };      // full tiles, live columns of the remainder tile, lanes a stretch needs, lanes from one stretch to the next, stretches per wave; on: the packed form serves this row length
LMF_HD inline LmfPack lmf_pack(int n1) {
  LmfPack p;
  p.full = n1 / LMF_WX; p.rem = n1 - LMF_WX * p.full; p.W = p.rem + 2; p.P = (p.W + 3) & ~3; p.S = 64 / p.P;
  p.on = p.full >= 1 && p.rem >= 1 && p.S >= 2;
  return p;
}
LMF_HD inline int lmf_pack_blocks(const LmfPack &p, int gy) { return (gy + p.S - 1) / p.S; }      // packed blocks for gy y tiles

// Thread (tx, ty) of packed block `by`: segment, column slot, cell column i (n1 + 1 in the upper halo lane: the kernel wraps it to 1), y tile, row j of the
// thread and the row jo whose |S|Sij it combines (as in the unpacked form: halo rows and rows beyond n2 take a row of the tile's interior), and `out`: the
// thread owns an output cell. Lanes behind a stretch's upper halo lane sit on that lane's column; lanes behind the last segment and segments whose y tile
// lies beyond the last one are dead: they sit on the last segment's / the last tile's rows, so that every address derived from (i, j, jo) stays inside the
// field, and put out nothing.
struct LmfLane { int seg, lx, i, tile, j, jo; bool live, out; };
LMF_HD inline LmfLane lmf_pack_lane(const LmfPack &p, int tx, int ty, int by, int by0, int tl, int n2) {
  LmfLane m;
  const int gy = (n2 + tl - 1) / tl;      // y tiles of the field
  m.seg = tx / p.P; m.lx = tx - m.seg * p.P;
  const int t = by * p.S + m.seg + by0;
  m.live = m.seg < p.S && t < gy;
  const int sg = m.seg < p.S ? m.seg : p.S - 1, tc = by * p.S + sg + by0;
  m.tile = tc < gy ? tc : gy - 1;
  m.i = LMF_WX * p.full + (m.lx < p.W ? m.lx : p.W - 1);
  m.j = m.tile * tl + ty;
  const int jin = m.j < m.tile * tl + tl ? m.j : m.tile * tl + tl, jn = jin < n2 ? jin : n2;
  m.jo = jn > m.tile * tl + 1 ? jn : m.tile * tl + 1;
  m.out = m.live && m.lx >= 1 && m.lx <= p.rem && ty >= 1 && ty <= tl && m.j <= n2;
  return m;
}
