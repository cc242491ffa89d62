/* cales_post.h -- the output side of the C-ABI (libcales_hip.so, libcales_hip_sp.so): parts of a field, read from the device.
 *
 * cales.h holds one entry per routine the reference driver calls INSIDE its time loop; these are the driver's output calls, made every iout2d / iout3d
 * steps from the case's out2d.h90 / out3d.h90 (reference src/main.f90:580-589): out2d (src/output.f90:164-189) and out3d (src/output.f90:191-242).
 * cales_get_field / cales_download_state copy the whole haloed array to the host; the entries below pack a plane, a box or a strided sample on the
 * device and copy only that.
 *
 * Conventions: those of cales.h -- every entry returns 0 on success and non-zero on error, cales_last_error(ctx) gives the text (cales_last_error(NULL)
 * for the host-only cales_box_share).
 *
 * A BOX is given by lo[3], hi[3], nskip[3]: the points lo[d] + m nskip[d] <= hi[d], m = 0, 1, ..., in GLOBAL indices of the haloed numbering
 * 0 ... ng(d)+1 (the same on every rank). Refused: nskip < 1, lo < 0, hi > ng+1, lo > hi.
 * A rank's SHARE of a box (y-slab decomposition of cales_case: nranks, rank): every point of the box in x and z; in y the points whose global row the
 * rank owns, rank ng2/nranks + 1 ... (rank + 1) ng2/nranks -- rank 0 also holds the global row 0, the last rank the row ng2+1. The halo rows between
 * two slabs are nobody's share: they are owned rows of the neighbour. The shares of the ranks are disjoint and their union, in rank order, is the box.
 */
#ifndef CALES_POST_H
#define CALES_POST_H
#include "cales.h"
#ifdef __cplusplus
extern "C" {
#endif

/* host-only, needs no GPU: the share of one rank (c->nranks, c->rank) in a strided box of GLOBAL haloed indices. first[d]: global index of the first
 * point of the share (where the host places the share in a file), count[d]: its number of points. count[1] may be 0: the rank holds no row of the box. */
int cales_box_share(const cales_case *c, const int32_t lo[3], const int32_t hi[3], const int32_t nskip[3],
                    int32_t first[3], int32_t count[3]);

/* the rank's share of the box, packed in Fortran order count[0] x count[1] x count[2] (sync). `field`: enum cales_field, refused when out of range or
 * not allocated (the rule of cales_get_field). count may be NULL. An empty share writes nothing and returns 0; buf may then be NULL.
 * Like cales_get_field the three entries below complete a pending projection and bring stale x ghost columns up to date before they read (cales_step
 * in cales.h), and allocate nothing. */
int cales_read_box(cales_ctx *ctx, int field, const int32_t lo[3], const int32_t hi[3], const int32_t nskip[3],
                   cales_real *buf, int32_t count[3]);

/* out2d (src/output.f90:164-189): interior plane of constant GLOBAL index islice (1 ... ng(inorm)) normal to inorm (1, 2, 3):
 * cales_read_box with lo = hi = islice in direction inorm, 1 ... ng in the other two, nskip = 1 */
int cales_out2d(cales_ctx *ctx, int field, int inorm, int islice, cales_real *buf, int32_t count[3]);

/* out3d (src/output.f90:191-242): interior points 1, 1+nskip, 1+2 nskip ... per direction: cales_read_box with lo = 1, hi = ng */
int cales_out3d(cales_ctx *ctx, int field, const int32_t nskip[3], cales_real *buf, int32_t count[3]);

#ifdef __cplusplus
}
#endif
#endif
