/* cales_derived.h -- derived fields of the stored velocity, formed on the device (libcales_hip.so, libcales_hip_sp.so): vorticity, SijSij, WijWij and
 * the Q-criterion of the reference's src/post.f90, which a case's out3d.h90 pastes in from utils/useful_fortran_blocks/vorticity-inc.f90 and
 * q-criterion-inc.f90 to write its vox_fld_* / qcr_fld_* visualisation files. Without these entries a host downloads u, v and w whole and does the
 * arithmetic itself; with them it receives the plane, box or strided sample it asked for, or finds the quantity in a field of the library on which
 * every other read-out works (cales_post.h, cales_pdf.h, cales_spectra.h).
 *
 * Conventions: those of cales_post.h -- every entry returns 0 on success and non-zero on error, cales_last_error(ctx) gives the text; the entries are
 * synchronous; a BOX is lo[3], hi[3], nskip[3] in GLOBAL indices of the haloed numbering, a rank's SHARE of it what cales_box_share says, packed in
 * Fortran order count[0] x count[1] x count[2]. count may be NULL. An empty share writes nothing and returns 0; buf may then be NULL.
 *
 * THE ARITHMETIC is the expression of src/post.f90 for the quantity, operation by operation in the order it is written there as Fortran and C parse
 * it (left to right within one precedence level, x**2 as x*x), every operation rounded once: no fused multiply-add is formed. A restatement in the same
 * order in IEEE arithmetic of the library's precision gives the same bits (tests/test_derived_host.py: derived_ref).
 *
 * The quantities are defined for INTERIOR cells 1 ... ng only, as in the reference. They read the ghost cells of u, v and w next to the interior, the
 * edge cells with two ghost indices among them (uz(i, j+1, k-1) at j = ng(2), k = 1), never a cell with three. A quantity is a function of the haloed
 * arrays AS THE CONTEXT HOLDS THEM once a pending projection has been completed and stale x ghost columns have been refreshed, which every entry below
 * does first (cales_step in cales.h): what cales_get_field would return for u, v and w at that moment. On y-slabs the ghost rows are those of the last
 * exchange; the entries are rank-local and exchange nothing. They allocate nothing.
 */
#ifndef CALES_DERIVED_H
#define CALES_DERIVED_H
#include "cales_post.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the quantities; the values are part of the ABI */
enum cales_derived {
  CALES_DERIVED_VOX = 0,       /* vorticity at the cell centre, x component (src/post.f90:14-56) */
  CALES_DERIVED_VOY = 1,       /* ... y component */
  CALES_DERIVED_VOZ = 2,       /* ... z component */
  CALES_DERIVED_STR = 3,       /* SijSij, Sij = (du_i/dx_j + du_j/dx_i)/2 (strain_rate, :58-102) */
  CALES_DERIVED_ENS = 4,       /* WijWij, Wij = (du_i/dx_j - du_j/dx_i)/2 (rotation_rate, :153-194) */
  CALES_DERIVED_QCR = 5,       /* Q = 0.5 (WijWij - SijSij) (q_criterion, :196-211) */
  CALES_DERIVED_VOX_EDGE = 6,  /* vorticity at the cell edge, x component (vorticity_one_component, :104-151) */
  CALES_DERIVED_VOY_EDGE = 7,  /* ... y component */
  CALES_DERIVED_VOZ_EDGE = 8,  /* ... z component */
  CALES_NDERIVED = 9
};

/* the rank's share of the box of quantity `quantity`. Refused: an unknown quantity; what cales_read_box refuses (nskip < 1, lo > hi); lo < 1 or
 * hi > ng in any direction, the quantities being those of interior cells; buf == NULL with a non-empty share. A refused call launches nothing and
 * leaves the context usable. */
int cales_derived_box(cales_ctx *ctx, int quantity, const int32_t lo[3], const int32_t hi[3], const int32_t nskip[3],
                      cales_real *buf, int32_t count[3]);

/* the plane of constant GLOBAL index islice (1 ... ng(inorm)) normal to inorm (1, 2, 3), as cales_out2d gives it for a field */
int cales_derived_out2d(cales_ctx *ctx, int quantity, int inorm, int islice, cales_real *buf, int32_t count[3]);

/* the interior points 1, 1+nskip, 1+2 nskip ... per direction, as cales_out3d gives them for a field */
int cales_derived_out3d(cales_ctx *ctx, int quantity, const int32_t nskip[3], cales_real *buf, int32_t count[3]);

/* the quantity at every interior cell of the rank, written into the INTERIOR of field CALES_PP. The correction pressure is dead between two steps once a
 * pending projection has been completed: this call OVERWRITES it. Its ghost cells are left as they were. Every entry that reads a field then works on
 * the derived quantity under the id CALES_PP: cales_read_box, cales_pdf_planes / cales_jpdf_planes (of Q against the eddy viscosity, say),
 * cales_spectra_lines. The next cales_step writes pp anew. */
int cales_derived_to_pp(cales_ctx *ctx, int quantity);

#ifdef __cplusplus
}
#endif
#endif
