/* cales_cospectra.h -- cross-spectra of two fields along x, along y and in x-y planes, transformed on the device (libcales_hip.so, libcales_hip_sp.so).
 *
 * The two-field counterpart of cales_spectra.h, as cales_jpdf_planes is that of cales_pdf_planes: the co-spectrum of u and w shows which wavelengths
 * carry the Reynolds shear stress that cales_out1d_single_point_chan gives as a plane total, the p-u and p-w cross-spectra do the same for the pressure
 * terms of cales_out1d_chan_budgets. Both fields are read once and their lines are transformed in LDS, where two calls of cales_get_field would copy
 * two whole haloed arrays for numpy.fft on the host. A header of its own, the sixth.
 *
 * Conventions: those of cales_spectra.h -- every entry returns 0 on success and non-zero on error, cales_last_error(ctx) gives the text. Both entries
 * are synchronous, complete a pending projection before they read (cales_step in cales.h) and materialise the lazy eddy viscosity; they allocate
 * nothing that outlives the call. A refused call leaves the context usable. The results are the same bits from run to run: no sum is formed with
 * floating-point atomics.
 *
 * SAMPLES: the stored values of the interior cells 1..n1 x 1..n2 of this rank's slab on plane k, at the SAME index (i, j, k) in both fields, where
 * the staggered grid keeps them: not interpolated, no mean removed (the rule of cales_jpdf_planes). Fields that sit at different points of the cell
 * (u on the x face, p at the centre) are half a cell apart along that direction: the phase this leaves in the cross-spectrum along x or y is the
 * caller's to take out (cales_amd/cospectra.py: stagger_phase); a shift along z cannot be taken out.
 *
 * TRANSFORMS: F^a_jk(m), G^a_ik(q) and H^a_k(m,ky) are the unnormalised forward DFTs F, G, H that cales_spectra.h defines, taken of field a, and
 * likewise of field b. The entries return SUMS and leave every normalisation to the host.
 *
 * Refused: either field out of range or not allocated, idir other than 1 or 2, a line longer than CALES_SPECTRA_MAX_LINE (cales_spectra.h),
 * cross / cross2 NULL, nplanes < 1, kplanes NULL or with an entry outside 1 ... ng(3), and idir = 2 or cales_cospectra_planes on a context with
 * nranks > 1 (one rank only). A line whose length has a prime factor above 5 is transformed by the plain sum over its points (correct, not fast);
 * the profile scope of such a call is named cospectra_lines_direct / cospectra_planes_direct.
 */
#ifndef CALES_COSPECTRA_H
#define CALES_COSPECTRA_H
#include "cales.h"
#include "cales_spectra.h"
#ifdef __cplusplus
extern "C" {
#endif

/* field_a == field_b is allowed. lsum_a and lsum_b may each be NULL: the complex line sums of cales_spectra_lines of either field, which the
 * kernel has for free and the host needs to take plane means out of mode 0 afterwards.
 * idir = 1 (lines along x), any number of ranks, THIS RANK'S sums over its rows; the caller adds the ranks:
 *   cross(0:1,m,k)  = sum_j F^a_jk(m) conj(F^b_jk(m)), real and imaginary part: co-spectrum and quadrature spectrum   (2, n1/2+1, n3) in Fortran order
 *   lsum_a(0:1,m,k) = sum_j F^a_jk(m), lsum_b likewise                                                                (2, n1/2+1, n3)
 * idir = 2 (lines along y), one rank only (a slab holds no whole y line): the same with G summed over i                (2, n2/2+1, n3) */
int cales_cospectra_lines (cales_ctx *ctx, int field_a, int field_b, int idir, cales_real *cross, cales_real *lsum_a, cales_real *lsum_b);

/* one rank only; kplanes: global k, 1 ... ng(3), any order, repeats allowed (the rule of cales_jpdf_planes and cales_spectra_planes):
 *   cross2(0:1,m,q,p) = sum over ky in {q, (n2-q) mod n2}, each DISTINCT ky once, of H^a_k(m,ky) conj(H^b_k(m,ky)), k = kplanes[p]
 *   shape (2, n1/2+1, n2/2+1, nplanes) in Fortran order */
int cales_cospectra_planes(cales_ctx *ctx, int field_a, int field_b, int nplanes, const int32_t *kplanes, cales_real *cross2);

#ifdef __cplusplus
}
#endif
#endif
