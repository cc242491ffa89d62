/* cales_spectra.h -- power spectra of a field along x, along y and in x-y planes, transformed on the device (libcales_hip.so, libcales_hip_sp.so).
 *
 * The reference's utils/spectra-stats.py time-averages 1-D spectra of u, v, w, p on every plane and 2-D spectra on chosen planes; the entries below
 * produce the sums such spectra are made of from the fields on the device: a field is read once and its lines are transformed in LDS, where
 * cales_get_field would copy the whole haloed array for numpy.fft on the host. cales.h holds the time loop, cales_post.h the driver's plane and volume
 * dumps, cales_pdf.h the histograms; this is a header of its own.
 *
 * Conventions: those of cales.h -- every entry returns 0 on success and non-zero on error, cales_last_error(ctx) gives the text. Both entries are
 * synchronous. Like cales_get_field they complete a pending projection before they read (cales_step in cales.h) and materialise the lazy eddy
 * viscosity; they allocate nothing that outlives the call. A refused call leaves the context usable. The results are the same bits from run to run:
 * no sum is formed with floating-point atomics.
 *
 * SAMPLES: the stored values of the interior cells 1..n1 x 1..n2 of this rank's slab on plane k, where the staggered grid keeps them, not
 * interpolated, no mean removed (the rule of cales_pdf.h). Boundary conditions are not consulted: the DFT of the samples is defined whatever they
 * are, and whether a direction is periodic is the caller's business.
 *
 * TRANSFORMS: unnormalised forward DFTs (numpy.fft.rfft along the line, numpy.fft.fft across), I the imaginary unit:
 *   F_jk(m) = sum_{i=1..n1} f(i,j,k) exp(-2 pi I m (i-1) / n1),   m = 0 ... n1/2 (integer division)
 *   G_ik(q) = sum_{j=1..n2} f(i,j,k) exp(-2 pi I q (j-1) / n2),   q = 0 ... n2/2
 *   H_k(m,ky) the 2-D DFT of plane k, m = 0 ... n1/2, ky = 0 ... n2-1
 * The entries return SUMS and leave every normalisation to the host, as the entries of cales_pdf.h return counts.
 *
 * Refused: a field out of range or not allocated, idir other than 1 or 2, a line longer than CALES_SPECTRA_MAX_LINE, power / power2 NULL,
 * nplanes < 1, kplanes NULL or with an entry outside 1 ... ng(3), and idir = 2 or cales_spectra_planes on a context with nranks > 1 (one rank only).
 * A line whose length has a prime factor above 5 is transformed by the plain sum over its points (correct, not fast); the profile scope of such a
 * call is named spectra_lines_direct / spectra_planes_direct.
 */
#ifndef CALES_SPECTRA_H
#define CALES_SPECTRA_H
#include "cales.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CALES_SPECTRA_MAX_LINE 2048   /* longest line transformed; longer: refused */

/* idir = 1 (lines along x), any number of ranks, THIS RANK'S sums over its rows; the caller adds the ranks:
 *   power(m,k)    = sum_j |F_jk(m)|^2                     (n1/2+1, n3) in Fortran order
 *   lsum(0:1,m,k) = sum_j F_jk(m), real and imaginary     (2, n1/2+1, n3); may be NULL
 * idir = 2 (lines along y), one rank only (a slab holds no whole y line):
 *   power(q,k)    = sum_i |G_ik(q)|^2                     (n2/2+1, n3)
 *   lsum(0:1,q,k) = sum_i G_ik(q)                         (2, n2/2+1, n3)
 * lsum is a complex sum, not a power: it stays additive over the ranks, and squared afterwards it is the spectrum of the line-averaged signal */
int cales_spectra_lines (cales_ctx *ctx, int field, int idir, cales_real *power, cales_real *lsum);

/* one rank only; kplanes: global k, 1 ... ng(3), any order, repeats allowed (the rule of cales_jpdf_planes):
 *   power2(m,q,p) = sum over ky in {q, (n2-q) mod n2}, each DISTINCT ky once, of |H_k(m,ky)|^2, k = kplanes[p]
 *   shape (n1/2+1, n2/2+1, nplanes) in Fortran order */
int cales_spectra_planes(cales_ctx *ctx, int field, int nplanes, const int32_t *kplanes, cales_real *power2);

#ifdef __cplusplus
}
#endif
#endif
