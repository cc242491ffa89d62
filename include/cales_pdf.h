/* cales_pdf.h -- per-plane probability density functions of a field and joint PDFs of two fields, binned on the device (libcales_hip.so,
 * libcales_hip_sp.so).
 *
 * The reference's utils/pdf-stats.py time-averages per-plane histograms of u, v, w, p and their joint histograms on chosen planes; the entries below
 * produce such counts from the fields on the device: a field is read once and a few kilobytes of integers travel to the host, where cales_get_field
 * would copy the whole haloed array. cales.h holds the time loop, cales_post.h the driver's plane and volume dumps; this is a header of its own.
 *
 * Conventions: those of cales.h -- every entry returns 0 on success and non-zero on error, cales_last_error(ctx) gives the text. Both entries are
 * synchronous. Like cales_get_field they complete a pending projection before they read (cales_step in cales.h) and materialise the lazy eddy
 * viscosity; they allocate nothing that outlives the call. A refused call leaves the context usable.
 *
 * SAMPLES: the stored values of the interior cells 1..n1 x 1..n2 of this rank's slab on plane k, where the staggered grid keeps them, not
 * interpolated (the way cales_out1d treats its field). With several ranks the result is THIS RANK'S sums; the caller adds the ranks (the convention of
 * the statistics entries of cales.h).
 *
 * BIN RULE, fixed to the letter so that the integer counts of two implementations can be compared for equality. All arithmetic in cales_real:
 *   s = (cales_real)nbins / (hi - lo)      once, on the host
 *   t = (x - lo) * s                        that subtraction, then that multiplication (never x*s - lo*s, never a fused multiply-add)
 *   t < 0          the sample counts as BELOW
 *   !(t < nbins)   the sample counts as ABOVE: x >= hi, +inf, NaN and a t that rounds up to nbins
 *   otherwise      bin (int)t
 * so x == lo is in bin 0 and x == hi is above (with a rounded s the product (hi - lo) * s may be the number below nbins: the three operations decide).
 * Refused: a field out of range or not allocated, nbins < 1 or above the cap, lo or hi not finite, hi <= lo, counts NULL.
 */
#ifndef CALES_PDF_H
#define CALES_PDF_H
#include "cales.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CALES_PDF_MAX_BINS  4096   /* 16 KB of 32-bit LDS counters per copy */
#define CALES_JPDF_MAX_BINS 128    /* per axis: 128 x 128 counters = 64 KB */

/* histogram of `field` (enum cales_field) on every plane k = 1 ... n3: counts(nbins, n3) in Fortran order; outside(2, n3), which may be NULL:
 * outside(0, k) the samples below, outside(1, k) those above. counts(:, k) and outside(:, k) together add up to n1 n2 */
int cales_pdf_planes (cales_ctx *ctx, int field, int nbins, cales_real lo, cales_real hi,
                      int64_t *counts, int64_t *outside);

/* joint histogram of field_a and field_b -- the two values of one sample are those at the same index (i, j, k) -- on the nplanes planes kplanes
 * (global k, 1 ... ng(3); any order, repeats allowed): counts(nbins, nbins, nplanes) in Fortran order, first axis = field_a; outside(nplanes), which
 * may be NULL: the samples for which either variable is outside its range. Also refused: nplanes < 1, kplanes NULL or with an entry outside 1 ... ng(3) */
int cales_jpdf_planes(cales_ctx *ctx, int field_a, int field_b, int nbins,
                      cales_real lo_a, cales_real hi_a, cales_real lo_b, cales_real hi_b,
                      int nplanes, const int32_t *kplanes,
                      int64_t *counts, int64_t *outside);

#ifdef __cplusplus
}
#endif
#endif
