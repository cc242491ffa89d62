"""Shared helpers for the tests: golden fixtures -> Case, comparison norms."""
import os

import numpy as np

from cales_amd.nml import parse_text

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RK = [(32. / 60., 0.), (25. / 60., -17. / 60.), (45. / 60., -25. / 60.)]      # reference src/param.f90:27-29
FULL_CASES = ["tgv_ppp", "tgv_dsmag_ppp", "chan_smag_wm", "chan_smag", "chan_dsmag", "chan_dsmag_wm", "duct_smag_wm", "duct_smag_wm_imp1d",
              "cavity_nnn", "devchan_nd", "halfchan_imp1d", "duct_dsmag_wm", "duct_dsmag", "cavity_dsmag",
              # the wall model beyond the shipped examples (wmodel.f90:65-335): faces in x, the laminar law, moving walls, a model on one side of a direction
              "cavity_smag_wm6", "cavity_dsmag_wm_mixed", "chan_smag_wm_mov", "halfchan_smag_wm_imp1d", "halfchan_dsmag_wm"]
# a further full case held operator by operator only (set-up, initial field, start-up and substeps, solver operands): a cavity with three different edge
# lengths and the laminar law on its x and y faces, the one place where that law's `l1d = l(idir)` (wmodel.f90:150,201) differs from l(3). It stays out of
# the plane statistics: the pressure-strain sum of v (row 13 of the budget, a sum that cancels) comes out 1.4e-13 of the row's maximum away from the
# reference's summation order on this case, against the 1e-13 those tests hold a numpy sum in another order to
STAGE_CASES = FULL_CASES + ["cavity_smag_wm_lam"]


# cases DERIVED from a golden file's input.nml (compared with the oracle only, no reference-made stage vectors carry these names)
DERIVED = {"duct_smag": ("duct_smag_wm", lambda case: case.lwm.fill(0))}      # static Smagorinsky duct with no-slip walls, no wall model


def load_golden(name):
    edit = None
    if name in DERIVED:
        name, edit = DERIVED[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    case = parse_text(str(g["input_nml"]))
    case.impdiff = int(g["impdiff"])
    if edit:
        edit(case)
    return g, case


def F(a):
    return np.asfortranarray(np.array(a, dtype=np.float64))


def relerr(a, b):
    """L-infinity error scaled by the field maximum."""
    a = np.asarray(a); b = np.asarray(b)
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() / scale


def triperiodic_solve_scipy(o, case, rhs):
    """The reference's solve of a triply periodic pressure problem (solver.f90:20-80 with gaussel_periodic / dgtsv_homebrewed, :109-179, +eps pivots,
    one operation at a time) evaluated with scipy's FFTs instead of the oracle's own: a second, independent evaluation of the SAME algorithm.
    Columns are solved with the reference's sequential order, vectorised over the columns (numpy rounds every operation, no contraction)."""
    import scipy.fft as sf
    eps = np.finfo(float).eps
    ng = tuple(int(x) for x in case.ng); n = ng[2]
    lam, a, b, c, nrm = o.solver_operands(0)
    hx = np.minimum(np.arange(ng[0]), ng[0] - np.arange(ng[0])); hy = np.minimum(np.arange(ng[1]), ng[1] - np.arange(ng[1]))
    L = lam[np.ix_(hx, hy)].reshape(-1)      # eigenvalue of complex mode (kx, ky) = that of the half-complex entries of wavenumbers min(k, n - k)

    def dgtsv(m, bb, p):
        d = np.zeros_like(bb); z = 1. / (bb[0] + eps); d[0] = c[0] * z; p[0] = p[0] * z
        for l in range(1, m):
            z = 1. / (bb[l] - a[l] * d[l - 1] + eps); d[l] = c[l] * z; p[l] = (p[l] - a[l] * p[l - 1]) * z
        for l in range(m - 2, -1, -1):
            p[l] = p[l] - d[l] * p[l + 1]

    def periodic(P):
        bb = b[:, None] + L[None, :]
        p1 = P[:n - 1].copy(); dgtsv(n - 1, bb, p1)
        p2 = np.zeros((n - 1, P.shape[1])); p2[0] = -a[0]; p2[n - 2] = -c[n - 2]; dgtsv(n - 1, bb, p2)
        pn = (P[n - 1] - c[n - 1] * p1[0] - a[n - 1] * p1[n - 2]) / (bb[n - 1] + c[n - 1] * p2[0] + a[n - 1] * p2[n - 2] + eps)
        out = np.empty_like(P); out[n - 1] = pn; out[:n - 1] = p1 + p2 * pn
        return out

    X = sf.fft2(rhs[1:-1, 1:-1, 1:-1], axes=(0, 1)).reshape(-1, n).T.copy()
    Y = periodic(X.real.copy()) + 1j * periodic(X.imag.copy())
    return sf.ifft2(Y.T.reshape(ng[0], ng[1], n), axes=(0, 1)).real


def perturbed_tgv_rhs(o, case, seed=7):
    """div(u*)/dt of the Taylor-Green field with 2 % noise (what the first pressure solve of the fuzzers' cases sees); returns (pp, u, v, w, p, dt)."""
    from cales_amd.hotpath import initflow
    ng = tuple(int(x) for x in case.ng)
    rng = np.random.RandomState(seed)
    u, v, w, p = initflow(case)
    for x in (u, v, w):
        x[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    o.fillps(1. / dt, u, v, w, pp)
    return pp, u, v, w, p, dt


def oracle_steps(case, nsteps, seed, ulp_seed=None, nthreads=8):
    """`nsteps` steps of the oracle from the perturbed initial field of the fuzzers / test_time_steps (2 % noise, RandomState(seed)); with `ulp_seed` every
    initial velocity value is moved by ONE unit in the last place, random sign. Returns (u, v, w, p, dt)."""
    from cales_amd.hotpath import initflow
    from oracle.oracle import Oracle
    ng = tuple(int(x) for x in case.ng)
    o = Oracle(case, nthreads=nthreads)
    rng = np.random.RandomState(seed)
    u, v, w, p = initflow(case)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    if ulp_seed is not None:
        r2 = np.random.RandomState(ulp_seed)
        for a in (u, v, w):
            a *= 1. + np.finfo(float).eps * (r2.randint(0, 2, size=a.shape) * 2 - 1)
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    for _ in range(nsteps):
        o.step(dt, u, v, w, p, pp, visct)
    o.close()
    return u, v, w, p, dt


def one_ulp_sensitivity(case, nsteps, seed, trials=2):
    """How far the reference algorithm's own result (the oracle's) moves when every initial velocity value moves by one unit in the last place:
    the largest relative change of u, v, w over `trials` random sign patterns. ~1e-15 for well-posed cases."""
    base = oracle_steps(case, nsteps, seed)
    worst = 0.
    for t in range(trials):
        pert = oracle_steps(case, nsteps, seed, ulp_seed=100 + t)
        worst = max(worst, max(relerr(pert[i], base[i]) for i in range(3)))
    return worst, base


def triperiodic_bounds(case, fields, p, dt, nsteps, sens):
    """Per-field bounds (relative to each field's own maximum, as relerr measures) for time steps of a triply periodic box whose pressure the reference
    algorithm returns as C + p' with a round-off-defined constant C (solver.f90:160-178 on a grid whose dzf is not exactly uniform): (1) four times the
    algorithm's own response to one unit in the last place (`sens`, one_ulp_sensitivity); (2) the digits C costs: p' is carried with an absolute error of
    eps |C| that depends on the summation order of the transforms (two CPU evaluations of the same algorithm differ by 2-200 eps |C| per solve,
    tests/test_oracle_solver.py; 100 here), and every one of the 3 nsteps projections moves the velocity by dt grad p'. |C| is taken from the mean of the
    accumulated pressure."""
    eps = np.finfo(float).eps
    C = abs(float(np.asarray(p)[1:-1, 1:-1, 1:-1].mean()))
    dxi = max(float(case.ng[d]) / float(case.l[d]) for d in range(3))
    return [1e-9 + 4. * sens + 100. * eps * C * dt * dxi * 3 * nsteps / max(float(np.abs(f).max()), 1e-300) for f in fields]


def open_case(xset, yset, ng, inflow=True):
    """devchan_nd with other BC pairs: xset / yset = (pair of the normal velocity, pair of the two tangential ones) in x / y, None = periodic; the
    pressure takes the complementary pair of the normal velocity (sanity.f90:140-189), z keeps its walls. Dirichlet faces get non-zero values."""
    g, case = load_golden("devchan_nd")
    case.ng[:] = ng; case.impdiff = 1; case.sgstype = "none"; case.lwm[:] = 0
    case.bcvel[:] = 0.; case.bcpre[:] = 0.
    comp = {"D": "N", "N": "D", "P": "P"}
    for d, pairs in ((0, xset), (1, yset)):
        for iv in range(3):
            pr = "PP" if pairs is None else (pairs[0] if iv == d else pairs[1])
            for side in (0, 1):
                case.cbcvel[side, d, iv] = pr[side]
                if inflow and pr[side] == "D":
                    case.bcvel[side, d, iv] = (0.7, 0.3, -0.2)[iv] * (1. if side == 0 else -0.5)
        prn = "PP" if pairs is None else pairs[0]
        for side in (0, 1):
            case.cbcpre[side, d] = comp[prn[side]]
    case.cbcsgs[:] = np.where(case.cbcvel[:, :, 0] == "P", "P", "D")
    case.is_forced[:] = False; case.bforce[:] = 0.
    return case


OPEN_SETS = [(("DN", "NN"), None, (16, 12, 10)),      # the developing channel: inflow / outflow (RODFT01/10 along u, REDFT10/01 across)
             (("DN", "DN"), None, (24, 8, 12)),       # tangential components Dirichlet at the inflow (RODFT11)
             (("ND", "ND"), None, (16, 12, 10)),      # REDFT10/01 with half-integer eigenvalues along u, REDFT11 across
             (("NN", "DD"), None, (18, 10, 10)),      # REDFT00 along u (2 (n-1)-point extension: 34 = 2 x 17)
             (None, ("DN", "NN"), (12, 16, 10)),      # the same along y
             (None, ("ND", "DN"), (12, 24, 10)),
             (None, ("NN", "ND"), (10, 18, 12)),
             (("DN", "NN"), ("DD", "DD"), (16, 12, 10)),      # inflow / outflow between side walls
             (("DD", "DD"), ("DN", "DN"), (12, 16, 10))]


# ------------------------------------------------------------------ the Helmholtz solve of 3-D implicit diffusion in extended precision
LD = np.longdouble


def helmholtz_pairs(oracle, ivel):
    """BC pairs ("PP", "DN", ...) of velocity component ivel in x, y, z, as the solve sees them (after initbc)"""
    bc = oracle.cbcvel()
    return [str(bc[0, d, ivel - 1]) + str(bc[1, d, ivel - 1]) for d in range(3)]


def helmholtz_unknowns(case, oracle, ivel):
    """points per direction that (1 + alpha L) q = q* solves for: a face that carries a Dirichlet value is no unknown -- the last face of a
    Dirichlet-Dirichlet direction of the component's own (fft.f90:63-143), the top face of w under a Dirichlet wall (solver.f90:49)"""
    nn = [int(x) for x in case.ng]; pr = helmholtz_pairs(oracle, ivel)
    for d in range(2):
        if d == ivel - 1 and pr[d] == "DD":
            nn[d] -= 1
    if ivel == 3 and pr[2][1] == "D":
        nn[2] -= 1
    return nn


def _line_transform(pair, own, n, whole=False):
    """One direction of the solve for a BC pair, across the component (cell-centred) or along it (face-centred), find_fft / eigenvalues of
    fft.f90:192-245 and initsolver.f90:66-98 from their closed forms in extended precision: (forward, backward, eigenvalues per stored mode in
    units of 1/h^2, divisor of the unnormalised pair, the same eigenvalues in the layout of the n-point line the reference stores). The transforms
    are FFTW's unnormalised r2r kinds (scipy's default scaling is the same)."""
    import scipy.fft as sf
    pi = 4 * np.arctan(LD(1))
    lam = lambda theta: -4 * np.sin(theta / 2) ** 2      # -2 (1 - cos theta) without the cancellation
    q = np.arange(n, dtype=LD)
    if pair == "PP" and whole:      # the second direction: its input may be complex (periodic x before it) -- all n wavenumbers; an r2r kind takes real and imaginary part alike
        lm = lam(2 * pi * q / n)
        return (lambda x, ax: sf.fft(x, axis=ax)), (lambda x, ax: sf.ifft(x, axis=ax, norm="forward")), lm, LD(n), lm
    if pair == "PP":      # R2HC / HC2R: modes 0 .. n/2; half-complex slot q holds wavenumber min(q, n - q)
        lm = lam(2 * pi * q[:n // 2 + 1] / n)
        return (lambda x, ax: sf.rfft(x, axis=ax)), (lambda x, ax: sf.irfft(x, n=n, axis=ax, norm="forward")), lm, LD(n), lm[np.minimum(np.arange(n), n - np.arange(n))]
    dct = lambda t: (lambda x, ax: sf.dct(x, type=t, axis=ax))
    dst = lambda t: (lambda x, ax: sf.dst(x, type=t, axis=ax))
    half = lam((2 * q + 1) * pi / (2 * n))
    if not own:
        if pair == "NN": return dct(2), dct(3), lam(q * pi / n), LD(2 * n), lam(q * pi / n)                      # REDFT10 / REDFT01
        if pair == "DD": return dst(2), dst(3), lam((q + 1) * pi / n), LD(2 * n), lam((q + 1) * pi / n)          # RODFT10 / RODFT01
        if pair == "ND": return dct(4), dct(4), half, LD(2 * n), half                                          # REDFT11
        if pair == "DN": return dst(4), dst(4), half, LD(2 * n), half                                          # RODFT11
    else:
        if pair == "NN": return dct(1), dct(1), lam(q * pi / n), LD(2 * (n - 1)), lam(q * pi / n)                # REDFT00 of n points with eigenvalues of period n (the reference's: not an exact inverse)
        if pair == "DD":                                                                                       # RODFT00 of n - 1 points
            lm = lam((q[:n - 1] + 1) * pi / n)
            return dst(1), dst(1), lm, LD(2 * n), np.concatenate([lm, [LD(0)]])
        if pair == "ND": return dct(2), dct(3), half, LD(2 * n), half                                          # REDFT10 / REDFT01 with half-integer eigenvalues (the reference's: not exact)
        if pair == "DN": return dst(3), dst(2), half, LD(2 * n), half                                          # RODFT01 / RODFT10
    raise ValueError(f"no transform for the BC pair {pair!r}")


def helmholtz_reference(case, oracle, ivel, alpha, rhs):
    """(1 + alpha L) q = q* of 3-D implicit diffusion (main.f90:423-491, solver.f90:20-80) for velocity component ivel in np.longdouble (x87 extended
    precision, 64-bit significand), independent of the oracle's transforms and of the library: scipy.fft on longdouble input for the transforms of x and y
    (one per direction, by the component's BC pair and staggering as find_fft defines them), eigenvalues and normalisation from their closed forms, a
    Thomas sweep over all modes at once for z. `rhs` is the haloed r.h.s. AFTER the boundary terms (updt_rhs_b_vel); the return value holds the unknowns
    only (helmholtz_unknowns). It follows the reference's algorithm, the two face-centred sets that are no exact inverses of the discrete operator (NN and
    ND along the component) included. Two things it does not copy: the +eps on every pivot of dgtsv_homebrewed (solver.f90:160-178; the pivots here are
    >= 1, so that is one more rounding of FP64 size, far below any bar this reference is used at) and periodic z, which no case that needs it has.
    The tridiagonal a, b, c are grid data and come from the oracle; its eigenvalues are compared with the closed forms here."""
    pr = helmholtz_pairs(oracle, ivel)
    if pr[2] == "PP":
        raise NotImplementedError("helmholtz_reference: periodic z")
    ng = [int(x) for x in case.ng]; nn = helmholtz_unknowns(case, oracle, ivel); nz = nn[2]
    lam_o, a, b, c, _ = oracle.solver_operands(ivel)
    x = np.array(rhs[1:nn[0] + 1, 1:nn[1] + 1, 1:nz + 1], dtype=LD)
    tr = [_line_transform(pr[d], d == ivel - 1, ng[d], whole=d == 1) for d in range(2)]
    h2i = [(LD(ng[d]) / LD(float(case.l[d]))) ** 2 for d in range(2)]
    full = tr[0][4][:, None] * h2i[0] + tr[1][4][None, :] * h2i[1]
    eps = np.finfo(np.float64).eps
    assert np.abs(full - lam_o).max() <= 8 * eps * np.abs(full).max(), ("eigenvalues", float(np.abs(full - lam_o).max() / np.abs(full).max()))
    x = tr[1][0](tr[0][0](x, 0), 1)
    assert x.dtype in (np.longdouble, np.clongdouble), x.dtype
    alpha = LD(alpha)
    lam = tr[0][2][:, None] * h2i[0] + tr[1][2][None, :] * h2i[1]
    aa = alpha * a[:nz].astype(LD); cc = alpha * c[:nz].astype(LD)
    bb = 1 + alpha * (b[:nz].astype(LD)[None, None, :] + lam[:, :, None])
    d = np.empty(bb.shape, dtype=LD)
    z = 1 / bb[:, :, 0]; d[:, :, 0] = cc[0] * z; x[:, :, 0] = x[:, :, 0] * z
    for l in range(1, nz):
        z = 1 / (bb[:, :, l] - aa[l] * d[:, :, l - 1]); d[:, :, l] = cc[l] * z
        x[:, :, l] = (x[:, :, l] - aa[l] * x[:, :, l - 1]) * z
    for l in range(nz - 2, -1, -1):
        x[:, :, l] = x[:, :, l] - d[:, :, l] * x[:, :, l + 1]
    x = tr[1][1](x, 1)
    if pr[0] != "PP":
        x = x.real      # real x modes: the imaginary part a periodic y left is round-off
    x = tr[0][1](x, 0)
    assert x.dtype == np.longdouble, x.dtype
    return x / (tr[0][3] * tr[1][3])


def helmholtz_exact_kinds(oracle, ivel):
    """whether the component's transform set diagonalises the discrete operator exactly: everything but NN and ND along the component"""
    pr = helmholtz_pairs(oracle, ivel)
    return all(not (d == ivel - 1 and pr[d] in ("NN", "ND")) for d in range(2))


def helmholtz_operator(case, oracle, ivel, alpha, x):
    """(1 + alpha L_h) x on the unknowns, in x's precision: second differences of the staggered component in x and y -- along the component a Dirichlet
    face is 0 and no unknown, a Neumann face mirrors its neighbours; across it the ghost cell is -/+ the first interior value (Dirichlet / Neumann) --
    and the tridiagonal a, b, c of the component in z (initsolver.f90:100-169). For the exact kinds only (helmholtz_exact_kinds)."""
    pr = helmholtz_pairs(oracle, ivel); ng = [int(v) for v in case.ng]
    assert helmholtz_exact_kinds(oracle, ivel)
    _, a, b, c, _ = oracle.solver_operands(ivel)
    T = x.dtype.type
    lap = np.zeros_like(x)
    for d in range(2):
        h2i = (T(ng[d]) / T(float(case.l[d]))) ** 2
        if pr[d] == "PP":
            lap += (np.roll(x, -1, d) - 2 * x + np.roll(x, 1, d)) * h2i
            continue
        e = np.pad(x, [(1, 1) if ax == d else (0, 0) for ax in range(3)])
        at = lambda i: tuple(i if ax == d else slice(None) for ax in range(3))
        if d == ivel - 1:      # faces
            if pr[d][0] == "N": e[at(0)] = e[at(2)]
            if pr[d][1] == "N": e[at(-1)] = e[at(-3)]
        else:                  # cell centres
            e[at(0)] = -e[at(1)] if pr[d][0] == "D" else e[at(1)]
            e[at(-1)] = -e[at(-2)] if pr[d][1] == "D" else e[at(-2)]
        lap += (e[at(slice(2, None))] - 2 * e[at(slice(1, -1))] + e[at(slice(0, -2))]) * h2i
    nz = x.shape[2]
    lz = b[:nz].astype(T)[None, None, :] * x
    lz[:, :, 1:] += a[1:nz].astype(T)[None, None, :] * x[:, :, :-1]
    lz[:, :, :-1] += c[:nz - 1].astype(T)[None, None, :] * x[:, :, 1:]
    return x + T(alpha) * (lap + lz)


# ------------------------------------------------------------------ bulk forcing in y and z, body force (rk.f90:82-86,209-221; mom.f90:311-335)
# is_forced, velf (None: the case's own), bforce. bforce acts only in a direction that is NOT forced -- a forced direction's increment cancels it --, so no
# set has both in one direction.
FORCING_SETS = {"A": ((False, True, False), (None, 0.3, None), (0.7, 0., 0.05)),
                "B": ((True, True, False), (None, 0.3, None), (0., 0., 0.)),
                "C": ((False, True, True), (None, 0.2, -0.15), (0.05, 0., 0.)),
                "D": ((True, True, True), (0.1, 0.2, -0.15), (0., 0., 0.)),
                "E": ((False, False, False), (None, None, None), (1., 0., 0.))}

# case, grid, sets, steps, what cales_describe_plan must say (the path the row is there for), switches of the row
FORCING_STEPS = [
    ("chan_smag", (24, 20, 12), "AB", 3, {"fillps": "own_pass", "bulk_forcing": "in_correction(means_own_pass)"}, {}),
    ("chan_smag", (64, 18, 12), "AB", 2, {"bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    ("chan_dsmag", (64, 20, 12), "AB", 2, {"projection": "in_strain_rate_pass", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    ("chan_dsmag", (128, 12, 20), "B", 2, {"projection": "in_strain_rate_pass", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),      # two x tiles, several k chunks
    ("chan_nosgs_x64", (64, 24, 16), "AB", 2, {"projection": "in_next_momentum_pass(substeps_1_2)", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    # (the increment rides in the pending projection over the step boundary)
    ("chan_nosgs_x64", (64, 24, 16), "AB", 3, {"projection": "in_next_momentum_pass(all_substeps)", "bulk_forcing": "in_correction(means_in_x_transform)"}, {"CALES_LAZY_PROJECTION": "1"}),
    ("chan_smag_wm", (32, 16, 16), "B", 3, {"first_wall_model_update": "skipped", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    ("chan_smag_wm", (32, 16, 8), "A", 3, {"first_wall_model_update": "skipped", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    # the first wall-model update kept, hence the forcing as a pass of its own before it. A sampling height inside the first cell would do that, but
    # cales_check_case refuses every such case (sanity.f90:224-231: hwm above the first cell centre), as it does at this grid's zc(1) = 0.057 < hwm = 0.1;
    # of make_plan's conditions only the reference's full ghost-cell sequence is left to reach the fragment
    ("chan_smag_wm", (32, 16, 8), "A", 3, {"first_wall_model_update": "kept", "bulk_forcing": "own_pass"}, {"CALES_UNMERGED_BC": "1"}),
    ("chan_dsmag_wm", (64, 16, 12), "B", 2, {"sgs": "dsmag_tiles*", "first_wall_model_update": "*"}, {}),      # ("*": any value that starts so)
    ("halfchan_imp1d", (16, 16, 16), "AB", 3, {"bulk_forcing": "in_helmholtz_sweep", "implicit_rhs": "in_helmholtz_sweep"}, {}),
    ("halfchan_imp1d", (16, 16, 16), "AB", 3, {"bulk_forcing": "own_pass", "implicit_rhs": "own_pass"}, {"CALES_UNFUSED_IMP_RHS": "1"}),
    ("couette_imp3d_ops", (16, 16, 16), "AB", 3, {"bulk_forcing": "own_pass"}, {}),
    # periodic z: w weighted with the cell-centre weights (three steps at the 64-cell rows for the reason given below)
    ("tgv_ppp", (32, 24, 16), "CD", 3, {"projection": "in_next_momentum_pass(substeps_1_2)", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    ("tgv_ppp", (64, 16, 16), "CD", 3, {"projection": "in_next_momentum_pass(substeps_1_2)", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    # the strain-rate fold with the increments of v and w, of u, v and w (three steps: the body force of set C moves u by bforce x elapsed time, 1e-2 of
    # its maximum after two steps of these grids and 1.4e-2 after three)
    ("tgv_dsmag_ppp", (64, 16, 24), "CD", 3, {"projection": "in_strain_rate_pass", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    ("tgv_dsmag_ppp", (64, 16, 32), "CD", 3, {"projection": "in_strain_rate_pass", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}),
    # body force only, nothing forced
    ("duct_smag_wm", (16, 24, 24), "E", 3, {"bulk_forcing": "none"}, {}),
    ("duct_dsmag", (64, 18, 20), "E", 2, {"bulk_forcing": "none"}, {}),
] + [
    # sets A and B through the forms behind the switches, at the 64-cell rows
    (name, ng, "AB", 2, expect, {env: "1"})
    for name, ng in (("chan_smag", (64, 18, 12)), ("chan_dsmag", (64, 20, 12)))
    for env, expect in (("CALES_UNFUSED_FORCING", {"bulk_forcing": "own_pass"}), ("CALES_UNFUSED_MEAN", {"bulk_forcing": "in_correction(means_own_pass)"}),
                        ("CALES_UNFOLDED_CORREC", {"projection": "own_pass(correc+updatep)"}), ("CALES_UNFOLDED_MOM", {"projection": "own_pass(correc+updatep)" if name == "chan_smag" else "in_strain_rate_pass"}),
                        ("CALES_UNFUSED_CORREC", {"projection": "own_passes", "bulk_forcing": "own_pass"}), ("CALES_XGHOSTS_IN_STEP", {"x_ghost_columns": "maintained"}))]
FORCING_STEP_PARAMS = [(name, ng, s, nsteps, expect, env) for name, ng, sets, nsteps, expect, env in FORCING_STEPS for s in sets]


def forcing_id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


FORCING_STEP_IDS = ["-".join([name, forcing_id(ng), s] + [k[6:] for k in env]) for name, ng, s, _, _, env in FORCING_STEP_PARAMS]


def forced_case(name, ng, fset):
    """golden case `name` on the grid `ng` with the forcing set `fset` of FORCING_SETS"""
    g, case = load_golden(name)
    case.ng[:] = ng
    is_forced, velf, bforce = FORCING_SETS[fset]
    case.is_forced[:] = is_forced
    for d in range(3):
        if velf[d] is not None:
            case.velf[d] = velf[d]
    case.bforce[:] = bforce
    return case


def perturbed_start(case, o, seed=1):
    """initflow plus 2 % noise, the start-up of main.f90:370-375 on the oracle `o`, dt = half the bound of chkdt; returns (u, v, w, p, visct, pp, dt) and a raw copy of u, v, w, p"""
    from cales_amd.hotpath import initflow
    ng = tuple(int(x) for x in case.ng)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(seed)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    raw = [a.copy(order="F") for a in (u, v, w, p)]
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    return (u, v, w, p, visct, pp, dt), raw


def oracle_forcing_of_substeps(o, case, dt, u, v, w, p, pp, visct, stale=None, dt_stale=None):
    """One step of the oracle operator by operator (the sequence of o_step, main.f90:417-508), on the caller's arrays; returns the forcing f of every substep.
    `stale` names ONE factor that is taken from the time step `dt_stale` instead (STALE_FACTORS: the mistakes a step that carries dt-dependent state over
    a step boundary can make; tests/test_variable_dt_oracle.py measures what each costs)."""
    assert stale is None or (stale in STALE_FACTORS and dt_stale is not None)
    fs = []
    for irk in (1, 2, 3):
        dtrk = (RK[irk - 1][0] + RK[irk - 1][1]) * dt; alpha = 0.
        dtrk_stale = (RK[irk - 1][0] + RK[irk - 1][1]) * dt_stale if stale else None
        f = o.rk(irk, dt_stale if (stale == "dt_of_rk_1" and irk == 1) else dt, p, visct, u, v, w); fs.append(f.copy())
        o.bulk_forcing(f, u, v, w)
        if case.impdiff:
            alpha = -.5 * case.visc * dtrk
            for iv, q in ((1, u), (2, v), (3, w)):
                if case.impdiff == 2:
                    o.updt_rhs_b_velz(iv, alpha, q); o.solver_gaussel_z(iv, alpha, q)
                else:
                    o.updt_rhs_b_vel(iv, alpha, q); o.solver_helmholtz(iv, alpha, q)
        o.bounduvw(u, v, w, True, False)
        o.fillps(1. / (dtrk_stale if (stale == "dtrki_of_fillps_1" and irk == 1) else dtrk), u, v, w, pp); o.updt_rhs_b_p(pp); o.solver(pp); o.boundp(pp, 0)
        o.correc(dtrk_stale if (stale == "dtrk_of_correc_3" and irk == 3) else dtrk, pp, u, v, w); o.bounduvw(u, v, w, True, True)
        o.updatep(alpha, pp, p); o.boundp(p, 0)
        o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    return fs


# ------------------------------------------------------------------ whole steps under a time step that changes at every step (main.f90:395-416: dt = min(cfl dtmax, dt_f) anew per icheck block)
# the factors on dt0 = half the bound of chkdt at the start: five different steps in seven, none above dt0
DT_FACTORS = (1., 0.7, 1., 0.5, 0.9, 0.7, 0.6)
STALE_FACTORS = ("dtrk_of_correc_3", "dt_of_rk_1", "dtrki_of_fillps_1")

_LAZY = {"CALES_LAZY_PROJECTION": "1"}
_MOM12, _MOM123, _STRAIN = "in_next_momentum_pass(substeps_1_2)", "in_next_momentum_pass(all_substeps)", "in_strain_rate_pass"
_OWN = "own_pass(correc+updatep)"
# case, grid, forcing set of FORCING_SETS (None: the case's own), edits of the Case, what cales_describe_plan must say (the path the row is there for; "*": any
# value that starts so), switches, the values of `reads` (both wherever the projection of a substep is applied by a later pass)
VARIABLE_DT_ROWS = [
    ("chan_nosgs_x64", (64, 24, 16), "B", {}, {"projection": _MOM12}, {}, (False, True)),
    ("chan_nosgs_x64", (64, 24, 16), "B", {}, {"projection": _MOM123}, _LAZY, (False, True)),
    ("chan_nosgs_x64", (64, 24, 16), "A", {}, {"projection": _MOM123}, _LAZY, (False, True)),      # the body force
    ("tgv_ppp", (32, 24, 16), "D", {}, {"projection": _MOM12}, {}, (False, True)),
    ("tgv_ppp", (32, 24, 16), "D", {}, {"projection": _MOM123}, _LAZY, (False, True)),
    ("tgv_ppp", (64, 16, 16), "D", {}, {"projection": _MOM12}, {}, (False, True)),
    ("tgv_ppp", (64, 16, 16), "D", {}, {"projection": _MOM123}, _LAZY, (False, True)),
    ("cavity_nnn", (16, 16, 16), None, {}, {"projection": _MOM12, "x_ghost_columns": "maintained"}, {}, (False, True)),      # walls in x
    ("cavity_nnn", (16, 16, 16), None, {}, {"projection": _MOM123, "x_ghost_columns": "maintained"}, _LAZY, (False, True)),
    # the projection inside the strain-rate pass: five |S|Sij fields (the default), six, two x tiles, periodic z, the local coefficient
    ("chan_dsmag", (64, 20, 12), "B", {}, {"projection": _STRAIN, "sgs": "dsmag_tiles(pair_fields)"}, {}, (False, True)),
    ("chan_dsmag", (64, 20, 12), "B", {}, {"projection": _STRAIN, "sgs": "dsmag_tiles(pair_fields)"}, {"CALES_SGS_SIX_COMPONENTS": "1"}, (False, True)),
    ("chan_dsmag", (128, 12, 20), "B", {}, {"projection": _STRAIN, "sgs": "dsmag_tiles(pair_fields)"}, {}, (False, True)),
    ("tgv_dsmag_ppp", (64, 16, 24), "D", {}, {"projection": _STRAIN}, {}, (False, True)),
    ("chan_dsmag", (64, 20, 12), "B", {"dsmag_average": "local"}, {"projection": _STRAIN, "sgs_average": "local"}, {}, (False, True)),
    # tiles without the fold
    ("chan_dsmag", (32, 16, 16), "B", {}, {"projection": _OWN, "sgs": "dsmag_tiles*"}, {}, (True,)),
    ("chan_dsmag", (80, 20, 12), "B", {}, {"projection": _OWN, "sgs": "dsmag_tiles*"}, {}, (True,)),
    # fillps as a pass of its own / inside the x transform
    ("chan_smag", (24, 20, 12), "B", {}, {"fillps": "own_pass", "projection": _OWN}, {}, (True,)),
    ("chan_smag", (64, 18, 12), "B", {}, {"fillps": "in_x_transform", "projection": _OWN}, {}, (True,)),
    ("chan_smag_wm", (32, 16, 16), "B", {}, {"first_wall_model_update": "skipped", "bulk_forcing": "in_correction(means_in_x_transform)"}, {}, (True,)),
    # further classes (wall model with the dynamic model, ducts, a cavity with the model, inflow / outflow): the plan as it stands
    ("chan_dsmag_wm", (64, 16, 12), "B", {}, {"projection": _OWN, "x_ghost_columns": "maintained", "first_wall_model_update": "skipped", "bulk_forcing": "in_correction(means_in_x_transform)",
                                              "sgs": "dsmag_tiles(pair_fields)"}, {}, (True,)),
    ("duct_dsmag", (64, 18, 20), None, {}, {"projection": _OWN, "x_ghost_columns": "wrapped", "bulk_forcing": "in_correction(means_in_x_transform)", "sgs": "dsmag_tiles"}, {}, (True,)),
    ("duct_smag_wm", (16, 24, 24), None, {}, {"projection": _OWN, "fillps": "own_pass", "first_wall_model_update": "skipped", "bulk_forcing": "in_correction(means_own_pass)", "sgs": "smag_rows"}, {}, (True,)),
    ("cavity_dsmag", (16, 16, 12), None, {}, {"projection": _OWN, "fillps": "own_pass", "bulk_forcing": "none", "sgs": "dsmag_reference_sequence"}, {}, (True,)),
    ("devchan_nd", (32, 16, 16), None, {}, {"projection": _OWN, "x_ghost_columns": "maintained", "fillps": "own_pass", "bulk_forcing": "none", "sgs": "none"}, {}, (True,)),
    ("couette_imp3d_ops", (16, 16, 16), None, {}, {"projection": "own_passes", "helmholtz_u": "*", "helmholtz_v": "*", "helmholtz_w": "*"}, {}, (True,)),      # 3-D implicit diffusion: a new alpha every step
] + [
    # the forms behind the switches, one at a time
    (name, ng, "B", {}, expect, {env: "1"}, (False, True))
    for name, ng in (("chan_smag", (64, 18, 12)), ("chan_dsmag", (64, 20, 12)))
    for env, expect in (("CALES_UNFUSED_CORREC", {"projection": "own_passes", "bulk_forcing": "own_pass"}), ("CALES_UNFOLDED_CORREC", {"projection": _OWN}),
                        ("CALES_UNFOLDED_MOM", {"projection": _OWN if name == "chan_smag" else _STRAIN}), ("CALES_UNFUSED_FORCING", {"bulk_forcing": "own_pass"}),
                        ("CALES_XGHOSTS_IN_STEP", {"x_ghost_columns": "maintained"}), ("CALES_EAGER_PROJECTION", {"projection": _OWN if name == "chan_smag" else _STRAIN}))]
VARIABLE_DT_PARAMS = [(name, ng, fset, edits, expect, env, r) for name, ng, fset, edits, expect, env, reads in VARIABLE_DT_ROWS for r in reads]
VARIABLE_DT_IDS = ["-".join([name, forcing_id(ng), str(fset)] + list(edits.values()) + [k[6:] for k in env] + ["reads" if r else "no_reads"])
                   for name, ng, fset, edits, expect, env, r in VARIABLE_DT_PARAMS]
# the grids of the switch combinations (tests/test_gpu_variable_dt.py, through test_time_steps: the case's own forcing)
VARIABLE_DT_COMBINATION_GRIDS = [("chan_dsmag", (32, 16, 16)), ("chan_smag_wm", (32, 16, 12)), ("chan_smag", (64, 12, 10))]


def variable_dt_case(name, ng, fset, edits):
    if fset is not None:
        case = forced_case(name, ng, fset)
    else:
        g, case = load_golden(name); case.ng[:] = ng
    for k, v in edits.items():
        setattr(case, k, v)
    return case


def last_forcing(h):
    """f(1:3) of the last substep on the device (cales_get_forcing)"""
    import ctypes as C
    f = np.zeros(3)
    h._chk(h.L.cales_get_forcing(h.h, f.ctypes.data_as(C.c_void_p)))
    return f


def steps_under_schedule(case, o, h, reads, factors=DT_FACTORS, hook=None, tag=""):
    """Oracle `o` and device `h` together through the steps dt_n = factors[n] * dt0 from perturbed_start, dt0 from the ORACLE (the device's chkdt is a
    quantity under test). Between two steps: nothing (`reads` False: whatever the step left to its successor crosses the boundary to a step with another
    dt) or the block of the production loop (main.f90:395-416 with the outputs of its 0-D file): chkdt, chkdiv, dpdl and the forcing of the last substep,
    each held to the oracle's value for THAT step -- chkdt 1e-7 relative (the loosest bar among its inputs, visct), divmax < 20 x oracle + 1e-14, dpdl and
    the forcing 1e-9 max(1, |.|). After the last step the block runs either way. `hook(n, 'started' | 'stepped' | 'read')` is called after the start-up (n = -1: the plan of the steps
    is known from here on), after step n and after its block.
    The oracle steps operator by operator (oracle_forcing_of_substeps; tests/test_variable_dt_oracle.py: bit for bit o.step, whose dpdl is -sum(f) / dt_n).
    Returns the oracle's (u, v, w, p, visct), dt0 and the largest measured error of every read, each in units of its bar's scale."""
    (u, v, w, p, visct, pp, dt0), raw = perturbed_start(case, o)
    h.upload(*raw); h.startup()
    if hook: hook(-1, "started")
    worst = {"chkdt": abs(h.chkdt() / (2. * dt0) - 1.), "dpdl": 0., "forcing": 0., "div": None}
    assert worst["chkdt"] < 1e-7, (tag, "chkdt at the start", worst["chkdt"])
    for n, fac in enumerate(factors):
        dtn = fac * dt0
        h.step(dtn)
        fs = oracle_forcing_of_substeps(o, case, dtn, u, v, w, p, pp, visct)
        if hook: hook(n, "stepped")
        if not (reads or n == len(factors) - 1):
            continue
        e = abs(h.chkdt() / o.chkdt(visct, u, v, w) - 1.)
        dg, do = h.chkdiv()[1], o.chkdiv(u, v, w)[1]
        dpdl = -sum(fs) / dtn
        hd, hf = h.dpdl(), last_forcing(h)
        ed = np.abs(hd - dpdl).max() / max(1., np.abs(dpdl).max()); ef = np.abs(hf - fs[2]).max() / max(1., np.abs(fs[2]).max())
        print(tag, "step", n, "dt/dt0", fac, "chkdt", e, "divmax", dg, do, "dpdl", hd, dpdl, ed, "f", hf, fs[2], ef)
        assert e < 1e-7, (tag, n, "chkdt", e)
        assert dg < 20. * do + 1e-14, (tag, n, "divmax", dg, do)
        assert ed < 1e-9, (tag, n, "dpdl", hd, dpdl)
        assert ef < 1e-9, (tag, n, "forcing", hf, fs[2])
        worst["chkdt"] = max(worst["chkdt"], e); worst["dpdl"] = max(worst["dpdl"], ed); worst["forcing"] = max(worst["forcing"], ef)
        if worst["div"] is None or dg / (20. * do + 1e-14) > worst["div"][0] / (20. * worst["div"][1] + 1e-14): worst["div"] = (dg, do)
        if hook: hook(n, "read")
    return (u, v, w, p, visct), dt0, worst
