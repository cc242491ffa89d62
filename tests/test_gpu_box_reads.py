"""include/cales_post.h on the device: cales_read_box, cales_out2d, cales_out3d (k_box_read) by value against numpy slicing of what was uploaded, and
held to the rules every field-reading entry of the C-ABI keeps -- the lazy eddy viscosity is materialised, stale x ghost columns are refreshed, a pending
projection is completed, nothing is allocated, a refused call leaves the context usable --, on one rank, on y-slabs, in single precision and from the
Fortran host.

The test fields are integer-coded, a[i,j,k] = i + 128 j + 2048 k (+ an offset per field): exact in float and double, so a wrong index is a wrong value."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.util import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(96, 12, 10),      # rows of more than one 64-lane wave: boxes cross the seam
         (40, 12, 10)]      # row pitch 48 != n1 + 2
FIELD_OFFSET = {"u": 0., "p": 100000., "dudt": -50000.}


def coded(ng, offset=0.):
    i, j, k = np.meshgrid(*[np.arange(n + 2, dtype=np.float64) for n in ng], indexing="ij")
    return np.asfortranarray(i + 128. * j + 2048. * k + offset)


def box_of(a, lo, hi, ns):
    return a[tuple(slice(l, h + 1, s) for l, h, s in zip(lo, hi, ns))]


def nosgs_channel(ng):
    """explicit channel without subgrid model"""
    g, case = load_golden("chan_smag")
    case.ng[:] = ng; case.sgstype = "none"
    return case


@pytest.fixture(scope="module", params=GRIDS, ids=lambda ng: "x".join(map(str, ng)))
def loaded(request):
    """a context with the coded fields u, p and dudt uploaded; reads change nothing, so the tests share it"""
    from cales_amd.hotpath import HotPath
    ng = request.param
    h = HotPath(nosgs_channel(ng))
    ref = {name: coded(ng, off) for name, off in FIELD_OFFSET.items()}
    for name, a in ref.items():
        h.set(name, a)
    yield h, ng, ref
    h.close()


def same(got, want):
    assert got.flags.f_contiguous and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(FIELD_OFFSET))
def test_boxes_by_value(loaded, name):
    h, ng, ref = loaded
    a = ref[name]
    top = tuple(n + 1 for n in ng)
    same(h.read_box(name, (0, 0, 0), top), a)                                   # the whole haloed field
    same(h.read_box(name, (1, 1, 1), ng), a[1:-1, 1:-1, 1:-1])                  # the interior
    for c in np.ndindex(2, 2, 2):                                               # each corner cell alone
        p = tuple(t * q for t, q in zip(top, c))
        same(h.read_box(name, p, p), a[p].reshape(1, 1, 1))
    rng = np.random.RandomState(5)
    for _ in range(50):                                                          # random strided boxes
        lo = [int(rng.randint(0, t + 1)) for t in top]
        hi = [int(rng.randint(l, t + 1)) for l, t in zip(lo, top)]
        ns = [int(rng.choice([1, 1, 2, 3, 7, 65])) for _ in range(3)]
        same(h.read_box(name, lo, hi, ns), box_of(a, lo, hi, ns))


@pytest.mark.parametrize("name", list(FIELD_OFFSET))
def test_out2d_and_out3d_by_value(loaded, name):
    h, ng, ref = loaded
    a = ref[name]
    for inorm in (1, 2, 3):
        for islice in (1, ng[inorm - 1] // 2, ng[inorm - 1]):
            sl = [slice(1, -1)] * 3; sl[inorm - 1] = slice(islice, islice + 1)
            same(h.out2d(name, inorm, islice), a[tuple(sl)])
    for ns in ((1, 1, 1), (2, 3, 4), (7, 1, 1), (1, 5, 1), (200, 200, 200)):
        same(h.out3d(name, ns), a[1:-1:ns[0], 1:-1:ns[1], 1:-1:ns[2]])
    assert h.out3d(name, (200, 200, 200)).shape == (1, 1, 1)


def test_reads_have_a_profile_scope_and_allocate_nothing(loaded):
    h, ng, ref = loaded
    before = h.memory_in_use()
    h.profile_reset(); h.profile(True)
    for q in range(5):
        h.read_box("u", (0, q, 0), (ng[0] + 1, ng[1] + 1, ng[2]), (1 + q, 1, 2))
        h.out2d("p", 1 + q % 3, 1 + q)
        h.out3d("dudt", (1 + q, 2, 1))
        h.read_box("p", (q, q, q), (q, q, q))
    h.profile(False)
    assert h.profile_stats()["box_read"][0] == 20      # one launch per read, under a scope of its own
    assert h.memory_in_use() == before


def test_refusals_leave_the_context_usable(loaded):
    from cales_amd import capi
    h, ng, ref = loaded
    L, H = h.L, h.h
    i3 = lambda v: (C.c_int32 * 3)(*v)
    buf = np.zeros(tuple(n + 2 for n in ng), order="F", dtype=capi.np_real)
    P, cnt = buf.ctypes.data_as(C.c_void_p), i3((0, 0, 0))
    U = capi.FIELDS["u"]
    one, top = (1, 1, 1), tuple(n + 1 for n in ng)
    refused = {
        "nskip < 1": lambda: L.cales_read_box(H, U, i3(one), i3(ng), i3((1, 1, 0)), P, cnt),
        "nskip < 1 (out3d)": lambda: L.cales_out3d(H, U, i3((0, 1, 1)), P, cnt),
        "lo < 0": lambda: L.cales_read_box(H, U, i3((-1, 1, 1)), i3(ng), i3(one), P, cnt),
        "hi > ng+1": lambda: L.cales_read_box(H, U, i3(one), i3((ng[0], ng[1] + 2, ng[2])), i3(one), P, cnt),
        "lo > hi": lambda: L.cales_read_box(H, U, i3((1, 1, 5)), i3((ng[0], ng[1], 4)), i3(one), P, cnt),
        "islice = 0": lambda: L.cales_out2d(H, U, 2, 0, P, cnt),
        "islice = ng+1": lambda: L.cales_out2d(H, U, 3, ng[2] + 1, P, cnt),
        "inorm = 0": lambda: L.cales_out2d(H, U, 0, 1, P, cnt),
        "inorm = 4": lambda: L.cales_out2d(H, U, 4, 1, P, cnt),
        "field -1": lambda: L.cales_read_box(H, -1, i3(one), i3(ng), i3(one), P, cnt),
        "field 15": lambda: L.cales_out3d(H, 15, i3(one), P, cnt),
        "field not allocated": lambda: L.cales_out2d(H, capi.FIELDS["dudtd"], 1, 1, P, cnt),      # (explicit diffusion: no implicit part)
        "NULL buf": lambda: L.cales_read_box(H, U, i3(one), i3(ng), i3(one), None, cnt),
    }
    valid = [((0, 0, 0), top, (1, 1, 1)), ((3, 2, 1), (ng[0], 9, 8), (5, 2, 3))]
    for q, (what, call) in enumerate(refused.items()):
        assert call() != 0, what
        assert L.cales_last_error(H).decode(), what
        lo, hi, ns = valid[q % 2]
        same(h.read_box("u", lo, hi, ns), box_of(ref["u"], lo, hi, ns))
    from cales_amd.hotpath import CalesError
    for bad in (lambda: h.out2d("u", 2, 0), lambda: h.out2d("u", 5, 1), lambda: h.out3d("u", (1, 0, 1)), lambda: h.read_box("u", (2, 2, 2), (1, 2, 2))):
        with pytest.raises(CalesError):
            bad()
    # an empty buffer is no error where nothing is to be written -- a NULL buf with an EMPTY share cannot occur on one rank (see the slab test)
    same(h.out2d("u", 2, ng[1]), ref["u"][1:-1, ng[1]:ng[1] + 1, 1:-1])


def test_every_entry_refuses_a_field_id_the_context_cannot_resolve():
    """Every entry of the C-ABI that takes a field id -- the four headers' -- resolves it through the one host-side check (field_ptr, api.hip) before
    it launches anything: an id out of range (-1, CALES_NFIELDS) and dudtd, which a context with explicit diffusion did not allocate, are refused
    with "<entry>: bad field id", nothing is allocated, no profile scope opens, and the context goes on to give the values numpy gives."""
    from cales_amd import capi
    from cales_amd.hotpath import HotPath
    from tests.test_pdf_host import pdf_ref
    ng = SLAB_NG      # the smallest explicit case of this file
    h = HotPath(nosgs_channel(ng))
    a = coded(ng); h.set("u", a)
    L, H = h.L, h.h
    i3 = lambda v: (C.c_int32 * 3)(*v)
    buf = np.zeros(tuple(n + 2 for n in ng), order="F", dtype=capi.np_real)      # room for the reals of every entry below
    ints = np.zeros(8 * 8 * 2 + 8 * ng[2] + 2 * ng[2], dtype=np.int64)
    kp = np.asarray([2, 1], dtype=np.int32)
    P, PC, PO, K = buf.ctypes.data_as(C.c_void_p), ints.ctypes.data_as(C.c_void_p), ints[128 + 8 * ng[2]:].ctypes.data_as(C.c_void_p), kp.ctypes.data_as(C.c_void_p)
    U, cnt, mean = capi.FIELDS["u"], i3((0, 0, 0)), capi.c_real(0.)
    entries = {
        "cales_get_field": lambda f: L.cales_get_field(H, f, P),
        "cales_set_field": lambda f: L.cales_set_field(H, f, P),
        "cales_read_box": lambda f: L.cales_read_box(H, f, i3((1, 1, 1)), i3(ng), i3((1, 1, 1)), P, cnt),
        "cales_boundp": lambda f: L.cales_boundp(H, f, 0),
        "cales_bulk_mean": lambda f: L.cales_bulk_mean(H, f, 1, C.byref(mean)),
        "cales_out1d": lambda f: L.cales_out1d(H, f, 3, 0, P),
        "cales_pdf_planes": lambda f: L.cales_pdf_planes(H, f, 8, 0., 1., PC, PO),
        "cales_jpdf_planes": lambda f: L.cales_jpdf_planes(H, f, U, 8, 0., 1., 0., 1., 2, K, PC, PO),
        "cales_jpdf_planes (second field)": lambda f: L.cales_jpdf_planes(H, U, f, 8, 0., 1., 0., 1., 2, K, PC, PO),
        "cales_spectra_lines": lambda f: L.cales_spectra_lines(H, f, 1, P, None),
        "cales_spectra_planes": lambda f: L.cales_spectra_planes(H, f, 2, K, P),
    }
    assert capi.FIELDS["dudtd"] < len(capi.FIELDS) == 15
    before = h.memory_in_use()
    h.profile_reset(); h.profile(True)
    for entry, call in entries.items():
        for f in (capi.FIELDS["dudtd"], -1, len(capi.FIELDS)):
            assert call(f) != 0, (entry, f)
            assert L.cales_last_error(H).decode() == entry.split(" ")[0] + ": bad field id", (entry, f, L.cales_last_error(H))
            assert h.memory_in_use() == before, (entry, f)
    h.profile(False)
    assert all(v[0] == 0 for v in h.profile_stats().values()), h.profile_stats()
    assert not buf.any() and not ints.any()
    # the context is as usable as before, and set_field has written nothing
    prof = h.out1d("u", 3)
    want = a[1:-1, 1:-1, 1:-1].mean(axis=(0, 1))      # (sums of integers: exact; the rounding is that of the grid ratio and the product)
    assert np.abs(prof - want).max() <= 8 * np.finfo(capi.np_real).eps * np.abs(want).max()
    counts, outside = h.pdf_planes("u", 64, 3000., 3000. + 64 * 256)
    wc, wo = pdf_ref(np.asarray(a[1:-1, 1:-1, 1:-1], dtype=capi.np_real), 64, 3000., 3000. + 64 * 256)
    assert np.array_equal(counts, wc) and np.array_equal(outside, wo) and counts.sum() > 0
    assert h.memory_in_use() == before
    h.close()


@pytest.mark.parametrize("read_first", [False, True], ids=["get_first", "read_first"])
def test_visct_is_materialised(read_first):
    """The dynamic model's tile passes leave visct = |S| cs(k) as |S| and the plane coefficients until somebody other than the momentum pass reads it:
    a plane read is such a reader, whether it comes before or after a full download."""
    from cales_amd.hotpath import HotPath, initflow
    g, case = load_golden("chan_dsmag"); case.ng[:] = (64, 16, 12)
    u0 = initflow(case)
    rng = np.random.RandomState(3)
    for a in u0[:3]:
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(64, 16, 12) - 0.5)
    h = HotPath(case); h.upload(*u0); h.startup()
    h.cmpt_sgs()
    if read_first:
        planes = [h.out2d("visct", inorm, s) for inorm, s in ((1, 7), (2, 8), (3, 5))]
        full = h.get("visct")
    else:
        full = h.get("visct"); h.cmpt_sgs()
        planes = [h.out2d("visct", inorm, s) for inorm, s in ((1, 7), (2, 8), (3, 5))]
    h.close()
    assert full[1:-1, 1:-1, 1:-1].max() > 0.
    same(planes[0], full[7:8, 1:-1, 1:-1]); same(planes[1], full[1:-1, 8:9, 1:-1]); same(planes[2], full[1:-1, 1:-1, 5:6])


def test_first_reader_of_stale_x_ghost_columns(monkeypatch):
    """The scheme of tests/test_gpu_golden.py::test_x_ghost_columns_are_refreshed_for_the_first_reader with read_box as the first entry after the steps,
    on a box that holds i = 0 and i = n1+1: the same bits as the eager form, in the box and in everything read after it."""
    from cales_amd.hotpath import HotPath, initflow
    ng = (64, 16, 12)
    g, case = load_golden("chan_dsmag"); case.ng[:] = ng
    u0 = initflow(case)
    rng = np.random.RandomState(2)
    for a in u0[:3]:
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)

    def run():
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.4 * h.chkdt()
        for _ in range(3):
            h.step(dt)
        box = h.read_box("w", (0, 0, 0), (ng[0] + 1, ng[1] + 1, ng[2] + 1), (1, 3, 2))
        out = [box] + h.download() + [np.asarray(h.chkdt()), np.asarray(h.chkdiv())]
        h.close()
        return out
    lazy = run()
    monkeypatch.setenv("CALES_EAGER_PROJECTION", "1")
    eager = run()
    assert np.abs(lazy[0][0]).max() > 0. and np.array_equal(lazy[0][0], lazy[0][-2])      # (periodic x: column 0 is column n1)
    for q, (a, b) in enumerate(zip(lazy, eager)):
        assert np.array_equal(a, b), q
    same(lazy[0], lazy[3][0::1, 0::3, 0::2])


def post_ctx_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cales_post.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(\s*(?:const\s+)?cales_ctx\s*\*", hdr)))


def test_every_post_entry_sees_the_projected_state(monkeypatch):
    """The scheme of tests/test_gpu_golden.py::test_every_entry_sees_the_projected_state for the second header: every entry of include/cales_post.h that
    takes a context, enumerated from the header, completes a projection that cales_step left pending before it reads."""
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initflow
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    g, case = load_golden("cavity_nnn"); case.ng[:] = (32, 16, 12)
    entries = post_ctx_entries()
    i3 = lambda v: (C.c_int32 * 3)(*v)
    buf = np.zeros((34, 18, 14), order="F", dtype=capi.np_real)
    P, cnt = buf.ctypes.data_as(C.c_void_p), i3((0, 0, 0))
    U = capi.FIELDS["u"]
    table = {"cales_read_box": lambda h: h.L.cales_read_box(h.h, U, i3((0, 0, 0)), i3((33, 17, 13)), i3((1, 1, 1)), P, cnt),
             "cales_out2d": lambda h: h.L.cales_out2d(h.h, U, 2, 8, P, cnt),
             "cales_out3d": lambda h: h.L.cales_out3d(h.h, U, i3((2, 2, 2)), P, cnt)}
    assert entries and sorted(table) == entries, f"entries of include/cales_post.h without a rule for a pending projection: {set(entries) ^ set(table)}"
    u0 = initflow(case)
    for e in entries:
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.5 * h.chkdt()
        ncorr = lambda: sum(h.profile_stats().get(k, (0, 0.))[0] for k in ("correc_updatep", "correc"))
        h.profile(True)
        h.step(dt)
        assert ncorr() == 0, (e, "the step was expected to leave its last projection pending")
        assert table[e](h) == 0, (e, h.L.cales_last_error(h.h))
        n1 = ncorr()
        assert n1 >= 1, (e, "did not complete the pending projection")
        assert h.chkdiv()[1] < 1e-12, e      # what the entry saw was the projected velocity
        assert ncorr() == n1, e              # ... and nothing was pending any more
        h.profile(False); h.close()


SLAB_NG = (32, 12, 10)
SLAB_READS = [("read_box", ((0, 0, 0), (33, 13, 11), (1, 1, 1))),       # rows 0 and ng2+1
              ("read_box", ((2, 0, 1), (30, 13, 9), (3, 13, 2))),        # ... alone: the ranks in the middle hold nothing
              ("read_box", ((1, 5, 1), (32, 6, 10), (1, 1, 1))),         # two rows: empty on most ranks
              ("read_box", ((5, 2, 3), (5, 11, 3), (1, 2, 1))),
              ("out2d", (1, 16)), ("out2d", (2, 7)), ("out2d", (2, 12)), ("out2d", (3, 10)),
              ("out3d", ((2, 5, 3),)), ("out3d", ((1, 1, 1),))]


def _slab_box(kind, args):
    if kind == "read_box":
        return args
    if kind == "out3d":
        return (1, 1, 1), SLAB_NG, args[0]
    lo, hi = [1, 1, 1], list(SLAB_NG)
    lo[args[0] - 1] = hi[args[0] - 1] = args[1]
    return tuple(lo), tuple(hi), (1, 1, 1)


@pytest.fixture(scope="module")
def one_rank_reads():
    from cales_amd.hotpath import HotPath
    a = coded(SLAB_NG)
    h = HotPath(nosgs_channel(SLAB_NG)); h.set("u", a)
    out = [getattr(h, kind)("u", *args) for kind, args in SLAB_READS]
    h.close()
    for (kind, args), got in zip(SLAB_READS, out):
        same(got, box_of(a, *_slab_box(kind, args)))
    return out


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_slab_shares_make_the_one_rank_result(nranks, one_rank_reads):
    from cales_amd import capi
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import box_share
    case = nosgs_channel(SLAB_NG)
    a = coded(SLAB_NG)

    def body(h, r):
        h.set_global("u", a)
        out = [getattr(h, kind)("u", *args) for kind, args in SLAB_READS]
        # a rank without a row of the box may pass no buffer at all
        lo, hi, ns = SLAB_READS[2][1]
        i3 = lambda v: (C.c_int32 * 3)(*v)
        cnt = i3((-1, -1, -1))
        rc = h.L.cales_read_box(h.h, capi.FIELDS["u"], i3(lo), i3(hi), i3(ns), None, cnt)
        return out, rc, tuple(cnt)
    res = run_loopback(case, nranks, body)
    empty = 0
    for q, (kind, args) in enumerate(SLAB_READS):
        lo, hi, ns = _slab_box(kind, args)
        whole = np.full(one_rank_reads[q].shape, np.nan, order="F")
        for r in range(nranks):
            first, count = box_share(case, lo, hi, ns, nranks=nranks, rank=r)
            share = res[r][0][q]
            assert share.shape == count, (kind, args, r)
            empty += count[1] == 0
            j0 = (first[1] - lo[1]) // ns[1]
            assert np.isnan(whole[:, j0:j0 + count[1], :]).all()
            whole[:, j0:j0 + count[1], :] = share
        assert np.array_equal(whole, one_rank_reads[q]), (kind, args)
    assert empty > 0
    for r in range(nranks):      # (the two-row box above: NULL is refused exactly where there is something to write)
        _, rc, cnt = res[r]
        assert (rc != 0) == (cnt[1] > 0) and cnt[0] == 32 and cnt[2] == 10, (r, rc, cnt)
    assert sum(res[r][2][1] for r in range(nranks)) == 2


def test_single_precision_library():
    """libcales_hip_sp.so in a process of its own (the precision is process-wide): the by-value cases of one grid on float fields"""
    env = dict(os.environ, CALES_PRECISION="single")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_box_reads_worker.py")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["dtype"] == "float32" and res["real_size"] == 4 and res["reads"] >= 20 and res["wrong"] == [], res


def test_fortran_host_reads_planes_and_strided_volumes(tmp_path):
    """`cales` with iout2d = iout3d = 2 and CALES_OUT3D_NSKIP=2,2,3: the volume files hold the interior points 1, 1+nskip, ... of the fields of a Python
    host that ran the same steps (a[1:-1:2, 1:-1:2, 1:-1:3] of the haloed arrays: with an even number of cells a[1::2] would also take the ghost cell
    ng+1), log_visu_3d.out carries `2 2 3`, and the plane files are what they were: row ng(2)/2 of the same fields."""
    from cales_amd.hotpath import HotPath, initflow
    from cales_amd.nml import parse_text
    from tests import test_gpu_fortran_host as FH
    if not os.path.exists(FH.EXE):
        pytest.skip("Fortran host not built (amdflang absent)")
    text = FH._nml("chan_dsmag", nstep=4, icheck=2, iout0d=2, iout1d=100, iout2d=2, iout3d=2, isave=100000)
    text = re.sub(r"stop_type\(1:3\) = .*", "stop_type(1:3) = T, F, F", text)
    out = FH._run(str(tmp_path), text, env=dict(os.environ, CALES_OUT3D_NSKIP="2,2,3"))
    assert "*** Fim ***" in out
    case = parse_text(text); case.impdiff = 0
    ng = tuple(int(x) for x in case.ng)
    h = HotPath(case)
    h.upload(*initflow(case)); h.startup()
    dt = min(case.cfl * h.chkdt(), case.dtmax)
    fields = {}
    for s in range(1, 5):
        h.step(dt)
        if s % 2 == 0:
            dt = min(case.cfl * h.chkdt(), case.dtmax)
            fields[s] = h.download()
    h.close()
    names = ("vex", "vey", "vez", "pre", "visct")
    for s in (2, 4):
        for nm, a in zip(names, fields[s]):
            want = a[1:-1:2, 1:-1:2, 1:-1:3]
            vol = np.fromfile(os.path.join(tmp_path, f"{nm}_fld_{s:07d}.bin"))
            assert vol.size == want.size and np.array_equal(vol.reshape(want.shape, order="F"), want), (nm, s)
            sl = np.fromfile(os.path.join(tmp_path, f"{nm}_slice_fld_{s:07d}.bin"))
            assert np.array_equal(sl.reshape((ng[0], ng[2]), order="F"), a[1:-1, ng[1] // 2, 1:-1]), (nm, s)
    assert np.abs(fields[4][4]).max() > 0.
    logl = open(os.path.join(tmp_path, "log_visu_3d.out")).read().splitlines()
    assert len(logl) == 15      # the initial field, steps 2 and 4
    for l in logl:
        w = l.split()
        assert w[2:11] == ["1", "1", "1"] + [str(n) for n in ng] + ["2", "2", "3"], l
    assert logl[10].split()[:2] == ["vex_fld_0000004.bin", "Velocity_X"] and int(logl[10].split()[-1]) == 4
    for l in open(os.path.join(tmp_path, "log_visu_2d_slice_1.out")).read().splitlines():
        assert l.split()[2:11] == ["1", str(ng[1] // 2), "1", str(ng[0]), str(ng[1] // 2), str(ng[2]), "1", "1", "1"], l
