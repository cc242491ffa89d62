"""The passes of cmpt_sgs (k_sgs.hip: SgsPath, filled by sgs_setup, launched by dsmag_fast / smag_fast and the two reference sequences): every instantiation
of k_strain_tile, k_corr_strain_tile, k_lmf_tile, k_lmf_plane_tile and k_smag_rows on a grid of a few thousand cells that reaches it, the two sequences and
the coefficient tail they share with the tile form, held to the commit before the pass records bit for bit: the plan string and a SHA-256 of the bytes of
the result (tests/golden/sgs_passes/digests.json, written by gen_digests.py beside it with that commit's library; it runs the functions of this file). No
tolerance: the same instructions run in the same geometry, in the same order.

Kinds of case. sgs: the interior eddy viscosity after one operator-level cmpt_sgs of the case's initial field plus 2 % noise (tests/test_gpu_filter2d._fields)
-- the strain-rate pass without the projection, six components (seed 3; volume averaging seed 4, which tests/test_gpu_dsmag_average.py picked by the
reference for a coefficient the clip does not zero; every case asserts a field that is not all zeros). step: u, v, w, p, visct after start-up and two cales_steps from that field -- where the plan
folds the projection into the strain-rate pass, k_corr_strain_tile and (one rank) five components. ranks: the same on two loopback ranks, in order or with
the second stream (the last pass split in three around the exchange), per rank.

The second test holds each row to the instantiations it claims: with CALES_TEST_BAD_LAUNCH (tests/test_gpu_launch_check.py) set to the name as sgs_setup
spells it, the runtime refuses that launch for its block size -- nothing runs -- and the case fails naming it. Without it the table could stop covering a
kernel and nobody would notice."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.util import GOLD

pytestmark = pytest.mark.gpu

DIGESTS = os.path.join(GOLD, "sgs_passes", "digests.json")
SWITCHES = ("CALES_WIDE_OFFSETS", "CALES_UNMERGED_BC", "CALES_DSMAG_XGHOSTS", "CALES_SGS_SIX_COMPONENTS", "CALES_LMF_UNPACKED_REMAINDER",
            "CALES_DSMAG_REFERENCE_SEQUENCE", "CALES_SMAG_REFERENCE_SEQUENCE", "CALES_DSMAG_AVERAGE", "CALES_FILTER_2D", "CALES_KCHUNK", "CALES_UNFOLDED_CORREC",
            "CALES_OVERLAP", "CALES_NO_OVERLAP", "CALES_LOOPBACK_EVENTS", "CALES_TEST_BAD_LAUNCH")
WIDE, UNMERGED, XGHOSTS, SIX = {"CALES_WIDE_OFFSETS": "1"}, {"CALES_UNMERGED_BC": "1"}, {"CALES_DSMAG_XGHOSTS": "1"}, {"CALES_SGS_SIX_COMPONENTS": "1"}
UNPACKED, SEQUENCE = {"CALES_LMF_UNPACKED_REMAINDER": "1"}, {"CALES_DSMAG_REFERENCE_SEQUENCE": "1"}
G = (64, 16, 12)

# the instantiations as sgs_setup spells them
S_PLAIN32, S_PLAIN64 = "k_strain_tile<unsigned, TYS, 0>", "k_strain_tile<size_t, TYS, 0>"
S_YW32, S_YW64 = "k_strain_tile<unsigned, TYS, 1>", "k_strain_tile<size_t, TYS, 1>"
S_PAIR, S_F2D32, S_F2D64 = "k_strain_tile<unsigned, TYS, 0, 1>", "k_strain_tile<unsigned, TYS, 0, 2>", "k_strain_tile<size_t, TYS, 0, 2>"
S_CORR, S_CORR_ROWS2, S_CORR5 = "k_corr_strain_tile<unsigned, TYC>", "k_corr_strain_tile<unsigned, TYC, 1>", "k_corr_strain_tile<unsigned, TYC, 2>"
L_PAIR, L_PAIR5 = "k_lmf_tile<unsigned, 0, 1, 1>", "k_lmf_tile<unsigned, 0, 1, 2>"
L_UCF32, L_UCF64, L_PLAIN32, L_PLAIN64 = "k_lmf_tile<unsigned, 0, 1>", "k_lmf_tile<size_t, 0, 1>", "k_lmf_tile<unsigned, 0, 0>", "k_lmf_tile<size_t, 0, 0>"
L_YW_UCF32, L_YW_UCF64, L_YW32, L_YW64 = "k_lmf_tile<unsigned, 1, 1>", "k_lmf_tile<size_t, 1, 1>", "k_lmf_tile<unsigned, 1, 0>", "k_lmf_tile<size_t, 1, 0>"
L_F2D32, L_F2D64 = "k_lmf_plane_tile<unsigned>", "k_lmf_plane_tile<size_t>"
L_LOCAL_PAIR, L_LOCAL_YW, L_LOCAL_UCF = "k_lmf_tile<unsigned, 0, 1, 5>", "k_lmf_tile<unsigned, 1, 1, 4>", "k_lmf_tile<unsigned, 0, 1, 4>"
L_PACKED, L_PACKED5 = "k_lmf_tile<unsigned, 0, 1, 9>", "k_lmf_tile<unsigned, 0, 1, 10>"
R_PLAIN32, R_PLAIN64, R_YW32, R_YW64 = "k_smag_rows<unsigned, 0>", "k_smag_rows<size_t, 0>", "k_smag_rows<unsigned, 1>", "k_smag_rows<size_t, 1>"

# (kind, golden, grid, environment, case fields, the kernels the case must launch)
CASES = [
    # stored x ghost columns: no ucf, no pair fields -- the plain instantiations of both passes
    ("sgs", "chan_dsmag", G, XGHOSTS, {}, (S_PLAIN32, L_PLAIN32)), ("sgs", "chan_dsmag", G, {**XGHOSTS, **WIDE}, {}, (S_PLAIN64, L_PLAIN64)),
    # a wall-model face and a free-slip one in z (both walls to the normal velocity: ucf, and pair fields while the offsets are narrow)
    ("sgs", "halfchan_dsmag_wm", G, {}, {}, (S_PAIR, L_PAIR)), ("sgs", "halfchan_dsmag_wm", G, WIDE, {}, (S_PLAIN64, L_UCF64)),
    # y walls
    ("sgs", "duct_dsmag", G, {}, {}, (S_YW32, L_YW_UCF32)), ("sgs", "duct_dsmag", G, WIDE, {}, (S_YW64, L_YW_UCF64)),
    ("sgs", "duct_dsmag", G, XGHOSTS, {}, (S_YW32, L_YW32)), ("sgs", "duct_dsmag", G, {**XGHOSTS, **WIDE}, {}, (S_YW64, L_YW64)),
    # the channel without pair fields
    ("sgs", "chan_dsmag", G, UNMERGED, {}, (S_PLAIN32, L_UCF32)), ("sgs", "chan_dsmag", G, WIDE, {}, (S_PLAIN64, L_UCF64)),
    # pair fields, six components (outside the step), the remainder tile packed (64 = 62 + 2 columns) and not
    ("sgs", "chan_dsmag_x64", G, {}, {}, (S_PAIR, L_PAIR, L_PACKED)), ("sgs", "chan_dsmag_x64", G, UNPACKED, {}, (S_PAIR, L_PAIR)),
    # the plane filter
    ("sgs", "chan_dsmag", G, {}, {"filter2d": True}, (S_F2D32, L_F2D32)), ("sgs", "chan_dsmag", G, WIDE, {"filter2d": True}, (S_F2D64, L_F2D64)),
    # the projection inside the strain-rate pass: five components, six by the switch; 128 x 24 x 10: three live packed segments
    ("step", "chan_dsmag_x64", G, {}, {}, (S_CORR5, L_PAIR5, L_PACKED5, L_PACKED)), ("step", "chan_dsmag_x64", G, SIX, {}, (S_CORR, L_PAIR, L_PACKED)),
    ("step", "chan_dsmag_x128", (128, 24, 10), {}, {}, (S_CORR5, L_PAIR5, L_PACKED5)), ("step", "chan_dsmag_x128", (128, 24, 10), UNPACKED, {}, (S_CORR5, L_PAIR5)),
    # ... from two ghost rows of the prediction on two ranks; with the second stream the last pass is launched in three parts around the exchange
    ("ranks", "chan_dsmag_x64", G, {}, {}, (S_CORR_ROWS2, L_PAIR)), ("ranks", "chan_dsmag_x64", G, {"CALES_OVERLAP": "1", "CALES_LOOPBACK_EVENTS": "1"}, {}, (S_CORR_ROWS2, L_PAIR)),
    # a coefficient per cell
    ("sgs", "chan_dsmag_x64", G, {}, {"dsmag_average": "local"}, (S_PAIR, L_LOCAL_PAIR)), ("sgs", "duct_dsmag", G, {}, {"dsmag_average": "local"}, (S_YW32, L_LOCAL_YW)),
    ("sgs", "chan_dsmag", G, UNMERGED, {"dsmag_average": "local"}, (S_PLAIN32, L_LOCAL_UCF)), ("step", "chan_dsmag_x64", G, {}, {"dsmag_average": "local"}, (S_CORR, L_LOCAL_PAIR)),
    # static Smagorinsky, the row-marching kernel
    ("sgs", "chan_smag", G, {}, {}, (R_PLAIN32,)), ("sgs", "chan_smag", G, WIDE, {}, (R_PLAIN64,)),
    ("sgs", "duct_smag_wm", G, {}, {}, (R_YW32,)), ("sgs", "duct_smag_wm", G, WIDE, {}, (R_YW64,)),
    # the two sequences (walls in x), x-line averaging (the sequence), and the tail both forms share: volume averaging in both, k_dsmag_final in the tile form
    # (a non-zero boundary value of visct: |S| is kept, not lazy) beside the k_dsmag_coef of every lazy case above
    ("sgs", "cavity_dsmag", (20, 16, 12), {}, {}, ("k_plane_sum", "k_dsmag_final")), ("sgs", "cavity_smag_wm6", (20, 16, 12), {}, {}, ("k_strain",)),
    ("sgs", "duct_dsmag", G, {}, {"dsmag_average": "xlines"}, ("k_contract_lines",)),
    ("sgs", "chan_dsmag", G, {}, {"dsmag_average": "volume", "seed": 4}, (L_PAIR, "k_plane_fold", "k_volume_fold", "k_dsmag_coef")),
    ("sgs", "chan_dsmag", G, SEQUENCE, {"dsmag_average": "volume", "seed": 4}, ("k_plane_sum", "k_volume_fold", "k_dsmag_final")),
    ("sgs", "chan_dsmag_x64", G, {}, {"bcsgs_z": 1e-5}, (L_PAIR, "k_dsmag_final")), ("step", "chan_dsmag_x64", G, {}, {"bcsgs_z": 1e-5}, (S_CORR5, L_PAIR5, "k_dsmag_final")),
]


def case_id(kind, name, ng, env, edits, kernels=()):
    return "-".join([kind, name, "%dx%dx%d" % tuple(ng)] + [k[6:].lower() for k in sorted(env)] + ["%s=%s" % (k, edits[k]) for k in sorted(edits)])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()).hexdigest()


def _case(name, ng, edits):
    from tests.test_gpu_filter2d import _shaped_case
    case = _shaped_case(name, ng)
    case.filter2d = bool(edits.get("filter2d", False))
    case.dsmag_average = edits.get("dsmag_average", "planes")
    if "bcsgs_z" in edits:
        case.bcsgs[:, 2] = edits["bcsgs_z"]
    return case


def _sgs(case, seed):
    from tests.test_gpu_filter2d import _fields
    from tests.test_gpu_golden import _hot
    from tests.util import F
    h = _hot(case)
    try:
        plan = h.describe_plan()
        h.upload(*(F(a) for a in _fields(case, seed))); h.bounduvw(True, False); h.boundp("p", 0)
        h.cmpt_sgs()
        visct = h.get("visct")[1:-1, 1:-1, 1:-1]
        assert np.isfinite(visct).all() and np.abs(visct).max() > 0.      # (a field of zeros would compare equal whatever the kernels do)
        return {"sgs": plan["sgs"], "visct": _sha(visct)}
    finally:
        h.close()


def _step(case, seed):
    from tests.test_gpu_filter2d import _fields
    from tests.test_gpu_golden import _hot
    from tests.util import F
    h = _hot(case)
    try:
        plan = h.describe_plan()
        h.upload(*(F(a) for a in _fields(case, seed))); h.startup()
        dt = 0.5 * h.chkdt()
        for _ in range(2):
            h.step(dt)
        got = h.download()
        assert np.abs(got[4]).max() > 0.
        out = {"sgs": plan["sgs"], "projection": plan["projection"]}
        out.update({k: _sha(a) for k, a in zip(("u", "v", "w", "p", "visct"), got)})
        return out
    finally:
        h.close()


def _ranks(case, seed):      # (the deterministic initial field, slab by slab)
    from cales_amd.decomp import run_loopback

    def body(h, r):
        plan = h.describe_plan()
        h.upload_initial(); h.startup()
        dt = 0.5 * h.chkdt()
        for _ in range(2):
            h.step(dt)
        return h.download() + [plan]
    out = {}
    for r, x in enumerate(run_loopback(case, 2, body)):
        assert np.abs(x[4]).max() > 0.
        out.update({"rank%d_%s" % (r, k): x[5][k] for k in ("sgs", "projection", "exchanges")})
        out.update({"rank%d_%s" % (r, k): _sha(a) for k, a in zip(("u", "v", "w", "p", "visct"), x)})
    return out


def run_case(kind, name, ng, env, edits, kernels=(), bad_launch=None):
    """the plan strings and digests of one case, with the switches of env set for the context's lifetime"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    if bad_launch:
        os.environ["CALES_TEST_BAD_LAUNCH"] = bad_launch
    try:
        return {"sgs": _sgs, "step": _step, "ranks": _ranks}[kind](_case(name, ng, edits), edits.get("seed", 3))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("case", CASES, ids=[case_id(*c) for c in CASES])
def test_sgs_passes_give_the_bits_of_the_commit_before(case):
    want = json.load(open(DIGESTS))[case_id(*case)]
    got = run_case(*case)
    print(case_id(*case), got)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], (k, got[k], want[k])


REACHES = [(c, k) for c in CASES for k in c[5]]


@pytest.mark.parametrize("case,kernel", REACHES, ids=["%s-%s" % (case_id(*c), k.replace(" ", "")) for c, k in REACHES])
def test_each_case_reaches_the_instantiation_it_claims(case, kernel):
    """with that one kernel made unlaunchable the case fails, and the message names it"""
    from cales_amd.hotpath import CalesError
    with pytest.raises(CalesError) as e:
        run_case(*case, bad_launch=kernel)
    assert "kernel launch failed" in str(e.value) and kernel in str(e.value), e.value
