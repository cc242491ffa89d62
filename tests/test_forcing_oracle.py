"""The cases of tests/test_gpu_forcing.py on the CPU restatement ALONE: every forcing set does something there. Bulk forcing in y or z taken away, or the
body force taken away, moves the component it acts on by at least 1e-2 of its maximum after the test's number of steps -- a device run that ignored
is_forced(2:3), velf(2:3) or bforce could not agree with the oracle to 1e-9. (bforce(3) between walls is a pure gradient: the pressure takes it.)"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import FORCING_STEP_PARAMS, forced_case, forcing_id, perturbed_start, relerr

# one row per (case, grid, set, steps): the switches select forms of the device code, not other cases
ROWS = sorted({(name, ng, s, nsteps) for name, ng, s, nsteps, _, _ in FORCING_STEP_PARAMS})
_cache = {}


def _steps(name, ng, fset, nsteps, edit=None):
    key = (name, ng, fset, nsteps, edit)
    if key not in _cache:
        case = forced_case(name, ng, fset)
        if edit is not None:
            what, d = edit
            if what == "is_forced": case.is_forced[d] = False
            else: case.bforce[d] = 0.
        o = Oracle(case, nthreads=4)
        (u, v, w, p, visct, pp, dt), _ = perturbed_start(case, o)
        if edit is not None:      # the same time step as the run it is compared with
            dt = _steps(name, ng, fset, nsteps)[4]
        for _ in range(nsteps):
            o.step(dt, u, v, w, p, pp, visct)
        o.close()
        _cache[key] = (u, v, w, p, dt)
    return _cache[key]


@pytest.mark.parametrize("name,ng,fset,nsteps", ROWS, ids=forcing_id)
def test_forcing_sets_are_no_no_ops(name, ng, fset, nsteps):
    case = forced_case(name, ng, fset)
    base = _steps(name, ng, fset, nsteps)
    assert all(np.isfinite(a).all() for a in base[:4])
    walls_z = case.cbcvel[0, 2, 2] != "P"
    checked = 0
    for d in range(3):
        if case.is_forced[d] and d > 0:      # (x forcing is what every other forced case of the suite has)
            other = _steps(name, ng, fset, nsteps, ("is_forced", d))
            err = relerr(other[d], base[d])
            print(name, ng, fset, "forcing", "xyz"[d], err)
            assert err >= 1e-2, ("forcing", d, err); checked += 1
        if case.bforce[d] != 0.:
            other = _steps(name, ng, fset, nsteps, ("bforce", d))
            q = 3 if (d == 2 and walls_z) else d
            a, b = other[q][1:-1, 1:-1, 1:-1], base[q][1:-1, 1:-1, 1:-1]
            err = relerr(a - a.mean(), b - b.mean()) if q == 3 else relerr(a, b)
            print(name, ng, fset, "bforce", "xyz"[d], "on", "uvwp"[q], err)
            assert err >= 1e-2, ("bforce", d, err); checked += 1
    assert checked > 0
