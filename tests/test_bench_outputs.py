"""bench.py as later measurements run it: a plain run is the headline alone, and --dump-outputs DIR writes the state its timed steps left."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Fields:
    """Stands in for a HotPath after its last step: download() returns u, v, w, p, visct."""

    def __init__(self, shape, seed):
        rng = np.random.RandomState(seed)
        self.fields = [np.asfortranarray(rng.rand(*shape)) for _ in range(5)]

    def download(self):
        return [f.copy(order="F") for f in self.fields]


def _read(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_fields_and_fixed_samples(tmp_path):
    import bench
    # small fields: written whole
    h = _Fields((10, 6, 8), 1)
    bench.dump_outputs(h, str(tmp_path / "small"))
    got = _read(tmp_path / "small")
    assert sorted(got) == sorted(k + s for k in ("u", "v", "w", "p", "visct") for s in (".npy", "_zmean.npy"))
    for k, f in zip(("u", "v", "w", "p", "visct"), h.fields):
        assert got[k + ".npy"].dtype == np.float64 and np.array_equal(got[k + ".npy"], f)
        assert np.allclose(got[k + "_zmean.npy"], f.mean(axis=(0, 1)))
    # fields above DUMP_VALUES: the same fixed positions from run to run and for every field, at most 64 MB in all
    shape = (104, 102, 102)
    h = _Fields(shape, 2)
    bench.dump_outputs(h, str(tmp_path / "a")); bench.dump_outputs(_Fields(shape, 3), str(tmp_path / "b"))
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in a) <= 64 * 2 ** 20
    idx = np.unique(np.random.RandomState(0).randint(0, int(np.prod(shape)), bench.DUMP_VALUES))
    assert idx.size <= bench.DUMP_VALUES
    for k, f in zip(("u", "v", "w", "p", "visct"), h.fields):
        assert np.array_equal(a[k + ".npy"], f.ravel(order="F")[idx])
        assert a[k + ".npy"].shape == b[k + ".npy"].shape and not np.array_equal(a[k + ".npy"], b[k + ".npy"])
        assert a[k + "_zmean.npy"].shape == (shape[2],)


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_its_outputs_are_the_timed_state(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one JSON line with the headline fields and none of the --full measurements; the
    dumped u, v, w, visct are W + K steps of the bench's case on the oracle (the CPU restatement), to the bound smoke() holds the same path to."""
    import bench
    from cales_amd.hotpath import initflow
    from oracle.oracle import Oracle
    ng, W, K = (64, 32, 32), 1, 3
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                        "--ng", *map(str, ng), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "time-steps/sec" and d["unit"] == "time-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == K and d["warmup"] == W and d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - 1.) < 1e-9
    assert not {"roofline", "calibration", "kernels_ms_per_step", "configs", "cpu_baseline"} & set(d), sorted(d)
    case = bench.channel_case(ng, "dsmag")
    u, v, w, p = initflow(case)
    o = Oracle(case)
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    for _ in range(W + K):
        o.step(d["config"]["dt"], u, v, w, p, pp, visct)
    o.close()
    got = _read(out)
    for k, ref in (("u", u), ("v", v), ("w", w), ("visct", visct)):
        assert got[k + ".npy"].shape == ref.shape and got[k + ".npy"].dtype == np.float64
        assert relerr(got[k + ".npy"], ref) < 1e-9, k
        assert np.abs(got[k + "_zmean.npy"] - ref.mean(axis=(0, 1))).max() <= 1e-9 * np.abs(ref).max(), k      # (v, w: plane means of round-off size)
