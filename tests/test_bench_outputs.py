"""bench.py --dump-outputs / --full: the dump helpers on the host, and one tiny plain run (C1:
Gamma point, 8^3 mesh) on the GPU whose result line and .npy files are checked."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_helpers():
    sys.path.insert(0, ROOT)
    import bench
    z = (np.arange(6) - 1j * np.arange(6)).reshape(2, 3)
    f = bench._as_f64(z)
    assert f.dtype == np.float64 and f.shape == (2, 3, 2)
    assert np.array_equal(f[..., 0], z.real) and np.array_equal(f[..., 1], z.imag)
    p = bench._as_f64(np.arange(5, dtype=np.int32))
    assert p.dtype == np.float64 and np.array_equal(p, np.arange(5))
    # small arrays are written whole; large ones as the same sorted sample every time, at the cap
    assert bench._sample_idx(1000, 16) is None
    n = bench.DUMP_CAP_BYTES // 16 * 3
    i, j = bench._sample_idx(n, 16), bench._sample_idx(n, 16)
    assert np.array_equal(i, j) and len(i) * 16 <= bench.DUMP_CAP_BYTES
    assert (np.diff(i) > 0).all() and i[0] >= 0 and i[-1] < n
    assert 5 * bench.DUMP_CAP_BYTES < 64 << 20


def test_full_is_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_dumps_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "c1", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["nk"] / (line["ms_per_step"] * 1e-3)) \
        <= 1e-3 * line["value"]
    # the legs behind --full did not run
    assert line["cpu_baseline"] is None and line["ao_eval"] is None
    assert "isolated" not in line["roofline"]
    nao, nip = line["config"]["nao"], line["config"]["nip"]
    # J, K as get_jk returned them (real at Gamma; complex arrays carry a trailing re/im axis)
    shapes = {"vj": (1, nao, nao), "vk": (1, nao, nao), "perm": (nip,),
              "w0": None, "wq_sample": None}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in shapes)
    total = 0
    for name, shape in shapes.items():
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float64 and np.isfinite(a).all() and a.size > 0, name
        if shape is not None:
            assert a.shape in (shape, shape + (2,)), (name, a.shape)
        total += a.nbytes
    assert total <= 64 << 20
    perm = np.load(out / "perm.npy")
    assert len(set(perm.tolist())) == nip and (perm == np.round(perm)).all()
    assert np.abs(np.load(out / "vj.npy")).max() > 0
