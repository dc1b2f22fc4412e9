"""bench.py --dump-outputs: what the last timed step computed, as .npy files of finite values a second build can be
compared with: the hit mask of the sampled rays, the outputs of those that hit, the gradient texture.  Two runs with the
same arguments trace the same rays, so their per-ray outputs agree bit for bit; the gradient texture is a float-atomic
sum, equal up to summation order.  The film is large enough that the per-ray outputs are a sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID, FILM, SPP, STEPS = 256, 128, 32, 3
SIZE = ["--grid", str(GRID), "--film", str(FILM), "--spp", str(SPP), "--steps", str(STEPS), "--warmup", "1",
        "--cpu-seconds", "0"]
PER_RAY = {"t": 1, "p": 3, "n": 3, "uv": 2, "sh_n": 3, "dp_du": 3, "dp_dv": 3, "pi_t": 1, "prim_uv": 2, "prim_index": 1}


def _bench(out_dir):
    env = dict(os.environ, HF_BENCH_EXTRAS="0")
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + SIZE + ["--dump-outputs", str(out_dir)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    files = sorted(os.listdir(d))
    assert files == sorted([k + ".npy" for k in PER_RAY] + ["valid.npy", "grad_heights.npy"]), files
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    for name, a in out.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    return out


def test_dump_outputs(hf, tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    line = _bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    a = _load(tmp_path / "a")
    k = bench.DUMP_RAYS
    assert FILM * FILM * SPP > k                      # the per-ray outputs are the seeded sample
    valid = a["valid"]
    assert valid.shape == (k,) and set(np.unique(valid)) <= {0.0, 1.0}
    assert abs(valid.mean() - line["config"]["hit_fraction_rank0"]) < 0.02
    m = int(valid.sum())                              # the outputs are those of the rays that hit
    for name, c in PER_RAY.items():
        assert a[name].shape == ((m,) if c == 1 else (c, m)), (name, a[name].shape)
    assert (a["t"] > 0).all() and np.array_equal(a["t"], a["pi_t"])
    g = a["grad_heights"]                             # the whole texture at this grid size
    assert g.shape == (GRID, GRID) and g.dtype == np.float32
    assert np.isclose(np.linalg.norm(g.astype(np.float64)), line["grad_l2"], rtol=1e-9)

    _bench(tmp_path / "b")
    b = _load(tmp_path / "b")
    for name in list(PER_RAY) + ["valid"]:
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert np.allclose(a["grad_heights"], b["grad_heights"], rtol=1e-5, atol=1e-6 * np.abs(a["grad_heights"]).max())
