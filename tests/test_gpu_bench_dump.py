"""bench.py --dump-outputs on the GPU: a plain run writes the f, |g| and x its timed steps ended
on (all of a short x, the fixed sample of a long one), the same as the same solve through the
binding, and its line carries the headline fields with everything behind --full left null."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402

pytestmark = pytest.mark.gpu
M, WARM, STEPS = 3, 2, 4


@pytest.mark.parametrize("n", [100_003, (1 << 22) + 5])  # all of x; the sample of a longer x
def test_plain_run_dumps_its_last_step(n, tmp_path, monkeypatch, capsys):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARM),
                                      "--size", str(n), "--history", str(M), "--dump-outputs", str(tmp_path)])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["warmup"] == WARM and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
    assert line["unit"] == "iters/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    for k in ("roofline", "cpu_baseline", "reference_parity", "vector_free", "persistent", "box_copy_tbps"):
        assert line[k] is None
    x0 = L.x0_uniform(n, 42, -2.0, 2.0)
    with L.Context(n, M) as c:
        c.init("rosenbrock", x0, "backtracking", tolerance=1e-5)
        c.step(M)
        c.step(WARM)
        r = c.step(STEPS)
        x = c.get_x()
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)  # noqa: E731
    f, g = np.load(tmp_path / "f.npy"), np.load(tmp_path / "gnorm.npy")
    assert f.dtype == g.dtype == np.float64
    assert np.array_equal(bits(f), bits([r["f"]])) and np.array_equal(bits(g), bits([r["gnorm"]]))
    assert line["solver"]["f"] == r["f"]
    if n <= bench.DUMP_SAMPLE:
        assert np.array_equal(bits(np.load(tmp_path / "x.npy")), bits(x))
    else:
        idx, xs = np.load(tmp_path / "x_sample_index.npy"), np.load(tmp_path / "x_sample.npy")
        assert xs.dtype == np.float64 and len(xs) == len(idx) > bench.DUMP_SAMPLE // 2
        assert np.array_equal(bits(xs), bits(x[idx.astype(np.int64)]))
