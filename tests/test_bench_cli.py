"""bench.py's command line: a plain run times the headline and nothing else, `--full` holds the
rest, `--dump-outputs DIR` writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_parse_plain_and_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    assert _parse(monkeypatch, "--sections", "headline").sections == "headline"
    a = _parse(monkeypatch, "--full", "--sections", "c3,c5", "--dump-outputs", "d")
    assert a.full and a.sections == "c3,c5" and a.dump_outputs == "d"
    with pytest.raises(SystemExit):  # the regime sections are behind --full
        _parse(monkeypatch, "--sections", "c3")


def test_dump_outputs_dtypes_and_sample(tmp_path, monkeypatch):
    t = {"a": torch.arange(12, dtype=torch.float32).reshape(3, 4),
         "b": torch.arange(5, dtype=torch.float64), "c": torch.arange(6, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / "o"), t)
    got = {n: np.load(tmp_path / "o" / f"{n}.npy") for n in t}
    assert got["a"].dtype == np.float32 and got["a"].shape == (3, 4)
    assert got["b"].dtype == np.float64 and got["c"].dtype == np.float64
    for n in t:
        assert np.array_equal(got[n], t[n].numpy())
    # over its share of the byte budget an array is written as the same sorted sample every time
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 16)  # 16 bytes per array
    for d in ("p", "q"):
        bench.dump_outputs(str(tmp_path / d), t)
    p = {n: np.load(tmp_path / "p" / f"{n}.npy") for n in t}
    assert p["a"].shape == (4,) and p["b"].shape == (2,) and p["c"].shape == (2,)
    assert sum(v.nbytes for v in p.values()) <= 3 * 16
    for n in t:
        assert np.array_equal(p[n], np.load(tmp_path / "q" / f"{n}.npy"))
        assert np.all(np.diff(p[n]) > 0) and np.isin(p[n], t[n].numpy()).all()


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps(tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4",
           "--warmup", "1", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONUNBUFFERED="1"),
                         capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["metric"] == bench.METRIC and r["unit"] == "samples/s" and r["dtype"] == "fp32"
    assert r["higher_is_better"] is True and r["steps"] == 4 and r["warmup"] == 1
    assert r["value"] > 0 and r["ms_per_step"] > 0
    rows = r["config"]["rows_per_repeat"] * r["config"]["repeats_per_step"]
    assert r["value"] == pytest.approx(rows / (r["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("regimes", "cpu_baseline", "phases_ms", "roofline", "graph_check_max_abs_diff"):
        assert key not in r, key
    S = r["config"]["subgraph_nodes"]
    got = {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert set(got) == {"weights_mean", "weights_std", "fit_weights", "logits", "kernel_weights"}
    assert got["weights_mean"].shape == (S,) and got["weights_std"].shape == (S,)
    assert got["fit_weights"].shape[-1] == S
    assert got["logits"].shape == got["kernel_weights"].shape
    assert got["kernel_weights"].dtype == np.float64
    for n in ("weights_mean", "weights_std", "fit_weights", "logits"):
        assert got[n].dtype == np.float32, n
    for n, a in got.items():
        assert np.isfinite(a).all(), n
    assert np.any(got["weights_mean"] != 0) and np.all(got["weights_std"] >= 0)
    assert ((got["logits"] >= 0) & (got["logits"] <= 1)).all()  # sigmoid head
    # the mean over the step's repeats of the last fit's weights
    assert np.allclose(got["fit_weights"].mean(0), got["weights_mean"], rtol=1e-5, atol=1e-7)
