"""bench.py's plain run and --dump-outputs: the dump writer on CPU; on the GPU, two fresh processes of the same command time
exactly --steps steps and write identical outputs (the weights are seeded, the decode step is deterministic)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_dump_outputs_dtypes_and_limit(tmp_path):
    names = bench.dump_outputs(str(tmp_path / "d"), {"logits": torch.randn(1, 32, dtype=torch.float16),
                                                     "next_token": torch.tensor([31999], dtype=torch.long)})
    assert names == ["logits", "next_token"]
    lg = np.load(tmp_path / "d" / "logits.npy")
    tok = np.load(tmp_path / "d" / "next_token.npy")
    assert lg.dtype == np.float32 and lg.shape == (1, 32)
    assert tok.dtype == np.float64 and tok.tolist() == [31999.0]
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, dtype=np.float32)})
    assert not (tmp_path / "big").exists()


def test_options_listed():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--dump-outputs" in out.stdout and "--full" in out.stdout


@pytest.mark.gpu
def test_plain_run_dumps_identical_outputs(tmp_path):
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--model", "tiny", "--steps", "6",
                              "--warmup", "2", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=REPO)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1, out.stdout
        lines.append(json.loads(js[0]))
        dumps.append({n: np.load(d / (n + ".npy")) for n in ("logits", "next_token")})
    for r in lines:
        assert r["steps"] == 6 and r["warmup"] == 2 and r["unit"] == "tokens/s" and r["higher_is_better"] is True
        assert r["ms_per_step"] > 0 and abs(r["value"] - 1e3 / r["ms_per_step"]) <= 5e-3 * r["value"]
        assert len(r["runs_tokens_per_s"]) == 1
        assert "roofline" not in r and "parity" not in r and "cpu_baseline" not in r
    a, b = dumps
    assert a["logits"].dtype == np.float32 and a["logits"].shape == (1, 512) and np.isfinite(a["logits"]).all()
    assert a["next_token"].dtype == np.float64 and a["next_token"].shape == (1,)
    tok = a["next_token"][0]
    assert tok == int(tok) and 0 <= tok < 512 and a["logits"][0, int(tok)] == a["logits"].max()     # the greedy token of these logits
    assert np.array_equal(a["logits"], b["logits"]) and np.array_equal(a["next_token"], b["next_token"])
