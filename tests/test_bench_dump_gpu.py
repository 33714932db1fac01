"""bench.py --dump-outputs: after the timed steps, what the last timed step computed lands in DIR/<name>.npy (float32) — the AE leg's
under plain names, the VAE leg's with the prefix vae_ — and --steps is the number of timed steps even when the region is short.
A plain run (no --full) dumps the same arrays as a --full one and leaves out what only --full measures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    proc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "3", "--warmup", "1", "--batch-size", "8",
                           "--dump-outputs", str(out_dir)] + extra, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=500)
    assert proc.returncode == 0, proc.stderr.decode("utf-8", "replace")[-3000:]
    lines = [l for l in proc.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    names = out["dump_outputs"]["arrays"]
    assert sorted(os.listdir(str(out_dir))) == sorted(n + ".npy" for n in names)
    return out, proc.stderr, {n: np.load(str(out_dir / (n + ".npy"))) for n in names}


@pytest.mark.timeout(900)
def test_bench_dumps_the_last_timed_step(tmp_path):
    # with the instrumented steps behind the timed region (they move the parameters again) ...
    out, err, arrays = _bench(tmp_path / "timers", ["--full", "--no-cpu-baseline", "--timer-steps", "2"])
    assert "roofline" in out and out["roofline"]["timing"].startswith("2 instrumented steps")
    # a short region still gives its line (with a warning exactly when it is short): the step count asked for is the one timed
    assert (b"too short to be a measurement" in err) == (out["timed_region_s"] < 0.1)
    assert out["steps"] == 3 and out["ms_per_step"] == pytest.approx(1e3 * out["timed_region_s"] / 3, abs=0.02)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for prefix, final in (("", out["config"]["final_loss"]), ("vae_", out["vae"]["final_loss"])):
        assert {prefix + n for n in ("loss", "params", "grad", "bn_running_stats")} <= set(arrays)
        assert float(arrays[prefix + "loss"][0]) == pytest.approx(final, abs=2e-6)
        assert arrays[prefix + "params"].shape == arrays[prefix + "grad"].shape and arrays[prefix + "params"].size > 10 ** 6
        assert np.abs(arrays[prefix + "grad"]).max() > 0
    assert "loss_reconstruction_loss" in arrays and "vae_loss_generation_loss" in arrays and "vae_loss_kl_loss" in arrays
    # ... the same arrays as a plain run, which has no instrumented steps: the seeded inputs and the step are the same, and the dump is
    # taken right after the last timed step (one more Adam step moves every parameter by about the learning rate)
    plain_out, _, plain = _bench(tmp_path / "plain", [])
    assert not {"roofline", "north_star", "cpu_baseline"} & set(plain_out) and "vae" in plain_out
    assert sorted(plain) == sorted(arrays)
    for name in arrays:
        assert np.array_equal(plain[name], arrays[name]), name
