#!/usr/bin/env python
"""Generate tests/golden/knn_kats.npz by running the UNMODIFIED reference evaluation/knn_images.py (sklearn's ball tree) on
generated datasets.  The reference is executed from its own file, never copied; seaborn, absent here, is stubbed as
tools/make_golden.py stubs absent modules.  Runs where the reference lives only.

Recorded per case: the sampled picks and titles, the neighbour indices and distances of the sampled rows, the unrounded error and
knn_mse.json's value.  Inputs are NOT stored: tests/knn_util.py regenerates them from the descriptors in the file.

For every case the tool asserts that the k + 2 smallest fp64 distances of EVERY row are more than 1e-9 apart (relative), so no fixture
is captured from an input whose order depends on rounding, and that the ball tree's neighbours equal a stable numpy argsort of the
fp64 differences-form distances, row for row, every row finding itself first.

    python tools/make_golden_eval.py            # writes tests/golden/knn_kats.npz
"""
from __future__ import print_function
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "knn_kats.npz")
sys.path.insert(0, os.path.join(REPO, "tests"))

import knn_util as ku  # noqa: E402

MIN_GAP = 1e-9


def _stub_modules():
    sb = types.ModuleType("seaborn")
    sb.set = lambda *a, **k: None
    sys.modules["seaborn"] = sb
    import matplotlib
    matplotlib.use("Agg")


def cases():
    out = []
    for n, d in ku.SEEDED_SHAPES:
        for n_samples in (5, 200):
            for seed in (1, 7):
                out.append(dict(name="n%d_d%d_s%d_seed%d" % (n, d, n_samples, seed), n=n, d=d, kind="plain", k=5,
                                n_samples=n_samples, seed=seed))
    out.append(dict(name="ground_truth", n=300, d=3, kind="ground-truth", k=5, n_samples=200, seed=1))
    out.append(dict(name="relative_pos", n=257, d=3, kind="relative-pos", k=5, n_samples=200, seed=1))
    return out


def run_reference(case):
    ds = ku.eval_dataset(case["n"], case["d"], case["kind"])
    searched = ds["true_states"] if case["kind"] == "ground-truth" else ds["states"]
    # the gap condition, on every row
    _, d2 = ku.brute_knn(searched, searched, case["k"] + 2)
    gap = float(ku.relative_gaps(d2).min())
    assert gap > MIN_GAP, (case["name"], gap)
    cwd = os.getcwd()
    argv = list(sys.argv)
    with tempfile.TemporaryDirectory() as root:
        log = ku.write_eval_dataset(root, ds)
        os.chdir(root)
        try:
            sys.argv = ["knn_images.py", "--log-folder", log, "--seed", str(case["seed"]), "-k", str(case["k"]),
                        "-n", str(case["n_samples"]), "--n-to-plot", "0"]
            if case["kind"] == "ground-truth":
                sys.argv.append("--ground-truth")
            if case["kind"] == "relative-pos":
                sys.argv.append("--relative-pos")
            g = runpy.run_path(os.path.join(REF, "evaluation", "knn_images.py"), run_name="__main__")
            with open(os.path.join(log, "knn_mse.json")) as f:
                result = json.load(f)
        finally:
            os.chdir(cwd)
            sys.argv = argv
    # the ball tree against the numpy oracle, all rows
    bi, bd2 = ku.brute_knn(searched, searched, case["k"] + 1)
    assert np.array_equal(np.asarray(g["neighbors_indices"]), bi), case["name"]
    assert np.array_equal(bi[:, 0], np.arange(case["n"])), case["name"]
    np.testing.assert_allclose(np.asarray(g["distances"]) ** 2, bd2, rtol=1e-12, atol=1e-300)
    picks = np.array([t[3] for t in g["data"]], dtype=np.int64)
    rec = {
        "picks": picks,
        "titles": np.array(result["images"]),
        "neighbors": np.array([t[1] for t in g["data"]], dtype=np.int64),
        "distances": np.array([t[2] for t in g["data"]], dtype=np.float64),
        "mean_error": np.float64(g["mean_error"]),
        "knn_mse": np.float64(result["knn_mse"]),
        "min_gap": np.float64(gap),
    }
    if case["kind"] == "relative-pos":
        rec["true_states_sum"] = np.float64(np.asarray(g["true_states"]).sum())
        rec["true_states_head"] = np.asarray(g["true_states"])[:60:7].copy()
    assert list(result["images"]) == list(g["images_titles"])
    return rec


def main():
    _stub_modules()
    out = {}
    cs = cases()
    for case in cs:
        rec = run_reference(case)
        for k, v in rec.items():
            out["%s/%s" % (case["name"], k)] = v
        print("%-28s min gap %.2e  knn_mse %s" % (case["name"], rec["min_gap"], rec["knn_mse"]))
    out["cases"] = np.array(json.dumps(cs))
    import sklearn
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
