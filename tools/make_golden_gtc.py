#!/usr/bin/env python
"""Generate tests/golden/gtc_kats.npz by running the UNMODIFIED reference: plotting/representation_plot.py as __main__ with
--correlation --print-corr on generated datasets (numpy's corrcoef), and evaluation/gather_results.py as __main__ over a small
generated log tree whose result files are already present (pandas writes its results.csv).  The reference is executed from its own
files, never copied; seaborn and termcolor, absent here, are stubbed as tools/make_golden.py stubs absent modules, and matplotlib
draws into the Agg backend.  Runs where the reference lives only.

Recorded: the case descriptors, gt_corr and gt_corr_mean of gt_correlation.json per case, and the results table cell by cell.
Inputs are NOT stored: tests/gtc_util.py regenerates the datasets and the log tree from the descriptors.

    python tools/make_golden_gtc.py            # writes tests/golden/gtc_kats.npz
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
OUT = os.path.join(REPO, "tests", "golden", "gtc_kats.npz")
sys.path.insert(0, os.path.join(REPO, "tests"))

import gtc_util as gu  # noqa: E402


def _stub_modules():
    sb = types.ModuleType("seaborn")
    sb.set = lambda *a, **k: None
    sys.modules["seaborn"] = sb
    tc = types.ModuleType("termcolor")
    tc.colored = lambda s, *a, **k: s
    sys.modules["termcolor"] = tc
    import matplotlib
    matplotlib.use("Agg")


def cases():
    return [
        dict(name="plain_s10", n=300, n_states=300, s=10, seed=21),
        dict(name="old_keys_s3", n=257, n_states=257, s=3, seed=22, old_keys=True),       # arm_states / button_positions
        dict(name="cut_to_120_s5", n=300, n_states=120, s=5, seed=23),                    # --training-set-size 120
        dict(name="state_dim_1", n=200, n_states=200, s=1, seed=24),
        dict(name="relative_pos_s65", n=1031, n_states=1031, s=65, seed=25, relative_pos=True),  # the npz's own states are read
    ]


def _run_reference(path, argv, cwd):
    """The reference's file as __main__ with `argv`, from `cwd`."""
    old_cwd, old_argv = os.getcwd(), list(sys.argv)
    os.chdir(cwd)
    try:
        sys.argv = [os.path.basename(path)] + argv
        return runpy.run_path(path, run_name="__main__")
    finally:
        os.chdir(old_cwd)
        sys.argv = old_argv


def run_correlation(case):
    ds = gu.gtc_dataset(case)
    with tempfile.TemporaryDirectory() as root:
        log = gu.write_gtc_dataset(root, ds, case)
        _run_reference(os.path.join(REF, "plotting", "representation_plot.py"),
                       ["-i", log + "/states_rewards.npz", "--data-folder", "data/" + gu.DATASET, "--correlation", "--print-corr"], root)
        with open(os.path.join(root, log, "gt_correlation.json")) as f:
            result = json.load(f)
    gt_corr = np.array(result["gt_corr"], dtype=np.float64)
    assert gt_corr.shape == (6,) and np.isfinite(gt_corr).all(), (case["name"], gt_corr)
    return {"gt_corr": gt_corr, "gt_corr_mean": np.float64(result["gt_corr_mean"])}


def run_gather_results():
    with tempfile.TemporaryDirectory() as root:
        log_dir = gu.write_log_tree(root)
        _run_reference(os.path.join(REF, "evaluation", "gather_results.py"), ["-i", log_dir], root)
        return gu.read_csv(os.path.join(log_dir, "results.csv"))


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    out = {}
    cs = cases()
    for case in cs:
        rec = run_correlation(case)
        for k, v in rec.items():
            out["%s/%s" % (case["name"], k)] = v
        print("%-20s gt_corr %s mean %r" % (case["name"], rec["gt_corr"], float(rec["gt_corr_mean"])))
    table = run_gather_results()
    for row in table:
        print(row)
    out["results_table"] = np.array(json.dumps(table))
    out["cases"] = np.array(json.dumps(cs))
    import pandas
    out["numpy_version"] = np.array(np.__version__)
    out["pandas_version"] = np.array(pandas.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
