"""Host side of the ground-truth correlation (no GPU): the command line of plotting.representation_plot, pipeline.correlationCall's
argument list, evaluation.gather_results against the results.csv the unmodified reference wrote for the same log tree
(tests/golden/gtc_kats.npz, tools/make_golden_gtc.py) and the argument checks of ops.gt_correlation."""
import json
import os
import sys

import numpy as np
import pytest

import gtc_util as gu


def test_parser_carries_the_reference_flags():
    from plotting import representation_plot as rp
    a = rp.buildParser().parse_args([])
    assert (a.input_file, a.data_folder) == ("", "")
    assert not (a.color_episode or a.plot_against or a.pretty_plot_against or a.correlation or a.projection or a.print_corr)
    a = rp.parseArguments(["-i", "logs/x/states_rewards.npz", "--data-folder", "data/ds", "--correlation", "--print-corr"])
    assert (a.input_file, a.data_folder, a.correlation, a.print_corr) == ("logs/x/states_rewards.npz", "ds", True, True)
    a = rp.parseArguments(["--input-file", "f.npz", "--data-folder", "ds", "--print-corr"])
    assert a.correlation is True  # --print-corr forces --correlation
    a = rp.parseArguments(["--data-folder", "ds", "--color-episode", "--plot-against", "--pretty-plot-against", "--projection"])
    assert a.color_episode and a.plot_against and a.pretty_plot_against and a.projection and not a.correlation
    with pytest.raises(AssertionError):
        rp.parseArguments(["-i", "f.npz", "--correlation"])  # needs a data folder
    with pytest.raises(AssertionError):
        rp.parseArguments(["-i", "f.npz", "--color-episode"])
    with pytest.raises(SystemExit):
        rp.buildParser().parse_args(["--no-such-flag"])


@pytest.mark.parametrize("argv", [["-i", "f.npz", "--plot-against"], ["-i", "f.npz", "--pretty-plot-against"],
                                  ["-i", "f.npz", "--data-folder", "ds", "--projection"], ["-i", "f.npz"], ["--data-folder", "ds"],
                                  ["-i", "f.npz", "--data-folder", "ds", "--correlation", "--plot-against"]])
def test_plot_flags_parse_then_stop(argv, capsys):
    from plotting import representation_plot as rp
    assert rp.main(argv) != 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1 and "plots are outside this build" in lines[0]


def test_nothing_to_do_without_input_and_data_folder(capsys):
    from plotting import representation_plot as rp
    assert rp.main([]) == 0
    assert "You must specify one of --input-file or --data-folder" in capsys.readouterr().out


@pytest.mark.parametrize("plot,tail", [(False, ["--print-corr"]), (True, [])])
def test_correlation_call_passes_the_reference_arguments(monkeypatch, plot, tail):
    import subprocess
    import pipeline
    cfg = {"log-folder": "logs/ds/run", "data-folder": "ds"}
    seen = {}

    def fake_call(cmd, **kw):
        seen["cmd"], seen["kw"] = list(cmd), kw
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    pipeline.correlationCall(cfg, plot=plot)
    assert seen["cmd"] == [sys.executable, "-m", "plotting.representation_plot", "-i", "logs/ds/run/states_rewards.npz",
                           "--data-folder", "data/ds", "--correlation"] + tail
    pkg = os.path.dirname(os.path.abspath(pipeline.__file__))
    assert seen["kw"]["env"]["PYTHONPATH"].split(os.pathsep)[0] == pkg  # the child finds the package from any working directory
    # the child's own parser takes that list
    from plotting.representation_plot import parseArguments
    a = parseArguments(seen["cmd"][3:])
    assert (a.input_file, a.data_folder, a.correlation, a.print_corr) == ("logs/ds/run/states_rewards.npz", "ds", True, not plot)
    monkeypatch.setattr(subprocess, "call", lambda cmd, **kw: 1)
    with pytest.raises(RuntimeError):
        pipeline.correlationCall(cfg)


def test_gather_results_writes_the_reference_table(tmp_path, monkeypatch, capsys):
    import subprocess
    from evaluation import gather_results
    z, _ = gu.load_golden()
    want = json.loads(str(z["results_table"]))
    log_dir = gu.write_log_tree(str(tmp_path))

    def no_child(*a, **k):
        raise AssertionError("every result file is present: nothing is to be launched (%s)" % (a,))
    monkeypatch.setattr(subprocess, "call", no_child)
    assert gather_results.main(["-i", log_dir]) == 0
    got = gu.read_csv(os.path.join(log_dir, "results.csv"))
    assert got[0] == want[0] == ['training-set-size', 'split-dimensions', 'state-dim', 'seed', 'losses_weights', 'experiments',
                                 'knn_mse', 'gt_corr', 'gt_mean']
    assert [row[5] for row in got[1:]] == [row[5] for row in want[1:]] and len(got) == 6
    assert "baselines/ground_truth" in [row[5] for row in got] and "no_config" in [row[5] for row in got]
    for grow, wrow in zip(got, want):
        assert len(grow) == len(wrow)
        for column, g, w in zip(got[0], grow, wrow):
            assert gu.same_cell(g, w), (wrow[5], column, g, w)
    out = capsys.readouterr().out
    assert "Found 5 experiments" in out and "exp_config not found for no_config" in out and "knn_mse.json not found" in out


def test_gather_results_fills_in_missing_files_through_the_pipeline(tmp_path, monkeypatch):
    """A missing gt_correlation.json / knn_mse.json: correlationCall / knnCall, then predict_dataset and one more try."""
    import subprocess
    from evaluation import gather_results
    log_dir = gu.write_log_tree(str(tmp_path))
    exp = os.path.join(log_dir, "18-01-01_10h00_00_custom_cnn_ST_DIM10_autoencoder")
    os.remove(os.path.join(exp, "gt_correlation.json"))
    os.remove(os.path.join(exp, "knn_mse.json"))
    cfg = json.load(open(os.path.join(exp, "exp_config.json")))
    cfg.update({"log-folder": exp, "knn-seed": 1, "knn-samples": 200, "n-neighbors": 5, "n-to-plot": 5})
    json.dump(cfg, open(os.path.join(exp, "exp_config.json"), "w"))
    modules = []

    def fake_call(cmd, **kw):
        assert cmd[0] == sys.executable and cmd[1] == "-m" and "env" in kw
        modules.append(cmd[2])
        if cmd[2] == "evaluation.predict_dataset":
            assert cmd[3:] == ["--name-suffix", "", "-n", "-1", "--log-dir", exp]
            return 0
        if modules.count(cmd[2]) == 1:
            return 1  # the first try fails: states_rewards.npz is missing
        name = "gt_correlation.json" if cmd[2] == "plotting.representation_plot" else "knn_mse.json"
        json.dump({"gt_corr": [0.5], "gt_corr_mean": 0.5, "knn_mse": 0.25}, open(os.path.join(exp, name), "w"))
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    assert gather_results.main(["-i", log_dir]) == 0
    assert modules == ["plotting.representation_plot", "evaluation.predict_dataset", "plotting.representation_plot",
                       "evaluation.knn_images", "evaluation.predict_dataset", "evaluation.knn_images"]
    rows = gu.read_csv(os.path.join(log_dir, "results.csv"))
    row = dict(zip(rows[0], rows[1]))
    assert (float(row["gt_mean"]), row["gt_corr"], float(row["knn_mse"])) == (0.5, "[0.5]", 0.25)


@pytest.mark.parametrize("kind", ["offset100", "offset1e4"])
def test_the_bound_tells_the_one_pass_form_apart(kind):
    """What the bound is for: fp64 sum x y - sum x sum y / N on the offset inputs is off by far more than it allows."""
    n, g, s, dtype = 4099, 3, 5, {"offset100": "f32", "offset1e4": "f64"}[kind]
    gt, states = gu.kernel_input(n, g, s, dtype, kind)
    rcorr, _ = gu.reference_rows(gt, states)
    both = np.concatenate([gt, states.astype(np.float64)], 1)
    sx, sxy = both.sum(0), both[:, :g].T.dot(both)
    cov = sxy - np.outer(sx[:g], sx) / n
    var = (both * both).sum(0) - sx * sx / n
    one_pass = cov / np.sqrt(var[:g, None]) / np.sqrt(var[None, :])
    assert float(np.abs(one_pass - rcorr).max()) > 1e3 * gu.bound(n)


def test_ops_gt_correlation_rejects_bad_input_before_touching_a_device(monkeypatch):
    import torch
    from srlz import ops

    def no_device(*a, **k):
        raise AssertionError("ops.gt_correlation asked for a device before it validated its input")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    gt, states = gu.kernel_input(20, 3, 4, "f32", "plain")
    bad = states.copy()
    bad[4, 1] = np.nan
    with pytest.raises(ValueError):
        ops.gt_correlation(gt, bad)
    bad_gt = gt.copy()
    bad_gt[0, 0] = np.inf
    with pytest.raises(ValueError):
        ops.gt_correlation(bad_gt, states)
    with pytest.raises(ValueError):
        ops.gt_correlation(gt, states[:19])  # mismatched N
    with pytest.raises(ValueError):
        ops.gt_correlation(gt[:1], states[:1])  # N = 1
    with pytest.raises(ValueError):
        ops.gt_correlation(np.zeros((20, 17)), states)  # G = 17
    with pytest.raises(ValueError):
        ops.gt_correlation(gt, np.zeros((20, 0), dtype=np.float32))  # S = 0
    with pytest.raises(ValueError):
        ops.gt_correlation(gt[:, 0], states)  # not 2-D
    with pytest.raises(ValueError):
        ops.gt_correlation(gt, torch.from_numpy(states).to(torch.float16))


def test_ops_gt_correlation_needs_a_gpu(monkeypatch):
    """No CPU fallback: without a device the project's usual RuntimeError."""
    import torch
    from srlz import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    gt, states = gu.kernel_input(20, 3, 4, "f32", "plain")
    with pytest.raises(RuntimeError):
        ops.gt_correlation(gt, states)
