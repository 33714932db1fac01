"""Host side of the evaluation (no GPU): the numpy oracle of the GPU tests against the reference's ball tree, the sampled test images,
the KNN-MSE error loop, the pre-processing of --ground-truth / --relative-pos, the command lines, pipeline.knnCall's argument list and
the argument checks of ops.knn — all against tests/golden/knn_kats.npz, recorded from the unmodified reference
(tools/make_golden_eval.py)."""
import json
import os
import sys

import numpy as np
import pytest

import knn_util as ku


@pytest.fixture(scope="module")
def golden():
    return ku.load_golden()


def _searched(case, ds):
    return ds["true_states"] if case["kind"] == "ground-truth" else ds["states"]


def _true_states(case, ds):
    from evaluation import knn_images
    if case["kind"] == "relative-pos":
        return knn_images.relativePositions(ds["true_states"], ds["target_positions"], ds["episode_starts"])
    return ds["true_states"]


def test_fixture_has_every_case(golden):
    z, cases = golden
    assert len(cases) == 22
    assert sorted(set((c["n"], c["d"]) for c in cases if c["kind"] == "plain")) == sorted(ku.SEEDED_SHAPES)
    assert {c["kind"] for c in cases} == {"plain", "ground-truth", "relative-pos"}
    for c in cases:
        assert float(z[c["name"] + "/min_gap"]) > 1e-9


def test_brute_knn_is_the_ball_tree(golden):
    """The oracle of the GPU tests returns the reference's neighbours: indices exactly, distances to 1e-12 relative."""
    z, cases = golden
    cache = {}
    for c in cases:
        key = (c["n"], c["d"], c["kind"] == "ground-truth")
        if key not in cache:
            s = _searched(c, ku.eval_dataset(c["n"], c["d"], c["kind"]))
            cache[key] = (s,) + ku.brute_knn(s, s, c["k"] + 1)
        s, idx, d2 = cache[key]
        picks = z[c["name"] + "/picks"]
        assert np.array_equal(idx[picks], z[c["name"] + "/neighbors"]), c["name"]
        np.testing.assert_allclose(np.sqrt(d2[picks]), z[c["name"] + "/distances"], rtol=1e-12, atol=0, err_msg=c["name"])
        # the sampled rows as queries give the same rows as the search over all rows
        qi, qd2 = ku.brute_knn(s, s[picks[:7]], c["k"] + 1)
        assert np.array_equal(qi, idx[picks[:7]]) and np.array_equal(qd2, d2[picks[:7]])


def test_sample_indices_are_the_reference_picks(golden):
    from evaluation.knn_images import sampleIndices
    z, cases = golden
    for c in cases:
        picks = sampleIndices(c["n"], c["n_samples"], c["seed"])
        assert len(picks) == min(c["n"], c["n_samples"])
        assert list(picks) == list(z[c["name"] + "/picks"]), c["name"]
    assert len(sampleIndices(3, 200, 1)) == 3  # capped to N by min


def test_knn_mse_on_recorded_neighbours(golden):
    from evaluation.knn_images import knnMse, resultDict
    z, cases = golden
    for c in cases:
        ds = ku.eval_dataset(c["n"], c["d"], c["kind"])
        titles, mean_error = knnMse(_true_states(c, ds), ds["images_path"], z[c["name"] + "/picks"], z[c["name"] + "/neighbors"], c["k"])
        want = float(z[c["name"] + "/mean_error"])
        assert abs(mean_error - want) <= 1e-12 * abs(want), (c["name"], mean_error, want)
        res = resultDict(titles, mean_error)
        assert res["knn_mse"] == float(z[c["name"] + "/knn_mse"]), c["name"]
        assert res["images"] == [str(t) for t in z[c["name"] + "/titles"]], c["name"]
        assert json.loads(json.dumps(res)) == res


def test_relative_pos_and_ground_truth_preprocessing(golden, tmp_path, monkeypatch):
    from evaluation import knn_images
    z, cases = golden
    by_kind = {c["kind"]: c for c in cases}
    c = by_kind["relative-pos"]
    ds = ku.eval_dataset(c["n"], c["d"], c["kind"])
    log = ku.write_eval_dataset(str(tmp_path), ds)
    monkeypatch.chdir(tmp_path)
    states, true_states, images_path = knn_images.loadEvaluationInputs(log, relative_pos=True)
    assert np.array_equal(states, ds["states"]) and list(images_path) == list(ds["images_path"])
    assert np.array_equal(true_states[:60:7], z[c["name"] + "/true_states_head"])
    assert abs(true_states.sum() - float(z[c["name"] + "/true_states_sum"])) <= 1e-12 * abs(true_states.sum())
    assert np.array_equal(np.load("data/knn_kats/ground_truth.npz")["ground_truth_states"], ds["true_states"])  # the file is untouched
    # --ground-truth: the search runs on the dataset's float64 states, unrounded
    c = by_kind["ground-truth"]
    ds = ku.eval_dataset(c["n"], c["d"], c["kind"])
    log = ku.write_eval_dataset(str(tmp_path), ds, log_folder="logs/knn_kats/gt")
    states, true_states, _ = knn_images.loadEvaluationInputs(log, ground_truth=True)
    assert states.dtype == np.float64 and np.array_equal(states, ds["true_states"]) and states is not true_states
    assert not np.array_equal(states, states.astype(np.float32))
    # the older key spellings
    np.savez("data/knn_kats/ground_truth.npz", images_path=ds["images_path"], arm_states=ds["true_states"],
             button_positions=ds["target_positions"])
    states2, true2, _ = knn_images.loadEvaluationInputs(log, relative_pos=True, ground_truth=True)
    assert np.array_equal(true2, knn_images.relativePositions(ds["true_states"], ds["target_positions"], ds["episode_starts"]))
    assert np.array_equal(states2, true2)


def test_parsers_carry_the_reference_flags():
    from evaluation import knn_images, predict_dataset
    with pytest.raises(SystemExit):
        knn_images.buildParser().parse_args([])  # --log-folder is required
    a = knn_images.buildParser().parse_args(["--log-folder", "x"])
    assert (a.log_folder, a.seed, a.n_neighbors, a.n_samples, a.n_to_plot) == ("x", 1, 5, 5, 5)
    assert (a.relative_pos, a.ground_truth, a.multi_view) == (False, False, False)
    a = knn_images.buildParser().parse_args(["--log-folder", "x", "-k", "3", "-n", "9", "--seed", "4", "--n-to-plot", "0",
                                             "--relative-pos", "--ground-truth", "--multi-view"])
    assert (a.n_neighbors, a.n_samples, a.seed, a.n_to_plot, a.relative_pos, a.ground_truth, a.multi_view) == (3, 9, 4, 0, True, True, True)
    a = knn_images.buildParser().parse_args(["--log-folder", "x", "--n-neighbors", "2", "--n-samples", "8"])
    assert (a.n_neighbors, a.n_samples) == (2, 8)
    with pytest.raises(SystemExit):
        predict_dataset.buildParser().parse_args([])  # -i is required
    p = predict_dataset.buildParser().parse_args(["-i", "logs/x"])
    assert (p.log_dir, p.name_suffix, p.no_cuda, p.n_samples) == ("logs/x", "_test", False, -1)
    p = predict_dataset.buildParser().parse_args(["--log-dir", "y", "--name-suffix", "_b", "--no-cuda", "--n-samples", "17"])
    assert (p.log_dir, p.name_suffix, p.no_cuda, p.n_samples) == ("y", "_b", True, 17)
    assert predict_dataset.VALID_MODELS == ["forward", "inverse", "reward", "episode-prior", "reward-prior", "triplet",
                                            "autoencoder", "vae"]


def test_states_stats():
    from evaluation.predict_dataset import statesStats
    s = np.random.RandomState(5).randn(17, 4).astype(np.float32)
    st = statesStats(s)
    assert sorted(st) == ["max", "mean", "min", "std"]
    assert np.array_equal(st["mean"], s.mean(0)) and np.array_equal(st["std"], s.std(0))
    assert np.array_equal(st["min"], s.min(0)) and np.array_equal(st["max"], s.max(0))


@pytest.mark.parametrize("extra,flags", [({}, []), ({"ground-truth": True}, ["--ground-truth"]), ({"multi-view": True}, ["--multi-view"]),
                                         ({"relative-pos": True}, ["--relative-pos"])])
def test_knn_call_passes_the_reference_arguments(tmp_path, monkeypatch, extra, flags):
    import subprocess
    import pipeline
    monkeypatch.chdir(tmp_path)
    log = "logs/ds/run"
    os.makedirs(log)
    cfg = {"log-folder": log, "knn-seed": 3, "knn-samples": 200, "n-neighbors": 5, "n-to-plot": 5, "data-folder": "ds"}
    cfg.update(extra)
    seen = {}

    def fake_call(cmd, **kw):
        seen["cmd"], seen["kw"] = list(cmd), kw
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    pipeline.knnCall(cfg)
    assert seen["cmd"] == [sys.executable, "-m", "evaluation.knn_images", "--seed", "3", "--n-samples", "200"] + flags + \
        ["--log-folder", log, "--n-neighbors", "5", "--n-to-plot", "5"]
    assert os.path.isdir(os.path.join(log, "NearestNeighbors"))
    pkg = os.path.dirname(os.path.abspath(pipeline.__file__))
    assert seen["kw"]["env"]["PYTHONPATH"].split(os.pathsep)[0] == pkg  # the child finds the package from any working directory
    # the child's own parser takes that list
    from evaluation.knn_images import buildParser
    a = buildParser().parse_args(seen["cmd"][3:])
    assert (a.seed, a.n_samples, a.n_neighbors, a.n_to_plot, a.log_folder) == (3, 200, 5, 5, log)
    monkeypatch.setattr(subprocess, "call", lambda cmd, **kw: 7)
    with pytest.raises(RuntimeError):
        pipeline.knnCall(cfg)


def test_ground_truth_folder_and_relative_position(tmp_path, monkeypatch):
    import pipeline
    monkeypatch.chdir(tmp_path)
    os.makedirs("data/ds")
    with open("data/ds/dataset_config.json", "w") as f:
        json.dump({"relative_pos": True}, f)
    assert pipeline.useRelativePosition("ds") is True
    with open("data/ds/dataset_config.json", "w") as f:
        json.dump({}, f)
    assert pipeline.useRelativePosition("ds") is False
    cfg = pipeline.createGroundTruthFolder({"data-folder": "ds", "knn-seed": 1})
    assert cfg["log-folder"] == "logs/ds/baselines/ground_truth/" and cfg["ground-truth"] is True
    assert json.load(open("logs/ds/baselines/ground_truth/exp_config.json"))["ground-truth"] is True


def test_ops_knn_rejects_bad_input_before_touching_a_device(monkeypatch):
    import torch
    from srlz import ops

    def no_device(*a, **k):
        raise AssertionError("ops.knn asked for a device before it validated its input")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    db = ku.seeded_input(20, 3)
    bad = db.copy()
    bad[4, 1] = np.nan
    with pytest.raises(ValueError):
        ops.knn(bad, 2)
    bad[4, 1] = np.inf
    with pytest.raises(ValueError):
        ops.knn(db, 2, queries=bad)
    with pytest.raises(ValueError):
        ops.knn(db, 2, queries=ku.seeded_input(5, 4))  # mismatched D
    with pytest.raises(ValueError):
        ops.knn(db, 21)  # k > N
    with pytest.raises(ValueError):
        ops.knn(db, 0)
    with pytest.raises(ValueError):
        ops.knn(torch.from_numpy(db).to(torch.float16), 2)


def test_ops_knn_needs_a_gpu(monkeypatch):
    """No CPU fallback: without a device the project's usual RuntimeError."""
    import torch
    from srlz import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError):
        ops.knn(ku.seeded_input(20, 3), 2)
