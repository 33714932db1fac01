"""evaluation.predict_reward end to end against the runs recorded from the unmodified reference (tests/golden/reward_probe.npz,
tools/make_golden.py reward_probe): main([...]) in-process after torch.manual_seed(preseed), on the regenerated dataset — with the
float rewards tests/dataset_util.make_dataset stores, which the reference itself cannot read.

The rule (the PCA baseline's, tests/test_pca_fit_gpu.py): every per-epoch loss and the final parameters lie within
max(1e-4, 10 x the recorded spread) of the quantity's scale, the spread being the reference's own float32-to-float64 distance
(tests/golden/reward_probe_spread.json).  Accuracies are compared as counts; a row whose float64 logit margin is below
1e-4 * max|z| may count either way (at most 1 % of a phase's rows, asserted on the float64 side).

Measured on one MI355X (both runs, 10 epochs at -bs 8): losses within 7.9e-8 relative of the reference's, parameters within 3.1e-8
by the end-point measure, the trained model's logits within 2.9e-7, every count equal."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util
import reward_util as ru

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "srl-zoo_amd")


def bound(spread, key):
    return max(1e-4, 10.0 * spread[key])


@pytest.fixture(scope="module")
def fixture():
    return ru.load_fixture()


@pytest.fixture(scope="module")
def float64_runs(fixture):
    """The float64 trajectory of every recorded run over its own minibatch order: computed once, read by the tests."""
    out = {}
    for case in ru.CASES:
        pre = case["name"] + "/"
        flat = ru.flatten_state_dict({k: fixture[pre + "init/" + k] for k in ru.KEYS})
        states = np.asarray(ru.case_states(case), dtype=np.float32)
        labels = np.maximum(ru.case_arrays(case)["rewards"], 0).astype(np.int64)
        m, v, t, phases = np.zeros_like(flat), np.zeros_like(flat), 0, []
        for train, val in ru.replay_tables(fixture[pre + "indices"], case["seed"], case["bs"], case["epochs"]):
            flat, m, v, ph, _ = ru.fit(flat, m, v, t, states, labels, train, case["lr"])
            t += len(train)
            phases.append((ph, ru.evaluate(flat, states, labels, val)))
        out[case["name"]] = dict(flat=flat, phases=phases, steps=t, states=states)
    return out


@pytest.mark.parametrize("case", ru.CASES, ids=[c["name"] for c in ru.CASES])
def test_recorded_run(case, fixture, float64_runs, tmp_path, monkeypatch, capsys):
    from evaluation import predict_reward
    pre = case["name"] + "/"
    spread = ru.load_spread()["cases"][case["name"]]
    argv = ru.write_case(str(tmp_path), case)  # float rewards: the cast to int64 is this build's
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(case["preseed"])
    result = predict_reward.main(argv, full=True)
    records = result.records
    text = capsys.readouterr().out

    # init order and RNG: the parameters the run starts from are the reference's, bit for bit
    for k in ru.KEYS:
        assert np.array_equal(result.initial_state[k].numpy(), fixture[pre + "init/" + k]), k
    assert list(result.model.state_dict().keys()) == list(ru.KEYS)

    sizes = fixture[pre + "phase_sizes"]
    f64 = float64_runs[case["name"]]
    worst_loss, any_soft = 0.0, False
    for e, rec in enumerate(records):
        for j, phase in enumerate(("train", "val")):
            r = rec[phase]
            assert r["n_samples"] == sizes[j] and r["n_batches"] == fixture[pre + "n_batches"][e, j]
            ref = fixture[pre + "loss"][e, j]
            err = abs(r["loss"] - ref) / abs(ref)
            worst_loss = max(worst_loss, err)
            assert err <= bound(spread, "loss"), (e, phase, r["loss"], ref)
            ph = f64["phases"][e][j]
            lo, hi, soft = ph.bounds()
            assert soft <= 0.01 * r["n_batches"] * case["bs"]
            got = np.array(r["counts"])
            assert (lo <= got).all() and (got <= hi).all(), (e, phase, got, lo, hi)
            any_soft = any_soft or soft > 0
            if soft == 0:  # then the reference's own counts are the float64 ones, and ours
                assert np.array_equal(got, fixture[pre + "counts"][e, j]), (e, phase, got, fixture[pre + "counts"][e, j])
                assert r["acc"] == fixture[pre + "acc"][e, j]
                assert np.array_equal(r["acc_per_class"], fixture[pre + "acc_per_class"][e, j], equal_nan=True)
    # final parameters and the trained model's logits on the first validation minibatch, by the end-point measure of the spread file
    sd = result.model.state_dict()
    flat = ru.flatten_state_dict(sd)
    logits = ru.forward(flat, ru.rows(f64["states"], fixture[pre + "eval_states/idx"]))[2]
    g = {k: fixture[pre + k] for k in ("final/names", "final/sums", "final/abss", "eval_states/full")}
    worst, _ = golden_util.endpoint_errors(sd, g, case["lr"], f64["steps"], logits)
    print("%s: loss %.2e param %.2e logits %.2e" % (case["name"], worst_loss, worst["param"], worst["eval_states"]))
    assert worst["param"] <= bound(spread, "param"), worst
    assert worst["eval_states"] <= bound(spread, "eval_states"), worst
    # the printed lines are the reference's, value for value at four decimals
    printed = re.findall(r"^(?:train|val) Loss: (\S+) Acc: (\S+)$", text, re.M)
    assert len(printed) == 2 * case["epochs"]
    assert np.abs(np.array([float(p[0]) for p in printed]).reshape(-1, 2) - fixture[pre + "printed/loss"]).max() <= 1.0001e-4
    if not any_soft:
        assert result.best_acc == float(fixture[pre + "best_val_acc"])


def test_command_line(tmp_path):
    case = dict(ru.CASES[0], epochs=2)
    argv = ru.write_case(str(tmp_path), case)
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    out = subprocess.run([sys.executable, "-m", "evaluation.predict_reward"] + argv, cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stdout
    assert re.findall(r"^Epoch (\d+)/(\d+)$", text, re.M) == [("1", "1"), ("2", "1")]
    assert len(re.findall(r"^(train|val) Loss: \d+\.\d{4} Acc: \d\.\d{4}$", text, re.M)) == 4
    assert len(re.findall(r"^Accuracy per class: (\d\.\d{4}|nan) (\d\.\d{4}|nan)$", text, re.M)) == 4
    assert re.search(r"^Training complete in \d+m \d+s$", text, re.M)
    best = re.search(r"^Best val Acc: (\d\.\d{6})$", text, re.M)
    assert best and 0.0 <= float(best.group(1)) <= 1.0
    assert "Using ground truth" in text and re.search(r"^\d+ samples$", text, re.M)
