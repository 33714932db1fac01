"""plotting.representation_plot.plotCorrelation on the GPU against what the unmodified reference wrote into gt_correlation.json
(tests/golden/gtc_kats.npz, tools/make_golden_gtc.py), on the inputs tests/gtc_util.py regenerates from the recorded descriptors:
gt_corr and gt_corr_mean within (4 N + 16) 2^-53, N the case's row count (tests/gtc_util.py::bound: numpy's fp64 corrcoef and the
kernel each stay within it of the exact value), plus 2 units in the last place of the recorded value."""
import numpy as np
import pytest

import gtc_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return gu.load_golden()


def _tolerance(case, recorded):
    return gu.bound(case["n_states"]) + 2 * np.spacing(np.abs(recorded))


def test_fixture_has_every_case(golden):
    z, cases = golden
    assert len(cases) == 5
    assert any(c.get("old_keys") for c in cases) and any(c["n_states"] < c["n"] for c in cases) and any(c["s"] == 1 for c in cases)
    for c in cases:
        assert z[c["name"] + "/gt_corr"].shape == (6,)


@pytest.mark.parametrize("index", range(5))
def test_plot_correlation_is_the_reference(golden, index, tmp_path, monkeypatch, capsys):
    from plotting.representation_plot import plotCorrelation
    from utils import loadData
    z, cases = golden
    case = cases[index]
    ds = gu.gtc_dataset(case)
    log = gu.write_gtc_dataset(str(tmp_path), ds, case)
    monkeypatch.chdir(tmp_path)
    states_rewards = np.load(log + "/states_rewards.npz")
    assert states_rewards["states"].shape == (case["n_states"], case["s"]) and states_rewards["states"].dtype == np.float32
    _, ground_truth, _, target_positions = loadData(gu.DATASET)
    assert ("arm_states" in ground_truth.keys()) == bool(case.get("old_keys"))
    assert len(target_positions) == case["n"]
    gt_corr, gt_corr_mean = plotCorrelation(states_rewards, ground_truth, target_positions, only_print=True)
    want, want_mean = z[case["name"] + "/gt_corr"], float(z[case["name"] + "/gt_corr_mean"])
    assert gt_corr.shape == (6,) and gt_corr.dtype == np.float64
    err = np.abs(gt_corr - want)
    print("%s: worst error %.3e (tolerance %.3e), mean %.3e" % (case["name"], err.max(), _tolerance(case, want).min(),
                                                              abs(gt_corr_mean - want_mean)))
    assert (err <= _tolerance(case, want)).all(), (case["name"], err.max())
    assert abs(gt_corr_mean - want_mean) <= _tolerance(case, want_mean), (case["name"], gt_corr_mean, want_mean)
    out = capsys.readouterr().out
    assert "Correlation value of the model's prediction with the Ground Truth:" in out
    assert " Max correlation vector (GTC): " in out and " Mean : {:.2f}".format(want_mean) in out
