"""srl_baselines.ipca.IncrementalPCA over the cases of tests/golden/pca_kats.npz, minibatch by minibatch, against what sklearn's
IncrementalPCA recorded from the same frames (tools/make_golden_pca.py).

Bound: max(1e-4, 10 x the case's recorded spread) of each quantity's scale (tests/pca_util.py::tolerance) — 1e-4 is the project's
parity bound for outputs, the spread is how far sklearn's float32 run lies from its own float64 run, and the factor 10 covers
float32 LAPACK (and float32 centring) against the fp64 Gram route.  The largest error seen is printed."""
import pickle

import numpy as np
import pytest
import torch

import pca_util as pu

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PER_BATCH = ("singular_values_", "explained_variance_", "explained_variance_ratio_", "noise_variance_")


@pytest.fixture(scope="module")
def kats():
    return pu.load_kats()


def rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("form", ["u8", "f32"])
@pytest.mark.parametrize("case", pu.CASES, ids=pu.case_name)
def test_fit_follows_sklearn_minibatch_by_minibatch(kats, case, form):
    from srl_baselines.ipca import IncrementalPCA
    name = pu.case_name(case)
    N, C, W, H, bs, k = case
    tol = pu.tolerance(pu.load_spread()[name])
    frames, cols = kats[name + "/frames"], kats[name + "/cols"]
    if form == "u8":
        on_device = torch.from_numpy(frames).to(DEV)
    else:  # the normalised float tensor [N, C, W, H], as a float loader would ship it
        on_device = torch.from_numpy(pu.normalised(frames, kats["lut"]).astype(np.float32).reshape(frames.shape)).to(DEV)
    ipca = IncrementalPCA(k)
    worst = {}
    i = 0
    for b in pu.minibatches(N, bs):
        if len(b) == 0:  # the trailing empty range: skipped (sklearn raises on it)
            continue
        ipca.partial_fit(on_device[int(b[0]):int(b[-1]) + 1])
        got = {"components_": ipca.components_[:, cols], "mean_": ipca.mean_[cols], "var_": ipca.var_[cols]}
        got.update({f: getattr(ipca, f) for f in PER_BATCH})
        for f, v in got.items():
            want = kats["%s/batch%d/%s" % (name, i, f)]
            assert np.shape(v) == want.shape, f
            if f == "noise_variance_":
                # the mean of the DISCARDED explained variances: measured on the explained variances' scale.  (On its own scale it
                # pins nothing where the discarded singular values are rounding noise — the first minibatch of m = k + 1 centred
                # rows has rank k: sklearn's float32 LAPACK returns 1e-7 of the largest there, the fp64 route an exact zero.)
                err = abs(float(v) - float(want)) / np.abs(kats["%s/batch%d/explained_variance_" % (name, i)]).max()
            else:
                err = rel(v, want)
            worst[f] = max(worst.get(f, 0.0), err)
        assert ipca.n_samples_seen_ == int(kats["%s/batch%d/n_samples_seen_" % (name, i)]) and ipca.n_components_ == k
        i += 1
    assert i == int(kats[name + "/n_batches"])
    worst["components_ (all columns)"] = rel(ipca.components_, kats[name + "/final/components_"])
    worst["mean_ (all columns)"] = rel(ipca.mean_, kats[name + "/final/mean_"])
    # sklearn's dtypes for float32 frames after more than one minibatch
    assert ipca.components_.dtype == ipca.singular_values_.dtype == ipca.mean_.dtype == ipca.var_.dtype == np.float64
    assert ipca.explained_variance_.dtype == ipca.explained_variance_ratio_.dtype == np.float64
    want = kats[name + "/final/states"]
    states = ipca.transform(on_device)
    assert states.shape == want.shape and states.dtype == np.float32
    worst["states"] = rel(states, want)
    # the pickle carries numpy arrays only, and transforms the same frames on the host
    blob = pickle.dumps(ipca)
    again = pickle.loads(blob)
    assert again._dev is None and all(isinstance(v, (np.ndarray, np.generic, int)) for v in again._host.values())
    worst["states (unpickled, host)"] = rel(again.transform(frames), want)
    assert rel(again.transform(frames), states.astype(np.float64)) <= 1e-6  # host and device transform agree to fp32 rounding
    print("%s %s: largest errors over all minibatches (bound %.1e): %s" % (name, form, tol, {f: "%.2e" % v for f, v in worst.items()}))
    for f, v in worst.items():
        assert v <= tol, "%s: %.3e of scale > %.1e" % (f, v, tol)


def test_first_minibatch_alone_has_sklearn_float32_dtypes_and_rejections(kats):
    from srl_baselines.ipca import IncrementalPCA
    name = pu.case_name(pu.CASES[0])
    frames = torch.from_numpy(kats[name + "/frames"]).to(DEV)
    ipca = IncrementalPCA(3).partial_fit(frames[:4])
    assert ipca.components_.dtype == ipca.singular_values_.dtype == ipca.explained_variance_.dtype == np.float32
    assert ipca.mean_.dtype == ipca.var_.dtype == ipca.explained_variance_ratio_.dtype == np.float64
    assert rel(ipca.singular_values_, kats[name + "/batch0/singular_values_"]) <= 1e-4
    with pytest.raises(ValueError, match="first partial_fit"):
        IncrementalPCA(5).partial_fit(frames[:4])
    with pytest.raises(ValueError, match="n_features"):
        IncrementalPCA(3).partial_fit(frames[:4, :1, :1, :2].float())
    with pytest.raises(ValueError, match="features has changed"):
        ipca.partial_fit(frames[:4].float().reshape(4, -1)[:, :100])


def test_fewer_distinct_frames_than_components_gives_zero_rows(kats, capsys):
    """Three copies of two frames, k = 3: one component has no singular value — a zero row and zero states, never a NaN."""
    from srl_baselines.ipca import IncrementalPCA
    name = pu.case_name(pu.CASES[0])
    two = torch.from_numpy(kats[name + "/frames"][:2]).to(DEV)
    frames = torch.cat([two, two, two])
    ipca = IncrementalPCA(3).partial_fit(frames)
    assert "no singular value" in capsys.readouterr().out
    assert np.isfinite(ipca.components_).all() and not ipca.components_[1:].any() and ipca.singular_values_[0] > 0
    assert not ipca.singular_values_[1:].any()
    states = ipca.transform(frames)
    assert np.isfinite(states).all() and not states[:, 1:].any() and np.abs(states[:, 0]).max() > 0
