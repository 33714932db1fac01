"""evaluation.enjoy_latent against the UNMODIFIED reference script (tests/golden/enjoy_kats.npz, tools/make_golden_enjoy.py): each
fixture model is rebuilt from its seed, written to a log folder and shown through main(gui=<scripted backend>) with the fixture's
slider script.

States equal the fixture's bit for bit; nearest-frame ticks choose the fixture's paths; shown images match the fixture's stride-4
subsample and its fp64 sums within  max(1e-4, 10 x the case's float32-to-float64 spread of the reference)  — images live in [0, 1],
1e-4 is the project's bar for outputs, the allowance is the one of tests/test_pca_fit_gpu.py.  The recorded spreads
(tests/golden/enjoy_spread.json) are 5.5e-7 (cnn_ae), 6.2e-7 (cnn_vae), 6.0e-7 (split_ae_inverse) and 7.4e-8 (mlp_ae), so the bound is
1e-4 for every case.  The sums are over 150528 values: |sum - sum'| <= 150528 * tol, |sumsq - sumsq'| <= 2 * 150528 * tol.

The mlp case: the reference's script dies on a dense auto-encoder (recorded as reference_error); its fixture images are the
reference's model and deNormalize with the flat vector viewed as the image, as this build shows it.
"""
import os

import numpy as np
import pytest
import torch

import enjoy_util as eu

pytestmark = pytest.mark.gpu

N_VALUES = 224 * 224 * 3


@pytest.fixture(scope="module")
def golden():
    return eu.load_golden()


@pytest.fixture(scope="module")
def enjoy():
    from evaluation import enjoy_latent
    return enjoy_latent


def _build(case, root):
    """The fixture's model from its seed on the GPU -> (log folder with a trailing slash, SRL4robotics)"""
    import preprocessing.preprocess as pre
    from models.learner import SRL4robotics
    pre.N_CHANNELS = 3
    log = os.path.join(str(root), "logs", case["name"]) + "/"
    srl = SRL4robotics(case["state_dim"], model_type=case["model_type"], seed=case["seed"], cuda=True, losses=case["losses"],
                       n_actions=eu.N_ACTIONS, split_dimensions=eu.split_dimensions(case), log_folder=log)
    sd = {k: v.detach().cpu().clone() for k, v in srl.model.state_dict().items()}
    eu.write_log_folder(log, case, sd, torch.save)
    return log, srl, sd


@pytest.fixture(scope="module")
def sessions(golden, enjoy, tmp_path_factory):
    """One scripted session of main() per case, run once: {name: (gui, state_dict as built)}"""
    root = tmp_path_factory.mktemp("enjoy_golden")
    out = {}
    cwd = os.getcwd()
    os.chdir(str(root))
    try:
        for case in eu.CASES:
            log, _, sd = _build(case, root)
            gui = eu.ScriptedGui(eu.case_script(case))
            enjoy.main(["--log-dir", log], gui=gui)
            out[case["name"]] = (gui, sd)
    finally:
        os.chdir(cwd)
    return out


@pytest.mark.parametrize("name", [c["name"] for c in eu.CASES])
def test_seeded_model_is_the_fixtures(golden, sessions, name):
    z, _ = golden
    sums, abss = eu.state_dict_digest(sessions[name][1])
    assert list(z[name + "/sd_names"]) == list(sessions[name][1].keys())
    np.testing.assert_allclose(sums, z[name + "/sd_sums"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(abss, z[name + "/sd_abss"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", [c["name"] for c in eu.CASES])
def test_session_follows_the_reference(golden, sessions, name):
    z, spread = golden
    gui = sessions[name][0]
    case = eu.case_by_name(name)
    tol = max(1e-4, 10 * spread[name])
    assert gui.destroyed and gui.tick == len(gui.script)
    want_windows = []
    for loss, start, end in eu.case_blocks(case):
        want_windows += [eu.figure_name(loss), "slider for " + eu.figure_name(loss)]
    assert gui.windows == want_windows
    assert list(z[name + "/windows"]) == want_windows
    assert ((name + "/reference_error") in z.files) == (case["model_type"] != "custom_cnn")
    assert [(t[0], t[2], t[3]) for t in gui.trackbars] == [(str(i), 50, 100) for loss, s, e in eu.case_blocks(case) for i in range(e - s)]
    assert len(gui.shown) == int(z[name + "/n_shown"])
    reads = list(gui.reads)
    worst = 0.0
    for i, rec in enumerate(gui.shown):
        key = "%s/shown%02d/" % (name, i)
        assert rec["tick"] == int(z[key + "tick"]) and rec["name"] == str(z[key + "name"])
        assert np.asarray(rec["state"], dtype=np.float64).tobytes() == z[key + "state"].tobytes()
        assert np.asarray(rec["full_state"], dtype=np.float64).tobytes() == z[key + "full_state"].tobytes()
        if key + "path" in z.files:
            tick, path = reads.pop(0)
            assert (tick, path) == (rec["tick"], str(z[key + "path"]))
            continue
        img = rec["img"]
        assert img.dtype == np.float32 and img.shape == (224, 224, 3)
        sub = np.abs(img[::eu.SUBSAMPLE, ::eu.SUBSAMPLE].astype(np.float64) - z[key + "sub"]).max()
        dsum = abs(img.astype(np.float64).sum() - float(z[key + "sum"]))
        dsq = abs((img.astype(np.float64) ** 2).sum() - float(z[key + "sumsq"]))
        print("%s image %d: subsample max diff %.3e, |d sum| / n %.3e, |d sumsq| / 2n %.3e (tol %.1e)" % (
            name, i, sub, dsum / N_VALUES, dsq / (2 * N_VALUES), tol))
        worst = max(worst, sub)
        assert sub <= tol, (name, i, sub)
        assert dsum <= N_VALUES * tol and dsq <= 2 * N_VALUES * tol, (name, i, dsum, dsq)
    assert not reads
    print("%s: largest subsample difference %.3e" % (name, worst))


def test_knn_case_has_a_query_off_its_nearest_row(golden):
    """The fixture holds at least one nearest-frame tick whose chosen row (the smallest index of the five) is not the nearest."""
    z, _ = golden
    case = eu.case_by_name("cnn_inverse")
    paths = eu.case_paths(case)
    off = 0
    for i in range(int(z["cnn_inverse/n_shown"])):
        key = "cnn_inverse/shown%02d/" % i
        chosen = str(z[key + "path"])
        nearest = "data/" + paths[int(z[key + "nearest"])].split(".jpg")[0] + ".jpg"
        off += chosen != nearest
        assert float(z[key + "min_gap"]) > 1e-9
    assert off >= 1


def test_knn_image_index_is_the_smallest_of_five(enjoy):
    import knn_util as ku
    case = eu.case_by_name("cnn_inverse")
    X = eu.case_states(case).astype(np.float64)
    rs = np.random.RandomState(5)
    for q in rs.randn(6, case["state_dim"]):
        idx, _ = ku.brute_knn(X, q[None], 5)
        assert enjoy.knnImageIndex(X, q) == int(idx[0].min())
    assert enjoy.knnImageIndex(X[:5], X[4]) == 0  # five rows: every query gets row 0


@pytest.fixture(scope="module")
def ae(tmp_path_factory):
    case = eu.case_by_name("cnn_ae")
    _, srl, _ = _build(case, tmp_path_factory.mktemp("enjoy_bn"))
    # running statistics that are not the initial 0 / 1, so that eval mode is a different function from training mode
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, b in srl.model.named_buffers():
            if k.endswith("running_mean"):
                b.copy_((torch.rand(b.shape, generator=gen) - 0.5).to(b.device))
            elif k.endswith("running_var"):
                b.copy_((0.5 + torch.rand(b.shape, generator=gen)).to(b.device))
    states = eu.case_states(case)[:5].astype(np.float64)
    return srl.model, states


def _buffers(model):
    return {k: b.detach().cpu().clone() for k, b in model.named_buffers()}


def _same_buffers(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_batchnorm_running_is_eval_decode(enjoy, ae):
    model, states = ae
    before = _buffers(model)
    assert any(k.endswith("running_mean") for k in before)
    for mode in (True, False):  # whatever mode the model is in when asked
        model.train(mode)
        got = enjoy.decodeStates(model.model, states, "running")
        assert model.training == mode and model.model.training == mode and _same_buffers(before, _buffers(model))
        model.eval()
        with torch.no_grad():
            want = model.model.decode(torch.from_numpy(states).float().cuda())
        assert tuple(got.shape) == (5, 3, 224, 224) and torch.equal(got, want)
    model.train()


def test_batchnorm_reference_is_one_training_mode_decode_per_state(enjoy, ae):
    model, states = ae
    model.train()
    before = _buffers(model)
    got = enjoy.decodeStates(model.model, states, "reference")
    assert model.training and _same_buffers(before, _buffers(model))
    # order of calls cannot matter: the same states in another order give the same images
    perm = [3, 0, 4, 1, 2]
    again = enjoy.decodeStates(model.model, states[perm], "reference")
    assert torch.equal(again, got[perm])
    with torch.no_grad():
        alone = model.model.decode(torch.from_numpy(states[2:3]).float().cuda())
    assert torch.equal(got[2:3], alone)
    with torch.no_grad():  # (that decode moved the running statistics, as the reference's does: put them back)
        for k, b in model.named_buffers():
            b.copy_(before[k])
    running = enjoy.decodeStates(model.model, states, "running")
    assert not torch.equal(running, got)
    device = torch.device("cuda")
    img = enjoy.getImage(model.model, states[2], device)
    from srlz import ops
    assert img.tobytes() == ops.decoded_to_bgr(alone).cpu().numpy()[0].tobytes() == eu.numpy_bgr(alone.cpu().numpy())[0].tobytes()
    with pytest.raises(ValueError):
        enjoy.decodeStates(model.model, states, "eval")


def test_six_channel_decoder_trips_the_reference_assertion(enjoy):
    class SixChannels(torch.nn.Module):
        def __init__(self):
            super(SixChannels, self).__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def decode(self, z):
            return torch.zeros((z.shape[0], 6, 224, 224), device=z.device)

    model = SixChannels().cuda()
    with pytest.raises(AssertionError, match=r"Color channel must be at the end of the tensor \(224, 224, 6\)"):
        enjoy.getImage(model, np.zeros(3), torch.device("cuda"))
