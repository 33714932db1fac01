"""Host side of the reward-prior / episode-prior losses (no GPU): the command line accepts them, the partner draw reproduces the
reference's draws index for index (tests/golden/prior_kats.npz, recorded from the unmodified reference), the seeded Discriminator has the
reference's keys and values, and FlatParams over the model and the discriminator keeps both as views with the right keys."""
import os
import sys

import numpy as np
import pytest
import torch

import golden_util as gu


def test_train_parser_accepts_prior_losses():
    import train
    args = train.buildParser().parse_args(["--data-folder", "x", "--losses", "inverse", "reward-prior", "episode-prior",
                                           "--balanced-sampling"])
    assert list(args.losses) == ["inverse", "reward-prior", "episode-prior"]
    assert args.balanced_sampling is True
    from models.learner import SUPPORTED_LOSSES
    assert {"reward-prior", "episode-prior"} <= SUPPORTED_LOSSES
    assert "priors" not in SUPPORTED_LOSSES


@pytest.mark.parametrize("mode", ["uniform", "balanced"])
def test_partner_draws_match_reference(mode):
    from losses.losses import sampleEpisodeOthers
    g = gu.load("prior_kats")
    cases = sorted({k.split("/")[0] for k in g.files if k.startswith("case")})
    assert cases
    for case in cases:
        eps = g[case + "/episodes"]
        for seed in (0, 1, 2):
            np.random.seed(seed)
            ref = g["%s/%s/seed%d" % (case, mode, seed)]
            for step in range(ref.shape[0]):
                others, same = sampleEpisodeOthers(eps, mode == "balanced")
                np.testing.assert_array_equal(others, ref[step], err_msg="%s %s seed %d step %d" % (case, mode, seed, step))
                np.testing.assert_array_equal(same, (eps == eps[ref[step]]).astype(np.float32))


def test_balanced_draw_single_episode_raises():
    from losses.losses import sampleEpisodeOthers
    g = gu.load("prior_kats")
    assert str(g["single_episode/error"]) == "ValueError"
    np.random.seed(0)
    with pytest.raises(ValueError):
        sampleEpisodeOthers(np.zeros(4, dtype=np.int64), True)
    np.random.seed(0)
    sampleEpisodeOthers(np.zeros(4, dtype=np.int64), False)  # (uniform sampling never needs another episode)


@pytest.mark.parametrize("S", [2, 200])
def test_discriminator_init_matches_reference(S):
    from models.priors import Discriminator
    g = gu.load("prior_kats")
    torch.manual_seed(5)
    sd = Discriminator(2 * S).state_dict()
    names = [str(n) for n in g["disc_s%d/names" % S]]
    assert list(sd.keys()) == names
    for k, s, a in zip(names, g["disc_s%d/sums" % S], g["disc_s%d/abss" % S]):
        v = sd[k].double()
        assert float(v.sum()) == pytest.approx(float(s), rel=1e-12, abs=1e-12), k
        assert float(v.abs().sum()) == pytest.approx(float(a), rel=1e-12), k


def test_flat_params_over_two_modules():
    from srlz import optim
    from models.priors import Discriminator
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2))
    disc = Discriminator(4)
    before = {("m", k): v.detach().clone() for k, v in model.state_dict().items()}
    before.update({("d", k): v.detach().clone() for k, v in disc.state_dict().items()})
    flat = optim.FlatParams(model, disc)
    params = list(model.parameters()) + list(disc.parameters())
    assert len(flat.params) == len(params) and all(a is b for a, b in zip(flat.params, params))
    assert list(disc.state_dict().keys()) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight",
                                              "net.4.bias"]
    for tag, mod in (("m", model), ("d", disc)):
        for k, v in mod.state_dict().items():
            assert torch.equal(v, before[(tag, k)]), k
    for p, off in zip(flat.params, flat.offsets):
        assert p.data_ptr() == flat.flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == flat.grad.data_ptr() + 4 * off
    with torch.no_grad():
        flat.flat.fill_(0.5)
    assert float(disc.net[4].bias) == 0.5 and float(model[0].weight[0, 0]) == 0.5
    # one module: as before
    m2 = torch.nn.Linear(3, 5)
    f2 = optim.FlatParams(m2)
    assert [p is q for p, q in zip(f2.params, m2.parameters())] == [True, True]
    assert f2.offsets == [0, 16]


def test_triplet_with_priors_rejected():
    from models.learner import SRL4robotics
    with pytest.raises(NotImplementedError, match="cannot be combined with 'triplet'"):
        SRL4robotics(10, model_type="custom_cnn", cuda=False, losses=["triplet", "reward-prior"])
