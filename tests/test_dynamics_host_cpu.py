"""The deployment dynamics on the host side (no GPU): the new symbols in header, library and binding; the limits of
srlz_rollout_supported; the route table of srlz.deploy.LatentDynamics by model class and head shape; the heads gating and its error
text; the loud rejections of a call's states and plans; the fp64 restatement of dynamics_util against the fixtures the unmodified
reference wrote (tools/make_golden_dynamics.py); and the seeded construction's checksums."""
import ctypes
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dynamics_util as dy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "dynamics_kats.npz")
SPREAD = os.path.join(REPO, "tests", "golden", "dynamics_spread.json")
NEW = ("srlz_rollout", "srlz_rollout_supported", "srlz_rollout_tile")


def _split(losses=("autoencoder", "forward", "reward"), dims=(4, 2, 2)):
    import preprocessing.preprocess as pre
    from models.modules import SRLModulesSplit
    pre.N_CHANNELS = 3
    torch.manual_seed(1)
    return SRLModulesSplit(state_dim=sum(dims), action_dim=6, cuda=False, model_type="custom_cnn", losses=list(losses),
                           split_dimensions=OrderedDict(zip(losses, dims)))


def _modules(state_dim, losses, **kw):
    import preprocessing.preprocess as pre
    from models.modules import SRLModules
    pre.N_CHANNELS = 3
    torch.manual_seed(2)
    return SRLModules(state_dim=state_dim, action_dim=6, cuda=False, losses=list(losses), **kw)


def test_header_library_and_binding_agree_on_the_new_symbols(cabi):
    text = open(os.path.join(REPO, "include", "srlz.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(cabi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in cabi.EXPORTED, name
    # one binding argument per parameter of the declaration
    for name in NEW:
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).strip()
        n_params = 0 if decl == "void" else decl.count(",") + 1
        assert len(cabi._PROTOS[name][1]) == n_params, name
    assert cabi.version() == cabi.ABI_VERSION == 104  # the additions are backward compatible
    assert "forward_inverse.py:21-31" in text and "forward_inverse.py:78-95" in text  # the header cites what it replaces


def test_supported_at_the_limits_and_one_past_each(cabi):
    ok = cabi.rollout_supported
    assert cabi.rollout_tile() == 32
    for s, a, h in ((1, 1, 1), (200, 6, 16), (512, 6, 16), (512, 65536, 32), (3, 6, 32), (1, 65536, 1)):
        assert ok(s, a, h, 2) == 1, (s, a, h)
    for s, a, h, nr in ((0, 6, 16, 2), (513, 6, 16, 2), (200, 0, 16, 2), (200, 65537, 16, 2), (200, 6, 0, 2), (200, 6, 33, 2),
                        (200, 6, 16, 1), (200, 6, 16, 3), (-1, 6, 16, 2)):
        assert ok(s, a, h, nr) == 0, (s, a, h, nr)
    from srlz import ops
    assert ops.rollout_supported(200, 6) and not ops.rollout_supported(513, 6)


def test_route_table_by_model_class_and_head_shape():
    from srlz import deploy
    for model_type, losses in (("custom_cnn", ["forward", "reward"]), ("custom_cnn", ["autoencoder", "forward", "inverse", "reward"]),
                               ("mlp", ["forward", "reward"]), ("linear", ["autoencoder", "reward"])):
        m = _modules(8, losses, model_type=model_type)
        assert deploy.dynamics_route_for(m) == "rollout", (model_type, losses)  # the heads do not depend on the encoder
        assert deploy.dynamics_dims(m) == (8, 6, 16, 2)
    assert deploy.dynamics_route_for(_modules(200, ["forward", "reward"])) == "rollout"
    assert deploy.dynamics_route_for(_modules(513, ["forward", "reward"])) == "model"   # S over the limit
    assert deploy.dynamics_route_for(_split()) == "model"                                # the heads see masked states
    wide = _modules(8, ["forward", "reward"])
    wide.initRewardNet(8, n_hidden=33)                                                    # H over the limit
    assert deploy.dynamics_route_for(wide) == "model"
    three = _modules(8, ["forward", "reward"])
    three.initRewardNet(8, n_rewards=3)
    assert deploy.dynamics_route_for(three) == "model"
    with pytest.raises(ValueError, match="heads"):
        deploy.dynamics_route_for(_modules(8, ["autoencoder"]).model)  # a bare encoder owns no heads


def test_heads_gating_names_the_models_losses():
    from srlz import deploy
    m = _modules(8, ["autoencoder", "forward"])
    assert deploy.trained_heads(m) == ("forward",)
    assert deploy.trained_heads(_modules(8, ["reward", "inverse", "forward"])) == ("forward", "inverse", "reward")
    deploy.check_head(m, "forward")
    with pytest.raises(ValueError) as e:
        deploy.check_head(m, "reward")
    assert "reward head" in str(e.value) and "['autoencoder', 'forward']" in str(e.value) and "untrained_ok" in str(e.value)
    with pytest.raises(ValueError, match="inverse head"):
        deploy.check_head(m, "inverse")
    deploy.check_head(m, "reward", untrained_ok=True)

    class Bare(torch.nn.Module):  # a module without .losses allows every head
        def __init__(self):
            super(Bare, self).__init__()
            self.forward_net = torch.nn.Linear(9, 3)
            self.reward_net = m.reward_net
    assert deploy.trained_heads(Bare()) == ("forward", "inverse", "reward")
    deploy.check_head(Bare(), "reward")


def test_states_and_plans_are_validated_loudly():
    from srlz import deploy, ops, _cabi as C
    pl = dy.plans(3, 4, 7, 6)
    assert deploy.check_plans(pl, 3, 6) == (4, 7, False, False)
    assert deploy.check_plans(pl[0], 3, 6) == (4, 7, True, False)            # [K,T] shared by every environment
    assert deploy.check_plans(pl[0, 0], 1, 6) == (1, 7, True, True)          # one bare plan
    assert deploy.check_plans(torch.from_numpy(pl).long(), 3, 6) == (4, 7, False, False)
    assert deploy.check_states(np.zeros(8, np.float32), 8) == (1, True)      # one bare state
    with pytest.raises(ValueError, match="integer"):
        deploy.check_plans(pl.astype(np.float32), 3, 6)
    with pytest.raises(ValueError, match="integer"):
        deploy.check_plans(torch.zeros((4, 7)), 3, 6)
    with pytest.raises(ValueError, match="environments"):
        deploy.check_plans(pl, 2, 6)
    with pytest.raises(ValueError, match="shape"):
        deploy.check_plans(pl.reshape(1, 3, 4, 7), 3, 6)
    with pytest.raises(ValueError, match="no action"):
        deploy.check_plans(pl[:, :, :0], 3, 6)
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        deploy.check_plans([[0, 1]], 1, 6)
    for bad in (6, -1):
        spoiled = pl.copy()
        spoiled[1, 2, 3] = bad
        with pytest.raises(ValueError, match=r"\[0, 6\)"):
            deploy.check_plans(spoiled, 3, 6)
        with pytest.raises(C.SrlzError, match=r"\[0, 6\)"):
            ops.rollout_plans(spoiled, 6, torch.device("cpu"))
    with pytest.raises(C.SrlzError, match="integers"):
        ops.rollout_plans(pl.astype(np.float64), 6, torch.device("cpu"))
    assert ops.rollout_plans(pl.astype(np.int64), 6, torch.device("cpu")).dtype == torch.int32
    with pytest.raises(ValueError, match="floating point"):
        deploy.check_states(np.zeros((3, 8), np.int32), 8)
    with pytest.raises(ValueError, match="state_dim"):
        deploy.check_states(np.zeros((3, 7), np.float32), 8)
    with pytest.raises(C.SrlzError, match="device tensor"):
        ops.rollout(torch.zeros((3, 8)), pl, torch.zeros((8, 14)), torch.zeros(8))  # host states: there is no CPU path


def test_constructor_judges_its_arguments_before_it_asks_for_a_gpu(monkeypatch):
    from srlz import deploy
    m = _modules(8, ["forward", "reward"])
    with pytest.raises(ValueError, match="route"):
        deploy.LatentDynamics(m, route="rollout")
    with pytest.raises(ValueError, match="max_rows"):
        deploy.LatentDynamics(m, max_rows=0)
    with pytest.raises(ValueError, match="heads"):
        deploy.LatentDynamics(m.model)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (so the test says the same on a machine that has one)
    with pytest.raises(RuntimeError, match="MI355X only"):
        deploy.LatentDynamics(m)
    with pytest.raises(RuntimeError, match="MI355X only"):
        deploy.LatentDynamics.from_log_folder("logs/none/")


@pytest.mark.parametrize("name", list(dy.CASES))
def test_seeded_construction_has_the_references_checksums_and_the_restatement_its_numbers(name):
    import models.modules as modules
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    kats = np.load(GOLDEN)
    model = dy.build_case(name, modules)
    got, want = dy.checksums(model.state_dict()), kats[name + "/checksums"]
    assert np.allclose(got, want, rtol=1e-12, atol=0), (got, want)
    z, pl = dy.case_inputs(name)
    gamma = float(kats["gamma"])
    ref = dy.restate(dy.head_params(model.state_dict()), z, pl, gamma=gamma)
    for q in dy.QUANTITIES:
        e = dy.rel_err(ref[q], kats["%s/%s64" % (name, q)], q != "returns")
        assert e <= 1e-12, (q, e)
    # the fixtures' own spread is the one on record, and the restatement at fp32 stays within the standing bound of it
    rec = json.load(open(SPREAD))["cases"][name]
    lo = dy.restate(dy.head_params(model.state_dict()), z, pl, gamma=gamma, dtype=torch.float32)
    for q in dy.QUANTITIES:
        per_step = q != "returns"
        assert dy.rel_err(kats["%s/%s32" % (name, q)], kats["%s/%s64" % (name, q)], per_step) == pytest.approx(rec[q], rel=1e-9)
        assert dy.rel_err(lo[q], kats["%s/%s64" % (name, q)], per_step) <= dy.bound(rec[q]), q
    if name == "s200_expanding":
        assert rec["last_step_scale"] > 1e7
