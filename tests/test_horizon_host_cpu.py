"""The k-step error of the dynamics on the host side (no GPU): the new symbols in header, library and binding; the limits of
srlz_horizon_supported and the LDS budget at them; valid_steps on hand-written episode layouts; the numpy restatement of the whole
metric against the fixture of the unmodified reference (tests/golden/horizon_kats.npz); srlz.deploy's own host sums against the same;
the route table; every ValueError; the command line's parser and JSON keys; and the condition the fixture records."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import dynamics_util as dy
import horizon_util as hu
from test_dynamics_host_cpu import _modules, _split

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW = ("srlz_horizon_supported", "srlz_horizon_rows", "srlz_horizon_sums")


def test_header_library_and_binding_agree_on_the_new_symbols(cabi):
    text = open(os.path.join(REPO, "include", "srlz.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(cabi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in cabi.EXPORTED, name
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).strip()
        assert len(cabi._PROTOS[name][1]) == decl.count(",") + 1, name  # one binding argument per parameter
    assert cabi.version() == cabi.ABI_VERSION == 104  # the additions are backward compatible
    assert "srlz_horizon_supported" in cabi._NOT_STATUS  # (its int is an answer, not a status)


def test_supported_at_each_limit_and_one_past_it(cabi):
    from srlz import ops
    hs = cabi.horizon_supported
    for s, a, h in ((1, 1, 1), (200, 6, 16), (512, 65536, 32), (33, 6, 32)):
        assert hs(s, a, h, 2, 1) == 1 and hs(s, a, 0, 0, 0) == 1 and hs(s, a, 77, 5, 0) == 1, (s, a, h)  # no head: H, n_rewards not looked at
    for s, a, h, nr in ((513, 6, 16, 2), (0, 6, 16, 2), (200, 0, 16, 2), (200, 65537, 16, 2), (200, 6, 33, 2), (200, 6, 0, 2), (200, 6, 16, 3)):
        assert hs(s, a, h, nr, 1) == 0, (s, a, h, nr)
    assert hs(513, 6, 16, 2, 0) == 0 and hs(200, 0, 16, 2, 0) == 0
    assert ops.horizon_supported(200, 6, 16, 2, True) and ops.horizon_supported(200, 6, 0, 0, has_reward=False)
    assert not ops.horizon_supported(513, 6)
    # the budget include/srlz.h states: both reductions' partials add 2 * 16 * 33 floats; at the limits the tile stays inside 160 KB
    tile = (512 * 33 + 8 * 32 * 33 + 2 * 32 * 33 + 32 * 32 + 4 * 32 + 4 + 2 * 32) * 4
    assert tile + 2 * 16 * 33 * 4 == 118928 and tile + 2 * 16 * 33 * 4 <= 160 * 1024


def test_valid_steps_on_hand_written_layouts():
    from srlz import deploy
    es = lambda *on: np.isin(np.arange(on[0]), on[1:])  # noqa: E731  (length, then the frames that start an episode)
    # one episode of six frames: the horizon, then the last frames
    assert deploy.valid_steps(es(6, 0), 3).tolist() == [3, 3, 3, 2, 1, 0]
    # a boundary at i + 1: frame 2 is the last of its episode, frame 3 an episode of one frame
    assert deploy.valid_steps(es(7, 0, 3, 4), 2).tolist() == [2, 1, 0, 0, 2, 1, 0]
    # an episode shorter than the horizon
    assert deploy.valid_steps(es(5, 0, 2), 10).tolist() == [1, 0, 2, 1, 0]
    # no flag at frame 0 (a truncated recording), integer and float flags, one frame, a horizon of one
    assert deploy.valid_steps(np.array([0, 0, 1, 0]), 5).tolist() == [1, 0, 1, 0]
    assert deploy.valid_steps(np.array([1.0, 0.0, 0.0]), 1).tolist() == [1, 1, 0]
    assert deploy.valid_steps(np.array([True]), 4).tolist() == [0]
    assert deploy.valid_steps(es(6, 0), 3).dtype == np.int32
    rs = np.random.RandomState(0)
    for _ in range(20):  # against the definition, frame by frame
        flags = rs.rand(rs.randint(1, 60)) < 0.2
        t = int(rs.randint(1, 12))
        assert np.array_equal(deploy.valid_steps(flags, t), hu.valid_steps(flags, t))
    _, _, _, flags = hu.recording(3)
    lens = deploy.valid_steps(flags, hu.HORIZON)
    assert sorted(set(lens.tolist())) == list(range(hu.HORIZON + 1)) and lens[0] == 0 and lens[1] == 1  # every length; an episode of one frame
    with pytest.raises(ValueError, match="horizon"):
        deploy.valid_steps(flags, 0)


def _fixture():
    return np.load(os.path.join(GOLDEN, "horizon_kats.npz")), json.load(open(os.path.join(GOLDEN, "horizon_spread.json")))


def test_fixture_records_its_condition():
    kats, spread = _fixture()
    assert spread["gap"] == hu.GAP and spread["gap_cap"] == hu.GAP_CAP == 0.05
    assert spread["horizon"] == hu.HORIZON == int(kats["horizon"]) and spread["n_frames"] == hu.N_FRAMES == int(kats["n_frames"])
    for name in dy.CASES:
        sp = spread["cases"][name]
        lens = hu.valid_steps(hu.recording(3)[3], hu.HORIZON)
        mask = hu.valid_mask(lens, hu.HORIZON)
        dec = kats[name + "/decided"]
        assert np.array_equal(dec, hu.decided(kats[name + "/logits64"], mask)), name  # the mask is the rule applied to the logits
        assert not dec[~mask].any() and sp["valid"] == int(mask.sum())
        assert abs(sp["left_out"] - (1.0 - dec.sum() / float(mask.sum()))) < 1e-12
        assert sp["hits_checked"] is (name in hu.HIT_CASES)
        if sp["hits_checked"]:
            assert sp["left_out"] <= hu.GAP_CAP, name
        # the fp32 composition of the reference itself answers every decided entry as the fp64 one does
        assert np.array_equal(hu.classes_of(kats[name + "/logits32"])[dec], hu.classes_of(kats[name + "/logits64"])[dec]), name
        for q in hu.ROW_QUANTITIES + hu.SUM_QUANTITIES:
            assert 0 <= sp[q] < 1e-5, (name, q)
    assert not spread["cases"]["s200_expanding"]["hits_checked"] and spread["cases"]["s200_expanding"]["left_out"] > hu.GAP_CAP


@pytest.mark.parametrize("name", list(dy.CASES))
def test_numpy_restatement_of_the_metric_is_the_fixtures_fp64(name):
    from srlz import deploy
    kats, _ = _fixture()
    s = dy.CASES[name]["state_dim"]
    states, actions, rewards, es = hu.recording(s)
    lens, starts = hu.valid_steps(es, hu.HORIZON), np.arange(hu.N_FRAMES)
    labels = hu.labels_of(rewards)
    mask = hu.valid_mask(lens, hu.HORIZON)
    # the whole metric from the model's parameters: forwardModel and rewardModel restated (dynamics_util.restate), then the rows and sums
    import models.modules as modules
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    model = dy.build_case(name, modules)
    assert np.allclose(dy.checksums(model.state_dict()), kats[name + "/checksums"], rtol=1e-6, atol=0)  # the fixture's heads
    plans = np.zeros((hu.N_FRAMES, 1, hu.HORIZON), np.int64)
    for r in range(hu.N_FRAMES):
        plans[r, 0, :lens[r]] = actions[r:r + lens[r]]
    out = dy.restate(dy.head_params(model.state_dict()), states, plans, dtype=torch.float64)
    err, base = hu.rows_from_trajectory(out["trajectory"][:, 0], states, starts, lens, np.float64)
    assert np.isnan(err[~mask]).all() and np.isnan(base[~mask]).all() and not np.isnan(err[mask]).any()
    assert hu.step_rel_err(err, kats[name + "/err64"], mask) < 1e-12 and hu.step_rel_err(base, kats[name + "/base64"], mask) < 1e-12
    assert hu.step_rel_err(out["reward_logits"][:, 0], kats[name + "/logits64"], mask) < 1e-12
    count, se, sb, hits = hu.totals(err, base, lens, out["reward_logits"][:, 0], labels, starts)
    assert np.array_equal(count, kats[name + "/count"]) and count.tolist() == [int((lens > t).sum()) for t in range(hu.HORIZON)]
    assert hu.vec_rel_err(se, kats[name + "/sum_err"]) < 1e-12 and hu.vec_rel_err(sb, kats[name + "/sum_base"]) < 1e-12
    if name in hu.HIT_CASES and kats[name + "/decided"][mask].all():
        assert np.array_equal(hits, kats[name + "/hits"])
    # srlz.deploy's own host sums (what route "model" reports) state the same rule
    c2, se2, sb2, h2 = deploy.horizon_totals(err, base, lens, out["reward_logits"][:, 0], labels, starts)
    assert np.array_equal(c2, count) and np.array_equal(h2, hits)
    assert hu.vec_rel_err(se2, se) < 1e-14 and hu.vec_rel_err(sb2, sb) < 1e-14
    major = deploy.majority_accuracy(labels, starts, lens, hu.HORIZON)
    for t in range(hu.HORIZON):
        lab = np.array([labels[r + t] for r in range(hu.N_FRAMES) if lens[r] > t])
        assert major[t] == max((lab == 1).mean(), (lab == 0).mean())
    h = deploy.HorizonError(hu.HORIZON, c2, se2, sb2, s, h2, major)
    assert np.allclose(h.mse, se / (count * s)) and np.allclose(h.baseline_mse, sb / (count * s)) and np.allclose(h.ratio, se / sb)
    assert np.allclose(h.reward_accuracy, hits / count) and h.err is None and h.logits is None


def test_route_table():
    from srlz import deploy
    both, fwd_only = _modules(8, ["forward", "reward"]), _modules(8, ["forward", "inverse"])
    for m in (both, fwd_only):
        for has_reward in (True, False):
            assert deploy.horizon_route_for(m, has_reward, 10) == "rollout"
            assert deploy.horizon_route_for(m, has_reward, 32) == "rollout" and deploy.horizon_route_for(m, has_reward, 33) == "model"
            assert deploy.horizon_route_for(m, has_reward, 10, max_horizon=8) == "model"
            assert deploy.horizon_route_for(m, has_reward, 0) == "model"
    for has_reward in (True, False):
        assert deploy.horizon_route_for(_split(), has_reward, 10) == "model"  # every split model: its heads see masked states
        assert deploy.horizon_route_for(_modules(513, ["forward", "reward"]), has_reward, 10) == "model"
    # the other tables keep their answers
    assert deploy.dynamics_route_for(both) == "rollout" and deploy.dynamics_route_for(_split()) == "model"
    assert deploy.goal_route_for(both) == "rollout" and deploy.plan_route_for(both, 64, 33) == "model"


def test_every_value_error_of_the_recording_checks():
    from srlz import deploy
    _, actions, rewards, es = hu.recording(3)
    n = hu.N_FRAMES
    acts, starts, lens = deploy.check_recording(n, actions, es, hu.HORIZON, hu.N_ACTIONS)
    full = hu.valid_steps(es, hu.HORIZON)
    assert np.array_equal(starts, np.flatnonzero(full >= 1)) and np.array_equal(lens, full[starts])  # the default: every frame with a step
    assert acts.dtype == starts.dtype == lens.dtype == np.int32
    assert (starts + lens <= n - 1).all() and (lens >= 1).all() and (lens <= hu.HORIZON).all()  # the kernel's contract
    _, st, ln = deploy.check_recording(n, torch.from_numpy(actions), torch.from_numpy(es), hu.HORIZON, hu.N_ACTIONS, starts=np.array([0, 39, 5, 5]))
    assert st.tolist() == [0, 39, 5, 5] and ln.tolist() == [0, 0, 6, 6]  # given starts are taken as they come, rows without a step included
    with pytest.raises(ValueError, match="one entry per frame"):
        deploy.check_recording(n, actions[:-1], es, hu.HORIZON, hu.N_ACTIONS)
    with pytest.raises(ValueError, match="one entry per frame"):
        deploy.check_recording(n, actions, es[:-1], hu.HORIZON, hu.N_ACTIONS)
    with pytest.raises(ValueError, match="integers"):
        deploy.check_recording(n, actions + 0.5, es, hu.HORIZON, hu.N_ACTIONS)
    with pytest.raises(ValueError, match="horizon"):
        deploy.check_recording(n, actions, es, 0, hu.N_ACTIONS)
    for bad in (np.array([-1]), np.array([n]), np.array([0.0])):
        with pytest.raises(ValueError, match="starts"):
            deploy.check_recording(n, actions, es, hu.HORIZON, hu.N_ACTIONS, starts=bad)
    with pytest.raises(ValueError, match="no start frame"):
        deploy.check_recording(3, actions[:3], np.ones(3, bool), hu.HORIZON, hu.N_ACTIONS)
    with pytest.raises(ValueError, match="no start frame"):
        deploy.check_recording(n, actions, es, hu.HORIZON, hu.N_ACTIONS, starts=np.zeros(0, np.int64))
    # an action out of range counts inside a valid step alone: frame 0 and frame 2 are the last of their episodes, frame 39 of the sequence
    for frame in (0, 2, 39):
        for v in (-1, hu.N_ACTIONS):
            moved = actions.copy()
            moved[frame] = v
            assert deploy.check_recording(n, moved, es, hu.HORIZON, hu.N_ACTIONS)[0][frame] == 0  # never read: handed on as 0
    for frame, v in ((1, -1), (5, hu.N_ACTIONS), (38, 99)):
        moved = actions.copy()
        moved[frame] = v
        with pytest.raises(ValueError, match="inside every valid step"):
            deploy.check_recording(n, moved, es, hu.HORIZON, hu.N_ACTIONS)
    # rewards: -1 is class 0; anything beyond two classes is refused
    assert deploy.reward_classes(rewards).tolist() == hu.labels_of(rewards).tolist() and deploy.reward_classes(rewards).dtype == np.int64
    assert (rewards < 0).any() and set(deploy.reward_classes(rewards).tolist()) == {0, 1}
    for bad in (np.array([0, 2]), np.array([0.0, 1.0, 3.5])):
        with pytest.raises(ValueError, match="two classes"):
            deploy.reward_classes(bad)


def test_parser_and_json_keys():
    from evaluation import predict_forward as pf
    from srlz import deploy
    a = pf.build_parser().parse_args(["--log-folder", "logs/ds/run/"])
    assert (a.log_folder, a.data_folder, a.input_file, a.horizon, a.training_set_size, a.no_cuda) == ("logs/ds/run/", "", "", 10, -1, False)
    a = pf.build_parser().parse_args(["--log-folder", "logs/ds/run", "--data-folder", "data/ds", "-i", "x.npz", "--horizon", "4",
                                      "--training-set-size", "100"])
    assert (a.data_folder, a.input_file, a.horizon, a.training_set_size) == ("data/ds", "x.npz", 4, 100)
    with pytest.raises(SystemExit):
        pf.build_parser().parse_args([])
    h = deploy.HorizonError(2, [3, 0], [6.0, 0.0], [12.0, 0.0], 2)
    d = h.as_dict()
    assert tuple(sorted(d)) == tuple(sorted(pf.KEYS)) and pf.OUTPUT == "forward_horizon.json"
    assert d["horizon"] == 2 and d["count"] == [3, 0] and d["mse"][0] == 1.0 and d["baseline_mse"][0] == 2.0 and d["ratio"][0] == 0.5
    assert d["mse"][1] is None and d["ratio"][1] is None  # a horizon no row reaches: null, not NaN
    assert d["reward_accuracy"] is None and d["majority_accuracy"] is None
    json.loads(json.dumps(d, allow_nan=False))
    with_head = deploy.HorizonError(1, [4], [1.0], [2.0], 1, hits=[3], majority_accuracy=np.array([0.75]))
    assert with_head.as_dict()["reward_accuracy"] == [0.75] and with_head.as_dict()["majority_accuracy"] == [0.75]
    lines = pf.report(with_head)
    assert len(lines) == 1 and "t+1" in lines[0] and "ratio 0.5000" in lines[0] and "reward acc 0.7500" in lines[0]
    assert len(pf.report(h)) == 2 and "reward" not in pf.report(h)[0]


def test_without_a_gpu_the_command_raises(monkeypatch):
    from evaluation import predict_forward as pf
    from srlz._cabi import SrlzError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SrlzError, match="GPU only"):
        pf.main(["--log-folder", "logs/none/"])
    with pytest.raises(SrlzError, match="--no-cuda"):
        pf.main(["--log-folder", "logs/none/", "--no-cuda"])
