"""The host side of the closed-form forward head (srlz/dynfit.py), the new entry points' predicates and the --fit flags of
evaluation.predict_forward: nothing here needs a GPU."""
import math

import numpy as np
import pytest
import torch

import dynfit_util as du

LAYOUTS = {
    "plain": [1, 0, 0, 0, 1, 0, 0, 1, 0, 0],
    "episode_of_one": [1, 0, 0, 1, 1, 0, 0, 0],          # frame 3 is an episode of length 1
    "start_at_the_last_frame": [1, 0, 0, 0, 1, 0, 0, 1],
    "no_flag_at_frame_0": [0, 0, 0, 1, 0, 0, 1, 0],
    "everything": [0, 0, 1, 1, 0, 0, 0, 1, 0, 1],
    "one_frame": [1],
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_transitions_is_the_selection_of_predict_reward(name):
    from srlz import dynfit, deploy
    es = np.array(LAYOUTS[name], bool)
    num_samples = len(es) - 1
    ref = np.array([i for i in range(num_samples) if not es[i + 1]], dtype="int64")  # evaluation/predict_reward.py:60
    got = dynfit.transitions(es)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert np.array_equal(got, np.flatnonzero(deploy.valid_steps(es, 1) >= 1))
    assert np.array_equal(dynfit.transitions(es.astype(np.float64)), ref)
    for n in range(len(es) + 1):  # the first n frames alone
        assert np.array_equal(dynfit.transitions(es, n), [i for i in range(n - 1) if not es[i + 1]])
    with pytest.raises(ValueError):
        dynfit.transitions(es, len(es) + 1)


def test_split_episodes_keeps_episodes_whole_and_follows_the_seed():
    from srlz import dynfit
    lens = [5, 1, 7, 3, 2, 6, 4]
    es = np.concatenate([[1] + [0] * (n - 1) for n in lens]).astype(bool)
    es[0] = False  # frame 0 opens an episode whether it is flagged or not
    ids = dynfit.episode_ids(es)
    assert ids[0] == 0 and ids[-1] == len(lens) - 1 and np.array_equal(np.bincount(ids), lens)
    every = dynfit.transitions(es)
    seen = set()
    for seed in range(6):
        train, val = dynfit.split_episodes(es, 0.3, seed)
        again = dynfit.split_episodes(es, 0.3, seed)
        assert np.array_equal(train, again[0]) and np.array_equal(val, again[1])
        assert train.dtype == np.int32 and val.dtype == np.int32
        assert np.array_equal(np.sort(np.concatenate((train, val))), every)
        assert not set(ids[train]) & set(ids[val])  # never a split episode
        perm = np.random.RandomState(seed).permutation(len(lens))
        n_val = int(math.ceil(0.3 * len(lens)))
        assert set(ids[val]) == set(perm[len(lens) - n_val:]) - {1}  # (episode 1 has one frame: no transition)
        seen.add(tuple(val))
    assert len(seen) > 1
    with pytest.raises(ValueError, match="at least 2 episodes"):
        dynfit.split_episodes(np.array([1, 0, 0, 0], bool))
    with pytest.raises(ValueError, match="at least 2 episodes"):
        dynfit.split_episodes(np.zeros(5, bool))
    with pytest.raises(ValueError, match="both sides"):  # two episodes, one of them a single frame
        dynfit.split_episodes(np.array([1, 0, 0, 1], bool), 0.5, 0)
    for bad in (0.0, 1.0, -0.2, float("nan")):
        with pytest.raises(ValueError, match="val_fraction"):
            dynfit.split_episodes(es, bad)


def _objective(w, b, x, nxt, acts, n_actions, ridge):
    """J in plain torch fp64: the reference's forwardModel (models/forward_inverse.py:30-31) under an MSE summed over the state
    dimensions and averaged over the transitions, plus the ridge term on the weights."""
    onehot = torch.nn.functional.one_hot(acts, n_actions).double()
    pred = x + torch.nn.functional.linear(torch.cat((x, onehot), dim=1), w, b)
    return ((nxt - pred) ** 2).sum(dim=1).mean() + ridge * (w ** 2).sum()


def _dataset(kind, s=3, a=2, n=50, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(n + 1, s)
    acts = rs.randint(0, a, n + 1)
    if kind == "constant_action":
        acts[:] = 1
    if kind == "duplicated_column":
        x[:, 2] = x[:, 0]
    return x, acts


@pytest.mark.parametrize("kind", ["random", "constant_action", "duplicated_column"])
@pytest.mark.parametrize("ridge", [1e-6, 1e-2])
def test_solve_forward_head_minimises_the_objective(kind, ridge):
    from srlz import dynfit
    s, a, n = 3, 2, 50
    x, acts = _dataset(kind)
    starts = np.arange(n)
    z, y = du.design(x, acts, starts, a)
    G, C = z.T @ z, z.T @ y
    w64, b64 = dynfit.solve_forward_head(G, C, n, s, a, ridge)
    assert w64.shape == (s, s + a) and b64.shape == (s,) and w64.dtype == np.float64
    tx, tn, ta = torch.from_numpy(x[:-1]), torch.from_numpy(x[1:]), torch.from_numpy(acts[:-1]).long()
    w = torch.from_numpy(w64).clone().requires_grad_(True)
    b = torch.from_numpy(b64).clone().requires_grad_(True)
    j = _objective(w, b, tx, tn, ta, a, ridge)
    j.backward()
    g = max(float(w.grad.abs().max()), float(b.grad.abs().max()))
    bound = 1e-10 * max(1.0, float(np.abs(C / n).max()))
    print("%s ridge %g: |grad J|_inf = %.3e (bound %.3e)" % (kind, ridge, g, bound))
    assert g <= bound
    # the unique minimiser: moving any entry by 1e-3 raises J
    j0 = float(j.detach())
    with torch.no_grad():
        for t in (w, b):
            flat = t.view(-1)
            for e in range(flat.numel()):
                for d in (1e-3, -1e-3):
                    flat[e] += d
                    assert float(_objective(w, b, tx, tn, ta, a, ridge)) > j0, (kind, e, d)
                    flat[e] -= d


def test_solve_forward_head_refuses_a_ridge_that_leaves_the_system_singular():
    from srlz import dynfit
    x, acts = _dataset("random")
    z, y = du.design(x, acts, np.arange(50), 2)
    G, C = z.T @ z, z.T @ y
    assert np.linalg.matrix_rank(G) < G.shape[0]  # the one-hot columns sum to the constant column
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ridge"):
            dynfit.solve_forward_head(G, C, 50, 3, 2, bad)
    with pytest.raises(ValueError):
        dynfit.solve_forward_head(G[:-1, :-1], C, 50, 3, 2, 1e-6)
    import inspect
    assert inspect.signature(dynfit.solve_forward_head).parameters["ridge"].default == 1e-6
    assert "positive definite" in dynfit.solve_forward_head.__doc__


def test_check_fit_recording_value_errors():
    from srlz import dynfit
    x, acts, es = du.planted_recording()
    n = len(acts)
    a, st, na = dynfit.check_fit_recording(x, acts, es)
    assert a.dtype == np.int32 and st.dtype == np.int32 and na == du.A and np.array_equal(st, dynfit.transitions(es))
    with pytest.raises(ValueError, match="one entry per frame"):
        dynfit.check_fit_recording(x, acts[:-1], es)
    with pytest.raises(ValueError, match="one entry per frame"):
        dynfit.check_fit_recording(x[:-1], acts, es)
    with pytest.raises(ValueError, match="must be integers"):
        dynfit.check_fit_recording(x, acts + 0.5, es)
    assert dynfit.check_fit_recording(x, acts.astype(np.float64), es)[2] == du.A
    with pytest.raises(ValueError, match="inside every listed transition"):
        dynfit.check_fit_recording(x, np.where(np.arange(n) == 5, du.A, acts), es, n_actions=du.A)
    with pytest.raises(ValueError, match="inside every listed transition"):
        dynfit.check_fit_recording(x, np.where(np.arange(n) == 5, -1, acts), es)
    # an action outside the range at a frame no listed transition starts from is not looked at
    last = du.EP_LEN - 1
    assert dynfit.check_fit_recording(x, np.where(np.arange(n) == last, 99, acts), es, n_actions=du.A)[0][last] == 0
    with pytest.raises(ValueError, match="no transition at all"):
        dynfit.check_fit_recording(x, acts, np.ones(n, bool))
    with pytest.raises(ValueError, match="starts must lie"):
        dynfit.check_fit_recording(x, acts, es, starts=np.array([0, n - 1]))
    with pytest.raises(ValueError, match="floating point"):
        dynfit.check_fit_recording(x.astype(np.int32), acts, es)
    with pytest.raises(ValueError, match=r"\[N,S\]"):
        dynfit.check_fit_recording(x[0], acts, es)
    with pytest.raises(ValueError, match="ridge"):
        dynfit.fit_forward(x, acts, es, ridge=0.0)
    with pytest.raises(ValueError, match="route"):
        dynfit.fit_forward(x, acts, es, route="rollout")
    bad = x.copy()
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        dynfit.fit_forward(bad, acts, es)


def test_abi_version_and_the_new_predicates_answer_without_a_gpu():
    from srlz import _cabi as cabi, ops, dynfit
    assert cabi.version() == cabi.ABI_VERSION == 104
    for name in ("srlz_dynfit_supported", "srlz_dynfit_chunk_rows", "srlz_dynfit_workspace", "srlz_dynfit_gram"):
        assert name in cabi.EXPORTED
    for s, a, ok in ((1, 1, True), (512, 64, True), (512, 1, True), (1, 64, True), (0, 1, False), (513, 1, False), (1, 0, False),
                     (1, 65, False), (-1, -1, False)):
        assert ops.dynfit_supported(s, a) is ok, (s, a)
        assert dynfit.fit_route_for(s, a) == ("gram" if ok else "torch")
        for m in (1, 33, 100000):
            r, ws = ops.dynfit_chunk_rows(m, s, a), ops.dynfit_workspace(m, s, a)
            if not ok:
                assert r == 0 and ws == 0
                continue
            p, ts = s + a + 1, (s + 15) // 16
            tp = (p + 15) // 16
            tiles = tp * (tp + 1) // 2 + tp * ts  # the lower triangle of G, and C
            chunks = (m + r - 1) // r
            assert r >= 1 and r % 32 == 0 and ws == tiles * chunks * 256 * 8
            assert chunks <= 256 and tiles * chunks <= 16384 and ws <= 32 << 20  # the stated cap
    assert ops.dynfit_chunk_rows(0, 3, 2) == 0 and ops.dynfit_workspace(0, 3, 2) == 0 and ops.dynfit_workspace(-5, 3, 2) == 0
    # the chunks cover the transitions whatever M
    for m in (1, 31, 32, 33, 8192, 8193, 2 ** 31 - 1):
        r = ops.dynfit_chunk_rows(m, 200, 6)
        assert r * ((m + r - 1) // r) >= m


def test_the_fit_flags_parse_and_the_old_invocations_keep_their_defaults():
    from evaluation import predict_forward as pf
    a = pf.build_parser().parse_args(["--log-folder", "logs/ds/run/"])
    assert (a.log_folder, a.data_folder, a.input_file, a.horizon, a.training_set_size, a.no_cuda) == ("logs/ds/run/", "", "", 10, -1, False)
    assert a.fit is False and a.ground_truth is False
    a = pf.build_parser().parse_args(["--log-folder", "logs/ds/run", "--data-folder", "data/ds", "-i", "x.npz", "--horizon", "4",
                                      "--training-set-size", "100"])
    assert (a.data_folder, a.input_file, a.horizon, a.training_set_size, a.fit) == ("data/ds", "x.npz", 4, 100, False)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit"])
    assert a.fit is True and (a.ridge, a.val_fraction, a.seed, a.ground_truth) == (1e-6, 0.2, 0, False)
    a = pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--ridge", "1e-3", "--val-fraction", "0.5", "--seed", "7", "--ground-truth"])
    assert (a.ridge, a.val_fraction, a.seed, a.ground_truth) == (1e-3, 0.5, 7, True)
    for extra in (["--ground-truth"], ["--ridge", "1e-6"], ["--val-fraction", "0.2"], ["--seed", "0"]):
        with pytest.raises(SystemExit):
            pf.build_parser().parse_args(["--log-folder", "l"] + extra)
    with pytest.raises(SystemExit):
        pf.build_parser().parse_args(["--log-folder", "l", "--fit", "--ground-truth", "-i", "x.npz"])
    assert pf.OUTPUT == "forward_horizon.json" and pf.OUTPUT_FIT == "forward_horizon_fit.json"
    assert pf.FIT_KEYS == ("ridge", "count", "val_fraction", "seed", "route", "state_dim", "n_actions")
