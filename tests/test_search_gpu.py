"""LatentDynamics.search and srlz_beam_search on the GPU.  Every assertion on a return is a bit equality against dyn.rollout, the
project's own contract (include/srlz.h: a call of T steps leaves the bits of T calls of one step; a row's outputs do not depend on the
other rows): no tolerance appears in this file.

Shapes, the smallest at which the thing tested can go wrong: S in {3, 33, 200} (a tail chunk alone; one whole chunk and a tail; more
than one 32-column block), (A, T) in {(2, 6), (3, 4), (6, 3)} for exact search — 216 leaves are seven tiles, the last partly
filled —, A = 3, T = 5 with W in {1, 2, 5, 33} for a pruned beam (W = 33: more than one tile a level, pruned at one level only), and
one tree whose levels reach the limit of 8192 children (A = 4, W = 2048: the finisher's sort at its largest) at S = 3.
  1  exact search is the enumeration: leaf_plans lexicographic, leaf_returns the bits of rollout(states, all plans).returns, best_plan
     its argmax;
  2  a pruned beam is a test-local beam written over dyn.rollout of the prefix plans (a (t+1)-step rollout's return is the prefix's
     ret), without a goal and with a running goal, with and without a reward head;
  3  in every mode (goal mode "final" included) and at every W the kept leaves' returns and best_return are the bits rollout gives
     for those plans;
  4  ties keep the lowest indices; a NaN state gives a NaN return and plan 0 .. 0 and leaves the other environments' bits alone;
  5  hygiene through the C ABI: two runs, sentinels behind every output, tickets zero after the call, a reused object, W * A = 8192
     exactly and one above;
  6  the routes, and reach(..., planner="search")."""
import copy
import functools
import itertools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import deploy_util as du
import dynamics_util as dy

pytestmark = pytest.mark.gpu

F_SENTINEL, I_SENTINEL, B_SENTINEL = 1234.5, -77, 0xAB
TAIL = 64
BAD_DESC, WORKSPACE, NULL = -1, -2, -4  # SRLZ_ERR_BAD_DESC, SRLZ_ERR_WORKSPACE, SRLZ_ERR_NULL of include/srlz.h
_MODELS = {}


def _dev():
    return torch.device("cuda", 0)


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def host(x):
    return x.detach().cpu().numpy()


def goals(n, s):
    """fp32 [n, s]: cos(0.23 i + 0.07 j) + 0.25 — a different goal for every environment."""
    i, j = np.meshgrid(np.arange(n), np.arange(s), indexing="ij")
    return (np.cos(0.23 * i + 0.07 * j) + 0.25).astype(np.float32)


def all_plans(a, t):
    """int32 [A^T, T]: every plan, in lexicographic order (a_0 the most significant digit)."""
    return np.array(list(itertools.product(range(a), repeat=t)), np.int32)


def _model(s, a, losses=None, flat_reward=False):
    """A seeded SRLModules of (S, A) on the device; losses: the same weights under losses that trained no reward head;
    flat_reward: the reward head's last layer zeroed — every prob is 0.5."""
    key = (s, a, tuple(losses) if losses else None, flat_reward)
    if key not in _MODELS:
        if losses is None and not flat_reward:
            import models.modules as modules
            import preprocessing.preprocess as pre
            pre.N_CHANNELS = 3
            torch.manual_seed(11)
            m = modules.SRLModules(state_dim=s, action_dim=a, cuda=False, model_type="custom_cnn", losses=list(dy.LOSSES)).to(_dev())
        else:
            m = copy.deepcopy(_model(s, a))
            if losses is not None:
                m.losses = list(losses)
            if flat_reward:
                with torch.no_grad():
                    m.reward_net[4].weight.zero_()
                    m.reward_net[4].bias.zero_()
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


@functools.lru_cache(maxsize=None)
def _dyn(s, a, head=True, flat_reward=False):
    from srlz import deploy
    return deploy.LatentDynamics(_model(s, a, None if head else ["forward", "inverse"], flat_reward), max_rows=8192, max_horizon=8)


@functools.lru_cache(maxsize=None)
def _enumerated(s, a, t, n, gamma, head=True, goal=None, mode="running"):
    """rollout(states, every plan): computed once per case and shared (returns fp32 [n, A^T] on the host, best [n])."""
    z = dy.sine_states(n, s)
    kw = {} if goal is None else dict(goal=goals(n, s) if goal == "each" else goals(1, s)[0], goal_weight=0.5, goal_mode=mode)
    out = _dyn(s, a, head).rollout(z, all_plans(a, t), gamma=gamma, **kw)
    return host(out.returns).copy(), host(out.best).copy()


# ---- 1: exact search equals enumeration ----
@pytest.mark.parametrize("s", [3, 33, 200])
@pytest.mark.parametrize("a,t", [(2, 6), (3, 4), (6, 3)])
def test_exact_search_is_the_enumeration(a, t, s):
    from srlz import deploy
    dyn, plans = _dyn(s, a), all_plans(a, t)
    for n in (1, 3):
        z = dy.sine_states(n, s)
        for gamma in (1.0, 0.9):
            r = dyn.search(z, t, beam=a ** (t - 1), gamma=gamma, keep_leaves=True)
            assert dyn.route == "rollout" and r.exact and r.leaves == a ** t and r.expanded == sum(a ** i for i in range(1, t + 1))
            got = [host(x).copy() for x in (r.leaf_plans, r.leaf_returns, r.best_plan, r.best_return, r.action)]
            returns, best = _enumerated(s, a, t, n, gamma)
            assert np.array_equal(got[0], np.broadcast_to(plans, (n,) + plans.shape)), (n, gamma)
            assert same_bits(got[1], returns), (n, gamma)
            assert np.array_equal(got[2], plans[best]) and same_bits(got[3], returns[np.arange(n), best]), (n, gamma)
            assert got[2].dtype == np.int32 and got[4].dtype == np.int64 and np.array_equal(got[4], plans[best][:, 0])
    # a beam wider than the tree is the same search; one bare state drops the N axis
    z = dy.sine_states(3, s)
    wide = dyn.search(z[1], t, beam=10 ** 6, gamma=0.9, keep_leaves=True)
    returns, best = _enumerated(s, a, t, 3, 0.9)
    assert wide.exact and wide.best_plan.shape == (t,) and wide.best_return.shape == () and wide.leaf_returns.shape == (a ** t,)
    assert same_bits(wide.leaf_returns, returns[1]) and np.array_equal(host(wide.best_plan), plans[best[1]])
    assert deploy.search_sizes(a ** (t - 1), t, a)["exact"] and not deploy.search_sizes(a ** (t - 1) - 1, t, a)["exact"]


# ---- 2: a pruned beam against a beam written over dyn.rollout of the prefix plans ----
def _reference_beam(dyn, z, a, t, w, gamma, **kw):
    """The algorithm of include/srlz.h with every ret taken from dyn.rollout of the prefix plans (not for goal mode final: there a
    prefix's rollout counts the distance at its own last step)."""
    n = z.shape[0]
    prefixes = np.zeros((n, 1, 0), np.int32)
    for level in range(t):
        f = prefixes.shape[1]
        last = np.broadcast_to(np.tile(np.arange(a, dtype=np.int32), f)[None, :, None], (n, f * a, 1))
        children = np.ascontiguousarray(np.concatenate((np.repeat(prefixes, a, axis=1), last), axis=2))
        ret = host(dyn.rollout(z, children, gamma=gamma, **kw).returns).copy()
        key = np.where(np.isnan(ret), np.float32(-np.inf), ret)
        if level < t - 1 and f * a > w:
            order = np.stack([np.array(sorted(range(f * a), key=lambda c: (-key[e, c], c))[:w]) for e in range(n)])
            children = np.take_along_axis(children, order[:, :, None], axis=1)
        prefixes = children
    top = np.array([min(range(ret.shape[1]), key=lambda c: (-key[e, c], c)) for e in range(n)])
    return children, ret, children[np.arange(n), top], ret[np.arange(n), top]


def _check_beam(dyn, z, a, t, w, gamma, **kw):
    r = dyn.search(z, t, beam=w, gamma=gamma, keep_leaves=True, **kw)
    got = [host(x).copy() for x in (r.leaf_plans, r.leaf_returns, r.best_plan, r.best_return)]
    assert dyn.route == "rollout" and not r.exact
    ref = _reference_beam(dyn, z, a, t, w, gamma, **kw)
    assert np.array_equal(got[0], ref[0]), w
    assert same_bits(got[1], ref[1]), w
    assert np.array_equal(got[2], ref[2]) and same_bits(got[3], ref[3]), w


@pytest.mark.parametrize("w", [1, 2, 5, 33])
def test_pruned_beam_without_a_goal(w):
    a, t = 3, 5
    for s in (33, 200):
        _check_beam(_dyn(s, a), dy.sine_states(3, s), a, t, w, 0.9)
    if w == 1:  # greedy: one node a level
        r = _dyn(33, a).search(dy.sine_states(3, 33), t, beam=1)
        assert r.leaves == a and r.expanded == a * t


@pytest.mark.parametrize("head", [True, False], ids=["head", "nohead"])
@pytest.mark.parametrize("w", [1, 2, 5, 33])
def test_pruned_beam_with_a_running_goal(w, head):
    a, t, s = 3, 5, 33
    z = dy.sine_states(3, s)
    _check_beam(_dyn(s, a, head), z, a, t, w, 0.9, goal=goals(3, s), goal_weight=0.5, goal_mode="running")
    _check_beam(_dyn(s, a, head), z, a, t, w, 1.0, goal=goals(1, s)[0], goal_weight=0.5, goal_mode="running")


# ---- 3: whatever is kept has the bits of its own rollout ----
@pytest.mark.parametrize("mode,head", [(None, True), ("running", True), ("running", False), ("final", True), ("final", False)],
                         ids=["nogoal", "running_head", "running_nohead", "final_head", "final_nohead"])
def test_kept_leaves_and_best_are_their_rollouts(mode, head):
    a, t, s, n = 3, 5, 33, 3
    dyn, z = _dyn(s, a, head), dy.sine_states(n, s)
    kw = {} if mode is None else dict(goal=goals(n, s), goal_weight=0.5, goal_mode=mode)
    for w in (1, 2, 5, 33, 81):
        r = dyn.search(z, t, beam=w, gamma=0.9, keep_leaves=True, **kw)
        plans, rets, bp, br = [host(x).copy() for x in (r.leaf_plans, r.leaf_returns, r.best_plan, r.best_return)]
        assert r.exact == (w == 81) and plans.shape == (n, r.leaves, t)
        rolled = host(dyn.rollout(z, plans, gamma=0.9, **kw).returns)
        assert same_bits(rets, rolled), (mode, w)
        assert same_bits(br, host(dyn.rollout(z, bp[:, None, :], gamma=0.9, **kw).returns)[:, 0]), (mode, w)
        top = np.argmax(rets, axis=1)
        assert np.array_equal(bp, plans[np.arange(n), top]) and same_bits(br, rets[np.arange(n), top])
        assert len({tuple(p) for p in plans[0]}) == r.leaves  # the leaves are pairwise different plans


def test_levels_at_the_limit_of_8192_children():
    """A = 4, W = 2048: levels of 4, 16, 64, 256, 1024, 4096, 8192 and 8192 children — the sort at 4096 and at 8192 words, 256
    tiles an environment."""
    a, t, s, w, n = 4, 8, 3, 2048, 1
    dyn, z = _dyn(s, a), dy.sine_states(n, s)
    r = dyn.search(z, t, beam=w, gamma=0.9, keep_leaves=True)
    plans, rets, bp, br = [host(x).copy() for x in (r.leaf_plans, r.leaf_returns, r.best_plan, r.best_return)]
    assert dyn.route == "rollout" and r.leaves == 8192 and not r.exact and r.expanded == 4 + 16 + 64 + 256 + 1024 + 4096 + 8192 + 8192
    assert same_bits(rets, host(dyn.rollout(z, plans, gamma=0.9).returns))
    top = np.argmax(rets, axis=1)
    assert np.array_equal(bp, plans[np.arange(n), top]) and same_bits(br, rets[np.arange(n), top])
    # the frontier of the last level is the 2048 best prefixes of the level before, best first
    pre = np.ascontiguousarray(plans[:, ::a, :t - 1])
    key = host(dyn.rollout(z, pre, gamma=0.9).returns)
    assert (np.diff(key, axis=1) <= 0).all() and len({tuple(p) for p in pre[0]}) == w


# ---- 4: ties and NaN ----
def test_ties_keep_the_lowest_indices():
    a, t, s = 3, 3, 33
    dyn, z = _dyn(s, a, flat_reward=True), dy.sine_states(2, s)
    r = dyn.search(z, t, beam=2, keep_leaves=True)
    want = np.array([(0, 0, x) for x in range(a)] + [(0, 1, x) for x in range(a)], np.int32)
    assert np.array_equal(host(r.leaf_plans), np.broadcast_to(want, (2,) + want.shape))
    assert (host(r.leaf_returns) == 1.5).all() and not host(r.best_plan).any() and (host(r.best_return) == 1.5).all()
    r = dyn.search(z, t, beam=9)
    assert r.exact and not host(r.best_plan).any()


@pytest.mark.parametrize("w", [2, 9])
def test_a_nan_state_stays_in_its_environment(w):
    a, t, s = 3, 3, 33
    dyn, z = _dyn(s, a), dy.sine_states(3, s)
    clean = dyn.search(z, t, beam=w, gamma=0.9, keep_leaves=True)
    clean = [host(x).copy() for x in (clean.leaf_plans, clean.leaf_returns, clean.best_plan, clean.best_return)]
    bad = z.copy()
    bad[1, 2] = np.nan
    r = dyn.search(bad, t, beam=w, gamma=0.9, keep_leaves=True)
    got = [host(x).copy() for x in (r.leaf_plans, r.leaf_returns, r.best_plan, r.best_return)]
    assert np.isnan(got[3][1]) and not got[2][1].any() and np.isnan(got[1][1]).all()
    for e in (0, 2):
        assert np.array_equal(got[0][e], clean[0][e]) and same_bits(got[1][e], clean[1][e])
        assert np.array_equal(got[2][e], clean[2][e]) and same_bits(got[3][e], clean[3][e])


# ---- 1 again, with goals ----
@pytest.mark.parametrize("head", [True, False], ids=["head", "nohead"])
@pytest.mark.parametrize("goal", ["each", "shared"])
@pytest.mark.parametrize("mode", ["running", "final"])
def test_exact_search_with_a_goal_is_the_enumeration(mode, goal, head):
    a, t, s, n = 3, 4, 33, 3
    dyn, plans, z = _dyn(s, a, head), all_plans(a, t), dy.sine_states(n, s)
    g = goals(n, s) if goal == "each" else goals(1, s)[0]
    r = dyn.search(z, t, beam=a ** (t - 1), gamma=0.9, keep_leaves=True, goal=g, goal_weight=0.5, goal_mode=mode)
    got = [host(x).copy() for x in (r.leaf_plans, r.leaf_returns, r.best_plan, r.best_return)]
    returns, best = _enumerated(s, a, t, n, 0.9, head, goal, mode)
    assert dyn.route == "rollout" and r.exact
    assert np.array_equal(got[0], np.broadcast_to(plans, (n,) + plans.shape)) and same_bits(got[1], returns)
    assert np.array_equal(got[2], plans[best]) and same_bits(got[3], returns[np.arange(n), best])


# ---- 5: hygiene, through the C ABI ----
def _buffer(numel, dtype=torch.float32, fill=F_SENTINEL):
    return torch.full((numel + TAIL,), fill, dtype=dtype, device=_dev())


def _take(buf, shape, fill, name):
    h = buf.cpu()
    numel = h.numel() - TAIL
    assert bool((h[numel:] == fill).all()), "%s: sentinel tail overwritten" % name
    return h[:numel].view(shape).numpy().copy()


@functools.lru_cache(maxsize=None)
def _heads(s, a, h=16):
    return tuple(p.to(_dev()) for p in dy.seeded_heads(s, a, h))


def beam_raw(s, a, n, w, t, gamma=0.9, goal=None, mode=0, keep=True, ws_short=0, head=True):
    """One srlz_beam_search call on seeded heads with a sentinel tail behind every output and behind the workspace.
    Returns ({name: numpy}, status, tickets [n] | None)."""
    from srlz import _cabi as C
    p = _heads(s, a)
    z = torch.from_numpy(dy.sine_states(n, s)).to(_dev())
    leaves = max(C.beam_leaves(w, a, t), 1)
    need = C.beam_workspace(n, w, t, s, a)
    bufs = {"best_plan": _buffer(n * t, torch.int32, I_SENTINEL), "best_return": _buffer(n)}
    if keep:
        bufs["leaf_plans"], bufs["leaf_returns"] = _buffer(n * leaves * t, torch.int32, I_SENTINEL), _buffer(n * leaves)
    ws = _buffer(max(need, 16) - ws_short, torch.uint8, B_SENTINEL)
    gl = None if goal is None else torch.from_numpy(goal).to(_dev())
    status = C._lib.srlz_beam_search(C.ptr(z), C.ptr(p[0]), C.ptr(p[1]), *[C.ptr(x) if head else None for x in p[2:]],
                                     C.ptr(bufs["best_plan"]), C.ptr(bufs["best_return"]), C.ptr(bufs.get("leaf_plans")),
                                     C.ptr(bufs.get("leaf_returns")), C.ptr(ws), max(need, 16) - ws_short, n, w, t, s, a, 16, 2, float(gamma),
                                     C.ptr(gl), 0 if gl is None or gl.dim() == 1 else s, 0.5, mode, C.stream())
    torch.cuda.synchronize()
    shapes = {"best_plan": (n, t), "best_return": (n,), "leaf_plans": (n, leaves, t), "leaf_returns": (n, leaves)}
    out = {q: _take(b, shapes[q], I_SENTINEL if b.dtype == torch.int32 else F_SENTINEL, q) for q, b in bufs.items()}
    raw = _take(ws, (max(need, 16) - ws_short,), B_SENTINEL, "workspace")
    return out, status, raw[:4 * n].view(np.uint32) if need else None


@pytest.mark.parametrize("case", [dict(s=33, a=3, n=3, w=5, t=5), dict(s=33, a=3, n=3, w=27, t=4),
                                  dict(s=33, a=3, n=3, w=5, t=5, goal="each", mode=1), dict(s=200, a=6, n=2, w=7, t=3, goal="shared"),
                                  dict(s=3, a=3, n=1, w=1, t=1)],
                         ids=["beam", "exact", "final_goal", "shared_goal", "one_step"])
def test_two_runs_sentinels_and_tickets(case):
    c = dict(case)
    g = c.pop("goal", None)
    if g is not None:
        c["goal"] = goals(c["n"], c["s"]) if g == "each" else goals(1, c["s"])[0]
    one, status, tickets = beam_raw(**c)
    assert status == 0 and not tickets.any()
    two, status, tickets = beam_raw(**c)
    assert status == 0 and not tickets.any()
    for q in one:
        assert np.array_equal(one[q].view(np.uint32) if one[q].dtype == np.float32 else one[q], two[q].view(np.uint32) if two[q].dtype == np.float32 else two[q]), q
    assert (one["leaf_plans"] >= 0).all() and (one["leaf_plans"] < c["a"]).all() and not (one["best_return"] == F_SENTINEL).any()
    # without the leaves: the same best
    bare, status, _ = beam_raw(keep=False, **c)
    assert status == 0 and np.array_equal(bare["best_plan"], one["best_plan"]) and same_bits(bare["best_return"], one["best_return"])


def test_the_limit_w_times_a_and_the_refusals(cabi):
    from srlz import _cabi as C
    bad_desc, null, short = BAD_DESC, NULL, WORKSPACE
    out, status, tickets = beam_raw(s=3, a=2, n=2, w=4096, t=2)  # W * A = 8192 exactly
    assert status == 0 and not tickets.any() and out["leaf_plans"].shape == (2, 4, 2)
    assert np.array_equal(out["leaf_plans"][0], all_plans(2, 2))
    assert C.beam_supported(3, 2, 16, 2, 1, 4096, 2) == 1 and C.beam_supported(3, 2, 16, 2, 1, 4097, 2) == 0
    assert C.beam_leaves(4097, 2, 2) == 0 and C.beam_workspace(2, 4097, 2, 3, 2) == 0

    def untouched(out):
        return all((v == (I_SENTINEL if v.dtype == np.int32 else np.float32(F_SENTINEL))).all() for v in out.values())
    for kw in (dict(w=4097, a=2, t=2), dict(w=5, a=3, t=33), dict(w=0, a=3, t=3), dict(w=5, a=3, t=0), dict(w=5, a=3, t=3, head=False),
               dict(w=5, a=3, t=3, goal=goals(2, 3), mode=2)):
        out, status, _ = beam_raw(s=3, n=2, **kw)
        assert status == bad_desc and untouched(out), kw
        assert "beam_search" in C.error_text()
    out, status, _ = beam_raw(s=3, a=3, n=2, w=5, t=3, ws_short=1)
    assert status == short and untouched(out)
    assert C._lib.srlz_beam_search(*([None] * 14), 64, 2, 5, 3, 3, 3, 16, 2, 1.0, None, 0, 1.0, 0, C.stream()) == bad_desc
    p, z = _heads(3, 3), torch.from_numpy(dy.sine_states(2, 3)).to(_dev())
    assert C._lib.srlz_beam_search(C.ptr(z), C.ptr(p[0]), C.ptr(p[1]), *[C.ptr(x) for x in p[2:]], None, None, None, None, None, 0, 2, 5,
                                   3, 3, 3, 16, 2, 1.0, None, 0, 1.0, 0, C.stream()) == null
    # the head is optional with a goal
    out, status, _ = beam_raw(s=3, a=3, n=2, w=5, t=3, head=False, goal=goals(2, 3))
    assert status == 0 and not untouched(out)


def test_a_second_smaller_call_is_a_fresh_objects():
    from srlz import deploy
    s, a = 33, 3
    used = deploy.LatentDynamics(_model(s, a), max_rows=8192, max_horizon=8)
    big = used.search(dy.sine_states(3, s), 5, beam=33, gamma=0.9, keep_leaves=True)
    assert big.leaf_returns.shape == (3, 99)
    z = dy.sine_states(2, s)
    again = used.search(z, 3, beam=2, gamma=0.9, keep_leaves=True)
    got = [host(x).copy() for x in (again.leaf_plans, again.leaf_returns, again.best_plan, again.best_return, again.action)]
    fresh = deploy.LatentDynamics(_model(s, a), max_rows=8192, max_horizon=8).search(z, 3, beam=2, gamma=0.9, keep_leaves=True)
    ref = [host(x) for x in (fresh.leaf_plans, fresh.leaf_returns, fresh.best_plan, fresh.best_return, fresh.action)]
    for x, y in zip(got, ref):
        assert x.shape == y.shape and (same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y))
    assert again.leaf_plans is not None and used.search(z, 3, beam=2).leaf_plans is None


# ---- 6: routes ----
def _split_model():
    if "split" not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        torch.manual_seed(1)
        losses = ["autoencoder", "forward", "reward"]
        m = modules.SRLModulesSplit(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=losses,
                                    split_dimensions=OrderedDict(zip(losses, (4, 2, 2))))
        _MODELS["split"] = m.to(_dev()).eval()
    return _MODELS["split"]


def test_routes():
    from srlz import deploy
    a, t, s, n = 6, 2, 8, 3
    z, plans = dy.sine_states(n, s), all_plans(a, t)
    plain = deploy.LatentDynamics(_model(s, a), max_rows=256, max_horizon=8)
    r = plain.search(z, t, beam=a, keep_leaves=True)
    assert plain.route == "rollout" and deploy.search_route_for(_model(s, a), a, t, n, 256) == "rollout"
    split = deploy.LatentDynamics(_split_model())
    small = deploy.LatentDynamics(_model(s, a), max_rows=8, max_horizon=8)  # 3 * 36 children > 8
    assert deploy.search_route_for(_split_model(), a, t, n) == "model" and deploy.search_route_for(_model(s, a), a, t, n, 8) == "model"
    g = goals(n, s)
    for dyn in (split, small):
        for kw in ({}, dict(goal=g, goal_weight=0.5, goal_mode="running"), dict(goal=g, goal_weight=0.5, goal_mode="final")):
            got = dyn.search(z, t, beam=a, gamma=0.9, keep_leaves=True, **kw)
            assert dyn.route == "model" and got.exact and got.best_plan.device.type == "cuda" and got.best_plan.dtype == torch.int32
            out = dyn.rollout(z, plans, gamma=0.9, **kw)
            assert dyn.route == "model"
            returns, best = host(out.returns), host(out.best)
            assert np.array_equal(host(got.leaf_plans), np.broadcast_to(plans, (n,) + plans.shape))
            assert same_bits(got.leaf_returns, returns)
            assert np.array_equal(host(got.best_plan), plans[best]) and same_bits(got.best_return, returns[np.arange(n), best])
            assert np.array_equal(host(got.action), plans[best][:, 0]) and got.action.dtype == torch.int64
    # beyond the kernel's horizon and beam: nothing is rejected for size
    long = small.search(z[0], 33, beam=1)
    assert small.route == "model" and long.best_plan.shape == (33,) and long.leaves == a and not long.exact
    with pytest.raises(ValueError, match="never trained"):
        deploy.LatentDynamics(_model(s, a, ["forward", "inverse"]), max_rows=256, max_horizon=8).search(z, t)
    with pytest.raises(ValueError, match="at least 1"):
        plain.search(z, 0)
    with pytest.raises(ValueError, match="goal_mode"):
        plain.search(z, t, goal=g, goal_mode="nearest")
    assert same_bits(r.leaf_returns, host(plain.rollout(z, plans).returns))


def test_reach_with_the_search_planner_is_search_on_the_encoders_states():
    from srlz import deploy
    import models.modules as modules
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    torch.manual_seed(5)
    model = modules.SRLModules(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=["autoencoder", "forward", "inverse"]).to(_dev())
    model.eval()
    frames = du.frames_nhwc(4, 224, 224, 3)
    now, then = frames[:2], frames[2:]
    now_d, then_d = torch.from_numpy(now).to(_dev()), torch.from_numpy(then).to(_dev())
    dyn = deploy.LatentDynamics(model, max_rows=256, max_horizon=8)
    enc = deploy.StateEncoder(model, max_batch=2)
    kw = dict(beam=7, goal_mode="final", keep_leaves=True)
    fields = ("best_plan", "best_return", "action", "leaf_plans", "leaf_returns")
    got = deploy.reach(enc, dyn, now, then, 3, planner="search", **kw)
    got = [getattr(got, q).clone() for q in fields]
    assert dyn.route == "rollout" and got[0].shape == (2, 3) and got[3].shape == (2, 42, 3)
    s_now, s_then = enc(now_d).clone(), enc(then_d).clone()
    ref = dyn.search(s_now, 3, goal=s_then, **kw)
    for x, q in zip(got, fields):
        assert torch.equal(x, getattr(ref, q)), q
    with pytest.raises(ValueError, match="planner"):
        deploy.reach(enc, dyn, now, then, 3, planner="greedy")
