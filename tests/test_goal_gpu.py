"""Goal-distance scores on the GPU: srlz_rollout_goal and srlz_plan_cem_goal through the C ABI, and LatentDynamics' goal arguments.

Shapes, the smallest at which the tile can go wrong: S in {1, 31, 32, 33, 200, 512} (below, on and above the goal sum's 16 column
groups and the 32-k chunk; the limit), rows 1, srlz_rollout_tile() and tile + 1, N = 5 with K = 7 (35 rows: two tiles, and tiles that
straddle environments with different goals), T in {1, 7, 32}, A in {1, 6}, a reward head of H in {1, 16, 32} and none.
What is held, and to what:
  1  trajectory, final_states and reward_logits are srlz_rollout's bits;
  2  goal_dist against fp64 from the kernel's own fp32 trajectory: |d - d64| <= (S + 4) 2^-24 d64 (one rounding for the difference —
     twice in the square —, one for the square, at most S - 1 for the sum, fadd or fma), every term non-negative;
  3  without a head, returns are the numpy-float32 restatement from the kernel's own goal_dist, bit for bit;
  4  with a head, returns against fp64 from the kernel's own logits and goal_dist within (T + 16) 2^-24 sum_t g_t (p_t + w c_t)
     (expf within 1 ulp, the division, five roundings a term, T adds);
  5  against the unmodified reference's fixture (tests/golden/goal_kats.npz) within max(1e-4, 10 x its own fp32-to-fp64 spread), and
     act(goal=..., goal_mode="final") takes plan k*'s first action;
  6  bit properties: two runs, a shared goal and the goal tiled, a row alone and among others, T steps and T calls of one step, an
     action out of range;
  7  the planner: the integer world against cem_host exactly; seeded float heads against the restatement of plan_util fed the kernel's
     own scores; the same seed, the same bits;
  8  every refusal's code, with nothing written (a sentinel tail — and body — behind every output);
  9  route "model" (a split model, a call beyond max_rows) and reach()."""
import copy
import functools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import deploy_util as du
import dynamics_util as dy
import goal_util as gu
import plan_util as pu

pytestmark = pytest.mark.gpu

F_SENTINEL, I_SENTINEL, B_SENTINEL = 1234.5, -77, 0xAB
TAIL = 64
ALL = ("final", "returns", "trajectory", "reward_logits", "goal_dist")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_MODELS = {}


def _dev():
    return torch.device("cuda", 0)


def _buffer(numel, dtype=torch.float32, fill=F_SENTINEL):
    return torch.full((numel + TAIL,), fill, dtype=dtype, device=_dev())


def _take(buf, shape, fill, name):
    host = buf.cpu()
    numel = host.numel() - TAIL
    assert bool((host[numel:] == fill).all()), "%s: sentinel tail overwritten" % name
    return host[:numel].view(shape).numpy().copy()


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def goals(n, s):
    """fp32 [n, s]: cos(0.23 i + 0.07 j) + 0.25 — a different goal for every environment."""
    i, j = np.meshgrid(np.arange(n), np.arange(s), indexing="ij")
    return (np.cos(0.23 * i + 0.07 * j) + 0.25).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(s, a, h, n, k, t):
    """Seeded heads, states, plans and goals of one shape (host and device), made once and shared."""
    params = dy.seeded_heads(s, a, h)
    z, pl, gl = dy.sine_states(n, s), dy.plans(n, k, t, a), goals(n, s)
    dev = _dev()
    return dict(params_dev=tuple(p.to(dev) for p in params), z=z, pl=pl, gl=gl, z_dev=torch.from_numpy(z).to(dev),
                pl_dev=torch.from_numpy(pl).to(dev), gl_dev=torch.from_numpy(gl).to(dev), dims=(s, a, h, n, k, t))


def roll(pb, head=True, goal=True, mode=0, weight=1.0, gamma=1.0, want=ALL, raw=False, z_dev=None, pl_dev=None, gl_dev=None, n=None, k=None,
         t=None, **over):
    """One srlz_rollout_goal call (goal=False: srlz_rollout on the same inputs).  Returns ({name: numpy}, status); every tail checked."""
    from srlz import _cabi as C
    s, a, h, n0, k0, t0 = pb["dims"]
    n, k, t = n0 if n is None else n, k0 if k is None else k, t0 if t is None else t
    nn, kk, tt = max(n, 1), max(k, 1), max(t, 1)
    sizes = {"final": (nn, kk, s), "returns": (nn, kk), "trajectory": (nn, kk, tt, s), "reward_logits": (nn, kk, tt, 2), "goal_dist": (nn, kk, tt)}
    want = [q for q in want if goal or q != "goal_dist"]
    bufs = {q: _buffer(int(np.prod(sizes[q]))) for q in want}
    p = pb["params_dev"]
    heads = [C.ptr(x) for x in p[2:]] if head is True else [None] * 6 if head is False else [C.ptr(x) if i in head else None for i, x in enumerate(p[2:])]
    pl_dev = pb["pl_dev"] if pl_dev is None else pl_dev
    gl_dev = pb["gl_dev"] if gl_dev is None else gl_dev
    args = [C.ptr(pb["z_dev"] if z_dev is None else z_dev), C.ptr(pl_dev), over.get("plan_stride", k * t if pl_dev.dim() == 3 else 0), C.ptr(p[0]),
            C.ptr(p[1])] + heads + [C.ptr(bufs.get(q)) for q in ALL[:4]] + \
           [n, k, t, over.get("s", s), a, over.get("h", h), over.get("n_rewards", 2), float(gamma)]
    if goal:
        args += [None if over.get("no_goal") else C.ptr(gl_dev), over.get("goal_stride", s if gl_dev.dim() == 2 else 0), float(weight), mode,
                 C.ptr(bufs.get("goal_dist"))]
    args.append(C.stream())
    name = "rollout_goal" if goal else "rollout"
    status = getattr(C._lib, "srlz_" + name)(*args) if raw else getattr(C, name)(*args)
    torch.cuda.synchronize()
    return {q: _take(b, sizes[q], F_SENTINEL, q) for q, b in bufs.items()}, status


#          S    A   H     N   K   T      (H = None: no reward head)
SHAPES = [(1, 1, 1, 1, 1, 1),
          (1, 6, None, 1, 33, 7),      # tile + 1 rows, the narrowest state
          (31, 6, 16, 1, 32, 7),       # exactly one tile
          (32, 6, 32, 1, 33, 7),
          (33, 1, 16, 5, 7, 7),        # 35 rows of five environments: both tiles straddle goals
          (33, 6, None, 1, 1, 32),
          (200, 6, 16, 5, 7, 7),
          (200, 6, None, 5, 7, 32),
          (200, 6, 1, 1, 32, 32),
          (512, 6, 32, 1, 33, 7),      # both limits
          (512, 6, None, 5, 7, 1)]
IDS = ["S%d_A%d_H%s_N%d_K%d_T%d" % v for v in SHAPES]


def _pb(shape):
    s, a, h, n, k, t = shape
    return problem(s, a, h or 16, n, k, t), h is not None


@functools.lru_cache(maxsize=None)
def _rolled(shape, mode, gamma, weight, head):
    pb, _ = _pb(shape)
    return roll(pb, head=head, mode=mode, gamma=gamma, weight=weight, want=ALL if head else [q for q in ALL if q != "reward_logits"])[0]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_states_and_logits_are_srlz_rollouts_bits(shape):
    from srlz import _cabi as C
    assert C.rollout_tile() == 32  # (the shapes above are sized by it)
    pb, head = _pb(shape)
    got = _rolled(shape, 0, 0.9, 0.5, head)
    ref = roll(pb, head=head, goal=False, gamma=0.9, want=ALL[:4] if head else ("final", "trajectory"))[0]
    for q in ("final", "trajectory") + (("reward_logits",) if head else ()):
        assert same_bits(got[q], ref[q]), q
    assert same_bits(got["final"], got["trajectory"][:, :, -1])
    # every optional output may be absent: the others keep their bits
    lean = roll(pb, head=head, gamma=0.9, weight=0.5, want=("final", "returns"))[0]
    assert same_bits(lean["final"], got["final"]) and same_bits(lean["returns"], got["returns"])
    only = roll(pb, head=head, gamma=0.9, weight=0.5, want=("final", "goal_dist"))[0]
    assert same_bits(only["goal_dist"], got["goal_dist"])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_goal_dist_against_fp64_of_the_kernels_own_trajectory(shape):
    pb, head = _pb(shape)
    s = shape[0]
    got = _rolled(shape, 0, 0.9, 0.5, head)
    d64 = gu.dist(got["trajectory"], pb["gl"], np.float64)
    err = np.abs(got["goal_dist"].astype(np.float64) - d64)
    worst = float((err / np.maximum(d64, 1e-300)).max())
    print("goal_dist %s: max |d - d64| / d64 = %.3g ulp-units of 2^-24 (bound %d)" % (IDS[SHAPES.index(shape)], worst * 2 ** 24, s + 4))
    assert np.isfinite(got["goal_dist"]).all() and (got["goal_dist"] >= 0).all() and d64.max() > 0
    assert (err <= gu.dist_bound_terms(s) * d64).all(), worst
    # both modes keep the same distances
    assert same_bits(_rolled(shape, 1, 0.9, 0.5, head)["goal_dist"], got["goal_dist"])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_returns_without_a_head_are_the_float32_restatement_bit_for_bit(shape):
    for mode in (0, 1):
        for gamma in (1.0, 0.9):
            got = _rolled(shape, mode, gamma, 0.5, False)
            ref = gu.scores(got["goal_dist"], None, gamma, 0.5, gu.MODES[mode], np.float32)
            assert same_bits(got["returns"], ref), (mode, gamma)
            assert (got["returns"] <= 0).all() and got["returns"].min() < 0
    # another weight, one that rounds
    got = _rolled(shape, 0, 0.9, 0.3, False)
    assert same_bits(got["returns"], gu.scores(got["goal_dist"], None, 0.9, 0.3, "running", np.float32))


@pytest.mark.parametrize("shape", [v for v in SHAPES if v[2] is not None], ids=[i for i, v in zip(IDS, SHAPES) if v[2] is not None])
def test_returns_with_a_head_against_fp64_of_the_kernels_own_logits_and_distances(shape):
    t = shape[5]
    for mode in (0, 1):
        for gamma in (1.0, 0.9):
            got = _rolled(shape, mode, gamma, 0.5, True)
            p64, d64 = gu.probs(got["reward_logits"], np.float64), got["goal_dist"].astype(np.float64)
            ref = gu.scores(d64, p64, gamma, 0.5, gu.MODES[mode], np.float64)
            mass = gu.scores(-d64, p64, gamma, 0.5, gu.MODES[mode], np.float64)  # sum_t g_t (p_t + w c_t)
            err = np.abs(got["returns"].astype(np.float64) - ref)
            print("score %s mode %d gamma %.1f: max err / (2^-24 mass) = %.3g (bound %d)"
                  % (IDS[SHAPES.index(shape)], mode, gamma, float((err / mass).max()) * 2 ** 24, t + 16))
            assert (mass > 0).all() and (err <= (t + 16) * 2.0 ** -24 * mass).all(), (mode, gamma)
    # in final mode the steps before the last add the reward term alone: with T = 1 both modes are one
    if t == 1:
        assert same_bits(_rolled(shape, 0, 0.9, 0.5, True)["returns"], _rolled(shape, 1, 0.9, 0.5, True)["returns"])


# ---- 6: bit properties ----
def test_two_runs_and_a_shared_goal_and_the_goal_tiled():
    shape = (200, 6, 16, 5, 7, 7)
    pb, _ = _pb(shape)
    for head in (True, False):
        want = ALL if head else [q for q in ALL if q != "reward_logits"]
        one, two = roll(pb, head=head, gamma=0.9, weight=0.5, want=want)[0], roll(pb, head=head, gamma=0.9, weight=0.5, want=want)[0]
        for q in want:
            assert same_bits(one[q], two[q]), q
        shared = roll(pb, head=head, gamma=0.9, weight=0.5, want=want, gl_dev=pb["gl_dev"][3].contiguous())[0]
        tiled = roll(pb, head=head, gamma=0.9, weight=0.5, want=want, gl_dev=pb["gl_dev"][3:4].repeat(5, 1).contiguous())[0]
        for q in want:
            assert same_bits(shared[q], tiled[q]), q
        assert same_bits(shared["goal_dist"][3], one["goal_dist"][3]) and not same_bits(shared["goal_dist"][2], one["goal_dist"][2])
        # shared plans [K,T] under per-environment goals: the bits of the same plans tiled
        sp = roll(pb, head=head, gamma=0.9, weight=0.5, want=want, pl_dev=pb["pl_dev"][1].contiguous())[0]
        tp = roll(pb, head=head, gamma=0.9, weight=0.5, want=want, pl_dev=pb["pl_dev"][1:2].repeat(5, 1, 1).contiguous())[0]
        for q in want:
            assert same_bits(sp[q], tp[q]), q


@pytest.mark.parametrize("head", [True, False], ids=["head", "nohead"])
def test_a_row_does_not_depend_on_the_other_rows_of_the_call(head):
    shape = (33, 6, 16, 5, 7, 7)
    pb, _ = _pb(shape)
    want = ("final", "returns", "goal_dist")
    whole = roll(pb, head=head, gamma=0.9, weight=0.5, want=want)[0]
    for n, k in ((0, 0), (2, 3), (4, 6)):  # row 17 sits in the middle of tile 0, row 34 in tile 1
        alone = roll(pb, head=head, gamma=0.9, weight=0.5, want=want, n=1, k=1, z_dev=pb["z_dev"][n:n + 1].contiguous(),
                     pl_dev=pb["pl_dev"][n, k:k + 1].unsqueeze(0).contiguous(), gl_dev=pb["gl_dev"][n:n + 1].contiguous())[0]
        for q in want:
            assert same_bits(alone[q][0, 0], whole[q][n, k]), (q, n, k)


@pytest.mark.parametrize("head", [True, False], ids=["head", "nohead"])
def test_t_steps_agree_with_t_calls_of_one_step(head):
    shape = (200, 6, 16, 5, 7, 7)
    pb, _ = _pb(shape)
    s, a, h, n, k, t = pb["dims"]
    whole = roll(pb, head=head, want=("final", "returns", "goal_dist"))[0]  # running mode, gamma = 1, w = 1
    # rows become environments: [n*k] states, one plan of one step each, each row its own environment's goal
    cur = pb["z_dev"].repeat_interleave(k, dim=0).contiguous()
    gl = pb["gl_dev"].repeat_interleave(k, dim=0).contiguous()
    for step in range(t):
        one = roll(pb, head=head, want=("final", "returns", "goal_dist"), n=n * k, k=1, t=1, z_dev=cur,
                   pl_dev=pb["pl_dev"][:, :, step].reshape(n * k, 1, 1).contiguous(), gl_dev=gl)[0]
        assert same_bits(one["goal_dist"].reshape(n, k), whole["goal_dist"][:, :, step]), step
        if not head:  # a one-step score is -fl(w * d)
            assert same_bits(one["returns"].reshape(n, k), -whole["goal_dist"][:, :, step])
        cur = torch.from_numpy(one["final"].reshape(n * k, s)).to(_dev())
    assert same_bits(one["final"].reshape(n, k, s), whole["final"])


@pytest.mark.parametrize("bad_action", [6, -1])
def test_an_action_out_of_range_turns_its_row_nan_from_that_step_on(bad_action):
    shape = (33, 6, 16, 5, 7, 7)
    pb, _ = _pb(shape)
    pl = pb["pl"].copy()
    pl[2, 3, 4] = bad_action  # row 17, step 4
    pl_dev = torch.from_numpy(pl).to(_dev())
    for head in (True, False):
        want = ALL if head else [q for q in ALL if q != "reward_logits"]
        for mode in (0, 1):
            well = roll(pb, head=head, mode=mode, gamma=0.9, weight=0.5, want=want)[0]
            sick = roll(pb, head=head, mode=mode, gamma=0.9, weight=0.5, want=want, pl_dev=pl_dev)[0]
            assert np.isnan(sick["goal_dist"][2, 3, 4:]).all() and np.isnan(sick["returns"][2, 3]) and np.isnan(sick["final"][2, 3]).all()
            assert same_bits(sick["goal_dist"][2, 3, :4], well["goal_dist"][2, 3, :4])
            mask = np.ones((5, 7), bool)
            mask[2, 3] = False
            for q in want:
                assert same_bits(sick[q][mask], well[q][mask]), q


# ---- 7: the planner ----
def cem(pb, k, t, head=True, mode=0, weight=1.0, gamma=0.9, iterations=1, elites=1, q=8, seed=0, keep=True, raw=False, z_dev=None,
        gl_dev=None, n=None, short_ws=0, **over):
    """One srlz_plan_cem_goal call.  Returns (dict of numpy arrays, status); every sentinel tail is checked here."""
    from srlz import _cabi as C
    s, a, h = pb["dims"][:3]
    n = pb["dims"][3] if n is None else n
    nn, kk, tt, ii = max(n, 1), max(k, 1), max(t, 1), max(iterations, 1)
    ws_bytes = max(int(C.plan_goal_workspace(nn, min(kk, 1024), min(tt, 32), int(keep))), nn * 8) - short_ws
    bufs = dict(best_plan=_buffer(nn * tt, torch.int32, I_SENTINEL), best_return=_buffer(nn), cum=_buffer(nn * tt * a, torch.int32, I_SENTINEL),
                ws=_buffer(ws_bytes, torch.uint8, B_SENTINEL))
    if keep:
        bufs["plans"] = _buffer(ii * nn * kk * tt, torch.int32, I_SENTINEL)
        bufs["returns"] = _buffer(ii * nn * kk)
    p = pb["params_dev"]
    heads = [C.ptr(x) for x in p[2:]] if head is True else [None] * 6 if head is False else [C.ptr(x) if i in head else None for i, x in enumerate(p[2:])]
    gl_dev = pb["gl_dev"] if gl_dev is None else gl_dev
    args = [C.ptr(pb["z_dev"] if z_dev is None else z_dev), C.ptr(p[0]), C.ptr(p[1])] + heads + \
           [None, over.get("init_stride", 0), C.ptr(bufs["best_plan"]), C.ptr(bufs["best_return"]), C.ptr(bufs["cum"]),
            C.ptr(bufs.get("plans")), None if over.get("half") else C.ptr(bufs.get("returns")), C.ptr(bufs["ws"]), ws_bytes, n, k, t,
            over.get("s", s), a, over.get("h", h), over.get("n_rewards", 2), iterations, elites, q, float(gamma), seed,
            None if over.get("no_goal") else C.ptr(gl_dev), over.get("goal_stride", s if gl_dev.dim() == 2 else 0), float(weight), mode,
            C.stream()]
    status = C._lib.srlz_plan_cem_goal(*args) if raw else C.plan_cem_goal(*args)
    torch.cuda.synchronize()
    fills = dict(best_plan=I_SENTINEL, best_return=F_SENTINEL, cum=I_SENTINEL, ws=B_SENTINEL, plans=I_SENTINEL, returns=F_SENTINEL)
    shapes = dict(best_plan=(nn, tt), best_return=(nn,), cum=(nn, tt, a), ws=(ws_bytes,), plans=(ii, nn, kk, tt), returns=(ii, nn, kk))
    out = {name: _take(b, shapes[name], fills[name], name) for name, b in bufs.items()}
    out["cum"] = out["cum"].view(np.uint32)
    out["tickets"] = out["ws"][:nn * 4].copy().view(np.uint32)
    return out, status


def _world():
    """The integer world of goal_util as a problem: two environments at the origin, one shared goal."""
    if "world" not in _MODELS:
        wf, bf = gu.world_heads()
        dev = _dev()
        filler = dy.seeded_heads(2, 4, 16)[2:]  # (a head that is never given)
        z = np.zeros((2, 2), np.float32)
        _MODELS["world"] = dict(params_dev=(torch.from_numpy(wf).to(dev), torch.from_numpy(bf).to(dev)) + tuple(x.to(dev) for x in filler),
                                z=z, z_dev=torch.from_numpy(z).to(dev), gl_dev=torch.from_numpy(gu.WORLD_GOAL).to(dev), dims=(2, 4, 16, 2))
    return _MODELS["world"]


@pytest.mark.parametrize("mode,want", [(0, -14.0), (1, 0.0)], ids=["running", "final"])
def test_planner_on_the_integer_world_is_cem_host_exactly(mode, want):
    from srlz import deploy
    w = gu.WORLD
    got = cem(_world(), w["k"], w["t"], head=False, mode=mode, gamma=1.0, iterations=w["iterations"], elites=w["elites"], q=w["q"],
              seed=w["seed"])[0]
    ref = deploy.cem_host(lambda pl: deploy.goal_scores(gu.world_trajectory(pl), gu.WORLD_GOAL, None, 1.0, 1.0, gu.MODES[mode])[0], 2, w["k"],
                          w["t"], w["a"], w["iterations"], w["elites"], w["q"], w["seed"], keep_population=True)
    assert np.array_equal(got["best_plan"], ref["best_plan"]) and not got["best_plan"].any()
    assert same_bits(got["best_return"], ref["best_return"]) and (got["best_return"] == want).all()
    assert np.array_equal(got["cum"], ref["cum"])
    assert np.array_equal(deploy.weights_of_table(got["cum"]), deploy.weights_of_table(ref["cum"]))
    assert np.array_equal(got["plans"], ref["plans"]) and same_bits(got["returns"], ref["returns"])
    assert not got["tickets"].any()


@pytest.mark.parametrize("shape", [(3, 6, 16, 3, 33, 5, True), (200, 6, 16, 2, 64, 10, True), (200, 6, 16, 2, 64, 10, False),
                                   (33, 6, 32, 1, 257, 7, False), (512, 6, 32, 2, 40, 32, True)],
                         ids=lambda v: "S%d_A%d_H%d_N%d_K%d_T%d_head%d" % v)
def test_planner_iterations_are_the_restatement_over_the_kernels_own_scores(shape):
    s, a, h, n, k, t, head = shape
    pb = problem(s, a, h, n, 1, 1)
    kw = dict(head=head, mode=0, weight=0.5, gamma=0.9, elites=min(8, k), q=8, seed=2 ** 40 + 5)
    got = cem(pb, k, t, iterations=3, **kw)[0]
    # every iteration's elite set, best and refit, restated in numpy from the kernel's own scores
    ref = pu.cem(None, n, k, t, a, 3, kw["elites"], 8, kw["seed"], given=list(got["returns"]))
    assert np.array_equal(got["plans"], ref["plans"]) and np.array_equal(got["cum"], ref["cums"][3])
    assert np.array_equal(got["best_plan"], ref["best_plan"]) and same_bits(got["best_return"], ref["best_return"])
    for upto in (1, 2):  # (a run of j iterations leaves the table the j-th refit made)
        part = cem(pb, k, t, iterations=upto, **kw)[0]
        assert np.array_equal(part["cum"], ref["cums"][upto]) and same_bits(part["returns"], got["returns"][:upto]), upto
    # the scores are srlz_rollout_goal's bits for the same plans (one text), in both modes
    for i in range(3):
        pl_dev = torch.from_numpy(got["plans"][i]).to(_dev())
        same = roll(pb, head=head, weight=0.5, gamma=0.9, want=("final", "returns"), k=k, t=t, pl_dev=pl_dev)[0]
        assert same_bits(same["returns"], got["returns"][i]), i
    final = cem(pb, k, t, iterations=1, **dict(kw, mode=1))[0]
    pl_dev = torch.from_numpy(final["plans"][0]).to(_dev())
    assert same_bits(roll(pb, head=head, mode=1, weight=0.5, gamma=0.9, want=("final", "returns"), k=k, t=t, pl_dev=pl_dev)[0]["returns"],
                     final["returns"][0])
    assert np.isfinite(got["returns"]).all() and got["returns"].std() > 0 and not got["tickets"].any()
    # without the population the same results; the same seed the same bits; another seed another population
    lean = cem(pb, k, t, iterations=3, keep=False, **kw)[0]
    again = cem(pb, k, t, iterations=3, **kw)[0]
    for name in ("best_plan", "cum", "best_return"):
        assert np.array_equal(lean[name].view(np.uint32), got[name].view(np.uint32)), name
    for name in ("plans", "returns", "best_plan", "best_return", "cum"):
        assert np.array_equal(again[name].view(np.uint32), got[name].view(np.uint32)), name
    assert not np.array_equal(cem(pb, k, t, iterations=1, **dict(kw, seed=7))[0]["plans"], got["plans"][:1])


def test_planner_reads_a_nan_score_as_minus_infinity():
    n, k, t, e, q = 3, 70, 5, 8, 8
    pb = problem(8, 6, 16, n, 1, 1)
    z = pb["z"].copy()
    z[1, 2] = np.nan
    z_dev = torch.from_numpy(z).to(_dev())
    for head in (True, False):
        sick = cem(pb, k, t, head=head, iterations=2, elites=e, q=q, z_dev=z_dev)[0]
        well = cem(pb, k, t, head=head, iterations=2, elites=e, q=q)[0]
        assert np.isnan(sick["returns"][:, 1]).all() and np.isnan(sick["best_return"][1])
        assert np.array_equal(sick["best_plan"][1], sick["plans"][0, 1, 0])       # every key -inf: ties go to the lowest k
        assert np.array_equal(sick["cum"][1], pu.refit(sick["plans"][1, 1, :e], 6, q))
        for env in (0, 2):  # the neighbours keep the bits they have without it
            for name in ("plans", "returns"):
                assert np.array_equal(sick[name][:, env].view(np.uint32), well[name][:, env].view(np.uint32)), (env, name)
            for name in ("best_plan", "best_return", "cum"):
                assert np.array_equal(sick[name][env].view(np.uint32), well[name][env].view(np.uint32)), (env, name)


# ---- 8: refusals ----
ROLL_REFUSED = [(dict(head=(0, 1, 2, 3, 4)), -1), (dict(head=(1,)), -1), (dict(s=513), -1), (dict(s=0), -1), (dict(h=33), -1), (dict(n_rewards=3), -1),
                (dict(n=0), -1), (dict(k=0), -1), (dict(t=0), -1), (dict(plan_stride=5), -1), (dict(weight=0.0), -1), (dict(weight=-1.0), -1),
                (dict(weight=float("nan")), -1), (dict(weight=float("inf")), -1), (dict(mode=2), -1), (dict(mode=-1), -1), (dict(goal_stride=7), -1),
                (dict(goal_stride=66), -1), (dict(head=False, want=("final", "reward_logits")), -1), (dict(no_goal=True), -4),
                (dict(want=("returns",)), -4)]


@pytest.mark.parametrize("case,code", ROLL_REFUSED, ids=lambda c: "_".join("%s%s" % kv for kv in c.items()) if isinstance(c, dict) else str(c))
def test_a_refused_rollout_returns_its_code_and_writes_nothing(case, code):
    from srlz import _cabi as C
    pb = problem(33, 6, 16, 5, 7, 7)
    kw = dict(raw=True)
    kw.update(case)
    out, status = roll(pb, **kw)
    assert status == code, (status, C.error_text())
    assert "rollout_goal" in C.error_text()
    for q, v in out.items():
        assert (v == F_SENTINEL).all(), q
    with pytest.raises(C.SrlzError, match="rollout_goal"):
        roll(pb, **dict(kw, raw=False))


PLAN_REFUSED = [(dict(head=(0, 2, 4)), -1), (dict(k=1025), -1), (dict(k=0), -1), (dict(t=33), -1), (dict(t=0), -1), (dict(n=0), -1), (dict(s=513), -1),
                (dict(h=33), -1), (dict(n_rewards=3), -1), (dict(iterations=0), -1), (dict(elites=0), -1), (dict(elites=34), -1), (dict(q=-1), -1),
                (dict(q=4097), -1), (dict(init_stride=7), -1), (dict(half=True), -1), (dict(weight=0.0), -1), (dict(weight=float("nan")), -1),
                (dict(weight=float("-inf")), -1), (dict(mode=2), -1), (dict(goal_stride=1), -1), (dict(no_goal=True), -4), (dict(short_ws=1), -2),
                (dict(short_ws=1, keep=False), -2)]


@pytest.mark.parametrize("case,code", PLAN_REFUSED, ids=lambda c: "_".join("%s%s" % kv for kv in c.items()) if isinstance(c, dict) else str(c))
def test_a_refused_plan_returns_its_code_and_writes_nothing(case, code):
    from srlz import _cabi as C
    pb = problem(3, 6, 16, 2, 1, 1)
    kw = dict(k=33, t=5, iterations=2, elites=8, q=8, raw=True)
    kw.update(case)
    out, status = cem(pb, **kw)
    assert status == code, (status, C.error_text())
    assert "plan_cem_goal" in C.error_text()
    for name, fill in (("best_plan", I_SENTINEL), ("plans", I_SENTINEL), ("best_return", F_SENTINEL), ("returns", F_SENTINEL), ("ws", B_SENTINEL)):
        if name in out:
            assert (out[name] == fill).all(), name
    assert (out["cum"].view(np.int32) == I_SENTINEL).all()


def test_the_head_is_optional_for_the_planner_and_returns_are_allowed_without_it():
    pb = problem(3, 6, 16, 2, 1, 1)
    out, status = cem(pb, 33, 5, head=False, iterations=2, elites=8, raw=True)
    assert status == 0 and np.isfinite(out["returns"]).all() and (out["returns"] < 0).all()
    out, status = roll(problem(33, 6, 16, 5, 7, 7), head=False, raw=True, want=("final", "returns"))
    assert status == 0 and (out["returns"] < 0).all()


# ---- 5: the unmodified reference's fixture, through LatentDynamics ----
def _model(name, losses=None):
    key = (name, tuple(losses) if losses else None)
    if key not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        m = dy.build_case(name, modules).to(_dev())
        if losses is not None:  # the same seeded weights under losses that trained no reward head
            m = copy.deepcopy(m)
            m.losses = list(losses)
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "goal_kats.npz"), allow_pickle=False) as z:
        kats = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "goal_spread.json")) as f:
        spread = json.load(f)
    return kats, spread


@pytest.mark.parametrize("name", list(dy.CASES))
def test_against_the_unmodified_reference(name, golden):
    from srlz import deploy
    kats, spread = golden
    sp = spread["cases"][name]
    z, plans = gu.case_inputs(name)
    goal = kats[name + "/goal"]
    with_head = deploy.LatentDynamics(_model(name), max_rows=16, max_horizon=8)
    without = deploy.LatentDynamics(_model(name, ["forward", "inverse"]), max_rows=16, max_horizon=8)
    assert without.heads == ("forward", "inverse")
    for key in gu.SCORE_KEYS:
        mode, head = key.split("_")
        dyn = with_head if head == "head" else without
        out = dyn.rollout(z, plans, gamma=gu.GAMMA, goal=goal, goal_weight=gu.WEIGHT, goal_mode=mode, keep_goal_dist=True)
        assert dyn.route == "rollout" and out.returns.shape == (dy.N_ENVS, dy.N_PLANS) and out.goal_dist.shape == plans.shape
        assert (out.reward_logits is None) and (out.trajectory is None)
        e_dist = dy.rel_err(out.goal_dist.cpu().numpy()[..., None], kats[name + "/goal_dist64"][..., None], True)
        e_score = dy.rel_err(out.returns.cpu().numpy(), kats["%s/%s64" % (name, key)], False)
        print("%s %s: goal_dist %.2e (bound %.2e), score %.2e (bound %.2e)"
              % (name, key, e_dist, dy.bound(sp["goal_dist"]), e_score, dy.bound(sp[key])))
        assert e_dist <= dy.bound(sp["goal_dist"]) and e_score <= dy.bound(sp[key]), (key, e_dist, e_score)
        assert torch.equal(out.best.cpu(), torch.from_numpy(np.nan_to_num(out.returns.cpu().numpy(), nan=-np.inf).argmax(axis=1)))
        if mode == "final" and head == "nohead":
            assert (out.best.cpu().numpy() == gu.KSTAR).all()
    # act ranks by the score with gamma = 1: plan k*'s first action in every environment, with the head and without it
    want = plans[np.arange(dy.N_ENVS), gu.KSTAR, 0]
    for dyn in (with_head, without):
        a = dyn.act(z, plans, goal=goal, goal_weight=gu.ACT_WEIGHT, goal_mode="final")
        assert a.dtype == torch.int64 and a.device.type == "cuda" and np.array_equal(a.cpu().numpy(), want), (a, want)
        best = dyn.rollout(z, plans, goal=goal, goal_weight=gu.ACT_WEIGHT, goal_mode="final").best
        assert (best.cpu().numpy() == gu.KSTAR).all()
    # a bare state, a bare plan and a shared goal drop their axes
    one = with_head.rollout(z[1], plans[1, 2], gamma=gu.GAMMA, goal=goal[1], goal_weight=gu.WEIGHT, keep_goal_dist=True)
    assert one.returns.shape == () and one.goal_dist.shape == (dy.HORIZON,) and one.best.shape == ()
    assert with_head.act(z[1], plans[1], goal=goal[1], goal_mode="final").shape == ()


def test_a_call_without_a_goal_is_todays_call_and_the_gating_holds():
    from srlz import deploy
    z, plans = gu.case_inputs("s8_mlp")
    dyn = deploy.LatentDynamics(_model("s8_mlp"), max_rows=16, max_horizon=8)
    plain = dyn.rollout(z, plans, gamma=0.9, keep_logits=True)
    assert plain.goal_dist is None and plain.returns is not None
    kept = {q: getattr(plain, q).clone() for q in ("final_states", "returns", "reward_logits")}
    goal = dyn.rollout(z, plans, gamma=0.9, keep_logits=True, goal=z[0], keep_goal_dist=True)
    assert torch.equal(goal.final_states, kept["final_states"]) and torch.equal(goal.reward_logits, kept["reward_logits"])
    assert not torch.equal(goal.returns, kept["returns"])
    with pytest.raises(ValueError, match="keep_goal_dist"):
        dyn.rollout(z, plans, keep_goal_dist=True)
    for bad, match in ((dict(goal=z[0][:7]), "wide"), (dict(goal=z[:2]), "environments"), (dict(goal=z[0], goal_weight=0), "goal_weight"),
                       (dict(goal=z[0], goal_mode="last"), "goal_mode")):
        with pytest.raises(ValueError, match=match):
            dyn.rollout(z, plans, **bad)
        with pytest.raises(ValueError, match=match):
            dyn.plan(z, 4, n_plans=8, elites=2, **bad)
    # a model whose losses trained no reward head: closed without a goal, open with one; the untrained head stays out of the score
    bare = deploy.LatentDynamics(_model("s8_mlp", ["forward", "inverse"]), max_rows=64, max_horizon=8)
    with pytest.raises(ValueError, match="reward head"):
        bare.act(z, plans)
    with pytest.raises(ValueError, match="reward head"):
        bare.plan(z, 4, n_plans=8, elites=2)
    assert bare.rollout(z, plans).returns is None
    lone = bare.rollout(z, plans, gamma=0.9, goal=z, goal_weight=0.5, keep_goal_dist=True)
    assert same_bits(lone.returns.cpu().numpy(), gu.scores(lone.goal_dist.cpu().numpy(), None, 0.9, 0.5, "running", np.float32))
    free = deploy.LatentDynamics(_model("s8_mlp", ["forward", "inverse"]), max_rows=64, max_horizon=8, untrained_ok=True)
    joined = free.rollout(z, plans, gamma=0.9, goal=z, goal_weight=0.5)
    assert torch.equal(joined.returns, dyn.rollout(z, plans, gamma=0.9, goal=z, goal_weight=0.5).returns)
    with pytest.raises(ValueError, match="reward head"):
        bare.rollout(z, plans, goal=z, keep_logits=True)


# ---- 7 and 9 through the public interface ----
KW = dict(n_plans=40, iterations=3, elites=6, sharpness=8, gamma=0.9, seed=11)


def _held(plan, ref, kept=True):
    b = lambda x: x.detach().cpu().numpy().view(np.uint32) if x.dtype == torch.float32 else x.detach().cpu().numpy()  # noqa: E731
    assert np.array_equal(b(plan.best_plan), ref["best_plan"]) and np.array_equal(b(plan.best_return), ref["best_return"].view(np.uint32))
    assert np.array_equal(b(plan.weights), pu.weights_of(ref["cum"])) and np.array_equal(b(plan.shifted()), pu.shifted(ref["cum"]))
    assert torch.equal(plan.action, plan.best_plan[..., 0].long())
    if kept:
        assert np.array_equal(b(plan.plans), ref["plans"]) and np.array_equal(b(plan.returns), ref["returns"].view(np.uint32))
    else:
        assert plan.plans is None and plan.returns is None


def _restated(dyn, z, goal, horizon, kw, gkw):
    return pu.cem(lambda pl: dyn.rollout(z, pl, gamma=kw["gamma"], goal=goal, **gkw).returns.cpu().numpy(), z.shape[0], kw["n_plans"], horizon,
                  dy.N_ACTIONS, kw["iterations"], kw["elites"], kw["sharpness"], kw["seed"])


@pytest.mark.parametrize("losses", [None, ("forward", "inverse")], ids=["head", "nohead"])
def test_plan_with_a_goal_is_the_restatement_over_rollouts_scores(losses):
    from srlz import deploy
    n, horizon = 3, 7
    z, goal = dy.sine_states(n, 8), goals(n, 8)
    dyn = deploy.LatentDynamics(_model("s8_mlp", losses), max_rows=256, max_horizon=32)
    for gkw in (dict(goal_weight=0.5, goal_mode="running"), dict(goal_weight=2.0, goal_mode="final")):
        plan = dyn.plan(z, horizon, keep_population=True, goal=goal, **dict(KW, **gkw))
        assert dyn.route == "rollout" and plan.best_return.shape == (n,) and plan.returns.shape == (3, n, 40)
        kept = [t.clone() for t in (plan.best_plan, plan.best_return)]
        again = dyn.rollout(z, kept[0].unsqueeze(1), gamma=KW["gamma"], goal=goal, **gkw).returns[:, 0]
        assert torch.equal(again, kept[1])  # best_return is the score of best_plan, bit for bit
        ref = _restated(dyn, z, goal, horizon, KW, gkw)
        _held(dyn.plan(z, horizon, keep_population=True, goal=goal, **dict(KW, **gkw)), ref)
        _held(dyn.plan(torch.from_numpy(z).to(_dev()), horizon, goal=torch.from_numpy(goal).to(_dev()), **dict(KW, **gkw)), ref, kept=False)
    bare = dyn.plan(z[0], horizon, keep_population=True, goal=goal[0], **dict(KW, **gkw))
    assert bare.best_plan.shape == (horizon,) and bare.best_return.shape == () and np.array_equal(bare.best_plan.cpu().numpy(), ref["best_plan"][0])
    # a goal shared by every environment: the bits of the goal tiled
    shared = dyn.plan(z, horizon, goal=goal[1], **KW).best_return.clone()
    assert torch.equal(shared, dyn.plan(z, horizon, goal=np.tile(goal[1], (n, 1)), **KW).best_return)


def _split_model():
    if "split" not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        torch.manual_seed(1)
        losses = ["autoencoder", "forward", "reward"]
        m = modules.SRLModulesSplit(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=losses,
                                    split_dimensions=OrderedDict(zip(losses, (4, 2, 2))))
        _MODELS["split"] = m.to(_dev())
    return _MODELS["split"]


def test_route_model_for_a_split_model_and_beyond_max_rows(golden):
    from srlz import deploy
    sp = golden[1]["cases"]["s8_mlp"]
    z, plans = gu.case_inputs("s8_mlp")
    goal = goals(dy.N_ENVS, 8)
    gkw = dict(goal=goal, goal_weight=gu.WEIGHT)
    # a split model: scored by goal_scores over the model's own step-by-step trajectory and reward head
    split = deploy.LatentDynamics(_split_model())
    out = split.rollout(z, plans, gamma=gu.GAMMA, keep_trajectory=True, keep_logits=True, keep_goal_dist=True, **gkw)
    assert split.route == "model" and out.goal_dist.shape == plans.shape
    plain = split.rollout(z, plans, gamma=gu.GAMMA, keep_trajectory=True, keep_logits=True)
    assert torch.equal(out.trajectory, plain.trajectory) and torch.allclose(out.reward_logits, plain.reward_logits, rtol=0, atol=1e-5)
    ref, d = deploy.goal_scores(out.trajectory, goal, torch.softmax(out.reward_logits, dim=-1)[..., 1], gu.GAMMA, gu.WEIGHT, "running")
    assert torch.equal(out.returns, ref) and torch.equal(out.goal_dist, d)
    a = split.act(z, plans, goal=goal, goal_mode="final")
    assert np.array_equal(a.cpu().numpy(), plans[np.arange(dy.N_ENVS), split.rollout(z, plans, goal=goal, goal_mode="final").best.cpu().numpy(), 0])
    kw = dict(KW, n_plans=12, iterations=2, elites=3)
    plan = split.plan(z, 5, keep_population=True, **dict(kw, **gkw))
    assert split.route == "model"
    _held(plan, _restated(split, z, goal, 5, kw, dict(goal_weight=gu.WEIGHT)))
    # beyond max_rows: within the recorded bound of the kernel's answer on the same inputs
    small = deploy.LatentDynamics(_model("s8_mlp"), max_rows=8, max_horizon=8)   # 12 rows > 8
    roomy = deploy.LatentDynamics(_model("s8_mlp"), max_rows=16, max_horizon=8)
    for mode in gu.MODES:
        m = small.rollout(z, plans, gamma=gu.GAMMA, goal_mode=mode, keep_goal_dist=True, **gkw)
        k = roomy.rollout(z, plans, gamma=gu.GAMMA, goal_mode=mode, keep_goal_dist=True, **gkw)
        assert small.route == "model" and roomy.route == "rollout"
        e_dist = dy.rel_err(m.goal_dist.cpu().numpy()[..., None], k.goal_dist.cpu().numpy()[..., None], True)
        e_score = dy.rel_err(m.returns.cpu().numpy(), k.returns.cpu().numpy(), False)
        print("route model against the kernel, %s: goal_dist %.2e, score %.2e" % (mode, e_dist, e_score))
        assert e_dist <= dy.bound(sp["goal_dist"]) and e_score <= dy.bound(sp[mode + "_head"])
    # beyond the kernel's horizon the planner takes the host loop
    long = roomy.plan(z[:1], 33, n_plans=4, iterations=1, elites=2, keep_population=True, goal=goal[0])
    assert roomy.route == "model" and long.best_plan.shape == (1, 33)
    assert np.array_equal(long.plans[0].cpu().numpy(), pu.sample(pu.uniform_cum(1, 33, 6), 0, 0, 4))


def test_reach_is_plan_on_the_encoders_states():
    from srlz import deploy
    import models.modules as modules
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    torch.manual_seed(5)
    model = modules.SRLModules(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=["autoencoder", "forward", "inverse"]).to(_dev())
    model.eval()
    frames = du.frames_nhwc(4, 224, 224, 3)
    now, then = frames[:2], frames[2:]
    # (the references below encode frames that are on the device already: two encoder calls back to back on HOST frames would refill
    # its pinned staging buffer while the first call's upload may still wait on the stream — reach itself uploads before it encodes)
    now_d, then_d = torch.from_numpy(now).to(_dev()), torch.from_numpy(then).to(_dev())
    dyn = deploy.LatentDynamics(model, max_rows=256, max_horizon=8)
    kw = dict(n_plans=33, iterations=2, elites=4, seed=3, goal_mode="final", keep_population=True)
    fields = ("best_plan", "best_return", "action", "plans", "returns", "weights")

    def kept(plan):
        return [getattr(plan, q).clone() for q in fields]
    # four frames beyond max_batch = 2: current and goal frames go through the encoder in two calls
    small = deploy.StateEncoder(model, max_batch=2)
    got = kept(deploy.reach(small, dyn, now, then, 5, **kw))
    assert small.route == "blocks" and dyn.route == "rollout" and got[0].shape == (2, 5) and got[1].device.type == "cuda"
    s_now, s_then = small(now_d).clone(), small(then_d).clone()
    for a, b in zip(got, kept(dyn.plan(s_now, 5, goal=s_then, **kw))):
        assert torch.equal(a, b)
    # within max_batch = 4: one call of the encoder for all four
    enc = deploy.StateEncoder(model, max_batch=4)
    got = kept(deploy.reach(enc, dyn, now, then, 5, **kw))
    both = enc(torch.cat((now_d, then_d))).clone()
    print("states of four frames in one encoder call against two calls of two: max |diff| %.3e, scale %.3e"
          % ((both - torch.cat((s_now, s_then))).abs().max().item(), s_now.abs().max().item()))
    assert (both - torch.cat((s_now, s_then))).abs().max().item() <= 1e-5 * s_now.abs().max().item()
    for a, b in zip(got, kept(dyn.plan(both[:2].contiguous(), 5, goal=both[2:].contiguous(), **kw))):
        assert torch.equal(a, b)
    # one bare frame each: every axis N dropped
    one = kept(deploy.reach(small, dyn, now[1], then[1], 5, **kw))
    pair = small(torch.stack((now_d[1], then_d[1]))).clone()
    assert one[0].shape == (5,) and one[1].shape == () and one[3].shape == (2, 33, 5)
    for a, b in zip(one, kept(dyn.plan(pair[0], 5, goal=pair[1], **kw))):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="same shape"):
        deploy.reach(enc, dyn, now, then[:1], 5)
    with pytest.raises(ValueError, match="goal_frames"):
        deploy.reach(enc, dyn, now, then, 5, goal=s_then)
