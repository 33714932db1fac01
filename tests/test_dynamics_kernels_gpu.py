"""csrc/rollout.hip on the GPU through the C ABI, against the fp64 restatement of dynamics_util (torch-CPU double).

Shapes: the smallest at which the kernel can go wrong.  S in {1, 2, 3, 31, 32, 33, 200, 512 = the limit} crosses the k-chunk of 16, the
column block of 32 and puts 1, 2, 7 and 16 blocks on the four waves; A in {1, 6, 37}; R = N * K in {1, 31, 32, 33, 257} sits below, on
and above the 32-row tile of a workgroup (srlz_rollout_tile) and spans nine of them; T in {1, 2, 7}; H in {1, 16, 32 = the limit}.
With and without the reward head, and with every optional output absent.  A sentinel tail behind every output.
Bound: 1e-4 of each step's scale (trajectory and logits per step, returns and final states as a whole) — the project's parity bar;
for the expanding recurrence max(1e-4, 10 x the spread of the fp32 torch-CPU composition against fp64 on the same inputs), computed
here and printed.  The measured maxima are printed (DESIGN.md 3.15 quotes them)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dynamics_util as dy

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
TAIL = 64
ALL = ("final", "returns", "trajectory", "reward_logits")


def _dev():
    return torch.device("cuda", 0)


def _buffer(numel):
    return torch.full((numel + TAIL,), SENTINEL, dtype=torch.float32, device=_dev())


def launch(params_dev, z_dev, pl_dev, n, k, t, s, a, h, gamma=1.0, reward=True, want=ALL, raw=False):
    """One srlz_rollout call.  Returns ({name: numpy array}, status); every buffer's sentinel tail is checked here."""
    from srlz import _cabi as C
    sizes = {"final": (n, k, s), "returns": (n, k), "trajectory": (n, k, t, s), "reward_logits": (n, k, t, 2)}
    bufs = {q: _buffer(int(np.prod(sizes[q]))) for q in want}
    head = [C.ptr(p) for p in params_dev[2:]] if reward else [None] * 6
    stride = k * t if pl_dev.dim() == 3 else 0
    args = [C.ptr(z_dev), C.ptr(pl_dev), stride, C.ptr(params_dev[0]), C.ptr(params_dev[1])] + head + \
           [C.ptr(bufs.get(q)) for q in ALL] + [n, k, t, s, a, h, 2, float(gamma), C.stream()]
    status = C._lib.srlz_rollout(*args) if raw else C.rollout(*args)
    torch.cuda.synchronize()
    out = {}
    for q, b in bufs.items():
        host = b.cpu()
        numel = host.numel() - TAIL
        assert bool((host[numel:] == SENTINEL).all()), "%s: sentinel tail overwritten" % q
        out[q] = host[:numel].view(sizes[q]).numpy().copy()
    return out, status


@functools.lru_cache(maxsize=None)
def problem(s, a, h, n, k, t, seed=0, scale=1.0):
    """Heads, inputs (host and device) and the fp64 reference of one shape, made once and shared."""
    params = dy.seeded_heads(s, a, h, seed=seed, scale=scale)
    z, pl = dy.sine_states(n, s), dy.plans(n, k, t, a)
    ref = dy.restate(params, z, pl, gamma=0.9)
    dev = _dev()
    return dict(params=params, z=z, pl=pl, ref=ref, params_dev=tuple(p.to(dev) for p in params), z_dev=torch.from_numpy(z).to(dev),
                pl_dev=torch.from_numpy(pl).to(dev), dims=(n, k, t, s, a, h))


def run(pb, **kw):
    n, k, t, s, a, h = pb["dims"]
    kw.setdefault("gamma", 0.9)
    return launch(pb["params_dev"], kw.pop("z_dev", pb["z_dev"]), kw.pop("pl_dev", pb["pl_dev"]), kw.pop("n", n), kw.pop("k", k),
                  kw.pop("t", t), s, a, h, **kw)[0]


def errors(got, ref):
    return {q: dy.rel_err(got[q], ref[q], q in ("trajectory", "reward_logits")) for q in got}


#          S    A   H   N   K   T
SHAPES = [(1, 1, 1, 1, 1, 1),
          (2, 6, 16, 1, 31, 2),
          (3, 6, 16, 3, 4, 7),
          (31, 37, 16, 1, 32, 2),
          (32, 6, 1, 3, 11, 7),      # R = 33
          (33, 1, 16, 1, 33, 1),
          (200, 6, 16, 1, 257, 2),   # nine tiles, the last with one row
          (200, 37, 32, 3, 4, 7),
          (512, 6, 16, 1, 33, 7),    # the S limit: four column blocks a wave
          (512, 37, 32, 2, 16, 2)]   # both limits


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "S%d_A%d_H%d_N%d_K%d_T%d" % v)
def test_rollout_matches_fp64(shape):
    s, a, h, n, k, t = shape
    pb = problem(s, a, h, n, k, t)
    got = run(pb)
    err = errors(got, pb["ref"])
    print("rollout S=%d A=%d H=%d R=%d T=%d: rel err %s" % (s, a, h, n * k, t, {q: "%.2e" % e for q, e in err.items()}))
    for q, e in err.items():
        assert e <= dy.FLOOR, (q, e)


@pytest.mark.parametrize("shape", [(3, 6, 16, 3, 4, 7), (200, 6, 16, 1, 33, 2), (33, 37, 1, 2, 17, 7)],
                         ids=lambda v: "S%d_A%d_H%d_N%d_K%d_T%d" % v)
def test_every_optional_output_may_be_absent_and_the_reward_head_too(shape):
    s, a, h, n, k, t = shape
    pb = problem(s, a, h, n, k, t)
    full = run(pb)
    for want in (("final",), ("final", "returns"), ("final", "trajectory"), ("final", "reward_logits"), ("final", "returns", "reward_logits")):
        got = run(pb, want=want)
        for q in want:
            assert np.array_equal(got[q], full[q]), (want, q)
    # no reward head: the same states, bit for bit, and nothing else is written
    for want in (("final",), ("final", "trajectory")):
        got = run(pb, want=want, reward=False)
        for q in want:
            assert np.array_equal(got[q], full[q]), (want, q)
        err = errors(got, pb["ref"])
        assert max(err.values()) <= dy.FLOOR, err


def test_expanding_recurrence_within_ten_times_the_fp32_spread():
    s, a, h, n, k, t = 200, 6, 16, 3, 4, 7
    pb = problem(s, a, h, n, k, t, seed=1, scale=20.0)
    spread = dy.spread(pb["params"], pb["z"], pb["pl"], gamma=0.9)
    got = run(pb)
    err = errors(got, pb["ref"])
    top = float(np.abs(pb["ref"]["trajectory"][:, :, -1]).max())
    print("expanding rollout: scale of the last step %.3g; fp32 torch-CPU spread %s; kernel rel err %s"
          % (top, {q: "%.2e" % v for q, v in spread.items()}, {q: "%.2e" % e for q, e in err.items()}))
    assert top > 1e5  # the recurrence does expand
    for q in dy.QUANTITIES:
        assert err[q] <= dy.bound(spread[q]), (q, err[q], spread[q])
    assert err["final"] <= dy.bound(spread["trajectory"])


def test_t_steps_leave_the_bits_of_t_calls_of_one_step():
    s, a, h, n, k, t = 200, 6, 16, 3, 13, 7  # R = 39: two tiles
    pb = problem(s, a, h, n, k, t)
    full = run(pb)
    cur = pb["z_dev"].view(n, 1, s).expand(n, k, s).contiguous().view(n * k, s)  # one row per (n, k) from here on
    for step in range(t):
        pl = pb["pl_dev"][:, :, step].contiguous().view(n * k, 1, 1)
        got = run(pb, z_dev=cur, pl_dev=pl, n=n * k, k=1, t=1)
        assert np.array_equal(got["trajectory"].reshape(n, k, s), full["trajectory"][:, :, step]), step
        assert np.array_equal(got["reward_logits"].reshape(n, k, 2), full["reward_logits"][:, :, step]), step
        assert np.array_equal(got["final"], got["trajectory"].reshape(n * k, 1, s))
        cur = torch.from_numpy(got["final"].reshape(n * k, s)).to(_dev())
    assert np.array_equal(cur.cpu().numpy().reshape(n, k, s), full["final"])


def test_a_row_does_not_depend_on_its_neighbours_or_its_place():
    s, a, h, n, k, t = 33, 6, 16, 2, 20, 7  # R = 40
    pb = problem(s, a, h, n, k, t)
    full = run(pb)
    pick = [17, 2, 9]
    got = run(pb, z_dev=pb["z_dev"][1:2].contiguous(), pl_dev=pb["pl_dev"][1:2, pick].contiguous(), n=1, k=3)
    for q in ALL:
        assert np.array_equal(got[q][0], full[q][1, pick]), q
    alone = run(pb, z_dev=pb["z_dev"][1:2].contiguous(), pl_dev=pb["pl_dev"][1:2, 19:20].contiguous(), n=1, k=1)
    for q in ALL:
        assert np.array_equal(alone[q][0, 0], full[q][1, 19]), q


def test_shared_plans_give_the_bits_of_tiled_plans_and_two_runs_agree():
    s, a, h, n, k, t = 31, 37, 16, 3, 11, 7
    pb = problem(s, a, h, n, k, t)
    shared = pb["pl_dev"][1].contiguous()            # [K,T]
    tiled = shared.unsqueeze(0).repeat(n, 1, 1).contiguous()
    one, two, again = run(pb, pl_dev=shared), run(pb, pl_dev=tiled), run(pb, pl_dev=shared)
    ref = dy.restate(pb["params"], pb["z"], pb["pl"][1], gamma=0.9)
    for q in ALL:
        assert np.array_equal(one[q], two[q]), q
        assert np.array_equal(one[q], again[q]), q
    assert max(errors(one, ref).values()) <= dy.FLOOR


@pytest.mark.parametrize("bad_action", [6, -1, 2 ** 31 - 1])
def test_an_action_out_of_range_turns_its_row_nan_from_that_step_on(bad_action):
    s, a, h, n, k, t = 33, 6, 16, 2, 20, 7
    pb = problem(s, a, h, n, k, t)
    clean = run(pb)
    pl = pb["pl_dev"].clone()
    pl[1, 7, 2] = bad_action
    got = run(pb, pl_dev=pl)  # (launch() checks the sentinel tails)
    for q in ("trajectory", "reward_logits"):
        assert np.isnan(got[q][1, 7, 2:]).all(), q
        assert np.array_equal(got[q][1, 7, :2], clean[q][1, 7, :2]), q
    assert np.isnan(got["final"][1, 7]).all() and np.isnan(got["returns"][1, 7])
    keep = np.ones((n, k), bool)
    keep[1, 7] = False
    for q in ALL:
        assert np.array_equal(got[q][keep], clean[q][keep]), q
        assert not np.isnan(got[q][keep]).any(), q


def test_a_refused_shape_returns_bad_desc_and_writes_nothing(cabi):
    tile = cabi.rollout_tile()
    assert tile == 32
    refused = [dict(s=513), dict(h=33), dict(a=65537), dict(n_rewards=3), dict(t=0), dict(k=0), dict(stride=5)]
    for change in refused:
        s, a, h, n, k, t = change.get("s", 8), change.get("a", 6), change.get("h", 16), 2, change.get("k", 3), change.get("t", 2)
        params = [p.to(_dev()) for p in dy.seeded_heads(s, min(a, 64), h)]
        z = torch.zeros((n, s), dtype=torch.float32, device=_dev())
        pl = torch.zeros((n, max(k, 1), max(t, 1)), dtype=torch.int32, device=_dev())
        bufs = [_buffer(n * max(k, 1) * max(t, 1) * s) for _ in range(4)]
        args = [cabi.ptr(z), cabi.ptr(pl), change.get("stride", k * t)] + [cabi.ptr(p) for p in params] + [cabi.ptr(b) for b in bufs] + \
               [n, k, t, s, a, h, change.get("n_rewards", 2), 1.0, cabi.stream()]
        assert cabi._lib.srlz_rollout(*args) == -1, change  # SRLZ_ERR_BAD_DESC
        assert "rollout" in cabi.error_text()
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b == SENTINEL).all()), change
    # returns without a reward head, and half a head
    params = [p.to(_dev()) for p in dy.seeded_heads(8, 6, 16)]
    z = torch.zeros((1, 8), dtype=torch.float32, device=_dev())
    pl = torch.zeros((1, 1, 1), dtype=torch.int32, device=_dev())
    fin, ret = _buffer(8), _buffer(1)
    tail = [1, 1, 1, 8, 6, 16, 2, 1.0, cabi.stream()]
    none = [None] * 6
    assert cabi._lib.srlz_rollout(cabi.ptr(z), cabi.ptr(pl), 1, cabi.ptr(params[0]), cabi.ptr(params[1]), *none, cabi.ptr(fin),
                                  cabi.ptr(ret), None, None, *tail) == -1
    half = [cabi.ptr(p) for p in params[2:5]] + [None] * 3
    assert cabi._lib.srlz_rollout(cabi.ptr(z), cabi.ptr(pl), 1, cabi.ptr(params[0]), cabi.ptr(params[1]), *half, cabi.ptr(fin),
                                  None, None, None, *tail) == -1
    torch.cuda.synchronize()
    assert bool((fin == SENTINEL).all()) and bool((ret == SENTINEL).all())


def test_weights_changed_in_place_are_picked_up_by_the_next_call():
    s, a, h, n, k, t = 8, 6, 16, 2, 5, 3
    params = dy.seeded_heads(s, a, h, seed=7)
    dev_params = tuple(p.to(_dev()) for p in params)
    z, pl = dy.sine_states(n, s), dy.plans(n, k, t, a)
    z_dev, pl_dev = torch.from_numpy(z).to(_dev()), torch.from_numpy(pl).to(_dev())
    before, _ = launch(dev_params, z_dev, pl_dev, n, k, t, s, a, h)
    dev_params[0].mul_(0.5)           # forward_net.weight
    dev_params[7].add_(torch.tensor([0.25, -0.5], device=_dev()))  # reward_net.4.bias
    after, _ = launch(dev_params, z_dev, pl_dev, n, k, t, s, a, h)
    changed = tuple(p.cpu() for p in dev_params)
    ref = dy.restate(changed, z, pl)
    assert max(errors(after, ref).values()) <= dy.FLOOR
    assert not np.array_equal(before["final"], after["final"]) and not np.array_equal(before["returns"], after["returns"])
