"""The k-step error of the dynamics on the GPU: srlz_horizon_rows and srlz_horizon_sums through the C ABI (a sentinel tail behind
every output), and LatentDynamics.horizon_error / evaluation.predict_forward on top of them.

Shapes, the smallest at which the tile can go wrong: S in {1, 31, 32, 33, 200, 512} (below, on and above the sums' 16 column groups
and the 32-k chunk; the limit), M in {1, 32, 33, 70} (one row, one tile, tile + 1, three tiles), T in {1, 7, 32}, A in {1, 6}, a reward
head of H in {1, 16, 32} and none; rows without a step, rows of every length, rows of all T steps.
What is held, and to what:
  1  for t < len, trajectory and reward_logits are srlz_rollout's bits for K = 1 plans built from the recorded actions;
  2  err against fp64 from the kernel's own fp32 trajectory, base against fp64 from the inputs: |d - d64| <= (S + 4) 2^-24 d64 (one
     rounding for the difference — twice in the square —, one for the square, at most S - 1 for the sum), every term non-negative;
     every t >= len is NaN;
  3  sum_err and sum_base against numpy's fp64 sum of the kernel's own rows within (M - 1) 2^-53 relative (M - 1 additions of
     non-negative terms, each rounded once, in any order); count and hits exactly a host recount from the kernel's own logits;
  4  against the unmodified reference's fixture (tests/golden/horizon_kats.npz) within max(1e-4, 10 x its own fp32-to-fp64 spread)
     of each quantity's scale; the predicted class equal on every (row, step) outside the recorded gap;
  5  bit properties: two runs, a row alone and among 69 others, T steps and one step, shuffled starts;
  6  every refusal's code, with nothing written;
  7  route "model" — forced on the same heads, and a split model against its own heads called from here — and the command line."""
import functools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dynamics_util as dy
import horizon_util as hu

pytestmark = pytest.mark.gpu

F_SENTINEL, I_SENTINEL = 1234.5, -77
TAIL = 64
N_REC = 110  # frames of the kernel tests' recorded sequence: 70 starts and 32 steps fit
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW_OUT = ("err", "base", "reward_logits", "trajectory")
SUM_OUT = ("count", "sum_err", "sum_base", "hits")
SUM_DTYPE = {"count": torch.int64, "sum_err": torch.float64, "sum_base": torch.float64, "hits": torch.int64}
_MODELS = {}


def _dev():
    return torch.device("cuda", 0)


def _buffer(numel, dtype=torch.float32):
    return torch.full((numel + TAIL,), I_SENTINEL if dtype == torch.int64 else F_SENTINEL, dtype=dtype, device=_dev())


def _take(buf, shape, name):
    host = buf.cpu()
    numel = host.numel() - TAIL
    fill = I_SENTINEL if host.dtype == torch.int64 else F_SENTINEL
    assert bool((host[numel:] == fill).all()), "%s: sentinel tail overwritten" % name
    return host[:numel].view(shape).numpy().copy()


def _untouched(out):
    for q, x in out.items():
        assert (x == (I_SENTINEL if x.dtype == np.int64 else F_SENTINEL)).all(), "%s written by a refused call" % q


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def layout(pattern, m, t, n=N_REC):
    """(starts int32 [m], lens int32 [m]) of a pattern; starts[r] + lens[r] <= n - 1 always."""
    r = np.arange(m)
    if pattern == "zero":
        return ((7 * r) % n).astype(np.int32), np.zeros(m, np.int32)
    if pattern == "full":
        assert m + t <= n
        return r.astype(np.int32), np.full(m, t, np.int32)
    starts = (7 * r) % (n - t - 1)  # mixed: starts out of order (and, beyond n - t - 1 rows, repeated), every length 0 .. t
    return starts.astype(np.int32), ((5 * r + 3) % (t + 1)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def problem(s, a, h):
    """Seeded heads and a recorded sequence of one head shape (host and device), made once and shared."""
    params = dy.seeded_heads(s, a, h)
    i = np.arange(N_REC)
    z, acts = dy.sine_states(N_REC, s), ((3 * i + i // 4) % a).astype(np.int32)
    labels = (i % 3 == 0).astype(np.int32)
    dev = _dev()
    return dict(params_dev=tuple(p.to(dev) for p in params), z=z, acts=acts, labels=labels, z_dev=torch.from_numpy(z).to(dev),
                acts_dev=torch.from_numpy(acts).to(dev), labels_dev=torch.from_numpy(labels).to(dev), dims=(s, a, h))


def rows(pb, starts, lens, t, head=True, want=ROW_OUT, raw=False, null=(), **over):
    """One srlz_horizon_rows call.  Returns ({name: numpy}, status); every tail checked."""
    from srlz import _cabi as C
    s, a, h = pb["dims"]
    m = len(starts)
    mm, tt = max(over.get("m", m), 1), max(t, 1)
    sizes = {"err": (mm, tt), "base": (mm, tt), "reward_logits": (mm, tt, 2), "trajectory": (mm, tt, s)}
    want = [q for q in want if head is not False or q != "reward_logits" or over.get("force_logits")]
    bufs = {q: _buffer(int(np.prod(sizes[q]))) for q in want}
    p = pb["params_dev"]
    heads = [C.ptr(x) for x in p[2:]] if head is True else [None] * 6 if head is False else [C.ptr(x) if i in head else None for i, x in enumerate(p[2:])]
    dev = _dev()
    st_dev, ln_dev = torch.from_numpy(np.asarray(starts, np.int32)).to(dev), torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    ins = OrderedDict([("states", pb["z_dev"]), ("actions", pb["acts_dev"]), ("starts", st_dev), ("len", ln_dev), ("wf", p[0]), ("bf", p[1])])
    args = [None if q in null else C.ptr(x) for q, x in ins.items()] + heads + \
           [None if q in null else C.ptr(bufs.get(q)) for q in ROW_OUT] + \
           [N_REC, over.get("m", m), t, over.get("s", s), over.get("a", a), over.get("h", h), over.get("n_rewards", 2), C.stream()]
    status = C._lib.srlz_horizon_rows(*args) if raw else C.horizon_rows(*args)
    torch.cuda.synchronize()
    return {q: _take(b, sizes[q], q) for q, b in bufs.items()}, status


def sums(pb, out, starts, lens, labels=True, raw=False, null=(), **over):
    """One srlz_horizon_sums call on the rows `out` of a rows() call.  Returns ({name: numpy}, status); every tail checked."""
    from srlz import _cabi as C
    m, t = out["err"].shape
    dev = _dev()
    ins = OrderedDict([("err", torch.from_numpy(out["err"]).to(dev)), ("base", torch.from_numpy(out["base"]).to(dev)),
                       ("reward_logits", torch.from_numpy(out["reward_logits"]).to(dev) if labels else None),
                       ("labels", pb["labels_dev"] if labels else None),
                       ("starts", torch.from_numpy(np.asarray(starts, np.int32)).to(dev)),
                       ("len", torch.from_numpy(np.asarray(lens, np.int32)).to(dev))])
    want = [q for q in SUM_OUT if labels or q != "hits"]
    bufs = {q: _buffer(max(over.get("t", t), 1), SUM_DTYPE[q]) for q in want}
    args = [None if (q in null or x is None) else C.ptr(x) for q, x in ins.items()] + [over.get("m", m), over.get("t", t)] + \
           [None if q in null else C.ptr(bufs.get(q)) for q in SUM_OUT] + [C.stream()]
    status = C._lib.srlz_horizon_sums(*args) if raw else C.horizon_sums(*args)
    torch.cuda.synchronize()
    return {q: _take(b, (max(over.get("t", t), 1),), q) for q, b in bufs.items()}, status


def rollout_of(pb, starts, lens, t, head):
    """srlz_rollout with K = 1 plans built from the recorded actions (action 0 past a row's steps) -> trajectory [M,T,S], logits [M,T,2] | None."""
    from srlz import ops
    m = len(starts)
    plans = np.zeros((m, 1, t), np.int32)
    for r in range(m):
        plans[r, 0, :lens[r]] = pb["acts"][starts[r]:starts[r] + lens[r]]
    dev = _dev()
    p = pb["params_dev"]
    z = pb["z_dev"][torch.from_numpy(np.asarray(starts, np.int64)).to(dev)].contiguous()
    traj = torch.empty((m, 1, t, pb["dims"][0]), dtype=torch.float32, device=dev)
    logits = torch.empty((m, 1, t, 2), dtype=torch.float32, device=dev) if head else None
    ops.rollout(z, torch.from_numpy(plans).to(dev), p[0], p[1], reward=p[2:] if head else None, trajectory=traj, reward_logits=logits)
    torch.cuda.synchronize()
    return traj.cpu().numpy()[:, 0], logits.cpu().numpy()[:, 0] if head else None


#          S    A   H     M   T   lens     (H = None: no reward head)
SHAPES = [(1, 1, 1, 1, 1, "full"),
          (1, 6, None, 33, 7, "mixed"),      # tile + 1 rows, the narrowest state
          (31, 6, 16, 32, 7, "mixed"),       # exactly one tile
          (32, 6, 32, 33, 7, "full"),
          (33, 1, 16, 70, 7, "mixed"),       # three tiles, the last one short
          (33, 6, None, 1, 32, "full"),
          (200, 6, 16, 70, 7, "mixed"),
          (200, 6, None, 33, 32, "mixed"),
          (200, 6, 1, 32, 32, "zero"),       # no row has a step
          (512, 6, 32, 33, 7, "mixed"),      # both limits
          (512, 6, None, 70, 1, "mixed")]
IDS = ["S%d_A%d_H%s_M%d_T%d_%s" % v for v in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_and_sums_through_the_c_abi(shape):
    s, a, h, m, t, pattern = shape
    head = h is not None
    pb = problem(s, a, h or 16)
    starts, lens = layout(pattern, m, t)
    assert (starts + lens <= N_REC - 1).all() and (lens <= t).all()
    out, status = rows(pb, starts, lens, t, head=head)
    assert status == 0
    mask = hu.valid_mask(lens, t)
    # 1: the tile's own bits
    traj, logits = rollout_of(pb, starts, lens, t, head)
    assert same_bits(out["trajectory"][mask], traj[mask])
    if head:
        assert same_bits(out["reward_logits"][mask], logits[mask])
    # 2: the reductions against fp64, and NaN where a row has no step
    assert np.isnan(out["err"][~mask]).all() and np.isnan(out["base"][~mask]).all()
    e64, b64 = hu.rows_from_trajectory(out["trajectory"], pb["z"], starts, lens, np.float64)
    bound = (s + 4) * 2.0 ** -24
    for got, ref, q in ((out["err"], e64, "err"), (out["base"], b64, "base")):
        assert not np.isnan(got[mask]).any() and (got[mask] >= 0).all(), q
        if mask.any():
            rel = np.abs(got[mask].astype(np.float64) - ref[mask]) / np.maximum(ref[mask], 1e-300)
            print("%s: max relative error against fp64 %.3e, bound %.3e" % (q, rel.max(), bound))
            assert (np.abs(got[mask].astype(np.float64) - ref[mask]) <= bound * ref[mask]).all(), q
    # 3: the sums
    tot, status = sums(pb, out, starts, lens, labels=head)
    assert status == 0
    count, se, sb, hits = hu.totals(out["err"], out["base"], lens, out["reward_logits"] if head else None, pb["labels"], starts)
    assert np.array_equal(tot["count"], count) and count.tolist() == [int((lens > step).sum()) for step in range(t)]
    if head:
        assert np.array_equal(tot["hits"], hits)
    for got, q in ((tot["sum_err"], "err"), (tot["sum_base"], "base")):
        ref = np.where(mask, out[q].astype(np.float64), 0.0).sum(axis=0)  # numpy's fp64 sum of the kernel's own rows
        assert (np.abs(got - ref) <= max(m - 1, 0) * 2.0 ** -53 * ref).all(), q
    if pattern == "zero":
        assert (tot["count"] == 0).all() and (tot["sum_err"] == 0).all() and (tot["sum_base"] == 0).all()


def test_an_action_out_of_range_turns_its_row_nan_from_that_step_on():
    pb = problem(33, 6, 16)
    t = 7
    starts, lens = layout("full", 33, t)
    acts = pb["acts"].copy()
    acts[5 + 2] = 6  # row 5 meets it at step 2, row 7 at step 0, row 8 never
    moved = dict(pb, acts=acts, acts_dev=torch.from_numpy(acts).to(_dev()))
    ok, _ = rows(pb, starts, lens, t)
    out, _ = rows(moved, starts, lens, t)
    assert np.isnan(out["err"][5, 2:]).all() and same_bits(out["err"][5, :2], ok["err"][5, :2]) and np.isnan(out["reward_logits"][5, 2:]).all()
    assert np.isnan(out["err"][7]).all() and np.isnan(out["err"][1, 6:]).all() and not np.isnan(out["err"][1, :6]).any()
    assert same_bits(out["base"], ok["base"])  # (the start state's distance never passes through the head)
    untouched = [r for r in range(33) if not (r <= 7 <= r + t - 1)]
    assert same_bits(out["err"][untouched], ok["err"][untouched]) and same_bits(out["trajectory"][untouched], ok["trajectory"][untouched])
    # a NaN inside a valid step propagates into its horizon's sum; the count and the other horizons' sums stand
    tot, _ = sums(moved, out, starts, lens)
    assert np.isnan(tot["sum_err"]).all() and not np.isnan(tot["sum_base"]).any() and (tot["count"] == 33).all()
    count, _, _, hits = hu.totals(out["err"], out["base"], lens, out["reward_logits"], pb["labels"], starts)
    assert np.array_equal(tot["hits"], hits)  # (NaN logits answer class 0, as torch's argmax does)


def test_bit_properties():
    pb = problem(200, 6, 16)
    m, t = 70, 7
    starts, lens = layout("mixed", m, t)
    mask = hu.valid_mask(lens, t)
    out, _ = rows(pb, starts, lens, t)
    again, _ = rows(pb, starts, lens, t)
    for q in ROW_OUT:  # two runs
        assert np.array_equal(out[q].view(np.uint32), again[q].view(np.uint32)), q
    tot, _ = sums(pb, out, starts, lens)
    tot2, _ = sums(pb, out, starts, lens)
    for q in SUM_OUT:
        assert np.array_equal(tot[q].view(np.uint64), tot2[q].view(np.uint64)), q
    for r in (0, 33, 69):  # a start alone: the rows it has among 69 others
        alone, _ = rows(pb, starts[r:r + 1], lens[r:r + 1], t)
        for q in ROW_OUT:
            assert np.array_equal(alone[q][0].view(np.uint32), out[q][r].view(np.uint32)), (q, r)
    one, _ = rows(pb, starts, np.minimum(lens, 1), 1)  # T steps: the first step of a T = 1 call
    first = mask[:, 0]
    for q in ROW_OUT:
        assert np.array_equal(one[q][first, 0].view(np.uint32), out[q][first, 0].view(np.uint32)), q
    assert np.isnan(one["err"][~first, 0]).all()
    perm = np.random.RandomState(0).permutation(m)  # shuffled starts: permuted rows
    moved, _ = rows(pb, starts[perm], lens[perm], t)
    for q in ROW_OUT:
        assert np.array_equal(moved[q].view(np.uint32), out[q][perm].view(np.uint32)), q
    tot3, _ = sums(pb, moved, starts[perm], lens[perm])
    assert np.array_equal(tot3["count"], tot["count"]) and np.array_equal(tot3["hits"], tot["hits"])


def test_every_refusal_returns_its_code_and_writes_nothing():
    from srlz import _cabi as C
    BAD, NULL = -1, -4
    pb = problem(33, 6, 16)
    t = 7
    starts, lens = layout("mixed", 33, t)

    def refused(code, **kw):
        out, status = rows(pb, starts, lens, kw.pop("t", t), raw=True, **kw)
        assert status == code, (kw, status)
        assert C.error_text(), kw
        _untouched(out)
    for q in ("states", "actions", "starts", "len", "wf", "bf", "err", "base"):
        refused(NULL, null=(q,))
    refused(BAD, m=0)
    refused(BAD, m=-3)
    for bad_t in (0, 33, -1):
        refused(BAD, t=bad_t)
    for part in ((0,), (0, 1, 2, 3, 4), (5,), (1, 3)):
        refused(BAD, head=part)
    refused(BAD, s=513)
    refused(BAD, s=0)
    refused(BAD, a=0)
    refused(BAD, a=65537)
    refused(BAD, h=33)
    refused(BAD, h=0)
    refused(BAD, n_rewards=3)
    refused(BAD, head=False, force_logits=True)  # logits without a head
    # without a head H and n_rewards are not looked at; trajectory and logits are optional
    out, status = rows(pb, starts, lens, t, head=False, raw=True, h=77, n_rewards=5, want=("err", "base"))
    assert status == 0 and not np.isnan(out["err"][hu.valid_mask(lens, t)]).any()
    good, _ = rows(pb, starts, lens, t)

    def refused_sums(code, **kw):
        tot, status = sums(pb, good, starts, lens, raw=True, **kw)
        assert status == code, (kw, status)
        assert C.error_text(), kw
        _untouched(tot)
    for q in ("err", "base", "starts", "len", "count", "sum_err", "sum_base"):
        refused_sums(NULL, null=(q,))
    for q in ("reward_logits", "labels", "hits"):  # the three come together
        refused_sums(BAD, null=(q,))
    refused_sums(BAD, m=0)
    for bad_t in (0, 33):
        refused_sums(BAD, t=bad_t)
    tot, status = sums(pb, good, starts, lens, labels=False, raw=True)
    assert status == 0 and "hits" not in tot


# ---- through LatentDynamics ----
def _model(name):
    if name not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        m = dy.build_case(name, modules).to(_dev())
        m.eval()
        _MODELS[name] = m
    return _MODELS[name]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "horizon_kats.npz")), json.load(open(os.path.join(GOLDEN, "horizon_spread.json")))


def _against_fixture(h, kats, sp, name, lens, labels, starts):
    """A HorizonError with its rows kept against the fixture of `name`, to the bar: max(1e-4, 10 x the recorded spread)."""
    t = hu.HORIZON
    mask = hu.valid_mask(lens, t)
    got = {"err": h.err.cpu().numpy(), "base": h.base.cpu().numpy(), "logits": h.logits.cpu().numpy()}
    for q in hu.ROW_QUANTITIES:
        e = hu.step_rel_err(got[q], kats["%s/%s64" % (name, q)], mask)
        print("%s %s: %.2e of scale (bound %.2e)" % (name, q, e, dy.bound(sp[q])))
        assert e <= dy.bound(sp[q]), (name, q)
    assert np.isnan(got["err"][~mask]).all() and np.isnan(got["base"][~mask]).all()
    assert np.array_equal(h.count, kats[name + "/count"])
    for q, v in (("sum_err", h.sum_err), ("sum_base", h.sum_base)):
        e = hu.vec_rel_err(v, kats["%s/%s" % (name, q)])
        print("%s %s: %.2e of scale (bound %.2e)" % (name, q, e, dy.bound(sp[q])))
        assert e <= dy.bound(sp[q]), (name, q)
    s = dy.CASES[name]["state_dim"]
    assert np.allclose(h.mse, h.sum_err / (h.count * s), rtol=1e-15) and np.allclose(h.ratio, h.sum_err / h.sum_base, rtol=1e-15)
    # the reported hits are the recount of the call's own logits; the classes are the fixture's wherever its gap decides
    assert np.array_equal(h.hits, hu.totals(got["err"], got["base"], lens, got["logits"], labels, starts)[3])
    if name in hu.HIT_CASES:
        dec = kats[name + "/decided"]
        assert np.array_equal(hu.classes_of(got["logits"])[dec], hu.classes_of(kats[name + "/logits64"])[dec]), name
        if dec[mask].all():
            assert np.array_equal(h.hits, kats[name + "/hits"]), name
    assert np.allclose(h.reward_accuracy, h.hits / h.count.astype(np.float64), rtol=1e-15)


@pytest.mark.parametrize("name", list(dy.CASES))
def test_horizon_error_against_the_reference_fixture(name, golden):
    from srlz import deploy
    kats, spread = golden
    s = dy.CASES[name]["state_dim"]
    states, actions, rewards, es = hu.recording(s)
    lens, starts, labels = hu.valid_steps(es, hu.HORIZON), np.arange(hu.N_FRAMES), hu.labels_of(rewards)
    dyn = deploy.LatentDynamics(_model(name), max_rows=16, max_horizon=8)  # (40 rows: max_rows does not apply to this call)
    h = dyn.horizon_error(states, actions, es, hu.HORIZON, rewards=rewards, starts=starts, keep_rows=True)
    assert dyn.route == "rollout" and h.err.shape == (hu.N_FRAMES, hu.HORIZON) and h.logits.shape == (hu.N_FRAMES, hu.HORIZON, 2)
    _against_fixture(h, kats, spread["cases"][name], name, lens, labels, starts)
    assert np.array_equal(h.majority_accuracy, deploy.majority_accuracy(labels, starts, lens, hu.HORIZON))
    # the default starts — every frame with a step —, device inputs, no rows kept: the same totals, bit for bit
    d = dyn.horizon_error(torch.from_numpy(states).to(_dev()), torch.from_numpy(actions).to(_dev()), es, hu.HORIZON, rewards=rewards)
    assert d.err is None and d.base is None and d.logits is None
    assert np.array_equal(d.count, h.count) and np.array_equal(d.hits, h.hits)
    keep = lens >= 1
    e, b = h.err.cpu().numpy()[keep], h.base.cpu().numpy()[keep]
    mask = hu.valid_mask(lens[keep], hu.HORIZON)
    for got, rows_ in ((d.sum_err, e), (d.sum_base, b)):
        ref = np.where(mask, rows_.astype(np.float64), 0.0).sum(axis=0)
        assert (np.abs(got - ref) <= (keep.sum() - 1) * 2.0 ** -53 * ref).all()
    # without rewards: no reward fields, the same errors
    bare = dyn.horizon_error(states, actions, es, hu.HORIZON, starts=starts)
    assert bare.reward_accuracy is None and bare.majority_accuracy is None and bare.hits is None
    assert np.array_equal(bare.sum_err, h.sum_err) and np.array_equal(bare.sum_base, h.sum_base)


def test_gating_and_value_errors_through_the_public_call():
    import copy
    from srlz import deploy
    states, actions, rewards, es = hu.recording(8)
    dyn = deploy.LatentDynamics(_model("s8_mlp"))
    with pytest.raises(ValueError, match="inside every valid step"):
        dyn.horizon_error(states, np.where(np.arange(hu.N_FRAMES) == 5, 6, actions), es, hu.HORIZON)
    with pytest.raises(ValueError, match="two classes"):
        dyn.horizon_error(states, actions, es, hu.HORIZON, rewards=rewards + 2)
    with pytest.raises(ValueError, match="one entry per frame"):
        dyn.horizon_error(states, actions, es, hu.HORIZON, rewards=rewards[:-1])
    with pytest.raises(ValueError, match="one entry per frame"):
        dyn.horizon_error(states[:-1], actions, es, hu.HORIZON)
    with pytest.raises(ValueError, match="recorded sequence"):
        dyn.horizon_error(states[0], actions, es, hu.HORIZON)
    with pytest.raises(ValueError, match="horizon"):
        dyn.horizon_error(states, actions, es, 0)
    # a forward head the losses never trained is refused; a reward head they never trained is left out
    m = copy.deepcopy(_model("s8_mlp"))
    m.losses = ["inverse", "reward"]
    with pytest.raises(ValueError, match="forward head"):
        deploy.LatentDynamics(m).horizon_error(states, actions, es, hu.HORIZON)
    assert deploy.LatentDynamics(m, untrained_ok=True).horizon_error(states, actions, es, hu.HORIZON).count[0] > 0
    m.losses = ["forward", "inverse"]
    out = deploy.LatentDynamics(m).horizon_error(states, actions, es, hu.HORIZON, rewards=rewards)
    assert out.reward_accuracy is None and out.majority_accuracy is None and out.count[0] > 0


def _split_model():
    if "split" not in _MODELS:
        import models.modules as modules
        import preprocessing.preprocess as pre
        pre.N_CHANNELS = 3
        torch.manual_seed(1)
        losses = ["autoencoder", "forward", "reward"]
        m = modules.SRLModulesSplit(state_dim=8, action_dim=6, cuda=False, model_type="custom_cnn", losses=losses,
                                    split_dimensions=OrderedDict(zip(losses, (4, 2, 2))))
        m.eval()
        _MODELS["split"] = m.to(_dev())
    return _MODELS["split"]


def test_route_model(golden):
    from srlz import deploy
    kats, spread = golden
    sp = spread["cases"]["s8_mlp"]
    states, actions, rewards, es = hu.recording(8)
    lens, starts, labels = hu.valid_steps(es, hu.HORIZON), np.arange(hu.N_FRAMES), hu.labels_of(rewards)
    mask = hu.valid_mask(lens, hu.HORIZON)
    kw = dict(rewards=rewards, starts=starts, keep_rows=True)
    # forced on the heads the kernel runs: the fixture's bar against the fixture, and against the kernel's answer
    forced = deploy.LatentDynamics(_model("s8_mlp"), route="model")
    m = forced.horizon_error(states, actions, es, hu.HORIZON, **kw)
    assert forced.route == "model"
    _against_fixture(m, kats, sp, "s8_mlp", lens, labels, starts)
    kernel = deploy.LatentDynamics(_model("s8_mlp"))
    k = kernel.horizon_error(states, actions, es, hu.HORIZON, **kw)
    assert kernel.route == "rollout"
    for q in hu.ROW_QUANTITIES:
        e = hu.step_rel_err(getattr(m, q).cpu().numpy(), getattr(k, q).cpu().numpy(), mask)
        print("route model against the kernel, %s: %.2e" % (q, e))
        assert e <= dy.bound(sp[q]), q
    assert np.array_equal(m.count, k.count)
    assert hu.vec_rel_err(m.sum_err, k.sum_err) <= dy.bound(sp["sum_err"]) and hu.vec_rel_err(m.sum_base, k.sum_base) <= dy.bound(sp["sum_base"])
    # beyond the kernel's horizon, and beyond max_horizon: the same call on the host loop
    assert kernel.horizon_error(states, actions, es, 33).count.shape == (33,) and kernel.route == "model"
    assert deploy.LatentDynamics(_model("s8_mlp"), max_horizon=4).horizon_error(states, actions, es, 5).count[4] > 0
    # a split model: its heads see masked states — against the model's own methods called step by step from here
    split_model = _split_model()
    split = deploy.LatentDynamics(split_model)
    got = split.horizon_error(states, actions, es, hu.HORIZON, **kw)
    assert split.route == "model" and deploy.horizon_route_for(split_model) == "model"
    x = torch.from_numpy(states).to(_dev())
    traj, logits = [], []
    with torch.no_grad():
        cur = x
        for step in range(hu.HORIZON):
            a = torch.from_numpy(np.where(lens > step, actions[np.minimum(starts + step, hu.N_FRAMES - 1)], 0)).long().to(_dev())
            nxt = split_model.forwardModel(cur, a)
            logits.append(split_model.rewardModel(cur, nxt))
            traj.append(nxt)
            cur = nxt
    traj, logits = torch.stack(traj, 1).cpu().numpy(), torch.stack(logits, 1).cpu().numpy()
    e64, b64 = hu.rows_from_trajectory(traj, states, starts, lens, np.float64)
    assert hu.step_rel_err(got.err.cpu().numpy(), e64, mask) <= 1e-4 and hu.step_rel_err(got.base.cpu().numpy(), b64, mask) <= 1e-4
    assert np.isnan(got.err.cpu().numpy()[~mask]).all()
    count, se, sb, hits = hu.totals(got.err.cpu().numpy(), got.base.cpu().numpy(), lens, logits, labels, starts)
    assert np.array_equal(got.count, count) and np.array_equal(got.hits, hits)
    assert hu.vec_rel_err(got.sum_err, se) <= 1e-12 and hu.vec_rel_err(got.sum_base, sb) <= 1e-12


def test_command_line_on_a_tiny_dataset(tmp_path, monkeypatch, capsys):
    import dataset_util
    import models.modules as modules
    import preprocessing.preprocess as pre
    from evaluation import predict_forward as pf
    pre.N_CHANNELS = 3
    root = str(tmp_path)
    name, _, actions, rewards, starts = dataset_util.make_dataset(root, name="tiny_horizon", n_episodes=3, ep_len=5)
    n = len(actions)
    log = os.path.join(root, "logs", name, "run")
    os.makedirs(log)
    with open(os.path.join(log, "exp_config.json"), "w") as f:
        json.dump(OrderedDict([("data-folder", name), ("state-dim", 8), ("losses", ["forward", "inverse", "reward"]), ("n_actions", 6),
                               ("model-type", "custom_cnn"), ("multi-view", False), ("inverse-model-type", "mlp")]), f)
    torch.save(OrderedDict((k, v.cpu()) for k, v in dy.build_case("s8_mlp", modules).state_dict().items()), os.path.join(log, "srl_model.pth"))
    states = dy.sine_states(n, 8)
    np.savez(os.path.join(log, "states_rewards.npz"), states=states, rewards=rewards)
    monkeypatch.chdir(root)
    out = pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "6"])
    text = capsys.readouterr().out
    assert tuple(sorted(out)) == tuple(sorted(pf.KEYS)) and out["horizon"] == 6
    assert out["count"] == [12, 9, 6, 3, 0, 0]  # three episodes of five frames
    assert out["mse"][4] is None and out["ratio"][5] is None and all(v is not None and v > 0 for v in out["mse"][:4])
    assert all(0 <= v <= 1 for v in out["reward_accuracy"][:4]) and all(0.5 <= v <= 1 for v in out["majority_accuracy"][:4])
    assert json.load(open(os.path.join(log, pf.OUTPUT))) == out
    assert text.count("\nt+") == 6 and "route rollout" in text
    # the same numbers as the public call on the same recording
    from srlz import deploy
    h = deploy.LatentDynamics(_model("s8_mlp")).horizon_error(states, actions, starts, 6, rewards=rewards)
    assert h.count.tolist() == out["count"] and [float(v) for v in h.mse[:4]] == out["mse"][:4]
    # fewer frames, another data folder argument, another input file
    np.savez(os.path.join(root, "other.npz"), states=states[:7])
    short = pf.main(["--log-folder", os.path.join("logs", name, "run") + "/", "--data-folder", "data/" + name, "-i", "other.npz",
                     "--horizon", "2", "--training-set-size", "100"])
    assert short["count"] == [5, 3]
    assert pf.main(["--log-folder", os.path.join("logs", name, "run"), "--horizon", "2", "--training-set-size", "6"])["count"] == [4, 3]
