"""srlz_headfit_fit / srlz_headfit_eval (csrc/headfit.hip) entry by entry against the float64 restatement of tests/headfit_util.py.

The bar is the project's gradient rule: every entry of last_grad within 1e-4 of its tensor's scale (max |reference|), the step loss
within 1e-4 relative.  The parameters after one step from zero moments are held through the gradient: Adam's first step is
lr * sign(g) wherever |g| >> eps, so a float64 trajectory would compare signs of entries that are zero up to rounding; instead the
kernel's own gradient goes through the float64 Adam and must give the kernel's moments (2e-6 of scale: a handful of float32
roundings per element) and its step (1e-5 of the step's scale: the parameter it is added to is stored in float32).  Bit guarantees
are asserted as bits.  Every buffer the kernels write has a sentinel tail.

Measured on one MI355X, worst over the 30 one-step cases: gradient entry 8.4e-06 of its tensor's scale (S = 1, H = 1, B = 259; 1.2e-06
at most elsewhere), step loss 5.2e-08 relative, step through the gradient 3.0e-06, m 6.5e-08, v 1.2e-07; three steps from non-zero
moments at t0 = 10: parameters' movement 8.0e-06, m 7.3e-08, v 1.3e-07, gradient 6.4e-07, losses 3.8e-08; eval loss within 7.9e-09
relative, no soft row in any case, every count equal."""
import ctypes

import numpy as np
import pytest
import torch

import headfit_util as hu
import reward_util as ru

pytestmark = pytest.mark.gpu

BAR = 1e-4
TAIL = 64
SENT = -12345.5
N = 40
LR = 0.005
# (1,1) the smallest head; (3,16) and (200,16) the reference head on ground truth and at the widest quoted state; (17,5) odd sizes that
# are no multiple of a quad or of the 16 lanes; (341,16) the largest S at H = 16 (chunks of 16 rows); (201,32) the largest H at its largest S
SHAPES = ((1, 1), (3, 16), (17, 5), (200, 16), (341, 16), (201, 32))


def _dev():
    return torch.device("cuda", 0)


def _batch_sizes(S, H):
    from srlz import ops
    r = ops.headfit_chunk_rows(S, H)
    return (1, 5, r, r + 1, 2 * r + 3)


CASES = [(S, H, bi) for S, H in SHAPES for bi in range(5)]


def _states(S, seed=0):
    return np.random.RandomState(seed).randn(N, S).astype(np.float32)


def _labels(seed=1):
    return np.random.RandomState(seed).randint(0, 2, N).astype(np.int64)


def _table(n_steps, B, seed):
    """int32 [n_steps, B] in [0, N - 2]; where a row has room it holds 0, N - 2 and one index twice."""
    t = np.random.RandomState(seed).randint(0, N - 1, (n_steps, B)).astype(np.int32)
    if B >= 4:
        t[:, 0], t[:, 1], t[:, 3] = 0, N - 2, t[:, 2]
    elif B == 1:
        t[:, 0] = np.where(np.arange(n_steps) % 2 == 0, N - 2, 0)
    return t


def _tailed(values, dtype):
    """A device buffer of len(values) + TAIL elements, the tail a sentinel -> (whole, view of the head)."""
    values = np.asarray(values)
    whole = torch.full((values.size + TAIL,), SENT if dtype.is_floating_point else -77, dtype=dtype, device=_dev())
    whole[:values.size] = torch.from_numpy(values).to(_dev(), dtype)
    return whole, whole[:values.size]


def _tail_ok(whole, n):
    t = whole[n:].cpu()
    return bool((t == (SENT if whole.dtype.is_floating_point else -77)).all()) and t.numel() == TAIL


class Run(object):
    """One srlz_headfit_fit call through ops.headfit_fit with sentinel tails everywhere; the results on the host."""

    def __init__(self, data, S, H, table, flat, m=None, v=None, t0=0, lr=LR, want_grad=True):
        from srlz import ops
        P, n = hu.n_params(S, H), table.shape[0]
        zeros = np.zeros(P, np.float32)
        self.bufs = {"params": _tailed(flat, torch.float32), "m": _tailed(zeros if m is None else m, torch.float32),
                     "v": _tailed(zeros if v is None else v, torch.float32), "loss": _tailed(np.zeros(1), torch.float64),
                     "counts": _tailed(np.zeros(5, np.int64), torch.int64), "step_loss": _tailed(np.full(n, SENT), torch.float64),
                     "last_grad": _tailed(np.full(P, SENT, np.float32), torch.float32)}
        b = {k: w[1] for k, w in self.bufs.items()}
        ops.headfit_fit(data, torch.from_numpy(table), H, b["params"], b["m"], b["v"], t0, lr, b["loss"], b["counts"], b["step_loss"],
                        b["last_grad"] if want_grad else None)
        torch.cuda.synchronize()
        for k, (whole, view) in self.bufs.items():
            assert _tail_ok(whole, view.numel()), "%s: sentinel tail overwritten" % k
            setattr(self, k, view.cpu().numpy().copy())
        if not want_grad:
            assert (self.last_grad == np.float32(SENT)).all()

    def bits(self, with_grad=False):
        keys = ("params", "m", "v", "loss", "counts", "step_loss") + (("last_grad",) if with_grad else ())
        return {k: getattr(self, k).view(np.uint8).copy() for k in keys}


def _data(S, states=None, labels=None):
    from srlz import ops
    return ops.reward_probe_data(_states(S) if states is None else states, _labels() if labels is None else labels)


def _tensor_errs(got, ref, S, H):
    return [ru.scale_err(g, r) for g, r in zip(hu.unflatten(np.asarray(got, np.float64), S, H), hu.unflatten(ref, S, H))]


@pytest.mark.parametrize("S,H,bi", CASES, ids=["S%d-H%d-b%d" % c for c in CASES])
def test_one_step_gradient_loss_and_update(S, H, bi):
    B = _batch_sizes(S, H)[bi]
    states, labels = _states(S, seed=S), _labels(seed=H)
    table = _table(1, B, seed=B)
    if B >= 4:
        assert 0 in table and N - 2 in table and len(set(table[0].tolist())) < B
    flat = hu.random_params(S, H, seed=7)
    run = Run(_data(S, states, labels), S, H, table, flat)
    loss, g, z = hu.loss_and_grad(flat.astype(np.float64), ru.rows(states, table[0]), labels[table[0]], H)
    errs = _tensor_errs(run.last_grad, g, S, H)
    e_loss = abs(run.step_loss[0] - loss) / abs(loss)
    # the update through the kernel's own gradient
    p64, m64, v64 = ru.adam(flat.astype(np.float64), run.last_grad.astype(np.float64), np.zeros_like(g), np.zeros_like(g), 1, LR)
    e_par = max(_tensor_errs(run.params - flat, p64 - flat, S, H))  # the step itself, not the parameter it is added to
    e_m, e_v = ru.scale_err(run.m, m64), ru.scale_err(run.v, v64)
    print("S %d H %d B %d: gradient %.2e loss %.2e step %.2e m %.2e v %.2e" % (S, H, B, max(errs), e_loss, e_par, e_m, e_v))
    assert max(errs) <= BAR, errs
    assert e_loss <= BAR
    assert e_m <= 2e-6 and e_v <= 2e-6  # a handful of float32 roundings (6e-8 each) per element, nothing else
    # the parameter is stored in float32: an entry of size 0.5 (random_params' largest) carries 3e-8 of rounding, 6e-6 of a step of LR
    assert e_par <= 1e-5
    assert abs(run.loss[0] - run.step_loss[0] * B) <= 1e-12 * B
    lo, hi, soft = ru.count_bounds(z, labels[table[0]])
    assert (lo <= run.counts).all() and (run.counts <= hi).all(), (run.counts, lo, hi)
    assert run.counts[3] + run.counts[4] == B and run.counts[1] + run.counts[2] == run.counts[0]


def test_three_steps_from_nonzero_moments_at_t0_10():
    S, H, B, t0, lr = 17, 5, 5, 10, 0.05  # (a rate at which three steps stand well clear of the float32 rounding of the parameters)
    states, labels = _states(S, seed=3), _labels(seed=4)
    table = _table(3, B, seed=9)
    rs = np.random.RandomState(5)
    flat, P = hu.random_params(S, H, seed=8), hu.n_params(S, H)
    m0, v0 = (0.01 * rs.randn(P)).astype(np.float32), rs.uniform(1e-3, 1e-2, P).astype(np.float32)  # v well above g^2 rounding: smooth steps
    run = Run(_data(S, states, labels), S, H, table, flat, m0, v0, t0=t0, lr=lr)
    p64, m64, v64, ph, grads = hu.fit(flat.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), t0, states, labels, table, lr, H)
    errs = {"params": max(_tensor_errs(run.params - flat, p64 - flat, S, H)), "m": ru.scale_err(run.m, m64), "v": ru.scale_err(run.v, v64),
            "grad": max(_tensor_errs(run.last_grad, grads[-1], S, H)), "loss": ru.scale_err(run.step_loss, ph.step_loss)}
    print("three steps at t0 = 10: %s" % errs)
    assert max(errs.values()) <= BAR, errs
    assert abs(run.loss[0] - ph.running_loss) <= BAR * ph.running_loss and np.array_equal(run.counts, ph.counts())


@pytest.mark.parametrize("S,H,B", [(17, 5, 5), (3, 16, 259), (200, 16, 49), (1, 1, 1)])
def test_bits_two_calls_and_seven_steps_in_one_call_or_seven(S, H, B):
    states, labels = _states(S, seed=11), _labels(seed=12)
    data = _data(S, states, labels)
    table = _table(7, B, seed=13)
    rs = np.random.RandomState(6)
    flat, P = hu.random_params(S, H, seed=14), hu.n_params(S, H)
    m0, v0, t0 = (0.01 * rs.randn(P)).astype(np.float32), rs.uniform(1e-4, 1e-3, P).astype(np.float32), 3
    one = Run(data, S, H, table, flat, m0, v0, t0=t0)
    two = Run(data, S, H, table, flat, m0, v0, t0=t0)
    for k, a in one.bits(True).items():
        assert np.array_equal(a, two.bits(True)[k]), "two calls differ in %s" % k
    # seven calls of one step, the statistics carried along
    p, m, v, counts, step_loss = flat, m0, v0, np.zeros(5, np.int64), []
    for s in range(7):
        r = Run(data, S, H, table[s:s + 1], p, m, v, t0=t0 + s, want_grad=(s % 2 == 0))
        p, m, v = r.params, r.m, r.v
        step_loss.append(r.step_loss[0])
        counts += r.counts
    assert np.array_equal(p.view(np.uint32), one.params.view(np.uint32))
    assert np.array_equal(m.view(np.uint32), one.m.view(np.uint32)) and np.array_equal(v.view(np.uint32), one.v.view(np.uint32))
    assert np.array_equal(np.array(step_loss).view(np.uint64), one.step_loss.view(np.uint64))
    assert np.array_equal(counts, one.counts)
    assert np.array_equal(r.last_grad.view(np.uint32), one.last_grad.view(np.uint32))  # the last step's gradient either way
    # running_loss: the same additions in the same order when the buffer is carried from call to call
    from srlz import ops
    loss = torch.zeros(1, dtype=torch.float64, device=_dev())
    cnt = torch.zeros(5, dtype=torch.int64, device=_dev())
    dp, dm, dv = (torch.from_numpy(a.copy()).to(_dev()) for a in (flat, m0, v0))
    for s in range(7):
        ops.headfit_fit(data, torch.from_numpy(table[s:s + 1].copy()), H, dp, dm, dv, t0 + s, LR, loss, cnt)
    assert np.array_equal(loss.cpu().numpy().view(np.uint64), one.loss.view(np.uint64)) and np.array_equal(cnt.cpu().numpy(), one.counts)
    assert np.array_equal(dp.cpu().numpy().view(np.uint32), one.params.view(np.uint32))


def test_bits_across_the_refill_of_the_step_scalar_table():
    """Adam's step scalars are computed 256 steps at a time: 300 steps in one call (one refill inside) against the same steps as two
    calls split at 131 (no refill in either: the 256th step of the whole lies in the middle of the second)."""
    S, H, B, n, cut, t0 = 3, 5, 1, 300, 131, 2
    states, labels = _states(S, seed=60), _labels(seed=61)
    data = _data(S, states, labels)
    table = _table(n, B, seed=62)
    flat = hu.random_params(S, H, seed=63)
    one = Run(data, S, H, table, flat, t0=t0)
    first = Run(data, S, H, table[:cut], flat, t0=t0)
    second = Run(data, S, H, table[cut:], first.params, first.m, first.v, t0=t0 + cut)
    for k in ("params", "m", "v", "last_grad"):
        assert np.array_equal(getattr(second, k).view(np.uint32), getattr(one, k).view(np.uint32)), k
    assert np.array_equal(np.concatenate((first.step_loss, second.step_loss)).view(np.uint64), one.step_loss.view(np.uint64))
    assert np.array_equal(first.counts + second.counts, one.counts)
    # (steps 256 .. 299 take their scalars from the refill in the one call and from the second call's first fill in the other:
    # equal bits mean the refill computes those of t0 + step + 1)
    assert one.step_loss.shape == (n,) and np.isfinite(one.step_loss).all() and np.isfinite(one.params).all()


@pytest.mark.parametrize("what", ["all_class_0", "all_class_1", "dead_first_layer"])
def test_degenerate_inputs_give_finite_results(what):
    S, H, B = 3, 16, 5
    states = _states(S, seed=20)
    labels = {"all_class_0": np.zeros(N, np.int64), "all_class_1": np.ones(N, np.int64), "dead_first_layer": _labels(seed=21)}[what]
    flat = hu.random_params(S, H, seed=22)
    if what == "dead_first_layer":  # W1 = 0 and b1 < 0: every ReLU of layer 1 is 0
        w = hu.unflatten(flat, S, H)
        w[0][:], w[1][:] = 0.0, -1.0
    table = _table(4, B, seed=23)
    run = Run(_data(S, states, labels), S, H, table, flat)
    p64, m64, v64, ph, grads = hu.fit(flat.astype(np.float64), np.zeros(flat.size), np.zeros(flat.size), 0, states, labels, table, LR, H)
    for k in ("params", "m", "v", "loss", "step_loss", "last_grad"):
        assert np.isfinite(getattr(run, k)).all(), k
    assert ru.scale_err(run.step_loss, ph.step_loss) <= BAR
    assert np.array_equal(run.counts[3:], ph.counts()[3:])
    if what == "all_class_0":
        assert run.counts[4] == 0 and run.counts[2] == 0
    if what == "all_class_1":
        assert run.counts[3] == 0 and run.counts[1] == 0
    if what == "dead_first_layer":
        g = hu.unflatten(run.last_grad, S, H)
        assert not g[0].any() and not g[1].any() and not g[2].any()  # nothing flows below the dead layer; W2's gradient needs h1
        w = hu.unflatten(run.params, S, H)
        assert not w[0].any() and (w[1] == -1.0).all()


@pytest.mark.parametrize("S,H,n_batches,B", [(1, 1, 1, 1), (3, 16, 3, 43), (17, 5, 2, 64), (200, 16, 5, 13), (341, 16, 1, 70), (201, 32, 2, 33)])
def test_eval_loss_and_counts(S, H, n_batches, B):
    from srlz import ops
    states, labels = _states(S, seed=30), _labels(seed=31)
    data = _data(S, states, labels)
    table = _table(n_batches, B, seed=32)
    flat = hu.random_params(S, H, seed=33)
    nbytes = (n_batches * B + 63) // 64 * 8
    pw, pv = _tailed(flat, torch.float32)
    lw, lv = _tailed(np.array([2.5]), torch.float64)  # added to, not overwritten
    cw, cv = _tailed(np.array([1, 0, 1, 0, 1], np.int64), torch.int64)
    ws = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device=_dev())
    for rep in range(2):  # the ticket is left zero: a second call adds the same again
        ops.headfit_eval(data, torch.from_numpy(table), H, pv, lv, cv, workspace=ws[:nbytes])
    torch.cuda.synchronize()
    assert _tail_ok(pw, flat.size) and _tail_ok(lw, 1) and _tail_ok(cw, 5) and bool((ws[nbytes:] == 0xA5).all())
    assert np.array_equal(pv.cpu().numpy().view(np.uint32), flat.view(np.uint32))  # params are only read
    ph = hu.evaluate(flat.astype(np.float64), states, labels, [table], H)
    got = (float(lv.cpu()[0]) - 2.5) / 2
    err = abs(got - ph.running_loss) / ph.running_loss
    lo, hi, soft = ph.bounds()
    counts = (cv.cpu().numpy() - np.array([1, 0, 1, 0, 1])) // 2
    print("eval S %d H %d rows %d: loss %.2e, %d soft rows" % (S, H, n_batches * B, err, soft))
    assert err <= BAR
    assert (lo <= counts).all() and (counts <= hi).all(), (counts, lo, hi)


def test_fit_and_eval_agree_on_the_forward():
    """One step with lr -> 0 leaves the parameters alone up to rounding: its loss is eval's loss on the same rows."""
    from srlz import ops
    S, H, B = 17, 5, 37
    states, labels = _states(S, seed=40), _labels(seed=41)
    data = _data(S, states, labels)
    table = _table(1, B, seed=42)
    flat = hu.random_params(S, H, seed=43)
    run = Run(data, S, H, table, flat, lr=1e-30)
    loss, counts = ops.reward_probe_stats(_dev())
    ops.headfit_eval(data, torch.from_numpy(table), H, torch.from_numpy(flat).to(_dev()), loss, counts)
    assert abs(float(loss.cpu()[0]) - run.loss[0]) <= 1e-5 * run.loss[0]  # (fit: the row loss in fp32; eval: in fp64)
    assert np.array_equal(counts.cpu().numpy(), run.counts)


def _raw_fit(data, S, H, table_dev, table_host, bufs, N_=None, n_steps=None, B=None, t0=0, null=None):
    from srlz import _cabi as C
    args = {"states": data.states, "labels": data.labels, "idx": table_dev, "params": bufs["params"][1], "m": bufs["m"][1], "v": bufs["v"][1],
            "loss": bufs["loss"][1], "counts": bufs["counts"][1], "step_loss": bufs["step_loss"][1], "last_grad": bufs["last_grad"][1]}
    p = {k: (None if k == null else C.ptr(t)) for k, t in args.items()}
    host = None if null == "idx_host" else ctypes.c_void_p(table_host.data_ptr())
    return C._lib.srlz_headfit_fit(p["states"], p["labels"], data.n if N_ is None else N_, S, H, p["idx"], host,
                                   table_host.shape[0] if n_steps is None else n_steps, table_host.shape[1] if B is None else B,
                                   p["params"], p["m"], p["v"], t0, LR, 0.9, 0.999, 1e-8, p["loss"], p["counts"], p["step_loss"],
                                   p["last_grad"], C.stream())


def test_refusals_leave_every_output_alone():
    from srlz import _cabi as C, ops
    S, H, B = 3, 16, 5
    data = _data(S)
    table = torch.from_numpy(_table(2, B, seed=50))
    d_table = table.to(_dev())
    P = hu.n_params(S, H)

    def fresh():
        return {"params": _tailed(np.full(P, SENT, np.float32), torch.float32), "m": _tailed(np.full(P, SENT, np.float32), torch.float32),
                "v": _tailed(np.full(P, SENT, np.float32), torch.float32), "loss": _tailed(np.full(1, SENT), torch.float64),
                "counts": _tailed(np.full(5, -77, np.int64), torch.int64), "step_loss": _tailed(np.full(2, SENT), torch.float64),
                "last_grad": _tailed(np.full(P, SENT, np.float32), torch.float32)}

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(bool((w == (SENT if w.dtype.is_floating_point else -77)).all()) for w, _ in bufs.values())
    bad_idx = table.clone()
    bad_idx[1, 2] = N - 1
    neg_idx = table.clone()
    neg_idx[0, 0] = -1
    for kw, code in ((dict(H=33), -1), (dict(H=0), -1), (dict(S=0), -1), (dict(host=bad_idx), -1), (dict(host=neg_idx), -1), (dict(N_=1), -1),
                     (dict(n_steps=0), -1), (dict(B=0), -1), (dict(t0=-1), -1), (dict(N_=1 << 30), -1),
                     (dict(null="params"), -4), (dict(null="m"), -4), (dict(null="v"), -4), (dict(null="states"), -4),
                     (dict(null="labels"), -4), (dict(null="idx"), -4), (dict(null="idx_host"), -4), (dict(null="loss"), -4),
                     (dict(null="counts"), -4)):
        bufs = fresh()
        kw = dict(kw)
        host = kw.pop("host", table)
        rc = _raw_fit(data, kw.pop("S", S), kw.pop("H", H), d_table, host, bufs, **kw)
        assert rc == code, (kw, rc, C.error_text())
        assert untouched(bufs), kw
    # step_loss and last_grad are optional
    bufs = fresh()
    bufs["params"][1].zero_(); bufs["m"][1].zero_(); bufs["v"][1].zero_(); bufs["loss"][1].zero_(); bufs["counts"][1].zero_()
    assert _raw_fit(data, S, H, d_table, table, bufs, null="step_loss") == 0
    torch.cuda.synchronize()
    assert bool((bufs["step_loss"][0] == SENT).all()) and not bool((bufs["last_grad"][1] == SENT).any())
    # eval: the same checks, and a short workspace
    loss_w, loss = _tailed(np.full(1, SENT), torch.float64)
    cnt_w, cnt = _tailed(np.full(5, -77, np.int64), torch.int64)
    ws = torch.full((64,), 0xA5, dtype=torch.uint8, device=_dev())
    ticket = torch.zeros(1, dtype=torch.int32, device=_dev())
    params = torch.zeros(P, dtype=torch.float32, device=_dev())

    def raw_eval(H_=H, host=table, ws_bytes=8, null=None, N_=N):
        a = {"states": data.states, "labels": data.labels, "idx": d_table, "params": params, "loss": loss, "counts": cnt, "ws": ws,
             "ticket": ticket}
        p = {k: (None if k == null else C.ptr(t)) for k, t in a.items()}
        return C._lib.srlz_headfit_eval(p["states"], p["labels"], N_, S, H_, p["idx"], ctypes.c_void_p(host.data_ptr()), 2, B, p["params"],
                                        p["loss"], p["counts"], p["ws"], ws_bytes, p["ticket"], C.stream())
    for kw, code in ((dict(H_=33), -1), (dict(host=bad_idx), -1), (dict(N_=1), -1), (dict(null="ws"), -4), (dict(null="ticket"), -4),
                     (dict(null="params"), -4), (dict(null="loss"), -4), (dict(ws_bytes=7), -2), (dict(ws_bytes=0), -2)):
        rc = raw_eval(**kw)
        torch.cuda.synchronize()
        assert rc == code, (kw, rc, C.error_text())
        assert bool((loss_w == SENT).all()) and bool((cnt_w == -77).all()) and bool((ws == 0xA5).all()) and int(ticket.cpu()[0]) == 0, kw
    assert "workspace" in C.error_text()
    # the Python layer: its own error types
    with pytest.raises(ValueError, match="srlz_headfit_supported"):
        ops.headfit_fit(data, table, 33, params, params, params, 0, LR, loss, cnt)
    with pytest.raises(ValueError, match="float32"):
        ops.headfit_fit(data, table, H, params.double(), params, params, 0, LR, loss, cnt)
    with pytest.raises(ValueError, match="holds"):
        ops.headfit_fit(data, table, H, params[:-1], params, params, 0, LR, loss, cnt)
    with pytest.raises(ValueError, match="contiguous"):
        ops.headfit_eval(data, table, H, torch.zeros(2 * P, device=_dev())[::2], loss, cnt)
    with pytest.raises(ValueError, match="int32"):
        ops.headfit_eval(data, table.long(), H, params, loss, cnt)
    with pytest.raises(C.SrlzError, match="no CPU fallback"):
        ops.headfit_eval(data, table, H, params.cpu(), loss, cnt)
    with pytest.raises(C.SrlzError, match="outside"):
        ops.headfit_fit(data, bad_idx, H, params, torch.zeros_like(params), torch.zeros_like(params), 0, LR, torch.zeros(1, dtype=torch.float64, device=_dev()),
                        torch.zeros(5, dtype=torch.int64, device=_dev()))
