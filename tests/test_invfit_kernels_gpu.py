"""srlz_invfit_fit / srlz_invfit_eval (csrc/invfit.hip) entry by entry against the float64 restatement of tests/invfit_util.py.

The bar is the project's gradient rule: every entry of last_grad within 1e-4 of its tensor's scale (max |reference|), the step loss
within 1e-4 relative.  The parameters after one step from zero moments are held through the gradient, as
tests/test_headfit_kernels_gpu.py holds them and for its reason: Adam's first step is lr * sign(g) wherever |g| >> eps, so a float64
trajectory would compare signs of entries that are zero up to rounding; instead the kernel's own gradient goes through the float64
Adam and must give the kernel's moments (2e-6 of scale: a handful of float32 roundings per element) and its step (1e-5 of the
step's scale: the parameter it is added to is stored in float32).  Bit guarantees are asserted as bits.  Every buffer the kernels
write has a sentinel tail.

Measured on one MI355X, worst over the 30 one-step cases: gradient entry 9.0e-07 of its tensor's scale (S = 17, A = 5, B = 259), step
loss 7.8e-08 relative and the step through the gradient 6.0e-06 (both at S = 1, A = 1676, B = 16), m 6.4e-08, v 1.3e-07; three steps
from non-zero moments at t0 = 10: parameters' movement 2.3e-06, m 7.9e-08, v 1.5e-07, gradient 7.1e-08, losses 4.7e-08; eval loss
within 3.4e-09 relative, no soft row in any case, every count equal."""
import ctypes

import numpy as np
import pytest
import torch

import invfit_util as iu
import reward_util as ru

pytestmark = pytest.mark.gpu

BAR = 1e-4
TAIL = 64
SENT = -12345.5
N = 40
LR = 0.005


def _largest_s(A):
    s = 1
    while iu.chunk_rows(s + 1, A):
        s += 1
    return s


def _largest_a():
    a = 2
    while iu.chunk_rows(1, a + 1):
        a += 1
    return a


# (1,2) the smallest head; (3,6) the reference head on ground truth; (17,5) odd sizes that are no multiple of a quad or of the 16 lanes;
# (200,6) the widest quoted state; the largest S the predicate accepts at A = 6 (chunks of 16 rows); the largest A it accepts, at that
# A's largest S.  The formula is the header's (tests/test_invfit_host_cpu.py holds the library to it).
SHAPES = ((1, 2), (3, 6), (17, 5), (200, 6), (_largest_s(6), 6), (_largest_s(_largest_a()), _largest_a()))
CASES = [(S, A, bi) for S, A in SHAPES for bi in range(5)]


def _dev():
    return torch.device("cuda", 0)


def _batch_sizes(S, A):
    from srlz import ops
    r = ops.invfit_chunk_rows(S, A)
    assert r == iu.chunk_rows(S, A) and r >= 16
    return (1, 5, r, r + 1, 2 * r + 3)


def _states(S, seed=0):
    return np.random.RandomState(seed).randn(N, S).astype(np.float32)


def _labels(A, seed=1):
    return np.random.RandomState(seed).randint(0, A, N).astype(np.int64)


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


def _data(states, labels):
    """(states, actions) on the device; the labels are NOT range-checked: the kernels count what they cannot index."""
    from srlz import ops
    return ops.RewardProbeData(torch.from_numpy(np.ascontiguousarray(states, np.float32)).to(_dev()),
                               torch.from_numpy(np.asarray(labels).astype(np.int32)).to(_dev()))


class Run(object):
    """One srlz_invfit_fit call through ops.invfit_fit with sentinel tails everywhere; the results on the host."""

    def __init__(self, data, S, A, table, flat, m=None, v=None, t0=0, lr=LR, want_grad=True):
        from srlz import ops
        P, n = iu.n_params(S, A), table.shape[0]
        zeros = np.zeros(P, np.float32)
        self.bufs = {"params": _tailed(flat, torch.float32), "m": _tailed(zeros if m is None else m, torch.float32),
                     "v": _tailed(zeros if v is None else v, torch.float32), "loss": _tailed(np.zeros(1), torch.float64),
                     "counts": _tailed(np.zeros(iu.n_counts(A), np.int64), torch.int64), "step_loss": _tailed(np.full(n, SENT), torch.float64),
                     "last_grad": _tailed(np.full(P, SENT, np.float32), torch.float32)}
        b = {k: w[1] for k, w in self.bufs.items()}
        ops.invfit_fit(data, torch.from_numpy(table), A, b["params"], b["m"], b["v"], t0, lr, b["loss"], b["counts"], b["step_loss"],
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


def _tensor_errs(got, ref, S, A):
    return [ru.scale_err(g, r) for g, r in zip(iu.unflatten(np.asarray(got, np.float64), S, A), iu.unflatten(ref, S, A))]


def _counts_ok(got, z, y):
    lo, hi, soft = iu.count_bounds(z, y)
    A = z.shape[1]
    assert (lo <= got).all() and (got <= hi).all(), (got, lo, hi)  # equal unless a row is soft
    assert got[0] == got[3:3 + A].sum() + got[2] and got[1] == got[3 + A:].sum() and (got[3 + A:] <= got[3:3 + A]).all()
    return soft


@pytest.mark.parametrize("S,A,bi", CASES, ids=["S%d-A%d-b%d" % c for c in CASES])
def test_one_step_gradient_loss_and_update(S, A, bi):
    B = _batch_sizes(S, A)[bi]
    states, labels = _states(S, seed=S), _labels(A, seed=A)
    table = _table(1, B, seed=B)
    if B >= 4:
        assert 0 in table and N - 2 in table and len(set(table[0].tolist())) < B
    flat = iu.random_params(S, A, seed=7)
    run = Run(_data(states, labels), S, A, table, flat)
    loss, g, z = iu.loss_and_grad(flat.astype(np.float64), ru.rows(states, table[0]), labels[table[0]], A)
    errs = _tensor_errs(run.last_grad, g, S, A)
    e_loss = abs(run.step_loss[0] - loss) / abs(loss)
    # the update through the kernel's own gradient
    p64, m64, v64 = ru.adam(flat.astype(np.float64), run.last_grad.astype(np.float64), np.zeros_like(g), np.zeros_like(g), 1, LR)
    e_par = max(_tensor_errs(run.params - flat, p64 - flat, S, A))  # the step itself, not the parameter it is added to
    e_m, e_v = ru.scale_err(run.m, m64), ru.scale_err(run.v, v64)
    print("S %d A %d B %d: gradient %.2e loss %.2e step %.2e m %.2e v %.2e" % (S, A, B, max(errs), e_loss, e_par, e_m, e_v))
    assert max(errs) <= BAR, errs
    assert e_loss <= BAR
    assert e_m <= 2e-6 and e_v <= 2e-6  # a handful of float32 roundings (6e-8 each) per element, nothing else
    # the parameter is stored in float32: an entry of size 0.5 (random_params' largest) carries 3e-8 of rounding, 6e-6 of a step of LR
    assert e_par <= 1e-5
    assert abs(run.loss[0] - run.step_loss[0] * B) <= 1e-12 * B
    _counts_ok(run.counts, z, labels[table[0]])
    assert run.counts[0] == B and run.counts[2] == 0


def test_three_steps_from_nonzero_moments_at_t0_10():
    S, A, B, t0, lr = 17, 5, 5, 10, 0.05  # (a rate at which three steps stand well clear of the float32 rounding of the parameters)
    states, labels = _states(S, seed=3), _labels(A, seed=4)
    table = _table(3, B, seed=9)
    rs = np.random.RandomState(5)
    flat, P = iu.random_params(S, A, seed=8), iu.n_params(S, A)
    m0, v0 = (0.01 * rs.randn(P)).astype(np.float32), rs.uniform(1e-3, 1e-2, P).astype(np.float32)  # v well above g^2 rounding: smooth steps
    run = Run(_data(states, labels), S, A, table, flat, m0, v0, t0=t0, lr=lr)
    p64, m64, v64, ph, grads = iu.fit(flat.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), t0, states, labels, table, lr, A)
    errs = {"params": max(_tensor_errs(run.params - flat, p64 - flat, S, A)), "m": ru.scale_err(run.m, m64), "v": ru.scale_err(run.v, v64),
            "grad": max(_tensor_errs(run.last_grad, grads[-1], S, A)), "loss": ru.scale_err(run.step_loss, ph.step_loss)}
    print("three steps at t0 = 10: %s" % errs)
    assert max(errs.values()) <= BAR, errs
    assert abs(run.loss[0] - ph.running_loss) <= BAR * ph.running_loss
    assert _counts_ok(run.counts, *ph.logits()) > 0 or np.array_equal(run.counts, ph.counts())


@pytest.mark.parametrize("S,A,B", [(17, 5, 5), (3, 6, 259), (200, 6, 75), (1, 2, 1)])
def test_bits_two_calls_and_seven_steps_in_one_call_or_seven(S, A, B):
    states, labels = _states(S, seed=11), _labels(A, seed=12)
    data = _data(states, labels)
    table = _table(7, B, seed=13)
    rs = np.random.RandomState(6)
    flat, P = iu.random_params(S, A, seed=14), iu.n_params(S, A)
    m0, v0, t0 = (0.01 * rs.randn(P)).astype(np.float32), rs.uniform(1e-4, 1e-3, P).astype(np.float32), 3
    one = Run(data, S, A, table, flat, m0, v0, t0=t0)
    two = Run(data, S, A, table, flat, m0, v0, t0=t0)
    for k, a in one.bits(True).items():
        assert np.array_equal(a, two.bits(True)[k]), "two calls differ in %s" % k
    # seven calls of one step, the statistics carried along
    p, m, v, counts, step_loss = flat, m0, v0, np.zeros(iu.n_counts(A), np.int64), []
    for s in range(7):
        r = Run(data, S, A, table[s:s + 1], p, m, v, t0=t0 + s, want_grad=(s % 2 == 0))
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
    cnt = torch.zeros(iu.n_counts(A), dtype=torch.int64, device=_dev())
    dp, dm, dv = (torch.from_numpy(a.copy()).to(_dev()) for a in (flat, m0, v0))
    for s in range(7):
        ops.invfit_fit(data, torch.from_numpy(table[s:s + 1].copy()), A, dp, dm, dv, t0 + s, LR, loss, cnt)
    assert np.array_equal(loss.cpu().numpy().view(np.uint64), one.loss.view(np.uint64)) and np.array_equal(cnt.cpu().numpy(), one.counts)
    assert np.array_equal(dp.cpu().numpy().view(np.uint32), one.params.view(np.uint32))


def test_bits_padded_entries_never_leak_into_params():
    """A = 5 is padded to 8 outputs (a stride of 12) in LDS.  What the pads hold must not matter: the same call gives the same bits
    after a launch of a wider head with large parameters has left other values where the pads (and everything else) will lie, and
    the result is the float64 one — a pad that joined the softmax or the update would move it."""
    S, A, B = 17, 5, 37
    states, labels = _states(S, seed=70), _labels(A, seed=71)
    data = _data(states, labels)
    table = _table(4, B, seed=72)
    flat = iu.random_params(S, A, seed=73)
    first = Run(data, S, A, table, flat)
    wide = 8
    Run(_data(states, _labels(wide, seed=74)), S, wide, table, 100.0 * iu.random_params(S, wide, seed=75), lr=0.5)
    second = Run(data, S, A, table, flat)
    for k, a in first.bits(True).items():
        assert np.array_equal(a, second.bits(True)[k]), "the call depends on what LDS held before it: %s" % k
    p64, m64, v64, ph, grads = iu.fit(flat.astype(np.float64), np.zeros(flat.size), np.zeros(flat.size), 0, states, labels, table, LR, A)
    assert ru.scale_err(first.step_loss, ph.step_loss) <= BAR and max(_tensor_errs(first.last_grad, grads[-1], S, A)) <= BAR
    assert first.params.shape == (iu.n_params(S, A),) and np.isfinite(first.params).all()


def test_bits_across_the_refill_of_the_step_scalar_table():
    """Adam's step scalars are computed 256 steps at a time: 300 steps in one call (one refill inside) against the same steps as two
    calls split at 131 (no refill in either: the 256th step of the whole lies in the middle of the second)."""
    S, A, B, n, cut, t0 = 3, 5, 1, 300, 131, 2
    states, labels = _states(S, seed=60), _labels(A, seed=61)
    data = _data(states, labels)
    table = _table(n, B, seed=62)
    flat = iu.random_params(S, A, seed=63)
    one = Run(data, S, A, table, flat, t0=t0)
    first = Run(data, S, A, table[:cut], flat, t0=t0)
    second = Run(data, S, A, table[cut:], first.params, first.m, first.v, t0=t0 + cut)
    for k in ("params", "m", "v", "last_grad"):
        assert np.array_equal(getattr(second, k).view(np.uint32), getattr(one, k).view(np.uint32)), k
    assert np.array_equal(np.concatenate((first.step_loss, second.step_loss)).view(np.uint64), one.step_loss.view(np.uint64))
    assert np.array_equal(first.counts + second.counts, one.counts)
    assert one.step_loss.shape == (n,) and np.isfinite(one.step_loss).all() and np.isfinite(one.params).all()


@pytest.mark.parametrize("bad_label", [6, -1, 1 << 30, -(1 << 31)])
def test_a_label_out_of_range_adds_nothing_and_is_counted(bad_label):
    """One row of the batch carries a label outside [0, A): loss and gradient are what they are without that row (the mean still
    divides by B), bad == 1, and nothing is indexed by the label — in the fit and in the eval."""
    from srlz import ops
    S, A, B = 3, 6, 21
    states, labels = _states(S, seed=80), _labels(A, seed=81)
    table = _table(1, B, seed=82)
    victim = next(int(i) for i in table[0, 4:] if (table[0] == i).sum() == 1)  # a frame the batch holds once: one bad row
    labels[victim] = bad_label
    flat = iu.random_params(S, A, seed=83)
    data = _data(states, labels)
    run = Run(data, S, A, table, flat)
    keep = table[0] != victim
    X, y = ru.rows(states, table[0]), labels[table[0]]
    loss, g, z = iu.loss_and_grad(flat.astype(np.float64), X, y, A)
    l_wo, g_wo, _ = iu.loss_and_grad(flat.astype(np.float64), X[keep], y[keep], A)
    assert abs(loss * B - l_wo * (B - 1)) < 1e-12 and np.abs(g * B - g_wo * (B - 1)).max() < 1e-12  # the restatement says the same
    assert max(_tensor_errs(run.last_grad, g, S, A)) <= BAR and abs(run.step_loss[0] - loss) <= BAR * loss
    assert run.counts[2] == 1 and run.counts[0] == B and run.counts[3:3 + A].sum() == B - 1
    _counts_ok(run.counts, z, y)
    loss_d = torch.zeros(1, dtype=torch.float64, device=_dev())
    cw, cv = _tailed(np.zeros(iu.n_counts(A), np.int64), torch.int64)
    ops.invfit_eval(data, torch.from_numpy(table), A, torch.from_numpy(flat).to(_dev()), loss_d, cv)
    torch.cuda.synchronize()
    assert _tail_ok(cw, iu.n_counts(A))
    got = cv.cpu().numpy()
    assert abs(float(loss_d.cpu()[0]) - loss * B) <= BAR * loss * B and got[2] == 1
    _counts_ok(got, z, y)


@pytest.mark.parametrize("S,A,n_batches,B", [(1, 2, 1, 1), (3, 6, 3, 43), (17, 5, 2, 64), (200, 6, 5, 13), (SHAPES[4][0], 6, 1, 70),
                                             (SHAPES[5][0], SHAPES[5][1], 2, 33)])
def test_eval_loss_and_counts(S, A, n_batches, B):
    from srlz import ops
    states, labels = _states(S, seed=30), _labels(A, seed=31)
    data = _data(states, labels)
    table = _table(n_batches, B, seed=32)
    flat = iu.random_params(S, A, seed=33)
    nbytes = (n_batches * B + 63) // 64 * 8
    base = np.arange(iu.n_counts(A), dtype=np.int64) % 3  # added to, not overwritten
    pw, pv = _tailed(flat, torch.float32)
    lw, lv = _tailed(np.array([2.5]), torch.float64)
    cw, cv = _tailed(base, torch.int64)
    ws = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device=_dev())
    for rep in range(2):  # the ticket is left zero: a second call adds the same again
        ops.invfit_eval(data, torch.from_numpy(table), A, pv, lv, cv, workspace=ws[:nbytes])
    torch.cuda.synchronize()
    assert _tail_ok(pw, flat.size) and _tail_ok(lw, 1) and _tail_ok(cw, base.size) and bool((ws[nbytes:] == 0xA5).all())
    assert np.array_equal(pv.cpu().numpy().view(np.uint32), flat.view(np.uint32))  # params are only read
    ph = iu.evaluate(flat.astype(np.float64), states, labels, [table], A)
    got = (float(lv.cpu()[0]) - 2.5) / 2
    err = abs(got - ph.running_loss) / ph.running_loss
    counts = (cv.cpu().numpy() - base) // 2
    soft = _counts_ok(counts, *ph.logits())
    print("eval S %d A %d rows %d: loss %.2e, %d soft rows" % (S, A, n_batches * B, err, soft))
    assert err <= BAR and counts[0] == n_batches * B and counts[2] == 0


def test_argmax_tie_goes_to_the_lowest_class():
    """Zero weights and a bias with its maximum at classes 1 and 3: exact in float32, every row predicts class 1."""
    from srlz import ops
    S, A, B = 3, 6, 20
    states = _states(S, seed=90)
    labels = np.array([1, 3] * (N // 2), np.int64)
    table = np.arange(B, dtype=np.int32).reshape(1, B)
    flat = np.zeros(iu.n_params(S, A), np.float32)
    flat[2 * S * A:] = (0.0, 0.5, 0.25, 0.5, -1.0, 0.0)
    data = _data(states, labels)
    run = Run(data, S, A, table, flat, lr=1e-30)
    loss, cnt = torch.zeros(1, dtype=torch.float64, device=_dev()), torch.zeros(iu.n_counts(A), dtype=torch.int64, device=_dev())
    ops.invfit_eval(data, torch.from_numpy(table), A, torch.from_numpy(flat).to(_dev()), loss, cnt)
    for got in (run.counts, cnt.cpu().numpy()):
        assert got[1] == B // 2 and got[3 + A + 1] == B // 2 and got[3 + A + 3] == 0 and got[3 + 1] == got[3 + 3] == B // 2


def test_fit_and_eval_agree_on_the_forward():
    """One step with lr -> 0 leaves the parameters alone up to rounding: its loss is eval's loss on the same rows."""
    from srlz import ops
    S, A, B = 17, 5, 37
    states, labels = _states(S, seed=40), _labels(A, seed=41)
    data = _data(states, labels)
    table = _table(1, B, seed=42)
    flat = iu.random_params(S, A, seed=43)
    run = Run(data, S, A, table, flat, lr=1e-30)
    loss, counts = torch.zeros(1, dtype=torch.float64, device=_dev()), torch.zeros(iu.n_counts(A), dtype=torch.int64, device=_dev())
    ops.invfit_eval(data, torch.from_numpy(table), A, torch.from_numpy(flat).to(_dev()), loss, counts)
    assert abs(float(loss.cpu()[0]) - run.loss[0]) <= 1e-5 * run.loss[0]  # (fit: the row loss in fp32; eval: in fp64)
    assert np.array_equal(counts.cpu().numpy(), run.counts)


def _raw_fit(data, S, A, table_dev, table_host, bufs, N_=None, n_steps=None, B=None, t0=0, null=None):
    from srlz import _cabi as C
    args = {"states": data.states, "labels": data.labels, "idx": table_dev, "params": bufs["params"][1], "m": bufs["m"][1], "v": bufs["v"][1],
            "loss": bufs["loss"][1], "counts": bufs["counts"][1], "step_loss": bufs["step_loss"][1], "last_grad": bufs["last_grad"][1]}
    p = {k: (None if k == null else C.ptr(t)) for k, t in args.items()}
    host = None if null == "idx_host" else ctypes.c_void_p(table_host.data_ptr())
    return C._lib.srlz_invfit_fit(p["states"], p["labels"], data.n if N_ is None else N_, S, A, p["idx"], host,
                                  table_host.shape[0] if n_steps is None else n_steps, table_host.shape[1] if B is None else B,
                                  p["params"], p["m"], p["v"], t0, LR, 0.9, 0.999, 1e-8, p["loss"], p["counts"], p["step_loss"],
                                  p["last_grad"], C.stream())


def test_refusals_leave_every_output_alone():
    from srlz import _cabi as C, ops
    S, A, B = 3, 6, 5
    data = _data(_states(S), _labels(A))
    table = torch.from_numpy(_table(2, B, seed=50))
    d_table = table.to(_dev())
    P, NC = iu.n_params(S, A), iu.n_counts(A)

    def fresh():
        return {"params": _tailed(np.full(P, SENT, np.float32), torch.float32), "m": _tailed(np.full(P, SENT, np.float32), torch.float32),
                "v": _tailed(np.full(P, SENT, np.float32), torch.float32), "loss": _tailed(np.full(1, SENT), torch.float64),
                "counts": _tailed(np.full(NC, -77, np.int64), torch.int64), "step_loss": _tailed(np.full(2, SENT), torch.float64),
                "last_grad": _tailed(np.full(P, SENT, np.float32), torch.float32)}

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(bool((w == (SENT if w.dtype.is_floating_point else -77)).all()) for w, _ in bufs.values())
    bad_idx = table.clone()
    bad_idx[1, 2] = N - 1
    neg_idx = table.clone()
    neg_idx[0, 0] = -1
    for kw, code in ((dict(A=1), -1), (dict(A=0), -1), (dict(A=1 << 20), -1), (dict(S=0), -1), (dict(host=bad_idx), -1), (dict(host=neg_idx), -1),
                     (dict(N_=1), -1), (dict(n_steps=0), -1), (dict(B=0), -1), (dict(t0=-1), -1), (dict(N_=1 << 30), -1),
                     (dict(null="params"), -4), (dict(null="m"), -4), (dict(null="v"), -4), (dict(null="states"), -4),
                     (dict(null="labels"), -4), (dict(null="idx"), -4), (dict(null="idx_host"), -4), (dict(null="loss"), -4),
                     (dict(null="counts"), -4)):
        bufs = fresh()
        kw = dict(kw)
        host = kw.pop("host", table)
        rc = _raw_fit(data, kw.pop("S", S), kw.pop("A", A), d_table, host, bufs, **kw)
        assert rc == code, (kw, rc, C.error_text())
        assert untouched(bufs), kw
    # step_loss and last_grad are optional
    bufs = fresh()
    bufs["params"][1].zero_(); bufs["m"][1].zero_(); bufs["v"][1].zero_(); bufs["loss"][1].zero_(); bufs["counts"][1].zero_()
    assert _raw_fit(data, S, A, d_table, table, bufs, null="step_loss") == 0
    torch.cuda.synchronize()
    assert bool((bufs["step_loss"][0] == SENT).all()) and not bool((bufs["last_grad"][1] == SENT).any())
    # eval: the same checks, and a short workspace
    loss_w, loss = _tailed(np.full(1, SENT), torch.float64)
    cnt_w, cnt = _tailed(np.full(NC, -77, np.int64), torch.int64)
    ws = torch.full((64,), 0xA5, dtype=torch.uint8, device=_dev())
    ticket = torch.zeros(1, dtype=torch.int32, device=_dev())
    params = torch.zeros(P, dtype=torch.float32, device=_dev())

    def raw_eval(A_=A, host=table, ws_bytes=8, null=None, N_=N):
        a = {"states": data.states, "labels": data.labels, "idx": d_table, "params": params, "loss": loss, "counts": cnt, "ws": ws,
             "ticket": ticket}
        p = {k: (None if k == null else C.ptr(t)) for k, t in a.items()}
        return C._lib.srlz_invfit_eval(p["states"], p["labels"], N_, S, A_, p["idx"], ctypes.c_void_p(host.data_ptr()), 2, B, p["params"],
                                       p["loss"], p["counts"], p["ws"], ws_bytes, p["ticket"], C.stream())
    for kw, code in ((dict(A_=1), -1), (dict(host=bad_idx), -1), (dict(N_=1), -1), (dict(null="ws"), -4), (dict(null="ticket"), -4),
                     (dict(null="params"), -4), (dict(null="loss"), -4), (dict(ws_bytes=7), -2), (dict(ws_bytes=0), -2)):
        rc = raw_eval(**kw)
        torch.cuda.synchronize()
        assert rc == code, (kw, rc, C.error_text())
        assert bool((loss_w == SENT).all()) and bool((cnt_w == -77).all()) and bool((ws == 0xA5).all()) and int(ticket.cpu()[0]) == 0, kw
    assert "workspace" in C.error_text()
    # the Python layer: its own error types, those of the headfit wrappers
    zl, zc = torch.zeros(1, dtype=torch.float64, device=_dev()), torch.zeros(NC, dtype=torch.int64, device=_dev())
    with pytest.raises(ValueError, match="srlz_invfit_supported"):
        ops.invfit_fit(data, table, 1, params, params, params, 0, LR, zl, zc)
    with pytest.raises(ValueError, match="float32"):
        ops.invfit_fit(data, table, A, params.double(), params, params, 0, LR, zl, zc)
    with pytest.raises(ValueError, match="holds"):
        ops.invfit_fit(data, table, A, params[:-1], params, params, 0, LR, zl, zc)
    with pytest.raises(ValueError, match="holds"):
        ops.invfit_eval(data, table, A, params, zl, zc[:-1])
    with pytest.raises(ValueError, match="contiguous"):
        ops.invfit_eval(data, table, A, torch.zeros(2 * P, device=_dev())[::2], zl, zc)
    with pytest.raises(ValueError, match="int32"):
        ops.invfit_eval(data, table.long(), A, params, zl, zc)
    with pytest.raises(C.SrlzError, match="no CPU fallback"):
        ops.invfit_eval(data, table, A, params.cpu(), zl, zc)
    with pytest.raises(C.SrlzError, match="outside"):
        ops.invfit_fit(data, bad_idx, A, params, torch.zeros_like(params), torch.zeros_like(params), 0, LR, zl, zc)
