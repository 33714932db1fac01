"""srlz_reward_probe_fit / srlz_reward_probe_eval (csrc/reward_probe.hip) through srlz.ops against the float64 restatement of
tests/reward_util.py.

Tolerances: a step's loss 1e-5 relative; updated parameters, m and v 1e-4 of each tensor's scale (the project's tolerance for
gradients and outputs); counts exact except for rows whose float64 logit margin is below 1e-4 * max|z| (at most 1 % of the rows,
asserted on the float64 side).  Conditions on the inputs, asserted on the float64 side before anything is compared: no gradient
element with 0 < |g| < 1e-6 * max|g| (Adam's first step is +-lr whatever |g| is), no pre-activation within 1e-5 of zero (the
float32 forward must take the same ReLU branches); the inputs are the first of a few seeds for which they hold.

Measured on one MI355X over the 56 single steps: loss within 7.2e-8, parameters 1.6e-6, m 1.2e-5, v 2.4e-5; running_loss of the
free-running 300-step case within 4e-8, of eval within 2e-9."""
import numpy as np
import pytest
import torch

import reward_util as ru

pytestmark = pytest.mark.gpu

LR = 0.005
SENTINEL = 12345.0
TAIL = 7
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from srlz import ops as _ops
    return _ops


def problem(S, N=96, seed=0, dead=False):
    """states float32 [N, S], labels, and torch-style initial parameters (uniform +-1/sqrt(fan_in)) rounded to float32."""
    rs = np.random.RandomState(1000 * S + seed)
    states = rs.randn(N, S).astype(np.float32)
    labels = (rs.rand(N) > 0.6).astype(np.int64)
    parts = []
    for shp, fan in zip(ru.shapes(S), (2 * S, 2 * S, 4, 4, 4, 4)):
        parts.append(rs.uniform(-1, 1, shp).reshape(-1) / np.sqrt(fan))
    flat = np.concatenate(parts)
    if dead:
        flat[8 * S + 2] = -1000.0  # b1[2]: hidden unit 2 of layer 1 never fires
    return states, labels, flat.astype(np.float32).astype(np.float64)


def table(N, n, B, seed):
    return np.random.RandomState(seed).randint(0, N - 1, (n, B)).astype(np.int64)


def padded(a, dtype):
    """A device buffer with a sentinel tail behind it -> (view of the payload, whole buffer)."""
    a = np.asarray(a)
    whole = torch.full((a.size + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    whole[:a.size] = torch.from_numpy(a.reshape(-1)).to(dtype)
    return whole[:a.size], whole


def tails_intact(*wholes):
    return all(bool((w[-TAIL:] == SENTINEL).all()) for w in wholes)


class Gpu(object):
    """The device side of one run: params / m / v / statistics, each with a sentinel tail."""

    def __init__(self, ops, states, labels, flat, m=None, v=None, n_steps=0):
        self.ops = ops
        self.data = ops.reward_probe_data(states, labels)
        zeros = np.zeros_like(flat)
        self.p, self.p_all = padded(flat, torch.float32)
        self.m, self.m_all = padded(zeros if m is None else m, torch.float32)
        self.v, self.v_all = padded(zeros if v is None else v, torch.float32)
        self.loss, self.loss_all = padded(np.zeros(1), torch.float64)
        self.counts, self.counts_all = padded(np.zeros(5), torch.int64)
        self.step_loss, self.step_all = padded(np.zeros(max(n_steps, 1)), torch.float64)

    def fit(self, tab, t0, step_loss=True, offset=0):
        tab = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.int32))
        sl = self.step_loss[offset:offset + len(tab)] if step_loss else None
        self.ops.reward_probe_fit(self.data, tab, self.p, self.m, self.v, t0, LR, self.loss, self.counts, step_loss=sl)
        torch.cuda.synchronize()

    def eval(self, tab):
        self.ops.reward_probe_eval(self.data, torch.from_numpy(np.ascontiguousarray(tab, dtype=np.int32)), self.p, self.loss, self.counts)
        torch.cuda.synchronize()

    def intact(self):
        return tails_intact(self.p_all, self.m_all, self.v_all, self.loss_all, self.counts_all, self.step_all)

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.p, self.m, self.v, self.loss, self.counts, self.step_loss)]


def well_posed(states, labels, flat, tab):
    """The conditions on the inputs (module docstring), on the float64 side -> None, or what is wrong."""
    for idx in tab:
        X = ru.rows(states, idx)
        w1, b1, w2, b2, _, _ = ru.unflatten(flat, X.shape[1] // 2)
        h1 = np.maximum(X @ w1.T + b1, 0)
        pre = np.concatenate([(X @ w1.T + b1).reshape(-1), (h1 @ w2.T + b2).reshape(-1)])
        if np.abs(pre).min() <= 1e-5:
            return "a pre-activation sits on the ReLU's corner"
        g = ru.loss_and_grad(flat, X, labels[idx])[1]
        nz = np.abs(g[g != 0])
        if not nz.size or nz.min() < 1e-6 * nz.max():
            return "a gradient element is almost zero: Adam's step would be ill-posed"
    return None


def per_tensor_err(got, ref, S):
    return max(ru.scale_err(g, r) for g, r in zip(ru.unflatten(np.asarray(got, dtype=np.float64), S), ru.unflatten(ref, S)))


def check_counts(got, phase):
    lo, hi, soft = phase.bounds()
    assert soft <= 0.01 * len(phase.logits()[1]), "too many rows without a margin: %d" % soft
    assert (lo <= got).all() and (got <= hi).all(), (got, lo, hi)


def teacher_forced(S, B, t0, dead, seed):
    """The float64 trajectory up to t0, cast to float32, is where BOTH sides start."""
    states, labels, flat = problem(S, seed=seed, dead=dead)
    N = len(states)
    warm = table(N, t0, B, seed=50 + seed)
    tab = table(N, 1, B, seed=60 + seed)
    flat, m, v, _, _ = ru.fit(flat, np.zeros_like(flat), np.zeros_like(flat), 0, states, labels, warm, LR)
    flat, m, v = [a.astype(np.float32).astype(np.float64) for a in (flat, m, v)]
    return states, labels, flat, m, v, tab


def single_step(ops, S, B, t0, dead=False, seed=0):
    # the inputs are chosen on the float64 side alone: the first of a few seeds whose step is well-posed
    for attempt in range(8):
        states, labels, flat, m, v, tab = teacher_forced(S, B, t0, dead, seed + 100 * attempt)
        why = well_posed(states, labels, flat, tab)
        if why is None:
            break
    assert why is None, why
    rflat, rm, rv, ph, grads = ru.fit(flat, m, v, t0, states, labels, tab, LR)
    g = Gpu(ops, states, labels, flat, m, v, n_steps=1)
    g.fit(tab, t0)
    p, gm, gv, loss, counts, step_loss = g.state()
    assert g.intact()
    print("S=%d B=%d t0=%d: loss %.9g vs %.9g, err p %.2e m %.2e v %.2e" % (
        S, B, t0, step_loss[0], ph.step_loss[0], per_tensor_err(p, rflat, S), per_tensor_err(gm, rm, S), per_tensor_err(gv, rv, S)))
    assert abs(step_loss[0] - ph.step_loss[0]) <= 1e-5 * abs(ph.step_loss[0])
    assert abs(loss[0] - ph.running_loss) <= 1e-5 * abs(ph.running_loss)
    assert per_tensor_err(p, rflat, S) <= 1e-4
    assert per_tensor_err(gm, rm, S) <= 1e-4
    assert per_tensor_err(gv, rv, S) <= 1e-4
    check_counts(counts, ph)
    # an element whose gradient is exactly zero (and whose moments are) does not move at all
    still = (grads[0] == 0) & (m == 0) & (v == 0)
    assert np.array_equal(p[still], flat[still].astype(np.float32)) and not gm[still].any() and not gv[still].any()
    return int(still.sum())


@pytest.mark.parametrize("B", [1, 2, 8, 32, 33])
@pytest.mark.parametrize("S", [1, 2, 3, 12, 200])
def test_single_step(ops, S, B):
    for t0 in (0, 7):
        single_step(ops, S, B, t0, seed=B)


def test_single_step_second_row_chunk(ops):
    """The smallest minibatch that needs a second row chunk at S = 200."""
    B = ops.reward_probe_chunk_rows(200) + 1
    assert 2 <= B <= 129
    for t0 in (0, 7):
        single_step(ops, 200, B, t0, seed=3)


@pytest.mark.parametrize("S,B", [(3, 8), (200, 32)])
def test_dead_hidden_unit_stays_put(ops, S, B):
    for t0 in (0, 7):
        still = single_step(ops, S, B, t0, dead=True, seed=4)
        assert still >= 2 * S + 1 + 4, "the dead unit's row of W1, its bias and its column of W2 have zero gradient"


def test_edge_rows(ops):
    S, B = 5, 8
    states, labels, flat = problem(S, N=40, seed=7)
    N = len(states)
    labels[:] = 0
    labels[[3, 4, 5]] = 1
    tab = np.array([[N - 2, N - 2, 0, 0, 17, N - 2, 1, 0],      # the last row is read as next_state; repeated indices
                    [3, 4, 5, 3, 4, 5, 3, 4],                   # class 1 only
                    [0, 1, 2, 6, 7, 8, 9, 10]], dtype=np.int64)  # class 0 only
    for row in tab:
        one = row[None]
        assert well_posed(states, labels, flat, one) is None
        rflat, rm, rv, ph, _ = ru.fit(flat, np.zeros_like(flat), np.zeros_like(flat), 0, states, labels, one, LR)
        assert ph.bounds()[2] == 0
        g = Gpu(ops, states, labels, flat, n_steps=1)
        g.fit(one, 0)
        p, gm, gv, loss, counts, step_loss = g.state()
        assert g.intact()
        assert abs(step_loss[0] - ph.step_loss[0]) <= 1e-5 * abs(ph.step_loss[0])
        assert per_tensor_err(p, rflat, S) <= 1e-4 and per_tensor_err(gm, rm, S) <= 1e-4 and per_tensor_err(gv, rv, S) <= 1e-4
        assert np.array_equal(counts, ph.counts()), (counts, ph.counts())
        e = Gpu(ops, states, labels, flat)
        e.eval(one)
        assert np.array_equal(e.state()[4], ph.counts())
    assert np.array_equal(ru.evaluate(flat, states, labels, tab[1:2]).counts()[3:], [0, B])


def test_argmax_tie_goes_to_class_0(ops):
    S, B = 4, 8
    states, labels, flat = problem(S, N=40, seed=8)
    w3, b3 = ru.unflatten(flat, S)[4:]
    w3[1] = w3[0]  # views into flat: both logits are the same number in every row
    b3[1] = b3[0]
    tab = table(len(states), 2, B, seed=9)
    y = labels[tab.reshape(-1)]
    want = np.array([(y == 0).sum(), (y == 0).sum(), 0, (y == 0).sum(), (y == 1).sum()])
    assert 0 < want[3] < 2 * B
    e = Gpu(ops, states, labels, flat)
    e.eval(tab)
    assert np.array_equal(e.state()[4], want)
    g = Gpu(ops, states, labels, flat)
    g.fit(tab[:1], 0, step_loss=False)
    y = labels[tab[0]]
    assert np.array_equal(g.state()[4], [(y == 0).sum(), (y == 0).sum(), 0, (y == 0).sum(), (y == 1).sum()])
    assert abs(g.state()[3][0] - B * np.log(2.0)) <= 1e-5 * B * np.log(2.0)


@pytest.mark.parametrize("S,B,n_steps,cut", [(12, 8, 3, 1), (12, 8, 40, 1), (200, 32, 40, 1), (200, 41, 3, 1), (3, 8, 300, 100)])
def test_multi_step(ops, S, B, n_steps, cut):
    """n steps in one launch = the same steps `cut` at a time, bit for bit (300 steps cross the 256-step table of Adam's scalars, and
    cuts of 100 do not line up with it); two runs agree bit for bit; the statistics follow the float64 trajectory."""
    states, labels, flat = problem(S, N=200, seed=11)
    tab = table(len(states), n_steps, B, seed=12)
    zeros = np.zeros_like(flat)
    _, _, _, ph, _ = ru.fit(flat, zeros, zeros, 0, states, labels, tab, LR)
    runs = []
    for _ in range(2):
        g = Gpu(ops, states, labels, flat, n_steps=n_steps)
        g.fit(tab, 0)
        assert g.intact()
        runs.append(g.state())
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two runs differ"
    g = Gpu(ops, states, labels, flat, n_steps=n_steps)
    for s in range(0, n_steps, cut):
        g.fit(tab[s:s + cut], s, offset=s)
    assert g.intact()
    for name, a, b in zip(("params", "m", "v", "running_loss", "counts", "step_loss"), runs[0], g.state()):
        assert np.array_equal(a, b), "%s depends on how the steps are cut into launches" % name
    p, gm, gv, loss, counts, step_loss = runs[0]
    print("S=%d B=%d n=%d: running_loss %.9g vs %.9g, worst step %.2e" % (
        S, B, n_steps, loss[0], ph.running_loss, np.abs(step_loss / np.array(ph.step_loss) - 1).max()))
    assert abs(loss[0] - ph.running_loss) <= 1e-5 * abs(ph.running_loss)
    check_counts(counts, ph)
    assert counts[3] + counts[4] == n_steps * B


@pytest.mark.parametrize("S,B,n_batches", [(12, 8, 1), (12, 8, 5), (12, 8, 300), (200, 32, 5), (1, 3, 300)])
def test_eval(ops, S, B, n_batches):
    states, labels, flat = problem(S, N=300, seed=13)
    tab = table(len(states), n_batches, B, seed=14)
    ph = ru.evaluate(flat, states, labels, tab)
    runs = []
    for _ in range(2):
        e = Gpu(ops, states, labels, flat, m=flat + 1, v=flat + 2)
        e.eval(tab)
        assert e.intact()
        p, m, v, loss, counts, _ = e.state()
        assert np.array_equal(p, flat.astype(np.float32)), "eval wrote to the parameters"
        runs.append((loss, counts))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    loss, counts = runs[0]
    print("S=%d B=%d n=%d: running_loss %.12g vs %.12g" % (S, B, n_batches, loss[0], ph.running_loss))
    assert abs(loss[0] - ph.running_loss) <= 1e-5 * abs(ph.running_loss)
    check_counts(counts, ph)
    e.eval(tab)  # the statistics are added to
    assert np.array_equal(e.state()[4], 2 * counts)


def test_rejections(ops):
    from srlz._cabi import SrlzError
    S, B = 6, 4
    states, labels, flat = problem(S, N=30, seed=15)
    N = len(states)
    good = table(N, 2, B, seed=16)
    g = Gpu(ops, states, labels, flat, n_steps=2)
    before = g.state()

    def i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))

    def both(check, **kw):
        for call in (lambda: ops.reward_probe_fit(kw.get("data", g.data), kw.get("idx", i32(good)), kw.get("p", g.p), g.m, g.v, 0, LR,
                                                  g.loss, kw.get("counts", g.counts)),
                     lambda: ops.reward_probe_eval(kw.get("data", g.data), kw.get("idx", i32(good)), kw.get("p", g.p), g.loss,
                                                   kw.get("counts", g.counts))):
            with pytest.raises(check):
                call()

    both(ValueError, idx=torch.from_numpy(good))                       # int64 indices
    bad = good.copy()
    bad[1, 2] = N - 1
    both(SrlzError, idx=i32(bad))                                      # row N - 1 has no successor
    bad[1, 2] = -1
    both(SrlzError, idx=i32(bad))
    with pytest.raises(ValueError):                                    # a label of 2
        wrong = labels.copy()
        wrong[5] = 2
        ops.reward_probe_data(states, wrong)
    other = ops.reward_probe_data(np.zeros((N, S + 1), dtype=np.float32), labels)
    both(ValueError, data=other)                                       # S does not match the parameters
    both(ValueError, counts=g.counts[:4])                              # a short output buffer
    with pytest.raises(ValueError):
        ops.reward_probe_fit(g.data, i32(good), g.p, g.m, g.v, 0, LR, g.loss, g.counts, step_loss=g.step_loss[:1])
    with pytest.raises(ValueError):                                    # S beyond what the fit kernel keeps on chip
        ops.reward_probe_data(np.zeros((4, 513), dtype=np.float32), np.zeros(4, dtype=np.int64))
    torch.cuda.synchronize()
    for a, b in zip(before, g.state()):
        assert np.array_equal(a, b), "a rejected call ran a kernel"
    assert g.intact()
