"""srlz_robotic_fwd / srlz_robotic_bwd (csrc/robotic.hip) entry by entry against the float64 restatement of tests/robotic_util.py
(which tests/test_robotic_host_cpu.py holds to the reference's own function called with double tensors).

The bars are the project's own (tests/test_invfit_kernels_gpu.py): every gradient entry within 1e-4 of its tensor's scale (max
|reference|), each of the four terms within 1e-4 relative.  The inputs keep the comparison well conditioned, and the tests assert
that they do: every step at least 1e-2 of the longest (the proportionality gradient divides by it), every squared distance inside a
pair at most 20 (no similarity underflows).  Bit guarantees are asserted as bits.  Every buffer the kernels write has a sentinel tail.

Measured on one MI355X, the operator, worst over the 18 cases (6 shapes x 3 orders of the pair lists): a term 5.0e-07 relative
(B = 3, S = 3), a gradient entry 1.1e-07 of its tensor's scale (B = 256 with one action); with one upstream gradient at a time
2.0e-07 (repeatability alone).  The fit kernel, one step, worst over the 12 cases: a term 4.6e-06 relative (D = 1, S = 1, B = 2), a weight
entry of last_grad 7.0e-07 and a bias entry 1.1e-07 of max |last_grad|, m 6.2e-08, v 1.2e-07, the step through the gradient 2.5e-06;
three steps from non-zero moments: the parameters' movement 7.2e-06, m 2.2e-07, v 1.4e-07, the running terms 1.8e-08; the eval kernel
1.2e-07."""
import numpy as np
import pytest
import torch

import robotic_util as ru

pytestmark = pytest.mark.gpu

BAR = 1e-4
TAIL = 64
SENT = -12345.5
VARIANTS = ("generated", "shuffled", "duplicates_reversed")
CASES = [(c, v) for c in ru.LOSS_CASES for v in range(3)]


def _dev():
    return torch.device("cuda", 0)


def _tailed(n, dtype):
    whole = torch.full((n + TAIL,), SENT, dtype=dtype, device=_dev())
    return whole, whole[:n]


def _tail_ok(whole, n):
    t = whole[n:].cpu()
    return bool((t == SENT).all()) and t.numel() == TAIL


def _conditioned(states, next_states, dis, same):
    s, step = states.astype(np.float64), next_states.astype(np.float64) - states.astype(np.float64)
    length = np.sqrt((step * step).sum(1))
    assert length.min() >= 1e-2 * length.max()
    for p in (dis, same):
        gap = s[p[:, 0]] - s[p[:, 1]]
        assert (gap * gap).sum(1).max() <= 20.0


class Run(object):
    """One forward and one backward launch through the C ABI with sentinel tails behind everything they write."""

    def __init__(self, states, next_states, dis, same, weights=(1.0, 1.0, 1.0, 1.0)):
        from srlz import ops, _cabi as C
        b, s = states.shape
        dev = _dev()
        self.s, self.ns = torch.from_numpy(states).to(dev), torch.from_numpy(next_states).to(dev)
        self.table = ops.robotic_table(dis, same, b, dev)
        self.bufs = {"norms": _tailed(b, torch.float32), "terms": _tailed(4, torch.float64), "terms32": _tailed(4, torch.float32),
                     "ds": _tailed(b * s, torch.float32), "dns": _tailed(b * s, torch.float32)}
        v = {k: w[1] for k, w in self.bufs.items()}
        t = self.table
        g = [torch.tensor(float(w), dtype=torch.float32, device=dev) for w in weights]
        C.robotic_fwd(C.ptr(self.s), C.ptr(self.ns), b, s, C.ptr(t.dis), t.n_dis, C.ptr(t.same), t.n_same, C.ptr(v["norms"]),
                      C.ptr(v["terms"]), C.ptr(v["terms32"]), C.stream())
        C.robotic_bwd(C.ptr(self.s), C.ptr(self.ns), C.ptr(v["norms"]), b, s, C.ptr(t.same_inc), t.n_same, C.ptr(t.dis_inc), t.n_dis,
                      C.ptr(g[0]), C.ptr(g[1]), C.ptr(g[2]), C.ptr(g[3]), C.ptr(v["ds"]), C.ptr(v["dns"]), C.stream())
        torch.cuda.synchronize()
        for k, (whole, view) in self.bufs.items():
            assert _tail_ok(whole, view.numel()), "%s: sentinel tail overwritten" % k
            setattr(self, k, view.cpu().numpy().copy())
        self.ds, self.dns = self.ds.reshape(b, s), self.dns.reshape(b, s)

    def bits(self):
        return {k: getattr(self, k).view(np.uint8).copy() for k in self.bufs}


def _scale_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / float(np.abs(ref).max())


def _compare(run, ref, what):
    terms, ds, dns = ref
    e_term = float((np.abs(run.terms - terms) / np.abs(terms)).max())
    e_32 = float((np.abs(run.terms32.astype(np.float64) - terms) / np.abs(terms)).max())
    e_ds, e_dns = _scale_err(run.ds, ds), _scale_err(run.dns, dns)
    print("%s: terms %.2e (fp32 copy %.2e), dstates %.2e, dnext_states %.2e" % (what, e_term, e_32, e_ds, e_dns))
    assert np.isfinite(run.ds).all() and np.isfinite(run.dns).all() and np.isfinite(run.terms).all()
    assert e_term <= BAR and e_32 <= BAR, (what, e_term, e_32)
    assert e_ds <= BAR and e_dns <= BAR, (what, e_ds, e_dns)
    np.testing.assert_array_equal(run.terms32, run.terms.astype(np.float32))


@pytest.mark.parametrize("case,v", CASES, ids=["%s-%s" % (c["name"], VARIANTS[v]) for c, v in CASES])
def test_loss_and_gradient(case, v):
    states, next_states, dis, same = ru.loss_case(case)
    name, d, p = ru.variants(dis, same, case["seed"])[v]
    assert name == VARIANTS[v]
    _conditioned(states, next_states, d, p)
    run = Run(states, next_states, d, p)
    _compare(run, ru.priors_f64(states, next_states, d, p), "%s %s" % (case["name"], name))
    length = np.sqrt(((next_states.astype(np.float64) - states) ** 2).sum(1))
    assert _scale_err(run.norms, length) <= 1e-6


def test_single_action_incidences():
    """B = 256 with one action: 32 640 same-action pairs, every row in 255 of them."""
    from srlz import ops
    _, _, dis, same = ru.loss_case(ru.LOSS_CASES[-1])
    assert len(same) == 32640
    inc = ops.robotic_incidence(same, 256)
    assert (np.diff(inc[:257]) == 255).all()


def test_upstream_gradients_weight_the_terms():
    """The four upstream gradients are four independent factors."""
    states, next_states, dis, same = ru.loss_case(ru.LOSS_CASES[3])
    for weights in ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.5, -2.0, 3.0, 0.25)):
        run = Run(states, next_states, dis, same, weights)
        _, ds, dns = ru.priors_f64(states, next_states, dis, same, weights)
        e = max(_scale_err(run.ds, ds), _scale_err(run.dns, dns) if np.abs(dns).max() > 0 else float(np.abs(run.dns).max()))
        print("weights %s: %.2e" % (weights, e))
        assert e <= BAR, (weights, e)


def test_zero_step_rows():
    """next_states[b] = states[b] in two rows: every output finite, and those rows receive no proportionality gradient."""
    states, next_states, dis, same = ru.zero_step_case()
    run = Run(states, next_states, dis, same)
    assert (run.norms[list(ru.ZERO_ROWS)] == 0).all()
    _compare(run, ru.priors_f64(states, next_states, dis, same), "zero step")
    only = Run(states, next_states, dis, same, (0.0, 0.0, 1.0, 0.0))
    assert np.isfinite(only.ds).all() and np.isfinite(only.dns).all()
    for b in ru.ZERO_ROWS:
        assert (only.ds[b] == 0).all() and (only.dns[b] == 0).all()
    others = [b for b in range(states.shape[0]) if b not in ru.ZERO_ROWS]
    assert np.abs(only.dns[others]).max() > 0


def test_two_calls_identical_bits():
    states, next_states, dis, same = ru.loss_case(ru.LOSS_CASES[-1])
    _, d, p = ru.variants(dis, same, 3)[2]
    a, b = Run(states, next_states, d, p).bits(), Run(states, next_states, d, p).bits()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_refusals_write_nothing():
    from srlz import _cabi as C, ops
    states, next_states, dis, same = ru.loss_case(ru.LOSS_CASES[2])
    b, s = states.shape
    dev = _dev()
    x, nx = torch.from_numpy(states).to(dev), torch.from_numpy(next_states).to(dev)
    t = ops.robotic_table(dis, same, b, dev)
    whole, out = _tailed(4, torch.float64)
    out.fill_(SENT)
    o32, norms = torch.full((4,), SENT, device=dev), torch.full((b,), SENT, device=dev)
    g = torch.ones((), device=dev)
    ds, dns = torch.full((b, s), SENT, device=dev), torch.full((b, s), SENT, device=dev)

    def fwd(B=b, S=s, n_dis=t.n_dis, n_same=t.n_same, states=x, norms_=norms):
        C.robotic_fwd(C.ptr(states), C.ptr(nx), B, S, C.ptr(t.dis), n_dis, C.ptr(t.same), n_same, C.ptr(norms_), C.ptr(out), C.ptr(o32),
                      C.stream())

    def bwd(B=b, S=s, n_dis=t.n_dis, n_same=t.n_same, g_pr=g):
        C.robotic_bwd(C.ptr(x), C.ptr(nx), C.ptr(norms), B, S, C.ptr(t.same_inc), n_same, C.ptr(t.dis_inc), n_dis, C.ptr(g), C.ptr(g),
                      C.ptr(g_pr), C.ptr(g), C.ptr(ds), C.ptr(dns), C.stream())

    for call in (fwd, bwd):
        for kw in (dict(B=0), dict(S=0), dict(n_dis=0), dict(n_same=0), dict(B=1 << 20, S=1 << 11)):
            with pytest.raises(C.SrlzError):
                call(**kw)
    with pytest.raises(C.SrlzError, match="null"):
        fwd(states=None)
    with pytest.raises(C.SrlzError, match="null"):
        fwd(norms_=None)
    with pytest.raises(C.SrlzError, match="null"):
        bwd(g_pr=None)
    torch.cuda.synchronize()
    for buf in (out, o32, norms, ds, dns):
        assert bool((buf == SENT).all())
    # the host checks of the operator
    with pytest.raises(ValueError, match="empty"):
        ops.robotic_table(np.zeros((0, 2), np.int64), same, b, dev)
    with pytest.raises(ValueError, match="must lie in"):
        ops.robotic_table(dis, np.array([[0, b]]), b, dev)
    with pytest.raises(ValueError, match="built for"):
        ops.RoboticPriorsFn.apply(x[:-1], nx[:-1], t)


# ---------------------------------------------------------------------------------------------------------------- the fit kernels
# srlz_robotic_fit / srlz_robotic_eval against the float64 restatement (robotic_util.map_grad_f64, adam_f64).  The gradient bar is
# the same 1e-4 of the tensor's scale, last_grad [P] being one tensor.  Its bias entries are special: every term depends on
# differences of states alone, so their exact value is 0 and what any implementation returns is the rounding error of sum_b (d states
# + d next_states)[b]; they are held like every other entry, within 1e-4 of max |reference last_grad|.  Moments and the
# step are held through the kernel's own gradient, as tests/test_invfit_kernels_gpu.py holds them and for its reason (Adam's first
# step is lr * sign(g)), with its bars: 2e-6 of scale for m and v, 1e-5 of the step's scale for the step.
N_FRAMES = 64
LR = 0.005


def _largest_d(S, B):
    from srlz import ops
    lo, hi = 1, 1 << 16
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if ops.robotic_supported(mid, S, B) else (lo, mid - 1)
    return lo


FIT_SHAPES = ((1, 1, 2), (5, 3, 16), (17, 2, 33), (200, 3, 32), (200, 8, 256), ("largest", 3, 32))


class Problem(object):
    """Seeded features, a map, n minibatches of B rows in [0, N - 2] (each holds 0, N - 2 and one frame twice where it has room)
    and their pair lists."""

    def __init__(self, D, S, B, n=4, seed=0):
        if D == "largest":
            D = _largest_d(S, B)
        rs = np.random.RandomState(seed + 7 * B + S)
        self.D, self.S, self.B, self.n = D, S, B, n
        self.x = rs.randn(N_FRAMES, D).astype(np.float32)
        self.w = (rs.uniform(-1, 1, (S, D)) / np.sqrt(D)).astype(np.float32)
        self.bias = rs.uniform(-0.5, 0.5, S).astype(np.float32)
        self.flat = np.concatenate((self.w.reshape(-1), self.bias))
        self.rows = rs.randint(0, N_FRAMES - 1, (n, B)).astype(np.int64)
        if B >= 4:
            self.rows[:, 0], self.rows[:, 1], self.rows[:, 3] = 0, N_FRAMES - 2, self.rows[:, 2]
        self.dis, self.same = [], []
        for k in range(n):
            actions, rewards = rs.randint(0, 3, B), rs.randint(0, 2, B)
            same = np.array([[i, j] for i in range(B) for j in range(i + 1, B) if actions[i] == actions[j]] or [[0, B - 1]], np.int64)
            dis = np.array([[i, j] for i, j in same if rewards[i] != rewards[j]] or [same[-1][::-1]], np.int64)
            self.same.append(same)
            self.dis.append(dis)

    def device(self):
        from srlz import ops
        return torch.from_numpy(self.x).to(_dev()), ops.robotic_fit_tables(self.rows, self.dis, self.same, _dev())

    def grad(self, flat, k):
        S, D = self.S, self.D
        return ru.map_grad_f64(flat[:S * D].reshape(S, D), flat[S * D:], self.x, self.rows[k], self.dis[k], self.same[k])


def _tailed_from(values, dtype):
    values = np.asarray(values)
    whole, view = _tailed(values.size, dtype)
    view.copy_(torch.from_numpy(values).to(_dev(), dtype))
    return whole, view


class FitRun(object):
    def __init__(self, x, tabs, order, flat, m=None, v=None, t0=0, running=None, want_grad=True):
        from srlz import ops
        P, n = flat.size, len(order)
        zeros = np.zeros(P, np.float32)
        self.bufs = {"params": _tailed_from(flat, torch.float32), "m": _tailed_from(zeros if m is None else m, torch.float32),
                     "v": _tailed_from(zeros if v is None else v, torch.float32),
                     "running": _tailed_from(np.zeros(4) if running is None else running, torch.float64),
                     "step_terms": _tailed(4 * n, torch.float64), "last_grad": _tailed(P, torch.float32)}
        b = {k: w[1] for k, w in self.bufs.items()}
        ops.robotic_fit(x, tabs, np.asarray(order), b["params"], b["m"], b["v"], t0, LR, b["running"], b["step_terms"],
                        b["last_grad"] if want_grad else None)
        torch.cuda.synchronize()
        for k, (whole, view) in self.bufs.items():
            assert _tail_ok(whole, view.numel()), "%s: sentinel tail overwritten" % k
            setattr(self, k, view.cpu().numpy().copy())
        self.step_terms = self.step_terms.reshape(n, 4)

    def bits(self):
        return {k: getattr(self, k).view(np.uint8).copy() for k in ("params", "m", "v", "running", "step_terms")}


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=["%s-%d-%d" % s for s in FIT_SHAPES])
def test_fit_one_step(shape):
    pb = Problem(*shape)
    S, D = pb.S, pb.D
    x, tabs = pb.device()
    for k in (0, pb.n - 1):
        run = FitRun(x, tabs, [k], pb.flat)
        terms, g = pb.grad(pb.flat, k)
        e_terms = float((np.abs(run.step_terms[0] - terms) / np.abs(terms)).max())
        scale = float(np.abs(g).max())
        err = np.abs(run.last_grad.astype(np.float64) - g) / scale
        e_w, e_b = float(err[:S * D].max()), float(err[S * D:].max())
        np.testing.assert_array_equal(run.running, run.step_terms[0])
        # moments and the step through the kernel's own gradient
        g32 = run.last_grad.astype(np.float64)
        p, m, v = ru.adam_f64(pb.flat.astype(np.float64), g32, np.zeros_like(g32), np.zeros_like(g32), 1, LR)
        e_m = _scale_err(run.m, m) if np.abs(m).max() > 0 else 0.0
        e_v = _scale_err(run.v, v) if np.abs(v).max() > 0 else 0.0
        step = p - pb.flat
        e_step = float(np.abs((run.params.astype(np.float64) - pb.flat) - step).max()) / float(np.abs(step).max())
        print("D=%d S=%d B=%d minibatch %d: terms %.2e, dW %.2e, db %.2e (both of max |last_grad|), m %.2e, v %.2e, step %.2e"
              % (D, S, pb.B, k, e_terms, e_w, e_b, e_m, e_v, e_step))
        assert e_terms <= BAR and e_w <= BAR and e_b <= BAR, (e_terms, e_w, e_b)
        assert e_m <= 2e-6 and e_v <= 2e-6 and e_step <= 1e-5, (e_m, e_v, e_step)


@pytest.mark.parametrize("shape", FIT_SHAPES[1:4], ids=["%s-%d-%d" % s for s in FIT_SHAPES[1:4]])
def test_fit_three_steps_from_moments(shape):
    """Three steps from non-zero moments at t0 = 10 against the float64 trajectory: away from a zero start Adam's step is no sign
    function, so the trajectories can be compared directly."""
    pb = Problem(*shape)
    S, D = pb.S, pb.D
    x, tabs = pb.device()
    rs = np.random.RandomState(3)
    _, g0 = pb.grad(pb.flat, 0)
    gs = float(np.abs(g0).max())
    m0 = (rs.randn(pb.flat.size) * gs).astype(np.float32)
    v0 = (rs.uniform(0.5, 1.5, pb.flat.size) * gs * gs).astype(np.float32)
    order = [2, 0, 1]
    run = FitRun(x, tabs, order, pb.flat, m0, v0, t0=10, running=np.array([1.0, 2.0, 3.0, 4.0]))
    p, m, v = pb.flat.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    total = np.array([1.0, 2.0, 3.0, 4.0])
    for i, k in enumerate(order):
        terms, g = pb.grad(p, k)
        assert float((np.abs(run.step_terms[i] - terms) / np.abs(terms)).max()) <= BAR
        total = total + terms
        p, m, v = ru.adam_f64(p, g, m, v, 11 + i, LR)
    move = p - pb.flat
    e_move = float(np.abs((run.params.astype(np.float64) - pb.flat) - move).max()) / float(np.abs(move).max())
    e_m, e_v = _scale_err(run.m, m), _scale_err(run.v, v)
    e_run = float((np.abs(run.running - total) / total).max())
    print("D=%d S=%d B=%d: movement %.2e, m %.2e, v %.2e, running %.2e" % (D, S, pb.B, e_move, e_m, e_v, e_run))
    assert e_move <= BAR and e_m <= BAR and e_v <= BAR and e_run <= BAR


@pytest.mark.parametrize("shape", (FIT_SHAPES[1], FIT_SHAPES[3]), ids=["5-3-16", "200-3-32"])
def test_fit_n_steps_equal_n_calls_as_bits(shape):
    pb = Problem(*shape)
    x, tabs = pb.device()
    order = [1, 3, 0, 2, 1]
    one = FitRun(x, tabs, order, pb.flat, want_grad=False)
    again = FitRun(x, tabs, order, pb.flat, want_grad=False)
    flat, m, v, running, terms = pb.flat, None, None, None, []
    for i, k in enumerate(order):
        r = FitRun(x, tabs, [k], flat, m, v, t0=i, running=running, want_grad=False)
        flat, m, v, running = r.params, r.m, r.v, r.running
        terms.append(r.step_terms[0])
    a, b = one.bits(), again.bits()
    for key in a:
        assert np.array_equal(a[key], b[key]), "two calls: " + key
    assert np.array_equal(one.params.view(np.uint8), flat.view(np.uint8))
    assert np.array_equal(one.m.view(np.uint8), m.view(np.uint8)) and np.array_equal(one.v.view(np.uint8), v.view(np.uint8))
    assert np.array_equal(one.running.view(np.uint8), running.view(np.uint8))
    assert np.array_equal(one.step_terms.view(np.uint8), np.stack(terms).view(np.uint8))
    assert (one.last_grad == np.float32(SENT)).all()


@pytest.mark.parametrize("shape", (FIT_SHAPES[0], FIT_SHAPES[2], FIT_SHAPES[4]), ids=["1-1-2", "17-2-33", "200-8-256"])
def test_eval_against_restatement_and_any_grid(shape):
    from srlz import ops
    pb = Problem(*shape, n=5)
    x, tabs = pb.device()
    params = torch.from_numpy(pb.flat).to(_dev())
    order = [4, 0, 2, 2, 1]
    whole, running = _tailed_from(np.array([0.5, 0.0, 0.0, 0.25]), torch.float64)
    ops.robotic_eval(x, tabs, order, params, running)
    torch.cuda.synchronize()
    assert _tail_ok(whole, 4)
    got = running.cpu().numpy()
    ref = np.array([0.5, 0.0, 0.0, 0.25]) + sum(pb.grad(pb.flat, k)[0] for k in order)
    err = float((np.abs(got - ref) / ref).max())
    print("D=%d S=%d B=%d eval: %.2e" % (pb.D, pb.S, pb.B, err))
    assert err <= BAR
    # one workgroup per call, five calls: the same additions in the same order
    _, single = _tailed_from(np.array([0.5, 0.0, 0.0, 0.25]), torch.float64)
    for k in order:
        ops.robotic_eval(x, tabs, [k], params, single)
    torch.cuda.synchronize()
    assert np.array_equal(single.cpu().numpy().view(np.uint8), got.view(np.uint8))
    assert torch.equal(params.cpu(), torch.from_numpy(pb.flat))


def test_fit_refusals_write_nothing():
    from srlz import ops, _cabi as C
    pb = Problem(5, 3, 16)
    x, tabs = pb.device()
    dev = _dev()
    P = pb.flat.size
    bufs = [torch.full((P,), SENT, device=dev) for _ in range(3)] + [torch.full((4,), SENT, dtype=torch.float64, device=dev)]
    params, m, v, running = bufs
    ws = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="srlz_robotic_supported"):   # an unsupported shape: B = 16 with D far beyond the LDS budget
        ops.robotic_fit(torch.zeros((N_FRAMES, 20000), device=dev), tabs, [0], torch.zeros(3 * 20001, device=dev),
                        torch.zeros(3 * 20001, device=dev), torch.zeros(3 * 20001, device=dev), 0, LR, running)
    bad = ops.robotic_fit_tables(np.where(pb.rows == 0, N_FRAMES - 1, pb.rows), pb.dis, pb.same, dev)  # a frame without a successor
    for call in (lambda: ops.robotic_fit(x, bad, [0], params, m, v, 0, LR, running),
                 lambda: ops.robotic_eval(x, bad, [0], params, running),
                 lambda: ops.robotic_fit(x, tabs, [pb.n], params, m, v, 0, LR, running),
                 lambda: ops.robotic_eval(x, tabs, [-1], params, running)):
        with pytest.raises(C.SrlzError, match="outside"):
            call()
    with pytest.raises(ValueError, match="workspace"):
        ops.robotic_eval(x, tabs, [0, 1, 2], params, running, workspace=ws)
    order = ops.robotic_order([0], dev)
    args = lambda **kw: [kw.get("x", C.ptr(x)), N_FRAMES, pb.D, pb.S, C.ptr(tabs.idx.device), tabs.idx.host_ptr(), tabs.n, tabs.batch,
                         C.ptr(tabs.tables.device), int(tabs.tables.host.numel()), C.ptr(tabs.dir.device), tabs.dir.host_ptr(),
                         C.ptr(order.device), order.host_ptr(), 1]
    with pytest.raises(C.SrlzError, match="null"):
        C.robotic_fit(*(args(x=None) + [C.ptr(params), C.ptr(m), C.ptr(v), 0, LR, 0.9, 0.999, 1e-8, C.ptr(running), None, None, C.stream()]))
    with pytest.raises(C.SrlzError, match="null"):
        C.robotic_fit(*(args() + [C.ptr(params), None, C.ptr(v), 0, LR, 0.9, 0.999, 1e-8, C.ptr(running), None, None, C.stream()]))
    huge = lambda: [C.ptr(x), N_FRAMES, 20000, pb.S] + args()[4:]  # (refused before any pointer is followed)
    with pytest.raises(C.SrlzError, match="srlz_robotic_supported"):
        C.robotic_fit(*(huge() + [C.ptr(params), C.ptr(m), C.ptr(v), 0, LR, 0.9, 0.999, 1e-8, C.ptr(running), None, None, C.stream()]))
    with pytest.raises(C.SrlzError, match="srlz_robotic_supported"):
        C.robotic_eval(*(huge() + [C.ptr(params), C.ptr(running), C.ptr(ws), 64, C.ptr(torch.zeros(1, dtype=torch.int32, device=dev)),
                                   C.stream()]))
    with pytest.raises(C.SrlzError, match="workspace"):
        C.robotic_eval(*(args() + [C.ptr(params), C.ptr(running), C.ptr(ws), 8, C.ptr(torch.zeros(1, dtype=torch.int32, device=dev)),
                                   C.stream()]))
    with pytest.raises(C.SrlzError):
        C.robotic_fit(*(args() + [C.ptr(params), C.ptr(m), C.ptr(v), -1, LR, 0.9, 0.999, 1e-8, C.ptr(running), None, None, C.stream()]))
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == SENT).all())
    assert bool((ws == 7).all())
