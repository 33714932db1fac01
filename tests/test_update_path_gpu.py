"""The update path kernel by kernel (GPU): everything between "every layer has written its gradient" and "the next step's weights" —
the fold of the staged gradients, Adam with the host and the device step counter, the BatchNorm replay, the composition of the loss
terms, the gradient fan-in, the joins and splits and the loss reductions — each C entry point called by name, against a plain CPU
reference of the same operation.

References: fp64 torch / numpy for arithmetic (torch.optim.Adam on a float64 copy for Adam); where a kernel promises a fixed order of
separately rounded fp32 operations, or is a pure copy, numpy float32 evaluated in exactly that order, compared bit for bit (NaNs
position for position; +0.0 and -0.0 are different).  Every output buffer carries a tail of GUARD NaN floats that must come back
untouched.  The searches for inputs that tell two orders of evaluation apart run on the CPU, in plain functions, and have an unmarked
test of their own."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from test_kernels_gpu import C, DEV, rel_err  # noqa: F401  (C: the module-scoped fixture of the kernel tests)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
GUARD = 64  # sentinel floats behind every output buffer
INT_SENTINEL = -12345
LR, EPS = 5e-3, 1e-8


def gpu(fn):
    """A test that needs the MI355X: marked `gpu`, and skipped (not failed) where no GPU is visible."""
    return pytest.mark.gpu(pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")(fn))


def header_constant(name):
    with open(os.path.join(REPO, "include", "srlz.h")) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, f.read(), re.M)
    assert m, "include/srlz.h does not define %s" % name
    return int(m.group(1))


# ---- buffers with a sentinel tail ---------------------------------------------------------------------------------------------
def guarded(src):
    """Device copy of a CPU tensor with GUARD sentinels behind it: (whole buffer, view of the payload in src's shape)."""
    n = src.numel()
    fill = NAN if src.is_floating_point() else INT_SENTINEL
    whole = torch.full((n + GUARD,), fill, dtype=src.dtype, device=DEV)
    whole[:n].copy_(src.reshape(-1))
    return whole, whole[:n].view(src.shape)


def nan_out(*shape):
    """An output buffer of NaNs with its tail: (whole, view)."""
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), NAN, device=DEV)
    return whole, whole[:n].view(shape)


def tail_intact(whole, n):
    t = whole[n:].cpu()
    return bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == INT_SENTINEL).all())


def all_nan(t):
    return bool(torch.isnan(t).all())


def same_bits(got, want):
    """fp32 tensors equal bit for bit; NaNs have to sit at the same positions (their payloads may differ between processors)."""
    got = got.detach().cpu().contiguous().reshape(-1)
    want = (torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want.detach().cpu()).contiguous().reshape(-1)
    assert got.dtype == torch.float32 and want.dtype == torch.float32
    if got.shape != want.shape:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(got.view(torch.int32)[~gn], want.view(torch.int32)[~wn])


def raises_srlz(C, fn, *args):
    with pytest.raises(C.SrlzError):
        fn(*args)
    torch.cuda.synchronize()


# ---- CPU-side searches for inputs that tell two orders of evaluation apart ----------------------------------------------------
def weighted_total_orders(w, l):
    """sum_i w_i * l_i three ways: (fp32 left to right with separately rounded products — what the kernel promises, fp32 left to
    right with fused multiply-adds, the exactly rounded sum of the exact products)."""
    sep, fma = np.float32(0), np.float32(0)
    for wi, li in zip(w, l):
        sep = np.float32(sep + np.float32(wi * li))
        fma = np.float32(np.float64(wi) * np.float64(li) + np.float64(fma))  # (the product of two fp32 is exact in fp64)
    exact = np.float32(math.fsum(float(wi) * float(li) for wi, li in zip(w, l)))
    return sep, fma, exact


def find_weighted_total_case(n, seed):
    """n fp32 weights and losses whose separately rounded left-to-right sum differs from the fused and from the exact one (n >= 2; a
    single term has one rounding whichever way it is evaluated)."""
    rs = np.random.RandomState(seed)
    for _ in range(10000):
        w = rs.uniform(0.1, 3.0, n).astype(np.float32)
        l = (rs.standard_normal(n) * rs.choice([1e-3, 1.0, 30.0], n)).astype(np.float32)
        sep, fma, exact = weighted_total_orders(w, l)
        if n == 1 or (sep != fma and sep != exact):
            return w, l
    raise AssertionError("no discriminating set of %d terms" % n)


def scale_orders(c, div, coef):
    """(c / div) * coef — what the kernel promises — and (c * coef) / div, both with every operation rounded to fp32."""
    c, div, coef = np.float32(c), np.float32(div), np.float32(coef)
    return np.float32(np.float32(c / div) * coef), np.float32(np.float32(c * coef) / div)


def find_scale_order_cases(count, seed, div, coef):
    """`count` upstream values c for which (c / div) * coef and (c * coef) / div round differently."""
    rs = np.random.RandomState(seed)
    found = []
    for _ in range(10000):
        c = np.float32(rs.uniform(0.1, 2.0))
        a, b = scale_orders(c, div, coef)
        if a != b:
            found.append(c)
            if len(found) == count:
                return np.array(found, dtype=np.float32)
    raise AssertionError("no %d discriminating values for div %r, coef %r" % (count, div, coef))


def adam_formula(p, g, m, v, lr, b1, b2, eps, t):
    """One update of torch.optim.Adam (no amsgrad, no weight decay) written out, on fp64 tensors."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


LONG_STEPS = 40


@functools.lru_cache(maxsize=None)
def adam_long_run(n):
    """LONG_STEPS steps of torch.optim.Adam on the CPU from one seeded sequence of fp32 gradients, in float64 (the oracle) and in
    float32 (whose distance from the oracle sets the bound for the kernel): (p0, grads [steps, n], {dtype: (p, m, v)})."""
    g = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=g)
    grads = torch.randn(LONG_STEPS, n, generator=g) * 0.1
    grads[:, torch.arange(n) % 5 == 2] = 0.0
    out = {}
    for dtype in (torch.float64, torch.float32):
        pr = p0.to(dtype).clone().requires_grad_(True)
        opt = torch.optim.Adam([pr], lr=LR)
        for s in range(LONG_STEPS):
            pr.grad = grads[s].to(dtype)
            opt.step()
        st = opt.state[pr]
        out[dtype] = (pr.detach(), st["exp_avg"], st["exp_avg_sq"])
    return p0, grads, out


def adam_long_bounds(n):
    """4 x the error of the fp32 CPU run against the fp64 run, for p, m and v (the kernel may contract multiply-adds the CPU does not)."""
    _, _, out = adam_long_run(n)
    errs = [rel_err(a, b) for a, b in zip(out[torch.float32], out[torch.float64])]
    assert all(e > 0 for e in errs)
    return errs, [4 * e for e in errs]


LONG_N = [10007, 2048 * 256 + 13]


def test_cpu_searches_find_discriminating_inputs():
    """The inputs the exact comparisons below rest on exist (no GPU needed): sets of loss terms whose three orders of evaluation
    differ, upstream scalars for which (c / div) * coef is not (c * coef) / div, and a non-zero fp32-vs-fp64 Adam error to take the
    long run's bound from."""
    for n in (2, 5, header_constant("SRLZ_MAX_LOSS_TERMS")):
        w, l = find_weighted_total_case(n, seed=n)
        sep, fma, exact = weighted_total_orders(w, l)
        assert sep != fma and sep != exact
    w, l = find_weighted_total_case(1, seed=1)
    assert w.shape == (1,) and l.shape == (1,)
    div, coef = np.float32(3 * 224 * 224), np.float32(-1.7)
    cs = find_scale_order_cases(8, 7, div, coef)
    assert len(set(cs.tolist())) == 8
    for c in cs:
        a, b = scale_orders(c, div, coef)
        assert a != b
    errs, bounds = adam_long_bounds(LONG_N[0])
    print("fp32 vs fp64 torch Adam after %d steps, n = %d: p %.3e m %.3e v %.3e" % ((LONG_STEPS, LONG_N[0]) + tuple(errs)))
    assert all(0 < e < 1e-5 for e in errs) and bounds == [4 * e for e in errs]


# ---- 1. fold_grads --------------------------------------------------------------------------------------------------------------
FOLD_BIG = 4 * 2048 * 256 + 4  # a second pass of the grid-stride loop whose only element is the bucket's last float4


def fold_inputs(n, nstage):
    g = torch.Generator().manual_seed(n + nstage)
    grad = torch.randn(n, generator=g).numpy()
    st = torch.randn(nstage, n, generator=g).numpy()
    # element 0: only negative zeros (-0.0 stays -0.0); 1: denormals; 2: an inf; 3: inf - inf (NaN) when a second stage exists
    grad[0], st[:, 0] = -0.0, -0.0
    grad[1], st[:, 1] = 1e-39, 0.0
    st[0, 1] = 1e-40
    st[0, 2] = float("inf")
    st[0, 3] = float("inf")
    if nstage > 1:
        st[1, 3] = -float("inf")
    return grad, st


def fold_reference(grad, st):
    out = grad.copy()
    with np.errstate(all="ignore"):
        for k in range(st.shape[0]):
            out = out + st[k]  # fp32 + fp32, rounded once: ((g + s0) + s1) + ...
    assert out.dtype == np.float32
    return out


@gpu
@pytest.mark.parametrize("nstage", [1, 3, 8])
@pytest.mark.parametrize("n", [4, 8, 1028, FOLD_BIG])
def test_fold_grads_is_the_left_to_right_fp32_sum_and_clears_the_stages(C, n, nstage):
    grad, st = fold_inputs(n, nstage)
    ref = fold_reference(grad, st)
    assert np.signbit(ref[0]) and ref[0] == 0 and 0 < ref[1] < 1.2e-38 and np.isinf(ref[2])
    assert np.isnan(ref[3]) == (nstage > 1)
    gw, gd = guarded(torch.from_numpy(grad))
    sw, sd = guarded(torch.from_numpy(st))
    C.fold_grads(C.ptr(gd), C.ptr(sd), n, nstage, C.stream())
    torch.cuda.synchronize()
    assert same_bits(gd, ref)
    assert bool((sd.view(torch.int32) == 0).all())  # every stage is +0.0 throughout
    assert tail_intact(gw, n) and tail_intact(sw, nstage * n)


@gpu
@pytest.mark.parametrize("n,nstage", [(6, 3), (8, 0), (8, 9)])
def test_fold_grads_rejects_bad_sizes_without_touching_the_buffers(C, n, nstage):
    gw, gd = nan_out(n)
    sw, sd = nan_out(9, n)
    raises_srlz(C, C.fold_grads, C.ptr(gd), C.ptr(sd), n, nstage, C.stream())
    assert all_nan(gw) and all_nan(sw)


class _Three(torch.nn.Module):
    """Three parameters whose sizes (5, 7, 10) are no multiples of FlatParams.ALIGN: the flat buffers have padding floats."""

    def __init__(self):
        super(_Three, self).__init__()
        g = torch.Generator().manual_seed(4)
        self.a = torch.nn.Parameter(torch.randn(5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(7, generator=g))
        self.c = torch.nn.Parameter(torch.randn(2, 5, generator=g))


def _padding_mask(flat):
    pad = torch.ones(flat.flat.numel(), dtype=torch.bool)
    for p, off in zip(flat.params, flat.offsets):
        pad[off:off + p.numel()] = False
    return pad


@gpu
def test_flat_params_deliver_discard_and_zero_grad(C):
    from srlz import optim
    flat = optim.FlatParams(_Three().to(DEV))
    assert flat.offsets == [0, 8, 16] and flat.flat.numel() == 28 and flat.stage.shape == (flat.NSTAGE, 28)
    pad = _padding_mask(flat)
    assert int(pad.sum()) == 6
    g = torch.Generator().manual_seed(12)

    def stage_two_contributions():
        vals = []
        for i, p in enumerate(flat.params):
            pair = [torch.randn(p.shape, generator=g) for _ in range(2)]
            for v in pair:
                flat.grad_buffer(i).copy_(v)
            vals.append(pair)
        return vals

    start = [torch.randn(p.shape, generator=g) for p in flat.params]  # a non-zero gradient to fold into
    for p, s in zip(flat.params, start):
        p.grad.copy_(s)
    vals = stage_two_contributions()
    assert float(flat.stage[:2].abs().sum()) > 0
    flat.deliver()
    torch.cuda.synchronize()
    want = [(s.numpy() + a.numpy()) + b.numpy() for s, (a, b) in zip(start, vals)]
    for p, w in zip(flat.params, want):
        assert same_bits(p.grad, w)
    assert bool((flat.grad.cpu()[pad].view(torch.int32) == 0).all())
    assert bool((flat.stage.view(torch.int32) == 0).all())
    flat.deliver()  # nothing staged: nothing changes
    torch.cuda.synchronize()
    for p, w in zip(flat.params, want):
        assert same_bits(p.grad, w)
    assert bool((flat.stage.view(torch.int32) == 0).all())
    # discard(): the staged contributions go, the gradient stays
    flat.zero_grad()
    for p, s in zip(flat.params, start):
        p.grad.copy_(s)
    stage_two_contributions()
    flat.discard()
    flat.deliver()
    torch.cuda.synchronize()
    for p, s in zip(flat.params, start):
        assert same_bits(p.grad, s)
    assert bool((flat.stage.view(torch.int32) == 0).all()) and bool((flat.grad.cpu()[pad].view(torch.int32) == 0).all())
    # zero_grad(): gradient and stages are zero, the next pass starts at stage 0 again, p.grad still views the bucket
    flat.zero_grad()
    for p, s in zip(flat.params, start):
        p.grad.copy_(s)
    stage_two_contributions()
    flat.zero_grad()
    torch.cuda.synchronize()
    assert bool((flat.bucket[:28].view(torch.int32) == 0).all()) and bool((flat.stage.view(torch.int32) == 0).all())
    for i, (p, off) in enumerate(zip(flat.params, flat.offsets)):
        assert p.grad.data_ptr() == flat.grad.data_ptr() + 4 * off
        assert flat.grad_buffer(i).data_ptr() == flat.stage.data_ptr() + 4 * off
    flat.deliver()
    torch.cuda.synchronize()
    assert bool((flat.grad.view(torch.int32) == 0).all())


# ---- 2. Adam ----------------------------------------------------------------------------------------------------------------
def _zero_grad_elements(n):
    return torch.arange(n) % 5 == 2  # elements whose gradient is exactly 0 in every step


def _adam(C, p, g, m, v, n, step, scale, betas=(0.9, 0.999)):
    C.adam_step(C.ptr(p), C.ptr(g), C.ptr(m), C.ptr(v), n, LR, betas[0], betas[1], EPS, step, scale, C.stream())


ADAM_CASES = [(1, 0.25, (0.9, 0.999)), (3, 0.125, (0.9, 0.999)), (257, 0.25, (0.5, 0.9)), (10007, 0.125, (0.9, 0.999)),
              (2048 * 256 + 13, 0.25, (0.9, 0.999))]  # the last one: a grid-stride pass with a ragged end


@gpu
@pytest.mark.parametrize("n,scale,betas", ADAM_CASES)
def test_adam_step_steps_1_to_3_against_fp64_torch(C, n, scale, betas):
    g = torch.Generator().manual_seed(33 + n)
    p0 = torch.randn(n, generator=g)
    zero = _zero_grad_elements(n)
    pr = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=LR, betas=betas, eps=EPS)
    (pw, p), (mw, m), (vw, v) = guarded(p0), guarded(torch.zeros(n)), guarded(torch.zeros(n))
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * (10.0 ** -step)
        gr[zero] = 0.0
        pr.grad = gr.double()
        opt.step()
        gw, gd = guarded(gr / scale)  # x 4 or x 8: exact, so the oracle sees the numbers the kernel sees
        _adam(C, p, gd, m, v, n, step, scale, betas)
        torch.cuda.synchronize()
        assert tail_intact(gw, n) and torch.equal(gd.cpu(), gr / scale)
    st = opt.state[pr]
    assert rel_err(p, pr) < 1e-6
    assert rel_err(m, st["exp_avg"]) < 5e-7 and rel_err(v, st["exp_avg_sq"]) < 5e-7
    assert tail_intact(pw, n) and tail_intact(mw, n) and tail_intact(vw, n)
    if bool(zero.any()):  # no gradient ever: moments exactly zero, the parameter bit for bit where it was
        assert bool((m.cpu()[zero].view(torch.int32) == 0).all()) and bool((v.cpu()[zero].view(torch.int32) == 0).all())
        assert same_bits(p.cpu()[zero], p0[zero])


@gpu
@pytest.mark.parametrize("n", LONG_N)
def test_adam_step_40_steps_within_4x_the_fp32_reference_error(C, n):
    p0, grads, out = adam_long_run(n)
    errs, bounds = adam_long_bounds(n)
    p64, m64, v64 = out[torch.float64]
    (pw, p), (mw, m), (vw, v) = guarded(p0), guarded(torch.zeros(n)), guarded(torch.zeros(n))
    gd = (grads * 8).to(DEV)
    for s in range(LONG_STEPS):
        _adam(C, p, gd[s], m, v, n, s + 1, 0.125)
    torch.cuda.synchronize()
    got = [rel_err(p, p64), rel_err(m, m64), rel_err(v, v64)]
    print("adam %d steps n=%d: fp32 torch vs fp64 p %.3e m %.3e v %.3e; kernel vs fp64 p %.3e m %.3e v %.3e"
          % ((LONG_STEPS, n) + tuple(errs) + tuple(got)))
    # Measured on the CPU, torch.optim.Adam in fp32 against fp64 after 40 steps (rel_err = max |diff| / max |ref|):
    #   n = 10007:  p 3.562e-07, m 1.107e-07, v 5.131e-07   ->  bounds (4 x) p 1.425e-06, m 4.429e-07, v 2.052e-06
    #   n = 524301: p 4.100e-07, m 1.293e-07, v 6.309e-07   ->  bounds (4 x) p 1.640e-06, m 5.171e-07, v 2.524e-06
    # The bounds are recomputed here from the same two CPU runs, so they follow the reference, never the kernel.
    assert got[0] <= bounds[0] and got[1] <= bounds[1] and got[2] <= bounds[2], (got, bounds)
    zero = _zero_grad_elements(n)
    assert bool((m.cpu()[zero].view(torch.int32) == 0).all()) and bool((v.cpu()[zero].view(torch.int32) == 0).all())
    assert same_bits(p.cpu()[zero], p0[zero])
    assert tail_intact(pw, n) and tail_intact(mw, n) and tail_intact(vw, n)


@gpu
def test_adam_step_at_steps_1000_and_100000_and_rejects_step_0(C):
    """Single updates where 1 - beta^t rounds towards 1, from the moments of a three-step warm-up, against the formula in fp64."""
    n = 10007
    g = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=g)
    (pw, p), (mw, m), (vw, v) = guarded(p0), guarded(torch.zeros(n)), guarded(torch.zeros(n))
    for step in range(1, 4):
        gd = (torch.randn(n, generator=g) * 0.1).to(DEV)
        _adam(C, p, gd, m, v, n, step, 1.0)
    torch.cuda.synchronize()
    warm = [t.cpu().clone() for t in (p, m, v)]
    gr = torch.randn(n, generator=g) * 0.1
    gd = gr.to(DEV)
    for t in (1000, 100000):
        bufs = [guarded(w) for w in warm]
        (pw2, p2), (mw2, m2), (vw2, v2) = bufs
        _adam(C, p2, gd, m2, v2, n, t, 1.0)
        torch.cuda.synchronize()
        pe, me, ve = adam_formula(warm[0].double(), gr.double(), warm[1].double(), warm[2].double(), LR, 0.9, 0.999, EPS, t)
        assert rel_err(p2, pe) < 1e-6 and rel_err(m2, me) < 5e-7 and rel_err(v2, ve) < 5e-7, t
        assert all(tail_intact(w, n) for w, _ in bufs)
    assert 1 - 0.9 ** 100000 == 1.0 and 1 - 0.999 ** 100000 == 1.0
    with pytest.raises(C.SrlzError):
        _adam(C, p, gd, m, v, n, 0, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), b) for a, b in zip((p, m, v), warm))


@gpu
@pytest.mark.parametrize("n", [3, 2048 * 256 + 13])
@pytest.mark.parametrize("start", [0, 999])
def test_adam_step_dev_counts_on_the_device(C, n, start):
    b1, b2, k = 0.9, 0.999, 3
    g = torch.Generator().manual_seed(n + start)
    p0 = torch.randn(n, generator=g)
    grads = torch.randn(k, n, generator=g) * 0.1
    grads[:, _zero_grad_elements(n)] = 0.0
    gd = (grads * 4).to(DEV)
    dev = [guarded(p0), guarded(torch.zeros(n)), guarded(torch.zeros(n))]
    host = [guarded(p0), guarded(torch.zeros(n)), guarded(torch.zeros(n))]
    tw, t_dev = guarded(torch.tensor([start], dtype=torch.int32))
    bw, bc = nan_out(2)
    pe, me, ve = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for i in range(k):
        t = start + i + 1
        C.adam_step_dev(C.ptr(dev[0][1]), C.ptr(gd[i]), C.ptr(dev[1][1]), C.ptr(dev[2][1]), n, LR, b1, b2, EPS, C.ptr(t_dev), C.ptr(bc),
                        0.25, C.stream())
        _adam(C, host[0][1], gd[i], host[1][1], host[2][1], n, t, 0.25)
        torch.cuda.synchronize()
        assert int(t_dev.item()) == t
        for got, want in ((float(bc[0]), LR / (1 - b1 ** t)), (float(bc[1]), math.sqrt(1 - b2 ** t))):
            assert abs(got - want) <= float(np.spacing(np.float32(want))), (t, got, want)  # one fp32 ulp
        pe, me, ve = adam_formula(pe, grads[i].double(), me, ve, LR, b1, b2, EPS, t)
    # the moments do not depend on the step scalars: bit for bit those of adam_step with the same step numbers
    assert same_bits(dev[1][1], host[1][1].cpu()) and same_bits(dev[2][1], host[2][1].cpu())
    assert rel_err(dev[0][1], pe) < 1e-6 and rel_err(dev[1][1], me) < 5e-7 and rel_err(dev[2][1], ve) < 5e-7
    assert rel_err(host[0][1], pe) < 1e-6
    assert all(tail_intact(w, n) for w, _ in dev + host) and tail_intact(tw, 1) and tail_intact(bw, 2)


@gpu
def test_fused_adam_switches_to_the_device_counter_mid_run(C):
    """Two host-counted steps, use_device_step(), three more: the same parameters and moments as five host-counted steps."""
    from srlz import optim
    g = torch.Generator().manual_seed(8)
    grads = [[torch.randn(s, generator=g) * 0.1 for s in ((5,), (7,), (2, 5))] for _ in range(5)]
    runs = []
    for switch_at in (None, 2):
        flat = optim.FlatParams(_Three().to(DEV))
        adam = optim.FusedAdam(flat, LR)
        for s in range(5):
            if s == switch_at:
                adam.use_device_step()
            adam.zero_grad()
            for p, gi in zip(flat.params, grads[s]):
                p.grad.copy_(gi)
            adam.step()
        torch.cuda.synchronize()
        assert adam.steps() == 5 and adam.device_step == (switch_at is not None)
        runs.append((flat.flat.cpu(), adam.m.cpu(), adam.v.cpu()))
    (p_h, m_h, v_h), (p_d, m_d, v_d) = runs
    assert rel_err(p_d, p_h) < 1e-6 and rel_err(m_d, m_h) < 5e-7 and rel_err(v_d, v_h) < 5e-7
    # and the host-counted run is torch.optim.Adam's in fp64
    ref = _Three().double()
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    for s in range(5):
        for p, gi in zip(ref.parameters(), grads[s]):
            p.grad = gi.double()
        opt.step()
    for (p, off), r in zip(zip(flat.params, flat.offsets), ref.parameters()):
        assert rel_err(p_h[off:off + p.numel()], r.reshape(-1)) < 1e-6
        assert rel_err(m_h[off:off + p.numel()], opt.state[r]["exp_avg"].reshape(-1)) < 5e-7
        assert rel_err(v_h[off:off + p.numel()], opt.state[r]["exp_avg_sq"].reshape(-1)) < 5e-7
    pad = _padding_mask(flat)
    assert bool((p_d[pad] == 0).all()) and bool((m_d[pad] == 0).all()) and bool((v_d[pad] == 0).all())


# ---- 3. bn_replay / bn_replay_many ----------------------------------------------------------------------------------------------
def _replay_setup(layers, seed):
    """`layers` BatchNorm layers between two layers that no launch may touch: running statistics [layers + 2, 64] with NaN rows at
    both ends, counters [layers + 2] with sentinels at both ends, one batch_stat[128] per layer."""
    g = torch.Generator().manual_seed(seed)
    stat = torch.randn(layers, 128, generator=g).abs() + 0.1
    rm, rv = torch.randn(layers + 2, 64, generator=g), torch.rand(layers + 2, 64, generator=g) + 0.5
    rm[0], rm[-1], rv[0], rv[-1] = NAN, NAN, NAN, NAN
    ticks = torch.arange(layers + 2, dtype=torch.int64) * 10 + 3
    ticks[0], ticks[-1] = INT_SENTINEL, INT_SENTINEL
    return stat, rm, rv, ticks


def _replay_table(C, stat, rm, rv, ticks, layers, no_tick=()):
    table = (C.BnReplayItem * max(layers, 1))()
    for i in range(layers):
        table[i].batch_stat, table[i].running_mean, table[i].running_var = stat[i].data_ptr(), rm[i + 1].data_ptr(), rv[i + 1].data_ptr()
        table[i].num_batches_tracked = None if i in no_tick else ticks[i + 1:i + 2].data_ptr()
    return table


@gpu
@pytest.mark.parametrize("layers", [1, 3, 8])
def test_bn_replay_many_updates_each_layer_once(C, layers):
    assert layers <= header_constant("SRLZ_BN_REPLAY_MAX")
    stat, rm, rv, ticks = _replay_setup(layers, layers)
    sd, rmd, rvd, td = stat.to(DEV), rm.to(DEV), rv.to(DEV), ticks.to(DEV)
    C.bn_replay_many(_replay_table(C, sd, rmd, rvd, td, layers), layers, 0.1, C.stream())
    # the same layers one by one through srlz_bn_replay
    rm1, rv1 = rm.to(DEV), rv.to(DEV)
    for i in range(layers):
        C.bn_replay(C.ptr(sd[i]), 0.1, C.ptr(rm1[i + 1]), C.ptr(rv1[i + 1]), C.stream())
    torch.cuda.synchronize()
    for i in range(layers):
        assert rel_err(rmd[i + 1], 0.9 * rm[i + 1].double() + 0.1 * stat[i, :64].double()) < 1e-6
        assert rel_err(rvd[i + 1], 0.9 * rv[i + 1].double() + 0.1 * stat[i, 64:].double()) < 1e-6
    assert same_bits(rmd[1:-1], rm1[1:-1].cpu()) and same_bits(rvd[1:-1], rv1[1:-1].cpu())
    want = ticks.clone()
    want[1:-1] += 1
    assert torch.equal(td.cpu(), want)
    for t in (rmd, rvd, rm1, rv1):  # the layers that are not in the table
        assert all_nan(t[0]) and all_nan(t[-1])
    assert torch.equal(sd.cpu(), stat)


@gpu
def test_bn_replay_many_without_a_counter_through_ops_and_its_limit(C):
    from srlz import ops
    limit = header_constant("SRLZ_BN_REPLAY_MAX")
    layers = 3
    stat, rm, rv, ticks = _replay_setup(layers, 21)
    sd, rmd, rvd, td = stat.to(DEV), rm.to(DEV), rv.to(DEV), ticks.to(DEV)
    # one item, tick = NULL: its statistics move, no counter does
    C.bn_replay_many(_replay_table(C, sd[1:], rmd[1:], rvd[1:], td[1:], 1, no_tick=(0,)), 1, 0.1, C.stream())
    torch.cuda.synchronize()
    assert torch.equal(td.cpu(), ticks)
    assert rel_err(rmd[2], 0.9 * rm[2].double() + 0.1 * stat[1, :64].double()) < 1e-6
    assert rel_err(rvd[2], 0.9 * rv[2].double() + 0.1 * stat[1, 64:].double()) < 1e-6
    for i in (1, 3):
        assert torch.equal(rmd[i].cpu(), rm[i]) and torch.equal(rvd[i].cpu(), rv[i])
    assert all_nan(rmd[0]) and all_nan(rmd[-1]) and all_nan(rvd[0]) and all_nan(rvd[-1])
    # the wrapper: three layers, the middle one without a counter
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    items = [(sd[i], rmd[i + 1], rvd[i + 1], None if i == 1 else td[i + 1:i + 2]) for i in range(layers)]
    ops.bn_replay_many(items)
    torch.cuda.synchronize()
    for i in range(layers):
        assert rel_err(rmd[i + 1], 0.9 * rm[i + 1].double() + 0.1 * stat[i, :64].double()) < 1e-6
        assert rel_err(rvd[i + 1], 0.9 * rv[i + 1].double() + 0.1 * stat[i, 64:].double()) < 1e-6
    want = ticks.clone()
    want[1] += 1
    want[3] += 1
    assert torch.equal(td.cpu(), want)
    assert all_nan(rmd[0]) and all_nan(rmd[-1]) and all_nan(rvd[0]) and all_nan(rvd[-1])
    # one item more than the header allows, and none: refused, nothing moves
    many = limit + 1
    stat, rm, rv, ticks = _replay_setup(many, 5)
    sd, rmd, rvd, td = stat.to(DEV), rm.to(DEV), rv.to(DEV), ticks.to(DEV)
    raises_srlz(C, C.bn_replay_many, _replay_table(C, sd, rmd, rvd, td, many), many, 0.1, C.stream())
    raises_srlz(C, C.bn_replay_many, _replay_table(C, sd, rmd, rvd, td, many), 0, 0.1, C.stream())
    with pytest.raises(C.SrlzError):
        ops.bn_replay_many([(sd[i], rmd[i + 1], rvd[i + 1], td[i + 1:i + 2]) for i in range(many)])
    torch.cuda.synchronize()
    assert torch.equal(td.cpu(), ticks)
    assert torch.equal(rmd[1:-1].cpu(), rm[1:-1]) and torch.equal(rvd[1:-1].cpu(), rv[1:-1])


# ---- 4. loss composition and gradient fan-in ------------------------------------------------------------------------------------
def _scalar_table(dev_scalars, n):
    return (ctypes.c_void_p * max(n, 1))(*[dev_scalars.data_ptr() + 4 * i for i in range(n)])


@gpu
@pytest.mark.parametrize("n", [1, 2, 5, "max"])
def test_weighted_total_is_the_separately_rounded_left_to_right_sum(C, n):
    most = header_constant("SRLZ_MAX_LOSS_TERMS")
    n = most if n == "max" else n
    w, l = find_weighted_total_case(n, seed=n)
    sep, fma, exact = weighted_total_orders(w, l)
    if n > 1:  # (one term is rounded once whichever way it is evaluated)
        assert sep != fma and sep != exact
    ld = torch.from_numpy(l).to(DEV)
    ptrs, wc = _scalar_table(ld, n), (ctypes.c_float * n)(*[float(x) for x in w])
    slots = 1 + most
    tw, total = nan_out(1)
    lw, tail = nan_out(slots)
    C.weighted_total(ptrs, wc, n, C.ptr(total), C.ptr(tail), C.stream())
    torch.cuda.synchronize()
    assert same_bits(total, np.array([sep]))
    assert same_bits(tail[:1], np.array([sep])) and same_bits(tail[1:1 + n], l)
    assert all_nan(tail[1 + n:]) and tail_intact(tw, 1) and tail_intact(lw, slots)
    # tail = NULL: the total alone
    tw, total = nan_out(1)
    C.weighted_total(ptrs, wc, n, C.ptr(total), None, C.stream())
    torch.cuda.synchronize()
    assert same_bits(total, np.array([sep])) and tail_intact(tw, 1)
    # backward: g[i] = fp32(dout * w_i), for an upstream gradient that is not 1
    dout = np.float32(0.7310586)
    dd = torch.from_numpy(np.array([dout])).to(DEV)
    gw, gd = nan_out(n)
    C.weighted_total_bwd(C.ptr(dd), wc, n, C.ptr(gd), C.stream())
    torch.cuda.synchronize()
    want = np.array([np.float32(dout * wi) for wi in w], dtype=np.float32)
    assert any(np.float32(wi) != gi for wi, gi in zip(w, want))
    assert same_bits(gd, want) and tail_intact(gw, n)


@gpu
def test_weighted_total_rejects_no_terms_and_too_many(C):
    most = header_constant("SRLZ_MAX_LOSS_TERMS")
    ld = torch.ones(most + 1, device=DEV)
    ptrs, wc = _scalar_table(ld, most + 1), (ctypes.c_float * (most + 1))(*([1.0] * (most + 1)))
    tw, total = nan_out(1)
    lw, tail = nan_out(most + 2)
    gw, gd = nan_out(most + 1)
    for n in (0, most + 1):
        raises_srlz(C, C.weighted_total, ptrs, wc, n, C.ptr(total), C.ptr(tail), C.stream())
        raises_srlz(C, C.weighted_total_bwd, C.ptr(ld), wc, n, C.ptr(gd), C.stream())
    assert all_nan(tw) and all_nan(lw) and all_nan(gw)


def _terms(nterms, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(nterms, n, generator=g) * torch.tensor([1.0, 1e-3, 50.0, 1e4][:nterms]).view(-1, 1)).numpy()
    if n >= 5:
        t[:, 0] = -0.0
        t[:, 1] = 1e-40
        t[0, 2] = float("inf")
    return t


def _left_to_right(terms):
    out = terms[0].copy()
    with np.errstate(all="ignore"):
        for k in range(1, terms.shape[0]):
            out = out + terms[k]
    assert out.dtype == np.float32
    return out


@gpu
@pytest.mark.parametrize("nterms", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 5, 1024 * 256 + 3])
def test_sum_terms_adds_left_to_right_in_fp32(C, n, nterms):
    t = _terms(nterms, n, 10 * n + nterms)
    td = torch.from_numpy(t).to(DEV)
    ptrs = (ctypes.c_void_p * nterms)(*[td[i].data_ptr() for i in range(nterms)])
    ow, out = nan_out(n)
    C.sum_terms(ptrs, nterms, C.ptr(out), n, C.stream())
    torch.cuda.synchronize()
    assert same_bits(out, _left_to_right(t)) and tail_intact(ow, n)
    assert same_bits(td, t)  # (the terms themselves are untouched)
    if n == 5:
        four = (ctypes.c_void_p * 5)(*[td[i % nterms].data_ptr() for i in range(5)])
        ow, out = nan_out(n)
        for bad in (0, 5):
            raises_srlz(C, C.sum_terms, four, bad, C.ptr(out), n, C.stream())
        assert all_nan(ow)


@gpu
def test_fan_sums_six_consumers_in_alias_order_through_a_chain_of_launches(C):
    """ops.Fan / FanOutFn.backward as it is written: at most four terms per launch, every launch into a fresh buffer, the partial sum
    first in the next launch (the output never aliases a term) — ((((g0 + g1) + g2) + g3) + g4) + g5 over the aliases' indices.
    take() hands the aliases out last index first."""
    from srlz import ops
    g = torch.Generator().manual_seed(6)
    t = torch.randn(33, 200, generator=g).to(DEV).requires_grad_(True)
    scales = [1.0, 1e-3, 50.0, 1e4, 0.3, 7.0]
    ws = [torch.randn(33, 200, generator=g) * s for s in scales]
    fan = ops.Fan(t, 6)
    taken = [fan.take() for _ in range(6)]
    assert all(x.data_ptr() == t.data_ptr() for x in taken)
    loss = None
    for x, w in zip(taken, ws):
        term = (x * w.to(DEV)).sum()
        loss = term if loss is None else loss + term
    loss.backward()
    torch.cuda.synchronize()
    in_alias_order = np.stack([w.numpy() for w in reversed(ws)])
    want = _left_to_right(in_alias_order)
    assert not np.array_equal(want, _left_to_right(in_alias_order[::-1].copy()))  # the order matters for these values
    assert same_bits(t.grad, want)


@gpu
@pytest.mark.parametrize("n_each", [4, 1028, 4 * 4096 * 256 + 4])
def test_join2_copies_both_halves(C, n_each):
    g = torch.Generator().manual_seed(n_each)
    a, b = torch.randn(n_each, generator=g), torch.randn(n_each, generator=g)
    a[0], a[-1], b[0], b[-1] = -0.0, 1e-40, float("inf"), NAN
    ad, bd = a.to(DEV), b.to(DEV)
    ow, out = nan_out(2 * n_each)
    C.join2(C.ptr(ad), C.ptr(bd), C.ptr(out), n_each, C.stream())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), torch.cat((a, b)).view(torch.int32)) and tail_intact(ow, 2 * n_each)


@gpu
def test_join2_rejects_unaligned_and_ragged_halves(C):
    buf = torch.randn(64, device=DEV)
    ow, out = nan_out(32)
    st = C.stream()
    raises_srlz(C, C.join2, C.ptr(buf), C.ptr(buf[16:]), C.ptr(out), 6, st)           # no multiple of 4
    raises_srlz(C, C.join2, C.ptr(buf[1:]), C.ptr(buf[16:]), C.ptr(out), 8, st)       # a: 4 bytes off
    raises_srlz(C, C.join2, C.ptr(buf), C.ptr(buf[17:]), C.ptr(out), 8, st)           # b
    raises_srlz(C, C.join2, C.ptr(buf), C.ptr(buf[16:]), C.ptr(out[2:]), 8, st)       # out
    raises_srlz(C, C.join2, C.ptr(buf), C.ptr(buf[16:]), C.ptr(out), 0, st)
    assert all_nan(ow)


@gpu
@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("ca,cb", [(1, 1), (200, 17), (3, 200)])
def test_cat_cols_and_split_cols_copy_bytes(C, rows, ca, cb):
    g = torch.Generator().manual_seed(rows * 1000 + ca)
    a, b = torch.randn(rows, ca, generator=g), torch.randn(rows, cb, generator=g)
    a[0, 0], b[-1, -1] = -0.0, NAN
    cat = torch.cat((a, b), 1)
    ad, bd, catd = a.to(DEV), b.to(DEV), cat.to(DEV)
    st = C.stream()
    ow, out = nan_out(rows, ca + cb)
    C.cat_cols(C.ptr(ad), C.ptr(bd), C.ptr(out), rows, ca, cb, st)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), cat.view(torch.int32)) and tail_intact(ow, rows * (ca + cb))
    for want_a, want_b in ((True, True), (False, True), (True, False)):  # a = NULL and b = NULL: the other side alone
        (aw, ao), (bw, bo) = nan_out(rows, ca), nan_out(rows, cb)
        C.split_cols(C.ptr(catd), C.ptr(ao) if want_a else None, C.ptr(bo) if want_b else None, rows, ca, cb, st)
        torch.cuda.synchronize()
        if want_a:
            assert torch.equal(ao.cpu().view(torch.int32), a.view(torch.int32)) and tail_intact(aw, rows * ca)
        else:
            assert all_nan(aw)
        if want_b:
            assert torch.equal(bo.cpu().view(torch.int32), b.view(torch.int32)) and tail_intact(bw, rows * cb)
        else:
            assert all_nan(bw)
    assert torch.equal(catd.cpu().view(torch.int32), cat.view(torch.int32))


SQ_GROUPS = [1, 2, 8]
SQ_SIZES = [4, 4100, 3 * 224 * 224]


@functools.lru_cache(maxsize=None)
def _sq_inputs(groups, npg):
    g = torch.Generator().manual_seed(groups * 7 + npg)
    a, b = torch.randn(groups, npg, generator=g), torch.randn(groups, npg, generator=g)
    a[:, 0], b[:, 0], a[:, -1], b[:, -1] = 1.0, 0.0, 1.0, 0.0  # a - b = 1 exactly: the gradient there is the scale factor itself
    ref = ((a.double() - b.double()) ** 2).sum(1)
    return a, b, ref


@gpu
@pytest.mark.parametrize("groups", SQ_GROUPS)
@pytest.mark.parametrize("npg", SQ_SIZES)
def test_sqdiff_sum_groups_and_mean(C, groups, npg):
    a, b, ref = _sq_inputs(groups, npg)
    ad, bd = a.to(DEV), b.to(DEV)
    st = C.stream()
    nbytes = C.reduce_workspace(npg)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ow, out = nan_out(groups)
    C.sqdiff_sum_groups(C.ptr(ad), C.ptr(bd), npg, groups, C.ptr(out), C.ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    got = out.cpu()
    assert tail_intact(ow, groups)
    for gi in range(groups):
        assert abs(float(got[gi]) - float(ref[gi])) <= 2e-6 * abs(float(ref[gi])), gi
        # each group exactly as a single call on its slice computes it
        sw, single = nan_out(1)
        C.sqdiff_sum(C.ptr(ad[gi]), C.ptr(bd[gi]), npg, C.ptr(single), C.ptr(ws), nbytes, st)
        torch.cuda.synchronize()
        assert same_bits(single, got[gi:gi + 1]) and tail_intact(sw, 1)
        if gi in (0, groups - 1):
            for div in (float(npg) + 1.0, 3.7):  # no powers of two: fp32(sum) / div, the division rounded on its own
                mw, mean = nan_out(1)
                C.sqdiff_mean(C.ptr(ad[gi]), C.ptr(bd[gi]), npg, div, C.ptr(mean), C.ptr(ws), nbytes, st)
                torch.cuda.synchronize()
                want = np.float32(np.float32(got[gi].item()) / np.float32(div))
                assert same_bits(mean, np.array([want])) and tail_intact(mw, 1)


@gpu
@pytest.mark.parametrize("groups", SQ_GROUPS)
@pytest.mark.parametrize("npg", SQ_SIZES)
def test_sqdiff_grad_groups_scales_by_c_over_div_times_coef(C, groups, npg):
    a, b, _ = _sq_inputs(groups, npg)
    ad, bd = a.to(DEV), b.to(DEV)
    div, coef = np.float32(3 * 224 * 224), np.float32(-1.7)
    cs = find_scale_order_cases(groups, 7, div, coef)
    cd = torch.from_numpy(cs).to(DEV)
    diff = a.double() - b.double()
    for stride in (0, 1):
        per_group = [cs[gi * stride] for gi in range(groups)]
        dw, da = nan_out(groups, npg)
        C.sqdiff_grad_groups(C.ptr(ad), C.ptr(bd), C.ptr(cd), stride, float(div), float(coef), C.ptr(da), npg, groups, C.stream())
        torch.cuda.synchronize()
        got = da.cpu()
        for gi, c in enumerate(per_group):
            kept, other = scale_orders(c, div, coef)
            assert kept != other
            # where a - b is exactly 1 the output IS the factor: (c / div) * coef, not (c * coef) / div
            assert same_bits(got[gi, [0, -1]], np.array([kept, kept]))
            assert rel_err(got[gi], (float(c) / float(div)) * float(coef) * diff[gi]) < 1e-6
        assert tail_intact(dw, groups * npg)


@gpu
def test_sqdiff_groups_reject_nine_groups_and_ragged_slices(C):
    a, b = torch.randn(9, 8, device=DEV), torch.randn(9, 8, device=DEV)
    st = C.stream()
    nbytes = 9 * 1024 * 8  # (room for nine groups, should the check ever let them through)
    assert nbytes >= C.reduce_workspace(8)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ow, out = nan_out(9)
    dw, da = nan_out(9, 8)
    coef = torch.ones(9, device=DEV)
    raises_srlz(C, C.sqdiff_sum_groups, C.ptr(a), C.ptr(b), 8, 9, C.ptr(out), C.ptr(ws), nbytes, st)
    raises_srlz(C, C.sqdiff_sum_groups, C.ptr(a), C.ptr(b), 6, 2, C.ptr(out), C.ptr(ws), nbytes, st)
    raises_srlz(C, C.sqdiff_grad_groups, C.ptr(a), C.ptr(b), C.ptr(coef), 1, 2.0, 1.0, C.ptr(da), 8, 9, st)
    raises_srlz(C, C.sqdiff_grad_groups, C.ptr(a), C.ptr(b), C.ptr(coef), 1, 2.0, 1.0, C.ptr(da), 6, 2, st)
    assert all_nan(ow) and all_nan(dw)


@gpu
@pytest.mark.parametrize("n", [1, 7, 1024 * 256 + 5])
def test_kl_grad_accumulates_into_its_outputs(C, n):
    g = torch.Generator().manual_seed(n)
    mu, lv = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.3
    old_mu, old_lv = torch.randn(n, generator=g), torch.randn(n, generator=g)
    mud, lvd = mu.to(DEV), lv.to(DEV)
    coef = torch.tensor(0.37, device=DEV)
    (mw, dmu), (lw, dlv) = guarded(old_mu), guarded(old_lv)
    C.kl_grad(C.ptr(mud), C.ptr(lvd), C.ptr(coef), 2.0, C.ptr(dmu), C.ptr(dlv), n, C.stream())
    torch.cuda.synchronize()
    k = float(np.float32(0.37)) * 2.0
    assert rel_err(dmu, old_mu.double() + k * mu.double()) < 1e-6
    assert rel_err(dlv, old_lv.double() + k * 0.5 * (lv.double().exp() - 1)) < 1e-5
    assert tail_intact(mw, n) and tail_intact(lw, n)


@gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_param_norms_grad_per_segment(C, mode):
    lens = [1, 2049, 70000]
    g = torch.Generator().manual_seed(40 + mode)
    params = [torch.randn(n, generator=g) for n in lens]
    params[1].zero_()
    scale, up = (1.0 if mode == 0 else 1.0 / 3), 0.37
    pr = [p.double().requires_grad_(True) for p in params]
    total = scale * sum(p.abs().sum() if mode == 0 else p.norm(2) for p in pr)
    (total * float(np.float32(up))).backward()
    pd = [p.to(DEV) for p in params]
    outs = [nan_out(n) for n in lens]
    ptrs = torch.tensor([p.data_ptr() for p in pd], dtype=torch.int64, device=DEV)
    gptrs = torch.tensor([o.data_ptr() for _, o in outs], dtype=torch.int64, device=DEV)
    lens_d = torch.tensor(lens, dtype=torch.int64, device=DEV)
    nw, norms = nan_out(3)
    tw, tot = nan_out(1)
    coef = torch.tensor(up, device=DEV)
    st = C.stream()
    C.param_norms(C.ptr(ptrs), C.ptr(lens_d), 3, mode, scale, C.ptr(norms), C.ptr(tot), st)
    C.param_norms_grad(C.ptr(ptrs), C.ptr(gptrs), C.ptr(lens_d), 3, mode, C.ptr(norms), C.ptr(coef), scale, st)
    torch.cuda.synchronize()
    assert rel_err(tot, total) < 1e-6 and tail_intact(nw, 3) and tail_intact(tw, 1)
    for (whole, got), ref, n in zip(outs, pr, lens):
        assert tail_intact(whole, n)
        if ref.grad.abs().max() == 0:
            assert bool((got == 0).all())  # exactly 0 (and no NaN from 0 / 0)
        else:
            assert rel_err(got, ref.grad) < 1e-6
    assert float(pr[1].grad.abs().max()) == 0.0  # (the all-zero segment: sign(0) = 0, and torch's d||p|| / dp = 0 at p = 0)
