"""The one-workgroup kernels that end in the shared fixed-order block sum (csrc/common.h: block_sum_d / block_sum_pairs_d), through
the C ABI against fp64 torch on the CPU, at row counts that leave waves of the block idle (1), partly filled (63), barely started (65)
and wrapped round the block (257): srlz_cross_entropy, srlz_triplet_fwd, srlz_prelu_bwd, srlz_mse_target_fwd, and srlz_param_norms
over segments shorter than a wave, just short of a block and longer than one pass of a block.

Every entry point is called twice and must give the same bits: the summation order is fixed.  Each tolerance is the one the older test
of the same entry point uses (named where it is applied)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
ROWS = [1, 63, 65, 257]


@pytest.fixture(scope="module")
def C():
    from srlz import _cabi
    assert torch.cuda.is_available()
    return _cabi


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def twice(call, *outs):
    """Run call() twice into NaN-filled outputs -> the first run's outputs on the CPU, after checking the second run's are the same bits."""
    runs = []
    for _ in range(2):
        for o in outs:
            o.fill_(NAN)
        call()
        torch.cuda.synchronize()
        runs.append([o.cpu().clone() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    return runs[0]


@pytest.mark.parametrize("B", ROWS)
def test_cross_entropy(C, B):
    A = 3
    g = torch.Generator().manual_seed(100 + B)
    logits = torch.randn(B, A, generator=g) * 2
    tgt = torch.randint(0, A, (B,), generator=g)
    lr = logits.double().requires_grad_(True)
    ref = F.cross_entropy(lr, tgt)
    ref.backward()
    logits_d, tgt_d = logits.to(DEV), tgt.to(DEV)
    out, dl = nans(1), nans(B, A)
    out_c, dl_c = twice(lambda: C.cross_entropy(C.ptr(logits_d), C.ptr(tgt_d), B, A, C.ptr(out), C.ptr(dl), C.stream()), out, dl)
    e = abs(out_c.item() - ref.item())
    print("cross_entropy B=%d: loss abs err %.2e, dlogits %.2e" % (B, e, rel_err(dl_c, lr.grad)))
    # tests/test_kernels_gpu.py::test_reparam_ce_onehot
    assert e < 1e-6 * max(1.0, abs(ref.item()))
    assert rel_err(dl_c, lr.grad) < 1e-5


@pytest.mark.parametrize("B", ROWS)
def test_triplet_fwd(C, B):
    S, alpha = 2, 0.2
    g = torch.Generator().manual_seed(200 + B)
    # the hinge argument |s-p|^2 - |s-n|^2 + alpha is far from 0 on either side (>= 0.75 or <= -5), so fp32 and fp64 take the same branch
    s, u, v = (torch.randn(B, S, generator=g) for _ in range(3))
    u, v = u / u.norm(dim=1, keepdim=True), v / v.norm(dim=1, keepdim=True)
    r = 1.0 + torch.rand(B, 1, generator=g)
    active = torch.rand(B, 1, generator=g) < 0.6
    active[0] = True
    p, n = s + r * u, s + torch.where(active, 0.5 * r, 1.5 * r + 1.0) * v
    arg = (s - p).double().pow(2).sum(1) - (s - n).double().pow(2).sum(1) + alpha
    assert bool(((arg > 0.5) == active.reshape(-1)).all()) and bool((arg.abs() > 0.5).all())
    ref = arg.clamp(min=0).mean()
    sd, pd, nd = s.to(DEV), p.to(DEV), n.to(DEV)
    out, hinge = nans(1), nans(B)
    out_c, hinge_c = twice(lambda: C.triplet_fwd(C.ptr(sd), C.ptr(pd), C.ptr(nd), B, S, alpha, C.ptr(out), C.ptr(hinge), C.stream()),
                           out, hinge)
    e = rel_err(out_c, ref.reshape(1))
    print("triplet_fwd B=%d: loss %.2e" % (B, e))
    assert torch.equal(hinge_c, active.reshape(-1).float())
    assert e < 1e-4  # tests/test_trunk_kernels_gpu.py::test_triplet_fwd_bwd (TOL)


@pytest.mark.parametrize("n", [1] + [B * 128 for B in ROWS])
def test_prelu_bwd(C, n):
    slope = 0.25
    g = torch.Generator().manual_seed(300 + n)
    x, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x[torch.rand(n, generator=g) < 0.15] = 0.0  # exact zeros: the slope's side of the subgradient
    if n == 1:
        x[0] = -0.75
    xr = x.double().requires_grad_(True)
    sr = torch.tensor([slope], dtype=torch.float64, requires_grad=True)
    F.prelu(xr, sr).backward(dy.double())
    xd, dyd = x.to(DEV), dy.to(DEV)
    sd = torch.tensor([slope], dtype=torch.float32, device=DEV)
    dx, ds = nans(n), nans(1)
    dx_c, ds_c = twice(lambda: C.prelu_bwd(C.ptr(xd), C.ptr(sd), C.ptr(dyd), C.ptr(dx), C.ptr(ds), n, C.stream()), dx, ds)
    e = (rel_err(dx_c, xr.grad), rel_err(ds_c, sr.grad))
    print("prelu_bwd n=%d: dx %.2e dslope %.2e" % ((n,) + e))
    assert max(e) < 1e-4, e  # tests/test_trunk_kernels_gpu.py::test_prelu_c_abi (TOL)


@pytest.mark.parametrize("B", ROWS)
def test_mse_target_fwd(C, B):
    S = 2
    g = torch.Generator().manual_seed(400 + B)
    pred, target = torch.randn(B, S, generator=g), 0.5 * torch.randn(B, S, generator=g) + 0.25
    d64 = pred.double() - target.double()
    ref_loss, ref_unit = (d64 * d64).mean(), 2.0 * d64 / (B * S)
    p, t = pred.to(DEV), target.to(DEV)
    loss, unit = nans(1), nans(B, S)
    loss_c, unit_c = twice(lambda: C.mse_target_fwd(C.ptr(p), C.ptr(t), B, S, C.ptr(loss), C.ptr(unit), C.stream()), loss, unit)
    e = (rel_err(loss_c, ref_loss.reshape(1)), rel_err(unit_c, ref_unit))
    print("mse_target_fwd B=%d: loss %.2e dpred_unit %.2e" % ((B,) + e))
    assert max(e) <= 1e-5, e  # tests/test_supervised_kernels_gpu.py::test_mse_target_matches_fp64_and_is_deterministic (TOL)


@pytest.mark.parametrize("mode", [0, 1])
def test_param_norms(C, mode):
    g = torch.Generator().manual_seed(500 + mode)
    params = [torch.randn(n, generator=g) for n in (1, 255, 2049)]
    ref_norms = torch.stack([p.double().abs().sum() if mode == 0 else p.double().norm(2) for p in params])
    scale = 1.0 if mode == 0 else 1.0 / len(params)
    pd = [p.to(DEV) for p in params]
    ptrs = torch.tensor([p.data_ptr() for p in pd], dtype=torch.int64, device=DEV)
    lens = torch.tensor([p.numel() for p in pd], dtype=torch.int64, device=DEV)
    norms, out = nans(len(pd)), nans(1)
    norms_c, out_c = twice(lambda: C.param_norms(C.ptr(ptrs), C.ptr(lens), len(pd), mode, scale, C.ptr(norms), C.ptr(out), C.stream()),
                           norms, out)
    # (every segment is one workgroup's block sum: each against its own magnitude)
    e = (((norms_c.double() - ref_norms) / ref_norms).abs().max().item(), rel_err(out_c, (ref_norms.sum() * scale).reshape(1)))
    print("param_norms mode=%d: norms %.2e total %.2e" % ((mode,) + e))
    assert max(e) < 1e-6, e  # tests/test_kernels_gpu.py::test_mask_columns_and_param_norms
