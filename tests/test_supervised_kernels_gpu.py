"""The supervised baseline's two kernels (csrc/supervised.hip) through the C ABI against fp64 torch on the CPU, a sentinel tail behind
every output: srlz_mse_target_fwd (loss and unit gradient in one launch, bit-identical between runs, backward through
srlz_scale_by_scalar) and srlz_dropout_fwd / srlz_dropout_bwd (exact against x * mask / (1 - p) in fp32).

Tolerance: 1e-5 of the output scale.  Measured on MI355X (printed by the tests): see DESIGN.md 3.7."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-5
SENTINEL = 12345.5
TAIL = 64


def _c():
    from srlz import _cabi as C
    return C


def _guarded(n):
    """An fp32 device buffer of n elements with TAIL sentinel elements behind it -> (whole, the n-element view)."""
    whole = torch.full((n + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
    return whole, whole[:n]


def _tail_intact(whole, n):
    return bool((whole[n:] == SENTINEL).all())


# (1, 1) ... (257, 3): the issue's shapes; the kernel is ONE workgroup of 1024 threads taking 4 elements per thread and pass, so
# 4096 elements are one full pass: (1024, 4) sits on that boundary, (1025, 4) and (1366, 3) (a second pass / a 2-element tail) just
# across it; (1024, 1024) is the largest B * S the entry point takes
MSE_SHAPES = [(1, 1), (3, 2), (5, 200), (257, 3), (1024, 4), (1025, 4), (1366, 3), (1024, 1024)]


@pytest.mark.parametrize("B,S", MSE_SHAPES)
def test_mse_target_matches_fp64_and_is_deterministic(B, S):
    C = _c()
    rs = np.random.RandomState(B * 7 + S)
    pred, target = rs.randn(B, S).astype(np.float32), (0.5 * rs.randn(B, S) + 0.25).astype(np.float32)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    n = B * S
    runs = []
    for _ in range(2):
        lw, loss = _guarded(1)
        uw, unit = _guarded(n)
        C.mse_target_fwd(C.ptr(p), C.ptr(t), B, S, C.ptr(loss), C.ptr(unit), C.stream())
        torch.cuda.synchronize()
        assert _tail_intact(lw, 1) and _tail_intact(uw, n)
        runs.append((loss.cpu().clone(), unit.cpu().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # bit-identical
    d64 = torch.from_numpy(pred).double() - torch.from_numpy(target).double()
    ref_loss, ref_unit = float((d64 * d64).mean()), 2.0 * d64 / n
    e_loss = abs(float(runs[0][0]) - ref_loss) / ref_loss
    e_unit = float((runs[0][1].double().view(B, S) - ref_unit).abs().max() / ref_unit.abs().max())
    print("mse_target B=%d S=%d: loss rel err %.2e, dpred_unit err %.2e of its scale" % (B, S, e_loss, e_unit))
    assert e_loss <= TOL and e_unit <= TOL, (e_loss, e_unit)


@pytest.mark.parametrize("B,S", [(3, 2), (257, 3), (1025, 4)])
def test_mse_target_backward_with_a_non_unit_incoming_gradient(B, S):
    from srlz import ops
    rs = np.random.RandomState(B + S)
    pred, target = rs.randn(B, S).astype(np.float32), rs.randn(B, S).astype(np.float32)
    p = torch.from_numpy(pred).cuda().requires_grad_(True)
    loss = ops.mse_target(p, torch.from_numpy(target).cuda())
    (loss * -2.75).backward()
    p64 = torch.from_numpy(pred).double().requires_grad_(True)
    ref = torch.nn.functional.mse_loss(p64, torch.from_numpy(target).double())
    (ref * -2.75).backward()
    torch.cuda.synchronize()
    e = float((p.grad.double().cpu() - p64.grad).abs().max() / p64.grad.abs().max())
    print("mse_target backward B=%d S=%d: err %.2e of its scale" % (B, S, e))
    assert abs(float(loss.detach()) - float(ref.detach())) <= TOL * float(ref.detach()) and e <= TOL, e
    with pytest.raises(Exception, match="target must not require a gradient"):
        ops.mse_target(p, torch.from_numpy(target).cuda().requires_grad_(True))


def test_mse_target_rejects_what_it_cannot_take():
    C = _c()
    from srlz import ops
    x = torch.zeros(8, device="cuda")
    for args, text in (((None, C.ptr(x), 1, 1, C.ptr(x), C.ptr(x)), "null"), ((C.ptr(x), C.ptr(x), 0, 4, C.ptr(x), C.ptr(x)), "B = 0"),
                       ((C.ptr(x), C.ptr(x), 2, 0, C.ptr(x), C.ptr(x)), "S = 0"),
                       ((C.ptr(x), C.ptr(x), 1024, 1025, C.ptr(x), C.ptr(x)), "exceeds")):
        with pytest.raises(C.SrlzError, match=text):
            C.mse_target_fwd(*(args + (C.stream(),)))
    big = torch.zeros((1 << 20) + 1, 1, device="cuda")
    with pytest.raises(C.SrlzError, match="exceeds"):  # ... and through the autograd seam: an error, never a silent fallback
        ops.mse_target(big, big.clone())


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 64), (5, 7), (33, 65)])
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("mask_kind", ["random", "zeros", "ones"])
def test_dropout_is_exact(rows, cols, p, mask_kind):
    C = _c()
    rs = np.random.RandomState(rows * 100 + cols)
    x = torch.from_numpy(rs.randn(rows, cols).astype(np.float32))
    dy = torch.from_numpy(rs.randn(rows, cols).astype(np.float32))
    mask = {"random": torch.from_numpy((rs.rand(rows, cols) < 1 - p).astype(np.uint8)), "zeros": torch.zeros(rows, cols, dtype=torch.uint8),
            "ones": torch.ones(rows, cols, dtype=torch.uint8)}[mask_kind]
    n = rows * cols
    m = mask.cuda()
    yw, y = _guarded(n)
    dw, dx = _guarded(n)
    xd, dyd = x.cuda(), dy.cuda()
    C.dropout_fwd(C.ptr(xd), C.ptr(m), 1.0 - p, C.ptr(y), rows, cols, C.stream())
    C.dropout_bwd(C.ptr(dyd), C.ptr(m), 1.0 - p, C.ptr(dx), rows, cols, C.stream())
    torch.cuda.synchronize()
    assert _tail_intact(yw, n) and _tail_intact(dw, n)
    assert torch.equal(y.cpu().view(rows, cols), x * mask / (1 - p))
    assert torch.equal(dx.cpu().view(rows, cols), dy * mask / (1 - p))


def test_dropout_seam_forward_backward_and_eval_launches_nothing():
    from models import DenseNetwork
    from srlz import ops
    x = torch.randn(5, 7, device="cuda", requires_grad=True)
    mask = (torch.rand(5, 7) < 0.9).to(torch.uint8)
    y = ops.DropoutFn.apply(x, mask.cuda(), 0.1)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu(), x.detach().cpu() * mask / (1 - 0.1))
    assert torch.equal(x.grad.cpu(), torch.ones(5, 7) * mask / (1 - 0.1))
    with pytest.raises(Exception, match="uint8"):
        ops.DropoutFn.apply(x, mask.float().cuda(), 0.1)
    # eval mode: the forward never reaches the dropout seam
    net = DenseNetwork(3 * 224 * 224, 3).cuda().eval()
    calls = []
    real = ops.DropoutFn.apply
    ops.DropoutFn.apply = lambda *a: calls.append(1) or real(*a)
    try:
        frames = torch.randint(0, 256, (2, 3, 224, 224), dtype=torch.uint8, device="cuda")
        with torch.no_grad():
            net(frames)
        assert not calls
        net.train()
        net(frames)
        assert calls == [1]
    finally:
        ops.DropoutFn.apply = real
