"""The dense kernels of --model-type mlp / linear (csrc/dense.hip through srlz/ops.py) against fp64 torch: the input layer's forward and
weight gradient, the output layer's forward, its fused reconstruction / generation loss and that loss's backward, on uint8 and fp32
operands.  The uint8 route must equal the fp32 route bit for bit, two runs must be bit-identical, and the loss-only route must give the
loss of the materialised frames.  Plus the static ISA audit of the new kernels (no scratch traffic around the MFMAs)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def rel(a, b):
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def frames(M, C, side, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (M, C, side, side), generator=g, dtype=torch.uint8).cuda()


def uniform(shape, bound, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound).float().cuda()


# (M, n, C, side): the step shapes (224 x 224 planes) and small planes for the odd corners
SHAPES = [(1, 2, 3, 224), (2, 50, 3, 224), (7, 64, 6, 32), (512, 50, 3, 224), (512, 200, 6, 224), (1024, 64, 3, 224),
          (1024, 200, 6, 64), (7, 200, 3, 16)]
ACTS = {0: lambda t: t, 1: torch.relu, 2: torch.tanh}


def in_layer(x, w, b, act, side, dy):
    from srlz import ops
    w = w.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    y = ops.DenseInFn.apply(x, w, b, act, side * side)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), w.grad, b.grad


@pytest.mark.gpu
@pytest.mark.parametrize("M,n,C,side", SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_dense_in_fwd_and_wgrad(M, n, C, side, act):
    from srlz import ops
    if act and (M, n) not in ((7, 64), (512, 50), (1024, 64)):
        pytest.skip("activations are covered on three shapes")
    K = C * side * side
    x8 = frames(M, C, side, 1)
    xf = ops.frames_as_float(x8)
    w, b = uniform((n, K), K ** -0.5, 2), uniform((n,), K ** -0.5, 3)
    dy = uniform((M, n), 1.0, 4)
    y8, dw8, db8 = in_layer(x8, w, b, act, side, dy)
    yf, dwf, dbf = in_layer(xf, w, b, act, side, dy)
    # uint8 frames through the normalisation table == the normalised fp32 frames, bit for bit
    assert torch.equal(y8, yf) and torch.equal(dw8, dwf) and torch.equal(db8, dbf)
    y2, dw2, db2 = in_layer(x8, w, b, act, side, dy)
    assert torch.equal(y8, y2) and torch.equal(dw8, dw2) and torch.equal(db8, db2)  # two runs
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    y64 = ACTS[act](torch.nn.functional.linear(xf.double().view(M, -1), w64, b64))
    y64.backward(dy.double())
    assert rel(yf, y64) < 1e-5
    assert rel(dwf, w64.grad) < 1e-5 and rel(dbf, b64.grad) < 1e-5


def out_layer(z, w, b, side, target=None, mean=True, dout=None):
    from srlz import ops
    z = z.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    if target is None:
        r = ops.DenseOutFn.apply(z, w, b, side * side)
        r.backward(dout)
    else:
        r = ops.DenseOutLossFn.apply(z, w, b, target, mean, side * side)
        r.backward()
    torch.cuda.synchronize()
    return r.detach(), z.grad, w.grad, b.grad


@pytest.mark.gpu
@pytest.mark.parametrize("M,n,C,side", SHAPES)
def test_dense_out_fwd_loss_and_bwd(M, n, C, side):
    from srlz import ops
    K = C * side * side
    z = uniform((M, n), 1.0, 5)
    w, b = uniform((K, n), n ** -0.5, 6), uniform((K,), n ** -0.5, 7)
    t8 = frames(M, C, side, 8)
    tf = ops.frames_as_float(t8)
    z64, w64, b64 = (t.double().requires_grad_(True) for t in (z, w, b))
    out64 = torch.nn.functional.linear(z64, w64, b64)
    # materialised route, with an arbitrary upstream gradient
    dout = uniform((M, K), 1.0, 9)
    out, dz, dw, db = out_layer(z, w, b, side, dout=dout)
    out64.backward(dout.double(), retain_graph=True)
    assert rel(out, out64) < 1e-5
    assert rel(dz, z64.grad) < 1e-5 and rel(dw, w64.grad) < 1e-5 and rel(db, b64.grad) < 1e-5
    out2, dz2, dw2, db2 = out_layer(z, w, b, side, dout=dout)
    assert torch.equal(out, out2) and torch.equal(dz, dz2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    if M % 2:
        return  # the fused loss is a pair loss: the two frames of a step
    for mean in (True, False):
        for t in (z64, w64, b64):
            t.grad = None
        half = M // 2
        d = out64 - tf.double().view(M, K)
        if mean:
            loss64 = (d[:half] ** 2).sum() / (half * K) + (d[half:] ** 2).sum() / (half * K)
        else:
            loss64 = (d ** 2).sum()
        loss64.backward(retain_graph=True)
        res8 = out_layer(z, w, b, side, target=t8, mean=mean)
        resf = out_layer(z, w, b, side, target=tf, mean=mean)
        for a, c in zip(res8, resf):
            assert torch.equal(a, c)  # uint8 target == fp32 target, bit for bit
        res2 = out_layer(z, w, b, side, target=t8, mean=mean)
        for a, c in zip(res8, res2):
            assert torch.equal(a, c)  # two runs
        loss, dz, dw, db = resf
        assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item())
        assert rel(dz, z64.grad) < 1e-5 and rel(dw, w64.grad) < 1e-5 and rel(db, b64.grad) < 1e-5
        # the loss-only route gives the loss of the materialised frames
        with torch.no_grad():
            frames_out = ops.DenseOutFn.apply(z, w, b, side * side).view(M, C, side, side)
            mat = ops.SqDiffPairLossFn.apply(frames_out, tf, mean)
        assert abs(loss.item() - mat.item()) <= 1e-6 * abs(mat.item())


@pytest.mark.gpu
def test_planar_u8_flat_index_is_the_reference_view():
    """The reference flattens x.view(B, -1) of the loader's [B, C, W, H] tensor (data_loader.py transposes the decoded [H, W, C] image
    by (2, 1, 0)): element c*W*H + w*H + h.  The input layer on the planar uint8 frames must equal F.linear on exactly that view of the
    normalised frames — with W != H, so that a swapped plane order would show."""
    from srlz import ops
    B, C, H, W = 3, 6, 24, 40
    g = torch.Generator().manual_seed(17)
    decoded = torch.randint(0, 256, (B, H, W, C), generator=g, dtype=torch.uint8)
    planar = decoded.permute(0, 3, 2, 1).contiguous().cuda()  # [B, C, W, H], what DataLoader(raw_uint8="planar") hands over
    K = C * W * H
    w, b = uniform((8, K), K ** -0.5, 18), uniform((8,), 0.1, 19)
    y = ops.DenseInFn.apply(planar, w, b, 0, W * H)
    # reference: normalise the decoded frame per pixel (utils.py:20-32), transpose, view(B, -1)
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)
    norm = (decoded.double() / 255.0 - mean.repeat(2)) / std.repeat(2)
    ref = torch.nn.functional.linear(norm.permute(0, 3, 2, 1).reshape(B, -1), w.double().cpu(), b.double().cpu())
    assert rel(y.cpu(), ref) < 1e-5


@pytest.mark.gpu
def test_tanh_and_noise_add():
    from srlz import ops
    x = uniform((7, 50), 3.0, 10).requires_grad_(True)
    y = ops.TanhFn.apply(x)
    dy = uniform((7, 50), 1.0, 11)
    y.backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    y64 = torch.tanh(x64)
    y64.backward(dy.double())
    assert rel(y.detach(), y64) < 1e-6 and rel(x.grad, x64.grad) < 1e-6
    c = uniform((7, 50), 1.0, 12)
    a = x.detach().clone().requires_grad_(True)
    s = ops.AddConstFn.apply(a, c)
    s.backward(dy)
    assert torch.equal(s.detach(), a.detach() + c) and torch.equal(a.grad, dy)


@pytest.mark.gpu
def test_shape_rejections_do_not_launch():
    from srlz import ops, _cabi
    w = torch.zeros((257, 3 * 16 * 16), device="cuda")
    with pytest.raises(_cabi.SrlzError):
        ops.DenseInFn.apply(torch.zeros((2, 3, 16, 16), device="cuda"), w, None, 0, 256)
    with pytest.raises(_cabi.SrlzError):  # an odd pair
        ops.DenseOutLossFn.apply(torch.zeros((3, 4), device="cuda"), torch.zeros((3 * 256, 4), device="cuda"), None,
                                 torch.zeros((3, 3, 16, 16), device="cuda"), True, 256)


def test_isa_audit_dense_kernels():
    """No spills in the tile kernel (a scratch reload inside the MFMA loop would drain every load in flight) and no serialised stores."""
    import shutil
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import isa_audit
    if not os.path.exists(isa_audit.HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    ks = list(isa_audit.kernels(isa_audit.disassemble(os.path.join(isa_audit.CSRC, "dense.hip"))))
    names = isa_audit.demangle([k for k, _ in ks])
    tiles = 0
    for (_, body), name in zip(ks, names):
        a = isa_audit.audit(body)
        assert a["store_wait_chain"] < 2, name
        assert a["scratch_reloads"] == 0, name
        if name.startswith("dense_tile_kernel"):
            tiles += 1
            assert a["mfma"] >= 16, name
    assert tiles >= 9
