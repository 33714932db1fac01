"""The construction of tests/test_kernels_gpu.py::test_conv64_bwd_fused_whole_block_backward, shared with the steady-state cases of
tests/test_persistent_steady_gpu.py: one decoder block's whole backward (srlz_conv64_bwd_fused) against fp64 autograd and against the
two-launch path, with every assertion of that test inside."""
import torch
import torch.nn.functional as F

DEV = "cuda"


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = ref.abs().max().item()
    return (got - ref).abs().max().item() / max(scale, 1e-30)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def whole_block_backward(C, n, hi, groups, training, zero_gamma, regime=None):
    """srlz_conv64_bwd_fused — data, weight and bias gradient of ConvTranspose2d(64,64,3,2) whose output went through
    BatchNorm2d + ReLU and whose input was relu(batchnorm(x)), from ONE staging of the rebuilt d(loss)/dy — against
    (i) fp64 autograd through relu(bn(x)) -> conv_transpose2d -> batch_norm -> relu per BatchNorm group, EVERY element of dx
    and dw to 1e-4 at every size, and
    (ii) the two-launch path srlz_conv64_bwd_data(dy_out) + srlz_conv64_bwd_weight: dx bit for bit, dw / db to rounding.

    The discrete decisions are taken out of the comparison the way tests/test_step_gpu.py does it for whole steps (two correct
    evaluations decide a ReLU at |bn(.)| ~ 1e-7 differently, and one flipped decision moves ~256 dx values by 1e-2 of the
    maximum): the INPUT activations are moved off the ReLU threshold of their record (the record is an input of the kernel), and
    the incoming gradient dA is zeroed wherever the device's own bn(y) lies within 1e-4 of the output ReLU's threshold — there the
    decision multiplies a zero in the data gradient, in the weight gradient and in both BatchNorm-backward sums, for either
    evaluation; everywhere else the fp32 and fp64 decisions agree (the two evaluations of bn(y) differ by ~1e-6)."""
    assert n % groups == 0
    g = torch.Generator().manual_seed(77 * hi + n)
    ho = (hi - 1) * 2 + 3
    x = torch.randn(n, 64, hi, hi, generator=g) * 1.2 + 0.1            # raw output of the previous layer
    w, b = torch.randn(64, 64, 3, 3, generator=g) * 0.05, torch.randn(64, generator=g) * 0.1
    gx, bx = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    if zero_gamma:  # input-side BatchNorm channels without a usable scale: exactly 0 (with a positive and a negative shift) and tiny
        gx[3], bx[3] = 0.0, 0.3
        gx[17], bx[17] = 0.0, -0.2
        gx[40], bx[40] = 1e-5, 0.25
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    rm, rv = torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5
    da = torch.randn(n, 64, ho, ho, generator=g)
    per = n // groups
    # ---- the input's BatchNorm record per group (fp32, as the kernel receives it); x moved off its ReLU threshold
    xrecs, recs64 = [], []
    for gi in range(groups):
        xs = x[gi * per:(gi + 1) * per].double()
        m, v = xs.mean((0, 2, 3)), xs.var((0, 2, 3), unbiased=False)
        inv = 1.0 / torch.sqrt(v + 1e-5)
        rec = torch.cat((m, inv, gx.double() * inv, bx.double() - m * gx.double() * inv)).float()
        xrecs.append(rec)
        sc, sh = rec[128:192].double().view(1, 64, 1, 1), rec[192:256].double().view(1, 64, 1, 1)
        recs64.append((sc, sh))
        z = xs * sc + sh
        near = z.abs() < 1e-3
        movable = (sc.abs() > 1e-2).expand_as(z)  # (a channel without a scale cannot be moved off the threshold — nor does it sit on it)
        xs = torch.where(near & movable, (torch.where(z >= 0, 2e-3, -2e-3) - sh) / torch.where(sc.abs() > 1e-2, sc, torch.ones(())), xs)
        x[gi * per:(gi + 1) * per] = xs.float()
        assert float(((x[gi * per:(gi + 1) * per].double() * sc + sh).abs()).min()) > 5e-4
    # ---- device: forward through the C ABI to get y, its statistics and the backward sums
    st = C.stream()
    d = C.Conv64Desc(n, hi, hi, ho, ho, 3, 2, 0, 1, groups)
    assert C.conv64_bwd_fused_supported(d) == 1
    if regime is not None:  # (the caller asserts which part of the persistent loop this size reaches, before anything is launched)
        regime(d)
    xd, wd, bd = nhwc(x).to(DEV), w.to(DEV), b.to(DEV)
    xbnp = torch.cat(xrecs).to(DEV)
    packs = torch.empty(2, C.conv64_packed_floats(), device=DEV)
    C.conv64_pack_weights(C.ptr(wd), C.ptr(packs[0]), C.ptr(packs[1]), d, st)
    y = torch.empty(n, ho, ho, 64, device=DEV)
    stats = torch.empty(C.conv64_fwd_tiles(d), 128, device=DEV)
    C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), C.ptr(bd), C.ptr(y), C.ptr(stats), C.ptr(xbnp), d, st)
    gd, bed, rmd, rvd = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
    bnp = torch.empty(256 * groups, device=DEV)
    nbn = C.bn_bwd_workspace(0)
    bws = torch.empty(nbn, dtype=torch.uint8, device=DEV)
    if training:
        bstat = torch.empty(128 * groups, device=DEV)
        C.bn_finalize(C.ptr(stats), stats.shape[0], groups, per * ho * ho, C.ptr(gd), C.ptr(bed), 1e-5, 0.1, 1, C.ptr(rmd), C.ptr(rvd),
                      None, C.ptr(bnp), C.ptr(bstat), C.ptr(bws), nbn, st)
    else:
        one = torch.empty(256, device=DEV)
        C.bn_eval_params(C.ptr(gd), C.ptr(bed), C.ptr(rmd), C.ptr(rvd), 1e-5, C.ptr(one), st)
        bnp = one.repeat(groups)
    # ---- dA = 0 wherever the device's bn(y) is within 1e-4 of the output ReLU's threshold
    torch.cuda.synchronize()
    rec_y = bnp.view(groups, 256).double().cpu()
    zy = nchw(y).double().cpu().view(groups, per, 64, ho, ho) * rec_y[:, 128:192].view(groups, 1, 64, 1, 1) \
        + rec_y[:, 192:256].view(groups, 1, 64, 1, 1)
    tie = (zy.abs() < 1e-4).view(n, 64, ho, ho)
    da = torch.where(tie, torch.zeros(()), da)
    dad = nhwc(da).to(DEV)
    # ---- fp64 reference, group by group (per-call BatchNorm statistics)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    dx_ref = []
    for gi in range(groups):
        sc, sh = recs64[gi]
        a = torch.relu(x[gi * per:(gi + 1) * per].double() * sc + sh).requires_grad_(True)
        yr = F.conv_transpose2d(a, wr, br, stride=2)
        zr = F.batch_norm(yr, rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), bool(training), 0.1, 1e-5)
        # outside the zeroed ties both evaluations take the same decision
        assert bool((((zr > 0) == (zy[gi] > 0)) | tie[gi * per:(gi + 1) * per]).all())
        F.relu(zr).backward(da[gi * per:(gi + 1) * per].double())
        dx_ref.append(a.grad)
    dx_ref = torch.cat(dx_ref)
    sums, dgm, dbt = torch.empty(128 * groups, device=DEV), torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    C.bn_relu_bwd_sums(C.ptr(y), C.ptr(bnp), C.ptr(dad), C.ptr(sums), C.ptr(dgm), C.ptr(dbt), C.ptr(bws), nbn, n * ho * ho, groups, st)
    # ---- two launches
    dy_out = torch.full((n, ho, ho, 64), float("nan"), device=DEV)
    op = C.BnBwdOperand(y.data_ptr(), bnp.data_ptr(), sums.data_ptr(), per * ho * ho, training, dy_out.data_ptr())
    dx0 = torch.full((n, hi, hi, 64), float("nan"), device=DEV)
    C.conv64_bwd_data(C.ptr(dad), C.ptr(packs[1]), C.ptr(dx0), op, d, st)
    nbytes = C.conv64_bwd_weight_workspace(d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw0, db0 = torch.full((64, 64, 3, 3), float("nan"), device=DEV), torch.full((64,), float("nan"), device=DEV)
    C.conv64_bwd_weight(C.ptr(xd), C.ptr(dy_out), C.ptr(dw0), C.ptr(db0), C.ptr(xbnp), None, C.ptr(ws), nbytes, d, st)
    # ---- one launch
    op1 = C.BnBwdOperand(y.data_ptr(), bnp.data_ptr(), sums.data_ptr(), per * ho * ho, training, None)
    dx1 = torch.full((n, hi, hi, 64), float("nan"), device=DEV)
    dw1, db1 = torch.full((64, 64, 3, 3), float("nan"), device=DEV), torch.full((64,), float("nan"), device=DEV)
    nb1 = C.conv64_bwd_fused_workspace(d)
    ws1 = torch.full((nb1 // 4,), float("nan"), device=DEV)
    rows = C.conv64_bwd_fused_bn_rows(d)
    part1 = torch.full((rows, 128), float("nan"), device=DEV)
    C.conv64_bwd_fused(C.ptr(xd), C.ptr(xbnp), C.ptr(dad), op1, C.ptr(packs[1]), C.ptr(dx1), C.ptr(dw1), C.ptr(db1), C.ptr(part1), C.ptr(ws1), nb1,
                       d, st)
    # determinism: a second launch, bit for bit (this one without the BatchNorm-backward records: the other outputs do not depend on them)
    dx2, dw2, db2 = torch.empty_like(dx1), torch.empty_like(dw1), torch.empty_like(db1)
    C.conv64_bwd_fused(C.ptr(xd), C.ptr(xbnp), C.ptr(dad), op1, C.ptr(packs[1]), C.ptr(dx2), C.ptr(dw2), C.ptr(db2), None, C.ptr(ws1), nb1, d, st)
    torch.cuda.synchronize()
    assert torch.isfinite(dx1).all() and torch.equal(dx1, dx0)
    assert torch.equal(dx2, dx1) and torch.equal(dw2, dw1) and torch.equal(db2, db1)
    # ---- round 6: the BatchNorm-backward sums of the layer that produced x, out of the same launch's flush (+ its companion for the
    # channels without a usable scale), against srlz_bn_relu_bwd_sums' separate pass over (x, dx) — sums per group, dgamma / dbeta
    assert torch.isfinite(part1).all()
    sums_a, dg_a, db_a = torch.empty(128 * groups, device=DEV), torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    C.bn_bwd_finalize_partials(C.ptr(part1), rows, groups, C.ptr(sums_a), C.ptr(dg_a), C.ptr(db_a), C.ptr(bws), nbn, st)
    sums_b, dg_b, db_b = torch.empty(128 * groups, device=DEV), torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    C.bn_relu_bwd_sums(C.ptr(xd), C.ptr(xbnp), C.ptr(dx1), C.ptr(sums_b), C.ptr(dg_b), C.ptr(db_b), C.ptr(bws), nbn, n * hi * hi, groups, st)
    torch.cuda.synchronize()
    for got, want in ((sums_a, sums_b), (dg_a, dg_b), (db_a, db_b)):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 2e-5 * scale, float((got - want).abs().max()) / scale
    if zero_gamma:  # those channels DID go through the companion (the activation is the constant max(shift, 0) there)
        assert float(sums_b.view(groups, 128)[:, 3].abs().min()) > 0 and float(sums_b.view(groups, 128)[:, 17].abs().max()) == 0.0
    # fp64 oracle with the decisions out of the way (docstring): EVERY element, every size
    dev_dx = (nchw(dx1).double().cpu() - dx_ref).abs() / float(dx_ref.abs().max())
    assert float(dev_dx.max()) < 1e-4, float(dev_dx.max())
    assert rel_err(dw1, dw0) < 2e-5
    assert rel_err(dw1, wr.grad) < 1e-4, rel_err(dw1, wr.grad)
    scale = float(da.abs().sum()) / 64
    assert float((db1 - db0).abs().max()) < 1e-5 * scale
    if training:  # the bias gradient of a convolution followed by train-mode BatchNorm is identically zero
        assert float(db1.abs().max()) < 1e-3 * scale
    else:
        assert rel_err(db1, br.grad) < 5e-5
    # for further checks of the caller: the moved input and its records, the fp64 gradient of the activated input and of the weights,
    # the device's results and the finalised BatchNorm-backward sums of the launch's own partial records
    return {"x": x, "xrecs": xrecs, "recs64": recs64, "dx_ref": dx_ref, "dw_ref": wr.grad, "db_ref": br.grad, "dx": dx1, "dw": dw1,
            "db": db1, "sums": sums_a, "dgamma_x": dg_a, "dbeta_x": db_a, "da": da, "desc": d}
