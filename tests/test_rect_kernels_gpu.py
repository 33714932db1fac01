"""Kernel-level parity (GPU) on RECTANGULAR maps: every spatial entry point of the auto-encoder's conv stacks — conv64 (direct, Winograd,
fused block backward, gather pipe), the two skinny layers, BatchNorm + ReLU + MaxPool, the layout transposers and the uint8 input
tail — called by name through srlz._cabi with hi != wi, both orientations of every pair, against fp64 torch-CPU ops on the same
seeded inputs.  The C ABI takes height and width separately (include/srlz.h); every other GPU test of these kernels passes one number
for both, so a kernel that used h where it meant w passed the suite.

Shape sets: the maps a 160 x 224 frame leaves in the network (conv1 160 x 224 -> 80 x 112, pooled 40 x 56, pooled 19 x 27, conv3
10 x 14, the ConvTranspose inputs 4 x 6, 9 x 13, 19 x 27, 39 x 55, 79 x 111) and their transposes; odd x even; one axis at its smallest
size; and sizes on both sides of the kernels' own tile edges: 128 grid positions per conv64 tile and the row table's second batch of
passes (a row of 80), the 2 x 2 Winograd patches, the 16 x 16 tiles of the skinny kernels, the 2 x 2 window blocks (HB x WB) of the
pool kernels, the 32 x 32 tiles of normalize_u8.  n in {1, 3, 4}, one and two BatchNorm groups wherever the descriptor has the field.

Every output is pre-filled with NaN and allocated with a sentinel-filled tail inside the same allocation (Outs): a launch that writes
w * w instead of h * w elements fails the test.  Statistics / partial records: every record must have been written (NaN pre-fill),
and every record is compared with the fp64 sums over the pixels its kernel files under it: conv64_fwd / conv64_bwd_data_pool_sums by
the tile geometry of the program (srlz_conv64_debug_program), conv64_bwd_fused's BatchNorm rows by 32-position quarters of those tiles,
the Winograd kernels by tiles of 32 patches, conv1_fwd / convT_out_bwd_data by 16 x 16 tiles, convT_out_bwd_fused by 28 x 16 strips.

Tolerances are those of the square-map tests of the same entry point in tests/test_kernels_gpu.py / test_wino_gpu.py: 2e-5 of the
reference's largest magnitude for convolutions at toy sizes, 5e-5 where a BatchNorm backward is rebuilt in the operand load, 1e-4
(BASELINE.json north_star) for the fused block backward and the whole stacks; bit-for-bit claims use torch.equal.  ReLU / max-pool
decisions are taken out of fp32-against-fp64 comparisons of gradients the way the square tests do: the reference is evaluated at the
device's own argmax (oracle.torch_twin._relu_pool pins), and dA is zeroed where the device's bn(y) lies within 1e-4 of a ReLU threshold.

Refused shapes: srlz_conv64_wino_supported refuses maps with an odd axis (asserted, both orientations);
srlz_conv64_gather_pipe_supported and srlz_conv64_bwd_fused_supported say no below 256 tiles per group / 8 tiles (asserted; the
un-fused route is then the one that is checked).  No launcher rejects a shape of these sets.  Measured figures: profiles/NOTES.md.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
TOL = 2e-5        # tests/test_kernels_gpu.py at toy sizes
TOL_BN = 5e-5     # ... where d(loss)/dy is rebuilt from (dA, y): test_fused_bn_backward_operand, test_bn_relu_pool
CEIL = 1e-4       # BASELINE.json north_star
EPS, MOM = 1e-5, 0.1
TAIL = 2048
SENT_F, SENT_B = -60000.0, 0xA5


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def C():
    from srlz import _cabi
    assert torch.cuda.is_available()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return _cabi


class Outs(object):
    """Output buffers: NaN-filled (0xEE for bytes), each followed INSIDE ITS ALLOCATION by sentinel elements that no launch may
    touch — at least TAIL, and as many as the output stretched by its largest over its smallest extent would need (new()); check() synchronises and looks at every tail."""

    def __init__(self):
        self.bufs = []

    def new(self, *shape, **kw):
        dtype = kw.get("dtype", torch.float32)
        n = int(np.prod(shape))
        # the tail covers what a launch that took one axis for another would write: the output stretched by its largest over its
        # smallest extent, rows past the end included (capped at 4 Mi elements)
        stretched = n * max(shape) // max(1, min(shape))
        tail = min(max(TAIL, stretched - n + TAIL), 1 << 22)
        buf = torch.empty(n + tail, dtype=dtype, device=DEV)
        if dtype == torch.uint8:
            buf[:n] = 0xEE
            buf[n:] = SENT_B
        else:
            buf[:n] = NAN
            buf[n:] = SENT_F
        self.bufs.append((buf, n))
        return buf[:n].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            tail = buf[n:]
            assert bool((tail == (SENT_B if buf.dtype == torch.uint8 else SENT_F)).all()), "a launch wrote behind its output (%d elements)" % n


def finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def both(pairs):
    """Every (h, w, ...) and its transpose (w, h, ...)."""
    return [c for p in pairs for c in (p, (p[1], p[0]) + tuple(p[2:]))]


def out_size(h, s, p, t):
    return (h - 1) * s - 2 * p + 3 if t else (h + 2 * p - 3) // s + 1


def records(x, groups, gen, gamma=None, beta=None):
    """Train-mode BatchNorm records {mean, invstd, scale, shift} of x [n,64,h,w] per group, fp32 as a kernel receives them
    ([groups][256]), with their (gamma, beta)."""
    per = x.shape[0] // groups
    gamma = torch.rand(64, generator=gen) + 0.5 if gamma is None else gamma
    beta = torch.randn(64, generator=gen) * 0.2 if beta is None else beta
    recs = []
    for g in range(groups):
        xs = x[g * per:(g + 1) * per].double()
        m, v = xs.mean((0, 2, 3)), xs.var((0, 2, 3), unbiased=False)
        inv = 1.0 / torch.sqrt(v + EPS)
        recs.append(torch.cat((m, inv, gamma.double() * inv, beta.double() - m * gamma.double() * inv)).float())
    return torch.stack(recs), gamma, beta


def activate(x, recs):
    """relu(scale * x + shift) per group in fp64 from the fp32 records."""
    groups = recs.shape[0]
    per = x.shape[0] // groups
    return torch.cat([F.relu(x[g * per:(g + 1) * per].double() * recs[g, 128:192].double().view(1, 64, 1, 1)
                             + recs[g, 192:].double().view(1, 64, 1, 1)) for g in range(groups)])


def off_threshold(x, recs):
    """x moved off the ReLU threshold of its records (|scale * x + shift| >= 2e-3): fp32 and fp64 then take the same decisions."""
    groups = recs.shape[0]
    per = x.shape[0] // groups
    x = x.clone()
    for g in range(groups):
        sc, sh = recs[g, 128:192].double().view(1, 64, 1, 1), recs[g, 192:].double().view(1, 64, 1, 1)
        xs = x[g * per:(g + 1) * per].double()
        z = xs * sc + sh
        xs = torch.where(z.abs() < 2e-3, (torch.where(z >= 0, 2.5e-3, -2.5e-3) - sh) / sc, xs)
        x[g * per:(g + 1) * per] = xs.float()
        assert float((x[g * per:(g + 1) * per].double() * sc + sh).abs().min()) > 1e-3
    return x


def conv_ref(a, w, b, s, p, t):
    return F.conv_transpose2d(a, w, b, stride=s, padding=p) if t else F.conv2d(a, w, b, stride=s, padding=p)


def pack64(C, w, d):
    wd = w.to(DEV)
    packs = torch.full((2, C.conv64_packed_floats()), NAN, device=DEV)
    C.conv64_pack_weights(C.ptr(wd), C.ptr(packs[0]), C.ptr(packs[1]), d, C.stream())
    return packs


def program(C, d, backward):
    buf = (ctypes.c_int * 64)()
    assert C.conv64_debug_program(d, backward, buf, 64) == 48, C.error_text()
    return dict(zip(["N", "PH", "PW", "ss", "Hs", "Ws", "ds", "Hd", "Wd", "min_off", "span", "s2"], list(buf)[:12]))


def _pixels(n, H, W):
    return torch.arange(n).view(n, 1, 1), torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)


def tiles_program(P, n, groups, positions=128):
    """Record index of every destination pixel [n,Hd,Wd] of a conv64 program: grid position q = image * PH * PW + (oy // ds) * PW +
    (ox // ds) of a group's virtual grid, `positions` consecutive positions per record, a group's records (tiles of 128 positions,
    rounded up) behind the previous group's."""
    per = n // groups
    assert per == P["N"]
    rpg = (per * P["PH"] * P["PW"] + 127) // 128 * (128 // positions)
    img, oy, ox = _pixels(n, P["Hd"], P["Wd"])
    q = (img % per) * (P["PH"] * P["PW"]) + (oy // P["ds"]) * P["PW"] + (ox // P["ds"])
    return (img // per) * rpg + q // positions, rpg


def tiles_skinny(n, hf, wf):
    """csrc/skinny.hip: 16 x 16 tiles of the feature map, row-major inside an image, image after image."""
    ty, tx = (hf + 15) // 16, (wf + 15) // 16
    img, oy, ox = _pixels(n, hf, wf)
    return img * (ty * tx) + (oy // 16) * tx + ox // 16


def tiles_wino(n, h, w, groups, rows_per_group):
    """csrc/wino.hip: 2 x 2 patches in row-major order inside an image (h / 2 rows of w / 2), image after image inside a group,
    32 patches per record; a group owns rows_per_group records."""
    per = n // groups
    img, oy, ox = _pixels(n, h, w)
    patch = (img % per) * ((h // 2) * (w // 2)) + (oy // 2) * (w // 2) + ox // 2
    return (img // per) * rows_per_group + patch // 32


def tiles_convT_fused(n, hf, wf):
    """csrc/convt_out.hip, backward: strips of 28 feature rows x 16 columns, record = (image * strips down + strip row) * strips
    across + strip column."""
    nseg, nchunk = (wf + 15) // 16, (hf + 27) // 28
    img, oy, ox = _pixels(n, hf, wf)
    return (img * nchunk + oy // 28) * nseg + ox // 16


def records_by_tile(tile, nrec, v1, v2):
    """Reference records [nrec][128] = per record the sums of v1 and of v2 ([n,64,H,W], fp64) over the pixels `tile` ([n,H,W]) files
    under it, and the same sums of magnitudes (the error scale)."""
    t = tile.expand(v1.shape[0], v1.shape[2], v1.shape[3]).reshape(-1)
    assert int(t.min()) >= 0 and int(t.max()) < nrec
    f1, f2 = v1.permute(0, 2, 3, 1).reshape(-1, 64), v2.permute(0, 2, 3, 1).reshape(-1, 64)
    ref = torch.zeros(nrec, 128, dtype=torch.float64)
    mag = torch.zeros(nrec, 128, dtype=torch.float64)
    ref[:, :64].index_add_(0, t, f1)
    ref[:, 64:].index_add_(0, t, f2)
    mag[:, :64].index_add_(0, t, f1.abs())
    mag[:, 64:].index_add_(0, t, f2.abs())
    return ref, mag


def record_refs(P, y, groups, ntiles):
    """Per-tile (sum, sum of squares) records of y [n,64,Hd,Wd] (fp64) as the program tiles it."""
    assert tuple(y.shape[2:]) == (P["Hd"], P["Wd"])
    tile, tpg = tiles_program(P, y.shape[0], groups)
    assert ntiles == groups * tpg
    return records_by_tile(tile, ntiles, y, y * y)


def bn_bwd_values(da, x, recs):
    """(dz, dz * xhat) of a BatchNorm + ReLU backward per group: dz = dA where relu(bn(x)) passes, xhat = (x - mean) * invstd of the
    group's record — what a data-gradient epilogue sums into its partial records."""
    groups = recs.shape[0]
    per = x.shape[0] // groups
    dz, dzx = [], []
    for g in range(groups):
        xs = x[g * per:(g + 1) * per].double()
        r = recs[g].double()
        pos = (xs * r[128:192].view(1, 64, 1, 1) + r[192:].view(1, 64, 1, 1)) > 0
        d = da[g * per:(g + 1) * per].double() * pos
        dz.append(d)
        dzx.append(d * (xs - r[:64].view(1, 64, 1, 1)) * r[64:128].view(1, 64, 1, 1))
    return torch.cat(dz), torch.cat(dzx)


def check_records(stats, ref, mag, tol=TOL):
    """Every record: sums within tol of the largest per-record sum of magnitudes (a sum's own value may cancel to nothing)."""
    got = stats.double().cpu()
    assert finite(got)
    e_s = float((got[:, :64] - ref[:, :64]).abs().max()) / float(mag[:, :64].max())
    e_q = float((got[:, 64:] - ref[:, 64:]).abs().max()) / float(mag[:, 64:].max())
    assert e_s < tol and e_q < tol, (e_s, e_q)
    return max(e_s, e_q)


def finalize_partials(C, part, groups):
    sums, dg, db = torch.full((128 * groups,), NAN, device=DEV), torch.full((64,), NAN, device=DEV), torch.full((64,), NAN, device=DEV)
    nb = C.bn_bwd_workspace(0)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    C.bn_bwd_finalize_partials(C.ptr(part), part.shape[0], groups, C.ptr(sums), C.ptr(dg), C.ptr(db), C.ptr(ws), nb, C.stream())
    torch.cuda.synchronize()
    return sums, dg, db


# ---------------------------------------------------------------------------------------------------------------------------------
# A. conv64: forward, data gradient, weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
# (hi, wi, stride, pad, transposed, n, groups); every case also runs transposed in space (wi, hi)
CONV64_RECT = both([
    (40, 56, 1, 1, 0, 3, 1), (19, 27, 2, 1, 0, 4, 2), (10, 14, 1, 1, 0, 4, 2),                 # conv2, conv3, conv3's output map
    (4, 6, 2, 0, 1, 4, 2), (9, 13, 2, 0, 1, 3, 1), (19, 27, 2, 0, 1, 4, 2), (39, 55, 2, 0, 1, 1, 1),   # the four ConvTranspose blocks
    (9, 80, 1, 1, 0, 1, 1),      # a row of 80: 128 + 2 * 82 + 2 staged rows, the row table's second batch of passes; 9 rows the other way
    (3, 8, 2, 1, 0, 3, 1), (3, 8, 2, 0, 1, 4, 2), (7, 12, 1, 1, 0, 4, 1),                        # odd x even
    (1, 5, 1, 1, 0, 4, 2), (1, 5, 2, 0, 1, 3, 1), (2, 9, 2, 1, 0, 1, 1),                         # one axis at its minimum
    (5, 25, 1, 1, 0, 1, 1),      # 5 x 27 = 135 grid positions: one tile and seven positions of the next
    (8, 21, 2, 0, 0, 4, 2), (6, 11, 2, 1, 1, 3, 1),                                              # unpadded stride 2, padded ConvTranspose
])


def _id64(c):
    return "%dx%d_s%dp%dt%d_n%dg%d" % c


@pytest.mark.parametrize("case", CONV64_RECT, ids=_id64)
def test_conv64_rect_forward_backward(C, case):
    """srlz_conv64_fwd (no bias + statistics record by record; bias; the fused relu(bn(x)) operand x_bnp), srlz_conv64_bwd_data
    (plain), srlz_conv64_bwd_weight (plain; x_bnp + dbias) against fp64 F.conv2d / F.conv_transpose2d and autograd; second launches
    bit for bit; srlz_conv64_gather_pipe_supported says no at these sizes (fewer than 256 tiles per group), so the synchronous kernel is
    what is checked here (the pipelined one: test_conv64_rect_gather_pipe)."""
    hi, wi, s, p, t, n, G = case
    ho, wo = out_size(hi, s, p, t), out_size(wi, s, p, t)
    gen = torch.Generator().manual_seed(hi * 131 + wi * 17 + s * 5 + p * 3 + t)
    x = torch.randn(n, 64, hi, wi, generator=gen)
    x[:, :, 0, :] += 1.0     # (the borders carry a signal of their own: a wrong padding mask or a swapped axis shows)
    x[:, :, :, -1] -= 1.0
    w = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    b = torch.randn(64, generator=gen)
    dy = torch.randn(n, 64, ho, wo, generator=gen)
    recs, _, _ = records(x, G, gen)
    # fp64 references
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_plain = conv_ref(xr, wr, None, s, p, t)
    y_plain.backward(dy.double())
    act = activate(x, recs)
    wr2 = w.double().requires_grad_(True)
    y_fused = conv_ref(act, wr2, b.double(), s, p, t)
    y_fused.backward(dy.double())
    assert tuple(y_plain.shape) == (n, 64, ho, wo)

    d = C.Conv64Desc(n, hi, wi, ho, wo, 3, s, p, t, G)
    assert C.conv64_gather_pipe_supported(d, 0) == 0 and C.conv64_gather_pipe_supported(d, 1) == 0
    st = C.stream()
    xd, dyd, bd, rd = nhwc(x).to(DEV), nhwc(dy).to(DEV), b.to(DEV), recs.to(DEV)
    packs = pack64(C, w, d)
    ntiles = C.conv64_fwd_tiles(d)
    P = program(C, d, 0)
    o = Outs()
    y0, s0 = o.new(n, ho, wo, 64), o.new(ntiles, 128)
    C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), None, C.ptr(y0), C.ptr(s0), None, d, st)
    y1 = o.new(n, ho, wo, 64)
    C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), C.ptr(bd), C.ptr(y1), None, None, d, st)
    y2, s2 = o.new(n, ho, wo, 64), o.new(ntiles, 128)
    C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), C.ptr(bd), C.ptr(y2), C.ptr(s2), C.ptr(rd), d, st)
    y3, s3 = o.new(n, ho, wo, 64), o.new(ntiles, 128)
    C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), None, C.ptr(y3), C.ptr(s3), None, d, st)
    dx = o.new(n, hi, wi, 64)
    C.conv64_bwd_data(C.ptr(dyd), C.ptr(packs[1]), C.ptr(dx), None, d, st)
    nb = C.conv64_bwd_weight_workspace(d)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dw0 = o.new(64, 64, 3, 3)
    C.conv64_bwd_weight(C.ptr(xd), C.ptr(dyd), C.ptr(dw0), None, None, None, C.ptr(ws), nb, d, st)
    dw1, db1 = o.new(64, 64, 3, 3), o.new(64)
    C.conv64_bwd_weight(C.ptr(xd), C.ptr(dyd), C.ptr(dw1), C.ptr(db1), C.ptr(rd), None, C.ptr(ws), nb, d, st)
    dw2, db2 = o.new(64, 64, 3, 3), o.new(64)
    ws.fill_(255)
    C.conv64_bwd_weight(C.ptr(xd), C.ptr(dyd), C.ptr(dw2), C.ptr(db2), C.ptr(rd), None, C.ptr(ws), nb, d, st)
    o.check()
    assert finite(packs, y0, y1, y2, dx, dw0, dw1, db1)
    errs = {"fwd": rel_err(nchw(y0), y_plain), "fwd+bias": rel_err(nchw(y1), y_plain.detach() + b.double().view(1, 64, 1, 1)),
            "fwd+x_bnp": rel_err(nchw(y2), y_fused), "bwd_data": rel_err(nchw(dx), xr.grad), "bwd_weight": rel_err(dw0, wr.grad),
            "bwd_weight+x_bnp": rel_err(dw1, wr2.grad), "dbias": rel_err(db1, dy.double().sum((0, 2, 3)))}
    errs["stats"] = check_records(s0, *record_refs(P, y_plain.detach(), G, ntiles))
    errs["stats+x_bnp"] = check_records(s2, *record_refs(P, y_fused.detach(), G, ntiles))
    print("conv64 %s: %s" % (_id64(case), " ".join("%s %.1e" % kv for kv in sorted(errs.items()))))
    assert all(e < TOL for e in errs.values()), errs
    assert torch.equal(y3, y0) and torch.equal(s3, s0)                       # two runs
    assert torch.equal(dw2, dw1) and torch.equal(db2, db1)                   # fixed-order split-K reduction


# (hi, wi, stride, pad, transposed, n, groups, training)
BNOP_RECT = both([(4, 6, 2, 0, 1, 4, 2, 1), (9, 13, 2, 0, 1, 4, 2, 1), (13, 19, 2, 0, 1, 4, 1, 1), (19, 27, 2, 0, 1, 4, 2, 1),
                  (3, 8, 2, 0, 1, 3, 1, 1), (10, 14, 1, 1, 0, 3, 1, 1), (19, 27, 2, 1, 0, 4, 2, 1), (13, 19, 2, 0, 1, 4, 2, 0)])


@pytest.mark.parametrize("case", BNOP_RECT, ids=lambda c: "%dx%d_s%dp%dt%d_n%dg%d_train%d" % c)
def test_conv64_rect_bn_backward_operand_and_fused_block_backward(C, case):
    """relu(bn(x)) -> conv / ConvTranspose (+ bias) -> BatchNorm -> ReLU, backward from dA on a rectangular map:
    srlz_conv64_bwd_data with srlz_bn_bwd_operand (d(loss)/dy rebuilt in the operand load, dy_out written exactly once per element),
    srlz_conv64_bwd_weight(x_bnp) on that dy_out with dbias, against fp64 autograd per BatchNorm group (5e-5, the bar of
    test_fused_bn_backward_operand); and for stride-2 ConvTranspose layers srlz_conv64_bwd_fused where
    srlz_conv64_bwd_fused_supported says yes — dx bit-identical to the two launches, dw / db to rounding, 1e-4 against fp64, its
    BatchNorm-backward records of the INPUT's BatchNorm through srlz_bn_bwd_finalize_partials against srlz_bn_relu_bwd_sums, a second
    launch bit for bit — and, where it says no (fewer than 8 tiles), the refusal of the launcher."""
    hi, wi, s, p, t, n, G, training = case
    ho, wo = out_size(hi, s, p, t), out_size(wi, s, p, t)
    per = n // G
    gen = torch.Generator().manual_seed(7 * hi + 1000 * wi + n)
    x = torch.randn(n, 64, hi, wi, generator=gen) * 1.2 + 0.1
    w, b = torch.randn(64, 64, 3, 3, generator=gen) * 0.05, torch.randn(64, generator=gen) * 0.1
    xrecs, _, _ = records(x, G, gen)
    x = off_threshold(x, xrecs)
    gamma, beta = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.2
    rm, rv = torch.randn(64, generator=gen) * 0.1, torch.rand(64, generator=gen) + 0.5
    da = torch.randn(n, 64, ho, wo, generator=gen)

    st = C.stream()
    d = C.Conv64Desc(n, hi, wi, ho, wo, 3, s, p, t, G)
    xd, bd, xbnp = nhwc(x).to(DEV), b.to(DEV), xrecs.to(DEV)
    packs = pack64(C, w, d)
    o = Outs()
    ntiles = C.conv64_fwd_tiles(d)
    y, stats = o.new(n, ho, wo, 64), o.new(ntiles, 128)
    C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), C.ptr(bd), C.ptr(y), C.ptr(stats), C.ptr(xbnp), d, st)
    gd, bed, rmd, rvd = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
    nbn = C.bn_bwd_workspace(0)
    bws = torch.empty(nbn, dtype=torch.uint8, device=DEV)
    if training:
        bnp, bstat = o.new(256 * G), o.new(128 * G)
        C.bn_finalize(C.ptr(stats), ntiles, G, per * ho * wo, C.ptr(gd), C.ptr(bed), EPS, MOM, 1, C.ptr(rmd), C.ptr(rvd), None, C.ptr(bnp),
                      C.ptr(bstat), C.ptr(bws), nbn, st)
    else:
        one = o.new(256)
        C.bn_eval_params(C.ptr(gd), C.ptr(bed), C.ptr(rmd), C.ptr(rvd), EPS, C.ptr(one), st)
        torch.cuda.synchronize()
        bnp = one.repeat(G)
    torch.cuda.synchronize()
    assert finite(y, stats, bnp)
    # dA = 0 wherever the device's bn(y) lies within 1e-4 of the ReLU threshold (either decision then multiplies a zero)
    rec_y = bnp.view(G, 256).double().cpu()
    zy = nchw(y).double().cpu().view(G, per, 64, ho, wo) * rec_y[:, 128:192].view(G, 1, 64, 1, 1) + rec_y[:, 192:].view(G, 1, 64, 1, 1)
    tie = (zy.abs() < 1e-4).view(n, 64, ho, wo)
    da = torch.where(tie, torch.zeros(()), da)
    dad = nhwc(da).to(DEV)
    # fp64 reference per group
    wr, br, gr, ber = (v.double().requires_grad_(True) for v in (w, b, gamma, beta))
    dx_ref, dy_ref, y_ref = [], [], []
    for g in range(G):
        a = activate(x[g * per:(g + 1) * per], xrecs[g:g + 1]).requires_grad_(True)
        yr = conv_ref(a, wr, br, s, p, t)
        yr.retain_grad()
        zr = F.batch_norm(yr, rm.double().clone(), rv.double().clone(), gr, ber, bool(training), MOM, EPS)
        assert bool((((zr > 0) == (zy[g] > 0)) | tie[g * per:(g + 1) * per]).all())
        F.relu(zr).backward(da[g * per:(g + 1) * per].double())
        dx_ref.append(a.grad)
        dy_ref.append(yr.grad)
        y_ref.append(yr.detach())
    dx_ref, dy_ref, y_ref = torch.cat(dx_ref), torch.cat(dy_ref), torch.cat(y_ref)
    assert rel_err(nchw(y), y_ref) < TOL
    check_records(stats, *record_refs(program(C, d, 0), y_ref, G, ntiles))

    sums, dgm, dbt = o.new(128 * G), o.new(64), o.new(64)
    C.bn_relu_bwd_sums(C.ptr(y), C.ptr(bnp), C.ptr(dad), C.ptr(sums), C.ptr(dgm), C.ptr(dbt), C.ptr(bws), nbn, n * ho * wo, G, st)
    dy_out, dx0 = o.new(n, ho, wo, 64), o.new(n, hi, wi, 64)
    op = C.BnBwdOperand(y.data_ptr(), bnp.data_ptr(), sums.data_ptr(), per * ho * wo, training, dy_out.data_ptr())
    C.conv64_bwd_data(C.ptr(dad), C.ptr(packs[1]), C.ptr(dx0), op, d, st)
    nb = C.conv64_bwd_weight_workspace(d)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dw0, db0 = o.new(64, 64, 3, 3), o.new(64)
    C.conv64_bwd_weight(C.ptr(xd), C.ptr(dy_out), C.ptr(dw0), C.ptr(db0), C.ptr(xbnp), None, C.ptr(ws), nb, d, st)
    o.check()
    assert finite(sums, dgm, dbt, dy_out, dx0, dw0, db0)
    if training:
        assert rel_err(dgm, gr.grad) < TOL_BN and rel_err(dbt, ber.grad) < TOL_BN
    e = {"dx": rel_err(nchw(dx0), dx_ref), "dy_out": rel_err(nchw(dy_out), dy_ref), "dw": rel_err(dw0, wr.grad)}
    print("conv64 bn operand %r: %s" % (case, e))
    assert all(v < TOL_BN for v in e.values()), e
    scale = float(da.abs().sum()) / 64
    if training:  # the bias gradient of a convolution followed by train-mode BatchNorm is identically zero
        assert float(db0.abs().max()) < 1e-3 * scale
    else:
        assert rel_err(db0, br.grad) < TOL_BN

    if not (t and s == 2):
        return
    op1 = C.BnBwdOperand(y.data_ptr(), bnp.data_ptr(), sums.data_ptr(), per * ho * wo, training, None)
    nb1 = C.conv64_bwd_fused_workspace(d)
    ws1 = torch.full((max(nb1 // 4, 1),), NAN, device=DEV)
    rows = C.conv64_bwd_fused_bn_rows(d)
    o2 = Outs()
    dx1, dw1, db1, part1 = o2.new(n, hi, wi, 64), o2.new(64, 64, 3, 3), o2.new(64), o2.new(rows, 128)
    if C.conv64_bwd_fused_supported(d) == 0:
        P = program(C, d, 1)
        assert G * ((per * P["PH"] * P["PW"] + 127) // 128) < 8   # the documented reason: fewer than 8 tiles
        with pytest.raises(C.SrlzError):
            C.conv64_bwd_fused(C.ptr(xd), C.ptr(xbnp), C.ptr(dad), op1, C.ptr(packs[1]), C.ptr(dx1), C.ptr(dw1), C.ptr(db1), C.ptr(part1),
                               C.ptr(ws1), nb1, d, st)
        o2.check()
        assert bool(torch.isnan(dx1).all())  # nothing was launched; the two launches above are the route, and they are right
        return
    C.conv64_bwd_fused(C.ptr(xd), C.ptr(xbnp), C.ptr(dad), op1, C.ptr(packs[1]), C.ptr(dx1), C.ptr(dw1), C.ptr(db1), C.ptr(part1), C.ptr(ws1),
                       nb1, d, st)
    dx2, dw2, db2, part2 = o2.new(n, hi, wi, 64), o2.new(64, 64, 3, 3), o2.new(64), o2.new(rows, 128)
    C.conv64_bwd_fused(C.ptr(xd), C.ptr(xbnp), C.ptr(dad), op1, C.ptr(packs[1]), C.ptr(dx2), C.ptr(dw2), C.ptr(db2), C.ptr(part2), C.ptr(ws1),
                       nb1, d, st)
    o2.check()
    assert finite(dx1, dw1, db1, part1)
    assert torch.equal(dx1, dx0)                                              # the fused launch is the two launches
    assert torch.equal(dx2, dx1) and torch.equal(dw2, dw1) and torch.equal(db2, db1) and torch.equal(part2, part1)
    assert rel_err(dw1, dw0) < TOL and float((db1 - db0).abs().max()) < 1e-5 * scale
    assert rel_err(nchw(dx1), dx_ref) < CEIL and rel_err(dw1, wr.grad) < CEIL
    # the BatchNorm-backward records of the layer that produced x, record by record: a tile's four wave rows file 32 grid positions each
    # under records 4 * tile .. 4 * tile + 3 of the group; the group's last records belong to the companion launch for channels without a
    # usable scale (none here: zeros)
    Pb = program(C, d, 1)
    rec_of, rpg = tiles_program(Pb, n, G, positions=32)
    assert rows % G == 0 and rows // G >= rpg
    rec_of = rec_of + (rec_of // rpg) * (rows // G - rpg)
    check_records(part1, *records_by_tile(rec_of, rows, *bn_bwd_values(dx_ref, x, xrecs)), tol=TOL_BN)
    sa = finalize_partials(C, part1, G)
    sb = [torch.full((k,), NAN, device=DEV) for k in (128 * G, 64, 64)]
    C.bn_relu_bwd_sums(C.ptr(xd), C.ptr(xbnp), C.ptr(dx1), C.ptr(sb[0]), C.ptr(sb[1]), C.ptr(sb[2]), C.ptr(bws), nbn, n * hi * wi, G, st)
    torch.cuda.synchronize()
    for got, want in zip(sa, sb):
        assert finite(got) and float((got - want).abs().max()) <= TOL * float(want.abs().max())
    # ... and in fp64: sum dA * [bn(x) > 0] and sum dA * [bn(x) > 0] * xhat per group
    for g in range(G):
        xs = x[g * per:(g + 1) * per].double()
        m, inv = xrecs[g, :64].double().view(1, 64, 1, 1), xrecs[g, 64:128].double().view(1, 64, 1, 1)
        pos = (xs * xrecs[g, 128:192].double().view(1, 64, 1, 1) + xrecs[g, 192:].double().view(1, 64, 1, 1)) > 0
        dz = dx_ref[g * per:(g + 1) * per] * pos
        want = torch.cat((dz.sum((0, 2, 3)), (dz * (xs - m) * inv).sum((0, 2, 3))))
        assert rel_err(sa[0][128 * g:128 * (g + 1)], want) < CEIL


@pytest.mark.parametrize("hi,wi,t,n,G", [(19, 27, 0, 240, 1), (27, 19, 0, 480, 2), (9, 13, 1, 240, 1), (13, 9, 1, 480, 2)])
def test_conv64_rect_gather_pipe(C, hi, wi, t, n, G):
    """conv64_gather_pipe_kernel (from 256 tiles per BatchNorm group on: a batch of small maps, not a large map) on the rectangular
    conv3 (19 x 27 -> 10 x 14) and on the data gradient of the ConvTranspose 9 x 13 -> 19 x 27, both orientations: bit-identical to the
    synchronous kernel (which takes the program when a zero bias is given), every element against fp64, statistics per group."""
    s, p = 2, (0 if t else 1)
    ho, wo = out_size(hi, s, p, t), out_size(wi, s, p, t)
    gen = torch.Generator().manual_seed(n + hi)
    w = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    d = C.Conv64Desc(n, hi, wi, ho, wo, 3, s, p, t, G)
    assert C.conv64_gather_pipe_supported(d, 1 if t else 0) == 1
    assert C.conv64_gather_pipe_supported(C.Conv64Desc(4 * G, hi, wi, ho, wo, 3, s, p, t, G), 1 if t else 0) == 0
    st = C.stream()
    packs = pack64(C, w, d)
    o = Outs()
    if not t:
        x = torch.randn(n, 64, hi, wi, generator=gen)
        ref = F.conv2d(x.double(), w.double(), None, stride=2, padding=1)
        xd = nhwc(x).to(DEV)
        tiles = C.conv64_fwd_tiles(d)
        zero = torch.zeros(64, device=DEV)
        ya, sa, yb, sb, yc = o.new(n, ho, wo, 64), o.new(tiles, 128), o.new(n, ho, wo, 64), o.new(tiles, 128), o.new(n, ho, wo, 64)
        C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), None, C.ptr(ya), C.ptr(sa), None, d, st)
        C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), C.ptr(zero), C.ptr(yb), C.ptr(sb), None, d, st)
        C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), None, C.ptr(yc), None, None, d, st)
        o.check()
        assert finite(ya, sa) and torch.equal(ya, yb) and torch.equal(yc, ya)
        assert float((sa.double() - sb.double()).abs().max()) <= 1e-5 * float(sb.double().abs().max())
        e = rel_err(nchw(ya), ref)
        check_records(sa, *record_refs(program(C, d, 0), ref, G, tiles))
    else:
        dy = torch.randn(n, 64, ho, wo, generator=gen)
        xr = torch.zeros(n, 64, hi, wi, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(xr, w.double(), None, stride=2).backward(dy.double())
        dyd = nhwc(dy).to(DEV)
        dx, dx2 = o.new(n, hi, wi, 64), o.new(n, hi, wi, 64)
        C.conv64_bwd_data(C.ptr(dyd), C.ptr(packs[1]), C.ptr(dx), None, d, st)
        C.conv64_bwd_data(C.ptr(dyd), C.ptr(packs[1]), C.ptr(dx2), None, d, st)
        o.check()
        assert finite(dx) and torch.equal(dx, dx2)
        # the synchronous kernel on the first images alone, below the pipe's threshold
        per = 8
        ds = C.Conv64Desc(per, hi, wi, ho, wo, 3, s, p, t, 1)
        assert C.conv64_gather_pipe_supported(ds, 1) == 0
        dxs = o.new(per, hi, wi, 64)
        C.conv64_bwd_data(C.ptr(dyd[:per].contiguous()), C.ptr(packs[1]), C.ptr(dxs), None, ds, st)
        o.check()
        assert rel_err(dxs, dx[:per]) < 2e-6   # (rounding order at most)
        e = rel_err(nchw(dx), xr.grad)
    print("gather pipe %dx%d t=%d n=%d: %.2e" % (hi, wi, t, n, e))
    assert e < TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# B. Winograd F(2x2, 3x3)
# ---------------------------------------------------------------------------------------------------------------------------------
WINO_RECT = both([(40, 56, 3, 1), (10, 14, 4, 2), (4, 6, 4, 2), (4, 18, 1, 1), (6, 34, 3, 1), (8, 12, 4, 1), (20, 28, 4, 2)])


@pytest.mark.parametrize("h,w_,n,G", WINO_RECT, ids=lambda v: str(v))
def test_conv64_wino_rect(C, h, w_, n, G):
    """srlz_conv64_wino_fwd (bias / none, statistics, x_bnp), srlz_conv64_wino_bwd_data, srlz_conv64_wino_bwd_weight on even
    h != w >= 4 against fp64 F.conv2d and autograd at the 2e-5 of tests/test_wino_gpu.py; second launches bit for bit."""
    gen = torch.Generator().manual_seed(h * 37 + w_)
    x = torch.randn(n, 64, h, w_, generator=gen)
    x[:, :, 0, :] += 1.5
    x[:, :, :, -1] -= 1.5
    w = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    b = torch.randn(64, generator=gen)
    dy = torch.randn(n, 64, h, w_, generator=gen)
    recs, _, _ = records(x, G, gen)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, 1, 1)
    y_ref.backward(dy.double())
    y_fused = F.conv2d(activate(x, recs), w.double(), b.double(), 1, 1)
    d = C.Conv64Desc(n, h, w_, h, w_, 3, 1, 1, 0, G)
    assert C.conv64_wino_supported(d) == 1
    st = C.stream()
    xd, wd, bd, dyd, rd = nhwc(x).to(DEV), w.to(DEV), b.to(DEV), nhwc(dy).to(DEV), recs.to(DEV)
    up = torch.full((2, C.conv64_wino_packed_floats()), NAN, device=DEV)
    C.conv64_wino_pack_weights(C.ptr(wd), C.ptr(up[0]), C.ptr(up[1]), st)
    rows = C.conv64_wino_tiles(d)
    assert rows > 0 and rows % G == 0
    o = Outs()
    y0, s0, y1, s1, y2 = o.new(n, h, w_, 64), o.new(rows, 128), o.new(n, h, w_, 64), o.new(rows, 128), o.new(n, h, w_, 64)
    C.conv64_wino_fwd(C.ptr(xd), C.ptr(up[0]), None, C.ptr(y0), C.ptr(s0), None, d, st)
    C.conv64_wino_fwd(C.ptr(xd), C.ptr(up[0]), C.ptr(bd), C.ptr(y1), C.ptr(s1), C.ptr(rd), d, st)
    C.conv64_wino_fwd(C.ptr(xd), C.ptr(up[0]), None, C.ptr(y2), None, None, d, st)
    dx = o.new(n, h, w_, 64)
    C.conv64_wino_bwd_data(C.ptr(dyd), C.ptr(up[1]), C.ptr(dx), d, st)
    nb = C.conv64_wino_bwd_weight_workspace(d)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dw, dw2 = o.new(64, 64, 3, 3), o.new(64, 64, 3, 3)
    C.conv64_wino_bwd_weight(C.ptr(xd), C.ptr(dyd), C.ptr(dw), C.ptr(ws), nb, d, st)
    ws.fill_(255)
    C.conv64_wino_bwd_weight(C.ptr(xd), C.ptr(dyd), C.ptr(dw2), C.ptr(ws), nb, d, st)
    o.check()
    assert finite(up, y0, s0, y1, s1, dx, dw)
    e = {"fwd": rel_err(nchw(y0), y_ref), "fwd+bias+x_bnp": rel_err(nchw(y1), y_fused), "bwd_data": rel_err(nchw(dx), xr.grad),
         "bwd_weight": rel_err(dw, wr.grad)}
    tile = tiles_wino(n, h, w_, G, rows // G)
    e["stats"] = check_records(s0, *records_by_tile(tile, rows, y_ref.detach(), y_ref.detach() ** 2))
    e["stats+x_bnp"] = check_records(s1, *records_by_tile(tile, rows, y_fused, y_fused ** 2))
    print("wino %dx%d n=%d g=%d: %s" % (h, w_, n, G, " ".join("%s %.1e" % kv for kv in sorted(e.items()))))
    assert all(v < TOL for v in e.values()), e
    assert torch.equal(y2, y0) and torch.equal(dw2, dw)


@pytest.mark.parametrize("h,w_", both([(5, 6), (4, 7), (39, 56), (2, 6)]))
def test_conv64_wino_refuses_a_map_with_an_odd_or_too_small_axis(C, h, w_):
    """One odd axis (either one) or an axis below 4: srlz_conv64_wino_supported says no, the launchers refuse, and the direct kernel
    takes the layer (what ops.Conv64Fn does) with the right answer."""
    n = 2
    d = C.Conv64Desc(n, h, w_, h, w_, 3, 1, 1, 0, 1)
    if min(h, w_) >= 4:
        assert (h % 2) + (w_ % 2) == 1
    assert C.conv64_wino_supported(d) == 0
    gen = torch.Generator().manual_seed(h + 10 * w_)
    x, w = torch.randn(n, 64, h, w_, generator=gen), torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    xd, wd = nhwc(x).to(DEV), w.to(DEV)
    up = torch.empty(2, C.conv64_wino_packed_floats(), device=DEV)
    C.conv64_wino_pack_weights(C.ptr(wd), C.ptr(up[0]), C.ptr(up[1]), C.stream())
    o = Outs()
    y = o.new(n, h, w_, 64)
    with pytest.raises(C.SrlzError):
        C.conv64_wino_fwd(C.ptr(xd), C.ptr(up[0]), None, C.ptr(y), None, None, d, C.stream())
    with pytest.raises(C.SrlzError):
        C.conv64_wino_bwd_data(C.ptr(xd), C.ptr(up[1]), C.ptr(y), d, C.stream())
    o.check()
    assert bool(torch.isnan(y).all())
    packs = pack64(C, w, d)
    C.conv64_fwd(C.ptr(xd), C.ptr(packs[0]), None, C.ptr(y), None, None, d, C.stream())
    o.check()
    assert rel_err(nchw(y), F.conv2d(x.double(), w.double(), None, 1, 1)) < TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# C. BatchNorm + ReLU + MaxPool(3, 2), alone and linked to the next convolution's data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def pool_out(h, pad):
    return (h + 2 * pad - 3) // 2 + 1


def pinned_pool(z, arg, pooled_pos, w, pad):
    """relu + max-pool of z [n,64,h,w] at the DEVICE's argmax bytes [n,hp,wp,64] (window index ky * 3 + kx)."""
    from oracle import torch_twin as T
    a = arg.long().cpu().permute(0, 3, 1, 2)
    hp, wp = a.shape[2], a.shape[3]
    py, px = torch.arange(hp).view(1, 1, hp, 1), torch.arange(wp).view(1, 1, 1, wp)
    iy, ix = py * 2 - pad + a // 3, px * 2 - pad + a % 3
    assert bool(((iy >= 0) & (iy < z.shape[2]) & (ix >= 0) & (ix < w)).all()), "an argmax points outside the map"
    return T._relu_pool(z, 3, 2, pad, (iy * w + ix, pooled_pos))


# (h, w, pool_pad, out_nchw, n, groups, training, stride of the next convolution or 0 = none)
POOL_RECT = both([(80, 112, 1, 0, 1, 1, 1, 1), (40, 56, 0, 0, 4, 2, 1, 2), (10, 14, 0, 1, 4, 2, 1, 0), (10, 14, 0, 1, 3, 1, 0, 0),
                  (7, 12, 1, 0, 4, 2, 1, 1), (3, 9, 0, 0, 3, 1, 1, 1), (5, 8, 0, 0, 4, 2, 1, 2), (4, 11, 1, 1, 4, 1, 1, 0),
                  (15, 22, 1, 0, 4, 2, 0, 1), (9, 35, 0, 0, 1, 1, 1, 2)])


@pytest.mark.parametrize("case", POOL_RECT, ids=lambda c: "%dx%d_pad%d_nchw%d_n%dg%d_train%d_next%d" % c)
def test_bn_relu_pool_rect(C, case):
    """srlz_bn_relu_pool_fwd (pad 0 / 1, NHWC / NCHW output, argmax), srlz_bn_relu_pool_bwd, srlz_bn_relu_pool_bwd_sums +
    srlz_bn_relu_pool_bwd_apply on h != w, one and two BatchNorm groups; and with a 3x3 convolution behind the pooled map
    srlz_conv64_bwd_data_pool_sums (+ srlz_conv64_wino_bwd_data_pool_sums where Winograd takes the layer) followed by
    srlz_bn_bwd_finalize_partials.  Reference: fp64 batch_norm -> relu -> max_pool2d (-> conv2d) per group; the backward is
    evaluated at the device's own argmax (two correct evaluations may break a max-pool near-tie differently), which itself must pick
    the window maximum."""
    h, w_, pad, out_nchw, n, G, training, nxt = case
    hp, wp = pool_out(h, pad), pool_out(w_, pad)
    per = n // G
    gen = torch.Generator().manual_seed(h * 11 + w_ * 5 + pad)
    y = torch.randn(n, 64, h, w_, generator=gen) * 1.7 + 0.3
    y[:, :, :, 0] += 0.8
    y[:, :, -1, :] -= 0.8
    rm, rv = torch.randn(64, generator=gen) * 0.1, torch.rand(64, generator=gen) + 0.5
    if training:
        recs, gamma, beta = records(y, G, gen)
    else:
        gamma, beta = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.2
        inv = 1.0 / torch.sqrt(rv.double() + EPS)
        one = torch.cat((rm.double(), inv, gamma.double() * inv, beta.double() - rm.double() * gamma.double() * inv)).float()
        recs = one.view(1, 256).repeat(G, 1)
    st = C.stream()
    yd, bnp = nhwc(y).to(DEV), recs.to(DEV)
    d = C.PoolDesc(n, h, w_, hp, wp, pad, out_nchw, G)
    o = Outs()
    pooled = o.new(n, 64, hp, wp) if out_nchw else o.new(n, hp, wp, 64)
    arg = o.new(n, hp, wp, 64, dtype=torch.uint8)
    p2 = o.new(*pooled.shape)
    C.bn_relu_pool_fwd(C.ptr(yd), C.ptr(bnp), C.ptr(pooled), C.ptr(arg), d, st)
    C.bn_relu_pool_fwd(C.ptr(yd), C.ptr(bnp), C.ptr(p2), None, d, st)   # eval form: no argmax
    o.check()
    assert finite(pooled) and torch.equal(p2, pooled) and int(arg.max()) <= 8
    # fp64 forward per group, and the pinned chain for the backward
    yr = y.double().requires_grad_(True)
    gs = [gamma.double().requires_grad_(True) for _ in range(G)]
    bs = [beta.double().requires_grad_(True) for _ in range(G)]
    z = torch.cat([F.batch_norm(yr[g * per:(g + 1) * per], rm.double().clone(), rv.double().clone(), gs[g], bs[g], bool(training), MOM, EPS)
                   for g in range(G)])
    p_ref = F.max_pool2d(F.relu(z), 3, 2, pad).detach()
    got_p = pooled if out_nchw else nchw(pooled)
    assert tuple(p_ref.shape) == (n, 64, hp, wp)
    e_fwd = rel_err(got_p, p_ref)
    assert e_fwd < 1e-5, e_fwd
    pin = pinned_pool(z, arg, got_p.cpu() > 0, w_, pad)
    assert rel_err(pin, p_ref) < 1e-5    # the device's argmax names the window's maximum
    if nxt:
        wc = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
        wcr = wc.double()
        ho, wo = out_size(hp, nxt, 1, 0), out_size(wp, nxt, 1, 0)
        dz = torch.randn(n, 64, ho, wo, generator=gen)
        F.conv2d(pin, wcr, None, nxt, 1).backward(dz.double())
        dp_ref = torch.autograd.grad(F.conv2d(p_ref.requires_grad_(True), wcr, None, nxt, 1), p_ref, dz.double())[0]
        dp = dp_ref.float()
    else:
        dp = torch.randn(n, 64, hp, wp, generator=gen)
        pin.backward(dp.double())
    dgamma = sum(g_.grad for g_ in gs)
    dbeta = sum(b_.grad for b_ in bs)
    sums_ref = torch.cat([torch.cat((bs[g].grad, gs[g].grad)) for g in range(G)])

    dpd = (dp if out_nchw else nhwc(dp)).to(DEV)
    nbw = C.bn_bwd_workspace(0)
    ws = torch.empty(nbw, dtype=torch.uint8, device=DEV)
    dy0, dg0, db0 = o.new(n, h, w_, 64), o.new(64), o.new(64)
    C.bn_relu_pool_bwd(C.ptr(yd), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), C.ptr(pooled), C.ptr(dy0), C.ptr(dg0), C.ptr(db0), training, C.ptr(ws),
                       nbw, d, st)
    dy1, dg1, db1 = o.new(n, h, w_, 64), o.new(64), o.new(64)
    C.bn_relu_pool_bwd(C.ptr(yd), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), None, C.ptr(dy1), C.ptr(dg1), C.ptr(db1), training, C.ptr(ws), nbw, d, st)
    sums, dg2, db2 = o.new(128 * G), o.new(64), o.new(64)
    C.bn_relu_pool_bwd_sums(C.ptr(yd), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), C.ptr(pooled), C.ptr(sums), C.ptr(dg2), C.ptr(db2), C.ptr(ws), nbw,
                            d, st)
    dy2 = o.new(n, h, w_, 64)
    C.bn_relu_pool_bwd_apply(C.ptr(yd), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), C.ptr(sums), C.ptr(dy2), training, d, st)
    o.check()
    assert finite(dy0, dg0, db0, dy1, sums, dy2)
    e = {"bwd": rel_err(nchw(dy0), yr.grad), "bwd(no pooled)": rel_err(nchw(dy1), yr.grad), "bwd_apply": rel_err(nchw(dy2), yr.grad),
         "dgamma": rel_err(dg0, dgamma), "dbeta": rel_err(db0, dbeta), "dgamma(sums)": rel_err(dg2, dgamma), "dbeta(sums)": rel_err(db2, dbeta),
         "sums": rel_err(sums, sums_ref)}
    print("pool %r: fwd %.1e %s" % (case, e_fwd, " ".join("%s %.1e" % kv for kv in sorted(e.items()))))
    assert all(v < TOL_BN for v in e.values()), e
    if not nxt:
        return
    # ---- the same two sums out of the next convolution's data-gradient launch
    dc = C.Conv64Desc(n, hp, wp, ho, wo, 3, nxt, 1, 0, G)
    packs = pack64(C, wc, dc)
    dzd = nhwc(dz).to(DEV)
    o3 = Outs()
    rows = C.conv64_bwd_data_tiles(dc)
    assert rows > 0
    dpl, part, dpp = o3.new(n, hp, wp, 64), o3.new(rows, 128), o3.new(n, hp, wp, 64)
    C.conv64_bwd_data_pool_sums(C.ptr(dzd), C.ptr(packs[1]), C.ptr(dpl), C.ptr(pooled), C.ptr(bnp), C.ptr(yd), C.ptr(arg), d, C.ptr(part),
                                dc, st)
    C.conv64_bwd_data(C.ptr(dzd), C.ptr(packs[1]), C.ptr(dpp), None, dc, st)
    o3.check()
    assert finite(dpl, part) and torch.equal(dpl, dpp)         # the epilogue changes nothing about the gradient itself
    assert rel_err(nchw(dpl), dp_ref) < TOL
    # record by record: dz = d(pooled) where the pooled value is positive, xhat from the value under the argmax
    posf = (got_p.cpu() > 0).double()
    xhat = (pin.detach() - beta.double().view(1, 64, 1, 1)) / gamma.double().view(1, 64, 1, 1)
    dzp = (dp_ref * posf, dp_ref * posf * xhat)
    tile, tpg = tiles_program(program(C, dc, 1), n, G)
    assert rows == G * tpg
    e2 = {"records": check_records(part, *records_by_tile(tile, rows, *dzp), tol=TOL_BN)}
    got = finalize_partials(C, part, G)
    e2.update({"sums": rel_err(got[0], sums_ref), "dgamma": rel_err(got[1], dgamma), "dbeta": rel_err(got[2], dbeta)})
    wino = C.conv64_wino_supported(dc)
    assert wino == (1 if nxt == 1 and hp % 2 == 0 and wp % 2 == 0 and min(hp, wp) >= 4 else 0)
    if wino:
        up = torch.empty(2, C.conv64_wino_packed_floats(), device=DEV)
        wcd = wc.to(DEV)
        C.conv64_wino_pack_weights(C.ptr(wcd), None, C.ptr(up[1]), st)
        rows_w = C.conv64_wino_bwd_data_rows(dc)
        dpw, part_w, dpw2 = o3.new(n, hp, wp, 64), o3.new(rows_w, 128), o3.new(n, hp, wp, 64)
        C.conv64_wino_bwd_data_pool_sums(C.ptr(dzd), C.ptr(up[1]), C.ptr(dpw), C.ptr(pooled), C.ptr(bnp), C.ptr(yd), C.ptr(arg), d,
                                         C.ptr(part_w), dc, st)
        C.conv64_wino_bwd_data(C.ptr(dzd), C.ptr(up[1]), C.ptr(dpw2), dc, st)
        o3.check()
        assert finite(dpw, part_w) and torch.equal(dpw2, dpw)
        assert rel_err(nchw(dpw), dp_ref) < TOL
        # (the Winograd d(pooled) differs from the direct one by its roundings: its sums are held to the fp64 sums of ITS gradient's
        # chain only through the tolerance below — the reference gradient dp_ref is the same)
        # (a group's last records come from the companion launch for channels without a usable scale: none here, zeros)
        assert rows_w % G == 0
        e2["wino records"] = check_records(part_w, *records_by_tile(tiles_wino(n, hp, wp, G, rows_w // G), rows_w, *dzp), tol=TOL_BN)
        gw = finalize_partials(C, part_w, G)
        e2.update({"wino sums": rel_err(gw[0], sums_ref), "wino dgamma": rel_err(gw[1], dgamma), "wino dbeta": rel_err(gw[2], dbeta)})
    print("pool link %r: %s" % (case, " ".join("%s %.1e" % kv for kv in sorted(e2.items()))))
    assert all(v < TOL_BN for v in e2.values()), e2


# ---------------------------------------------------------------------------------------------------------------------------------
# D. conv1: Conv2d(C, 64, 7, 2, 3) on [N,C,H,W] images
# ---------------------------------------------------------------------------------------------------------------------------------
# (himg, wimg, c, n, groups): 16 x 16 tiles over the feature map (forward, weight gradient) and over the image (data gradient)
CONV1_RECT = both([(160, 224, 3, 1, 1), (32, 34, 6, 4, 2), (17, 48, 3, 3, 1), (2, 38, 6, 4, 2), (33, 16, 3, 4, 1), (50, 70, 6, 1, 1),
                   (1, 31, 3, 3, 1)])


def lut_host():
    from preprocessing.utils import preprocessInput
    v = np.arange(256, dtype=np.float32).reshape(256, 1, 1).repeat(3, axis=2)   # [256, 1, 3]: value v in every channel
    return torch.from_numpy(np.ascontiguousarray(preprocessInput(v.copy()).reshape(256, 3).T))   # [3][256]


@pytest.mark.parametrize("case", CONV1_RECT, ids=lambda c: "%dx%d_c%d_n%dg%d" % c)
def test_conv1_rect(C, case):
    """srlz_conv1_fwd / srlz_conv1_fwd_u8 (bit-identical), statistics per group, srlz_conv1_bwd_data, srlz_conv1_bwd_weight, and the
    first block's fused weight gradient srlz_conv1_bwd_weight_fused / _u8 (bit-identical) behind BatchNorm -> ReLU -> MaxPool(3, 2, 1)
    on the device's own y, records, argmax and sums — against fp64 F.conv2d and autograd, for 3 and 6 image channels."""
    H, W, c, n, G = case
    hf, wf = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    hp, wp = pool_out(hf, 1), pool_out(wf, 1)
    per = n // G
    rs = np.random.RandomState(H * 3 + W)
    u8 = torch.from_numpy(rs.randint(0, 256, (n, c, H, W)).astype(np.uint8))
    lut_h = lut_host()
    x = torch.stack([lut_h[ch % 3][u8[:, ch].long()] for ch in range(c)], dim=1)     # the normalised frames, fp32
    gen = torch.Generator().manual_seed(H + 7 * W + c)
    w = torch.randn(64, c, 7, 7, generator=gen) * 0.1
    dy = torch.randn(n, 64, hf, wf, generator=gen)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, stride=2, padding=3)
    assert tuple(y_ref.shape) == (n, 64, hf, wf)
    y_ref.backward(dy.double())

    st = C.stream()
    d = C.SkinnyDesc(n, c, H, W, hf, wf, 0, G)
    u8d, wd, dyd = u8.to(DEV), w.to(DEV), nhwc(dy).to(DEV)
    lut = torch.full((3, 256), NAN, device=DEV)
    C.normalize_lut(C.ptr(lut), st)
    o = Outs()
    xd = o.new(n, c, H, W)
    C.normalize_u8_planar(C.ptr(u8d), C.ptr(lut), C.ptr(xd), n, c, H * W, st)
    o.check()
    assert torch.equal(lut.cpu(), lut_h) and torch.equal(xd.cpu(), x)
    tiles = C.skinny_tiles(d)
    assert tiles > 0 and tiles % G == 0
    y, stats, yu, su = o.new(n, hf, wf, 64), o.new(tiles, 128), o.new(n, hf, wf, 64), o.new(tiles, 128)
    C.conv1_fwd(C.ptr(xd), C.ptr(wd), C.ptr(y), C.ptr(stats), d, st)
    C.conv1_fwd_u8(C.ptr(u8d), C.ptr(lut), C.ptr(wd), C.ptr(yu), C.ptr(su), d, st)
    dx = o.new(n, c, H, W)
    C.conv1_bwd_data(C.ptr(dyd), C.ptr(wd), C.ptr(dx), d, st)
    nb = C.skinny_bwd_weight_workspace(d)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dw = o.new(64, c, 7, 7)
    C.conv1_bwd_weight(C.ptr(xd), C.ptr(dyd), C.ptr(dw), C.ptr(ws), nb, d, st)
    o.check()
    assert finite(y, stats, dx, dw)
    assert torch.equal(yu, y) and torch.equal(su, stats)                     # the uint8 route is the fp32 route
    e = {"fwd": rel_err(nchw(y), y_ref), "bwd_data": rel_err(dx, xr.grad), "bwd_weight": rel_err(dw, wr.grad)}
    assert tiles == n * ((hf + 15) // 16) * ((wf + 15) // 16)
    e["stats"] = check_records(stats, *records_by_tile(tiles_skinny(n, hf, wf), tiles, y_ref.detach(), y_ref.detach() ** 2))

    # ---- the fused first block: conv1 -> BatchNorm (train, G groups) -> ReLU -> MaxPool(3, 2, 1), weight gradient from d(pooled)
    gamma, beta = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.1
    rm, rv = torch.randn(64, generator=gen) * 0.1, torch.rand(64, generator=gen) + 0.5
    dp = torch.randn(n, 64, hp, wp, generator=gen)
    gd, bd, rmd, rvd = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
    nbw = C.bn_bwd_workspace(0)
    bws = torch.empty(nbw, dtype=torch.uint8, device=DEV)
    bnp, bstat = o.new(256 * G), o.new(128 * G)
    C.bn_finalize(C.ptr(stats), tiles, G, per * hf * wf, C.ptr(gd), C.ptr(bd), EPS, MOM, 1, C.ptr(rmd), C.ptr(rvd), None, C.ptr(bnp), C.ptr(bstat),
                  C.ptr(bws), nbw, st)
    pd = C.PoolDesc(n, hf, wf, hp, wp, 1, 0, G)
    pooled, arg = o.new(n, hp, wp, 64), o.new(n, hp, wp, 64, dtype=torch.uint8)
    C.bn_relu_pool_fwd(C.ptr(y), C.ptr(bnp), C.ptr(pooled), C.ptr(arg), pd, st)
    dpd = nhwc(dp).to(DEV)
    sums, dgm, dbt = o.new(128 * G), o.new(64), o.new(64)
    C.bn_relu_pool_bwd_sums(C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), C.ptr(pooled), C.ptr(sums), C.ptr(dgm), C.ptr(dbt), C.ptr(bws), nbw,
                            pd, st)
    dwf, dwu, dwf2 = o.new(64, c, 7, 7), o.new(64, c, 7, 7), o.new(64, c, 7, 7)
    C.conv1_bwd_weight_fused(C.ptr(xd), C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), C.ptr(sums), 1, C.ptr(dwf), C.ptr(ws), nb, d, pd, st)
    C.conv1_bwd_weight_fused_u8(C.ptr(u8d), C.ptr(lut), C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), C.ptr(sums), 1, C.ptr(dwu), C.ptr(ws), nb,
                                d, pd, st)
    C.conv1_bwd_weight_fused(C.ptr(xd), C.ptr(y), C.ptr(bnp), C.ptr(arg), C.ptr(dpd), C.ptr(sums), 1, C.ptr(dwf2), C.ptr(ws), nb, d, pd, st)
    o.check()
    assert finite(bnp, pooled, sums, dwf)
    assert torch.equal(dwu, dwf) and torch.equal(dwf2, dwf)
    wr2 = w.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y2 = F.conv2d(x.double(), wr2, None, stride=2, padding=3)
    z = torch.cat([F.batch_norm(y2[g * per:(g + 1) * per], rm.double().clone(), rv.double().clone(), gr, br, True, MOM, EPS) for g in range(G)])
    p_ref = F.max_pool2d(F.relu(z), 3, 2, 1)
    e["pooled"] = rel_err(nchw(pooled), p_ref)
    pin = pinned_pool(z, arg, nchw(pooled).cpu() > 0, wf, 1)
    assert rel_err(pin, p_ref) < 1e-5
    pin.backward(dp.double())
    e["bwd_weight_fused"] = rel_err(dwf, wr2.grad)
    e["dgamma"], e["dbeta"] = rel_err(dgm, gr.grad), rel_err(dbt, br.grad)
    print("conv1 %r: %s" % (case, " ".join("%s %.1e" % kv for kv in sorted(e.items()))))
    assert all(e[k] < TOL for k in ("fwd", "bwd_data", "bwd_weight", "stats", "pooled")), e
    assert all(e[k] < TOL_BN for k in ("bwd_weight_fused", "dgamma", "dbeta")), e   # test_encoder_input_block_fused_backward's bar


# ---------------------------------------------------------------------------------------------------------------------------------
# E. the last layer: ConvTranspose2d(64, C, 4, 2) -> [N,C,H,W]
# ---------------------------------------------------------------------------------------------------------------------------------
# (hf, wf, c, n, groups)
CONVT_RECT = both([(79, 111, 3, 1, 1), (16, 17, 6, 4, 2), (5, 33, 3, 3, 1), (1, 20, 6, 4, 2), (9, 24, 3, 4, 1), (2, 3, 3, 3, 1),
                   (19, 27, 6, 4, 2)])


@pytest.mark.parametrize("case", CONVT_RECT, ids=lambda c: "%dx%d_c%d_n%dg%d" % c)
def test_convT_out_rect(C, case):
    """srlz_convT_out_fwd (plain and x_bnp), srlz_convT_out_bwd_data without and with the BatchNorm-backward sums,
    srlz_convT_out_bwd_weight (x_bnp; (himg * wimg) & 3 == 0 holds for every map: himg = 2 hf + 2 is even on both axes),
    srlz_convT_out_bwd_fused against the two launches and fp64 autograd per BatchNorm group; 3 and 6 image channels."""
    hf, wf, c, n, G = case
    H, W = 2 * hf + 2, 2 * wf + 2
    assert (H * W) & 3 == 0
    per = n // G
    gen = torch.Generator().manual_seed(hf * 101 + wf * 3 + c)
    x = torch.randn(n, 64, hf, wf, generator=gen) * 1.3 + 0.2
    x[:, :, 0, :] += 1.0
    x[:, :, :, -1] -= 1.0
    recs, _, _ = records(x, G, gen)
    x = off_threshold(x, recs)
    w, b = torch.randn(64, c, 4, 4, generator=gen) * 0.1, torch.randn(c, generator=gen)
    dimg = torch.randn(n, c, H, W, generator=gen)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y_plain = F.conv_transpose2d(xr, wr, br, stride=2)
    assert tuple(y_plain.shape) == (n, c, H, W)
    y_plain.backward(dimg.double())
    act = activate(x, recs).requires_grad_(True)
    wr2 = w.double().requires_grad_(True)
    y_fused = F.conv_transpose2d(act, wr2, b.double(), stride=2)
    y_fused.backward(dimg.double())

    st = C.stream()
    d = C.SkinnyDesc(n, c, H, W, hf, wf, 1, G)
    xd, wd, bd, dd, rd = nhwc(x).to(DEV), w.to(DEV), b.to(DEV), dimg.to(DEV), recs.to(DEV)
    o = Outs()
    y0, y1 = o.new(n, c, H, W), o.new(n, c, H, W)
    C.convT_out_fwd(C.ptr(xd), C.ptr(wd), C.ptr(bd), C.ptr(y0), None, d, st)
    C.convT_out_fwd(C.ptr(xd), C.ptr(wd), C.ptr(bd), C.ptr(y1), C.ptr(rd), d, st)
    da0, da1 = o.new(n, hf, wf, 64), o.new(n, hf, wf, 64)
    tiles = C.skinny_tiles(d)
    assert tiles > 0 and tiles % G == 0
    p0 = o.new(tiles, 128)
    C.convT_out_bwd_data(C.ptr(dd), C.ptr(wd), C.ptr(da0), None, None, None, d, st)
    C.convT_out_bwd_data(C.ptr(dd), C.ptr(wd), C.ptr(da1), C.ptr(xd), C.ptr(rd), C.ptr(p0), d, st)
    nb = C.skinny_bwd_weight_workspace(d)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dw0, db0, dw1, db1 = o.new(64, c, 4, 4), o.new(c), o.new(64, c, 4, 4), o.new(c)
    C.convT_out_bwd_weight(C.ptr(xd), C.ptr(dd), C.ptr(dw0), C.ptr(db0), None, C.ptr(ws), nb, d, st)
    C.convT_out_bwd_weight(C.ptr(xd), C.ptr(dd), C.ptr(dw1), C.ptr(db1), C.ptr(rd), C.ptr(ws), nb, d, st)
    o.check()
    assert finite(y0, y1, da0, da1, p0, dw0, db0, dw1, db1)
    assert torch.equal(da1, da0)
    e = {"fwd": rel_err(y0, y_plain), "fwd+x_bnp": rel_err(y1, y_fused), "bwd_data": rel_err(nchw(da0), xr.grad),
         "bwd_weight": rel_err(dw0, wr.grad), "bwd_weight+x_bnp": rel_err(dw1, wr2.grad), "dbias": rel_err(db0, br.grad),
         "dbias+x_bnp": rel_err(db1, br.grad)}
    # the BatchNorm-backward sums of the block that produced x: sum dA [bn(x) > 0] and sum dA [bn(x) > 0] xhat per group, in fp64
    sums_ref = []
    for g in range(G):
        xs = x[g * per:(g + 1) * per].double()
        m, inv = recs[g, :64].double().view(1, 64, 1, 1), recs[g, 64:128].double().view(1, 64, 1, 1)
        dz = act.grad[g * per:(g + 1) * per] * (act[g * per:(g + 1) * per] > 0)
        sums_ref.append(torch.cat((dz.sum((0, 2, 3)), (dz * (xs - m) * inv).sum((0, 2, 3)))))
    sums_ref = torch.cat(sums_ref)
    dzv = bn_bwd_values(act.grad, x, recs)
    assert tiles == n * ((hf + 15) // 16) * ((wf + 15) // 16)
    e["bn records"] = check_records(p0, *records_by_tile(tiles_skinny(n, hf, wf), tiles, *dzv), tol=TOL)
    s0 = finalize_partials(C, p0, G)
    e["bn sums"] = rel_err(s0[0], sums_ref)
    assert C.convT_out_bwd_fused_supported(d) == 1
    o2 = Outs()
    ft = C.convT_out_bwd_fused_tiles(d)
    assert ft > 0 and ft % G == 0
    nf = C.convT_out_bwd_fused_workspace(d)
    wsf = torch.empty(nf, dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        da, p, dw, db = o2.new(n, hf, wf, 64), o2.new(ft, 128), o2.new(64, c, 4, 4), o2.new(c)
        C.convT_out_bwd_fused(C.ptr(dd), C.ptr(wd), C.ptr(da), C.ptr(xd), C.ptr(rd), C.ptr(p), C.ptr(dw), C.ptr(db), C.ptr(wsf), nf, None, 1.0, 1.0,
                              d, st)
        outs.append((da, p, dw, db))
    o2.check()
    da, p, dw, db = outs[0]
    assert finite(da, p, dw, db) and all(torch.equal(a_, b_) for a_, b_ in zip(outs[0], outs[1]))
    assert rel_err(da, da0) < 5e-6 and rel_err(dw, dw1) < TOL       # test_convT_out_bwd_fused_matches_the_two_launches
    assert ft == n * ((hf + 27) // 28) * ((wf + 15) // 16)
    e["fused bn records"] = check_records(p, *records_by_tile(tiles_convT_fused(n, hf, wf), ft, *dzv), tol=TOL)
    s1 = finalize_partials(C, p, G)
    for a_, b_ in zip(s0, s1):
        assert rel_err(b_, a_) < TOL
    e.update({"fused dA": rel_err(nchw(da), act.grad), "fused dw": rel_err(dw, wr2.grad), "fused bn sums": rel_err(s1[0], sums_ref)})
    tol_db = 3e-6 * (n * H * W) ** 0.5
    assert float((db.double().cpu() - br.grad).abs().max()) <= tol_db and float((db1.double().cpu() - br.grad).abs().max()) <= tol_db
    print("convT_out %r: %s" % (case, " ".join("%s %.1e" % kv for kv in sorted(e.items()))))
    assert all(v < TOL for v in e.values()), e


# (hf, wf, c, n, groups, mean): the batch is the two frames of a step, so n is even
LOSS_RECT = both([(79, 111, 3, 2, 2, 1), (16, 17, 6, 4, 2, 0), (5, 33, 3, 4, 2, 1), (1, 20, 3, 2, 1, 0), (9, 24, 6, 2, 2, 1), (19, 27, 3, 4, 2, 0)])


@pytest.mark.parametrize("case", LOSS_RECT, ids=lambda c: "%dx%d_c%d_n%dg%d_mean%d" % c)
def test_convT_out_fwd_loss_rect(C, case):
    """srlz_convT_out_fwd_loss and srlz_convT_out_fwd_loss_u8 (the pair loss of a step's two frames in the last layer's epilogue) on a
    rectangular image: the error is srlz_convT_out_fwd's output minus the target bit for bit, the uint8 route is the fp32 route bit for
    bit, the optional reconstruction is srlz_convT_out_fwd's, the loss through srlz_pair_loss_finalize against fp64 (both `mean`
    settings), and srlz_convT_out_bwd_fused fed with the error + gain equals the same kernel fed with the materialised gradient."""
    hf, wf, c, n, G, mean = case
    H, W = 2 * hf + 2, 2 * wf + 2
    gen = torch.Generator().manual_seed(hf * 13 + wf * 7 + c)
    x = torch.randn(n, 64, hf, wf, generator=gen) * 1.1 + 0.1
    recs, _, _ = records(x, G, gen)
    w, b = torch.randn(64, c, 4, 4, generator=gen) * 0.1, torch.randn(c, generator=gen)
    rs = np.random.RandomState(hf + wf)
    u8 = torch.from_numpy(rs.randint(0, 256, (n, c, H, W)).astype(np.uint8))
    lut_h = lut_host()
    tgt = torch.stack([lut_h[ch % 3][u8[:, ch].long()] for ch in range(c)], dim=1)
    ref = F.conv_transpose2d(activate(x, recs), w.double(), b.double(), stride=2)
    sq = ((ref - tgt.double()) ** 2).reshape(2, -1).sum(1)
    per = tgt.numel() // 2
    expect = (sq[0] / per + sq[1] / per) if mean else (sq[0] + sq[1])

    st = C.stream()
    d = C.SkinnyDesc(n, c, H, W, hf, wf, 1, G)
    xd, wd, bd, rd, td, u8d = nhwc(x).to(DEV), w.to(DEV), b.to(DEV), recs.to(DEV), tgt.to(DEV), u8.to(DEV)
    lut = torch.empty(3, 256, device=DEV)
    C.normalize_lut(C.ptr(lut), st)
    nwg = C.convT_out_fwd_loss_workgroups(d)
    assert nwg > 0
    o = Outs()
    dec0 = o.new(n, c, H, W)
    C.convT_out_fwd(C.ptr(xd), C.ptr(wd), C.ptr(bd), C.ptr(dec0), C.ptr(rd), d, st)
    err, dec1, part = o.new(n, c, H, W), o.new(n, c, H, W), o.new(2 * nwg, dtype=torch.float64)
    C.convT_out_fwd_loss(C.ptr(xd), C.ptr(wd), C.ptr(bd), C.ptr(td), C.ptr(err), C.ptr(dec1), C.ptr(rd), C.ptr(part), d, st)
    err_u, part_u = o.new(n, c, H, W), o.new(2 * nwg, dtype=torch.float64)
    C.convT_out_fwd_loss_u8(C.ptr(xd), C.ptr(wd), C.ptr(bd), C.ptr(u8d), C.ptr(lut), C.ptr(err_u), None, C.ptr(rd), C.ptr(part_u), d, st)
    sums, comb = o.new(2), o.new(1)
    C.pair_loss_finalize(C.ptr(part), nwg, per, mean, C.ptr(sums), C.ptr(comb), st)
    o.check()
    assert finite(dec0, err, part, sums, comb)
    assert torch.equal(dec1, dec0) and torch.equal(err, dec0 - td)
    assert torch.equal(err_u, err) and torch.equal(part_u, part)
    e = {"dec": rel_err(dec0, ref), "sums": rel_err(sums, sq), "loss": abs(float(comb) - float(expect)) / abs(float(expect))}
    print("convT_out loss %r: %s" % (case, e))
    assert e["dec"] < TOL and e["sums"] < 1e-5 and e["loss"] < 1e-5       # test_convT_out_forward_with_the_loss_in_its_epilogue
    # the backward on the stored error + gain == on the materialised gradient, bit for bit
    up = torch.tensor(1.7, device=DEV)
    div = float(per) if mean else 1.0
    grad = o.new(n, c, H, W)
    C.scale_by_scalar(C.ptr(err), C.ptr(up), div, 2.0, C.ptr(grad), err.numel(), st)
    ft, nf = C.convT_out_bwd_fused_tiles(d), C.convT_out_bwd_fused_workspace(d)
    wsf = torch.empty(nf, dtype=torch.uint8, device=DEV)
    outs = []
    for src, gain in ((grad, (None, 1.0, 1.0)), (err, (C.ptr(up), div, 2.0))):
        da, p, dw, db = o.new(n, hf, wf, 64), o.new(ft, 128), o.new(64, c, 4, 4), o.new(c)
        C.convT_out_bwd_fused(C.ptr(src), C.ptr(wd), C.ptr(da), C.ptr(xd), C.ptr(rd), C.ptr(p), C.ptr(dw), C.ptr(db), C.ptr(wsf), nf, gain[0],
                              gain[1], gain[2], d, st)
        outs.append((da, p, dw, db))
    o.check()
    for a_, b_ in zip(outs[0], outs[1]):
        assert finite(a_) and torch.equal(a_, b_)


# ---------------------------------------------------------------------------------------------------------------------------------
# F. layout and the uint8 input tail
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w_", both([(4, 6), (1, 9), (7, 33), (40, 56), (5, 2)]))
@pytest.mark.parametrize("n,c", [(1, 64), (3, 64), (4, 3)])
def test_layout_rect(C, n, c, h, w_):
    """srlz_nchw_to_nhwc / srlz_nhwc_to_nchw on h != w, bit for bit."""
    gen = torch.Generator().manual_seed(n + c + h * 5 + w_)
    x = torch.randn(n, c, h, w_, generator=gen)
    xd = x.to(DEV)
    o = Outs()
    y, back = o.new(n, h, w_, c), o.new(n, c, h, w_)
    C.nchw_to_nhwc(C.ptr(xd), C.ptr(y), n, c, h, w_, C.stream())
    C.nhwc_to_nchw(C.ptr(y), C.ptr(back), n, c, h, w_, C.stream())
    o.check()
    assert torch.equal(y.cpu(), nhwc(x)) and torch.equal(back.cpu(), x)


@pytest.mark.parametrize("h,w_", both([(160, 224), (33, 70), (5, 64), (1, 40), (31, 32)]))
@pytest.mark.parametrize("n,c", [(1, 3), (3, 6), (4, 3)])
def test_normalize_u8_rect(C, n, c, h, w_):
    """srlz_normalize_u8: [N,H,W,C] bytes -> normalised fp32 [N,C,W,H] (the loader's transpose(0, 3, 2, 1)), bit-identical to the host
    arithmetic as in test_normalize_u8_bit_exact; srlz_normalize_u8_planar on the transposed bytes gives the same tensor."""
    from preprocessing.utils import preprocessInput
    rs = np.random.RandomState(n + c + h + 3 * w_)
    frames = rs.randint(0, 256, (n, h, w_, c)).astype(np.uint8)
    ref = np.stack([np.dstack([preprocessInput(f[..., 3 * v:3 * v + 3].astype(np.float32)) for v in range(c // 3)]).transpose(2, 1, 0)
                    for f in frames])
    assert ref.shape == (n, c, w_, h)
    fd = torch.from_numpy(frames).to(DEV)
    planar = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 3, 2, 1))).to(DEV)
    lut = torch.empty(3, 256, device=DEV)
    C.normalize_lut(C.ptr(lut), C.stream())
    o = Outs()
    out, out_p = o.new(n, c, w_, h), o.new(n, c, w_, h)
    C.normalize_u8(C.ptr(fd), C.ptr(out), n, h, w_, c, C.stream())
    C.normalize_u8_planar(C.ptr(planar), C.ptr(lut), C.ptr(out_p), n, c, w_ * h, C.stream())
    o.check()
    assert np.array_equal(out.cpu().numpy(), ref) and torch.equal(out_p, out)


@pytest.mark.parametrize("wd,hd", both([(20, 36), (7, 64), (160, 224)]))
@pytest.mark.parametrize("c", [3, 6])
def test_occlude_frames_u8_rect(C, c, wd, hd):
    """srlz_occlude_frames_u8 on [C, W, H] planes with W != H: the rectangle (h1, h2, w1, w2) of a view set to 0, everything else through
    the table — with rectangles that touch ONE border only (top, bottom, left, right in turn), so that a kernel that compared h against
    the w bounds, or divided the flat index by W instead of H, shows."""
    rs = np.random.RandomState(wd + hd + c)
    n_store, n = 6, 4
    store = torch.from_numpy(rs.randint(0, 256, (n_store, c, wd, hd)).astype(np.uint8))
    index = torch.tensor([4, 0, 3, 2], dtype=torch.int64)
    shift = 1
    views = c // 3
    border = [(0, hd // 3, wd // 4, wd // 2), (hd - hd // 4, hd, wd // 3, wd - 2), (hd // 4, hd // 2, 0, wd // 3), (2, hd - 3, wd - wd // 4, wd)]
    rects = torch.tensor([[border[(i + v) % 4] for v in range(views)] for i in range(n)], dtype=torch.int32)
    lut_h = lut_host()
    ref = torch.empty(n, c, wd, hd)
    for i in range(n):
        f = store[int(index[i]) + shift]
        for ch in range(c):
            ref[i, ch] = lut_h[ch % 3][f[ch].long()]
            h1, h2, w1, w2 = [int(v) for v in rects[i, ch // 3]]
            ref[i, ch, w1:w2, h1:h2] = 0.0
    sd, idx_d, rd = store.to(DEV), index.to(DEV), rects.to(DEV)
    lut = torch.empty(3, 256, device=DEV)
    C.normalize_lut(C.ptr(lut), C.stream())
    o = Outs()
    out = o.new(n, c, wd, hd)
    C.occlude_frames_u8(C.ptr(sd), C.ptr(idx_d), shift, C.ptr(rd), C.ptr(lut), C.ptr(out), n, c, wd, hd, C.stream())
    o.check()
    assert torch.equal(out.cpu(), ref)
    assert int((ref == 0).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# G. the two conv stacks on a rectangular frame
# ---------------------------------------------------------------------------------------------------------------------------------
def _pins_from_taps(taps):
    """The decisions of one TAPS forward, in oracle.torch_twin's `pins` format (as tests/test_step_gpu.py::pins_from_taps)."""
    pins = {}
    for name, pad in (("encoder_conv.3", 1), ("encoder_conv.7", 0), ("encoder_conv.11", 0)):
        t = taps[name]
        y, _bnp, arg = t.grad_fn.saved_tensors[:3]
        w = y.shape[2]
        a = arg.long().cpu().permute(0, 3, 1, 2)
        hp, wp = a.shape[2], a.shape[3]
        py, px = torch.arange(hp).view(1, 1, hp, 1), torch.arange(wp).view(1, 1, 1, wp)
        pooled = t.detach().cpu()
        if pooled.shape != a.shape:
            pooled = pooled.permute(0, 3, 1, 2)
        pins[name] = ((py * 2 - pad + a // 3) * w + (px * 2 - pad + a % 3), pooled > 0)
    for name in ("decoder_conv.2", "decoder_conv.5", "decoder_conv.8", "decoder_conv.11"):
        pins[name] = taps[name].detach().cpu().permute(0, 3, 1, 2) > 0
    return pins


@pytest.mark.parametrize("route", ["default", "plain"])
@pytest.mark.parametrize("c", [3, 6])
@pytest.mark.parametrize("H,W", [(160, 224), (224, 160)])
def test_conv_stacks_on_a_rectangular_frame(H, W, c, route):
    """hotpath.encoder_forward + hotpath.decoder_forward on a batched pair of 160 x 224 / 224 x 160 frames (two BatchNorm groups,
    training mode): the encoder ends at 4 x 6 / 6 x 4, the decoder returns the input's size.  `default`: every fusion that accepts the
    shape, uint8 frames into the first block, the reconstruction loss in the decoder's epilogue (recon_loss_into); `plain`: hotpath.TAPS
    on — the un-fused chain, fp32 frames, the loss from the decoded tensor, the two frames as two calls of one BatchNorm group each
    (TAPS materialises activations with one record).  Outputs, the loss and the gradient of every convolution and
    BatchNorm parameter against oracle.torch_twin.encoder_conv / decoder_conv in fp64 at the run's own ReLU / max-pool decisions, 1e-4
    (the biases in front of a train-mode BatchNorm have an analytically zero gradient: summation noise, as in tests/route_check.py).
    The dense heads are sized for 6 x 6 x 64: this is the conv stacks alone, the code in between is the identity."""
    from collections import OrderedDict
    import preprocessing.preprocess as pre
    from models.models import _encoder_stack, _decoder_stack
    from oracle import torch_twin as T
    from srlz import hotpath, ops
    import golden_util as gu
    assert torch.cuda.is_available()
    B = 1  # frames per BatchNorm group
    old_c = pre.N_CHANNELS
    pre.N_CHANNELS = c
    try:
        torch.manual_seed(5)
        enc, dec = _encoder_stack(), _decoder_stack()
    finally:
        pre.N_CHANNELS = old_c
    gen = torch.Generator().manual_seed(H + c)
    with torch.no_grad():  # BatchNorm layers that are not the (1, 0) of a fresh module
        for m in list(enc) + list(dec):
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(64, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(64, generator=gen) * 0.2)
    sd = OrderedDict([(pre_ + k, v.detach().clone().double() if v.is_floating_point() else v.detach().clone())
                      for pre_, m in (("model.encoder_conv.", enc), ("model.decoder_conv.", dec)) for k, v in m.state_dict().items()])
    for k, v in sd.items():
        if k.endswith((".weight", ".bias")):
            v.requires_grad_(True)
    enc, dec = enc.to(DEV).train(), dec.to(DEV).train()
    rs = np.random.RandomState(H * 2 + W + c)
    u8 = torch.from_numpy(rs.randint(0, 256, (2 * B, c, H, W)).astype(np.uint8))
    # smooth-ish frames: neighbouring pixels correlated, as an image's are (plain noise makes every max-pool window a near-tie lottery)
    u8 = (u8.float().view(2 * B, c, H // 4, 4, W // 4, 4).mean((3, 5), keepdim=True).expand(2 * B, c, H // 4, 4, W // 4, 4)
          .reshape(2 * B, c, H, W) * 0.7 + u8.float() * 0.3).round().clamp(0, 255).to(torch.uint8)
    lut_h = lut_host()
    x = torch.stack([lut_h[ch % 3][u8[:, ch].long()] for ch in range(c)], dim=1)
    he, we = (4, 6) if H < W else (6, 4)

    params = [p for p in list(enc.parameters()) + list(dec.parameters())]
    try:
        if route == "plain":
            # hotpath.TAPS materialises activations with ONE BatchNorm record: the two frames go through as two calls of one group
            # each (what tests/test_step_gpu.py::hip_step does), the gradients of both accumulate in one backward
            xd = x.to(DEV)
            es, outs_, pins, loss = [], [], [], 0.0
            for i in range(2):
                hotpath.TAPS = taps = {}
                ei = hotpath.encoder_forward(enc, xd[i * B:(i + 1) * B].contiguous(), True)
                oi = hotpath.decoder_forward(dec, ei, True)
                pins.append(_pins_from_taps(taps))   # (the nodes' saved tensors: before backward frees them)
                hotpath.TAPS = None
                loss = loss + ((oi - xd[i * B:(i + 1) * B]) ** 2).sum() / oi.numel()
                es.append(ei)
                outs_.append(oi)
            e, out = torch.cat(es), torch.cat(outs_)
            assert tuple(e.shape) == (2 * B, 64, he, we) and tuple(out.shape) == (2 * B, c, H, W)
            loss.backward()
            launched = set()
        else:
            assert hotpath.TAPS is None
            hotpath.OBSERVE = {}
            frames = u8.to(DEV)
            with ops.batch_groups(2):
                with hotpath.recon_loss_into(frames, True) as req:
                    e = hotpath.encoder_forward(enc, frames, True)
                    out = hotpath.decoder_forward(dec, e, True)
                assert req.loss is not None, "the reconstruction loss was not taken in the decoder's epilogue"
                loss = req.loss
                observed = hotpath.OBSERVE
                assert tuple(e.shape) == (2 * B, 64, he, we) and tuple(out.shape) == (2 * B, c, H, W)
                ops.timers_enable(True)
                loss.backward()
                launched = set(k.split("/")[0] for k in ops.timers_report())
                ops.timers_enable(False)
        torch.cuda.synchronize()
        if route == "default":
            pins = gu.pins_from_observed(observed, B)
    finally:
        hotpath.OBSERVE = None
        hotpath.TAPS = None
        ops.timers_enable(False)
    if route == "default":  # it WAS the default route
        assert "conv64_dgrad_poolsum_kernel" in launched and "convT_out_os_bwd_kernel" in launched, sorted(launched)
    # ---- fp64 oracle, frame by frame (one BatchNorm call each), at those decisions
    enc_ref, dec_ref, total = [], [], 0.0
    for i in range(2):
        xi = x[i * B:(i + 1) * B].double()
        ei = T.encoder_conv(sd, xi, True, pins=pins[i])
        di = T.decoder_conv(sd, ei, True, pins=pins[i])
        total = total + ((di - xi) ** 2).sum() / di.numel()
        enc_ref.append(ei.detach())
        dec_ref.append(di.detach())
    total.backward()
    enc_ref, dec_ref = torch.cat(enc_ref), torch.cat(dec_ref)
    errs = {"encoder": rel_err(e, enc_ref), "loss": abs(float(loss.detach()) - float(total.detach())) / abs(float(total.detach()))}
    errs["decoder"] = rel_err(out + x.to(DEV), dec_ref) if route == "default" else rel_err(out, dec_ref)   # (default: out = dec - target)
    names = ["model.encoder_conv." + k for k, _ in enc.named_parameters()] + ["model.decoder_conv." + k for k, _ in dec.named_parameters()]
    noise = tuple("decoder_conv.%d.bias" % i for i in (0, 3, 6, 9))
    for name, p in zip(names, params):
        assert p.grad is not None and finite(p.grad), name
        gref = sd[name].grad
        if name.endswith(noise):
            scale = float(sd[name.replace(".bias", ".weight")].grad.abs().max())
            assert float((p.grad.double().cpu() - gref).abs().max()) < 1e-4 * scale, name
            continue
        errs[name] = rel_err(p.grad, gref)
    print("stacks %dx%d c=%d %s: %s" % (H, W, c, route, " ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(v < CEIL for v in errs.values()), {k: v for k, v in errs.items() if v >= CEIL}
