"""Host restatement of csrc/wino.hip (numpy and torch on the CPU): what tests/test_wino_host_cpu.py and tests/test_wino_entry_gpu.py
hold the Winograd F(2x2, 3x3) kernels of conv3x3(64, 64) to.

  * G, B^T, A^T of  Y = A^T [(G g G^T) .* (B^T d B)] A  as in the file's comments;
  * the pack layout upack[p][4 xi + nu][g][m][e], contraction channel k = 16 p + 4 g + e, for both directions (forward: m = co, k = ci;
    data gradient: m = ci, k = co, kernel flipped), in fp64;
  * an fp32 emulation of the algorithm (transforms in the kernel's order of additions, a sequential 64-long fp32 chain, the fold in the
    kernel's order) — used by the CPU test alone: it shows that the integer cases are exact in fp32 and that the element bounds below
    leave room;
  * the tile map (patches in the order (n, a, b) inside a BatchNorm group, 32 a tile), the launch grid and the XCD runs of tiles;
  * the weight gradient's plan, restated from wino_wgrad_program;
  * integer operands that assert their own exactness conditions, random operands, and the fp64 references of both.

Element bounds (derived, not measured).  u = 2^-24.  A computed sum of products in which every term passes through at most R roundings
differs from the exact value by at most ((1 + u)^R - 1) sum |terms| <= 1.01 R u sum |terms| for the R used here.

Forward and data gradient:  |got - ref64| <= 1.01 (64 + T_FWD) u mag + 64 * 2^-126,
    mag[n, co, i, j] = sum_{xi, nu} |A^T|[i, xi] |A|[nu, j] sum_ci |U64||V64| + |bias|,
U64 = G g G^T and V64 = B^T d B the fp64 transforms of the fp32 operands.  The chain is 64 products and 63 additions: 64 roundings per
term in any order, fused or not.  T_FWD = 11 counts the roundings outside the chain, read from the code:
    4  the pack: t = 0.5 (g0 +- g1 + g2) is two additions (the halving is exact), applied along kx and again along ky;
    2  the patch transform: one addition per value along the columns, one along the rows (wn_land);
    5  the fold and the bias: t0 = (m0 + m1) + m2 is two additions, y = ((bias + t[a]) +- t[b]) +- t[c] three more.
(The transform roundings are relative to the transform's partial sums, which the bound, like the kernel's own header, takes at the size
of the transformed value; the CPU test shows what the emulation leaves of the bound.)  The fused operand takes V64 from
relu(fma(raw, scale, shift)) evaluated in fp32 on the host (fma32 below, correctly rounded): the value the kernel forms, so no extra term.

Weight gradient:  |got - ref64| <= 1.01 (8 spw + T_WGRAD) u mag,  mag = |G^T| (sum over patches |Z64||V64|) |G|.  A workgroup's fp32
chain runs over its slice's 8 spw patches; the second stage (eight chunks, G^T . G) is fp64 and vanishes in the 1 %.  T_WGRAD = 5:
    2  Z = A dY A^T: one addition along the columns, one along the rows (wg_land);
    2  V = B^T d B as above;
    1  the cast of the fp64 result to fp32.

BatchNorm partial records against the kernel's own y: 1.01 * 130 u sum |y| and the same on y^2 (128 values a record: at most eight
levels of additions and one squaring, far inside 130).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
TP = 32                    # patches per tile
WN_CHUNK = 16 * 4 * 64 * 4  # floats of one 16-channel chunk of the packed weights
PACKED = 4 * WN_CHUNK
ZBLOCKS = 64               # cold records per group behind the tile records of the pooled-block sums
WG_SP = 8                  # patches per stage of the weight gradient
WG_CHUNKS = 8
T_FWD = 11
T_WGRAD = 5
LIMIT = 2 ** 24


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the pack -----------------------------------------------------------------------------------------------------------------------
def direction_weights(w, bwd):
    """g[m][k][ky][kx] of one direction from the reference layout w[co][ci][ky][kx]."""
    w = np.asarray(w)
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]) if bwd else w


def transform_weights(g):
    """U64[m, k, xi, nu] = G g G^T."""
    return np.einsum("xa,mkab,nb->mkxn", G, np.asarray(g, dtype=np.float64), G)


def _g_rows(a0, a1, a2):
    h = np.float32(0.5)
    return [a0, h * ((a0 + a1) + a2), h * ((a0 - a1) + a2), a2]


def transform_weights_f32(g):
    """The same in fp32, in conv64_wino_pack_kernel's order of additions."""
    g = np.asarray(g, dtype=np.float32)
    t = np.stack(_g_rows(g[..., 0], g[..., 1], g[..., 2]), -1)                  # [m, k, ky, nu]
    return np.stack(_g_rows(t[:, :, 0, :], t[:, :, 1, :], t[:, :, 2, :]), 2)      # [m, k, xi, nu]


def pack_layout(u):
    """U[m, k, xi, nu] -> the 4 * WN_CHUNK values of upack[p][4 xi + nu][g][m][e], k = 16 p + 4 g + e."""
    return np.ascontiguousarray(u.reshape(64, 4, 4, 4, 4, 4).transpose(1, 4, 5, 2, 0, 3)).reshape(-1)


def pack_ref(w, bwd):
    return pack_layout(transform_weights(direction_weights(w, bwd)))


# ---- patches and their transforms ---------------------------------------------------------------------------------------------------
def patches(x):
    """x [n, H, W, C] -> the 4 x 4 input patches [n, PA, PB, 4, 4, C]: rows 2a - 1 .. 2a + 2, columns 2b - 1 .. 2b + 2, zeros outside."""
    n, H, W, C = x.shape
    PA, PB = H // 2, W // 2
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.empty((n, PA, PB, 4, 4, C), dtype=x.dtype)
    for r in range(4):
        for c in range(4):
            out[:, :, :, r, c] = xp[:, r:r + 2 * PA:2, c:c + 2 * PB:2]
    return out


def quads(y):
    """y [n, H, W, C] -> the 2 x 2 output patches [n, PA, PB, 2, 2, C]."""
    n, H, W, C = y.shape
    return y.reshape(n, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5)


def unquads(q):
    n, PA, PB = q.shape[:3]
    return np.ascontiguousarray(q.transpose(0, 1, 3, 2, 4, 5)).reshape(n, 2 * PA, 2 * PB, q.shape[-1])


def transform_patches(d):
    """V64[..., xi, nu, C] = B^T d B."""
    return np.einsum("xr,...rcC,yc->...xyC", BT, np.asarray(d, dtype=np.float64), BT, optimize=True)


def _bt(a0, a1, a2, a3):
    return [a0 - a2, a1 + a2, a2 - a1, a1 - a3]


def transform_patches_f32(d):
    """The same in fp32, in wn_land's order: along the columns, then along the rows."""
    d = np.asarray(d, dtype=np.float32)
    e = np.stack(_bt(*[d[..., :, c, :] for c in range(4)]), -2)   # [..., r, nu, C]
    return np.stack(_bt(*[e[..., r, :, :] for r in range(4)]), -3)  # [..., xi, nu, C]


def transform_grads(q):
    """Z64[..., xi, nu, C] = A dY A^T of the 2 x 2 output gradients."""
    return np.einsum("ix,...ijC,jy->...xyC", AT, np.asarray(q, dtype=np.float64), AT, optimize=True)


def _a(a0, a1):
    return [a0, a0 + a1, a0 - a1, -a1]


def transform_grads_f32(q):
    """The same in fp32, in wg_land's order: along the columns, then along the rows."""
    q = np.asarray(q, dtype=np.float32)
    t = np.stack(_a(q[..., :, 0, :], q[..., :, 1, :]), -2)      # [..., i, nu, C]
    return np.stack(_a(t[..., 0, :, :], t[..., 1, :, :]), -3)   # [..., xi, nu, C]


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded: the product is exact in fp64, the sum is rounded to odd (TwoSum), then to fp32."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def activate(raw, recs, groups):
    """relu(fma(raw, scale, shift)) per BatchNorm group in fp32: raw [n, H, W, 64], recs [G, 256] (scale at 128, shift at 192)."""
    per = raw.shape[0] // groups
    out = np.empty_like(raw, dtype=np.float32)
    for g in range(groups):
        z = fma32(raw[g * per:(g + 1) * per], recs[g, 128:192], recs[g, 192:256])
        out[g * per:(g + 1) * per] = np.maximum(z, np.float32(0))
    return out


# ---- fp32 emulation (CPU test only) -------------------------------------------------------------------------------------------------
def emulate_conv(x, g, bias=None, spoil=None):
    """conv64_wino_kernel in fp32 numpy: x [n, H, W, 64] (the layer's input), g[m][k][3][3] the direction's weights -> y [n, H, W, 64].
    spoil: a function applied to the transformed patches (the CPU test's deliberately wrong kernels)."""
    u = transform_weights_f32(g).reshape(64, 64, 16)                     # [m, k, comp]
    v = transform_patches_f32(patches(np.asarray(x, dtype=np.float32)))  # [n, PA, PB, xi, nu, k]
    if spoil is not None:
        v = spoil(v)
    n, PA, PB = v.shape[:3]
    v = v.reshape(-1, 16, 64)
    acc = None
    for k in range(64):
        prod = v[:, :, k, None] * u[:, k, :].T[None]
        acc = prod if acc is None else acc + prod
    assert acc.dtype == np.float32
    m = acc.reshape(-1, 4, 4, 64)
    t0 = (m[:, 0] + m[:, 1]) + m[:, 2]   # [P, nu, co]
    t1 = (m[:, 1] - m[:, 2]) - m[:, 3]
    bz = np.zeros(64, np.float32) if bias is None else np.asarray(bias, dtype=np.float32)
    q = np.empty((v.shape[0], 2, 2, 64), np.float32)
    for i, t in enumerate((t0, t1)):
        q[:, i, 0] = ((bz + t[:, 0]) + t[:, 1]) + t[:, 2]
        q[:, i, 1] = ((bz + t[:, 1]) - t[:, 2]) - t[:, 3]
    return unquads(q.reshape(n, PA, PB, 2, 2, 64))


def emulate_wgrad(x, dy, spw):
    """conv64_wino_wgrad_kernel and its second stage: fp32 chains over slices of 8 spw patches, the rest in fp64 -> dw[co][ci][3][3]."""
    v = transform_patches_f32(patches(np.asarray(x, dtype=np.float32))).reshape(-1, 16, 64)
    z = transform_grads_f32(quads(np.asarray(dy, dtype=np.float32))).reshape(-1, 16, 64)
    total = np.zeros((16, 64, 64), np.float64)
    step = spw * WG_SP
    for s0 in range(0, v.shape[0], step):
        acc = np.zeros((16, 64, 64), np.float32)
        for p in range(s0, min(s0 + step, v.shape[0])):
            acc = acc + z[p][:, :, None] * v[p][:, None, :]
        assert acc.dtype == np.float32
        total += acc
    return np.einsum("xa,xyCD,yb->CDab", G, total.reshape(4, 4, 64, 64), G).astype(np.float32)


# ---- tiles, grids and plans ---------------------------------------------------------------------------------------------------------
def fwd_plan(n, h, w, groups):
    per = n // groups
    ppi = (h // 2) * (w // 2)
    ppg = per * ppi
    tpg = cdiv(ppg, TP)
    return {"per": per, "ppi": ppi, "ppg": ppg, "tpg": tpg, "tiles": groups * tpg, "rows": groups * (tpg + ZBLOCKS)}


def tile_of_pixel(n, h, w, groups, rows_per_group):
    """[n, h, w]: the record a pixel is summed into."""
    per = n // groups
    img, oy, ox = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    patch = (img % per) * ((h // 2) * (w // 2)) + (oy // 2) * (w // 2) + ox // 2
    return (img // per) * rows_per_group + patch // TP


def tile_sums(v, groups):
    """v [n, H, W, C] (fp64) -> [G, tpg, C]: the sums over each tile's patches."""
    n, H, W, C = v.shape
    P = fwd_plan(n, H, W, groups)
    q = quads(v).reshape(groups, P["ppg"], 4, C).sum(2)
    pad = np.zeros((groups, P["tpg"] * TP, C), dtype=v.dtype)
    pad[:, :P["ppg"]] = q
    return pad.reshape(groups, P["tpg"], TP, C).sum(2)


def launch_grid(ntiles, cus):
    return (min(2 * cus, ntiles) + 7) & ~7


def tiles_of_workgroups(ntiles, grid):
    """The tiles each workgroup of conv64_wino_kernel takes, in its order (block b: XCD b & 7, the XCD's run dealt out round robin)."""
    wpx, tq, tr = grid >> 3, ntiles >> 3, ntiles & 7
    out = []
    for b in range(grid):
        xcd, wi = b & 7, b >> 3
        tbase = xcd * (tq + 1) if xcd < tr else tr * (tq + 1) + (xcd - tr) * tq
        tcnt = tq + (1 if xcd < tr else 0)
        out.append([tbase + k for k in range(wi, tcnt, wpx)])
    return out


def big_n(cus):
    """56 x 56 in two groups: the smallest even n with G * tpg > 2 CUs + 8 — some workgroups take two tiles, some across the groups."""
    n = 2
    while fwd_plan(n, 56, 56, 2)["tiles"] <= 2 * cus + 8:
        n += 2
    return n


def wgrad_plan(n, h, w, cus):
    total = n * (h // 2) * (w // 2)
    stages = cdiv(total, WG_SP)
    g = (2 * cus + 15) & ~15
    while g > 16 and (g >> 1) * 4 > stages:
        g -= 16
    slices = g >> 1
    spw = cdiv(stages, slices)
    return {"total": total, "stages": stages, "grid": g, "slices": slices, "spw": spw, "empty": slices - cdiv(stages, spw),
            "workspace": g * 8 * 4096 * 4 + WG_CHUNKS * 16 * 4096 * 8}


def slice_of_workgroup(b, grid):
    """conv64_wino_wgrad_kernel: (slice, component half) of workgroup b."""
    xcd, wi, wpx = b & 7, b >> 3, grid >> 3
    return xcd * (wpx >> 1) + (wi >> 1), wi & 1


def wgrad_partials(x, dy, plan):
    """[grid, 8, 64, 64] fp64: what each workgroup of conv64_wino_wgrad_kernel leaves in the workspace — its slice's sum over patches of
    Z[co] V[ci] for the components (xi, nu = 2 half + j) at index 2 xi + j (exact on the integer cases)."""
    v = transform_patches(patches(np.asarray(x, dtype=np.float64))).reshape(-1, 4, 4, 64)
    z = transform_grads(quads(np.asarray(dy, dtype=np.float64))).reshape(-1, 4, 4, 64)
    step = plan["spw"] * WG_SP
    out = np.zeros((plan["grid"], 8, 64, 64))
    for b in range(plan["grid"]):
        s, half = slice_of_workgroup(b, plan["grid"])
        zs, vs = (a[s * step:(s + 1) * step, :, 2 * half:2 * half + 2].reshape(-1, 8, 64) for a in (z, v))
        if len(zs):
            out[b] = np.matmul(zs.transpose(1, 2, 0), vs.transpose(1, 0, 2))
    return out


# (h, w, n, groups); n = 0: big_n(CUs)
FWD_SHAPES = [(4, 4, 1, 1), (4, 4, 9, 1), (6, 10, 3, 1), (6, 10, 3, 3), (8, 8, 2, 1), (8, 8, 4, 2), (4, 68, 1, 1), (68, 4, 1, 1),
              (16, 20, 3, 3), (56, 56, 0, 2)]
FWD_TILES = [1, 2, 2, 3, 1, 2, 3, 3, 9, None]
# (h, w, n); the weight gradient has no groups
WGRAD_SHAPES = [(4, 4, 1), (6, 6, 1), (10, 10, 5), (14, 14, 7), (40, 40, 2), (56, 56, 0)]
# (grid, spw, empty slices) per CU count
WGRAD_PLANS = {256: [(16, 1, 7), (16, 1, 6), (16, 2, 0), (16, 6, 0), (48, 5, 4), (512, 9, 16)],
               8: [(16, 1, 7), (16, 1, 6), (16, 2, 0), (16, 6, 0), (16, 13, 0), (16, 25, 0)]}
BIG_N = {256: 22, 8: 2}


def resolve(shape, cus):
    return tuple(big_n(cus) if (i == 2 and v == 0) else v for i, v in enumerate(shape))


def wgrad_groups(shape):
    """The weight gradient has no groups; its 56 x 56 case takes the operands (and references) of the forward's, which has two."""
    return 2 if shape[2] == 0 else 1


def shape_id(s):
    return "%dx%d-n%s%s" % (s[0], s[1], s[2] or "big", "-g%d" % s[3] if len(s) > 3 else "")


# ---- operands and references (made once, never modified) ----------------------------------------------------------------------------
def nchw64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).transpose(0, 3, 1, 2)))


def nhwc_np(t):
    return np.ascontiguousarray(t.detach().numpy().transpose(0, 2, 3, 1))


def conv64(x, w, bias=None):
    """fp64 F.conv2d of NHWC x -> NHWC."""
    b = None if bias is None else torch.from_numpy(np.asarray(bias, dtype=np.float64))
    return nhwc_np(F.conv2d(nchw64(x), torch.from_numpy(np.asarray(w, dtype=np.float64)), b, stride=1, padding=1))


def grads64(x, w, dy):
    """fp64 autograd of conv2d: (dx NHWC, dw [co][ci][3][3])."""
    xr = nchw64(x).requires_grad_(True)
    wr = torch.from_numpy(np.asarray(w, dtype=np.float64)).requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(xr, wr, None, stride=1, padding=1), (xr, wr), nchw64(dy))
    return nhwc_np(gx), gw.numpy()


def chain_mag(x, g):
    """sum_ci |U64||V64| per patch, component and output channel: [n, PA, PB, 4, 4, 64]."""
    u = np.ascontiguousarray(np.abs(transform_weights(g)).reshape(64, 64, 16).transpose(2, 1, 0))        # [comp, k, m]
    v = np.abs(transform_patches(patches(np.asarray(x, dtype=np.float64))))
    shp = v.shape[:3]
    v = np.ascontiguousarray(v.reshape(-1, 16, 64).transpose(1, 0, 2))                                 # [comp, P, k]
    return np.ascontiguousarray(np.matmul(v, u).transpose(1, 0, 2)).reshape(shp + (4, 4, 64))


def fold_mag(s, bias=None):
    """mag[n, H, W, co] of the element bound from chain_mag's sums."""
    a = np.abs(AT)
    m = unquads(np.einsum("ix,jy,napxyc->napijc", a, a, s, optimize=True))
    return m if bias is None else m + np.abs(np.asarray(bias, dtype=np.float64))


def bound_fwd(mag):
    return 1.01 * (64 + T_FWD) * U * mag + 64 * 2.0 ** -126


def wgrad_mag(x, dy):
    v = np.abs(transform_patches(patches(np.asarray(x, dtype=np.float64)))).reshape(-1, 16, 64)
    z = np.abs(transform_grads(quads(np.asarray(dy, dtype=np.float64)))).reshape(-1, 16, 64)
    m = np.stack([z[:, c].T @ v[:, c] for c in range(16)]).reshape(4, 4, 64, 64)
    a = np.abs(G)
    return np.einsum("xa,xyCD,yb->CDab", a, m, a)


def bound_wgrad(mag, spw):
    return 1.01 * (WG_SP * spw + T_WGRAD) * U * mag


def bound_records(sum_abs):
    return 1.01 * 130 * U * sum_abs


def worst_ratio(got, ref, bnd):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(np.where(err == 0, 0.0, err / np.maximum(bnd, 1e-300)).max())


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _seed(kind, h, w, n, groups):
    return ((h * 131 + w) * 131 + n) * 7 + groups + (1 << 20 if kind == "int" else 0)


@functools.lru_cache(maxsize=None)
def weights(kind):
    """(w [co][ci][3][3], bias [64]) of a kind, shared by every shape: integers of [-2, 2], or normal x 0.05 and normal."""
    rs = np.random.RandomState(20 if kind == "int" else 21)
    if kind == "int":
        w, b = rs.randint(-2, 3, size=(64, 64, 3, 3)), rs.randint(-2, 3, size=64)
    else:
        w, b = rs.standard_normal((64, 64, 3, 3)) * 0.05, rs.standard_normal(64)
    w, b = w.astype(np.float32), b.astype(np.float32)
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


@functools.lru_cache(maxsize=None)
def operands(kind, h, w, n, groups):
    """x, dy [n, h, w, 64] and the fused operand's records [G, 256] (mean and invstd unused: NaN) with act = relu(fma(x, scale, shift)).
    int: integers of [-2, 2], scale in {-2 .. 2}, shift in [-3, 3].  rnd: normal, the border rows and columns of x offset by +-1.5; one
    scale in five negative."""
    rs = np.random.RandomState(_seed(kind, h, w, n, groups))
    recs = np.full((groups, 256), np.nan, dtype=np.float32)
    if kind == "int":
        x, dy = rs.randint(-2, 3, size=(n, h, w, 64)), rs.randint(-2, 3, size=(n, h, w, 64))
        recs[:, 128:192], recs[:, 192:] = rs.randint(-2, 3, size=(groups, 64)), rs.randint(-3, 4, size=(groups, 64))
    else:
        x, dy = rs.standard_normal((n, h, w, 64)), rs.standard_normal((n, h, w, 64))
        x[:, 0, :] += 1.5
        x[:, -1, :] -= 1.5
        x[:, :, 0] -= 1.5
        x[:, :, -1] += 1.5
        sign = np.where(rs.randint(0, 5, size=(groups, 64)) == 0, -1.0, 1.0)
        recs[:, 128:192], recs[:, 192:] = sign * (0.5 + np.abs(rs.standard_normal((groups, 64)))), rs.standard_normal((groups, 64)) * 0.5
    d = {"x": x.astype(np.float32), "dy": dy.astype(np.float32), "recs": recs}
    d["act"] = activate(d["x"], recs, groups)
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def conv_refs(kind, h, w, n, groups):
    """fp64 references of one shape: y (no bias), y_fused (of act), dx and dw (of x and dy); for the bounds the magnitudes m_x, m_act
    (forward weights) and m_dy (data-gradient weights) of fold_mag without a bias, and smax: the largest sum_ci |U64||V64| of each."""
    d, (wt, _) = operands(kind, h, w, n, groups), weights(kind)
    r = {"y": conv64(d["x"], wt), "y_fused": conv64(d["act"], wt)}
    r["dx"], r["dw"] = grads64(d["x"], wt, d["dy"])
    r["smax"] = {}
    for k, src, g in (("x", "x", wt), ("act", "act", wt), ("dy", "dy", direction_weights(wt, True))):
        s = chain_mag(d[src], g)
        r["smax"][k], r["m_" + k] = float(s.max()), fold_mag(s)
    if kind == "int":
        assert_conv_exact(d, r, groups)
    return _freeze(r)


def assert_conv_exact(d, r, groups):
    """The conditions under which every fp32 order of the kernel's operations returns the integer convolution: the transform values are
    multiples of 1/4 (U) and integers (V), so four times every chain's sum of magnitudes below 2^24 makes every partial sum exact; then
    the outputs (with any bias of [-2, 2]) and every tile's sum |y| and sum y^2 per channel."""
    for k, s in r["smax"].items():
        assert 4 * s < LIMIT, (k, s)
    for k in ("y", "y_fused", "dx"):
        v = r[k]
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() + 2 < LIMIT
        if k != "dx":
            v = np.abs(v) + 2
            assert tile_sums(v, groups).max() < LIMIT and tile_sums(v * v, groups).max() < LIMIT, k
    assert np.array_equal(r["dw"], np.rint(r["dw"])) and np.abs(r["dw"]).max() < LIMIT


def assert_wgrad_exact(d, spw):
    """patches of a slice x max |Z| x max |V| < 2^24: a workgroup's fp32 chain of integer products is exact in any order (the second stage
    is fp64 on quarters of integers)."""
    vmax = np.abs(transform_patches(patches(d["x"]))).max()
    zmax = np.abs(transform_grads(quads(d["dy"]))).max()
    assert WG_SP * spw * zmax * vmax < LIMIT, (spw, zmax, vmax)


# ---- the pooled block in front of the data gradient ---------------------------------------------------------------------------------
def pool_in(hp, pad):
    """The smallest map MaxPool(3, 2, pad) turns into hp rows."""
    return 2 * hp + 1 - 2 * pad


@functools.lru_cache(maxsize=None)
def pool_operands(hp, wp, n, groups, pad):
    """Integer inputs of srlz_conv64_wino_bwd_data_pool_sums: pool_y [n, h, w, 64] raw integers of [-3, 3]; records with integer mean and
    shift, invstd and scale in {+-0.5, +-1, +-2}, channels 5 and 40 of every group at scale 0 (shift +2: the ReLU open everywhere,
    and -1: closed).  dy is operands("int", hp, wp, n, groups)["dy"]."""
    rs = np.random.RandomState(_seed("int", hp, wp, n, groups) + 99 + pad)
    h, w = pool_in(hp, pad), pool_in(wp, pad)
    vals = np.array([-2, -1, -.5, .5, 1, 2], dtype=np.float32)
    recs = np.empty((groups, 256), dtype=np.float32)
    recs[:, :64] = rs.randint(-2, 3, size=(groups, 64))
    recs[:, 64:128] = vals[rs.randint(0, 6, size=(groups, 64))]
    recs[:, 128:192] = vals[rs.randint(0, 6, size=(groups, 64))]
    recs[:, 192:] = rs.randint(-3, 4, size=(groups, 64))
    recs[:, 128 + 5], recs[:, 192 + 5] = 0.0, 2.0
    recs[:, 128 + 40], recs[:, 192 + 40] = 0.0, -1.0
    return _freeze({"pool_y": rs.randint(-3, 4, size=(n, h, w, 64)).astype(np.float32), "recs": recs, "h": h, "w": w})


def pool_forward(pool_y, recs, groups, pad):
    """fp64 max_pool2d(relu(y * scale + shift), 3, 2, pad) per group -> [n, hp, wp, 64] (exact on these operands)."""
    per = pool_y.shape[0] // groups
    z = np.concatenate([pool_y[g * per:(g + 1) * per].astype(np.float64) * recs[g, 128:192] + recs[g, 192:] for g in range(groups)])
    return nhwc_np(F.max_pool2d(F.relu(nchw64(z)), 3, 2, pad))


def pool_sum_values(da, argmax, pool_y, recs, groups, pad):
    """(dz, dz * xhat) [n, hp, wp, 64] in fp64: dz = dA where relu(bn(.)) passes the value under the recorded argmax, xhat = (that value
    - mean) * invstd — what the pooled block's BatchNorm backward sums, for every channel alike."""
    n, hp, wp, _ = da.shape
    per = n // groups
    a = argmax.astype(np.int64)
    iy = (np.arange(hp) * 2 - pad)[None, :, None, None] + a // 3
    ix = (np.arange(wp) * 2 - pad)[None, None, :, None] + a % 3
    assert iy.min() >= 0 and iy.max() < pool_y.shape[1] and ix.min() >= 0 and ix.max() < pool_y.shape[2], "an argmax points outside the map"
    vy = pool_y[np.arange(n)[:, None, None, None], iy, ix, np.arange(64)[None, None, None, :]].astype(np.float64)
    r = np.repeat(recs.astype(np.float64), per, axis=0)[:, None, None, :]
    dz = np.where(vy * r[..., 128:192] + r[..., 192:] > 0, da.astype(np.float64), 0.0)
    return dz, dz * (vy - r[..., :64]) * r[..., 64:128]


def assert_pool_exact(da, z, recs, groups):
    """dA is an integer, the pooled value z a multiple of 1/2, pA = invstd / scale and pB = -(shift / scale + mean) invstd multiples of
    1/4: every term of a tile's  pA sum dA z + pB sum dA  is a multiple of 1/8, and 16 times the tile's sum of magnitudes stays below
    2^24 — any fp32 order of the epilogue is exact."""
    zero = zero_scale(recs)
    r = recs.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pA = np.where(zero, 0.0, r[:, 64:128] / r[:, 128:192])
        pB = np.where(zero, 0.0, -(r[:, 192:] / r[:, 128:192] + r[:, :64]) * r[:, 64:128])
    assert np.array_equal(pA * 4, np.rint(pA * 4)) and np.array_equal(pB * 4, np.rint(pB * 4)) and np.array_equal(z * 2, np.rint(z * 2))
    per = da.shape[0] // groups
    wgt = np.abs(z) * np.repeat(np.abs(pA), per, axis=0)[:, None, None, :] + np.repeat(np.abs(pB), per, axis=0)[:, None, None, :]
    assert 16 * tile_sums(np.abs(da) * (wgt + 1), groups).max() < LIMIT


def zero_scale(recs):
    """[G, 64]: the channels the tile records leave to the cold records (the kernel's own threshold)."""
    sc, sh = recs[:, 128:192], recs[:, 192:]
    return (np.abs(sc) <= np.float32(1e-3) * np.abs(sh)) | (sc == 0)
