"""The reward-prior and episode-prior kernels (csrc/priors.hip) through the C ABI (srlz.ops.RewardPriorFn / EpisodePriorFn) against an
fp64 torch restatement of the losses written from their definitions (correlation of the reward row, BCE of a three-layer
discriminator over state pairs, reversed state gradient), and run-to-run bit identity."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _ops():
    from srlz import ops
    return ops


def reward_prior64(states, r, eps=1e-8):
    """1 - mean_j |clamp(corr[S, j])| of X = cat([states, r], 1)^T, every step in fp64 and differentiable."""
    x = torch.cat([states, r.view(-1, 1)], 1).t()
    xc = x - x.mean(1, keepdim=True)
    cov = xc @ xc.t() / (x.shape[1] - 1)
    inv = torch.rsqrt(torch.diag(cov) + eps)
    corr = (cov * inv.view(1, -1) * inv.view(-1, 1)).clamp(-1.0, 1.0)
    return 1 - corr[-1].abs().mean()


def episode_prior64(states, others, same, params):
    w1, b1, w2, b2, w3, b3 = params
    x = torch.cat([states, states[others]], 1)
    h = torch.relu(F.linear(x, w1, b1))
    h = torch.relu(F.linear(h, w2, b2))
    z = F.linear(h, w3, b3).view(-1)
    return z


def bce_sum(p, y):
    return -(y * torch.clamp(torch.log(p), min=-100) + (1 - y) * torch.clamp(torch.log(1 - p), min=-100)).sum()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("B,S", [(2, 3), (8, 12), (256, 200), (257, 7), (1000, 2)])
@pytest.mark.parametrize("kind", ["random", "constant_reward", "zero_var_column"])
def test_reward_prior_matches_fp64(B, S, kind):
    ops = _ops()
    rng = np.random.RandomState(B * 31 + S)
    s = rng.randn(B, S).astype(np.float32)
    r = rng.randint(-1, 2, B).astype(np.float32)
    if kind == "constant_reward":
        r[:] = 1.0
    if kind == "random":  # correlate a column with the reward
        s[:, 0] += 2.0 * r
    if kind == "zero_var_column":
        s[:, S // 2] = 0.75
        if B == 2:
            r = np.array([0.0, 1.0], dtype=np.float32)
    st = torch.from_numpy(s).cuda().requires_grad_(True)
    rt = torch.from_numpy(r).cuda()
    g = 3.0
    loss = ops.RewardPriorFn.apply(st, rt)
    (g * loss).backward()
    s64 = torch.from_numpy(s).double().requires_grad_(True)
    ref = reward_prior64(s64, torch.from_numpy(r).double())
    (g * ref).backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(abs(float(ref)), 1e-6), (float(loss), float(ref))
    gs = st.grad.double().cpu()
    scale = max(s64.grad.abs().max().item(), 1e-6)
    if kind == "zero_var_column":  # fp64 leaves round-off in that column's centred values: its correlation is 0 for the kernel only
        keep = [k for k in range(S) if k != S // 2]
        assert gs[:, S // 2].abs().max().item() == 0.0
        gs, ref_g = gs[:, keep], s64.grad[:, keep]
    else:
        ref_g = s64.grad
    if kind == "constant_reward":
        assert gs.abs().max().item() == 0.0
        return
    assert (gs - ref_g).abs().max().item() <= 1e-4 * scale


def _disc_params(S, scale, seed):
    gen = torch.Generator().manual_seed(seed)
    shapes = ((64, 2 * S), (64,), (64, 64), (64,), (1, 64), (1,))
    ps = [torch.randn(shape, generator=gen) * (scale / np.sqrt(shape[-1] if len(shape) == 2 else 64)) for shape in shapes]
    ps[1] += 0.1
    ps[3] += 0.1
    return ps


def _draw(B, balanced, rng):
    eps = np.sort(rng.randint(0, max(2, B // 5), B))
    if balanced:  # repeats and missing rows
        others = rng.randint(0, B, B)
        others[: B // 2] = others[0]
    else:
        others = rng.permutation(B)
    return others, (eps == eps[others]).astype(np.float32)


def _episode_run(ops, s, others, same, ps):
    st = torch.from_numpy(s).cuda().requires_grad_(True)
    params = [p.clone().cuda().requires_grad_(True) for p in ps]
    o = torch.from_numpy(others.astype(np.int32)).cuda()
    y = torch.from_numpy(same).cuda()
    loss = ops.EpisodePriorFn.apply(st, o, y, *params)
    # the kernel's own sigmoid outputs, from the workspace the forward keeps for the backward (h1 [B, 64], h2 [B, 64], then p [B]):
    # a logit at a rounding edge of the fp32 sigmoid may land on either side of it, and near saturation the two sides differ in
    # kind (p = 1 - 2^-24 still passes a gradient, p = 1.0 clamps the log at -100 and passes none) — the restatement is evaluated
    # at the kernel's p, after checking that p against the fp32 sigmoid of the fp64 logits
    ws = loss.grad_fn.saved_tensors[3]
    B = s.shape[0]
    p_kernel = ws[B * 512:B * 512 + B * 4].view(torch.float32).cpu().clone()
    (0.5 * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), st.grad.cpu(), [p.grad.cpu() for p in params], p_kernel


@pytest.mark.parametrize("B", [2, 7, 256, 300])
@pytest.mark.parametrize("S", [2, 12, 200])
@pytest.mark.parametrize("balanced", [False, True])
@pytest.mark.parametrize("scale", [1.0, 40.0])
def test_episode_prior_matches_fp64(B, S, balanced, scale):
    ops = _ops()
    rng = np.random.RandomState(B * 7 + S + int(balanced))
    s = rng.randn(B, S).astype(np.float32)
    others, same = _draw(B, balanced, rng)
    ps = _disc_params(S, scale, seed=B + S)
    loss, ds, grads, p_kernel = _episode_run(ops, s, others, same, ps)

    # fp64 restatement: the logits in fp64; p is the fp32 Sigmoid output (the kernel's, checked against the fp32 sigmoid here)
    s64 = torch.from_numpy(s).double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in ps]
    z = episode_prior64(s64, torch.from_numpy(others), None, p64)
    p_cpu = torch.sigmoid(z.detach().float())
    assert (p_kernel.double() - p_cpu.double()).abs().max().item() <= 2e-3  # (fp32 logits over 2S terms against fp64 ones)
    p32 = p_kernel.double()
    y = torch.from_numpy(same).double()
    ref = bce_sum(p32.detach(), y)
    # backward of BCE(sum) then sigmoid at the rounded p: dz = g (p - y) / max(p (1 - p), 1e-12) * p (1 - p)
    pq = (p32 * (1 - p32)).detach()
    dz = 0.5 * (p32.detach() - y) / torch.clamp(pq, min=1e-12) * pq
    z.backward(dz)
    if scale > 1.0:
        assert (p32 == 1.0).any() or (p32 == 0.0).any(), "the scaled case should saturate some rows"
    assert abs(float(loss) - float(ref)) <= 1e-4 * max(abs(float(ref)), 1.0), (float(loss), float(ref))
    # the states get the REVERSED gradient (ReverseLayerF, lambda = 1)
    assert (ds.double() + s64.grad).abs().max().item() <= 1e-4 * max(s64.grad.abs().max().item(), 1e-6)
    for name, gk, pk in zip(("w1", "b1", "w2", "b2", "w3", "b3"), grads, p64):
        assert (gk.double() - pk.grad).abs().max().item() <= 1e-4 * max(pk.grad.abs().max().item(), 1e-6), name


def test_priors_bit_identical_between_runs():
    ops = _ops()
    rng = np.random.RandomState(5)
    B, S = 300, 200
    s = rng.randn(B, S).astype(np.float32)
    r = rng.randn(B).astype(np.float32)
    others, same = _draw(B, True, rng)
    ps = _disc_params(S, 3.0, seed=3)
    a = _episode_run(ops, s, others, same, ps)
    b = _episode_run(ops, s, others, same, ps)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)

    def rp():
        st = torch.from_numpy(s).cuda().requires_grad_(True)
        loss = ops.RewardPriorFn.apply(st, torch.from_numpy(r).cuda())
        loss.backward()
        return loss.detach().cpu(), st.grad.cpu()
    x, y = rp(), rp()
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def test_priors_reject_bad_arguments():
    ops = _ops()
    from srlz._cabi import SrlzError
    st = torch.randn(1, 4, device="cuda")
    with pytest.raises(SrlzError):
        ops.RewardPriorFn.apply(st, torch.zeros(1, device="cuda"))
    st = torch.randn(4, 3, device="cuda")
    ps = [p.cuda() for p in _disc_params(3, 1.0, 0)]
    with pytest.raises(SrlzError):  # int64 indices
        ops.EpisodePriorFn.apply(st, torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, device="cuda"), *ps)
    with pytest.raises(SrlzError):  # a discriminator of another state size
        ops.EpisodePriorFn.apply(st, torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda"),
                                 *[p.cuda() for p in _disc_params(5, 1.0, 0)])


def test_episode_prior_partner_index_range():
    """Host indices are range-checked; on the device an index outside the batch pairs its row with itself in the forward AND in both
    backward passes (the same result as naming the row itself)."""
    ops = _ops()
    from srlz._cabi import SrlzError
    rng = np.random.RandomState(9)
    B, S = 7, 12
    s = rng.randn(B, S).astype(np.float32)
    others, same = _draw(B, False, rng)
    ps = _disc_params(S, 1.0, seed=1)
    st = torch.from_numpy(s).cuda()
    with pytest.raises(SrlzError):
        ops.EpisodePriorFn.apply(st, torch.tensor([0, 1, 2, 3, 4, 5, B]), torch.from_numpy(same).cuda(), *[p.cuda() for p in ps])
    outside, itself = others.copy(), others.copy()
    outside[3], itself[3] = B + 5, 3
    a = _episode_run(ops, s, outside, same, ps)
    b = _episode_run(ops, s, itself, same, ps)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    # host indices in range take the same path as uploaded ones
    h = ops.EpisodePriorFn.apply(st, torch.from_numpy(others.astype(np.int64)), torch.from_numpy(same).cuda(), *[p.cuda() for p in ps])
    d = ops.EpisodePriorFn.apply(st, torch.from_numpy(others.astype(np.int32)).cuda(), torch.from_numpy(same).cuda(),
                                 *[p.cuda() for p in ps])
    assert torch.equal(h.cpu(), d.cpu())
