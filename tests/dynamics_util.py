"""Shared by the deployment-dynamics tests and tools/make_golden_dynamics.py: the golden cases, states and plans from closed
formulas (no state is stored), seeded heads for the kernel tests and the restatement of a rollout in torch at any precision
(fp64: the reference every bound is taken against; fp32 on the CPU: the spread of fp32 arithmetic itself).
Nothing here touches a GPU or reads a file."""
from collections import OrderedDict

import numpy as np
import torch

N_ACTIONS = 6
N_ENVS, N_PLANS, HORIZON = 3, 4, 7
SEED = 3
# seeded SRLModules(state_dim, action_dim=6, losses=[forward, inverse, reward]); scale multiplies forward_net.weight after construction
CASES = OrderedDict([
    ("s3_linear", dict(state_dim=3, inverse_model_type="linear", scale=1.0)),
    ("s8_mlp", dict(state_dim=8, inverse_model_type="mlp", scale=1.0)),
    ("s200", dict(state_dim=200, inverse_model_type="linear", scale=1.0)),
    ("s200_expanding", dict(state_dim=200, inverse_model_type="linear", scale=20.0)),
])
LOSSES = ["forward", "inverse", "reward"]
QUANTITIES = ("trajectory", "reward_logits", "returns")
FLOOR = 1e-4  # the project's parity bar, of each quantity's scale


def states(n, s):
    """fp32 [n, s]: z[i][j] = 0.5 * (((5 i + 3 j) mod 7) - 3)."""
    i, j = np.meshgrid(np.arange(n), np.arange(s), indexing="ij")
    return (0.5 * (((5 * i + 3 * j) % 7) - 3)).astype(np.float32)


def sine_states(n, s):
    """fp32 [n, s]: sin(0.37 i + 0.11 j + 0.5) — values that are no multiples of a power of two."""
    i, j = np.meshgrid(np.arange(n), np.arange(s), indexing="ij")
    return np.sin(0.37 * i + 0.11 * j + 0.5).astype(np.float32)


def plans(n, k, t, a):
    """int32 [n, k, t]: (7 n + 3 k + 5 t + n k t) mod a."""
    ni, ki, ti = np.meshgrid(np.arange(n), np.arange(k), np.arange(t), indexing="ij")
    return ((7 * ni + 3 * ki + 5 * ti + ni * ki * ti) % a).astype(np.int32)


def build_case(name, modules, cuda=False):
    """The seeded model of a golden case (the reference's constructor or this build's: the same RNG stream, the same keys)."""
    c = CASES[name]
    torch.manual_seed(SEED)
    m = modules.SRLModules(state_dim=c["state_dim"], action_dim=N_ACTIONS, cuda=cuda, model_type="custom_cnn", losses=list(LOSSES),
                           inverse_model_type=c["inverse_model_type"])
    if c["scale"] != 1.0:
        with torch.no_grad():
            m.forward_net.weight.mul_(c["scale"])
    return m


def case_inputs(name):
    s = CASES[name]["state_dim"]
    return sine_states(N_ENVS, s), plans(N_ENVS, N_PLANS, HORIZON, N_ACTIONS)


HEAD_KEYS = ("forward_net.weight", "forward_net.bias", "reward_net.0.weight", "reward_net.0.bias", "reward_net.2.weight",
             "reward_net.2.bias", "reward_net.4.weight", "reward_net.4.bias")


def head_params(state_dict):
    """(wf, bf, w1, b1, w2, b2, w3, b3) of a state_dict."""
    return tuple(state_dict[k].detach() for k in HEAD_KEYS)


def checksums(state_dict):
    """fp64 [len(HEAD_KEYS), 2]: sum and sum of squares of each head parameter."""
    return np.array([[float(state_dict[k].double().sum()), float((state_dict[k].double() ** 2).sum())] for k in HEAD_KEYS])


def seeded_heads(s, a, h, seed=0, scale=1.0):
    """fp32 head parameters of any (S, A, H) for the kernel tests: nn.Linear's uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)) from a seeded
    generator; `scale` multiplies the forward weight (an expanding recurrence above ~1)."""
    g = torch.Generator().manual_seed(1000 + seed)

    def u(shape, fan_in):
        b = 1.0 / np.sqrt(fan_in)
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * b).float()
    wf = u((s, s + a), s + a) * scale
    return (wf, u((s,), s + a), u((h, 2 * s), 2 * s), u((h,), 2 * s), u((h, h), h), u((h,), h), u((2, h), h), u((2,), h))


def restate(params, z, pl, gamma=1.0, dtype=torch.float64, reward=True):
    """The rollout in torch on the CPU at `dtype`: per row s_0 = z[n], d = Wf [s ; onehot(a)] + bf, s' = s + d,
    l = W3 relu(W2 relu(W1 [s ; s'] + b1) + b2) + b3, ret += g softmax(l)[1], g *= gamma (forward_inverse.py:21-31, 78-95).
    z [N,S], pl [N,K,T] or [K,T] -> dict of numpy arrays: trajectory [N,K,T,S], final [N,K,S], reward_logits [N,K,T,2], returns [N,K]."""
    wf, bf, w1, b1, w2, b2, w3, b3 = [torch.as_tensor(p).to(dtype) for p in params]
    z = torch.as_tensor(z).to(dtype)
    pl = torch.as_tensor(np.asarray(pl)).long()
    n, s = z.shape
    if pl.dim() == 2:
        pl = pl.unsqueeze(0).expand(n, -1, -1)
    k, t = pl.shape[1], pl.shape[2]
    a = wf.shape[1] - s
    cur = z.unsqueeze(1).expand(n, k, s).reshape(n * k, s)
    acts = pl.reshape(n * k, t)
    traj, logits = [], []
    ret, g = torch.zeros(n * k, dtype=dtype), torch.ones((), dtype=dtype)
    gam = torch.tensor(gamma, dtype=torch.float32).to(dtype)  # the kernel takes gamma as a float
    for step in range(t):
        onehot = torch.zeros(n * k, a, dtype=dtype)
        onehot[torch.arange(n * k), acts[:, step]] = 1
        nxt = cur + torch.nn.functional.linear(torch.cat((cur, onehot), dim=1), wf, bf)
        traj.append(nxt)
        if reward:
            x = torch.cat((cur, nxt), dim=1)
            x = torch.relu(torch.nn.functional.linear(x, w1, b1))
            x = torch.relu(torch.nn.functional.linear(x, w2, b2))
            lg = torch.nn.functional.linear(x, w3, b3)
            logits.append(lg)
            ret = ret + g * torch.softmax(lg, dim=1)[:, 1]
            g = g * gam
        cur = nxt
    out = {"trajectory": torch.stack(traj, dim=1).reshape(n, k, t, s).numpy(), "final": cur.reshape(n, k, s).numpy()}
    if reward:
        out["reward_logits"] = torch.stack(logits, dim=1).reshape(n, k, t, 2).numpy()
        out["returns"] = ret.reshape(n, k).numpy()
    return out


def step_scale(x):
    """Scale of a per-step quantity [N,K,T,*]: max |x| of each step, shaped to broadcast ([1,1,T,1]), never below 1e-30."""
    x = np.asarray(x, np.float64)
    return np.maximum(np.abs(x).max(axis=(0, 1, 3), keepdims=True), 1e-30)


def rel_err(got, ref, per_step):
    """max |got - ref| over the quantity's scale: per step for trajectory and logits, one scale for returns."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = step_scale(ref) if per_step else max(np.abs(ref).max(), 1e-30)
    return float((np.abs(got - ref) / scale).max())


def spread(params, z, pl, gamma=1.0):
    """The fp32 torch-CPU composition against fp64 on the same inputs: {quantity: relative error}."""
    lo, hi = restate(params, z, pl, gamma, torch.float32), restate(params, z, pl, gamma, torch.float64)
    return {q: rel_err(lo[q], hi[q], q != "returns") for q in QUANTITIES}


def bound(spread_value):
    """max(1e-4, 10 x the recorded spread) of the quantity's scale."""
    return max(FLOOR, 10.0 * float(spread_value))
