"""The forward head in closed form: fit `state + Linear(cat(state, onehot(action)))` to a recorded sequence by least squares.

    fit = fit_forward(states, actions, episode_starts)            # -> ForwardFit: weight, bias (fp32), weight64, bias64, gram, cross ..
    dyn = LatentDynamics.from_recording(states, actions, episode_starts)     # srlz/deploy.py: dynamics for a representation that
    dyn.refit_forward(states, actions, episode_starts)                       # has no trained forward head (PCA, ground truth, an AE ..)

The reference's forward head predicts the state's change with one Linear (models/forward_inverse.py:16,30-31) and is trained with an
MSE.  Over a recorded dataset the minimiser needs no SGD: with z = [s | onehot(a) | 1] and y = s' - s it solves the normal equations
of a (S + A + 1)-square system.  The only work that grows with the dataset is G = sum z zᵀ and C = sum z yᵀ over the transitions:
route "gram" is csrc/dynfit.hip (fp64 MFMA, nothing materialised, reproducible bits, G exactly symmetric), route "torch" builds Z and
Y in fp64 on the device and takes two matmuls — for shapes srlz_dynfit_supported refuses, or when forced for a measurement.  The
small system is solved in fp64 numpy on the host.  DESIGN.md §3.20.  The reward head of the same representations has no closed
form: srlz/headfit.py trains it on the recording (LatentDynamics.refit_reward, from_recording(rewards=)), and srlz/invfit.py the
inverse head (refit_inverse, from_recording(inverse_fit=)); the split by episodes and the heads-only module are shared with them.

transitions, split_episodes and solve_forward_head are pure host functions: no GPU is asked for.
"""
import math

import numpy as np
import torch

from . import ops

ROUTE_GRAM, ROUTE_TORCH = "gram", "torch"
DEFAULT_RIDGE = 1e-6


def transitions(episode_starts, n=None):
    """int32 indices i with i + 1 < n and not episode_starts[i + 1]: the frames whose successor belongs to the same episode — the
    selection of evaluation/predict_reward.py:60 and of deploy.valid_steps(., 1).  n: the frames looked at (default: all)."""
    es = np.asarray(episode_starts).reshape(-1) != 0
    n = es.shape[0] if n is None else int(n)
    if n < 0 or n > es.shape[0]:
        raise ValueError("n must lie in [0, %d], got %d" % (es.shape[0], n))
    if n < 2:
        return np.zeros(0, np.int32)
    return np.flatnonzero(~es[1:n]).astype(np.int32)


def episode_ids(episode_starts):
    """int64 [N]: the episode of every frame, counted from 0; frame 0 opens an episode whether it is flagged or not."""
    es = np.asarray(episode_starts).reshape(-1) != 0
    if es.shape[0] == 0:
        return np.zeros(0, np.int64)
    first = es.copy()
    first[0] = True
    return np.cumsum(first).astype(np.int64) - 1


def split_episodes(episode_starts, val_fraction=0.2, seed=0):
    """(train_starts, val_starts): the transitions of the recording, int32 ascending, whole episodes on one side.  The draw is
    np.random.RandomState(seed).permutation(E) over the E episodes and the last ceil(val_fraction * E) of it are validation.
    ValueError with fewer than 2 episodes, a val_fraction outside (0, 1), or when either side ends up without a transition."""
    vf = float(val_fraction)
    if not (0.0 < vf < 1.0):
        raise ValueError("val_fraction must lie in (0, 1), got %r" % (val_fraction,))
    ids = episode_ids(episode_starts)
    n_episodes = int(ids[-1]) + 1 if ids.size else 0
    if n_episodes < 2:
        raise ValueError("a split by episodes needs at least 2 episodes, the recording has %d" % n_episodes)
    perm = np.random.RandomState(seed).permutation(n_episodes)
    n_val = int(math.ceil(vf * n_episodes))
    is_val = np.zeros(n_episodes, bool)
    is_val[perm[n_episodes - n_val:]] = True
    tr = transitions(episode_starts)
    side = is_val[ids[tr]]
    train, val = tr[~side], tr[side]
    if train.size < 1 or val.size < 1:
        raise ValueError("the split leaves %d training and %d validation transitions: both sides need at least one"
                         % (train.size, val.size))
    return train, val


def check_ridge(ridge):
    r = float(ridge)
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("ridge must be finite and > 0, got %r (the one-hot columns sum to the constant column: without it the "
                         "system is singular)" % (ridge,))
    return r


def solve_forward_head(G, C, n, S, A, ridge=DEFAULT_RIDGE):
    """(weight64 [S, S+A], bias64 [S]) from the normal equations G [P,P] = sum z zᵀ, C [P,S] = sum z yᵀ over n transitions,
    P = S + A + 1: the unique minimiser of
        J(W, b) = (1/n) sum_i |y_i - W z'_i - b|^2 + ridge |W|_F^2,        z' = z without the constant column,
    i.e. the solution of (G/n + ridge D) thetaᵀ = C/n with D = diag(1, .., 1, 0): the bias is not penalised.
    The one-hot columns of z sum to its constant column, so G alone is ALWAYS singular; ridge must be finite and > 0 (ValueError),
    and then the system is positive definite: G/n is positive semi-definite, ridge D is positive on every direction but the constant
    one, and on that one G/n gives 1.  fp64 numpy: one solve and one step of iterative refinement."""
    r = check_ridge(ridge)
    S, A, n = int(S), int(A), int(n)
    p = S + A + 1
    G, C = np.asarray(G, np.float64), np.asarray(C, np.float64)
    if G.shape != (p, p) or C.shape != (p, S):
        raise ValueError("G and C must be [%d,%d] and [%d,%d], got %s and %s" % (p, p, p, S, G.shape, C.shape))
    if n < 1:
        raise ValueError("no transition at all (n=%d)" % n)
    lhs = G / n
    lhs[np.arange(p - 1), np.arange(p - 1)] += r
    rhs = C / n
    theta = np.linalg.solve(lhs, rhs)
    theta = theta + np.linalg.solve(lhs, rhs - lhs @ theta)
    return np.ascontiguousarray(theta[:p - 1].T), np.ascontiguousarray(theta[p - 1])


class ForwardFit(object):
    """What fit_forward returns.  weight [S, S+A] and bias [S]: fp32 numpy, shaped like forward_net.weight / .bias; weight64, bias64:
    the fp64 solution they were rounded from; count: the transitions; gram [P,P], cross [P,S]: the fp64 normal equations on the
    host; ridge, state_dim, n_actions; route: "gram" or "torch"."""
    __slots__ = ("weight", "bias", "weight64", "bias64", "count", "gram", "cross", "ridge", "state_dim", "n_actions", "route")

    def __init__(self, weight64, bias64, count, gram, cross, ridge, state_dim, n_actions, route):
        self.weight64, self.bias64 = weight64, bias64
        self.weight, self.bias = weight64.astype(np.float32), bias64.astype(np.float32)
        self.count, self.gram, self.cross, self.ridge = int(count), gram, cross, float(ridge)
        self.state_dim, self.n_actions, self.route = int(state_dim), int(n_actions), route


def fit_route_for(S, A):
    """The route fit_forward takes for state_dim S and A actions (host only: no GPU is asked for)."""
    return ROUTE_GRAM if ops.dynfit_supported(S, A) else ROUTE_TORCH


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def check_fit_recording(states, actions, episode_starts, n_actions=None, starts=None):
    """Validate the recording of a fit_forward call -> (actions int32 [N], starts int32 [M], n_actions), host arrays.  ValueError
    (the wording of deploy.check_recording): states that are not floating point [N,S], lengths that disagree, non-integer actions,
    a start without a successor, no transition at all, an action outside [0, n_actions) inside a listed transition."""
    if not isinstance(states, (np.ndarray, torch.Tensor)):
        raise ValueError("states must be a numpy array or a torch tensor, got %s" % type(states).__name__)
    is_float = np.issubdtype(states.dtype, np.floating) if isinstance(states, np.ndarray) else states.dtype.is_floating_point
    if not is_float:
        raise ValueError("states must be floating point (got %s)" % (states.dtype,))
    if len(states.shape) != 2 or states.shape[1] < 1:
        raise ValueError("states must be a recorded sequence [N,S], got shape %s" % (tuple(states.shape),))
    n = int(states.shape[0])
    actions = _host(actions).reshape(-1)
    if not np.issubdtype(actions.dtype, np.integer):
        if not np.all(actions == np.floor(actions)):
            raise ValueError("actions must be integers (got %s)" % (actions.dtype,))
        actions = actions.astype(np.int64)
    es = _host(episode_starts).reshape(-1)
    if actions.shape[0] != n or es.shape[0] != n:
        raise ValueError("states, actions and episode_starts must have one entry per frame, got %d, %d and %d"
                         % (n, actions.shape[0], es.shape[0]))
    if starts is None:
        starts = transitions(es)
    else:
        starts = _host(starts).reshape(-1)
        if not np.issubdtype(starts.dtype, np.integer):
            raise ValueError("starts must be integer frame indices (got %s)" % (starts.dtype,))
        if starts.size and (starts.min() < 0 or starts.max() > n - 2):
            raise ValueError("starts must lie in [0, %d] (a transition needs frames i and i + 1), got %d .. %d"
                             % (n - 2, starts.min(), starts.max()))
    if starts.size < 1:
        raise ValueError("no transition at all: every frame is the last of its episode")
    used = actions[starts]
    lo, hi = int(used.min()), int(used.max())
    if n_actions is None:
        n_actions = hi + 1
    n_actions = int(n_actions)
    if n_actions < 1 or lo < 0 or hi >= n_actions:
        raise ValueError("actions must lie in [0, %d) inside every listed transition, got %d .. %d" % (n_actions, lo, hi))
    listed = np.zeros(n, bool)
    listed[starts] = True
    return np.where(listed, actions, 0).astype(np.int32), np.ascontiguousarray(starts.astype(np.int32)), n_actions


def _torch_gram(x, d_actions, d_starts, n_actions):
    """Route "torch": Z [M,P] and Y [M,S] in fp64 on the device, then two matmuls."""
    i = d_starts.long()
    s0 = x[i].double()
    onehot = torch.nn.functional.one_hot(d_actions[i].long(), n_actions).double()
    z = torch.cat((s0, onehot, torch.ones((i.shape[0], 1), dtype=torch.float64, device=x.device)), dim=1)
    y = x[i + 1].double() - s0
    return z.t() @ z, z.t() @ y


def fit_forward(states, actions, episode_starts, n_actions=None, ridge=DEFAULT_RIDGE, starts=None, route=None):
    """Least-squares fit of the forward head on a recorded sequence -> ForwardFit.
    states: floating point [N,S], a host array or a device tensor (read as fp32, the heads' precision); actions, episode_starts [N];
    starts: the transitions to fit on, frame indices (default: transitions(episode_starts)); n_actions: default max(action) + 1 over
    the listed transitions; ridge: see solve_forward_head; route: None (fit_route_for), "gram" or "torch"."""
    r = check_ridge(ridge)
    if route not in (None, ROUTE_GRAM, ROUTE_TORCH):
        raise ValueError("route must be None, 'gram' or 'torch', got %r" % (route,))
    acts, st, a = check_fit_recording(states, actions, episode_starts, n_actions, starts)
    n, s = int(states.shape[0]), int(states.shape[1])
    picked = route
    if picked is None:
        picked = fit_route_for(s, a) if n * s < 2 ** 31 else ROUTE_TORCH
    elif picked == ROUTE_GRAM and not ops.dynfit_supported(s, a):
        raise ValueError("route 'gram' does not take state_dim %d with %d actions (srlz_dynfit_supported)" % (s, a))
    if isinstance(states, np.ndarray) and not np.isfinite(states).all():
        raise ValueError("states must be finite: the recording holds NaN or infinite entries")
    from models.learner import _requireGpu
    _requireGpu(True)
    if isinstance(states, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(states, dtype=np.float32)).cuda()
    else:
        x = states.detach().to("cuda" if states.device.type != "cuda" else states.device, torch.float32).contiguous()
        if not bool(torch.isfinite(x).all()):
            raise ValueError("states must be finite: the recording holds NaN or infinite entries")
    d_acts = torch.from_numpy(acts).to(x.device)
    h_starts = torch.from_numpy(st)
    if picked == ROUTE_GRAM:
        gram, cross = ops.dynfit_gram(x, d_acts, h_starts, a)
    else:
        gram, cross = _torch_gram(x, d_acts, h_starts.to(x.device), a)
    gram, cross = gram.cpu().numpy(), cross.cpu().numpy()
    w64, b64 = solve_forward_head(gram, cross, st.shape[0], s, a, r)
    return ForwardFit(w64, b64, st.shape[0], gram, cross, r, s, a, picked)


_HEADS_ONLY = []


def heads_only_modules(state_dim, n_actions):
    """SRLModules with the three heads and NO encoder, losses = ["forward"]: what LatentDynamics.from_recording puts behind a
    representation that has no network (created on the host, as every model here; move it with .to(device))."""
    if not _HEADS_ONLY:
        from models.modules import SRLModules
        from models.forward_inverse import BaseForwardModel, BaseInverseModel, BaseRewardModel

        class HeadsOnlyModules(SRLModules):
            def __init__(self, state_dim, action_dim):
                self.model_type, self.losses = "custom_cnn", ["forward"]
                BaseForwardModel.__init__(self)
                BaseInverseModel.__init__(self)
                BaseRewardModel.__init__(self)
                self.cuda = True  # (sic: SRLModules stores the flag under this name)
                self.initForwardNet(state_dim, action_dim)
                self.initInverseNet(state_dim, action_dim)
                self.initRewardNet(state_dim)
                self.model = None

            def getStates(self, observations):
                raise NotImplementedError("a recording has no encoder: its states are the representation")

            def forward(self, x):
                raise NotImplementedError("a recording has no encoder: its states are the representation")
        _HEADS_ONLY.append(HeadsOnlyModules)
    return _HEADS_ONLY[0](int(state_dim), int(n_actions))
