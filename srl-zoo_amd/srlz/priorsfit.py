"""A state map fitted on a recording by the four robotic priors alone: s = W x + b, W [S, D] (Jonschkowski & Brock's linear map).

    fit = fit_priors(features, actions, rewards, episode_starts, state_dim=3)        # -> PriorsFit: weight, bias, history ..
    states = fit.transform(features)                                                 # -> fp32 [N, S] on the device
    dyn = LatentDynamics.from_recording(states, actions, episode_starts)             # srlz/deploy.py: heads, plans, metrics

The features are whatever a recording already has: the PCA baseline's components (srl_baselines.pca), an auto-encoder's states,
down-sampled pixels.  The model is nn.Linear(D, S) with its own seeded initialisation, the loss the reference's roboticPriorsLoss
(losses/losses.py:62-99: temporal coherence, causality, proportionality, repeatability, weight 1 each), the optimizer
torch.optim.Adam, the defaults train.py's own (30 epochs, batch size 32, learning rate 0.005).  The loop is the learner's
(reference models/learner.py:277-297): the transitions that stay inside an episode are shuffled once and cut into sorted
minibatches (the ragged tail dropped), round(val_size * n) minibatches are held out, the pairs are mined ONCE over that list
(losses/utils.py priors_pairs, its over-sampling included), the ORDER of the training minibatches is reshuffled every epoch, and
the kept epoch is the one with the lowest validation loss.  One difference, as in srlz/headfit.py and srlz/invfit.py: an epoch is
its training phase and then its validation phase; the reference interleaves validation minibatches with training steps.

Route "kernel" runs a whole training phase in ONE launch (csrc/robotic.hip, srlz_robotic_fit), the validation phase in one more
(srlz_robotic_eval) and copies the parameters into a snapshot row — per epoch, with no host synchronisation until the last epoch
is enqueued.  The pair tables of all minibatches are uploaded once; a launch takes the epoch's order as a list of minibatch ids.
Route "torch" is the same tables through autograd and torch.optim.Adam on the device: for shapes srlz_robotic_supported refuses, or
when forced for a measurement.  Nothing is rejected for size.  There is no CPU path.  Two fits give identical bits on route
"kernel".  DESIGN.md §3.23.

fit_route_for, initial_parameters, check_fit_priors and minibatch_list are pure host functions: no GPU is asked for.
"""
import contextlib
import io
import math

import numpy as np
import torch

from . import ops

ROUTE_KERNEL, ROUTE_TORCH = "kernel", "torch"
TERMS = ops.ROBOTIC_TERMS
DEFAULT_EPOCHS, DEFAULT_BATCH_SIZE, DEFAULT_LR = 30, 32, 0.005


def fit_route_for(D, S, B):
    """The route fit_priors takes for D features, state_dim S and minibatches of B (host only: no GPU is asked for)."""
    return ROUTE_KERNEL if ops.robotic_supported(D, S, B) else ROUTE_TORCH


def initial_parameters(D, S, seed):
    """nn.Linear(D, S)'s own initialisation as (weight fp32 [S, D], bias fp32 [S]) numpy arrays, built under
    torch.random.fork_rng() with torch.manual_seed(seed): the caller's RNG state is untouched."""
    with torch.random.fork_rng():
        torch.manual_seed(int(seed))
        layer = torch.nn.Linear(int(D), int(S))
    return layer.weight.detach().numpy().copy(), layer.bias.detach().numpy().copy()


def minibatch_list(episode_starts, batch_size, seed, val_size=0.2, epochs=1):
    """The learner's cut (reference models/learner.py:277-292) from ONE np.random.RandomState(seed): the transitions i with
    episode_starts[i + 1] false, shuffled, cut into sorted minibatches of batch_size (the ragged tail dropped); then
    round(val_size * n) validation minibatch ids, the head of a permutation; then, per epoch, a permutation of the training ids.
    -> (minibatches: list of int64 arrays, val_ids int64 ascending-by-draw, orders: list of int64 arrays)."""
    es = np.asarray(episode_starts).reshape(-1) != 0
    b = int(batch_size)
    rs = np.random.RandomState(int(seed))
    indices = np.flatnonzero(~es[1:]).astype(np.int64)
    rs.shuffle(indices)
    mlist = [np.array(sorted(indices[s:s + b])) for s in range(0, len(indices) - b + 1, b)]
    n_val = int(np.round(float(val_size) * len(mlist)))
    val_ids = rs.permutation(len(mlist))[:n_val].astype(np.int64)
    held = set(int(v) for v in val_ids)
    train_ids = np.array([k for k in range(len(mlist)) if k not in held], np.int64)
    orders = [train_ids[rs.permutation(len(train_ids))] for _ in range(int(epochs))]
    return mlist, val_ids, orders


class PriorsFit(object):
    """What fit_priors returns.  weight fp32 [S, D], bias fp32 [S]: the kept epoch's map for the RAW features (a standardisation is
    folded in); state_dim, feature_dim; history: per epoch {train_loss, val_loss (means per minibatch of the four terms' sum),
    train_terms, val_terms (the four means, in the order of TERMS)}; best_epoch: the kept epoch, from 0; steps: the Adam steps
    taken; count / val_count: the training / validation transitions; minibatches_resampled: the minibatches the over-sampling
    gave a frame of another minibatch; minibatches, val_ids, dissimilar_pairs, same_actions_pairs: the tables the fit ran on;
    route: "kernel" or "torch"; seed, epochs, batch_size, lr, keep, standardize."""
    __slots__ = ("weight", "bias", "state_dim", "feature_dim", "history", "best_epoch", "steps", "count", "val_count",
                 "minibatches_resampled", "minibatches", "val_ids", "dissimilar_pairs", "same_actions_pairs", "route", "seed", "epochs",
                 "batch_size", "lr", "keep", "standardize", "_device")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))
        self._device = {}

    def transform(self, features):
        """features [M, D] (a host array or a device tensor) -> the states fp32 [M, S] on the device, one srlz_linear_fwd launch."""
        from models.learner import _requireGpu
        _requireGpu(True)
        x = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).cuda() if isinstance(features, np.ndarray) \
            else features.detach().to("cuda" if features.device.type != "cuda" else features.device, torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.feature_dim:
            raise ValueError("features must be [M, %d], got %s" % (self.feature_dim, tuple(x.shape)))
        wb = self._device.get(x.device)
        if wb is None:
            wb = self._device[x.device] = (torch.from_numpy(self.weight).to(x.device), torch.from_numpy(self.bias).to(x.device))
        with torch.no_grad():
            return ops.LinearFn.apply(x, wb[0], wb[1], False)


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def check_fit_priors(features, actions, rewards, episode_starts, state_dim, n_actions=None, epochs=DEFAULT_EPOCHS,
                     batch_size=DEFAULT_BATCH_SIZE, lr=DEFAULT_LR, seed=1, val_size=0.2, standardize=True, init=None, keep="best",
                     route=None):
    """Every check of fit_priors that needs no GPU -> dict(actions, rewards int64 [N], n_actions, minibatches, val_ids, orders,
    weight, bias (the initial map), route ..).  ValueError: features that are not floating point [N, D] or (a host array) not
    finite; lengths that disagree; non-integer actions or actions outside [0, n_actions); state_dim < 1; epochs < 1; batch_size <
    1 or larger than the transitions; a val_size that holds out no minibatch or all of them; a non-positive or non-finite lr; an
    init of another shape; an unknown keep or route; route "kernel" for a shape it does not take."""
    if not isinstance(features, (np.ndarray, torch.Tensor)):
        raise ValueError("features must be a numpy array or a torch tensor, got %s" % type(features).__name__)
    is_float = np.issubdtype(features.dtype, np.floating) if isinstance(features, np.ndarray) else features.dtype.is_floating_point
    if not is_float:
        raise ValueError("features must be floating point (got %s)" % (features.dtype,))
    if len(features.shape) != 2 or features.shape[1] < 1 or features.shape[0] < 2:
        raise ValueError("features must be a recorded sequence [N, D] of at least two frames, got shape %s" % (tuple(features.shape),))
    n, d = int(features.shape[0]), int(features.shape[1])
    if isinstance(features, np.ndarray) and not np.isfinite(features).all():
        raise ValueError("features must be finite: the recording holds NaN or infinite entries")
    actions, rewards, es = _host(actions).reshape(-1), _host(rewards).reshape(-1), _host(episode_starts).reshape(-1)
    if actions.shape[0] != n or rewards.shape[0] != n or es.shape[0] != n:
        raise ValueError("features, actions, rewards and episode_starts must have one entry per frame, got %d, %d, %d and %d"
                         % (n, actions.shape[0], rewards.shape[0], es.shape[0]))
    if not np.issubdtype(actions.dtype, np.integer):
        if not np.all(actions == np.floor(actions)):
            raise ValueError("actions must be integers (got %s)" % (actions.dtype,))
        actions = actions.astype(np.int64)
    s = int(state_dim)
    if s < 1:
        raise ValueError("state_dim must be at least 1, got %r" % (state_dim,))
    if keep not in ("best", "last"):
        raise ValueError("keep must be 'best' or 'last', got %r" % (keep,))
    if route not in (None, ROUTE_KERNEL, ROUTE_TORCH):
        raise ValueError("route must be None, 'kernel' or 'torch', got %r" % (route,))
    ep, b = int(epochs), int(batch_size)
    if ep < 1 or b < 1:
        raise ValueError("epochs and batch_size must be at least 1, got %r and %r" % (epochs, batch_size))
    rate = float(lr)
    if not (math.isfinite(rate) and rate > 0.0):
        raise ValueError("lr must be finite and > 0, got %r" % (lr,))
    a = int(actions.max()) + 1 if n_actions is None else int(n_actions)
    if actions.min() < 0 or actions.max() >= a:
        raise ValueError("actions must lie in [0, %d), got %d .. %d" % (a, int(actions.min()), int(actions.max())))
    n_trans = int((es[1:] == 0).sum())
    if b > n_trans:
        raise ValueError("batch_size %d is larger than the recording's %d transitions" % (b, n_trans))
    mlist, val_ids, orders = minibatch_list(es, b, seed, val_size, ep)
    if len(val_ids) < 1 or len(val_ids) >= len(mlist):
        raise ValueError("val_size %r holds out %d of %d minibatches: at least one and not all are needed" % (val_size, len(val_ids), len(mlist)))
    if init is None:
        w, bias = initial_parameters(d, s, seed)
    else:
        w, bias = [np.ascontiguousarray(_host(t), dtype=np.float32) for t in init]
        if w.shape != (s, d) or bias.shape != (s,):
            raise ValueError("init must be (weight [%d, %d], bias [%d]), got %s and %s" % (s, d, s, w.shape, bias.shape))
        if not (np.isfinite(w).all() and np.isfinite(bias).all()):
            raise ValueError("init holds NaN or infinite entries")
    fits = ops.robotic_supported(d, s, b) and n * d < 2 ** 31
    picked = route
    if picked is None:
        picked = ROUTE_KERNEL if fits else ROUTE_TORCH
    elif picked == ROUTE_KERNEL and not fits:
        raise ValueError("route 'kernel' does not take %d features, state_dim %d and minibatches of %d over %d frames "
                         "(srlz_robotic_supported)" % (d, s, b, n))
    return {"actions": actions.astype(np.int64), "rewards": rewards, "n_actions": a, "minibatches": mlist, "val_ids": val_ids,
            "orders": orders, "weight": w, "bias": bias, "route": picked, "seed": int(seed), "epochs": ep, "batch_size": b, "lr": rate,
            "keep": keep, "state_dim": s, "feature_dim": d, "standardize": bool(standardize)}


def _torch_terms(x, w, bias, rows, dis, same):
    """The four terms of one minibatch through torch operations (the reference's own formulation, losses/losses.py:75-90)."""
    s = torch.nn.functional.linear(x[rows], w, bias)
    ns = torch.nn.functional.linear(x[rows + 1], w, bias)
    diff = ns - s
    norm = diff.norm(2, dim=1)

    def similarity(p, q):
        return torch.exp(-(p - q).norm(2, dim=1) ** 2)
    i, j = same[:, 0], same[:, 1]
    return torch.stack(((norm ** 2).mean(), similarity(s[dis[:, 0]], s[dis[:, 1]]).mean(), ((norm[i] - norm[j]) ** 2).mean(),
                        (similarity(s[i], s[j]) * (diff[i] - diff[j]).norm(2, dim=1) ** 2).mean()))


def _torch_tables(minibatches, dis, same, device):
    """Route "torch": the same tables as int64 device tensors, uploaded once."""
    up = lambda arrays: [torch.from_numpy(np.asarray(a, np.int64)).to(device) for a in arrays]
    return up(minibatches), up(dis), up(same)


def _torch_epoch(x, w, bias, opt, tables, order, out):
    """Route "torch", one training phase: the steps of `order` through autograd and torch.optim.Adam, the terms added on the device."""
    rows, d_dis, d_same = tables
    for k in order:
        terms = _torch_terms(x, w, bias, rows[k], d_dis[k], d_same[k])
        opt.zero_grad(set_to_none=True)
        terms.sum().backward()
        opt.step()
        out += terms.detach().double()


def fit_priors(features, actions, rewards, episode_starts, state_dim, n_actions=None, epochs=DEFAULT_EPOCHS,
               batch_size=DEFAULT_BATCH_SIZE, lr=DEFAULT_LR, seed=1, val_size=0.2, standardize=True, init=None, keep="best", route=None):
    """Fit the linear state map on a recorded sequence -> PriorsFit.
    features: floating point [N, D], a host array or a device tensor (read as fp32); actions, rewards, episode_starts [N]; the
    transition of frame i is (features[i], features[i + 1]), its action actions[i], its reward rewards[i + 1]; n_actions: default
    max(action) + 1; standardize: fit on (x - mean) / std per feature (a constant feature keeps std 1) and fold both back into the
    returned weight and bias; init: (weight [S, D], bias [S]) for the features the fit runs on (default: initial_parameters(D, S,
    seed)); keep: "best" (lowest validation loss, ties to the earliest epoch) or "last"; route: None (fit_route_for), "kernel" or
    "torch".  The ValueErrors are check_fit_priors's, raised before any GPU work; losses.utils.NoPairsError (a ValueError) where a
    minibatch is left without a pair."""
    cfg = check_fit_priors(features, actions, rewards, episode_starts, state_dim, n_actions, epochs, batch_size, lr, seed, val_size,
                           standardize, init, keep, route)
    from losses.utils import priors_pairs
    s, d, ep, picked = cfg["state_dim"], cfg["feature_dim"], cfg["epochs"], cfg["route"]
    mlist, val_ids, orders = cfg["minibatches"], cfg["val_ids"], cfg["orders"]
    before = [m.copy() for m in mlist]
    with contextlib.redirect_stdout(io.StringIO()):  # (the reference's statistics lines: a library call prints nothing)
        dis, same = priors_pairs(cfg["batch_size"], mlist, cfg["actions"], cfg["rewards"], cfg["n_actions"],
                                 np.zeros(cfg["n_actions"], np.int64))
    resampled = sum(1 for a, b in zip(before, mlist) if not np.array_equal(a, b))
    from models.learner import _requireGpu
    _requireGpu(True)
    if isinstance(features, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).cuda()
    else:
        x = features.detach().to("cuda" if features.device.type != "cuda" else features.device, torch.float32).contiguous()
        if not bool(torch.isfinite(x).all()):
            raise ValueError("features must be finite: the recording holds NaN or infinite entries")
    dev = x.device
    mean = std = None
    if cfg["standardize"]:
        x64 = x.double()
        mean, std = x64.mean(0), x64.std(0, unbiased=False)
        std = torch.where(std > 0, std, torch.ones_like(std))
        x = ((x64 - mean) / std).float().contiguous()
    n_par = s * d + s
    params = torch.from_numpy(np.concatenate((cfg["weight"].reshape(-1), cfg["bias"]))).to(dev)
    snaps = torch.empty((ep, n_par), dtype=torch.float32, device=dev)
    tr, va = torch.zeros((ep, 4), dtype=torch.float64, device=dev), torch.zeros((ep, 4), dtype=torch.float64, device=dev)
    steps = 0
    if picked == ROUTE_KERNEL:
        tabs = ops.robotic_fit_tables(np.stack(mlist), dis, same, dev)
        d_orders = [ops.robotic_order(o, dev) for o in orders]
        d_val = ops.robotic_order(val_ids, dev)
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        for e in range(ep):
            ops.robotic_fit(x, tabs, d_orders[e], params, m, v, steps, cfg["lr"], tr[e])
            steps += len(orders[e])
            ops.robotic_eval(x, tabs, d_val, params, va[e])
            snaps[e].copy_(params)
    else:
        tables = _torch_tables(mlist, dis, same, dev)
        w = params[:s * d].view(s, d).clone().requires_grad_(True)
        bias = params[s * d:].clone().requires_grad_(True)
        opt = torch.optim.Adam([w, bias], lr=cfg["lr"])
        for e in range(ep):
            _torch_epoch(x, w, bias, opt, tables, orders[e], tr[e])
            steps += len(orders[e])
            with torch.no_grad():
                for k in val_ids:
                    va[e] += _torch_terms(x, w, bias, tables[0][k], tables[1][k], tables[2][k]).double()
                torch.cat((w.detach().reshape(-1), bias.detach()), out=snaps[e])
    # the one synchronisation of the run: the per-epoch statistics come to the host
    tr, va = tr.cpu().numpy() / len(orders[0]), va.cpu().numpy() / len(val_ids)
    history = [{"train_loss": float(tr[e].sum()), "val_loss": float(va[e].sum()), "train_terms": [float(t) for t in tr[e]],
                "val_terms": [float(t) for t in va[e]]} for e in range(ep)]
    best = int(np.argmin([h["val_loss"] for h in history])) if cfg["keep"] == "best" else ep - 1  # argmin: ties to the earliest
    flat = snaps[best].double()
    w64, b64 = flat[:s * d].view(s, d), flat[s * d:]
    if mean is not None:
        w64 = w64 / std
        b64 = b64 - w64.mv(mean)
    b_sz = cfg["batch_size"]
    return PriorsFit(weight=w64.float().cpu().numpy(), bias=b64.float().cpu().numpy(), state_dim=s, feature_dim=d, history=history,
                     best_epoch=best, steps=steps, count=len(orders[0]) * b_sz, val_count=len(val_ids) * b_sz,
                     minibatches_resampled=resampled, minibatches=mlist, val_ids=val_ids, dissimilar_pairs=dis, same_actions_pairs=same,
                     route=picked, seed=cfg["seed"], epochs=ep, batch_size=b_sz, lr=cfg["lr"], keep=cfg["keep"],
                     standardize=cfg["standardize"])
