"""The reward head fitted on a recording: `Linear(2S,H)-ReLU-Linear(H,H)-ReLU-Linear(H,2)` on [state ; next_state], cross-entropy, Adam.

    fit = fit_reward(states, rewards, episode_starts)             # -> RewardFit: state_dict, history, best_epoch ..
    dyn = LatentDynamics.from_recording(states, actions, episode_starts, rewards=rewards)    # srlz/deploy.py: forward AND reward head
    dyn.refit_reward(states, rewards, episode_starts)                                        # of a representation without trained heads

The forward head has a closed form (srlz/dynfit.py); the reference's reward head (models/forward_inverse.py:78-95) has none and needs
SGD.  The defaults are train.py's own (30 epochs, batch size 32, learning rate 0.005), the labels the learner's (the reward of frame
i, -1 read as 0: deploy.reward_classes), the loss the reference's plain cross-entropy (losses/losses.py:158), the kept epoch the
one with the lowest validation loss (the learner's rule for srl_model.pth).  A minibatch of this size is launch latency and nothing
else, so route "kernel" runs a whole epoch in ONE launch (csrc/headfit.hip, srlz_headfit_fit), the validation phase in one more
(srlz_headfit_eval) and copies the parameters into a snapshot row — per epoch, with no host synchronisation until the last epoch is
enqueued.  Route "torch" is the same loop with autograd and torch.optim.Adam on the device over the same tables: for shapes
srlz_headfit_supported refuses, or when forced for a measurement.  There is no CPU path.  DESIGN.md §3.21.

minibatch_tables, validation_tables, split_starts, fit_route_for, initial_parameters and check_fit_reward are pure host functions: no GPU is asked for.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from . import ops

ROUTE_KERNEL, ROUTE_TORCH = "kernel", "torch"
KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")  # reward_net's state_dict, in order
COUNTS = ops.REWARD_PROBE_COUNTS
DEFAULT_HIDDEN, DEFAULT_EPOCHS, DEFAULT_BATCH_SIZE, DEFAULT_LR = 16, 30, 32, 0.005


def fit_route_for(S, H):
    """The route fit_reward takes for state_dim S and H hidden units (host only: no GPU is asked for)."""
    return ROUTE_KERNEL if ops.headfit_supported(S, H) else ROUTE_TORCH


def param_shapes(S, H):
    """The six shapes of the head's state_dict, in order."""
    return ((H, 2 * S), (H,), (H, H), (H,), (2, H), (2,))


def minibatch_tables(train, epochs, batch_size, seed):
    """The training tables, one int32 [steps, B] per epoch: np.random.RandomState(seed + epoch).permutation(train) cut into full
    batches, the ragged tail dropped; B = min(batch_size, len(train))."""
    train = np.asarray(train, np.int32).reshape(-1)
    if train.size < 1 or int(batch_size) < 1 or int(epochs) < 1:
        raise ValueError("minibatch_tables needs at least one transition, one epoch and a batch of one, got %d, %d and %d"
                         % (train.size, epochs, batch_size))
    b = min(int(batch_size), train.size)
    steps = train.size // b
    return [np.ascontiguousarray(np.random.RandomState(int(seed) + e).permutation(train)[:steps * b].reshape(steps, b).astype(np.int32))
            for e in range(int(epochs))]


def validation_tables(val, batch_size):
    """The validation transitions in ascending order: (int32 [n, B] of the full batches or None, int32 [1, r] of the short last one
    or None); B = min(batch_size, len(val))."""
    val = np.sort(np.asarray(val, np.int32).reshape(-1))
    if val.size < 1 or int(batch_size) < 1:
        raise ValueError("validation_tables needs at least one transition and a batch of one")
    b = min(int(batch_size), val.size)
    n = val.size // b
    full = np.ascontiguousarray(val[:n * b].reshape(n, b))
    tail = np.ascontiguousarray(val[n * b:].reshape(1, -1)) if val.size > n * b else None
    return full, tail


def split_starts(starts, episode_starts, val_fraction=0.2, seed=0):
    """A list of transitions cut in two by whole episodes -> (fit, select), int32 ascending: RandomState(seed).permutation over the E
    episodes that `starts` touches, the last ceil(val_fraction * E) of it are `select`.  What a caller uses who keeps its own
    validation transitions out of the choice of the epoch.  ValueError with fewer than 2 such episodes."""
    from . import dynfit
    starts = np.unique(np.asarray(starts, np.int64).reshape(-1))
    vf = float(val_fraction)
    if not (0.0 < vf < 1.0):
        raise ValueError("val_fraction must lie in (0, 1), got %r" % (val_fraction,))
    ids = dynfit.episode_ids(episode_starts)
    if starts.size and (starts.min() < 0 or starts.max() >= ids.size):
        raise ValueError("starts must be frame indices of the recording")
    episodes = np.unique(ids[starts])
    if episodes.size < 2:
        raise ValueError("a split by episodes needs at least 2 episodes, the transitions touch %d" % episodes.size)
    perm = np.random.RandomState(int(seed)).permutation(episodes.size)
    chosen = episodes[perm[episodes.size - int(math.ceil(vf * episodes.size)):]]
    side = np.isin(ids[starts], chosen)
    return starts[~side].astype(np.int32), starts[side].astype(np.int32)


def initial_parameters(S, H, seed):
    """The reference head's own initialisation as an OrderedDict of fp32 tensors: BaseRewardModel.initRewardNet(S, n_hidden=H) built
    under torch.random.fork_rng() with torch.manual_seed(seed) — the caller's RNG state is untouched."""
    from models.forward_inverse import BaseRewardModel
    with torch.random.fork_rng():
        torch.manual_seed(int(seed))
        head = BaseRewardModel()
        head.initRewardNet(int(S), n_hidden=int(H))
    return OrderedDict((k, v.detach().clone().float()) for k, v in head.reward_net.state_dict().items())


def flatten(state, S, H):
    """A state dict with the head's six keys -> fp32 numpy [P] in state_dict order.  ValueError: a missing key or another shape."""
    parts = []
    for key, shape in zip(KEYS, param_shapes(S, H)):
        if key not in state:
            raise ValueError("init lacks the key %r (the head's keys are %s)" % (key, list(KEYS)))
        t = state[key]
        t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        if tuple(t.shape) != shape:
            raise ValueError("init[%r] has shape %s, the head with state_dim %d and %d hidden units needs %s"
                             % (key, tuple(t.shape), S, H, shape))
        if not np.isfinite(t).all():
            raise ValueError("init[%r] holds NaN or infinite entries" % key)
        parts.append(np.ascontiguousarray(t, dtype=np.float32).reshape(-1))
    return np.concatenate(parts)


def unflatten(flat, S, H):
    """fp32 [P] in state_dict order -> OrderedDict of fp32 tensors with the head's six keys."""
    flat = np.asarray(flat, np.float32).reshape(-1)
    out, off = OrderedDict(), 0
    for key, shape in zip(KEYS, param_shapes(S, H)):
        n = int(np.prod(shape))
        out[key] = torch.from_numpy(flat[off:off + n].reshape(shape).copy())
        off += n
    return out


class RewardFit(object):
    """What fit_reward returns.  state_dict: the kept epoch's parameters, fp32 tensors under the six reward_net-relative keys;
    params: the same, flat; hidden, state_dim; history: per epoch {train_loss, val_loss, train_counts, val_counts (the five counters
    of ops.REWARD_PROBE_COUNTS), train_accuracy, val_accuracy}; best_epoch: the kept epoch, from 0; steps: the Adam steps taken;
    count / val_count: the training / validation transitions; route: "kernel" or "torch"; seed, epochs, batch_size (as used), lr,
    keep."""
    __slots__ = ("state_dict", "params", "hidden", "state_dim", "history", "best_epoch", "steps", "count", "val_count", "route", "seed",
                 "epochs", "batch_size", "lr", "keep")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def as_dict(self):
        """What evaluation.predict_forward --fit-reward writes under "reward_fit"."""
        return {"route": self.route, "hidden": self.hidden, "epochs": self.epochs, "batch_size": self.batch_size, "lr": self.lr,
                "seed": self.seed, "best_epoch": self.best_epoch, "count": self.count, "val_count": self.val_count,
                "train_loss": [h["train_loss"] for h in self.history], "val_loss": [h["val_loss"] for h in self.history],
                "train_accuracy": [h["train_accuracy"] for h in self.history],
                "val_accuracy": [h["val_accuracy"] for h in self.history]}


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _check_starts(starts, name, n):
    starts = _host(starts).reshape(-1)
    if not np.issubdtype(starts.dtype, np.integer):
        raise ValueError("%s must be integer frame indices (got %s)" % (name, starts.dtype))
    if starts.size and (starts.min() < 0 or starts.max() > n - 2):
        raise ValueError("%s must lie in [0, %d] (a transition needs frames i and i + 1), got %d .. %d"
                         % (name, n - 2, starts.min(), starts.max()))
    if starts.size < 1:
        raise ValueError("%s holds no transition: both sides need at least one" % name)
    return np.ascontiguousarray(starts.astype(np.int32))


def check_fit_reward(states, rewards, episode_starts, hidden=DEFAULT_HIDDEN, epochs=DEFAULT_EPOCHS, batch_size=DEFAULT_BATCH_SIZE,
                     lr=DEFAULT_LR, seed=0, starts=None, val_starts=None, init=None, keep="best", route=None):
    """Every check of fit_reward that needs no GPU -> dict(labels int32 [N], train, val int32, hidden, epochs, batch_size, lr, init
    fp32 [P], route).  ValueError: states that are not floating point [N,S] or (a host array) not finite; lengths that disagree; a
    third reward class; fewer than one transition on a side, or a transition on both; epochs < 1, batch_size < 1, hidden < 1, a non-positive or non-finite
    lr; an init whose keys or shapes do not match; an unknown keep or route; route "kernel" for a shape it refuses."""
    from . import deploy, dynfit
    if not isinstance(states, (np.ndarray, torch.Tensor)):
        raise ValueError("states must be a numpy array or a torch tensor, got %s" % type(states).__name__)
    is_float = np.issubdtype(states.dtype, np.floating) if isinstance(states, np.ndarray) else states.dtype.is_floating_point
    if not is_float:
        raise ValueError("states must be floating point (got %s)" % (states.dtype,))
    if len(states.shape) != 2 or states.shape[1] < 1 or states.shape[0] < 2:
        raise ValueError("states must be a recorded sequence [N,S] of at least two frames, got shape %s" % (tuple(states.shape),))
    n, s = int(states.shape[0]), int(states.shape[1])
    if isinstance(states, np.ndarray) and not np.isfinite(states).all():
        raise ValueError("states must be finite: the recording holds NaN or infinite entries")
    rewards, es = _host(rewards).reshape(-1), _host(episode_starts).reshape(-1)
    if rewards.shape[0] != n or es.shape[0] != n:
        raise ValueError("states, rewards and episode_starts must have one entry per frame, got %d, %d and %d"
                         % (n, rewards.shape[0], es.shape[0]))
    if keep not in ("best", "last"):
        raise ValueError("keep must be 'best' or 'last', got %r" % (keep,))
    if route not in (None, ROUTE_KERNEL, ROUTE_TORCH):
        raise ValueError("route must be None, 'kernel' or 'torch', got %r" % (route,))
    h, ep, b = int(hidden), int(epochs), int(batch_size)
    if h < 1 or ep < 1 or b < 1:
        raise ValueError("hidden, epochs and batch_size must be at least 1, got %r, %r and %r" % (hidden, epochs, batch_size))
    rate = float(lr)
    if not (math.isfinite(rate) and rate > 0.0):
        raise ValueError("lr must be finite and > 0, got %r" % (lr,))
    labels = deploy.reward_classes(rewards).astype(np.int32)  # (a third class is its ValueError)
    if starts is None or val_starts is None:
        tr, va = dynfit.split_episodes(es, 0.2, seed)
        starts = tr if starts is None else starts
        val_starts = va if val_starts is None else val_starts
    train, val = _check_starts(starts, "starts", n), _check_starts(val_starts, "val_starts", n)
    both = np.intersect1d(train, val)
    if both.size:
        raise ValueError("starts and val_starts share %d transitions (the first: frame %d): the kept epoch would be picked on "
                         "transitions that were trained on" % (both.size, int(both[0])))
    flat = flatten(initial_parameters(s, h, seed) if init is None else init, s, h)
    picked = route
    if picked is None:
        picked = fit_route_for(s, h) if n * s < 2 ** 31 else ROUTE_TORCH
    elif picked == ROUTE_KERNEL and not (ops.headfit_supported(s, h) and n * s < 2 ** 31):
        raise ValueError("route 'kernel' does not take state_dim %d with %d hidden units over %d frames (srlz_headfit_supported)"
                         % (s, h, n))
    return {"labels": labels, "train": train, "val": val, "hidden": h, "epochs": ep, "batch_size": b, "lr": rate, "init": flat,
            "route": picked, "seed": int(seed), "keep": keep, "state_dim": s}


def _split_flat(flat, S, H):
    out, off = [], 0
    for shape in param_shapes(S, H):
        n = int(np.prod(shape))
        out.append(flat[off:off + n].view(shape))
        off += n
    return out


def _torch_logits(x, p):
    f = torch.nn.functional
    return f.linear(f.relu(f.linear(f.relu(f.linear(x, p[0], p[1])), p[2], p[3])), p[4], p[5])


def _torch_counts(z, lab):
    pred = (z[:, 1] > z[:, 0]).long()  # a tie goes to class 0
    ok, one = pred == lab, lab == 1
    return torch.stack(((ok).sum(), (ok & ~one).sum(), (ok & one).sum(), (~one).sum(), one.sum()))


def _torch_epoch(data, table, p, opt, loss_out, counts_out):
    """Route "torch", one training epoch: the same steps through autograd and torch.optim.Adam, the statistics added on the device."""
    x, lab = data.states, data.labels.long()
    for row in table:
        i = row.long()
        z = _torch_logits(torch.cat((x[i], x[i + 1]), dim=1), p)
        y = lab[i]
        loss = torch.nn.functional.cross_entropy(z, y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        with torch.no_grad():
            loss_out += loss.detach().double() * row.shape[0]
            counts_out += _torch_counts(z.detach(), y)


def _torch_eval(data, table, p, loss_out, counts_out):
    with torch.no_grad():
        i = table.reshape(-1).long()
        z = _torch_logits(torch.cat((data.states[i], data.states[i + 1]), dim=1), p)
        y = data.labels.long()[i]
        loss_out += torch.nn.functional.cross_entropy(z.double(), y, reduction="sum")
        counts_out += _torch_counts(z, y)


def fit_reward(states, rewards, episode_starts, hidden=DEFAULT_HIDDEN, epochs=DEFAULT_EPOCHS, batch_size=DEFAULT_BATCH_SIZE,
               lr=DEFAULT_LR, seed=0, starts=None, val_starts=None, init=None, keep="best", route=None):
    """Train the reward head on a recorded sequence -> RewardFit.
    states: floating point [N,S], a host array or a device tensor (read as fp32); rewards, episode_starts [N]; starts / val_starts:
    the training / validation transitions, frame indices (default: dynfit.split_episodes(episode_starts, 0.2, seed), whole episodes
    on one side); init: a state dict with the head's six keys (default: initial_parameters(S, hidden, seed)); keep: "best" (lowest
    validation loss, ties to the earliest epoch) or "last"; route: None (fit_route_for), "kernel" or "torch".  The ValueErrors are
    check_fit_reward's, raised before any GPU work."""
    cfg = check_fit_reward(states, rewards, episode_starts, hidden, epochs, batch_size, lr, seed, starts, val_starts, init, keep, route)
    s, h, ep, picked = cfg["state_dim"], cfg["hidden"], cfg["epochs"], cfg["route"]
    tables = minibatch_tables(cfg["train"], ep, cfg["batch_size"], cfg["seed"])
    val_full, val_tail = validation_tables(cfg["val"], cfg["batch_size"])
    from models.learner import _requireGpu
    _requireGpu(True)
    if isinstance(states, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(states, dtype=np.float32)).cuda()
    else:
        x = states.detach().to("cuda" if states.device.type != "cuda" else states.device, torch.float32).contiguous()
        if not bool(torch.isfinite(x).all()):
            raise ValueError("states must be finite: the recording holds NaN or infinite entries")
    dev = x.device
    data = ops.RewardProbeData(x, torch.from_numpy(cfg["labels"]).to(dev))
    # every table is built and uploaded once
    up = (lambda t: ops.headfit_table(data, torch.from_numpy(t))) if picked == ROUTE_KERNEL else (lambda t: torch.from_numpy(t).to(dev))
    d_tables = [up(t) for t in tables]
    d_val = [up(t) for t in (val_full, val_tail) if t is not None]
    n_par = ops.headfit_n_params(s, h)
    params = torch.from_numpy(cfg["init"]).to(dev)
    snaps = torch.empty((ep, n_par), dtype=torch.float32, device=dev)
    tr_loss, va_loss = torch.zeros(ep, dtype=torch.float64, device=dev), torch.zeros(ep, dtype=torch.float64, device=dev)
    tr_counts, va_counts = torch.zeros((ep, 5), dtype=torch.int64, device=dev), torch.zeros((ep, 5), dtype=torch.int64, device=dev)
    steps = 0
    if picked == ROUTE_KERNEL:
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        for e in range(ep):
            ops.headfit_fit(data, d_tables[e], h, params, m, v, steps, cfg["lr"], tr_loss[e:e + 1], tr_counts[e])
            steps += tables[e].shape[0]
            for tb in d_val:
                ops.headfit_eval(data, tb, h, params, va_loss[e:e + 1], va_counts[e])
            snaps[e].copy_(params)
    else:
        leaves = [t.clone().requires_grad_(True) for t in _split_flat(params, s, h)]
        opt = torch.optim.Adam(leaves, lr=cfg["lr"])
        for e in range(ep):
            _torch_epoch(data, d_tables[e], leaves, opt, tr_loss[e:e + 1], tr_counts[e])
            steps += tables[e].shape[0]
            for tb in d_val:
                _torch_eval(data, tb, leaves, va_loss[e:e + 1], va_counts[e])
            with torch.no_grad():
                torch.cat([t.detach().reshape(-1) for t in leaves], out=snaps[e])
    # the one synchronisation of the run: the per-epoch statistics come to the host
    tr_loss, va_loss, tr_counts, va_counts = tr_loss.cpu().numpy(), va_loss.cpu().numpy(), tr_counts.cpu().numpy(), va_counts.cpu().numpy()
    rows, val_rows = int(tables[0].size), int(cfg["val"].size)
    history = []
    for e in range(ep):
        history.append({"train_loss": float(tr_loss[e] / rows), "val_loss": float(va_loss[e] / val_rows),
                        "train_counts": [int(c) for c in tr_counts[e]], "val_counts": [int(c) for c in va_counts[e]],
                        "train_accuracy": float(tr_counts[e][0]) / rows, "val_accuracy": float(va_counts[e][0]) / val_rows})
    best = int(np.argmin([hh["val_loss"] for hh in history])) if cfg["keep"] == "best" else ep - 1  # argmin: ties to the earliest
    flat = snaps[best].cpu().numpy()
    return RewardFit(state_dict=unflatten(flat, s, h), params=flat, hidden=h, state_dim=s, history=history, best_epoch=best, steps=steps,
                     count=int(cfg["train"].size), val_count=val_rows, route=picked, seed=cfg["seed"], epochs=ep,
                     batch_size=int(tables[0].shape[1]), lr=cfg["lr"], keep=cfg["keep"])
