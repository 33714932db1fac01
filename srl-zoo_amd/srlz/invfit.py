"""The inverse head fitted on a recording: `Linear(2S, A)` on [state ; next_state] under a cross-entropy, Adam.

    fit = fit_inverse(states, actions, episode_starts)            # -> InverseFit: state_dict, history, best_epoch ..
    dyn = LatentDynamics.from_recording(states, actions, episode_starts, inverse_fit={})     # srlz/deploy.py: forward AND inverse head
    dyn.refit_inverse(states, actions, episode_starts)                                       # of a representation without trained heads
    dyn.action_accuracy(states, actions, episode_starts)          # accuracy, majority accuracy, per-action recall

"Can the action be read off (state, next state) in this representation?" is what this zoo's default loss optimises
(--losses inverse).  The forward head has a closed form (srlz/dynfit.py) and the reward head is trained by srlz/headfit.py; this is
the third.  The head is the reference's inverseModel (models/forward_inverse.py, --inverse-model-type linear), the loss its
inverseModelLoss (losses/losses.py:117-129: nn.CrossEntropyLoss against the action of frame i), the defaults train.py's own (30
epochs, batch size 32, learning rate 0.005), the kept epoch the one with the lowest validation loss.  Transitions are
dynfit.transitions: no pair crosses an episode boundary.  The split and the minibatch tables are headfit's own functions.

Route "kernel" runs a whole epoch in ONE launch (csrc/invfit.hip, srlz_invfit_fit), the validation phase in one more
(srlz_invfit_eval) and copies the parameters into a snapshot row — per epoch, with no host synchronisation until the last epoch is
enqueued.  Route "torch" is the same loop with autograd and torch.optim.Adam on the device over the same tables: for shapes
srlz_invfit_supported refuses, for the `mlp` inverse head (Linear-ReLU-Linear-ReLU-Linear, H = 128), or when forced for a
measurement.  Nothing is rejected for size.  There is no CPU path.  DESIGN.md §3.22.

fit_route_for, initial_parameters and check_fit_inverse are pure host functions: no GPU is asked for.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .headfit import minibatch_tables, split_starts, validation_tables, _check_starts, _host  # the split and the tables are headfit's

ROUTE_KERNEL, ROUTE_TORCH = "kernel", "torch"
LINEAR, MLP = "linear", "mlp"
KEYS = {LINEAR: ("weight", "bias"), MLP: ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")}  # inverse_net's state_dict
MLP_HIDDEN = 128  # initInverseNet's n_hidden
COUNTS = ops.INVFIT_COUNTS
DEFAULT_EPOCHS, DEFAULT_BATCH_SIZE, DEFAULT_LR = 30, 32, 0.005


def fit_route_for(S, A, inverse_model_type=LINEAR):
    """The route fit_inverse takes for state_dim S, A actions and this head (host only: no GPU is asked for)."""
    if inverse_model_type not in KEYS:
        raise ValueError("inverse_model_type must be 'linear' or 'mlp', got %r" % (inverse_model_type,))
    return ROUTE_KERNEL if inverse_model_type == LINEAR and ops.invfit_supported(S, A) else ROUTE_TORCH


def param_shapes(S, A, inverse_model_type=LINEAR):
    """The shapes of the head's state_dict, in order."""
    if inverse_model_type == LINEAR:
        return ((A, 2 * S), (A,))
    h = MLP_HIDDEN
    return ((h, 2 * S), (h,), (h, h), (h,), (A, h), (A,))


def initial_parameters(S, A, seed, inverse_model_type=LINEAR):
    """The reference head's own initialisation as an OrderedDict of fp32 tensors: BaseInverseModel.initInverseNet(S, A) built under
    torch.random.fork_rng() with torch.manual_seed(seed) — the caller's RNG state is untouched."""
    from models.forward_inverse import BaseInverseModel
    with torch.random.fork_rng():
        torch.manual_seed(int(seed))
        head = BaseInverseModel()
        head.initInverseNet(int(S), int(A), model_type=inverse_model_type)
    return OrderedDict((k, v.detach().clone().float()) for k, v in head.inverse_net.state_dict().items())


def flatten(state, S, A, inverse_model_type=LINEAR):
    """A state dict with the head's keys -> fp32 numpy [P] in state_dict order.  ValueError: a missing key or another shape."""
    keys, parts = KEYS[inverse_model_type], []
    for key, shape in zip(keys, param_shapes(S, A, inverse_model_type)):
        if key not in state:
            raise ValueError("init lacks the key %r (the head's keys are %s)" % (key, list(keys)))
        t = state[key]
        t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        if tuple(t.shape) != shape:
            raise ValueError("init[%r] has shape %s, the %s head with state_dim %d and %d actions needs %s"
                             % (key, tuple(t.shape), inverse_model_type, S, A, shape))
        if not np.isfinite(t).all():
            raise ValueError("init[%r] holds NaN or infinite entries" % key)
        parts.append(np.ascontiguousarray(t, dtype=np.float32).reshape(-1))
    return np.concatenate(parts)


def unflatten(flat, S, A, inverse_model_type=LINEAR):
    """fp32 [P] in state_dict order -> OrderedDict of fp32 tensors with the head's keys."""
    flat = np.asarray(flat, np.float32).reshape(-1)
    out, off = OrderedDict(), 0
    for key, shape in zip(KEYS[inverse_model_type], param_shapes(S, A, inverse_model_type)):
        n = int(np.prod(shape))
        out[key] = torch.from_numpy(flat[off:off + n].reshape(shape).copy())
        off += n
    return out


def recall(counts, n_actions):
    """Per-action recall hits[a] / support[a] from the counters (rows, correct, bad, support[A], hits[A]); None where an action has
    no row."""
    c = [int(x) for x in counts]
    sup, hit = c[3:3 + n_actions], c[3 + n_actions:3 + 2 * n_actions]
    return [(float(h) / s if s else None) for h, s in zip(hit, sup)]


class InverseFit(object):
    """What fit_inverse returns.  state_dict: the kept epoch's parameters, fp32 tensors under inverse_net's own keys (`weight`,
    `bias`; the mlp head's six); params: the same, flat; n_actions, state_dim, inverse_model_type; history: per epoch {train_loss,
    val_loss, train_counts, val_counts (rows, correct, bad, support[A], hits[A]), train_accuracy, val_accuracy, train_recall,
    val_recall (per action, None without a row)}; best_epoch: the kept epoch, from 0; steps: the Adam steps taken; count /
    val_count: the training / validation transitions; route: "kernel" or "torch"; seed, epochs, batch_size (as used), lr, keep."""
    __slots__ = ("state_dict", "params", "n_actions", "state_dim", "inverse_model_type", "history", "best_epoch", "steps", "count",
                 "val_count", "route", "seed", "epochs", "batch_size", "lr", "keep")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def check_fit_inverse(states, actions, episode_starts, n_actions=None, epochs=DEFAULT_EPOCHS, batch_size=DEFAULT_BATCH_SIZE,
                      lr=DEFAULT_LR, seed=0, val_fraction=0.2, starts=None, val_starts=None, init=None, keep="best", route=None,
                      inverse_model_type=LINEAR):
    """Every check of fit_inverse that needs no GPU -> dict(labels int32 [N], train, val int32, n_actions, epochs, batch_size, lr,
    init fp32 [P], route ..).  ValueError: states that are not floating point [N,S] or (a host array) not finite; lengths that
    disagree; non-integer actions; n_actions < 2; an action outside [0, n_actions) inside a listed transition; fewer than one
    transition on a side, or a transition on both; epochs < 1, batch_size < 1, a non-positive or non-finite lr; an init whose keys or
    shapes do not match; an unknown keep, route or head; route "kernel" for a shape or a head it does not take."""
    from . import dynfit
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
    actions, es = _host(actions).reshape(-1), _host(episode_starts).reshape(-1)
    if actions.shape[0] != n or es.shape[0] != n:
        raise ValueError("states, actions and episode_starts must have one entry per frame, got %d, %d and %d"
                         % (n, actions.shape[0], es.shape[0]))
    if not np.issubdtype(actions.dtype, np.integer):
        if not np.all(actions == np.floor(actions)):
            raise ValueError("actions must be integers (got %s)" % (actions.dtype,))
        actions = actions.astype(np.int64)
    if keep not in ("best", "last"):
        raise ValueError("keep must be 'best' or 'last', got %r" % (keep,))
    if route not in (None, ROUTE_KERNEL, ROUTE_TORCH):
        raise ValueError("route must be None, 'kernel' or 'torch', got %r" % (route,))
    if inverse_model_type not in KEYS:
        raise ValueError("inverse_model_type must be 'linear' or 'mlp', got %r" % (inverse_model_type,))
    ep, b = int(epochs), int(batch_size)
    if ep < 1 or b < 1:
        raise ValueError("epochs and batch_size must be at least 1, got %r and %r" % (epochs, batch_size))
    rate = float(lr)
    if not (math.isfinite(rate) and rate > 0.0):
        raise ValueError("lr must be finite and > 0, got %r" % (lr,))
    if starts is None or val_starts is None:
        tr, va = dynfit.split_episodes(es, val_fraction, seed)
        starts = tr if starts is None else starts
        val_starts = va if val_starts is None else val_starts
    train, val = _check_starts(starts, "starts", n), _check_starts(val_starts, "val_starts", n)
    both = np.intersect1d(train, val)
    if both.size:
        raise ValueError("starts and val_starts share %d transitions (the first: frame %d): the kept epoch would be picked on "
                         "transitions that were trained on" % (both.size, int(both[0])))
    used = actions[np.concatenate((train, val))]
    lo, hi = int(used.min()), int(used.max())
    a = hi + 1 if n_actions is None else int(n_actions)
    if a < 2:
        raise ValueError("n_actions must be at least 2 (a classifier of one class learns nothing), got %d" % a)
    if lo < 0 or hi >= a:
        raise ValueError("actions must lie in [0, %d) inside every listed transition, got %d .. %d" % (a, lo, hi))
    listed = np.zeros(n, bool)
    listed[train], listed[val] = True, True
    labels = np.where(listed, actions, 0).astype(np.int32)  # (a frame no transition starts at is never read)
    flat = flatten(initial_parameters(s, a, seed, inverse_model_type) if init is None else init, s, a, inverse_model_type)
    fits = inverse_model_type == LINEAR and ops.invfit_supported(s, a) and n * s < 2 ** 31
    picked = route
    if picked is None:
        picked = ROUTE_KERNEL if fits else ROUTE_TORCH
    elif picked == ROUTE_KERNEL and not fits:
        raise ValueError("route 'kernel' does not take the %s head with state_dim %d and %d actions over %d frames "
                         "(srlz_invfit_supported)" % (inverse_model_type, s, a, n))
    return {"labels": labels, "train": train, "val": val, "n_actions": a, "epochs": ep, "batch_size": b, "lr": rate, "init": flat,
            "route": picked, "seed": int(seed), "keep": keep, "state_dim": s, "inverse_model_type": inverse_model_type}


def _split_flat(flat, S, A, inverse_model_type=LINEAR):
    out, off = [], 0
    for shape in param_shapes(S, A, inverse_model_type):
        n = int(np.prod(shape))
        out.append(flat[off:off + n].view(shape))
        off += n
    return out


def _torch_logits(x, p):
    f = torch.nn.functional
    for w, b in zip(p[0:-2:2], p[1:-2:2]):
        x = f.relu(f.linear(x, w, b))
    return f.linear(x, p[-2], p[-1])


def _torch_counts(z, lab, A):
    """int64 [3 + 2A] on the device: rows, correct, bad (none: the labels were checked on the host), support, hits."""
    ok = z.argmax(dim=1) == lab  # (the first maximal value: a tie goes to the lowest class)
    support = torch.bincount(lab, minlength=A)
    hits = torch.bincount(lab, weights=ok.double(), minlength=A).long()  # (whole numbers in fp64: exact in any order; no mask, no sync)
    return torch.cat((support.sum().reshape(1), hits.sum().reshape(1), torch.zeros_like(support[:1]), support, hits))


def _torch_epoch(data, table, p, opt, loss_out, counts_out, A):
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
            counts_out += _torch_counts(z.detach(), y, A)


def _torch_eval(data, table, p, loss_out, counts_out, A):
    with torch.no_grad():
        i = table.reshape(-1).long()
        z = _torch_logits(torch.cat((data.states[i], data.states[i + 1]), dim=1), p)
        y = data.labels.long()[i]
        loss_out += torch.nn.functional.cross_entropy(z.double(), y, reduction="sum")
        counts_out += _torch_counts(z, y, A)


def fit_inverse(states, actions, episode_starts, n_actions=None, epochs=DEFAULT_EPOCHS, batch_size=DEFAULT_BATCH_SIZE, lr=DEFAULT_LR,
                seed=0, val_fraction=0.2, starts=None, val_starts=None, init=None, keep="best", route=None, inverse_model_type=LINEAR):
    """Train the inverse head on a recorded sequence -> InverseFit.
    states: floating point [N,S], a host array or a device tensor (read as fp32); actions, episode_starts [N]; the label of
    transition i is actions[i]; n_actions: default max(action) + 1 over the listed transitions; starts / val_starts: the training /
    validation transitions, frame indices (default: dynfit.split_episodes(episode_starts, val_fraction, seed), whole episodes on one
    side); init: a state dict with the head's keys (default: initial_parameters(S, A, seed)); keep: "best" (lowest validation loss,
    ties to the earliest epoch) or "last"; route: None (fit_route_for), "kernel" or "torch"; inverse_model_type: "linear", or "mlp"
    (route "torch" only).  The ValueErrors are check_fit_inverse's, raised before any GPU work; after a "kernel" run whose counters
    report a label outside [0, A) (device data changed under the run) ValueError too."""
    cfg = check_fit_inverse(states, actions, episode_starts, n_actions, epochs, batch_size, lr, seed, val_fraction, starts, val_starts,
                            init, keep, route, inverse_model_type)
    s, a, ep, picked, kind = cfg["state_dim"], cfg["n_actions"], cfg["epochs"], cfg["route"], cfg["inverse_model_type"]
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
    n_par, n_cnt = int(cfg["init"].size), ops.invfit_n_counts(a)
    params = torch.from_numpy(cfg["init"]).to(dev)
    snaps = torch.empty((ep, n_par), dtype=torch.float32, device=dev)
    tr_loss, va_loss = torch.zeros(ep, dtype=torch.float64, device=dev), torch.zeros(ep, dtype=torch.float64, device=dev)
    tr_counts, va_counts = torch.zeros((ep, n_cnt), dtype=torch.int64, device=dev), torch.zeros((ep, n_cnt), dtype=torch.int64, device=dev)
    steps = 0
    if picked == ROUTE_KERNEL:
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        for e in range(ep):
            ops.invfit_fit(data, d_tables[e], a, params, m, v, steps, cfg["lr"], tr_loss[e:e + 1], tr_counts[e])
            steps += tables[e].shape[0]
            for tb in d_val:
                ops.invfit_eval(data, tb, a, params, va_loss[e:e + 1], va_counts[e])
            snaps[e].copy_(params)
    else:
        leaves = [t.clone().requires_grad_(True) for t in _split_flat(params, s, a, kind)]
        opt = torch.optim.Adam(leaves, lr=cfg["lr"])
        for e in range(ep):
            _torch_epoch(data, d_tables[e], leaves, opt, tr_loss[e:e + 1], tr_counts[e], a)
            steps += tables[e].shape[0]
            for tb in d_val:
                _torch_eval(data, tb, leaves, va_loss[e:e + 1], va_counts[e], a)
            with torch.no_grad():
                torch.cat([t.detach().reshape(-1) for t in leaves], out=snaps[e])
    # the one synchronisation of the run: the per-epoch statistics come to the host
    tr_loss, va_loss, tr_counts, va_counts = tr_loss.cpu().numpy(), va_loss.cpu().numpy(), tr_counts.cpu().numpy(), va_counts.cpu().numpy()
    bad = int(tr_counts[:, 2].sum() + va_counts[:, 2].sum())
    if bad:
        raise ValueError("the run met %d labels outside [0, %d): the actions on the device are not the ones that were checked" % (bad, a))
    rows, val_rows = int(tables[0].size), int(cfg["val"].size)
    history = []
    for e in range(ep):
        history.append({"train_loss": float(tr_loss[e] / rows), "val_loss": float(va_loss[e] / val_rows),
                        "train_counts": [int(c) for c in tr_counts[e]], "val_counts": [int(c) for c in va_counts[e]],
                        "train_accuracy": float(tr_counts[e][1]) / rows, "val_accuracy": float(va_counts[e][1]) / val_rows,
                        "train_recall": recall(tr_counts[e], a), "val_recall": recall(va_counts[e], a)})
    best = int(np.argmin([hh["val_loss"] for hh in history])) if cfg["keep"] == "best" else ep - 1  # argmin: ties to the earliest
    flat = snaps[best].cpu().numpy()
    return InverseFit(state_dict=unflatten(flat, s, a, kind), params=flat, n_actions=a, state_dim=s, inverse_model_type=kind,
                      history=history, best_epoch=best, steps=steps, count=int(cfg["train"].size), val_count=val_rows, route=picked,
                      seed=cfg["seed"], epochs=ep, batch_size=int(tables[0].shape[1]), lr=cfg["lr"], keep=cfg["keep"])
