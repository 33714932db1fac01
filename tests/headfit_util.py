"""The reward head of srlz/headfit.py restated in float64 numpy, from its definition, for any hidden width H:

    x_b   = [states[i_b] ; states[i_b + 1]]                                    (2S values)
    h1    = relu(W1 x + b1),  h2 = relu(W2 h1 + b2),  z = W3 h2 + b3           (W1 [H, 2S], W2 [H, H], W3 [2, H])
    loss  = mean_b (logsumexp(z_b) - z_b[y_b])                                 (cross-entropy, mean over the minibatch)
    Adam, statistics: tests/reward_util.py (adam, count, count_bounds, Phase), which do not depend on the width

Parameters are ONE flat vector in state_dict order: 0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias (reward_net's own keys).
Also here: the recordings, splits and minibatch tables of the recorded runs (tools/make_golden_headfit.py writes
tests/golden/headfit_kats.npz from them; the GPU tests replay them).  The split and the tables are restated from their definition,
not imported from the package: tests/test_headfit_host_cpu.py holds the package's functions to these.
Nothing in this file is taken from the reference's program text."""
import json
import math
import os

import numpy as np

import reward_util as ru

KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")
C = 2


def n_params(S, H):
    return 2 * S * H + H + H * H + H + 2 * H + 2


def shapes(S, H):
    return ((H, 2 * S), (H,), (H, H), (H,), (C, H), (C,))


def unflatten(flat, S, H):
    out, o = [], 0
    for shp in shapes(S, H):
        n = int(np.prod(shp))
        out.append(flat[o:o + n].reshape(shp))
        o += n
    assert o == flat.size, (o, flat.size)
    return out


def flatten_state_dict(sd):
    """state_dict (torch tensors or arrays) -> flat float64 vector in KEYS order."""
    return np.concatenate([np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float64).reshape(-1)
                           for k in KEYS])


def forward(flat, X, H):
    w1, b1, w2, b2, w3, b3 = unflatten(flat, X.shape[1] // 2, H)
    h1 = np.maximum(X @ w1.T + b1, 0.0)
    h2 = np.maximum(h1 @ w2.T + b2, 0.0)
    return h1, h2, h2 @ w3.T + b3


def loss_and_grad(flat, X, y, H):
    """-> (mean loss, gradient as a flat vector, logits)."""
    w1, b1, w2, b2, w3, b3 = unflatten(flat, X.shape[1] // 2, H)
    h1, h2, z = forward(flat, X, H)
    B = X.shape[0]
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    dz = p.copy()
    dz[np.arange(B), y] -= 1.0
    dz /= B
    da2 = (dz @ w3) * (h2 > 0)
    da1 = (da2 @ w2) * (h1 > 0)
    g = np.concatenate([(da1.T @ X).reshape(-1), da1.sum(0), (da2.T @ h1).reshape(-1), da2.sum(0), (dz.T @ h2).reshape(-1), dz.sum(0)])
    return float(ru.row_losses(z, y).mean()), g, z


def fit(flat, m, v, t0, states, labels, table, lr, H):
    """len(table) Adam steps -> (flat, m, v, Phase, per-step gradients)."""
    ph, grads = ru.Phase(), []
    labels = np.asarray(labels, dtype=np.int64)
    for s, idx in enumerate(np.asarray(table, dtype=np.int64)):
        loss, g, z = loss_and_grad(flat, ru.rows(states, idx), labels[idx], H)
        ph.add(loss, z, labels[idx])
        grads.append(g)
        flat, m, v = ru.adam(flat, g, m, v, t0 + s + 1, lr)
    return flat, m, v, ph, grads


def evaluate(flat, states, labels, tables, H):
    """The forward over every table of `tables` (minibatches of any length) -> Phase; its running_loss is the sum of the row losses."""
    ph = ru.Phase()
    labels = np.asarray(labels, dtype=np.int64)
    for table in tables:
        for idx in np.asarray(table, dtype=np.int64):
            z = forward(flat, ru.rows(states, idx), H)[2]
            ph.add(float(ru.row_losses(z, labels[idx]).mean()), z, labels[idx])
    return ph


def random_params(S, H, seed, scale=0.5):
    """A flat float32 parameter vector with entries of both signs, large enough that every layer matters."""
    rs = np.random.RandomState(seed)
    parts = [rs.uniform(-1, 1, shp) * scale / math.sqrt(max(1, shp[-1] if len(shp) == 2 else 1)) for shp in shapes(S, H)]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the recorded runs (tools/make_golden_headfit.py)
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = (
    dict(name="latent_12", S=12, H=16, n_episodes=10, ep_len=30, data_seed=21, seed=4, bs=8, epochs=5, lr=0.005, latent=12),
    dict(name="ground_truth_3", S=3, H=16, n_episodes=10, ep_len=30, data_seed=22, seed=5, bs=8, epochs=5, lr=0.005, latent=0),
)


def case_recording(case):
    """-> (states float32 [N,S], rewards float [N], episode_starts bool [N], actions [N]): 6 actions, about one reward in five is 1."""
    arrays = ru.dataset_arrays(case["n_episodes"], case["ep_len"], n_actions=6, seed=case["data_seed"])
    st = ru.latent_states(arrays, case["latent"], case["data_seed"] + 100) if case["latent"] else arrays["ground_truth_states"]
    return np.asarray(st, np.float32), arrays["rewards"], arrays["episode_starts"], arrays["actions"]


def labels_of(rewards):
    """The learner's rule: the reward of frame i, -1 read as 0."""
    return np.maximum(np.asarray(rewards), 0).astype(np.int64)


def split(episode_starts, val_fraction, seed):
    """(train, val) transitions, int32 ascending, whole episodes on one side: RandomState(seed).permutation(E), the last
    ceil(val_fraction * E) episodes of it are validation; a transition is a frame whose successor does not start an episode."""
    es = np.asarray(episode_starts).reshape(-1) != 0
    first = es.copy()
    first[0] = True
    ids = np.cumsum(first) - 1
    E = int(ids[-1]) + 1
    perm = np.random.RandomState(seed).permutation(E)
    is_val = np.zeros(E, bool)
    is_val[perm[E - int(math.ceil(val_fraction * E)):]] = True
    tr = np.flatnonzero(~es[1:]).astype(np.int32)
    return tr[~is_val[ids[tr]]], tr[is_val[ids[tr]]]


def train_tables(train, epochs, bs, seed):
    """Per epoch RandomState(seed + epoch).permutation(train) cut into full batches of min(bs, len(train)), the tail dropped."""
    b = min(bs, len(train))
    n = len(train) // b
    return [np.random.RandomState(seed + e).permutation(train)[:n * b].reshape(n, b).astype(np.int32) for e in range(epochs)]


def val_tables(val, bs):
    """val ascending in batches of min(bs, len(val)); a short last batch is a table of its own."""
    val = np.sort(np.asarray(val, np.int32))
    b = min(bs, len(val))
    n = len(val) // b
    out = [val[:n * b].reshape(n, b)]
    if len(val) > n * b:
        out.append(val[n * b:].reshape(1, -1))
    return out


def case_tables(case):
    """-> (train starts, val starts, [train table per epoch], [val tables]) of a recorded run: the split and the tables of seed."""
    es = case_recording(case)[2]
    train, val = split(es, 0.2, case["seed"])
    return train, val, train_tables(train, case["epochs"], case["bs"], case["seed"]), val_tables(val, case["bs"])


def float64_run(case, init_flat):
    """The float64 trajectory of a recorded run from `init_flat` -> dict(flat, phases [(train Phase, val Phase)], steps, loss
    [epochs, 2] as the runs report it: running sum over the rows of the phase)."""
    states, rewards, _, _ = case_recording(case)
    labels = labels_of(rewards)
    train, val, tables, vtabs = case_tables(case)
    flat = np.asarray(init_flat, np.float64).copy()
    m, v, t, phases = np.zeros_like(flat), np.zeros_like(flat), 0, []
    loss = np.zeros((case["epochs"], 2))
    for e, table in enumerate(tables):
        flat, m, v, ph, _ = fit(flat, m, v, t, states, labels, table, case["lr"], case["H"])
        t += len(table)
        pv = evaluate(flat, states, labels, vtabs, case["H"])
        phases.append((ph, pv))
        loss[e] = ph.running_loss / table.size, pv.running_loss / len(val)
    return dict(flat=flat, phases=phases, steps=t, loss=loss, states=states, labels=labels)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    return np.load(os.path.join(GOLDEN, "headfit_kats.npz"), allow_pickle=False)


def load_spread():
    with open(os.path.join(GOLDEN, "headfit_spread.json")) as f:
        return json.load(f)
