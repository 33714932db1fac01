"""The inverse head of srlz/invfit.py restated in float64 numpy, from its definition, for any number of actions A:

    x_b   = [states[i_b] ; states[i_b + 1]]                                    (2S values)
    z     = W x + b                                                            (W [A, 2S], b [A])
    loss  = mean_b (logsumexp(z_b) - z_b[y_b]),  y_b = actions[i_b]            (cross-entropy, mean over the minibatch)
    a label outside [0, A): its row adds nothing to the loss or the gradient (the mean still divides by B) and counts as `bad`
    Adam: tests/reward_util.py (adam), which does not depend on the model
    stats : running_loss += loss * B;  prediction = argmax z (a tie -> the lowest class);
            counts = rows, correct, bad, support[A] (rows labelled a), hits[A] (of which predicted a)

Parameters are ONE flat vector in state_dict order: weight, bias (inverse_net's own keys).
Also here: the recordings, splits and minibatch tables of the recorded runs (tools/make_golden_invfit.py writes
tests/golden/invfit_kats.npz from them; the GPU tests replay them).  The split and the tables are headfit_util's restatements,
which tests/test_invfit_host_cpu.py holds the package's functions to.
Nothing in this file is taken from the reference's program text."""
import json
import os

import numpy as np

import headfit_util as hu
import reward_util as ru

KEYS = ("weight", "bias")
MARGIN = 1e-4  # a row whose two largest logits lie within MARGIN * max|z| of each other may be predicted either way in float32


def n_params(S, A):
    return 2 * S * A + A


def n_counts(A):
    return 3 + 2 * A


def chunk_rows(S, A):
    """include/srlz.h, srlz_invfit_chunk_rows: the formula, restated."""
    if S < 1 or A < 2:
        return 0
    K, APAD = 2 * S, ((A + 3) & ~3) | 4
    room = 40444 - 2 * (K + 2) * APAD
    if room < 0:
        return 0
    r = room // ((K | 1) + APAD + 3)
    return 0 if r < 16 else min(128, r)


def unflatten(flat, S, A):
    assert flat.size == n_params(S, A), (flat.size, S, A)
    return [flat[:2 * S * A].reshape(A, 2 * S), flat[2 * S * A:]]


def flatten_state_dict(sd):
    return np.concatenate([np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float64).reshape(-1)
                           for k in KEYS])


def forward(flat, X, A):
    w, b = unflatten(flat, X.shape[1] // 2, A)
    return X @ w.T + b


def row_losses(z, y):
    """The row losses; 0 for a label outside [0, A)."""
    good = (y >= 0) & (y < z.shape[1])
    ys = np.where(good, y, 0)
    mx = z.max(axis=1)
    l = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1)) - z[np.arange(len(y)), ys]
    return np.where(good, l, 0.0)


def loss_and_grad(flat, X, y, A):
    """-> (mean loss, gradient as a flat vector, logits)."""
    z = forward(flat, X, A)
    B = X.shape[0]
    good = (y >= 0) & (y < A)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    dz = p.copy()
    dz[np.arange(B)[good], y[good]] -= 1.0
    dz[~good] = 0.0
    dz /= B
    g = np.concatenate([(dz.T @ X).reshape(-1), dz.sum(0)])
    return float(row_losses(z, y).sum() / B), g, z


def count(z, y):
    """-> int64 [3 + 2A]; a tie predicts the lowest class."""
    A = z.shape[1]
    good = (y >= 0) & (y < A)
    pred = z.argmax(axis=1)
    ok = good & (pred == y)
    support = np.bincount(y[good], minlength=A)
    hits = np.bincount(y[ok], minlength=A)
    return np.concatenate(([len(y), ok.sum(), (~good).sum()], support, hits)).astype(np.int64)


def soft_rows(z):
    """Rows whose prediction a float32 forward may flip: the two largest logits within MARGIN * max|z| of each other."""
    top = np.sort(z, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < MARGIN * np.abs(z).max()


def count_bounds(z, y):
    """(lowest, highest) value of every counter when each soft row may go either way, and the number of soft rows."""
    A = z.shape[1]
    good = (y >= 0) & (y < A)
    soft = soft_rows(z) & good
    ok = good & (z.argmax(axis=1) == y) & ~soft
    support = np.bincount(y[good], minlength=A)
    lo = np.concatenate(([len(y), ok.sum(), (~good).sum()], support, np.bincount(y[ok], minlength=A))).astype(np.int64)
    hi = lo.copy()
    hi[1] += soft.sum()
    hi[3 + A:] += np.bincount(y[soft], minlength=A)
    return lo, hi, int(soft.sum())


class Phase(ru.Phase):
    def counts(self):
        return count(*self.logits())

    def bounds(self):
        return count_bounds(*self.logits())


def fit(flat, m, v, t0, states, labels, table, lr, A):
    """len(table) Adam steps -> (flat, m, v, Phase, per-step gradients)."""
    ph, grads = Phase(), []
    labels = np.asarray(labels, dtype=np.int64)
    for s, idx in enumerate(np.asarray(table, dtype=np.int64)):
        loss, g, z = loss_and_grad(flat, ru.rows(states, idx), labels[idx], A)
        ph.add(loss, z, labels[idx])
        grads.append(g)
        flat, m, v = ru.adam(flat, g, m, v, t0 + s + 1, lr)
    return flat, m, v, ph, grads


def evaluate(flat, states, labels, tables, A):
    """The forward over every table of `tables` (minibatches of any length) -> Phase; its running_loss is the sum of the row losses."""
    ph = Phase()
    labels = np.asarray(labels, dtype=np.int64)
    for table in tables:
        for idx in np.asarray(table, dtype=np.int64):
            z = forward(flat, ru.rows(states, idx), A)
            ph.add(float(row_losses(z, labels[idx]).mean()), z, labels[idx])
    return ph


def random_params(S, A, seed, scale=0.5):
    """A flat float32 parameter vector with entries of both signs, large enough that the logits differ."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(-1, 1, (A, 2 * S)) * scale / np.sqrt(2 * S)
    return np.concatenate([w.reshape(-1), rs.uniform(-1, 1, A) * scale]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the recorded runs (tools/make_golden_invfit.py)
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = (
    dict(name="ground_truth_3", S=3, A=6, n_episodes=10, ep_len=30, data_seed=31, seed=2, bs=8, epochs=5, lr=0.005, latent=0),
    dict(name="latent_12", S=12, A=4, n_episodes=10, ep_len=30, data_seed=32, seed=3, bs=8, epochs=5, lr=0.005, latent=12),
)


def case_recording(case):
    """-> (states float32 [N,S], actions int64 [N], episode_starts bool [N]).  The state moves by its action: frame i + 1 = frame i
    + step[a_i] + noise in the first three coordinates of the ground truth, so the inverse head has something to find; the latent
    case sees it through a fixed random map, bent, plus a little noise."""
    rs = np.random.RandomState(case["data_seed"])
    A, n = case["A"], case["n_episodes"] * case["ep_len"]
    step = 0.08 * rs.randn(A, 3)
    actions = rs.randint(0, A, n)
    starts = (np.arange(n) % case["ep_len"]) == 0
    pos = np.zeros((n, 3))
    for i in range(n):
        pos[i] = rs.rand(3) if starts[i] else pos[i - 1] + step[actions[i - 1]] + 0.03 * rs.randn(3)
    if case["latent"]:
        mix = rs.randn(3, case["latent"])
        pos = np.tanh(pos @ mix) + 0.02 * rs.randn(n, case["latent"])
    return pos.astype(np.float32), actions.astype(np.int64), starts


def case_tables(case):
    """-> (train starts, val starts, [train table per epoch], [val tables]) of a recorded run: the split and the tables of seed."""
    es = case_recording(case)[2]
    train, val = hu.split(es, 0.2, case["seed"])
    return train, val, hu.train_tables(train, case["epochs"], case["bs"], case["seed"]), hu.val_tables(val, case["bs"])


def float64_run(case, init_flat):
    """The float64 trajectory of a recorded run from `init_flat` -> dict(flat, phases [(train Phase, val Phase)], steps, loss
    [epochs, 2] as the runs report it: running sum over the rows of the phase, states, labels)."""
    states, actions, _ = case_recording(case)
    train, val, tables, vtabs = case_tables(case)
    flat = np.asarray(init_flat, np.float64).copy()
    m, v, t, phases = np.zeros_like(flat), np.zeros_like(flat), 0, []
    loss = np.zeros((case["epochs"], 2))
    for e, table in enumerate(tables):
        flat, m, v, ph, _ = fit(flat, m, v, t, states, actions, table, case["lr"], case["A"])
        t += len(table)
        pv = evaluate(flat, states, actions, vtabs, case["A"])
        phases.append((ph, pv))
        loss[e] = ph.running_loss / table.size, pv.running_loss / len(val)
    return dict(flat=flat, phases=phases, steps=t, loss=loss, states=states, labels=actions)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    return np.load(os.path.join(GOLDEN, "invfit_kats.npz"), allow_pickle=False)


def load_spread():
    with open(os.path.join(GOLDEN, "invfit_spread.json")) as f:
        return json.load(f)
