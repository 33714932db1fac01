"""The reward probe of evaluation/predict_reward.py restated in float64 numpy, from its definition:

    x_b   = [states[i_b] ; states[i_b + 1]]                                    (2S values)
    h1    = relu(W1 x + b1),  h2 = relu(W2 h1 + b2),  z = W3 h2 + b3           (W1 [4, 2S], W2 [4, 4], W3 [2, 4])
    loss  = mean_b (logsumexp(z_b) - z_b[y_b])                                 (cross-entropy, mean over the minibatch)
    Adam  : m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,
            p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)        (torch's defaults: b1 0.9, b2 0.999, eps 1e-8)
    stats : running_loss += loss * B;  prediction = argmax z (a tie -> class 0);  correct / per-class counts

Parameters are ONE flat vector in state_dict order: reward_net.0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias.
Also here: the generated datasets of the reward-probe tests (the arrays of tests/dataset_util.make_dataset without its frames) and
the comparison helpers the GPU tests share.  Nothing in this file is taken from the reference's program text."""
import json
import os

import numpy as np

H, C = 4, 2
KEYS = ("reward_net.0.weight", "reward_net.0.bias", "reward_net.2.weight", "reward_net.2.bias", "reward_net.4.weight",
        "reward_net.4.bias")
COUNTS = ("correct", "correct_0", "correct_1", "rows_0", "rows_1")
MARGIN = 1e-4  # a row whose |z1 - z0| is below MARGIN * max|z| may be predicted either way by a float32 forward


def n_params(S):
    return 8 * S + 34


def shapes(S):
    return ((H, 2 * S), (H,), (H, H), (H,), (C, H), (C,))


def unflatten(flat, S):
    out, o = [], 0
    for shp in shapes(S):
        n = int(np.prod(shp))
        out.append(flat[o:o + n].reshape(shp))
        o += n
    assert o == flat.size, (o, flat.size)
    return out


def flatten_state_dict(sd):
    """state_dict (torch tensors or arrays) -> flat float64 vector in KEYS order."""
    return np.concatenate([np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float64).reshape(-1)
                           for k in KEYS])


def rows(states, idx):
    idx = np.asarray(idx, dtype=np.int64)
    st = np.asarray(states, dtype=np.float64)
    return np.concatenate([st[idx], st[idx + 1]], axis=1)


def forward(flat, X):
    w1, b1, w2, b2, w3, b3 = unflatten(flat, X.shape[1] // 2)
    h1 = np.maximum(X @ w1.T + b1, 0.0)
    h2 = np.maximum(h1 @ w2.T + b2, 0.0)
    z = h2 @ w3.T + b3
    return h1, h2, z


def row_losses(z, y):
    mx = z.max(axis=1)
    return mx + np.log(np.exp(z - mx[:, None]).sum(axis=1)) - z[np.arange(len(y)), y]


def loss_and_grad(flat, X, y):
    """-> (mean loss, gradient as a flat vector, logits)."""
    S = X.shape[1] // 2
    w1, b1, w2, b2, w3, b3 = unflatten(flat, S)
    h1, h2, z = forward(flat, X)
    B = X.shape[0]
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    dz = p.copy()
    dz[np.arange(B), y] -= 1.0
    dz /= B
    da2 = (dz @ w3) * (h2 > 0)
    da1 = (da2 @ w2) * (h1 > 0)
    g = np.concatenate([(da1.T @ X).reshape(-1), da1.sum(0), (da2.T @ h1).reshape(-1), da2.sum(0), (dz.T @ h2).reshape(-1), dz.sum(0)])
    return float(row_losses(z, y).mean()), g, z


def adam(flat, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """One step, t 1-based -> (flat, m, v), new arrays."""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
    return flat - lr / (1.0 - b1 ** t) * (m / denom), m, v


def count(z, y):
    """-> int64 [5] in COUNTS order; a tie predicts class 0."""
    pred = (z[:, 1] > z[:, 0]).astype(np.int64)
    ok = pred == y
    return np.array([ok.sum(), (ok & (y == 0)).sum(), (ok & (y == 1)).sum(), (y == 0).sum(), (y == 1).sum()], dtype=np.int64)


def soft_rows(z):
    """Rows whose prediction a float32 forward may flip."""
    return np.abs(z[:, 1] - z[:, 0]) < MARGIN * np.abs(z).max()


def count_bounds(z, y):
    """(lowest, highest) value of every counter when each soft row may go either way, and the number of soft rows."""
    soft = soft_rows(z)
    pred = (z[:, 1] > z[:, 0]).astype(np.int64)
    ok = (pred == y) & ~soft
    lo = np.array([ok.sum(), (ok & (y == 0)).sum(), (ok & (y == 1)).sum(), (y == 0).sum(), (y == 1).sum()], dtype=np.int64)
    hi = lo + np.array([soft.sum(), (soft & (y == 0)).sum(), (soft & (y == 1)).sum(), 0, 0], dtype=np.int64)
    return lo, hi, int(soft.sum())


class Phase(object):
    """What one phase (a table of minibatches) leaves behind."""

    def __init__(self):
        self.running_loss, self.step_loss, self.z, self.y = 0.0, [], [], []

    def add(self, loss, z, y):
        self.running_loss += loss * len(y)
        self.step_loss.append(loss)
        self.z.append(z)
        self.y.append(y)

    def logits(self):
        return np.concatenate(self.z), np.concatenate(self.y)

    def counts(self):
        return count(*self.logits())

    def bounds(self):
        return count_bounds(*self.logits())


def fit(flat, m, v, t0, states, labels, table, lr):
    """len(table) Adam steps -> (flat, m, v, Phase, per-step gradients)."""
    ph, grads = Phase(), []
    labels = np.asarray(labels, dtype=np.int64)
    for s, idx in enumerate(np.asarray(table, dtype=np.int64)):
        loss, g, z = loss_and_grad(flat, rows(states, idx), labels[idx])
        ph.add(loss, z, labels[idx])
        grads.append(g)
        flat, m, v = adam(flat, g, m, v, t0 + s + 1, lr)
    return flat, m, v, ph, grads


def evaluate(flat, states, labels, table):
    ph = Phase()
    labels = np.asarray(labels, dtype=np.int64)
    for idx in np.asarray(table, dtype=np.int64):
        z = forward(flat, rows(states, idx))[2]
        ph.add(float(row_losses(z, labels[idx]).mean()), z, labels[idx])
    return ph


def scale_err(got, ref):
    """max |got - ref| over the scale max |ref| of the tensor."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------------------
# datasets
# ---------------------------------------------------------------------------------------------------------------------------------
def dataset_arrays(n_episodes, ep_len, n_actions=6, seed=0):
    """The arrays tests/dataset_util.make_dataset stores (same random stream, same values), without rendering its frames."""
    rs = np.random.RandomState(seed)
    actions, rewards, starts, states, targets = [], [], [], [], []
    for _ in range(n_episodes):
        targets.append(rs.rand(3))
        pos = rs.rand(3)
        for t in range(ep_len):
            actions.append(rs.randint(0, n_actions))
            rewards.append(float(rs.rand() > 0.8))
            starts.append(t == 0)
            states.append(pos.copy())
            pos = np.clip(pos + 0.05 * rs.randn(3), 0, 1)
    return dict(actions=np.array(actions), rewards=np.array(rewards), episode_starts=np.array(starts),
                ground_truth_states=np.array(states), target_positions=np.array(targets))


def write_dataset(root, name, arrays, int_rewards=False):
    """data/<name>/{preprocessed_data.npz, ground_truth.npz, dataset_config.json} under `root` (no frames: the probe reads none)."""
    folder = os.path.join(root, "data", name)
    os.makedirs(folder, exist_ok=True)
    rewards = arrays["rewards"].astype(np.int64) if int_rewards else arrays["rewards"]
    np.savez(os.path.join(folder, "preprocessed_data.npz"), actions=arrays["actions"], rewards=rewards,
             episode_starts=arrays["episode_starts"])
    np.savez(os.path.join(folder, "ground_truth.npz"), ground_truth_states=arrays["ground_truth_states"],
             target_positions=arrays["target_positions"])
    with open(os.path.join(folder, "dataset_config.json"), "w") as f:
        json.dump({"relative_pos": False}, f)
    return name


def latent_states(arrays, dim, seed):
    """A stand-in for learned states, float32 [N, dim]: a fixed random map of the ground truth, bent, plus a little noise and a
    faint trace of the reward, so that the probe has something to find."""
    rs = np.random.RandomState(seed)
    gt = arrays["ground_truth_states"]
    a = rs.randn(gt.shape[1], dim)
    st = np.tanh(gt @ a) + 0.05 * rs.randn(gt.shape[0], dim)
    st[:, 0] += 0.5 * np.roll(arrays["rewards"], -1)  # the reward of a transition shows in its next state
    return st.astype(np.float32)


DATASET = "reward_probe_test"
# the recorded runs (tools/make_golden.py reward_probe); `preseed` is the torch seed set before the script starts
CASES = (
    dict(name="ground_truth", n_episodes=12, ep_len=40, data_seed=5, preseed=11, seed=1, bs=8, epochs=10, lr=0.005, latent=0),
    dict(name="latent_12", n_episodes=12, ep_len=40, data_seed=6, preseed=12, seed=3, bs=8, epochs=10, lr=0.005, latent=12),
)


def replay_tables(indices, seed, bs, epochs):
    """The minibatch order of the run, from its definition: torch seeded with `seed`, sklearn's train_test_split(indices,
    test_size=0.8, random_state=seed), one shuffling DataLoader over the train indices and one in-order DataLoader over the val
    indices, walked train then val once per epoch; minibatches shorter than bs are drawn but dropped.
    :return: [(train table, val table)] per epoch, int64 arrays [full minibatches, bs]"""
    import torch as th
    from sklearn.model_selection import train_test_split
    from torch.utils.data import TensorDataset, DataLoader
    th.manual_seed(seed)
    x_train, x_val = train_test_split(np.asarray(indices, dtype=np.int64), test_size=0.8, random_state=seed)
    loaders = [DataLoader(TensorDataset(th.from_numpy(x_train)), batch_size=bs, shuffle=True),
               DataLoader(TensorDataset(th.from_numpy(x_val)), batch_size=bs, shuffle=False)]
    out = []
    for _ in range(epochs):
        out.append(tuple(np.array([b[0].numpy() for b in loader if len(b[0]) >= bs], dtype=np.int64).reshape(-1, bs)
                         for loader in loaders))
    return out


def case_arrays(case):
    return dataset_arrays(case["n_episodes"], case["ep_len"], seed=case["data_seed"])


def write_case(root, case, int_rewards=False):
    """-> argv of predict_reward for this case (run it with `root` as the working directory)."""
    arrays = case_arrays(case)
    write_dataset(root, DATASET, arrays, int_rewards=int_rewards)
    argv = ["--data-folder", "data/" + DATASET, "--epochs", str(case["epochs"]), "-bs", str(case["bs"]), "--seed", str(case["seed"]),
            "-lr", str(case["lr"])]
    if case["latent"]:
        path = os.path.join(root, "states_rewards.npz")
        np.savez(path, states=latent_states(arrays, case["latent"], case["data_seed"] + 100), rewards=arrays["rewards"])
        argv += ["-i", path]
    return argv


def case_states(case):
    arrays = case_arrays(case)
    return latent_states(arrays, case["latent"], case["data_seed"] + 100) if case["latent"] else arrays["ground_truth_states"]


def load_fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reward_probe.npz"), allow_pickle=False)


def load_spread():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reward_probe_spread.json")) as f:
        return json.load(f)
