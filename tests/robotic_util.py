"""Shared by the robotic-priors tests and tools/make_golden_robotic.py: seeded recordings, their minibatch lists as the learner cuts
them (reference models/learner.py:277-286), seeded loss cases, and a float64 numpy restatement of roboticPriorsLoss and of its
gradient, written for the tests (it shares no code with csrc/robotic.hip or with the reference)."""
import numpy as np

# N frames in E episodes of equal length, A actions, rewards = rand < p, minibatches of B, everything from `seed`
RECORDINGS = (
    dict(name="plain", N=240, E=6, A=4, p=0.3, B=16, seed=0),      # no minibatch needs the over-sampling
    dict(name="resampled", N=240, E=6, A=6, p=0.3, B=8, seed=0),   # 4 minibatches do
    dict(name="sparse", N=240, E=6, A=6, p=0.1, B=8, seed=1),      # 10 do
)
TOUCHED = {"plain": 0, "resampled": 4, "sparse": 10}               # minibatches the reference's overSampling dealt with
N_MINIBATCHES = {"plain": 14, "resampled": 29, "sparse": 29}


def recording(rec):
    """-> actions int64 [N], rewards int64 [N] (0 / 1), episode_starts bool [N]."""
    rs = np.random.RandomState(rec["seed"])
    actions = rs.randint(0, rec["A"], rec["N"]).astype(np.int64)
    rewards = (rs.rand(rec["N"]) < rec["p"]).astype(np.int64)
    starts = np.zeros(rec["N"], bool)
    starts[::rec["N"] // rec["E"]] = True
    return actions, rewards, starts


def minibatch_list(rec, episode_starts, sort=True):
    """The learner's cut: the transitions that stay inside an episode, shuffled once under np.random.seed(seed), cut into minibatches
    of B (sorted, unless sort=False), the ragged tail dropped.  The global numpy RNG is left as it was found."""
    n, b = rec["N"], rec["B"]
    indices = np.array([i for i in range(n - 1) if not episode_starts[i + 1]], dtype="int64")
    state = np.random.get_state()
    np.random.seed(rec["seed"])
    np.random.shuffle(indices)
    np.random.set_state(state)
    cut = [indices[s:s + b] for s in range(0, len(indices) - b + 1, b)]
    return [np.array(sorted(m)) if sort else np.array(m) for m in cut]


# (B, S, actions, seed): loss cases; the pairs are all same-action pairs i < j, the dissimilar ones by a seeded 0 / 1 reward
LOSS_CASES = (
    dict(name="b2s1", B=2, S=1, A=1, seed=11),
    dict(name="b3s3", B=3, S=3, A=1, seed=12),
    dict(name="b16s3", B=16, S=3, A=3, seed=13),
    dict(name="b33s8", B=33, S=8, A=4, seed=14),
    dict(name="b259s5", B=259, S=5, A=6, seed=15),
    dict(name="b256one", B=256, S=3, A=1, seed=16),   # ONE action: 32 640 same-action pairs, 255 incidences per row
)


def loss_case(case):
    """-> states, next_states float32 [B, S] (unit normal, shrunk where two rows would lie further apart than |.|^2 = 18, so that no
    similarity underflows towards 0; next = states + a unit normal step), dis int64 [nD, 2], same int64 [nP, 2] in generation
    order.  Without a dissimilar pair in the seeded rewards the first same-action pair serves as one."""
    rs = np.random.RandomState(case["seed"])
    b, s = case["B"], case["S"]
    states = rs.randn(b, s)
    gram = states.dot(states.T)
    widest = (np.diag(gram)[:, None] + np.diag(gram)[None, :] - 2.0 * gram).max()
    states = (states * min(1.0, np.sqrt(18.0 / widest))).astype(np.float32)  # no two rows further apart than |.|^2 = 18
    next_states = (states + rs.randn(b, s)).astype(np.float32)
    actions = rs.randint(0, case["A"], b)
    rewards = rs.randint(0, 2, b)
    same = np.array([[i, j] for i in range(b) for j in range(i + 1, b) if actions[i] == actions[j]], dtype=np.int64)
    dis = np.array([[i, j] for i, j in same if rewards[i] != rewards[j]], dtype=np.int64)
    if dis.size == 0:
        dis = same[:1].copy()
    return states, next_states, dis, same


ZERO_ROWS = (2, 5)


def zero_step_case():
    """The b16s3 case with next_states[b] = states[b] in the rows ZERO_ROWS: their step has length 0."""
    states, next_states, dis, same = loss_case(LOSS_CASES[2])
    next_states = next_states.copy()
    for b in ZERO_ROWS:
        next_states[b] = states[b]
    return states, next_states, dis, same


def ragged(arrays):
    """A list of [n_k, 2] arrays -> (their concatenation [sum n_k, 2], offsets [len + 1]); split() undoes it."""
    offsets = np.concatenate(([0], np.cumsum([len(a) for a in arrays]))).astype(np.int64)
    flat = np.concatenate([np.asarray(a, np.int64).reshape(-1, 2) for a in arrays])
    return flat, offsets


def split(flat, offsets):
    return [flat[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def variants(dis, same, seed):
    """The pair lists in generated order, shuffled, and with duplicates and reversed pairs (plus one i == j entry each)."""
    rs = np.random.RandomState(seed)
    out = [("generated", dis, same)]
    out.append(("shuffled", dis[rs.permutation(len(dis))], same[rs.permutation(len(same))]))

    def rough(p):
        extra = p[rs.randint(0, len(p), max(1, len(p) // 3))]
        q = np.concatenate((p, extra, np.array([[p[0, 0], p[0, 0]]])))
        flip = rs.rand(len(q)) < 0.5
        q[flip] = q[flip][:, ::-1]
        return q[rs.permutation(len(q))]
    out.append(("duplicates_reversed", rough(dis), rough(same)))
    return out


def priors_f64(states, next_states, dis, same, weights=(1.0, 1.0, 1.0, 1.0)):
    """float64: the four terms [4] and the gradients of sum_k weights[k] * term_k with respect to states and next_states.
    Where a row's step has length 0 the proportionality term sends nothing into it (the subgradient torch.norm's backward takes)."""
    s, ns = np.asarray(states, np.float64), np.asarray(next_states, np.float64)
    dis, same = np.asarray(dis, np.int64), np.asarray(same, np.int64)
    b = s.shape[0]
    step = ns - s
    length = np.sqrt((step * step).sum(1))
    terms = np.zeros(4)
    g_step, g_s = np.zeros_like(s), np.zeros_like(s)
    terms[0] = (length ** 2).mean()
    g_step += weights[0] * 2.0 * step / b
    i, j = dis[:, 0], dis[:, 1]
    gap = s[i] - s[j]
    sim = np.exp(-(gap * gap).sum(1))
    terms[1] = sim.mean()
    pull = (weights[1] * -2.0 * sim / len(dis))[:, None] * gap
    np.add.at(g_s, i, pull)
    np.add.at(g_s, j, -pull)
    i, j = same[:, 0], same[:, 1]
    gap, sgap = s[i] - s[j], step[i] - step[j]
    sim, far = np.exp(-(gap * gap).sum(1)), (sgap * sgap).sum(1)
    dl = length[i] - length[j]
    terms[2] = (dl ** 2).mean()
    terms[3] = (sim * far).mean()
    safe = np.where(length > 0, length, 1.0)
    unit = np.where((length > 0)[:, None], step / safe[:, None], 0.0)
    w = (weights[2] * 2.0 * dl / len(same))[:, None]
    np.add.at(g_step, i, w * unit[i])
    np.add.at(g_step, j, -w * unit[j])
    w = (weights[3] * 2.0 * sim / len(same))[:, None] * sgap
    np.add.at(g_step, i, w)
    np.add.at(g_step, j, -w)
    pull = (weights[3] * -2.0 * sim * far / len(same))[:, None] * gap
    np.add.at(g_s, i, pull)
    np.add.at(g_s, j, -pull)
    return terms, g_s - g_step, g_step


def incidence_by_hand(pairs, batch):
    """The incidence table written as loops: offsets [batch + 1], then for every row its partners in pair order."""
    rows = [[] for _ in range(batch)]
    for i, j in pairs:
        rows[i].append(j)
        rows[j].append(i)
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    return np.concatenate((offsets, [q for r in rows for q in r])).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the fit
# whole fits of the first recording (no minibatch depends on the over-sampling): D features, state_dim S
FIT_CASES = (
    dict(name="plain_raw", rec=0, D=12, S=3, epochs=5, lr=0.005, seed=0, val_size=0.2, standardize=False, scale=1.0, shift=0.0),
    dict(name="plain_standardized", rec=0, D=12, S=3, epochs=5, lr=0.005, seed=0, val_size=0.2, standardize=True, scale=50.0, shift=20.0),
)


def fit_features(case):
    """float32 [N, D]: a smooth random walk per episode plus noise, times scale, plus shift."""
    rec = RECORDINGS[case["rec"]]
    rs = np.random.RandomState(1000 + case["seed"])
    n, d = rec["N"], case["D"]
    walk = np.cumsum(0.3 * rs.randn(n, d), axis=0)
    per = n // rec["E"]
    for e in range(rec["E"]):
        walk[e * per:(e + 1) * per] -= walk[e * per]
    return ((walk + 0.1 * rs.randn(n, d)) * case["scale"] + case["shift"]).astype(np.float32)


def fit_tables(rec, seed, val_size, epochs):
    """The tables of a fit, from ONE np.random.RandomState(seed): the learner's cut (the stream of np.random.seed(seed) +
    np.random.shuffle), then the validation minibatch ids (the head of a permutation), then per epoch a permutation of the
    training ids.  -> (minibatches, val_ids, orders)."""
    _, _, starts = recording(rec)
    b = rec["B"]
    rs = np.random.RandomState(seed)
    indices = np.array([i for i in range(rec["N"] - 1) if not starts[i + 1]], dtype="int64")
    rs.shuffle(indices)
    mlist = [np.array(sorted(indices[s:s + b])) for s in range(0, len(indices) - b + 1, b)]
    n_val = int(np.round(val_size * len(mlist)))
    val_ids = rs.permutation(len(mlist))[:n_val].astype(np.int64)
    train_ids = np.array([k for k in range(len(mlist)) if k not in set(val_ids.tolist())], np.int64)
    orders = [train_ids[rs.permutation(len(train_ids))] for _ in range(epochs)]
    return mlist, val_ids, orders


def standardized(x):
    """float64 (x - mean) / std per feature (population std; a constant feature keeps std 1) -> (z, mean, std)."""
    x = np.asarray(x, np.float64)
    mean, std = x.mean(0), x.std(0)
    std = np.where(std > 0, std, 1.0)
    return (x - mean) / std, mean, std


def map_grad_f64(w, bias, x, rows, dis, same):
    """float64: the four terms of the minibatch `rows` under s = x W^T + b, and the gradient of their sum with respect to
    (W, b), flat in state_dict order."""
    w, bias, x = np.asarray(w, np.float64), np.asarray(bias, np.float64), np.asarray(x, np.float64)
    rows = np.asarray(rows, np.int64)
    s, ns = x[rows].dot(w.T) + bias, x[rows + 1].dot(w.T) + bias
    terms, ds, dns = priors_f64(s, ns, dis, same)
    dw = ds.T.dot(x[rows]) + dns.T.dot(x[rows + 1])
    return terms, np.concatenate((dw.reshape(-1), (ds + dns).sum(0)))


def adam_f64(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step number t (from 1) in float64 -> (p, m, v)."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    step = lr / (1 - b1 ** t)
    return p - step * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps), m, v
