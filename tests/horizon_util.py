"""Shared by the horizon-error tests and tools/make_golden_horizon.py: the fixture's recorded sequence from closed formulas (nothing
is stored), valid_steps and the whole metric restated in numpy independently of srlz.deploy, and the comparison helpers.
Nothing here touches a GPU or reads a file."""
import numpy as np

N_FRAMES = 40
HORIZON = 7
N_ACTIONS = 6
EPISODE_STARTS = (0, 1, 3, 12, 25)  # an episode of one frame, one of two, and rows of every length 0 .. 7
GAP = 2e-4      # a (row, step) whose fp64 logit gap |l1 - l0| is below GAP x the logits' scale is left out of the hit comparison
GAP_CAP = 0.05  # at most this share may be left out in the cases the hit count is checked in
HIT_CASES = ("s3_linear", "s8_mlp", "s200")  # s200_expanding: its logits saturate, it is held to the error quantities only
ROW_QUANTITIES = ("err", "base", "logits")
SUM_QUANTITIES = ("sum_err", "sum_base")


def recording(s, n=N_FRAMES):
    """(states fp32 [n,s], actions int32 [n], rewards fp64 [n], episode_starts bool [n]) of the fixture."""
    import dynamics_util as dy
    i = np.arange(n)
    actions = ((3 * i + i // 4) % N_ACTIONS).astype(np.int32)
    rewards = np.where(i % 3 == 0, 1.0, np.where(i % 7 == 3, -1.0, 0.0))
    es = np.zeros(n, bool)
    es[[e for e in EPISODE_STARTS if e < n]] = True
    return dy.sine_states(n, s), actions, rewards, es


def valid_steps(episode_starts, horizon):
    """int32 [N], by the definition, frame by frame: the largest L <= horizon with frames i+1 .. i+L present and none an episode start."""
    es = np.asarray(episode_starts).astype(bool)
    n = len(es)
    out = np.zeros(n, np.int32)
    for i in range(n):
        steps = 0
        while steps < horizon and i + steps + 1 < n and not es[i + steps + 1]:
            steps += 1
        out[i] = steps
    return out


def labels_of(rewards):
    """The learner's labelling: -1 counts as 0."""
    r = np.array(rewards, copy=True)
    r[r < 0] = 0
    return r.astype(np.int64)


def rows_from_trajectory(trajectory, states, starts, lens, dtype):
    """err, base [M,T] at `dtype` (NaN past a row's steps) from imagined states trajectory [M,T,S] and the recorded states."""
    tr, x = np.asarray(trajectory).astype(dtype), np.asarray(states).astype(dtype)
    m, t, _ = tr.shape
    err, base = np.full((m, t), np.nan, dtype), np.full((m, t), np.nan, dtype)
    for r in range(m):
        for step in range(int(lens[r])):
            tg = x[starts[r] + step + 1]
            e, b = tr[r, step] - tg, x[starts[r]] - tg
            err[r, step], base[r, step] = (e * e).sum(dtype=dtype), (b * b).sum(dtype=dtype)
    return err, base


def classes_of(logits):
    """torch's argmax over two classes: 1 where l1 > l0, else (a tie, a NaN) 0."""
    lg = np.asarray(logits)
    with np.errstate(invalid="ignore"):
        return (lg[..., 1] > lg[..., 0]).astype(np.int64)


def totals(err, base, lens, logits=None, labels=None, starts=None):
    """(count int64 [T], sum_err, sum_base fp64 [T], hits int64 [T] | None): the metric's sums, row by row in fp64."""
    err, base = np.asarray(err, np.float64), np.asarray(base, np.float64)
    m, t = err.shape
    count, hits = np.zeros(t, np.int64), np.zeros(t, np.int64)
    se, sb = np.zeros(t), np.zeros(t)
    cls = classes_of(logits) if logits is not None else None
    for r in range(m):
        for step in range(int(lens[r])):
            count[step] += 1
            se[step] += err[r, step]
            sb[step] += base[r, step]
            if cls is not None:
                hits[step] += int(cls[r, step] == labels[starts[r] + step])
    return count, se, sb, (hits if cls is not None else None)


def valid_mask(lens, t):
    return np.arange(t)[None, :] < np.asarray(lens).reshape(-1, 1)


def step_rel_err(got, ref, mask):
    """max over the valid entries of |got - ref| over the step's scale (max |ref| of that step's valid entries)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    while mask.ndim < ref.ndim:
        mask = mask[..., None]
    mask = np.broadcast_to(mask, ref.shape)
    worst = 0.0
    for step in range(ref.shape[1]):
        mk = mask[:, step]
        if not mk.any():
            continue
        scale = max(np.abs(ref[:, step][mk]).max(), 1e-30)
        worst = max(worst, float((np.abs(got[:, step][mk] - ref[:, step][mk]) / scale).max()))
    return worst


def vec_rel_err(got, ref):
    """max |got - ref| over max |ref| of a per-horizon vector."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def decided(logits64, mask):
    """bool [M,T]: the valid entries whose fp64 logit gap is at least GAP x the logits' scale — where a hit cannot turn on rounding."""
    lg = np.asarray(logits64, np.float64)
    scale = max(np.abs(lg[mask]).max(), 1e-30) if mask.any() else 1.0
    return mask & (np.abs(lg[..., 1] - lg[..., 0]) >= GAP * scale)
