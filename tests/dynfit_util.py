"""Shared by the closed-form forward-head tests: the planted recording and numpy's own normal equations."""
import numpy as np

EPISODES, EP_LEN, S, A = 12, 40, 8, 4


def planted_head(s=S, a=A, seed=5):
    """(W* fp64 [s, s+a], b* fp64 [s]): a mild contraction with a little coupling on the state block, a shift per action."""
    rs = np.random.RandomState(seed)
    w = np.concatenate((-0.1 * np.eye(s) + 0.02 * rs.randn(s, s), 0.1 * rs.randn(s, a)), axis=1)
    return w, 0.01 * rs.randn(s)


def planted_states(actions, episode_starts, s=S, a=A, seed=5):
    """fp32 [N, s]: a random state where an episode starts, else s[i+1] = fl32(s[i] + W* z[i] + b*) with z = [s[i] | onehot(a[i])]."""
    w, b = planted_head(s, a, seed)
    rs = np.random.RandomState(seed + 1)
    actions, es = np.asarray(actions).reshape(-1), np.asarray(episode_starts).reshape(-1) != 0
    x = np.zeros((len(actions), s), np.float32)
    for i in range(len(actions)):
        if i == 0 or es[i]:
            x[i] = rs.randn(s).astype(np.float32)
        else:
            z = np.concatenate((x[i - 1].astype(np.float64), np.eye(a)[actions[i - 1]]))
            x[i] = (x[i - 1].astype(np.float64) + w @ z + b).astype(np.float32)
    return x


def planted_recording(seed=5):
    """(states fp32 [480, 8], actions int64 [480], episode_starts bool [480]): 12 episodes of 40 frames."""
    n = EPISODES * EP_LEN
    actions = np.random.RandomState(seed + 2).randint(0, A, n)
    es = (np.arange(n) % EP_LEN) == 0
    return planted_states(actions, es), actions, es


def design(states, actions, starts, n_actions, dtype=np.float64):
    """(Z [M,P], Y [M,S]) of the listed transitions, exactly as include/srlz.h states them."""
    x = np.asarray(states).astype(dtype)
    i = np.asarray(starts, np.int64)
    a = np.asarray(actions)[i]
    onehot = (a[:, None] == np.arange(n_actions)[None, :]).astype(dtype)
    z = np.concatenate((x[i], onehot, np.ones((len(i), 1), dtype)), axis=1)
    return z, x[i + 1] - x[i]
