"""Shared by the goal-distance tests and tools/make_golden_goal.py: the fixture's constants and the scoring rule of include/srlz.h
restated in numpy at any precision, independently of srlz.deploy.goal_scores.  Nothing here touches a GPU or reads a file."""
import numpy as np

KSTAR = 2        # the plan whose final state (the reference's own, fp64) is each environment's goal
GAMMA = 0.9
WEIGHT = 0.5
MODES = ("running", "final")
SCORE_KEYS = tuple("%s_%s" % (m, h) for m in MODES for h in ("head", "nohead"))
ACT_WEIGHT = 1.0  # act() rolls with gamma = 1; the fixture records k*'s margin under this weight, final mode, with the head


def case_inputs(name):
    """States and plans of a fixture case: dynamics_util.case_inputs' states, and its plans moved by k (t + 1)^2 + (k // 2) t
    (mod A).  The plans of dynamics_util repeat — in environment 0 plan k + 2 IS plan k — so no k* could be the unique argmin of
    anything there.  The first term sets plan k* apart from step 0 on: the first action is the one an expanding recurrence amplifies
    most, so plans alike there end alike.  The second makes every environment's plans pairwise different (with the first alone plans 0
    and 3 of environment 1 coincide).  tools/make_golden_goal.py checks the margin this buys."""
    import dynamics_util as dy
    z, pl = dy.case_inputs(name)
    k, t = np.meshgrid(np.arange(pl.shape[1]), np.arange(pl.shape[2]), indexing="ij")
    return z, ((pl + (k * (t + 1) * (t + 1) + (k // 2) * t)[None]) % dy.N_ACTIONS).astype(np.int32)


def goals_of(trajectory64, kstar=KSTAR):
    """fp32 [N,S]: the state plan k* reaches at the last step."""
    return np.asarray(trajectory64)[:, kstar, -1].astype(np.float32)


def dist(trajectory, goal, dtype):
    """[N,K,T] at `dtype`: sum_j (s_{t+1}[j] - goal[j])^2; goal [S] or [N,S]."""
    tr, g = np.asarray(trajectory).astype(dtype), np.asarray(goal).astype(dtype)
    g = g.reshape(1, 1, 1, -1) if g.ndim == 1 else g[:, None, None, :]
    e = tr - g
    return (e * e).sum(axis=-1, dtype=dtype)


def probs(logits, dtype):
    """[N,K,T] at `dtype`: softmax(l)[1] = 1 / (1 + exp(l0 - l1))."""
    lg = np.asarray(logits).astype(dtype)
    with np.errstate(over="ignore"):  # (exp overflows to inf for a hopeless row: the probability is then 0, as in the kernel)
        return (1 / (1 + np.exp(lg[..., 0] - lg[..., 1]))).astype(dtype)


def scores(d, p, gamma, weight, mode, dtype):
    """[N,K] at `dtype`: ret = ret + g * term_t, g_0 = 1, g *= gamma, each operation rounded at `dtype` (for float32: the kernel's own
    order and roundings); term_t = p_t - w c_t, or -(w c_t) for p = None; gamma and weight as the float32 the kernel takes."""
    d = np.asarray(d).astype(dtype)
    t = d.shape[-1]
    ty = np.dtype(dtype).type
    w, gam, g = ty(np.float32(weight)), ty(np.float32(gamma)), ty(1)
    ret = np.zeros(d.shape[:-1], dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for step in range(t):
            c = d[..., step] if (mode == "running" or step == t - 1) else np.zeros(d.shape[:-1], dtype)
            wc = (w * c).astype(dtype)
            term = -wc if p is None else (np.asarray(p[..., step]).astype(dtype) - wc).astype(dtype)
            ret = (ret + (g * term).astype(dtype)).astype(dtype)
            g = ty(g * gam)
    return ret


def all_scores(d, p, dtype, gamma=GAMMA, weight=WEIGHT):
    """{key of SCORE_KEYS: [N,K]} — both modes, with the head's probabilities and without."""
    return {"%s_%s" % (m, h): scores(d, p if h == "head" else None, gamma, weight, m, dtype) for m in MODES for h in ("head", "nohead")}


def dist_bound_terms(s):
    """The relative bound of test 2: one rounding for the difference (twice in the square), one for the square, S - 1 for the sum."""
    return (s + 4) * 2.0 ** -24


# ---- an integer world: every quantity of the goal term is exact in fp32, so kernel, host planner and restatement agree bit for bit ----
# S = 2, A = 4: Wf[:, :S] = 0, bf = 0, the action columns +e_x, -e_x, +e_y, -e_y; from (0, 0) the goal (4, 0) is reached in T = 4 steps by
# the all-(+x) plan alone: distances 9, 4, 1, 0 — score -(9 + 4 + 1 + 0) = -14 in running mode, 0 in final mode (gamma = 1, w = 1, no head).
WORLD_MOVES = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], np.float32)
WORLD_GOAL = np.array([4, 0], np.float32)
# K, iterations, elites, sharpness and seed chosen on the CPU (tests/test_goal_host_cpu.py) so that cem_host finds the plan in both modes
WORLD = dict(s=2, a=4, t=4, k=64, iterations=6, elites=8, q=8, seed=1)


def world_heads():
    """(wf [2,6], bf [2]) fp32 of the integer world."""
    wf = np.zeros((2, 6), np.float32)
    wf[:, 2:] = WORLD_MOVES.T
    return wf, np.zeros(2, np.float32)


def world_trajectory(plans, start=None):
    """fp32 [N,K,T,2]: the states the plans int [N,K,T] walk through from `start` [N,2] (the origin)."""
    tr = np.cumsum(WORLD_MOVES[np.asarray(plans)], axis=2, dtype=np.float32)
    return tr if start is None else tr + np.asarray(start, np.float32)[:, None, None, :]


def world_scores(plans, mode, gamma=1.0, weight=1.0):
    """fp32 [N,K]: the goal-only score of the integer world's plans (exact)."""
    return scores(dist(world_trajectory(plans), WORLD_GOAL, np.float32), None, gamma, weight, mode, np.float32)
