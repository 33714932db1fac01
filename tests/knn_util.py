"""Shared by the evaluation tests and tools/make_golden_eval.py: the numpy oracle of the exact k-nearest-neighbour search, the seeded
inputs of the kernel tests and the generated datasets behind tests/golden/knn_kats.npz (the fixture records results only; inputs are
regenerated here from the seeds it names)."""
import json
import os

import numpy as np

# (N, D) of the seeded inputs: RandomState(0).randn(N, D).astype(float32).  Minimum relative gap between the 7 smallest fp64
# distances of any row: 4.2e-5, 1.7e-6, 8.0e-7, 2.6e-5, 1.7e-5 — seven orders of magnitude above fp64 rounding; the gap at
# (1031, 200) is about fp32 rounding at D = 200, so a search that ranks in fp32 fails there.
SEEDED_SHAPES = [(257, 3), (1000, 2), (1031, 200), (2049, 7), (300, 65)]


def seeded_input(n, d, seed=0):
    return np.random.RandomState(seed).randn(n, d).astype(np.float32)


def brute_knn(db, queries, k, block=64):
    """(idx int64 [Q, k], dist2 float64 [Q, k]): fp64, differences form, every pair's sum one chain over d = 0 .. D-1, then a STABLE
    sort on dist2 — i.e. ascending (dist2, index), equal distances to the lower index."""
    db = np.asarray(db, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.float64)
    nq, dim = queries.shape
    idx = np.empty((nq, k), dtype=np.int64)
    dist2 = np.empty((nq, k), dtype=np.float64)
    dbt = np.ascontiguousarray(db.T)
    for q0 in range(0, nq, block):
        q = queries[q0:q0 + block]
        acc = np.zeros((q.shape[0], db.shape[0]), dtype=np.float64)
        for d in range(dim):
            t = q[:, d, None] - dbt[d][None, :]
            acc += t * t
        order = np.argsort(acc, axis=1, kind="stable")[:, :k]
        idx[q0:q0 + block] = order
        dist2[q0:q0 + block] = np.take_along_axis(acc, order, axis=1)
    return idx, dist2


def relative_gaps(dist2_sorted):
    """(d[j+1] - d[j]) / d[j+1] along the last axis (0 where both are 0)."""
    a, b = dist2_sorted[..., :-1], dist2_sorted[..., 1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(b > 0, (b - a) / b, 0.0)
    return g


# ---- the generated evaluation datasets of tests/golden/knn_kats.npz ---------------------------------------------------------
EPISODE_LEN = 50


def eval_dataset(n, d, kind="plain"):
    """The dataset of a fixture case, regenerated from its descriptor.
    kind 'plain':        learned states = seeded_input(n, d); ground truth RandomState(1).rand(n, 3) (float64)
    kind 'ground-truth': the search runs on the ground truth itself: RandomState(2).randn(n, d) float64 (not representable in float32)
    kind 'relative-pos': as 'plain' with per-episode target positions RandomState(3).rand(episodes, 3) to subtract
    :return: dict(states float32 [n, d] or None, true_states float64, images_path, episode_starts, target_positions)"""
    episodes = (n + EPISODE_LEN - 1) // EPISODE_LEN
    images_path = np.array(["knn_kats/record_%03d/frame%06d" % (i // EPISODE_LEN, i % EPISODE_LEN) for i in range(n)])
    episode_starts = np.array([i % EPISODE_LEN == 0 for i in range(n)])
    target_positions = np.random.RandomState(3).rand(episodes, 3)
    if kind == "ground-truth":
        true_states = np.random.RandomState(2).randn(n, d)
        states = None
    else:
        true_states = np.random.RandomState(1).rand(n, 3)
        states = seeded_input(n, d)
    return dict(states=states, true_states=true_states, images_path=images_path, episode_starts=episode_starts,
                target_positions=target_positions)


def write_eval_dataset(root, ds, log_folder="logs/knn_kats/run", name="knn_kats"):
    """data/<name>/{ground_truth,preprocessed_data}.npz, dataset_config.json and <log_folder>/{exp_config.json,states_rewards.npz}
    under `root`.  :return: the log folder (relative to root)"""
    folder = os.path.join(root, "data", name)
    os.makedirs(folder, exist_ok=True)
    os.makedirs(os.path.join(root, log_folder), exist_ok=True)
    n = len(ds["images_path"])
    np.savez(os.path.join(folder, "ground_truth.npz"), images_path=ds["images_path"], ground_truth_states=ds["true_states"],
             target_positions=ds["target_positions"])
    np.savez(os.path.join(folder, "preprocessed_data.npz"), actions=np.zeros(n, dtype=np.int64), rewards=np.zeros(n),
             episode_starts=ds["episode_starts"])
    with open(os.path.join(folder, "dataset_config.json"), "w") as f:
        json.dump({"relative_pos": False}, f)
    with open(os.path.join(root, log_folder, "exp_config.json"), "w") as f:
        json.dump({"data-folder": name}, f)
    if ds["states"] is not None:
        np.savez(os.path.join(root, log_folder, "states_rewards.npz"), states=ds["states"], rewards=np.zeros(n))
    return log_folder


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_kats.npz")


def load_golden():
    """:return: (npz, [case descriptor dicts: name, n, d, kind, k, n_samples, seed])"""
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"]))
