"""Shared by the ground-truth-correlation (GTC) tests and tools/make_golden_gtc.py: the seeded inputs and the error bound of the kernel
tests, the generated datasets and the generated log tree behind tests/golden/gtc_kats.npz (the fixture records results only; inputs
are regenerated here from the descriptors it names)."""
import csv
import json
import os

import numpy as np

U = 2.0 ** -53  # unit roundoff of fp64


def bound(n):
    """Absolute bound on a coefficient over n rows: three length-n fp64 sums enter it, each with relative error <= n u, plus the
    mean's second-order term and a few roundings for the square roots and divisions: (4 n + 16) u."""
    return (4.0 * n + 16.0) * U


# (N, G, S, states dtype, kind) of the kernel tests.  kind 'plain': gt = randn, states = gt W + randn (so the coefficients spread
# over (-1, 1)); 'offset100': every value 100 + 0.01 randn; 'offset1e4': every value 1e4 + randn — the inputs on which the one-pass
# sum x^2 - (sum x)^2 / N loses eight digits and more.
KERNEL_CASES = [
    (2, 1, 1, "f32", "plain"),          # smallest legal shape
    (7, 2, 3, "f32", "plain"),          # small, odd
    (63, 3, 65, "f32", "plain"),        # crosses a 64-column tile
    (1025, 3, 200, "f32", "plain"),     # one row past a chunk
    (4099, 6, 67, "f64", "plain"),
    (4099, 16, 5, "f64", "plain"),      # G at its limit
    (4099, 3, 5, "f32", "offset100"),
    (4099, 3, 5, "f64", "offset1e4"),
]


def kernel_input(n, g, s, dtype, kind):
    """:return: (gt float64 [n, g], states [n, s] of the case's dtype)"""
    rs = np.random.RandomState(1000 * g + s + n)
    dt = {"f32": np.float32, "f64": np.float64}[dtype]
    if kind == "plain":
        gt = rs.randn(n, g)
        states = (gt.dot(rs.randn(g, s)) + 2.0 * rs.randn(n, s)).astype(dt)
    elif kind == "offset100":
        gt = 100.0 + 0.01 * rs.randn(n, g)
        states = (100.0 + 0.01 * rs.randn(n, s)).astype(dt)
    elif kind == "offset1e4":
        gt = 1e4 + rs.randn(n, g)
        states = (1e4 + rs.randn(n, s)).astype(dt)
    else:
        raise ValueError(kind)
    return gt, states


def reference_rows(gt, states):
    """Rows 0 .. G-1 of numpy's own corrcoef in extended precision, and the column means / variances (ddof 1) beside them.
    :return: (corr longdouble [G, G + S], colstats longdouble [2, G + S])"""
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = np.corrcoef(gt, states, rowvar=0, dtype=np.longdouble)[:gt.shape[1]]
    both = np.concatenate([np.asarray(gt, dtype=np.longdouble), np.asarray(states, dtype=np.longdouble)], axis=1)
    return corr, np.stack([both.mean(0), both.var(0, ddof=1)])


# ---- the generated datasets of tests/golden/gtc_kats.npz --------------------------------------------------------------------
EPISODE_LEN = 50
DATASET = "gtc_kats"


def gtc_dataset(case):
    """The dataset of a fixture case, regenerated from its descriptor: dict(name, n, n_states, s, seed, old_keys, relative_pos).
    Ground truth RandomState(seed).rand(n, 3) float64, one target RandomState(seed).rand(3) per episode of 50 frames, learned states
    float32 = [gt | per-frame target] W + 0.5 randn cut to the first n_states rows (what --training-set-size leaves).
    :return: dict(states, rewards, true_states, target_positions (per episode), episode_starts, images_path)"""
    n, rs = case["n"], np.random.RandomState(case["seed"])
    episodes = (n + EPISODE_LEN - 1) // EPISODE_LEN
    true_states = rs.rand(n, 3)
    target_positions = rs.rand(episodes, 3)
    per_frame = target_positions[np.arange(n) // EPISODE_LEN]
    states = (np.concatenate([true_states, per_frame], 1).dot(rs.randn(6, case["s"])) + 0.5 * rs.randn(n, case["s"])).astype(np.float32)
    return dict(states=states[:case["n_states"]], rewards=np.zeros(case["n_states"]), true_states=true_states,
                target_positions=target_positions, episode_starts=np.array([i % EPISODE_LEN == 0 for i in range(n)]),
                images_path=np.array(["%s/record_%03d/frame%06d" % (DATASET, i // EPISODE_LEN, i % EPISODE_LEN) for i in range(n)]))


def write_gtc_dataset(root, ds, case, log_folder="logs/gtc_kats/run"):
    """data/gtc_kats/{ground_truth,preprocessed_data}.npz, dataset_config.json and <log_folder>/{exp_config.json,states_rewards.npz}
    under `root`.  :return: the log folder (relative to root)"""
    folder = os.path.join(root, "data", DATASET)
    os.makedirs(folder, exist_ok=True)
    os.makedirs(os.path.join(root, log_folder), exist_ok=True)
    n = len(ds["images_path"])
    if case.get("old_keys"):
        np.savez(os.path.join(folder, "ground_truth.npz"), images_path=ds["images_path"], arm_states=ds["true_states"],
                 button_positions=ds["target_positions"])
    else:
        np.savez(os.path.join(folder, "ground_truth.npz"), images_path=ds["images_path"], ground_truth_states=ds["true_states"],
                 target_positions=ds["target_positions"])
    np.savez(os.path.join(folder, "preprocessed_data.npz"), actions=np.zeros(n, dtype=np.int64), rewards=np.zeros(n),
             episode_starts=ds["episode_starts"])
    with open(os.path.join(folder, "dataset_config.json"), "w") as f:
        json.dump({"relative_pos": bool(case.get("relative_pos", False))}, f)
    with open(os.path.join(root, log_folder, "exp_config.json"), "w") as f:
        json.dump({"data-folder": DATASET, "log-folder": log_folder}, f)
    np.savez(os.path.join(root, log_folder, "states_rewards.npz"), states=ds["states"], rewards=ds["rewards"])
    return log_folder


# ---- the generated log tree behind the recorded results table -------------------------------------------------------------------
def write_log_tree(root):
    """logs/gtc_kats/ with two experiments, a folder without exp_config.json, two baselines and a stray file; every experiment that
    has an exp_config.json also has both result files, so that gather_results launches nothing.
    :return: the log dir (absolute)"""
    log_dir = os.path.join(root, "logs", DATASET)

    def put(name, config=None, corr=None, knn=None):
        folder = os.path.join(log_dir, name)
        os.makedirs(folder, exist_ok=True)
        for fname, content in (("exp_config.json", config), ("gt_correlation.json", corr), ("knn_mse.json", knn)):
            if content is not None:
                with open(os.path.join(folder, fname), "w") as f:
                    json.dump(content, f)

    put("18-01-01_10h00_00_custom_cnn_ST_DIM10_autoencoder",
        {"data-folder": DATASET, "training-set-size": -1, "split-dimensions": -1, "state-dim": 10, "seed": 1,
         "losses_weights": {"autoencoder": 1.0}, "losses": ["autoencoder"]},
        {"gt_corr": [0.91, 0.52, 0.33, 0.125, 0.25, 0.0625], "gt_corr_mean": 0.36625}, {"images": ["a/b"], "knn_mse": 0.01234})
    put("18-01-02_11h30_05_custom_cnn_ST_DIM5_forward_inverse",
        {"data-folder": DATASET, "training-set-size": 500, "split-dimensions": {"forward": 2, "inverse": 3}, "state-dim": 5, "seed": 2,
         "losses_weights": {"forward": 1.0, "inverse": 2.0}},
        {"gt_corr": [0.75, 0.5, 0.25], "gt_corr_mean": 0.5}, {"images": [], "knn_mse": 0.5})
    put("no_config", None, {"gt_corr": [0.1, 0.2], "gt_corr_mean": 0.15000000000000002}, None)
    put("baselines/ground_truth", {"data-folder": DATASET, "ground-truth": True, "seed": 1},
        {"gt_corr": [1.0, 1.0, 1.0, 0.3, 0.2, 0.1], "gt_corr_mean": 0.6}, {"images": [], "knn_mse": 0.00021})
    put("baselines/pca_ST_DIM3", {"data-folder": DATASET, "training-set-size": -1, "state-dim": 3, "batch-size": 16},
        {"gt_corr": [0.4, 0.3, 0.2, 0.1, 0.05, 0.025], "gt_corr_mean": 0.17916666666666667}, {"images": [], "knn_mse": 0.2})
    with open(os.path.join(log_dir, "notes.txt"), "w") as f:
        f.write("not an experiment\n")
    return log_dir


def read_csv(path):
    """:return: [[cell, ...], ...] — the header row first"""
    with open(path, newline="") as f:
        return [list(row) for row in csv.reader(f)]


def same_cell(a, b):
    """Numeric cells compare as floats, the rest as strings."""
    try:
        return float(a) == float(b)
    except ValueError:
        return a == b


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtc_kats.npz")


def load_golden():
    """:return: (npz, [case descriptor dicts])"""
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"]))
