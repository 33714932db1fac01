#!/usr/bin/env python
"""Generate the PCA baseline's fixtures (tests/golden/pca_kats.npz, loop_pca.npz, pca_spread.json) from the UNMODIFIED reference
(srl_baselines/pca.py) and the installed sklearn (IncrementalPCA), on the CPU.

The reference and sklearn are imported, never copied, with the module stubs and the cv2 shim of tools/make_golden.py; the reference's
plotting module is stubbed as well (nothing is drawn).  Fixtures are DATA: uint8 frames, and what sklearn computed from them.

    python tools/make_golden_pca.py            # the three files

pca_kats.npz — per case (N, C, W, H, bs, k): the planar uint8 frames and, after EVERY minibatch of IncrementalPCA.partial_fit on
    the normalised float32 frames: singular values, explained variance and ratio, noise variance, n_samples_seen, and the columns
    cols = 0, s, 2 s, ... (at most 64) of components_, mean_ and var_; after the last minibatch components_ (as float32) and mean_ in full, and the
    states transform() gives all frames.  (The column subsample keeps the file small; every minibatch builds on the whole previous basis, so
    the full arrays of the last one pin the rest.)
loop_pca.npz — the reference's srl_baselines/pca.py run as a script (runpy) on the tests/dataset_util.make_dataset dataset, 72 frames of
    224 x 224, --state-dim 3, default batch size: the states it saved and the fields of its pca.pkl (the three large ones as digests).
pca_spread.json — per case, how far sklearn's float32 run lies from its own float64 run on the same frames: max |states32 - states64|
    and max |components32 - components64| over the quantity's scale.  A case whose spread exceeds 1e-5 has a spectrum too degenerate
    to pin anything and is refused: change its seed or k.
"""
from __future__ import print_function
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (helpers only: stubs, shims)
from golden_util import tensor_digest  # noqa: E402
from pca_util import CASES, case_name, column_subsample, minibatches  # noqa: E402

OUT, REF = mg.OUT, mg.REF
MAX_SPREAD = 1e-5
PER_BATCH = ("singular_values_", "explained_variance_", "explained_variance_ratio_", "noise_variance_", "n_samples_seen_")
LARGE = ("components_", "mean_", "var_")


def import_reference():
    mg._stub_modules()
    plot = types.ModuleType("plotting.representation_plot")
    plot.INTERACTIVE_PLOT = False
    plot.plotRepresentation = plot.plotImage = lambda *a, **k: None
    plot.plt = types.ModuleType("matplotlib.pyplot")  # (imported by the reference's models/learner.py, never called here)
    pkg = types.ModuleType("plotting")
    pkg.representation_plot = plot
    sys.modules["plotting"], sys.modules["plotting.representation_plot"] = pkg, plot
    sys.path.insert(0, REF)


def reference_lut():
    """[3, 256] float32: the reference's preprocessInput (preprocessing/utils.py:20-32) of the byte values."""
    from preprocessing.utils import preprocessInput
    x = np.repeat(np.arange(256, dtype=np.float32)[:, None, None], 3, axis=2)
    return np.ascontiguousarray(preprocessInput(x)[:, 0, :].T)


def make_frames(N, C, W, H, k, seed):
    """A seeded low-rank signal of rank k + 4 with decaying weights plus noise, quantised to uint8 [N, C, W, H]."""
    rs = np.random.RandomState(seed)
    D, rank = C * W * H, k + 4
    base = rs.randn(rank, D)
    coef = rs.randn(N, rank) * (40.0 * 0.85 ** np.arange(rank))
    x = 128 + coef.dot(base) + 2.0 * rs.randn(N, D)
    return np.clip(np.rint(x), 0, 255).astype(np.uint8).reshape(N, C, W, H)


def normalised(frames, lut):
    """What the reference's loader hands toNumpyMatrix (srl_baselines/pca.py:47-54): float32 [N, C * W * H]."""
    N, C = frames.shape[:2]
    return np.stack([lut[c % 3][frames[:, c]] for c in range(C)], axis=1).reshape(N, -1).astype(np.float32)


def kat_case(case, lut, spread):
    from sklearn.decomposition import IncrementalPCA
    N, C, W, H, bs, k = case
    name = case_name(case)
    frames = make_frames(N, C, W, H, k, seed=sum(case))
    X = normalised(frames, lut)
    cols = column_subsample(X.shape[1])
    p32, p64 = IncrementalPCA(n_components=k), IncrementalPCA(n_components=k)
    out = {name + "/frames": frames, name + "/cols": cols}
    batches = [b for b in minibatches(N, bs) if len(b)]  # (sklearn raises on the empty trailing range)
    for i, b in enumerate(batches):
        p32.partial_fit(X[b].copy())
        p64.partial_fit(X[b].astype(np.float64))
        for f in PER_BATCH:
            out["%s/batch%d/%s" % (name, i, f)] = np.asarray(getattr(p32, f))
        out["%s/batch%d/components_" % (name, i)] = p32.components_[:, cols]
        out["%s/batch%d/mean_" % (name, i)] = p32.mean_[cols]
        out["%s/batch%d/var_" % (name, i)] = p32.var_[cols]
    # (sklearn's arrays are float64 from the second minibatch on — np.vstack with the float64 correction row; the one large array is
    # stored rounded to float32, 6e-8 of its scale, to keep the file below the largest existing fixture)
    out[name + "/final/components_"] = p32.components_.astype(np.float32)
    out[name + "/final/mean_"] = p32.mean_
    s32, s64 = p32.transform(X), p64.transform(X.astype(np.float64))
    out[name + "/final/states"] = s32
    out[name + "/n_batches"] = np.array(len(batches))
    out[name + "/dtypes"] = np.array(json.dumps({f: str(np.asarray(getattr(p32, f)).dtype) for f in PER_BATCH + LARGE}))
    spread[name] = {"states": float(np.abs(s32 - s64).max() / np.abs(s64).max()),
                    "components": float(np.abs(p32.components_ - p64.components_).max() / np.abs(p64.components_).max())}
    print(name, "singular values", np.round(p64.singular_values_, 1), json.dumps(spread[name]))
    worst = max(spread[name].values())
    if worst > MAX_SPREAD:
        raise SystemExit("%s: sklearn float32 vs float64 differ by %.2e > %.0e: the kept spectrum is too degenerate to pin anything; "
                         "change the seed or k" % (name, worst, MAX_SPREAD))
    return out


def loop_case(n_episodes=3, ep_len=24, state_dim=3):
    """srl_baselines/pca.py of the reference as a script, in a scratch working directory that holds the generated dataset."""
    import pickle
    import runpy
    import shutil
    import tempfile
    from dataset_util import make_dataset
    import_reference()
    mg._install_cv2_shim()
    import torch as th
    th.set_num_threads(1)
    tmp = tempfile.mkdtemp(prefix="srlz_pca_")
    cwd, argv = os.getcwd(), sys.argv
    try:
        name = make_dataset(tmp, n_episodes=n_episodes, ep_len=ep_len)[0]
        os.chdir(tmp)
        sys.argv = ["pca.py", "--data-folder", name, "--state-dim", str(state_dim), "--no-display-plots"]
        runpy.run_module("srl_baselines.pca", run_name="__main__")
        log = "logs/%s/baselines/pca_ST_DIM%d" % (name, state_dim)
        with open(log + "/pca.pkl", "rb") as f:
            ipca = pickle.load(f)
        out = {"states": np.load(log + "/states_rewards.npz")["states"],
               "files": np.array(sorted(os.listdir(log))),
               "config": np.array(json.dumps(dict(n_episodes=n_episodes, ep_len=ep_len, state_dim=state_dim, log_folder=log))),
               "exp_config": np.array(open(log + "/exp_config.json").read())}
        for f in PER_BATCH + ("n_components_",):
            out["pkl/" + f] = np.asarray(getattr(ipca, f))
        for f in LARGE:
            for key, v in tensor_digest(getattr(ipca, f)).items():
                out["pkl/%s/%s" % (f, key)] = v
        return out
    finally:
        sys.argv = argv
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


def save(name, d):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print("wrote %-20s %6.1f KB  (%d arrays)" % (name + ".npz", os.path.getsize(path) / 1024.0, len(d)))


def main():
    os.makedirs(OUT, exist_ok=True)
    import subprocess
    import tempfile
    import_reference()
    lut, spread, kats = reference_lut(), {}, {}
    for case in CASES:
        kats.update(kat_case(case, lut, spread))
    kats["lut"] = lut
    save("pca_kats", kats)
    with open(os.path.join(OUT, "pca_spread.json"), "w") as f:
        json.dump({"metric": "max |sklearn float32 - sklearn float64| over max |float64|, IncrementalPCA on the frames of pca_kats.npz",
                   "refused_above": MAX_SPREAD, "cases": spread}, f, indent=1, sort_keys=True)
    # the whole script in a FRESH interpreter: its loader forks (see tools/make_golden.py)
    tmp = tempfile.mktemp(suffix=".npz")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--loop-child", tmp], timeout=1500)
    with np.load(tmp, allow_pickle=False) as z:
        save("loop_pca", {k: z[k] for k in z.files})
    os.remove(tmp)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--loop-child":
        np.savez_compressed(sys.argv[2], **loop_case())
    else:
        main()
