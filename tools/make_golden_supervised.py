#!/usr/bin/env python
"""Generate the supervised baseline's fixtures (tests/golden/*sup*.npz, supervised_spread.json) by running the UNMODIFIED reference
(srl_baselines/supervised.py, models/supervised.py, preprocessing/data_loader.py:283-365) on the CPU with one thread.

The reference is imported, never copied, with the module stubs and the cv2 shim of tools/make_golden.py and the installed sklearn.
One more shim: the reference's loader keeps its ragged target list as np.array(targets), which numpy >= 1.24 refuses; the loader
module sees a numpy whose `array` falls back to dtype=object for exactly that case — what the numpy of the reference's day returned.
Fixtures are DATA: inputs are regenerated from seeds (tests/supervised_util.py), outputs are stored as digests.

    python tools/make_golden_supervised.py            # every fixture
    python tools/make_golden_supervised.py --spread   # tests/golden/supervised_spread.json (after the fixtures)
"""
from __future__ import print_function
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (helpers only: stubs, shims, digests)
from golden_util import tensor_digest, endpoint_errors, load  # noqa: E402
from supervised_util import sup_inputs, best_epoch, STATE_DIM  # noqa: E402

OUT, REF = mg.OUT, mg.REF
LR = 1e-4
SPLIT_SIZES, SPLIT_SEEDS = (3, 10, 52, 78, 101), (0, 1, 7)


def import_reference():
    mg._stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)
    return th


def build(th, model_type, seed=1):
    """The seeded model as SupervisedLearning.__init__ builds it (BaseLearner seeds numpy and torch, then the constructor runs)."""
    from models import DenseNetwork, CustomCNN  # the reference's
    from preprocessing.preprocess import getInputDim
    np.random.seed(seed)
    th.manual_seed(seed)
    return CustomCNN(STATE_DIM) if model_type == "custom_cnn" else DenseNetwork(getInputDim(), STATE_DIM)


def split_case():
    from sklearn.model_selection import train_test_split
    out = {"sizes": np.array(SPLIT_SIZES), "seeds": np.array(SPLIT_SEEDS)}
    for n in SPLIT_SIZES:
        for seed in SPLIT_SEEDS:
            x = np.arange(n).astype(np.int64)
            x_train, x_val, y_train, y_val = train_test_split(x, x.astype(np.float32), test_size=0.33, random_state=seed)
            assert (x_train == y_train).all() and (x_val == y_val).all()
            out["n%d/seed%d/train" % (n, seed)], out["n%d/seed%d/val" % (n, seed)] = x_train, x_val
    return out


def step_case(th, model_type, B, n_steps=1, lr=None, threads=1, final_sd=None):
    """Loop bodies of srl_baselines/supervised.py:97-122 on the reference classes: n_steps training minibatches (inputs seed
    1234 + step; the mlp's dropout draws from th.manual_seed(99 + step)), then, for a trace, one eval-mode validation minibatch
    without gradients (inputs seed 1234 + n_steps)."""
    import torch.nn as nn
    import torch.nn.functional as F
    model = build(th, model_type)
    th.set_num_threads(threads)
    opt = th.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=lr) if lr is not None else None
    criterion = nn.MSELoss()
    out, trace = {}, []
    for step in range(n_steps):
        obs, tgt = sup_inputs(B, 1234 + step)
        obs, tgt = th.from_numpy(obs), th.from_numpy(tgt)
        model.train()
        seen = {}
        hooks = []
        if model_type == "mlp":
            th.manual_seed(99 + step)
            state = th.get_rng_state()
            hooks = [model.fc1.register_forward_hook(lambda _m, _i, o: seen.__setitem__("fc1", o.detach().clone())),
                     model.fc2.register_forward_pre_hook(lambda _m, i: seen.__setitem__("dropped", i[0].detach().clone()))]
        pred = model(obs)
        for h in hooks:
            h.remove()
        if model_type == "mlp":
            # the product redraws the mask as th.empty(B, n_hidden).bernoulli_(1 - p) at the same generator state: it must give the
            # reference's F.dropout output bit for bit
            after = th.get_rng_state()
            th.set_rng_state(state)
            mask = th.empty(B, seen["fc1"].shape[1]).bernoulli_(1 - model.drop_p)
            assert th.equal(th.get_rng_state(), after), "the redraw consumes the generator differently from F.dropout"
            assert th.equal(F.relu(seen["fc1"]) * mask / (1 - model.drop_p), seen["dropped"]), "the redrawn mask is not F.dropout's"
            out["dropout_mask/step%d" % step] = mask.numpy().astype(np.uint8)
        if opt is not None:
            opt.zero_grad()
        loss = criterion(pred, tgt.detach())
        loss.backward()
        trace.append(float(loss.item()))
        if step == 0:
            out["loss/supervised"] = np.array(float(loss.item()))
            for k, v in tensor_digest(pred).items():
                out["states/" + k] = v
            mg.grads_digest(model, out)
            mg.bn_digest(model, out)
        if opt is not None:
            opt.step()
    if opt is not None:
        out["trace/values"] = np.array(trace)
        sd = mg.digest_state_dict(model.state_dict())
        out["final/names"], out["final/sums"], out["final/abss"] = sd["names"], sd["sums"], sd["abss"]
        mg.bn_digest(model, out, prefix="final_bn/")
        model.eval()
        with th.no_grad():
            obs, tgt = sup_inputs(B, 1234 + n_steps)
            pred = model(th.from_numpy(obs))
            out["val/loss"] = np.array(float(criterion(pred, th.from_numpy(tgt)).item()))
            out["val/states"] = pred.double().numpy()
    model.eval()
    with th.no_grad():
        out["eval_states/full"] = model(th.from_numpy(sup_inputs(B, 1234)[0])).double().numpy()
    th.set_num_threads(1)
    if final_sd is not None:  # (the spread measurement wants the end point's tensors themselves)
        final_sd.update(model.state_dict())
    return out


def _ragged_numpy_shim(module):
    """See the module docstring: np.array(ragged list) -> an object array, for the reference loader module only."""
    shim = types.ModuleType("numpy")
    shim.__dict__.update(np.__dict__)

    def array(obj, *a, **k):
        try:
            return np.array(obj, *a, **k)
        except ValueError:
            res = np.empty(len(obj), dtype=object)
            for i, o in enumerate(obj):
                res[i] = o
            return res
    shim.array = array
    module.np = shim


LOOP_CASES = {"loop_sup_cnn": dict(model_type="custom_cnn"), "loop_sup_mlp": dict(model_type="mlp")}


def loop_case(th, model_type, n_epochs=2, bs=8, test_bs=16, seed=3, lr=LR, n_episodes=3, ep_len=26):
    """The UNMODIFIED SupervisedLearning.learn() (srl_baselines/supervised.py:61-152) on the generated dataset of
    tests/dataset_util.py; TEST_BATCH_SIZE lowered so that the validation set (26 frames) ends in a ragged minibatch."""
    import shutil
    import tempfile
    from dataset_util import make_dataset
    mg._install_cv2_shim()
    import preprocessing.data_loader as ref_dl
    _ragged_numpy_shim(ref_dl)
    import srl_baselines.supervised as RS
    from utils import loadData
    tmp = tempfile.mkdtemp(prefix="srlz_sup_")
    cwd = os.getcwd()
    try:
        name = make_dataset(tmp, n_episodes=n_episodes, ep_len=ep_len)[0]
        os.chdir(tmp)
        os.makedirs("logs/run", exist_ok=True)
        RS.DISPLAY_PLOTS, RS.N_EPOCHS, RS.BATCH_SIZE, RS.TEST_BATCH_SIZE = False, n_epochs, bs, test_bs
        training_data, ground_truth, true_states, _ = loadData(name)
        srl = RS.SupervisedLearning(true_states.shape[1], model_type=model_type, seed=seed, log_folder="logs/run", learning_rate=lr,
                                    cuda=False)
        states = srl.learn(true_states, ground_truth['images_path'], training_data['rewards'])
        with np.load("logs/run/loss.npz") as z:
            train, val = np.asarray(z["train"], dtype=np.float64), np.asarray(z["val"], dtype=np.float64)
        out = {"states/full": np.asarray(states, dtype=np.float64), "loss/train": train, "loss/val": val,
               "best_epoch": np.array(best_epoch(val))}
        sd = mg.digest_state_dict(th.load("logs/run/srl_supervised_model.pth"))
        out["final/names"], out["final/sums"], out["final/abss"] = sd["names"], sd["sums"], sd["abss"]
        out["config"] = np.array(json.dumps(dict(model_type=model_type, n_epochs=n_epochs, bs=bs, test_bs=test_bs, seed=seed, lr=lr,
                                                 n_episodes=n_episodes, ep_len=ep_len)))
        return out
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


def run_loop_child(name):
    # a FRESH interpreter per loop: learn() forks its loader processes (see tools/make_golden.py)
    import subprocess
    import tempfile
    tmp = tempfile.mktemp(suffix=".npz")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--loop-child", name, tmp], timeout=1500)
    with np.load(tmp, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    os.remove(tmp)
    return d


def spread():
    """How far the reference's own 3-step trajectory moves under fp32 rounding alone: the trace re-run at 1 and at 8 intra-op threads
    against the (1-thread) fixture, in the metric of tests/golden_util.py::endpoint_errors — as tools/measure_spread.py measures
    trajectory_spread.json for the auto-encoder traces."""
    th = import_reference()
    out = {}
    for case, (mt, B, n_steps) in {"trace_sup_cnn_b2": ("custom_cnn", 2, 3)}.items():
        g = load(case)
        res = []
        for threads in (1, 8):
            sd = {}
            d = step_case(th, mt, B, n_steps=n_steps, lr=LR, threads=threads, final_sd=sd)
            res.append(endpoint_errors(sd, g, LR, n_steps, d["eval_states/full"])[0])
        out[case] = {k: max(r[k] for r in res) for k in res[0]}
        print(case, json.dumps(out[case]))
    with open(os.path.join(OUT, "supervised_spread.json"), "w") as f:
        json.dump({"metric": "tests/golden_util.py::endpoint_errors of the reference run (1 thread, 8 threads) vs the reference "
                             "fixture, max", "cases": out}, f, indent=1, sort_keys=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    th = import_reference()
    only = [a for a in sys.argv[1:] if not a.startswith("-")]

    def save(name, fn):
        if only and not any(name.startswith(o) for o in only):
            return
        d = fn()
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        print("wrote %-28s %6.1f KB  (%d arrays)" % (name + ".npz", os.path.getsize(path) / 1024.0, len(d)))

    save("sup_split", split_case)
    save("init_sup_cnn", lambda: mg.digest_state_dict(build(th, "custom_cnn").state_dict()))
    save("init_sup_mlp", lambda: mg.digest_state_dict(build(th, "mlp").state_dict()))
    save("step_sup_cnn_b3", lambda: step_case(th, "custom_cnn", 3))
    save("step_sup_mlp_b3", lambda: mg.dense_subs(step_case(th, "mlp", 3)))
    save("trace_sup_cnn_b2", lambda: step_case(th, "custom_cnn", 2, n_steps=3, lr=LR))
    for lname in LOOP_CASES:
        save(lname, lambda: run_loop_child(lname))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--loop-child":
        th = import_reference()
        np.savez_compressed(sys.argv[3], **loop_case(th, **LOOP_CASES[sys.argv[2]]))
    elif "--spread" in sys.argv[1:]:
        spread()
    else:
        main()
