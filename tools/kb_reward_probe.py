#!/usr/bin/env python
"""Wall time of the reward probe's training run on one GPU: python tools/kb_reward_probe.py [--out profiles/kb_reward_probe.json]

The run of evaluation/predict_reward.py at its defaults on a generated dataset: N frames in episodes of 250, states of dimension S,
-bs 32, 10 epochs, 20 % of the samples trained on, 80 % validated on.  Three loops over the SAME split and the same kind of
DataLoader objects, alternated --reps times after one warm-up run each, host clock around a run that ends in a device synchronise:
  * `hip`            the product's loop: one minibatch table per phase, srlz.ops.reward_probe_fit / reward_probe_eval, two launches
                     per epoch;
  * `torch_as_fed`   the reference's loop on stock torch-ROCm operators, fed as the reference feeds it: every minibatch gathered
                     from the host array and uploaded, nn.Sequential forward, CrossEntropyLoss, backward, Adam, the five statistics
                     with their .item() reads;
  * `torch_resident` the same with the states and labels resident on the device (index_select there): the stock stack at its best.
Also recorded: the part of `hip` that is host work (building the tables from the DataLoader), the device time of the two launches
(HIP events), launches per epoch — counted calls for `hip`, torch.profiler's device-kernel count over 20 train and 20 val
minibatches for the stock loop — and the final train loss of each loop (they must agree to float32 noise: same order, same init).
Prints one JSON object and writes it to --out.  For the record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import TensorDataset, DataLoader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))


def dataset(n, s, seed=0):
    rs = np.random.RandomState(seed)
    w = rs.randn(s)
    states = rs.randn(n, s).astype(np.float32)
    labels = ((states @ w) / np.sqrt(s) + 0.5 * rs.randn(n) > 0.8).astype(np.int64)  # about one positive in four, learnable
    starts = np.arange(n) % 250 == 0
    indices = np.array([i for i in range(n - 1) if not starts[i + 1]], dtype=np.int64)
    return states, labels, indices


def split(indices, seed):
    from sklearn.model_selection import train_test_split
    x_train, x_val = train_test_split(indices, test_size=0.8, random_state=seed)
    return torch.from_numpy(x_train), torch.from_numpy(x_val)


def loaders(x_train, x_val, bs):
    return {"train": DataLoader(TensorDataset(x_train), batch_size=bs, shuffle=True),
            "val": DataLoader(TensorDataset(x_val), batch_size=bs, shuffle=False)}


def new_model(s, seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(2 * s, 4), nn.ReLU(), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 2))


def run_hip(ops, pr, data, model, ld, sizes, args, timing=None):
    dev = data.states.device
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).float().to(dev)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    steps, losses, launches, host_s = 0, [], 0, 0.0
    for _ in range(args.epochs):
        for phase in ("train", "val"):
            t = time.perf_counter()
            table = pr.phaseTable(ld[phase], args.bs)
            host_s += time.perf_counter() - t
            loss, counts = ops.reward_probe_stats(dev)
            if timing is not None:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
            if phase == "train":
                ops.reward_probe_fit(data, table, params, m, v, steps, args.lr, loss, counts)
                steps += len(table)
            else:
                ops.reward_probe_eval(data, table, params, loss, counts)
            launches += 1
            if timing is not None:
                b.record()
                timing.append((phase, a, b))
            losses.append(loss.item() / sizes[phase])
            counts.cpu()
    torch.cuda.synchronize()
    return {"final_train_loss": losses[-2], "final_val_loss": losses[-1], "launches": launches, "table_building_s": host_s}


def run_torch(states, labels, model, ld, sizes, args, dev, resident, max_batches=None):
    """The reference's loop (its statements in its order) on stock operators."""
    model = model.to(dev)
    criterion = nn.CrossEntropyLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    if resident:
        st_d, lab_d = torch.from_numpy(states).to(dev), torch.from_numpy(labels).to(dev)
    losses = []
    for _ in range(args.epochs):
        for phase in ("train", "val"):
            running_loss, running_corrects = 0.0, 0
            corrects, n_per_class = {0: 0, 1: 0}, {0: 0, 1: 0}
            for k, (idx,) in enumerate(ld[phase]):
                if max_batches is not None and k >= max_batches:
                    break
                if resident:
                    i = idx.to(dev)
                    lab, inputs, next_inputs = lab_d[i], st_d[i], st_d[i + 1]
                else:
                    index = idx.numpy()
                    lab = torch.from_numpy(labels[index]).to(dev)
                    inputs = torch.Tensor(states[idx, :]).float().to(dev)
                    next_inputs = torch.Tensor(states[idx + 1, :]).float().to(dev)
                if len(next_inputs) < args.bs:
                    continue
                optimizer.zero_grad()
                with torch.set_grad_enabled(phase == "train"):
                    outputs = model(torch.cat((inputs, next_inputs), dim=1))
                    _, preds = torch.max(outputs, dim=1)
                    loss = criterion(outputs, lab)
                    if phase == "train":
                        loss.backward()
                        optimizer.step()
                running_loss += loss.item() * inputs.size(0)
                running_corrects += torch.sum(preds == lab)
                for c in range(2):
                    corrects[c] += torch.sum((preds == lab) * (preds == c).byte())
                    n_per_class[c] += torch.sum(lab == c).item()
            losses.append(running_loss / sizes[phase])
            float(running_corrects)
            [float(corrects[c]) for c in range(2)]
    torch.cuda.synchronize()
    return {"final_train_loss": losses[-2], "final_val_loss": losses[-1]}


def count_torch_kernels(states, labels, model, ld, sizes, args, dev):
    """Device kernels of 20 train and of 20 val minibatches of the resident stock loop -> per minibatch."""
    from torch.autograd import DeviceType
    from torch.profiler import profile, ProfilerActivity
    one = argparse.Namespace(**vars(args))
    one.epochs = 1
    out = {}
    for phase in ("train", "val"):
        only = {p: (ld[p] if p == phase else []) for p in ("train", "val")}
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run_torch(states, labels, model, only, sizes, one, dev, resident=True, max_batches=20)
        n = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
        out[phase] = n / 20.0
    return out


def save(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_reward_probe.json"))
    ap.add_argument("-n", type=int, default=50000)
    ap.add_argument("-s", type=int, default=200)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.005)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profiler", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_reward_probe measures on a GPU"
    from srlz import ops
    from evaluation import predict_reward as pr
    dev = torch.device("cuda", 0)
    states, labels, indices = dataset(args.n, args.s)
    x_train, x_val = split(indices, args.seed)
    sizes = {"train": len(x_train), "val": len(x_val)}
    data = ops.reward_probe_data(states, labels)
    res = {"N": args.n, "S": args.s, "bs": args.bs, "epochs": args.epochs, "device": torch.cuda.get_device_name(0),
           "train_steps_per_epoch": sizes["train"] // args.bs, "val_minibatches_per_epoch": sizes["val"] // args.bs,
           "positives": float(labels.mean()), "torch": torch.__version__, "runs": {"hip": [], "torch_as_fed": [], "torch_resident": []}}

    def one(kind, timing=None):
        torch.manual_seed(args.seed)
        ld = loaders(x_train, x_val, args.bs)
        model = new_model(args.s, seed=7)
        torch.manual_seed(args.seed)
        torch.cuda.synchronize()
        t = time.perf_counter()
        if kind == "hip":
            r = run_hip(ops, pr, data, model, ld, sizes, args, timing)
        else:
            r = run_torch(states, labels, model, ld, sizes, args, dev, resident=(kind == "torch_resident"))
        r["wall_s"] = time.perf_counter() - t
        return r

    for kind in res["runs"]:  # warm-up: code objects, allocator, DataLoader machinery
        one(kind)
    for _ in range(args.reps):
        for kind in res["runs"]:
            res["runs"][kind].append(one(kind))
            print(kind, json.dumps(res["runs"][kind][-1]))
    timing = []
    one("hip", timing)
    res["hip_device_ms_per_epoch"] = {p: sum(a.elapsed_time(b) for q, a, b in timing if q == p) / args.epochs for p in ("train", "val")}
    res["hip_launches_per_epoch"] = res["runs"]["hip"][0]["launches"] / args.epochs
    res["wall_s_median"] = {k: float(np.median([r["wall_s"] for r in v])) for k, v in res["runs"].items()}
    save(res, args.out)  # before the profiler pass: the timings stand without it
    if not args.no_profiler:
        try:
            torch.manual_seed(args.seed)
            per = count_torch_kernels(states, labels, new_model(args.s, seed=7), loaders(x_train, x_val, args.bs), sizes, args, dev)
            res["torch_kernels_per_minibatch"] = per
            res["torch_launches_per_epoch"] = per["train"] * res["train_steps_per_epoch"] + per["val"] * res["val_minibatches_per_epoch"]
        except Exception as e:  # the count is a courtesy: the timings above stand without it
            res["torch_kernels_per_minibatch"] = "not measured: %s" % e
    print(json.dumps(res))
    save(res, args.out)


if __name__ == "__main__":
    main()
