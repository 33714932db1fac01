#!/usr/bin/env python
"""What an epoch of the robotic-priors fit costs on one GPU: python tools/kb_robotic.py [--out profiles/kb_robotic.json]

At N = 100 000 frames in episodes of 250, A = 6, state_dim 3, batch sizes 32 and 256 and D in {3, 32, 200} features, on the training
minibatches of srlz.priorsfit.minibatch_list (80 % of the minibatches), the two routes of srlz.priorsfit.fit_priors side by side in
one process:
  * kernel  one srlz_robotic_fit launch: every Adam step of the epoch by one persistent workgroup;
  * torch   srlz.priorsfit._torch_epoch: the same steps over the same tables through autograd and torch.optim.Adam.
Device time per epoch from HIP events around one epoch (tools/kb_horizon.py's timed() with a burst of 1: every repetition times both
sides in turn, a side's own spread is the difference between the medians of its even and odd repetitions).  Both sides start every
epoch from the same parameters and zero moments, so both do the same arithmetic every time.  The baseline is the torch route in the
same run on the same GPU, never the kernel against itself.  Also recorded: the distance between the two routes' weights after one
epoch (not the bias: its gradient is rounding noise) and the host time of the pair mining.
Prints one JSON object and writes it to --out with csrc_sha16, the fingerprint of the kernel sources it was recorded at."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, REPO)

N_FRAMES, EP_LEN, A, S = 100000, 250, 6, 3
FEATURE_DIMS = (3, 32, 200)
BATCH_SIZES = (32, 256)
LR = 0.005


def recording(d):
    rs = np.random.RandomState(d)
    actions = rs.randint(0, A, N_FRAMES)
    rewards = (rs.rand(N_FRAMES) < 0.3).astype(np.int64)
    x = np.cumsum(0.1 * rs.randn(N_FRAMES, d), axis=0).astype(np.float32)
    x = ((x - x.mean(0)) / x.std(0)).astype(np.float32)
    return x, actions, rewards, (np.arange(N_FRAMES) % EP_LEN) == 0


def sides(d, b):
    from srlz import priorsfit as pf, ops
    from losses.utils import priors_pairs
    dev = torch.device("cuda", 0)
    x, actions, rewards, es = recording(d)
    cfg = pf.check_fit_priors(x, actions, rewards, es, S, n_actions=A, epochs=1, batch_size=b, lr=LR, standardize=False)
    mlist, order = cfg["minibatches"], cfg["orders"][0]
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        dis, same = priors_pairs(b, mlist, cfg["actions"], cfg["rewards"], A, np.zeros(A, np.int64))
    mining_ms = (time.perf_counter() - t0) * 1e3
    xd = torch.from_numpy(x).to(dev)
    init = torch.from_numpy(np.concatenate((cfg["weight"].reshape(-1), cfg["bias"]))).to(dev)
    tabs, k_order = ops.robotic_fit_tables(np.stack(mlist), dis, same, dev), ops.robotic_order(order, dev)
    t_tables = pf._torch_tables(mlist, dis, same, dev)
    params, m, v = init.clone(), torch.zeros_like(init), torch.zeros_like(init)
    running, t_running = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
    w = init[:S * d].view(S, d).clone().requires_grad_(True)
    bias = init[S * d:].clone().requires_grad_(True)

    def kernel_side():
        params.copy_(init)
        m.zero_()
        v.zero_()
        ops.robotic_fit(xd, tabs, k_order, params, m, v, 0, LR, running)

    def torch_side():
        with torch.no_grad():
            w.copy_(init[:S * d].view(S, d))
            bias.copy_(init[S * d:])
        opt = torch.optim.Adam([w, bias], lr=LR)  # (fresh moments; its construction is host work outside the kernels' time)
        pf._torch_epoch(xd, w, bias, opt, t_tables, order, t_running)

    info = {"feature_dim": d, "state_dim": S, "n_actions": A, "batch_size": b, "n_frames": N_FRAMES, "minibatches": len(mlist),
            "steps_per_epoch": int(len(order)), "pairs_per_minibatch": float(np.mean([len(p) for p in same]) + np.mean([len(p) for p in dis])),
            "pair_mining_host_ms": mining_ms, "n_params": ops.robotic_n_params(d, S)}

    def agreement():
        kernel_side()
        torch_side()
        torch.cuda.synchronize()
        return float((params[:S * d] - w.detach().reshape(-1)).abs().max() / w.detach().abs().max())
    return {"kernel": kernel_side, "torch": torch_side}, agreement, info, (xd, tabs, t_tables)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_robotic.json"))
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_robotic measures on a GPU"
    import bench
    from kb_horizon import timed
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup, "burst": 1,
           "lr": LR, "shapes": []}
    for d in FEATURE_DIMS:
        for b in BATCH_SIZES:
            launches, agreement, rec, keep = sides(d, b)
            rec["weight_rel_diff_after_one_epoch"] = agreement()
            rec.update(timed(launches, args.reps, args.warmup, 1))
            rec["torch_over_kernel"] = rec["torch_us"] / rec["kernel_us"]
            rec["kernel_us_per_step"] = rec["kernel_us"] / rec["steps_per_epoch"]
            rec["torch_us_per_step"] = rec["torch_us"] / rec["steps_per_epoch"]
            res["shapes"].append(rec)
            print(json.dumps(rec), flush=True)
            del launches, agreement, keep
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
