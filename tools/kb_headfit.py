#!/usr/bin/env python
"""What an epoch of the reward head's fit costs on one GPU: python tools/kb_headfit.py [--out profiles/kb_headfit.json]

At N = 100 000 frames in episodes of 250, H = 16, batch sizes 32 and 256 and S in {3, 32, 200}, on the training transitions of
srlz.dynfit.split_episodes (80 % of the episodes), the two routes of srlz.headfit.fit_reward side by side in one process:
  * kernel  one srlz_headfit_fit launch: every Adam step of the epoch by one persistent workgroup;
  * torch   srlz.headfit._torch_epoch: the same steps over the same uploaded table through autograd and torch.optim.Adam.
Device time per epoch from HIP events around one epoch (tools/kb_horizon.py's timed() with a burst of 1: every repetition times both
sides in turn, a side's own spread is the difference between the medians of its even and odd repetitions).  Both sides start every
epoch from the same parameters and zero moments, so both do the same arithmetic every time.  The baseline is the torch route in the
same run on the same GPU, never the kernel against itself.  Then the wall time of a whole default fit_reward (30 epochs, batch size
32: upload, 30 fit and eval launches, the statistics read once) per route — the torch route's at --whole-torch-dims only, it takes
minutes — and the distance between the two routes' parameters after one epoch.
Prints one JSON object and writes it to --out with csrc_sha16, the fingerprint of the kernel sources it was recorded at."""
import argparse
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

N_FRAMES, EP_LEN, H = 100000, 250, 16
STATE_DIMS = (3, 32, 200)
BATCH_SIZES = (32, 256)
LR = 0.005


def recording(s):
    rs = np.random.RandomState(s)
    x = rs.randn(N_FRAMES, s).astype(np.float32)
    rewards = (rs.rand(N_FRAMES) > 0.8).astype(np.float64)
    x[1:, 0] += 0.5 * rewards[:-1].astype(np.float32)  # the reward of a transition shows in its next state
    return x, rewards, (np.arange(N_FRAMES) % EP_LEN) == 0


def sides(s, b):
    from srlz import headfit, ops
    dev = torch.device("cuda", 0)
    x, rewards, es = recording(s)
    cfg = headfit.check_fit_reward(x, rewards, es, hidden=H, epochs=1, batch_size=b, lr=LR)
    table = headfit.minibatch_tables(cfg["train"], 1, b, 0)[0]
    data = ops.RewardProbeData(torch.from_numpy(x).to(dev), torch.from_numpy(cfg["labels"]).to(dev))
    init = torch.from_numpy(cfg["init"]).to(dev)
    k_table, t_table = ops.headfit_table(data, torch.from_numpy(table)), torch.from_numpy(table).to(dev)
    params, m, v = init.clone(), torch.zeros_like(init), torch.zeros_like(init)
    loss, counts = ops.reward_probe_stats(dev)
    leaves = [t.clone().requires_grad_(True) for t in headfit._split_flat(init, s, H)]
    t_loss, t_counts = ops.reward_probe_stats(dev)

    def kernel_side():
        params.copy_(init)
        m.zero_()
        v.zero_()
        ops.headfit_fit(data, k_table, H, params, m, v, 0, LR, loss, counts)

    def torch_side():
        with torch.no_grad():
            for leaf, src in zip(leaves, headfit._split_flat(init, s, H)):
                leaf.copy_(src)
        opt = torch.optim.Adam(leaves, lr=LR)  # (fresh moments; its construction is host work outside the kernels' time)
        headfit._torch_epoch(data, t_table, leaves, opt, t_loss, t_counts)

    def whole(route, reps):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            headfit.fit_reward(x, rewards, es, route=route)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3
    info = {"state_dim": s, "hidden": H, "batch_size": b, "n_frames": N_FRAMES, "transitions": int(cfg["train"].size),
            "steps_per_epoch": int(table.shape[0]), "chunk_rows": ops.headfit_chunk_rows(s, H), "n_params": ops.headfit_n_params(s, H)}

    def agreement():
        kernel_side()
        torch_side()
        torch.cuda.synchronize()
        flat = torch.cat([t.detach().reshape(-1) for t in leaves])
        return float((params - flat).abs().max() / flat.abs().max())
    return {"kernel": kernel_side, "torch": torch_side}, agreement, whole, info, (data, k_table, t_table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_headfit.json"))
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--whole-torch-dims", type=int, nargs="*", default=[32])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_headfit measures on a GPU"
    import bench
    from kb_horizon import timed
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup, "burst": 1,
           "lr": LR, "shapes": []}
    for s in STATE_DIMS:
        for b in BATCH_SIZES:
            launches, agreement, whole, rec, keep = sides(s, b)
            rec["params_rel_diff_after_one_epoch"] = agreement()
            rec.update(timed(launches, args.reps, args.warmup, 1))
            rec["torch_over_kernel"] = rec["torch_us"] / rec["kernel_us"]
            rec["kernel_us_per_step"] = rec["kernel_us"] / rec["steps_per_epoch"]
            rec["torch_us_per_step"] = rec["torch_us"] / rec["steps_per_epoch"]
            if b == 32:
                rec["fit_reward_kernel_ms"] = whole("kernel", args.whole_reps)
                if s in args.whole_torch_dims:
                    rec["fit_reward_torch_ms"] = whole("torch", 1)
            res["shapes"].append(rec)
            print(json.dumps(rec), flush=True)
            del launches, agreement, whole, keep
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
