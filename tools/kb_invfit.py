#!/usr/bin/env python
"""What an epoch of the inverse head's fit costs on one GPU: python tools/kb_invfit.py [--out profiles/kb_invfit.json]

At N = 100 000 frames in episodes of 250, A = 6, batch sizes 32 and 256 and S in {3, 32, 200}, on the training transitions of
srlz.dynfit.split_episodes (80 % of the episodes), the two routes of srlz.invfit.fit_inverse side by side in one process:
  * kernel  one srlz_invfit_fit launch: every Adam step of the epoch by one persistent workgroup;
  * torch   srlz.invfit._torch_epoch: the same steps over the same uploaded table through autograd and torch.optim.Adam.
Device time per epoch from HIP events around one epoch (tools/kb_horizon.py's timed() with a burst of 1: every repetition times both
sides in turn, a side's own spread is the difference between the medians of its even and odd repetitions).  Both sides start every
epoch from the same parameters and zero moments, so both do the same arithmetic every time.  The baseline is the torch route in the
same run on the same GPU, never the kernel against itself.  Then the wall time of a whole default fit_inverse (30 epochs, batch size
32: upload, 30 fit and eval launches, the statistics read once) per route — the torch route's at --whole-torch-dims only, it takes
the better part of a minute — and the distance between the two routes' parameters after one epoch.
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

N_FRAMES, EP_LEN, A = 100000, 250, 6
STATE_DIMS = (3, 32, 200)
BATCH_SIZES = (32, 256)
LR = 0.005


def recording(s):
    rs = np.random.RandomState(s)
    actions = rs.randint(0, A, N_FRAMES)
    x = rs.randn(N_FRAMES, s).astype(np.float32)
    x[1:, 0] += 0.3 * actions[:-1].astype(np.float32)  # the action of a transition shows in its next state
    return x, actions, (np.arange(N_FRAMES) % EP_LEN) == 0


def sides(s, b):
    from srlz import invfit, ops
    dev = torch.device("cuda", 0)
    x, actions, es = recording(s)
    cfg = invfit.check_fit_inverse(x, actions, es, n_actions=A, epochs=1, batch_size=b, lr=LR)
    table = invfit.minibatch_tables(cfg["train"], 1, b, 0)[0]
    data = ops.RewardProbeData(torch.from_numpy(x).to(dev), torch.from_numpy(cfg["labels"]).to(dev))
    init = torch.from_numpy(cfg["init"]).to(dev)
    k_table, t_table = ops.headfit_table(data, torch.from_numpy(table)), torch.from_numpy(table).to(dev)
    params, m, v = init.clone(), torch.zeros_like(init), torch.zeros_like(init)
    n_cnt = ops.invfit_n_counts(A)
    loss, counts = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(n_cnt, dtype=torch.int64, device=dev)
    leaves = [t.clone().requires_grad_(True) for t in invfit._split_flat(init, s, A)]
    t_loss, t_counts = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(n_cnt, dtype=torch.int64, device=dev)

    def kernel_side():
        params.copy_(init)
        m.zero_()
        v.zero_()
        ops.invfit_fit(data, k_table, A, params, m, v, 0, LR, loss, counts)

    def torch_side():
        with torch.no_grad():
            for leaf, src in zip(leaves, invfit._split_flat(init, s, A)):
                leaf.copy_(src)
        opt = torch.optim.Adam(leaves, lr=LR)  # (fresh moments; its construction is host work outside the kernels' time)
        invfit._torch_epoch(data, t_table, leaves, opt, t_loss, t_counts, A)

    def whole(route, reps):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            invfit.fit_inverse(x, actions, es, n_actions=A, route=route)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3
    info = {"state_dim": s, "n_actions": A, "batch_size": b, "n_frames": N_FRAMES, "transitions": int(cfg["train"].size),
            "steps_per_epoch": int(table.shape[0]), "chunk_rows": ops.invfit_chunk_rows(s, A), "n_params": ops.invfit_n_params(s, A)}

    def agreement():
        kernel_side()
        torch_side()
        torch.cuda.synchronize()
        flat = torch.cat([t.detach().reshape(-1) for t in leaves])
        return float((params - flat).abs().max() / flat.abs().max())
    return {"kernel": kernel_side, "torch": torch_side}, agreement, whole, info, (data, k_table, t_table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_invfit.json"))
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--whole-torch-dims", type=int, nargs="*", default=[32])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_invfit measures on a GPU"
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
                rec["fit_inverse_kernel_ms"] = whole("kernel", args.whole_reps)
                if s in args.whole_torch_dims:
                    rec["fit_inverse_torch_ms"] = whole("torch", 1)
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
