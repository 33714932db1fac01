#!/usr/bin/env python
"""What scoring candidate plans on the learned state costs on one GPU: python tools/kb_dynamics.py [--out profiles/kb_dynamics.json]

For S in {3, 200}, A = 6 and (N, K, T) in {(1, 64, 10), (32, 256, 10)} — one environment with 64 candidate plans, and 32 environments
with 256 each, over a horizon of 10 — and the two routes of srlz.deploy.LatentDynamics — "rollout" (csrc/rollout.hip: one launch) and
"model" (the model's own forwardModel and rewardModel step by step: the training kernels, six launches a step, the code of the route
before the kernel existed) — on the same seeded SRLModules:
  * kernel_ms: HIP events around --burst back-to-back rollout calls on states and plans that are already on the device (the device's
    time per call; on the launch-bound "model" route this is the time its launches take to issue and drain);
  * launch_ms ("rollout" only): the same around --burst bare launches of srlz_rollout (no argument checks, no argmax): the kernel;
  * call_ms: host clock from host states and host plans in to the returns on the host, one synchronisation.
Both routes run interleaved in one process, call by call, after a warm-up; the figures are medians over --reps repetitions.  The two
routes' returns at each timed shape are compared as well (max difference over the returns' scale).  Also reported per shape: the
rollout's arithmetic from the shapes (2 R T (S (S + A) + 2 S H + H H + 2 H) FLOP) over its launch_ms.
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
sys.path.insert(0, REPO)

STATE_DIMS = (3, 200)
SHAPES = ((1, 64, 10), (32, 256, 10))
N_ACTIONS = 6
GAMMA = 0.95


def kernel_ms(dyn, z, pl, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        dyn.rollout(z, pl, gamma=GAMMA)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst


def launch_ms(dyn, z, pl, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, k, t = pl.shape
    s, o = dyn.state_dim, dyn.owner
    rn = o.reward_net
    head = (rn[0].weight, rn[0].bias, rn[2].weight, rn[2].bias, rn[4].weight, rn[4].bias)
    final, returns = dyn._final[:n * k * s].view(n, k, s), dyn._returns[:n * k].view(n, k)
    from srlz import ops
    a.record()
    for _ in range(burst):
        ops.rollout(z, pl, o.forward_net.weight, o.forward_net.bias, reward=head, final=final, returns=returns, gamma=GAMMA)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst


def call_ms(dyn, z, pl):
    t0 = time.perf_counter()
    dyn.rollout(z, pl, gamma=GAMMA).returns.cpu()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_dynamics.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_dynamics measures on a GPU"
    import bench
    import dynamics_util as dy
    from models.modules import SRLModules
    from srlz import deploy
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "n_actions": N_ACTIONS, "gamma": GAMMA, "model": "SRLModules custom_cnn, losses forward inverse reward",
           "shapes": []}
    for s in STATE_DIMS:
        torch.manual_seed(1)
        model = SRLModules(state_dim=s, action_dim=N_ACTIONS, cuda=True, model_type="custom_cnn",
                           losses=["forward", "inverse", "reward"]).to(torch.device("cuda", 0))
        dyns = {"rollout": deploy.LatentDynamics(model, max_rows=8192, max_horizon=10), "model": deploy.LatentDynamics(model, route="model")}
        h = model.reward_net[0].out_features
        for n, k, t in SHAPES:
            z, pl = dy.sine_states(n, s), dy.plans(n, k, t, N_ACTIONS)
            z_dev, pl_dev = torch.from_numpy(z).cuda(), torch.from_numpy(pl).cuda()
            for _ in range(args.warmup):
                for d in dyns.values():
                    call_ms(d, z, pl)
                    kernel_ms(d, z_dev, pl_dev, 2)
            torch.cuda.synchronize()
            tm = {r: {"kernel_ms": [], "call_ms": []} for r in dyns}
            for _ in range(args.reps):
                for r, d in dyns.items():  # interleaved: a drift of the machine falls on both routes alike
                    tm[r]["call_ms"].append(call_ms(d, z, pl))
                for r, d in dyns.items():
                    tm[r]["kernel_ms"].append(kernel_ms(d, z_dev, pl_dev, args.burst))
                tm["rollout"].setdefault("launch_ms", []).append(launch_ms(dyns["rollout"], z_dev, pl_dev, 4 * args.burst))
            assert dyns["rollout"].route == "rollout" and dyns["model"].route == "model"
            ra = dyns["rollout"].rollout(z_dev, pl_dev, gamma=GAMMA).returns.double().cpu()
            rb = dyns["model"].rollout(z_dev, pl_dev, gamma=GAMMA).returns.double().cpu()
            rec = {"state_dim": s, "n": n, "k": k, "t": t, "rows": n * k,
                   "returns_max_diff_over_scale": float((ra - rb).abs().max() / rb.abs().max())}
            for r in dyns:
                for q in ("kernel_ms", "call_ms"):
                    rec["%s_%s" % (r, q)] = float(np.median(tm[r][q]))
                    rec["%s_%s_min" % (r, q)] = float(np.min(tm[r][q]))
            rec["rollout_launch_ms"] = float(np.median(tm["rollout"]["launch_ms"]))
            rec["rollout_launch_ms_min"] = float(np.min(tm["rollout"]["launch_ms"]))
            rec["call_speedup"] = rec["model_call_ms"] / rec["rollout_call_ms"]
            rec["kernel_speedup"] = rec["model_kernel_ms"] / rec["rollout_kernel_ms"]
            rec["rollout_faster_in_call_latency"] = bool(rec["rollout_call_ms"] < rec["model_call_ms"])
            rec["rollout_faster_in_device_time"] = bool(rec["rollout_kernel_ms"] < rec["model_kernel_ms"])
            flop = 2.0 * n * k * t * (s * (s + N_ACTIONS) + 2 * s * h + h * h + 2 * h)
            rec["rollout_gflop"] = flop / 1e9
            rec["rollout_tflops_over_launch_ms"] = flop / (rec["rollout_launch_ms"] * 1e-3) / 1e12
            res["shapes"].append(rec)
            print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
