#!/usr/bin/env python
"""What planning on the learned state costs on one GPU: python tools/kb_plan.py [--out profiles/kb_plan.json]

For S in {3, 200}, A = 6 and (N, K, T, I) in {(1, 64, 10, 4), (32, 256, 10, 4)} — one environment searching with 64 plans, and 32
environments with 256 each, over a horizon of 10 and 4 iterations of the cross-entropy method, 8 elites — on the same seeded SRLModules:
  * "plan": srlz.deploy.LatentDynamics.plan (csrc/plan.hip: one launch per iteration, no plan on the host);
  * "hostloop": what the code offered before the planner existed — the same search as a host loop over LatentDynamics.rollout on its
    route "rollout": numpy sampling, upload, one launch, download of the returns, numpy select and refit, per iteration
    (srlz.deploy.cem_host over dyn.rollout: the two sides reach the same best plan, bit for bit, which is checked).
Timed:
  * call_ms: host clock from states on the device in to the first action of the best plan on the host, one call;
  * device_ms: "plan": HIP events around --burst back-to-back plan calls, per call; "hostloop": I times the same around --burst
    back-to-back rollout calls on plans already on the device (its device work alone: the host loop itself synchronises every iteration).
Both sides run interleaved in one process, call by call, after a warm-up; the figures are medians over --reps repetitions.
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
SHAPES = ((1, 64, 10, 4), (32, 256, 10, 4))
N_ACTIONS = 6
ELITES, SHARPNESS, GAMMA, SEED = 8, 8, 0.95, 7


def plan_call(dyn, z, k, t, it):
    return dyn.plan(z, t, n_plans=k, iterations=it, elites=ELITES, sharpness=SHARPNESS, gamma=GAMMA, seed=SEED)


def hostloop_call(dyn, z, k, t, it):
    from srlz import deploy
    n = z.shape[0]
    return deploy.cem_host(lambda pl: dyn.rollout(z, pl, gamma=GAMMA).returns.cpu().numpy(), n, k, t, N_ACTIONS, it, ELITES, SHARPNESS,
                           SEED)


def call_ms(side, dyn, z, k, t, it):
    t0 = time.perf_counter()
    if side == "plan":
        plan_call(dyn, z, k, t, it).action.cpu()
    else:
        hostloop_call(dyn, z, k, t, it)["best_plan"][:, 0]
    return (time.perf_counter() - t0) * 1e3


def device_ms(side, dyn, z, pl, k, t, it, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        if side == "plan":
            plan_call(dyn, z, k, t, it)
        else:
            dyn.rollout(z, pl, gamma=GAMMA)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst * (1 if side == "plan" else it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_plan.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_plan measures on a GPU"
    import bench
    import dynamics_util as dy
    from models.modules import SRLModules
    from srlz import deploy
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "n_actions": N_ACTIONS, "elites": ELITES, "sharpness": SHARPNESS, "gamma": GAMMA, "seed": SEED,
           "model": "SRLModules custom_cnn, losses forward inverse reward", "shapes": []}
    sides = ("plan", "hostloop")
    for s in STATE_DIMS:
        torch.manual_seed(1)
        model = SRLModules(state_dim=s, action_dim=N_ACTIONS, cuda=True, model_type="custom_cnn",
                           losses=["forward", "inverse", "reward"]).to(torch.device("cuda", 0))
        dyn = deploy.LatentDynamics(model, max_rows=8192, max_horizon=10)
        for n, k, t, it in SHAPES:
            z_dev = torch.from_numpy(dy.sine_states(n, s)).cuda()
            pl_dev = torch.from_numpy(dy.plans(n, k, t, N_ACTIONS)).cuda()
            for _ in range(args.warmup):
                for side in sides:
                    call_ms(side, dyn, z_dev, k, t, it)
                    device_ms(side, dyn, z_dev, pl_dev, k, t, it, 2)
            torch.cuda.synchronize()
            tm = {side: {"call_ms": [], "device_ms": []} for side in sides}
            for _ in range(args.reps):
                for side in sides:  # interleaved: a drift of the machine falls on both sides alike
                    tm[side]["call_ms"].append(call_ms(side, dyn, z_dev, k, t, it))
                for side in sides:
                    tm[side]["device_ms"].append(device_ms(side, dyn, z_dev, pl_dev, k, t, it, args.burst))
            got = plan_call(dyn, z_dev, k, t, it)
            assert dyn.route == "rollout"
            best_plan, best_return = got.best_plan.cpu().numpy(), got.best_return.cpu().numpy()
            ref = hostloop_call(dyn, z_dev, k, t, it)
            assert dyn.route == "rollout"
            rec = {"state_dim": s, "n": n, "k": k, "t": t, "iterations": it,
                   "same_best_plan_and_return": bool(np.array_equal(best_plan, ref["best_plan"]) and
                                                     np.array_equal(best_return.view(np.uint32), ref["best_return"].view(np.uint32)))}
            for side in sides:
                for q in ("call_ms", "device_ms"):
                    rec["%s_%s" % (side, q)] = float(np.median(tm[side][q]))
                    rec["%s_%s_min" % (side, q)] = float(np.min(tm[side][q]))
            rec["call_speedup"] = rec["hostloop_call_ms"] / rec["plan_call_ms"]
            rec["device_ratio_plan_over_hostloop"] = rec["plan_device_ms"] / rec["hostloop_device_ms"]
            rec["plan_faster_in_call_latency"] = bool(rec["plan_call_ms"] < rec["hostloop_call_ms"])
            rec["plan_faster_in_device_time"] = bool(rec["plan_device_ms"] < rec["hostloop_device_ms"])
            res["shapes"].append(rec)
            print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
