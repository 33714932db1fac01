#!/usr/bin/env python
"""What tree search on the learned state costs on one GPU: python tools/kb_search.py [--out profiles/kb_search.json]

Seeded heads at S = 200, H = 16 (SRLModules, losses forward inverse reward).  Shapes: exact search at (A = 6, T = 4) and (A = 4,
T = 6), N = 1 and N = 32 environments; a beam of 64 at T = 10 (A = 6), N = 1 and N = 32.  On the same model, in one process:
  * "search": srlz.deploy.LatentDynamics.search (csrc/beam.hip: one launch per level, every prefix expanded once);
  * "enumerate" (exact shapes): LatentDynamics.rollout over the same A^T enumerated plans, already on the device, and the argmax of
    its returns — the same optimum, bit for bit (checked), at T * A^T forward steps;
  * "cem": LatentDynamics.plan with its defaults (64 plans, 4 iterations), timed the same way; its regret — the exact best_return
    minus the planner's best_return — as mean and max over 32 seeded environments (exact shapes).
Timed:
  * call_ms: host clock from states on the device in to the first action of the best plan on the host, one call;
  * device_ms: HIP events around --burst back-to-back calls, per call.
The sides run interleaved, call by call, after a warm-up; the figures are medians over --reps repetitions.
Prints one JSON object and writes it to --out with csrc_sha16, the fingerprint of the kernel sources it was recorded at."""
import argparse
import itertools
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

STATE_DIM = 200
#          A  T   beam (None: exact)
TREES = ((6, 4, None), (4, 6, None), (6, 10, 64))
ENVS = (1, 32)
GAMMA = 0.95
REGRET_ENVS = 32


def run(side, dyn, z, t, beam, plans):
    """One call of a side; returns the tensor whose arrival on the host ends the call."""
    if side == "search":
        return dyn.search(z, t, beam=beam, gamma=GAMMA).action
    if side == "cem":
        return dyn.plan(z, t, gamma=GAMMA).action
    out = dyn.rollout(z, plans, gamma=GAMMA)
    return plans[out.best, 0]


def call_ms(side, dyn, z, t, beam, plans):
    t0 = time.perf_counter()
    run(side, dyn, z, t, beam, plans).cpu()
    return (time.perf_counter() - t0) * 1e3


def device_ms(side, dyn, z, t, beam, plans, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        run(side, dyn, z, t, beam, plans)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_search.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_search measures on a GPU"
    import bench
    import dynamics_util as dy
    from models.modules import SRLModules
    from srlz import deploy
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "state_dim": STATE_DIM, "gamma": GAMMA, "model": "SRLModules custom_cnn, losses forward inverse reward",
           "cem": "LatentDynamics.plan defaults: n_plans 64, iterations 4, elites 8, sharpness 8, seed 0", "shapes": []}
    for a, t, beam in TREES:
        torch.manual_seed(1)
        model = SRLModules(state_dim=STATE_DIM, action_dim=a, cuda=True, model_type="custom_cnn",
                           losses=["forward", "inverse", "reward"]).to(torch.device("cuda", 0))
        exact = beam is None
        w = a ** (t - 1) if exact else beam
        sizes = deploy.search_sizes(w, t, a)
        dyn = deploy.LatentDynamics(model, max_rows=max(ENVS) * sizes["leaves"], max_horizon=t)
        plans = torch.from_numpy(np.array(list(itertools.product(range(a), repeat=t)), np.int32)).cuda() if exact else None
        sides = ("search", "enumerate", "cem") if exact else ("search", "cem")
        regret = None
        if exact:  # the regret of the sampling planner, over 32 seeded environments
            z = torch.from_numpy(dy.sine_states(REGRET_ENVS, STATE_DIM)).cuda()
            best = dyn.search(z, t, beam=w, gamma=GAMMA).best_return.clone()
            gap = (best - dyn.plan(z, t, gamma=GAMMA).best_return).double().cpu().numpy()
            regret = {"mean": float(gap.mean()), "max": float(gap.max()), "min": float(gap.min()), "envs": REGRET_ENVS,
                      "exact_best_return_mean": float(best.double().mean())}
        for n in ENVS:
            z = torch.from_numpy(dy.sine_states(n, STATE_DIM)).cuda()
            for _ in range(args.warmup):
                for side in sides:
                    call_ms(side, dyn, z, t, w, plans)
                    device_ms(side, dyn, z, t, w, plans, 2)
            torch.cuda.synchronize()
            tm = {side: {"call_ms": [], "device_ms": []} for side in sides}
            for _ in range(args.reps):
                for side in sides:  # interleaved: a drift of the machine falls on every side alike
                    tm[side]["call_ms"].append(call_ms(side, dyn, z, t, w, plans))
                for side in sides:
                    tm[side]["device_ms"].append(device_ms(side, dyn, z, t, w, plans, args.burst))
            got = dyn.search(z, t, beam=w, gamma=GAMMA)
            assert dyn.route == "rollout" and got.exact == exact
            rec = {"n_actions": a, "t": t, "n": n, "beam": w, "exact": exact, "leaves": sizes["leaves"], "expanded_steps": sizes["expanded"]}
            if exact:
                best_plan, best_return = got.best_plan.cpu().numpy(), got.best_return.cpu().numpy()
                out = dyn.rollout(z, plans, gamma=GAMMA)
                assert dyn.route == "rollout"
                top = out.best.cpu().numpy()
                ref = out.returns.cpu().numpy()[np.arange(n), top]
                rec["enumerated_steps"] = t * a ** t
                rec["same_best_plan_and_return"] = bool(np.array_equal(best_plan, plans.cpu().numpy()[top]) and
                                                        np.array_equal(best_return.view(np.uint32), ref.view(np.uint32)))
                rec["cem_regret"] = regret
            for side in sides:
                for q in ("call_ms", "device_ms"):
                    rec["%s_%s" % (side, q)] = float(np.median(tm[side][q]))
                    rec["%s_%s_min" % (side, q)] = float(np.min(tm[side][q]))
            if exact:
                rec["device_ratio_search_over_enumerate"] = rec["search_device_ms"] / rec["enumerate_device_ms"]
                rec["search_faster_than_enumerate_in_device_time"] = bool(rec["search_device_ms"] < rec["enumerate_device_ms"])
                rec["search_faster_than_enumerate_in_call_latency"] = bool(rec["search_call_ms"] < rec["enumerate_call_ms"])
            rec["device_ratio_search_over_cem"] = rec["search_device_ms"] / rec["cem_device_ms"]
            res["shapes"].append(rec)
            print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
