#!/usr/bin/env python
"""What the goal term costs on one GPU: python tools/kb_goal.py [--base-lib OTHER/libsrlz_hip.so] [--out profiles/kb_goal.json]

At S = 200, A = 6, H = 16 (seeded heads of tests/dynamics_util.py) and the README's two shapes (N, K, T) = (1, 64, 10) and
(32, 256, 10), the planner with I = 4 iterations and 8 elites:
  * device time per call, HIP events around --burst back-to-back calls through the C ABI on buffers made once, of
      rollout             srlz_rollout with the reward head            rollout_nohead       srlz_rollout without it
      rollout_goal        srlz_rollout_goal with the head              rollout_goal_nohead  the goal term alone
      plan                srlz_plan_cem                                plan_goal / plan_goal_nohead   srlz_plan_cem_goal
    so that  head = rollout - rollout_nohead  and  goal = rollout_goal - rollout  are the two terms' costs at the same shape;
  * with --base-lib, the library of another tree (the parent commit's, built beside this one) loaded into the same process:
    base_rollout and base_plan are its srlz_rollout / srlz_plan_cem on the same buffers.  Every repetition times all sides in turn
    (interleaved: a drift of the machine falls on all alike); the parent's own run-to-run spread is the difference between the medians
    of its even and its odd repetitions, and this tree's is taken the same way — a difference between the two trees inside those
    spreads is no difference.  The outputs of the two libraries are compared bit for bit;
  * route "model" against the kernel route through srlz.deploy.LatentDynamics (rollout and plan with a goal): host clock around one
    call that ends in a device synchronise.
Prints one JSON object and writes it to --out with csrc_sha16, the fingerprint of the kernel sources it was recorded at."""
import argparse
import ctypes
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

S, A, H = 200, 6, 16
SHAPES = ((1, 64, 10), (32, 256, 10))
ITERATIONS, ELITES, SHARPNESS, GAMMA, SEED, WEIGHT = 4, 8, 8, 0.95, 7, 0.5


def base_library(path, C):
    """Another tree's library with the prototypes of the two calls both trees have."""
    lib = ctypes.CDLL(path)
    for name in ("srlz_rollout", "srlz_plan_cem", "srlz_plan_workspace"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C._PROTOS[name]
    return lib


def sides_of(C, base, n, k, t):
    """{side: (launch once, the tensor whose bits are compared)} on buffers made here."""
    import dynamics_util as dy
    dev = torch.device("cuda", 0)
    p = tuple(x.to(dev) for x in dy.seeded_heads(S, A, H))
    z = torch.from_numpy(dy.sine_states(n, S)).to(dev)
    goal = torch.from_numpy(dy.sine_states(n + 1, S)[1:].copy()).to(dev)
    pl = torch.from_numpy(dy.plans(n, k, t, A)).to(dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    ptr, stream = C.ptr, C.stream
    head, nohead = [ptr(x) for x in p[2:]], [None] * 6
    ws = torch.empty(int(C.plan_workspace(n, k, t, 0)), dtype=torch.uint8, device=dev)
    sides = {}

    def rollout(fn, hd, goal_args, key):
        final, ret = f32(n, k, S), f32(n, k)
        args = [ptr(z), ptr(pl), k * t, ptr(p[0]), ptr(p[1])] + hd + [ptr(final), ptr(ret) if hd is head or goal_args else None, None, None,
                                                                       n, k, t, S, A, H, 2, GAMMA] + goal_args
        sides[key] = (lambda: fn(*(args + [stream()])), ret if hd is head or goal_args else final)

    def plan(fn, hd, goal_args, key):
        best, ret, cum = i32(n, t), f32(n), i32(n, t, A)
        args = [ptr(z), ptr(p[0]), ptr(p[1])] + hd + [None, 0, ptr(best), ptr(ret), ptr(cum), None, None, ptr(ws), ws.numel(), n, k, t, S, A, H, 2,
                                                      ITERATIONS, ELITES, SHARPNESS, GAMMA, SEED] + goal_args
        sides[key] = (lambda: fn(*(args + [stream()])), ret)
    g = [ptr(goal), S, WEIGHT, 0]
    rollout(C.rollout, head, [], "rollout")
    rollout(C.rollout, nohead, [], "rollout_nohead")
    rollout(C.rollout_goal, head, g + [None], "rollout_goal")
    rollout(C.rollout_goal, nohead, g + [None], "rollout_goal_nohead")
    plan(C.plan_cem, head, [], "plan")
    plan(C.plan_cem_goal, head, g, "plan_goal")
    plan(C.plan_cem_goal, nohead, g, "plan_goal_nohead")
    if base is not None:
        rollout(base.srlz_rollout, head, [], "base_rollout")
        plan(base.srlz_plan_cem, head, [], "base_plan")
    sides["_keep"] = (p, z, goal, pl, ws)  # (the launches hold raw pointers)
    return sides


def burst_us(launch, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst * 1e3


def routes(n, k, t, reps):
    """Host-clock ms of one synchronised call with a goal, kernel route against route "model", rollout and plan."""
    import dynamics_util as dy
    from models.modules import SRLModules
    from srlz import deploy
    torch.manual_seed(1)
    model = SRLModules(state_dim=S, action_dim=A, cuda=True, model_type="custom_cnn", losses=["forward", "inverse", "reward"]).to(torch.device("cuda", 0))
    z = torch.from_numpy(dy.sine_states(n, S)).cuda()
    goal = torch.from_numpy(dy.sine_states(n + 1, S)[1:].copy()).cuda()
    pl = torch.from_numpy(dy.plans(n, k, t, A)).cuda()
    out = {}
    for route in ("rollout", "model"):
        dyn = deploy.LatentDynamics(model, max_rows=8192, max_horizon=t, route=None if route == "rollout" else "model")
        calls = {"rollout_goal": lambda: dyn.rollout(z, pl, gamma=GAMMA, goal=goal, goal_weight=WEIGHT).returns,
                 "plan_goal": lambda: dyn.plan(z, t, n_plans=k, iterations=ITERATIONS, elites=ELITES, sharpness=SHARPNESS, gamma=GAMMA, seed=SEED,
                                               goal=goal, goal_weight=WEIGHT).best_plan}
        for name, call in calls.items():
            times = []
            for i in range(reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if i >= 2:  # (two warm-up calls)
                    times.append((time.perf_counter() - t0) * 1e3)
            assert dyn.route == route, (dyn.route, route)
            out["%s_route_%s_call_ms" % (name, route)] = float(np.median(times))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_goal.json"))
    ap.add_argument("--base-lib", default=None, help="libsrlz_hip.so of another tree (the parent commit) for the in-process A/B")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--route-reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_goal measures on a GPU"
    import bench
    from srlz import _cabi as C
    base = base_library(args.base_lib, C) if args.base_lib else None
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "state_dim": S, "n_actions": A, "hidden": H, "iterations": ITERATIONS, "elites": ELITES, "gamma": GAMMA,
           "goal_weight": WEIGHT, "base_lib": bool(base), "shapes": []}
    for n, k, t in SHAPES:
        sides = sides_of(C, base, n, k, t)
        names = [s for s in sides if not s.startswith("_")]
        for _ in range(args.warmup):
            for s in names:
                burst_us(sides[s][0], 5)
        tm = {s: [] for s in names}
        for _ in range(args.reps):
            for s in names:
                tm[s].append(burst_us(sides[s][0], args.burst))
        rec = {"n": n, "k": k, "t": t}
        for s in names:
            v = np.array(tm[s])
            rec[s + "_us"] = float(np.median(v))
            rec[s + "_us_min"] = float(v.min())
            rec[s + "_spread"] = float(abs(np.median(v[0::2]) - np.median(v[1::2])) / np.median(v))  # run to run, same code
        rec["head_cost_us"] = rec["rollout_us"] - rec["rollout_nohead_us"]
        rec["goal_cost_us"] = rec["rollout_goal_us"] - rec["rollout_us"]
        rec["goal_cost_nohead_us"] = rec["rollout_goal_nohead_us"] - rec["rollout_nohead_us"]
        rec["plan_goal_cost_us"] = rec["plan_goal_us"] - rec["plan_us"]
        if base is not None:
            for new, old in (("rollout", "base_rollout"), ("plan", "base_plan")):
                rec["%s_over_base" % new] = rec[new + "_us"] / rec[old + "_us"]
                rec["%s_same_bits_as_base" % new] = bool(torch.equal(sides[new][1].view(torch.int32), sides[old][1].view(torch.int32)))
        rec.update(routes(n, k, t, args.route_reps))
        res["shapes"].append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
