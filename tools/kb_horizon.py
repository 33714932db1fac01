#!/usr/bin/env python
"""What the k-step error costs on one GPU: python tools/kb_horizon.py [--base-lib OTHER/libsrlz_hip.so] [--out profiles/kb_horizon.json]

At S = 200, A = 6, H = 16 (seeded heads of tests/dynamics_util.py), T = 10 and M = 20 000 and 100 000 consecutive starts of one
recorded episode of M + T + 1 frames (every row has all T steps):
  * device time per call, HIP events around --burst back-to-back calls on buffers made once, of
      horizon     srlz_horizon_rows + srlz_horizon_sums through the C ABI: the two launches of LatentDynamics.horizon_error
      rows, sums  each of the two alone
      rollout     the route the tree offered for the same answer before: srlz_rollout with K = 1 plans (made beforehand, not timed)
                  and the trajectory [M,T,S] and logits kept, then torch reductions — the squared differences against the recorded
                  rows (a strided view, nothing is gathered), the per-horizon fp64 sums and the hit count
    with the bytes each route moves beside the imagined states and the agreement of the two answers;
  * with --base-lib, the library of another tree (the parent commit's, built beside this one) loaded into the same process: its
    srlz_rollout, srlz_rollout_goal, srlz_plan_cem and srlz_plan_cem_goal against this tree's at tools/kb_goal.py's shapes, outputs
    compared bit for bit.  Every repetition times all sides in turn (interleaved); a side's own run-to-run spread is the difference
    between the medians of its even and its odd repetitions — a ratio between the two trees inside those spreads is no difference.
Prints one JSON object and writes it to --out with csrc_sha16, the fingerprint of the kernel sources it was recorded at."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, REPO)

S, A, H, T = 200, 6, 16, 10
ROWS = (20000, 100000)
SHARED = ("srlz_rollout", "srlz_rollout_goal", "srlz_plan_cem", "srlz_plan_cem_goal")


def base_library(path, C):
    """Another tree's library with the prototypes of the calls both trees have."""
    lib = ctypes.CDLL(path)
    for name in SHARED + ("srlz_plan_workspace",):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C._PROTOS[name]
    return lib


def horizon_sides(C, m):
    """{side: launch once} at M = m consecutive starts, and a function giving both routes' answers."""
    import dynamics_util as dy
    from srlz import ops
    dev = torch.device("cuda", 0)
    n = m + T + 1
    p = tuple(x.to(dev) for x in dy.seeded_heads(S, A, H))
    i = np.arange(n)
    z = torch.from_numpy(dy.sine_states(n, S)).to(dev)
    acts = torch.from_numpy(((3 * i + i // 4) % A).astype(np.int32)).to(dev)
    labels = torch.from_numpy((i % 3 == 0).astype(np.int32)).to(dev)
    starts = torch.arange(m, dtype=torch.int32, device=dev)
    lens = torch.full((m,), T, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    err, base, logits = f32(m, T), f32(m, T), f32(m, T, 2)
    count, hits = torch.empty(T, dtype=torch.int64, device=dev), torch.empty(T, dtype=torch.int64, device=dev)
    sum_err, sum_base = torch.empty(T, dtype=torch.float64, device=dev), torch.empty(T, dtype=torch.float64, device=dev)

    def rows():
        ops.horizon_rows(z, acts, starts, lens, p[0], p[1], err, base, T, reward=p[2:], reward_logits=logits)

    def sums():
        ops.horizon_sums(err, base, starts, lens, count, sum_err, sum_base, reward_logits=logits, labels=labels, hits=hits)

    def horizon():
        rows()
        sums()
    # the earlier route: K = 1 plans from the recorded actions, the whole trajectory written and read back
    plans = acts.unfold(0, T, 1)[:m].contiguous().view(m, 1, T)
    z0 = z[:m]
    final, traj, lg = f32(m, 1, S), f32(m, 1, T, S), f32(m, 1, T, 2)
    target = z[1:].unfold(0, T, 1)[:m].permute(0, 2, 1)          # [M,T,S] view: entry (r, t) = states[r + t + 1]
    lab = labels.unfold(0, T, 1)[:m]                               # [M,T] view: entry (r, t) = labels[r + t]
    answer = {}

    def rollout():
        ops.rollout(z0, plans, p[0], p[1], reward=p[2:], final=final, trajectory=traj, reward_logits=lg)
        e = (traj[:, 0] - target).pow(2).sum(-1)
        b = (z0[:, None, :] - target).pow(2).sum(-1)
        answer["sum_err"], answer["sum_base"] = e.double().sum(0), b.double().sum(0)
        answer["hits"] = ((lg[:, 0, :, 1] > lg[:, 0, :, 0]).to(torch.int32) == lab).sum(0)

    def agreement():
        horizon()
        rollout()
        torch.cuda.synchronize()
        rel = lambda a, b: float(((a - b).abs() / b.abs()).max())  # noqa: E731
        return {"sum_err_rel_diff": rel(sum_err, answer["sum_err"]), "sum_base_rel_diff": rel(sum_base, answer["sum_base"]),
                "hits_equal": bool(torch.equal(hits, answer["hits"])), "count_ok": bool((count == m).all())}
    keep = (p, z, acts, labels, starts, lens, plans)  # (the launches hold raw pointers)
    return {"horizon": horizon, "rows": rows, "sums": sums, "rollout": rollout}, agreement, keep


def tree_sides(C, base, n, k, t):
    """{side: (launch once, the tensor whose bits are compared)} of the calls both trees have, this tree's and `base_`'s."""
    import dynamics_util as dy
    import kb_goal as kg
    dev = torch.device("cuda", 0)
    p = tuple(x.to(dev) for x in dy.seeded_heads(S, A, H))
    z = torch.from_numpy(dy.sine_states(n, S)).to(dev)
    goal = torch.from_numpy(dy.sine_states(n + 1, S)[1:].copy()).to(dev)
    pl = torch.from_numpy(dy.plans(n, k, t, A)).to(dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    ptr, stream = C.ptr, C.stream
    head = [ptr(x) for x in p[2:]]
    ws = torch.empty(int(C.plan_workspace(n, k, t, 0)), dtype=torch.uint8, device=dev)
    g = [ptr(goal), S, kg.WEIGHT, 0]
    sides = {}
    for prefix, lib in (("", C._lib), ("base_", base)):
        for name, goal_args in (("rollout", []), ("rollout_goal", g + [None])):
            fn = getattr(lib, "srlz_" + name)
            final, ret = f32(n, k, S), f32(n, k)
            args = [ptr(z), ptr(pl), k * t, ptr(p[0]), ptr(p[1])] + head + [ptr(final), ptr(ret), None, None, n, k, t, S, A, H, 2, kg.GAMMA] + goal_args
            sides[prefix + name] = (lambda fn=fn, args=args: fn(*(args + [stream()])), ret, final)
        for name, goal_args in (("plan_cem", []), ("plan_cem_goal", g)):
            fn = getattr(lib, "srlz_" + name)
            best, ret, cum = i32(n, t), f32(n), i32(n, t, A)
            args = [ptr(z), ptr(p[0]), ptr(p[1])] + head + [None, 0, ptr(best), ptr(ret), ptr(cum), None, None, ptr(ws), ws.numel(), n, k, t, S, A, H,
                                                            2, kg.ITERATIONS, kg.ELITES, kg.SHARPNESS, kg.GAMMA, kg.SEED] + goal_args
            sides[prefix + name] = (lambda fn=fn, args=args: fn(*(args + [stream()])), ret, best)
    sides["_keep"] = (p, z, goal, pl, ws)
    return sides


def burst_us(launch, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst * 1e3


def timed(launches, reps, warmup, burst):
    """{side: {us, us_min, spread}}: every repetition times all sides in turn."""
    names = list(launches)
    for _ in range(warmup):
        for s in names:
            burst_us(launches[s], 2)
    tm = {s: [] for s in names}
    for _ in range(reps):
        for s in names:
            tm[s].append(burst_us(launches[s], burst))
    rec = {}
    for s in names:
        v = np.array(tm[s])
        rec[s + "_us"], rec[s + "_us_min"] = float(np.median(v)), float(v.min())
        rec[s + "_spread"] = float(abs(np.median(v[0::2]) - np.median(v[1::2])) / np.median(v))  # run to run, same code
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_horizon.json"))
    ap.add_argument("--base-lib", default=None, help="libsrlz_hip.so of another tree (the parent commit) for the in-process A/B")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--tree-burst", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_horizon measures on a GPU"
    import bench
    import kb_goal as kg
    from srlz import _cabi as C
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "state_dim": S, "n_actions": A, "hidden": H, "horizon": T, "base_lib": bool(args.base_lib), "rows": [],
           "trees": []}
    for m in ROWS:
        launches, agreement, keep = horizon_sides(C, m)
        rec = {"m": m, "n_frames": m + T + 1}
        rec.update(agreement())
        rec.update(timed(launches, args.reps, args.warmup, args.burst))
        rec["rollout_over_horizon"] = rec["rollout_us"] / rec["horizon_us"]
        rec["states_bytes"] = (m + T + 1) * S * 4
        rec["trajectory_bytes"] = m * T * S * 4  # what the earlier route writes and reads back; the new one never writes it
        rec["states_bytes_per_us_rows"] = rec["states_bytes"] / rec["rows_us"]
        res["rows"].append(rec)
        print(json.dumps(rec))
        del launches, agreement, keep
        torch.cuda.empty_cache()
    if args.base_lib:
        base = base_library(args.base_lib, C)
        for n, k, t in kg.SHAPES:
            sides = tree_sides(C, base, n, k, t)
            rec = {"n": n, "k": k, "t": t}
            rec.update(timed({s: v[0] for s, v in sides.items() if not s.startswith("_")}, 30, 3, args.tree_burst))
            for name in ("rollout", "rollout_goal", "plan_cem", "plan_cem_goal"):
                rec[name + "_over_base"] = rec[name + "_us"] / rec["base_" + name + "_us"]
                rec[name + "_same_bits_as_base"] = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                                                        for a, b in zip(sides[name][1:], sides["base_" + name][1:]))
            res["trees"].append(rec)
            print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
