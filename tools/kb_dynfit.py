#!/usr/bin/env python
"""What the forward head's normal equations cost on one GPU: python tools/kb_dynfit.py [--out profiles/kb_dynfit.json]

At N = 100 000 frames in episodes of 250 (99 600 transitions), A = 6 and S in {3, 32, 200}, the two routes of srlz.dynfit.fit_forward
side by side in one process:
  * gram    srlz_dynfit_gram through srlz.ops.dynfit_gram: the table of transitions uploaded, two launches into buffers made once;
  * torch   srlz.dynfit._torch_gram: the same upload, Z [M, S+A+1] and Y [M, S] built in fp64 on the device, two matmuls.
Device time per call from HIP events around --burst back-to-back calls (tools/kb_horizon.py's timed(): every repetition times both
sides in turn, a side's own spread is the difference between the medians of its even and odd repetitions), the peak of the caching
allocator above the resident inputs for one call of each (what the torch route materialises), the wall time of a whole fit_forward per
route (upload, normal equations, download, host solve), and the agreement of the two answers.
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


def recording(s):
    rs = np.random.RandomState(s)
    x = (rs.randn(N_FRAMES, s) * np.array([1e-2, 1.0, 1e2])[np.arange(s) % 3]).astype(np.float32)
    return x, rs.randint(0, A, N_FRAMES), (np.arange(N_FRAMES) % EP_LEN) == 0


def sides(s):
    from srlz import dynfit, ops
    dev = torch.device("cuda", 0)
    x, acts, es = recording(s)
    acts32, starts, a = dynfit.check_fit_recording(x, acts, es)
    d_x, d_acts, h_starts = torch.from_numpy(x).to(dev), torch.from_numpy(acts32).to(dev), torch.from_numpy(starts)
    m, p = len(starts), s + a + 1
    gram = torch.empty((p, p), dtype=torch.float64, device=dev)
    cross = torch.empty((p, s), dtype=torch.float64, device=dev)
    ws = torch.empty(ops.dynfit_workspace(m, s, a), dtype=torch.uint8, device=dev)
    answer = {}

    def gram_side():
        ops.dynfit_gram(d_x, d_acts, h_starts, a, gram=gram, cross=cross, workspace=ws)

    def torch_side():
        answer["G"], answer["C"] = dynfit._torch_gram(d_x, d_acts, h_starts.to(dev), a)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    def whole(route, reps=5):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dynfit.fit_forward(x, acts, es, route=route)
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3
    info = {"state_dim": s, "n_actions": a, "n_frames": N_FRAMES, "transitions": m, "system": p,
            "chunk_rows": ops.dynfit_chunk_rows(m, s, a), "workspace_bytes": int(ws.numel()),
            "materialised_bytes_torch": m * (p + s) * 8}
    return {"gram": gram_side, "torch": torch_side}, answer, (gram, cross), peak, whole, info, (d_x, d_acts, h_starts, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_dynfit.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--burst", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_dynfit measures on a GPU"
    import bench
    from kb_horizon import timed
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "shapes": []}
    for s in STATE_DIMS:
        launches, answer, (gram, cross), peak, whole, rec, keep = sides(s)
        launches["gram"]()
        launches["torch"]()
        torch.cuda.synchronize()
        scale_g, scale_c = float(answer["G"].abs().max()), float(answer["C"].abs().max())
        rec["gram_rel_diff"] = float((gram - answer["G"]).abs().max()) / scale_g
        rec["cross_rel_diff"] = float((cross - answer["C"]).abs().max()) / scale_c
        rec["gram_exactly_symmetric"] = bool(torch.equal(gram, gram.t()))
        rec["torch_exactly_symmetric"] = bool(torch.equal(answer["G"], answer["G"].t()))
        rec["gram_peak_bytes"], rec["torch_peak_bytes"] = peak(launches["gram"]), peak(launches["torch"])
        rec.update(timed(launches, args.reps, args.warmup, args.burst))
        rec["torch_over_gram"] = rec["torch_us"] / rec["gram_us"]
        rec["fit_forward_gram_ms"], rec["fit_forward_torch_ms"] = whole("gram"), whole("torch")
        res["shapes"].append(rec)
        print(json.dumps(rec))
        del launches, answer, gram, cross, peak, whole, keep
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
