#!/usr/bin/env python
"""Cost of the fp64 ground-truth correlation (csrc/gtc.hip) on one GPU: python tools/kb_gtc.py [--out profiles/kb_gtc.json]

Per shape (N, S), G = 3 (the agent's position, or the target's):
  * the five launches of srlz_gtc_rows_f64 on resident buffers, HIP events over warmed-up repetitions, every timed window at least
    --window seconds long;
  * the bytes the shape implies — N (G + S) fp64 values, read once per pass, two passes (means, then centred products) — and the
    rates they give over the kernel time: `read_once_gbps` counts the matrix once (the floor a one-read design would be held to),
    `two_pass_gbps` counts what the two passes actually request;
  * ops.gt_correlation as a user calls it (host arrays in, host array out) and its upload alone;
  * the reference's own route, np.corrcoef(gt, states, rowvar=0) over all (G + S)^2 pairs, as wall seconds on the host.
Prints one JSON object and writes it to --out.  The numbers are for the record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))

SHAPES = [(20000, 3), (20000, 200), (200000, 200)]
G = 3


def timed_window(fn, window_s, warm=3):
    """Milliseconds per call over a window of at least window_s seconds (HIP events around the whole window)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(5, int(np.ceil(window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def host_timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_gtc.json"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_gtc measures on a GPU"
    from srlz import _cabi as C, ops
    dev = torch.device("cuda", 0)
    res = {"G": G, "device": torch.cuda.get_device_name(0), "window_s": args.window, "numpy": np.__version__, "shapes": []}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for n, s in SHAPES:
        rs = np.random.RandomState(0)
        gt = rs.rand(n, G)
        states = (gt.dot(rs.randn(G, s)) + rs.randn(n, s)).astype(np.float32)
        gt_d = torch.from_numpy(gt).to(dev)
        st_d = torch.from_numpy(states.astype(np.float64)).to(dev)
        corr = torch.empty((G, G + s), dtype=torch.float64, device=dev)
        colstats = torch.empty((2, G + s), dtype=torch.float64, device=dev)
        nbytes = C.gtc_workspace(n, G, s)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def kernels():
            C.gtc_rows_f64(C.ptr(gt_d), C.ptr(st_d), n, G, s, C.ptr(corr), C.ptr(colstats), C.ptr(ws), nbytes, C.stream())
        ms, reps = timed_window(kernels, args.window)
        matrix_bytes = 8.0 * n * (G + s)
        s64 = states.astype(np.float64)
        up = host_timed(lambda: (torch.from_numpy(gt).to(dev), torch.from_numpy(s64).to(dev)))
        whole = host_timed(lambda: ops.gt_correlation(gt, states), reps=3)
        rec = {"N": n, "G": G, "S": s, "kernel_ms": ms, "reps": reps, "window_ms": ms * reps, "matrix_bytes": matrix_bytes,
               "read_once_gbps": matrix_bytes / (ms * 1e-3) / 1e9, "two_pass_gbps": 2 * matrix_bytes / (ms * 1e-3) / 1e9,
               "workspace_bytes": int(nbytes), "upload_ms": up, "ops_gt_correlation_host_to_host_ms": whole, "ref_corrcoef_s": None}
        if not args.no_ref:
            t = time.perf_counter()
            ref = np.corrcoef(gt, states, rowvar=0)[:G]
            rec["ref_corrcoef_s"] = time.perf_counter() - t
            rec["max_abs_diff_to_ref"] = float(np.abs(corr.cpu().numpy() - ref).max())
        res["shapes"].append(rec)
        print(json.dumps(rec))
        save()
        del gt_d, st_d, ws
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
