#!/usr/bin/env python
"""Cost of the exact fp64 k-nearest-neighbour search (csrc/knn.hip) on one GPU: python tools/kb_knn.py [--out profiles/kb_knn.json]

Per shape (N, D, Q), K = 6 (the evaluation's 5 neighbours + the row itself):
  * the three kernels of srlz_knn_f64 on resident buffers, HIP events over warmed-up repetitions, every timed window at least
    --window seconds long;
  * the fp64 operations the shapes imply — 3 Q N D: a subtraction, a multiplication and an addition per pair and dimension, issued
    as one v_add_f64 and one v_fma_f64 — and the rate they give over the kernel time;
  * ops.knn as a user calls it (host arrays in, host arrays out) and its upload and download alone;
  * the reference's own route, NearestNeighbors(n_neighbors=6, algorithm='ball_tree').fit(s).kneighbors(s) over all N, as wall
    seconds on the host (with the reference's default of one thread, and with every core the job may use) — where sklearn imports
    and N <= --ref-max-n (the time grows with N^2 at D = 200; beyond it null is recorded, not an estimate).
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))

SHAPES = [(20000, 3, 200), (20000, 200, 200), (100000, 200, 200), (20000, 200, 20000)]
K = 6


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_knn.json"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--ref-max-n", type=int, default=20000, help="largest N the reference's ball tree is timed at")
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_knn measures on a GPU"
    from srlz import _cabi as C, ops
    dev = torch.device("cuda", 0)
    res = {"K": K, "device": torch.cuda.get_device_name(0), "window_s": args.window, "shapes": []}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for n, d, q in SHAPES:
        s = np.random.RandomState(0).randn(n, d).astype(np.float32)
        queries = s if q == n else s[np.random.RandomState(1).permutation(n)[:q]]
        db_d = torch.from_numpy(s.astype(np.float64)).to(dev)
        q_d = db_d if q == n else torch.from_numpy(queries.astype(np.float64)).to(dev)
        idx = torch.empty((q, K), dtype=torch.int32, device=dev)
        dist2 = torch.empty((q, K), dtype=torch.float64, device=dev)
        nbytes = C.knn_workspace(n, q, d, K)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def kernels():
            C.knn_f64(C.ptr(db_d), n, C.ptr(q_d), q, d, K, C.ptr(idx), C.ptr(dist2), C.ptr(ws), nbytes, C.stream())
        ms, reps = timed_window(kernels, args.window)
        flop = 3.0 * q * n * d
        s64 = s.astype(np.float64)
        q64 = queries.astype(np.float64)
        up = host_timed(lambda: (torch.from_numpy(s64).to(dev), None if q == n else torch.from_numpy(q64).to(dev)))
        down = host_timed(lambda: (idx.cpu(), dist2.cpu()))
        whole = host_timed(lambda: ops.knn(s, K, queries=None if q == n else queries), reps=3)
        rec = {"N": n, "D": d, "Q": q, "kernel_ms": ms, "reps": reps, "window_ms": ms * reps, "fp64_ops": flop,
               "fp64_tflops": flop / (ms * 1e-3) / 1e12, "workspace_bytes": int(nbytes), "upload_ms": up, "download_ms": down,
               "ops_knn_host_to_host_ms": whole, "ref_ball_tree_s": None, "ref_ball_tree_all_cores_s": None}
        res["shapes"].append(rec)
        print(json.dumps(rec))
        save()
        del db_d, q_d, ws

    if not args.no_ref:
        try:
            from sklearn.neighbors import NearestNeighbors
            import sklearn
            res["sklearn"] = sklearn.__version__
        except ImportError:
            NearestNeighbors = None
            res["sklearn"] = None
        done = {}
        for rec in res["shapes"]:
            n, d = rec["N"], rec["D"]
            if NearestNeighbors is None:
                continue
            if n > args.ref_max_n:
                rec["ref_note"] = "not run: N above --ref-max-n %d" % args.ref_max_n
                continue
            if (n, d) not in done:  # (the reference searches all N rows whatever Q is)
                s = np.random.RandomState(0).randn(n, d).astype(np.float32)
                out = []
                for jobs in (None, int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()):
                    t = time.perf_counter()
                    NearestNeighbors(n_neighbors=K, algorithm='ball_tree', n_jobs=jobs).fit(s).kneighbors(s)
                    out.append(time.perf_counter() - t)
                done[(n, d)] = out
            rec["ref_ball_tree_s"], rec["ref_ball_tree_all_cores_s"] = done[(n, d)]
            print(json.dumps({"N": n, "D": d, "ref_ball_tree_s": done[(n, d)]}))
            save()
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
