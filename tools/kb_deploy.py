#!/usr/bin/env python
"""What a getStates call of the deployment encoder costs on one GPU: python tools/kb_deploy.py [--out profiles/kb_deploy.json]

For N in {1, 4, 16, 32} frames of 224 x 224 x 3 and the two routes of srlz.deploy.StateEncoder — "blocks" (csrc/infer.hip: one launch
per encoder block + the state head) and "model" (the model's own getStates in eval mode, the code of the route before the encoder
existed) — on the same CNN auto-encoder:
  * kernel_ms: HIP events around --burst back-to-back calls on frames that are already on the device (the device's time per call);
  * call_ms: host clock from uint8 host frames in to the states on the host, one synchronisation (enc.numpy).
Both routes run interleaved in one process, call by call, after a warm-up; the figures are medians over --reps repetitions.
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
sys.path.insert(0, REPO)

BATCHES = (1, 4, 16, 32)


def frames_nhwc(n, h=224, w=224, c=3):
    i, y, x, ch = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((y * 3 + x * 5 + ch * 41 + i * 67 + ((y * x + 7 * i + 13 * ch) % 29) * 4) % 256).astype(np.uint8)


def kernel_ms(enc, dev_frames, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        enc(dev_frames)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst


def call_ms(enc, host_frames):
    t0 = time.perf_counter()
    enc.numpy(host_frames)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_deploy.json"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burst", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_deploy measures on a GPU"
    import bench
    from models.modules import SRLModules
    from srlz import deploy
    torch.manual_seed(1)
    model = SRLModules(state_dim=8, action_dim=6, cuda=True, model_type="custom_cnn", losses=["autoencoder"]).to(torch.device("cuda", 0))
    model.eval()
    encs = {"blocks": deploy.StateEncoder(model, max_batch=max(BATCHES)), "model": deploy.StateEncoder(model, route="model")}
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "frame": [224, 224, 3], "model": "custom_cnn autoencoder S=8", "batches": []}
    for n in BATCHES:
        host = frames_nhwc(n)
        dev = torch.from_numpy(host).cuda()
        for _ in range(args.warmup):
            for enc in encs.values():
                enc.numpy(host)
                enc(dev)
        torch.cuda.synchronize()
        t = {r: {"kernel_ms": [], "call_ms": []} for r in encs}
        for _ in range(args.reps):
            for r, enc in encs.items():  # interleaved: a drift of the machine falls on both routes alike
                t[r]["call_ms"].append(call_ms(enc, host))
            for r, enc in encs.items():
                t[r]["kernel_ms"].append(kernel_ms(enc, dev, args.burst))
        assert encs["blocks"].route == "blocks" and encs["model"].route == "model"
        rec = {"n": n}
        for r in encs:
            for k in ("kernel_ms", "call_ms"):
                rec["%s_%s" % (r, k)] = float(np.median(t[r][k]))
                rec["%s_%s_min" % (r, k)] = float(np.min(t[r][k]))
        rec["call_speedup"] = rec["model_call_ms"] / rec["blocks_call_ms"]
        rec["kernel_speedup"] = rec["model_kernel_ms"] / rec["blocks_kernel_ms"]
        rec["blocks_faster_in_call_latency"] = bool(rec["blocks_call_ms"] < rec["model_call_ms"])
        res["batches"].append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
