#!/usr/bin/env python
"""What a decode call of the deployment decoder costs on one GPU: python tools/kb_decode.py [--out profiles/kb_decode.json]

For N in {1, 4, 16, 32} states of a custom_cnn auto-encoder (S = 8, 224 x 224 x 3 frames) and the two routes of
srlz.deploy.FrameDecoder — "blocks" (csrc/infer_dec.hip: decoder_fc + one launch per decoder layer, bytes from the last kernel) and
"model" (the model's own decode in eval mode and the byte expression on its tensor: the code of the route before the decoder existed):
  * kernel_ms: HIP events around --burst back-to-back calls on states that are already on the device (the device's time per call);
  * call_ms: host clock from fp32 host states in to the uint8 frames on the host, one synchronisation (dec.numpy).
Both routes run interleaved in one process, call by call, after a warm-up; the figures are medians and interquartile ranges over --reps
repetitions.  "blocks" counts as faster at an N when its median call latency is lower by more than the two routes' interquartile
ranges together; the default max_batch is the largest measured N at which it still is.
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
STATE_DIM = 8


def states(n, s=STATE_DIM):
    i, j = np.meshgrid(np.arange(n), np.arange(s), indexing="ij")
    return (0.5 * (((5 * i + 3 * j) % 7) - 3)).astype(np.float32)


def kernel_ms(dec, dev_states, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        dec(dev_states)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / burst


def call_ms(dec, host_states):
    t0 = time.perf_counter()
    dec.numpy(host_states)
    return (time.perf_counter() - t0) * 1e3


def iqr(v):
    q1, q3 = np.percentile(v, [25, 75])
    return float(q3 - q1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_decode.json"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burst", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_decode measures on a GPU"
    import bench
    from models.modules import SRLModules
    from srlz import deploy
    torch.manual_seed(1)
    model = SRLModules(state_dim=STATE_DIM, action_dim=6, cuda=True, model_type="custom_cnn",
                       losses=["autoencoder"]).to(torch.device("cuda", 0))
    model.eval()
    decs = {"blocks": deploy.FrameDecoder(model, max_batch=max(BATCHES)), "model": deploy.FrameDecoder(model, route="model")}
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": bench.csrc_sha16(), "reps": args.reps, "warmup": args.warmup,
           "burst": args.burst, "frame": [224, 224, 3], "model": "custom_cnn autoencoder S=8", "batches": []}
    for n in BATCHES:
        host = states(n)
        dev = torch.from_numpy(host).cuda()
        for _ in range(args.warmup):
            for dec in decs.values():
                dec.numpy(host)
                dec(dev)
        torch.cuda.synchronize()
        t = {r: {"kernel_ms": [], "call_ms": []} for r in decs}
        for _ in range(args.reps):
            for r, dec in decs.items():  # interleaved: a drift of the machine falls on both routes alike
                t[r]["call_ms"].append(call_ms(dec, host))
            for r, dec in decs.items():
                t[r]["kernel_ms"].append(kernel_ms(dec, dev, args.burst))
        assert decs["blocks"].route == "blocks" and decs["model"].route == "model"
        rec = {"n": n}
        for r in decs:
            for k in ("kernel_ms", "call_ms"):
                rec["%s_%s" % (r, k)] = float(np.median(t[r][k]))
                rec["%s_%s_iqr" % (r, k)] = iqr(t[r][k])
                rec["%s_%s_min" % (r, k)] = float(np.min(t[r][k]))
        rec["call_speedup"] = rec["model_call_ms"] / rec["blocks_call_ms"]
        rec["kernel_speedup"] = rec["model_kernel_ms"] / rec["blocks_kernel_ms"]
        rec["blocks_faster_in_call_latency"] = bool(rec["model_call_ms"] - rec["blocks_call_ms"]
                                                    > rec["model_call_ms_iqr"] + rec["blocks_call_ms_iqr"])
        res["batches"].append(rec)
        print(json.dumps(rec))
    wins = [b["n"] for b in res["batches"] if b["blocks_faster_in_call_latency"]]
    res["blocks_meets_its_purpose_at_n1"] = bool(res["batches"][0]["blocks_faster_in_call_latency"])
    res["largest_n_blocks_wins"] = max(wins) if wins else None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
