"""HIP-event timings of the dense kernels of --model-type mlp / linear (csrc/dense.hip) and of whole bs = 256 training steps (forward,
backward, Adam on the flat bucket) of the mlp AE, mlp VAE and linear AE at state_dim 200, next to the same models written with stock
torch.nn layers (rocBLAS GEMMs) + torch.optim.Adam in the same process — the reference's own stack on this GPU.

    python tools/kb_dense.py [--steps 20 --warmup 5 --batch-size 256 --out profiles/kb_dense.json]

Per kernel: algorithmic FLOP (n as given) and executed FLOP (n and M padded to the 64-wide tiles), and the fraction of the fp32 MFMA
peak (157.3 TF) each reaches."""
import argparse
import contextlib
import io
import json
import os
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "srl-zoo_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK = 157.3e12


def pad64(v):
    return (v + 63) // 64 * 64


def torch_model(kind, K, S):
    if kind == "mlp_ae":
        enc = nn.Sequential(nn.Linear(K, 50), nn.Tanh(), nn.Linear(50, 50), nn.Tanh(), nn.Linear(50, S))
        dec = nn.Sequential(nn.Linear(S, 50), nn.Tanh(), nn.Linear(50, 50), nn.Tanh(), nn.Linear(50, K))
    elif kind == "linear_ae":
        enc, dec = nn.Linear(K, S), nn.Linear(S, K)
    else:
        enc = None
    if enc is not None:
        m = nn.ModuleDict(dict(enc=enc, dec=dec))

        def step(x):
            s = m["enc"](x)
            d = m["dec"](s)
            h = x.shape[0] // 2
            return ((d[:h] - x[:h]) ** 2).sum() / x[:h].numel() + ((d[h:] - x[h:]) ** 2).sum() / x[h:].numel()
        return m, step
    m = nn.ModuleDict(dict(fc1=nn.Linear(K, 50), fc21=nn.Linear(50, S), fc22=nn.Linear(50, S),
                           dec=nn.Sequential(nn.Linear(S, 50), nn.ReLU(), nn.Linear(50, 50), nn.ReLU(), nn.Linear(50, K))))

    def step(x):
        h = torch.relu(m["fc1"](x))
        mu, logvar = m["fc21"](h), m["fc22"](h)
        z = torch.randn_like(mu) * torch.exp(0.5 * logvar) + mu
        d = m["dec"](z)
        kl = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
        return kl + 0.5e-6 * ((d - x) ** 2).sum()
    return m, step


def time_loop(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--state-dim", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from losses.losses import LossManager
    from models.learner import SRL4robotics
    from srlz import ops
    B, S, K = a.batch_size, a.state_dim, 3 * 224 * 224
    M = 2 * B
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(3)
    frames = torch.randint(0, 256, (M, 3, 224, 224), generator=g, dtype=torch.uint8).to(dev)
    res = {"batch_size": B, "state_dim": S, "K": K, "M": M, "peak_fp32_mfma_tflops": PEAK / 1e12, "models": {}}
    for kind, mt, losses in (("mlp_ae", "mlp", ["autoencoder"]), ("mlp_vae", "mlp", ["vae"]), ("linear_ae", "linear", ["autoencoder"])):
        with contextlib.redirect_stdout(io.StringIO()):
            srl = SRL4robotics(S, model_type=mt, seed=1, learning_rate=1e-4, cuda=True, losses=losses, n_actions=6, log_folder="/tmp")
        o, no = srl._toDevicePair(frames[:B], frames[B:])
        act = torch.zeros((B, 1), dtype=torch.int64, device=dev)
        lm = LossManager(srl.model, None)
        hip_ms = time_loop(lambda: srl.trainStep(o, no, act, lm), a.steps, a.warmup)
        ops.timers_enable(True)
        srl.trainStep(o, no, act, lm)
        rep = ops.timers_report()
        ops.timers_enable(False)
        kernels = {}
        for key, r in rep.items():
            if "/" not in key:
                continue
            what = key.split("/", 1)[1]
            parts = {p[0]: int(p[1:]) for p in what.split() if p[0] in "mnk" and p[1:].isdigit()}
            m_, n_, k_ = int(parts.get("m", 0)), int(parts.get("n", 0)), int(parts.get("k", 0))
            execd = r["flop"] * (pad64(m_) * pad64(n_)) / max(m_ * n_, 1)
            # (one timed call is several kernels: tile + split-K sum; tile + column sum; tile alone; dOut tile + dW tile + dz tile + sum)
            per = {"in_fwd": 2, "in_wgrad": 2, "out_fwd": 1, "out_fwd+loss": 1, "out_bwd": 4}[what.split()[0]]
            kernels[what] = {"ms": r["ms"], "calls": r["launches"], "kernel_launches": r["launches"] * per,
                             "gflop": r["flop"] / 1e9, "executed_gflop": execd / 1e9,
                             "frac": r["flop"] / (r["ms"] * 1e-3) / PEAK, "executed_frac": execd / (r["ms"] * 1e-3) / PEAK}
        del srl, o, no, lm
        torch.cuda.empty_cache()
        torch.manual_seed(1)
        tm, tstep = torch_model(kind, K, S)
        tm = tm.to(dev)
        opt = torch.optim.Adam(tm.parameters(), lr=1e-4)
        x = ops.frames_as_float(frames).view(M, -1)

        def torch_step():
            opt.zero_grad()
            tstep(x).backward()
            opt.step()
        torch_ms = time_loop(torch_step, a.steps, a.warmup)
        del tm, opt, x
        torch.cuda.empty_cache()
        res["models"][kind] = {"hip_step_ms": hip_ms, "torch_nn_step_ms": torch_ms, "speedup_vs_torch": torch_ms / hip_ms,
                               "kernels": kernels}
        print("%-10s HIP step %.3f ms   torch.nn step %.3f ms" % (kind, hip_ms, torch_ms))
        for what, r in sorted(kernels.items()):
            print("    %-40s %8.3f ms  %6.1f GFLOP  frac %.3f  executed %.3f" % (what, r["ms"], r["gflop"], r["frac"], r["executed_frac"]))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
