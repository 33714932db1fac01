#!/usr/bin/env python
"""Cost of the reward-prior and episode-prior losses on one GPU: python tools/kb_priors.py [--out profiles/kb_priors.json]

  * each kernel pair (forward + backward) at B = 256, S = 200, timed with HIP events over many repetitions;
  * the same two losses composed from stock torch ops on the same states (for comparison only: the product never runs them);
  * the bs = 256 auto-encoder training step (SRL4robotics.trainStep) with and without both losses.
Prints one JSON object and writes it to --out."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_priors.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    from srlz import ops
    from models.priors import Discriminator
    B, S = 256, 200
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    states = torch.from_numpy(rng.randn(B, S).astype(np.float32)).to(dev).requires_grad_(True)
    rewards = torch.from_numpy(rng.randint(-1, 2, B).astype(np.float32)).to(dev)
    ids = np.sort(rng.randint(0, 20, B))
    others = rng.permutation(B)
    o = torch.from_numpy(others.astype(np.int32)).to(dev)
    y = torch.from_numpy((ids == ids[others]).astype(np.float32)).to(dev)
    disc = Discriminator(2 * S).to(dev)
    res = {"B": B, "S": S}

    def rp():
        ops.RewardPriorFn.apply(states, rewards).backward()

    def ep():
        ops.EpisodePriorFn.apply(states, o, y, *disc.params()).backward()

    def rp_torch():
        x = torch.cat([states, rewards.view(-1, 1)], 1).t()
        xc = x - x.mean(1, keepdim=True)
        cov = xc.mm(xc.t()) / (B - 1)
        inv = torch.rsqrt(torch.diag(cov) + 1e-8)
        corr = (cov * inv.expand_as(cov) * inv.expand_as(cov).t()).clamp(-1, 1)
        (1 - corr[-1:].abs().mean()).backward()

    oi = torch.from_numpy(others).to(dev)

    def ep_torch():
        x = torch.cat([states, states[oi]], 1)
        p = torch.sigmoid(disc.net[4](torch.relu(disc.net[2](torch.relu(disc.net[0](x))))))
        torch.nn.functional.binary_cross_entropy(p.squeeze(1), y, reduction="sum").backward()

    res["reward_prior_fwd_bwd_ms"] = timed(rp, args.reps)
    res["episode_prior_fwd_bwd_ms"] = timed(ep, args.reps)
    res["torch_reward_prior_fwd_bwd_ms"] = timed(rp_torch, args.reps)
    res["torch_episode_prior_fwd_bwd_ms"] = timed(ep_torch, args.reps)

    import preprocessing.preprocess as pre
    import golden_util as gu
    from models.learner import SRL4robotics
    from losses.losses import LossManager, episodeInputs
    pre.N_CHANNELS = 3
    for tag, losses in (("ae", ["autoencoder"]), ("ae_rp_ep", ["autoencoder", "reward-prior", "episode-prior"])):
        with contextlib.redirect_stdout(io.StringIO()):
            srl = SRL4robotics(S, model_type="custom_cnn", seed=1, learning_rate=1e-4, cuda=True, losses=losses, n_actions=6,
                               log_folder="/tmp")
        obs_np, next_np, actions = gu.golden_inputs(B, 3, 6, seed=1234)
        o8 = torch.from_numpy(np.clip(obs_np * 60 + 128, 0, 255).astype(np.uint8)).to(dev)
        n8 = torch.from_numpy(np.clip(next_np * 60 + 128, 0, 255).astype(np.uint8)).to(dev)
        act = torch.from_numpy(actions).view(-1, 1).to(dev)
        kw = {}
        if "reward-prior" in losses:
            kw = dict(reward_prior_st=rewards)
            kw["episode_others"], kw["episode_same"] = episodeInputs(others, (ids == ids[others]).astype(np.float32), srl.device)

        def step():
            a, b = srl._toDevicePair(o8, n8)
            srl.trainStep(a, b, act, LossManager(srl.model, None), **kw)
        res["step_%s_ms" % tag] = timed(step, args.steps, warm=3)
    res["priors_added_ms"] = res["step_ae_rp_ep_ms"] - res["step_ae_ms"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
