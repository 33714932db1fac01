#!/usr/bin/env python
"""Generate tests/golden/dynamics_kats.npz and tests/golden/dynamics_spread.json by running the UNMODIFIED reference model classes on
the CPU.  The reference is imported from its own files, never copied (found and stubbed as tools/make_golden_deploy.py does).  Runs
where the reference lives only.

Per case of tests/dynamics_util.py::CASES (seeded SRLModules with losses forward inverse reward: S = 3 with a linear inverse head,
S = 8 with inverse_model_type="mlp", S = 200, and S = 200 with forward_net.weight x 20 — an expanding recurrence):
  * the head parameters' checksums are stored, not the weights;
  * N = 3 states from the sine formula dynamics_util.sine_states and N x K x T = 3 x 4 x 7 plans from the integer formula
    dynamics_util.plans (nothing is stored);
  * the composition a rollout is defined as — forwardModel, then rewardModel on (state, next state), the return the sum of
    gamma^t softmax(logits)[1] with gamma = 0.9 — by the reference's own methods (models/forward_inverse.py:21-31, 78-95) under no_grad,
    in fp32 and, with the model converted to float64, in fp64.
dynamics_kats.npz holds the trajectories, logits and returns (both precisions) and the checksums; dynamics_spread.json the reference's
own fp32-to-fp64 spread per case and quantity (trajectory and logits per step's scale) — the tests' bound is max(1e-4, 10 x that
spread) of each quantity's scale.

    python tools/make_golden_dynamics.py
"""
from __future__ import print_function
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_golden_deploy import REF, _stub_modules  # noqa: E402  (where the reference lives, and the modules it lacks here)

GOLDEN = os.path.join(REPO, "tests", "golden", "dynamics_kats.npz")
SPREAD = os.path.join(REPO, "tests", "golden", "dynamics_spread.json")
GAMMA = 0.9
MAX_BYTES = 605060  # the largest fixture of tests/golden: these stay far below it


def compose(th, model, z, plans, gamma, dtype):
    """The rollout by the model's own methods at `dtype`: z [N,S], plans [N,K,T] -> trajectory, reward_logits, returns (numpy)."""
    n, s = z.shape
    _, k, t = plans.shape
    cur = th.from_numpy(z).to(dtype).unsqueeze(1).expand(n, k, s).reshape(n * k, s)
    acts = th.from_numpy(plans.astype(np.int64)).reshape(n * k, t)
    traj, logits = [], []
    ret, g = th.zeros(n * k, dtype=dtype), th.ones((), dtype=dtype)
    gam = th.tensor(gamma, dtype=th.float32).to(dtype)  # gamma as the float the kernel takes
    with th.no_grad():
        for step in range(t):
            nxt = model.forwardModel(cur, acts[:, step:step + 1])
            lg = model.rewardModel(cur, nxt)
            ret = ret + g * th.softmax(lg, dim=1)[:, 1]
            g = g * gam
            traj.append(nxt)
            logits.append(lg)
            cur = nxt
    return {"trajectory": th.stack(traj, 1).reshape(n, k, t, s).numpy(), "reward_logits": th.stack(logits, 1).reshape(n, k, t, 2).numpy(),
            "returns": ret.reshape(n, k).numpy()}


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # single-threaded: deterministic summation order
    import dynamics_util as dy
    import models.modules as ref_modules  # the reference's
    assert os.path.abspath(ref_modules.__file__).startswith(os.path.abspath(REF)), ref_modules.__file__
    merged, spreads = {}, {}
    for name in dy.CASES:
        model = dy.build_case(name, ref_modules)
        model.eval()
        merged[name + "/checksums"] = dy.checksums(model.state_dict())
        z, plans = dy.case_inputs(name)
        lo = compose(th, model, z, plans, GAMMA, th.float32)
        hi = compose(th, model.double(), z, plans, GAMMA, th.float64)
        spreads[name] = {}
        for q in dy.QUANTITIES:
            merged["%s/%s32" % (name, q)] = lo[q].astype(np.float32)
            merged["%s/%s64" % (name, q)] = hi[q].astype(np.float64)
            spreads[name][q] = dy.rel_err(lo[q], hi[q], q != "returns")
        spreads[name]["last_step_scale"] = float(np.abs(hi["trajectory"][:, :, -1]).max())
        print("%-16s S = %3d  spread %s  scale of the last step %.3g" % (name, dy.CASES[name]["state_dim"], {
            q: "%.2e" % spreads[name][q] for q in dy.QUANTITIES}, spreads[name]["last_step_scale"]))
    merged["gamma"] = np.float64(GAMMA)
    np.savez_compressed(GOLDEN, **merged)
    with open(SPREAD, "w") as f:
        json.dump({"what": "max |fp32 - fp64| over the quantity's scale (trajectory and reward_logits per step, returns as a whole) of "
                           "the unmodified reference's forwardModel / rewardModel composition on the CPU",
                   "gamma": GAMMA, "cases": spreads}, f, indent=1, sort_keys=True)
        f.write("\n")
    for p in (GOLDEN, SPREAD):
        assert os.path.getsize(p) < MAX_BYTES, (p, os.path.getsize(p))
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
