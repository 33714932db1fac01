#!/usr/bin/env python
"""Generate tests/golden/goal_kats.npz and tests/golden/goal_spread.json by running the UNMODIFIED reference model classes on the CPU.
The reference is imported from its own files, never copied (found and stubbed as tools/make_golden_deploy.py does).  Runs where the
reference lives only.

Per case of tests/dynamics_util.py::CASES, with the states and plans of goal_util.case_inputs (dynamics_util.case_inputs with the
plans made pairwise different) rolled by the reference's own
forwardModel / rewardModel (tools/make_golden_dynamics.py::compose, models/forward_inverse.py:21-31, 78-95) in fp32 and fp64:
  * goal[n] = fp32(trajectory64[n, k* = 2, T-1]): a state the reference itself reaches;
  * goal_dist [N,K,T] = |s_{t+1} - goal|^2 from the fp32 trajectory in fp32 and from the fp64 trajectory in fp64;
  * the scores of include/srlz.h with gamma = 0.9, w = 0.5, both modes, with the head's probabilities and without (tests/goal_util.py).
goal_kats.npz holds the goals, both goal_dist and all scores; goal_spread.json the reference's own fp32-to-fp64 spread per case and
quantity (goal_dist per step's scale, each score as a whole) — the tests' bound is dynamics_util.bound: max(1e-4, 10 x that spread) —
and, checked here, that plan k* is the unique argmin of the final distance in every environment, and the argmax of the score act()
ranks by (gamma = 1, final mode, with the head, weight goal_util.ACT_WEIGHT), with the margins and that each exceeds twice the bound
(asserted for every case: an answer within the bound then cannot change either argmin).

    python tools/make_golden_goal.py
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
from make_golden_dynamics import compose, MAX_BYTES  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "goal_kats.npz")
SPREAD = os.path.join(REPO, "tests", "golden", "goal_spread.json")


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # single-threaded: deterministic summation order
    import dynamics_util as dy
    import goal_util as gu
    import models.modules as ref_modules  # the reference's
    assert os.path.abspath(ref_modules.__file__).startswith(os.path.abspath(REF)), ref_modules.__file__
    merged, spreads = {}, {}
    for name in dy.CASES:
        model = dy.build_case(name, ref_modules)
        model.eval()
        z, plans = gu.case_inputs(name)  # (dynamics_util's states; its plans made pairwise different)
        lo = compose(th, model, z, plans, gu.GAMMA, th.float32)
        hi = compose(th, model.double(), z, plans, gu.GAMMA, th.float64)
        goal = gu.goals_of(hi["trajectory"])
        d32, d64 = gu.dist(lo["trajectory"], goal, np.float32), gu.dist(hi["trajectory"], goal, np.float64)
        p32, p64 = gu.probs(lo["reward_logits"], np.float32), gu.probs(hi["reward_logits"], np.float64)
        s32, s64 = gu.all_scores(d32, p32, np.float32), gu.all_scores(d64, p64, np.float64)
        merged[name + "/goal"] = goal
        merged[name + "/goal_dist32"], merged[name + "/goal_dist64"] = d32, d64
        sp = {"goal_dist": dy.rel_err(d32[..., None], d64[..., None], True)}
        for key in gu.SCORE_KEYS:
            merged["%s/%s32" % (name, key)], merged["%s/%s64" % (name, key)] = s32[key], s64[key]
            sp[key] = dy.rel_err(s32[key], s64[key], False)
        # the condition: k* is the unique argmin of the final distance, by more than twice the bound of the last step's scale
        last = d64[:, :, -1]
        others = np.delete(last, gu.KSTAR, axis=1)
        margin = float(((others.min(axis=1) - last[:, gu.KSTAR]) / last.max()).min())
        assert (last.argmin(axis=1) == gu.KSTAR).all() and margin > 0, (name, margin)
        sp["final_margin"], sp["final_margin_exceeds_bound"] = margin, bool(margin > 2 * dy.bound(sp["goal_dist"]))
        # ... and the argmax of the score act() ranks by
        a32 = gu.scores(d32, p32, 1.0, gu.ACT_WEIGHT, "final", np.float32)
        a64 = gu.scores(d64, p64, 1.0, gu.ACT_WEIGHT, "final", np.float64)
        merged[name + "/act_score64"] = a64
        sp["act_score"] = dy.rel_err(a32, a64, False)
        a_others = np.delete(a64, gu.KSTAR, axis=1)
        a_margin = float(((a64[:, gu.KSTAR] - a_others.max(axis=1)) / np.abs(a64).max()).min())
        assert (a64.argmax(axis=1) == gu.KSTAR).all() and a_margin > 0, (name, a_margin)
        sp["act_margin"], sp["act_margin_exceeds_bound"] = a_margin, bool(a_margin > 2 * dy.bound(sp["act_score"]))
        assert sp["final_margin_exceeds_bound"] and sp["act_margin_exceeds_bound"], (name, sp)  # in every case: else pick another k*
        spreads[name] = sp
        print("%-16s S = %3d  %s" % (name, dy.CASES[name]["state_dim"], {q: "%.2e" % v for q, v in sorted(sp.items())}))
    merged["gamma"], merged["weight"], merged["kstar"] = np.float64(gu.GAMMA), np.float64(gu.WEIGHT), np.int64(gu.KSTAR)
    np.savez_compressed(GOLDEN, **merged)
    with open(SPREAD, "w") as f:
        json.dump({"what": "max |fp32 - fp64| over the quantity's scale (goal_dist per step, each score as a whole) of the goal term on "
                           "the unmodified reference's forwardModel / rewardModel composition on the CPU; final_margin: how far plan "
                           "k* leads the final distance's argmin, of the last step's scale (checked > 2 x the bound); act_margin: the "
                           "same for the score act() ranks by (gamma 1, final mode, head, act_weight)",
                   "gamma": gu.GAMMA, "weight": gu.WEIGHT, "kstar": gu.KSTAR, "act_weight": gu.ACT_WEIGHT, "cases": spreads}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    for p in (GOLDEN, SPREAD):
        assert os.path.getsize(p) < MAX_BYTES, (p, os.path.getsize(p))
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
