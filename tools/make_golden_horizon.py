#!/usr/bin/env python
"""Generate tests/golden/horizon_kats.npz and tests/golden/horizon_spread.json by running the UNMODIFIED reference model classes on
the CPU.  The reference is imported from its own files, never copied (found and stubbed as tools/make_golden_deploy.py does).  Runs
where the reference lives only.

Per case of tests/dynamics_util.py::CASES, on the recorded sequence of tests/horizon_util.py::recording (N = 40 frames from closed
formulas, episodes starting at frames 0, 1, 3, 12 and 25, T = 7), one row per frame (rows of every length 0 .. 7): the recorded
actions through the reference's own forwardModel, the imagined pairs through its rewardModel (models/forward_inverse.py:21-31,
78-95), step by step under no_grad, in fp32 and, with the model converted to float64, in fp64.
horizon_kats.npz holds per case err, base [M,T] and logits [M,T,2] in both precisions, the per-horizon sums count, sum_err, sum_base
and hits (fp64), and `decided`: the (row, step) whose fp64 logit gap |l1 - l0| is at least 2e-4 of the logits' scale — the entries a
hit is compared on.  horizon_spread.json holds the reference's own fp32-to-fp64 spread of each quantity (rows per step's scale, sums
as a whole; the tests' bound is dynamics_util.bound: max(1e-4, 10 x that spread)) and the share of valid entries left out; asserted
here: at most 5 % in the cases of horizon_util.HIT_CASES.  Were a case to break that cap, the inputs change, not the cap.

    python tools/make_golden_horizon.py
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
from make_golden_dynamics import MAX_BYTES  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "horizon_kats.npz")
SPREAD = os.path.join(REPO, "tests", "golden", "horizon_spread.json")


def compose(th, model, states, actions, starts, lens, t, dtype):
    """The open-loop rollout by the model's own methods at `dtype` -> trajectory [M,T,S], logits [M,T,2] (numpy); past a row's
    steps action 0 is taken and the entries mean nothing."""
    x = th.from_numpy(states).to(dtype)
    acts = th.from_numpy(actions.astype(np.int64))
    st, ln = th.from_numpy(starts.astype(np.int64)), th.from_numpy(lens.astype(np.int64))
    n = x.shape[0]
    cur = x[st]
    traj, logits = [], []
    with th.no_grad():
        for step in range(t):
            a = th.where(ln > step, acts[th.clamp(st + step, max=n - 1)], th.zeros_like(st))
            nxt = model.forwardModel(cur, a.view(-1, 1))
            logits.append(model.rewardModel(cur, nxt))
            traj.append(nxt)
            cur = nxt
    return th.stack(traj, 1).numpy(), th.stack(logits, 1).numpy()


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # single-threaded: deterministic summation order
    import dynamics_util as dy
    import horizon_util as hu
    import models.modules as ref_modules  # the reference's
    assert os.path.abspath(ref_modules.__file__).startswith(os.path.abspath(REF)), ref_modules.__file__
    merged, spreads = {}, {}
    t = hu.HORIZON
    for name in dy.CASES:
        s = dy.CASES[name]["state_dim"]
        model = dy.build_case(name, ref_modules)
        model.eval()
        states, actions, rewards, es = hu.recording(s)
        labels = hu.labels_of(rewards)
        assert set(labels.tolist()) == {0, 1} and (rewards < 0).any()
        starts = np.arange(hu.N_FRAMES)
        lens = hu.valid_steps(es, t)
        assert sorted(set(lens.tolist())) == list(range(t + 1)), lens
        mask = hu.valid_mask(lens, t)
        tr32, lg32 = compose(th, model, states, actions, starts, lens, t, th.float32)
        tr64, lg64 = compose(th, model.double(), states, actions, starts, lens, t, th.float64)
        e32, b32 = hu.rows_from_trajectory(tr32, states, starts, lens, np.float32)
        e64, b64 = hu.rows_from_trajectory(tr64, states, starts, lens, np.float64)
        c32, se32, sb32, _ = hu.totals(e32, b32, lens, lg32, labels, starts)
        c64, se64, sb64, h64 = hu.totals(e64, b64, lens, lg64, labels, starts)
        dec = hu.decided(lg64, mask)
        left_out = 1.0 - dec.sum() / float(mask.sum())
        if name in hu.HIT_CASES:
            assert left_out <= hu.GAP_CAP, (name, left_out)  # else: change the inputs, not the cap
        for key, lo, hi in (("err", e32, e64), ("base", b32, b64), ("logits", lg32, lg64)):
            merged["%s/%s32" % (name, key)], merged["%s/%s64" % (name, key)] = lo.astype(np.float32), hi.astype(np.float64)
        merged[name + "/count"], merged[name + "/sum_err"], merged[name + "/sum_base"], merged[name + "/hits"] = c64, se64, sb64, h64
        merged[name + "/decided"] = dec
        merged[name + "/checksums"] = dy.checksums(model.float().state_dict())
        spreads[name] = {"err": hu.step_rel_err(e32, e64, mask), "base": hu.step_rel_err(b32, b64, mask),
                         "logits": hu.step_rel_err(lg32, lg64, mask), "sum_err": hu.vec_rel_err(se32, se64),
                         "sum_base": hu.vec_rel_err(sb32, sb64), "left_out": float(left_out),
                         "hits_checked": name in hu.HIT_CASES, "valid": int(mask.sum())}
        print("%-16s S = %3d  %s" % (name, s, {q: ("%.2e" % v if isinstance(v, float) else v) for q, v in sorted(spreads[name].items())}))
    merged["horizon"], merged["n_frames"] = np.int64(t), np.int64(hu.N_FRAMES)
    np.savez_compressed(GOLDEN, **merged)
    with open(SPREAD, "w") as f:
        json.dump({"what": "max |fp32 - fp64| over the quantity's scale (err, base and logits per step, the sums as a whole) of the "
                           "k-step error on the unmodified reference's forwardModel / rewardModel on the CPU; left_out: the share of "
                           "valid (row, step) whose fp64 logit gap is below gap x the logits' scale (not compared for hits; at most "
                           "gap_cap where hits_checked)",
                   "gap": hu.GAP, "gap_cap": hu.GAP_CAP, "horizon": t, "n_frames": hu.N_FRAMES, "cases": spreads}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    for p in (GOLDEN, SPREAD):
        assert os.path.getsize(p) < MAX_BYTES, (p, os.path.getsize(p))
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
