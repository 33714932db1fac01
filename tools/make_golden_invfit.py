#!/usr/bin/env python
"""Generate tests/golden/invfit_kats.npz and invfit_spread.json by running the UNMODIFIED reference on the CPU.

The reference's BaseInverseModel (its initInverseNet and inverseModel) and inverseModelLoss are imported, never copied (the
reference's location and the stubs of its absent third-party modules are tools/make_golden.py's), and trained with torch.optim.Adam
in float32, single-threaded, over the recordings, splits and minibatch tables of tests/invfit_util.py — the inverse part of the
learner's loop without its encoder.  The fixture is DATA only: initial parameters, the tables, per-epoch train / val losses and
counts, the final parameters as sums and abs-sums, the trained logits of the first validation batch.  The spread file holds the
reference's own float32-to-float64 distance per quantity, against the float64 restatement of tests/invfit_util.py from the same
initial parameters over the same tables.

While generating, the float64 run must leave at most 1 % of every phase's rows with a gap between their two largest logits below
1e-4 * max|z| (the cap of tests/test_invfit_fit_gpu.py): change the case's seed in tests/invfit_util.py until it does.

    python tools/make_golden_invfit.py
"""
from __future__ import print_function
import json
import os
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import make_golden as mg  # noqa: E402  (puts tests/ on the path)

import golden_util  # noqa: E402
import invfit_util as iu  # noqa: E402
import reward_util as ru  # noqa: E402


def reference_run(th, case):
    from models.forward_inverse import BaseInverseModel
    from losses.losses import LossManager, inverseModelLoss
    S, A, lr = case["S"], case["A"], case["lr"]
    states, actions, _ = iu.case_recording(case)
    assert states.shape[1] == S and actions.max() == A - 1
    train, val, tables, vtabs = iu.case_tables(case)
    th.manual_seed(case["seed"])
    head = BaseInverseModel()
    head.initInverseNet(S, A)
    net = head.inverse_net
    init = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    assert tuple(init.keys()) == iu.KEYS
    opt = th.optim.Adam(net.parameters(), lr=lr)
    lm = LossManager(net)
    x, y = th.from_numpy(states), th.from_numpy(actions)
    epochs = case["epochs"]
    loss, counts = np.zeros((epochs, 2)), np.zeros((epochs, 2, iu.n_counts(A)), np.int64)

    def batch(idx):
        i = th.from_numpy(np.asarray(idx, np.int64))
        lm.resetLosses()
        pred = head.inverseModel(x[i], x[i + 1])
        return pred, inverseModelLoss(pred, y[i].unsqueeze(1), 1.0, lm), y[i]

    for e in range(epochs):
        run = 0.0
        for idx in tables[e]:
            opt.zero_grad()
            pred, l, yy = batch(idx)
            l.backward()
            opt.step()
            run += l.item() * len(idx)
            counts[e, 0] += iu.count(pred.detach().double().numpy(), yy.numpy())
        loss[e, 0] = run / tables[e].size
        run = 0.0
        with th.no_grad():
            for table in vtabs:
                for idx in table:
                    pred, l, yy = batch(idx)
                    run += l.item() * len(idx)
                    counts[e, 1] += iu.count(pred.double().numpy(), yy.numpy())
        loss[e, 1] = run / len(val)
    rec = {"init/" + k: init[k] for k in iu.KEYS}
    final = [net.state_dict()[k].detach().double() for k in iu.KEYS]
    rec["final/names"] = np.array(iu.KEYS)
    rec["final/sums"] = np.array([float(t.sum()) for t in final])
    rec["final/abss"] = np.array([float(t.abs().sum()) for t in final])
    idx = vtabs[0][0]
    with th.no_grad():
        rec["eval_states/full"] = batch(idx)[0].double().numpy()
    rec["eval_states/idx"] = np.asarray(idx, np.int64)
    rec["loss"], rec["counts"] = loss, counts
    rec["best_epoch"] = np.array(int(np.argmin(loss[:, 1])))
    rec["train"], rec["val"] = train, val
    rec["tables"] = np.stack(tables)
    rec["steps"] = np.array(sum(len(t) for t in tables))
    return rec


def spread_of(th, case, rec):
    flat = iu.flatten_state_dict({k: rec["init/" + k] for k in iu.KEYS})
    f64 = iu.float64_run(case, flat)
    rows = (rec["tables"][0].size, len(rec["val"]))
    for e, phases in enumerate(f64["phases"]):
        for j, ph in enumerate(phases):
            soft = ph.bounds()[2]
            assert soft <= 0.01 * rows[j], "%s: epoch %d phase %d has %d soft rows of %d: change the case's seed" \
                % (case["name"], e, j, soft, rows[j])
    sd = {k: th.from_numpy(np.ascontiguousarray(a)) for k, a in zip(iu.KEYS, iu.unflatten(f64["flat"], case["S"], case["A"]))}
    logits = iu.forward(f64["flat"], ru.rows(f64["states"], rec["eval_states/idx"]), case["A"])
    g = {k: rec[k] for k in ("final/names", "final/sums", "final/abss", "eval_states/full")}
    worst, _ = golden_util.endpoint_errors(sd, g, case["lr"], f64["steps"], logits)
    return {"param": worst["param"], "eval_states": worst["eval_states"],
            "loss": float((np.abs(rec["loss"] - f64["loss"]) / np.abs(f64["loss"])).max()),
            "loss_first_last": [float(rec["loss"][0, 0]), float(rec["loss"][-1, 0])],
            "val_loss": [float(v) for v in rec["loss"][:, 1]]}


def main():
    mg._stub_modules()
    sys.path.insert(0, mg.REF)
    import torch as th
    th.set_num_threads(1)
    out, spread = {}, {}
    for case in iu.CASES:
        rec = reference_run(th, case)
        spread[case["name"]] = spread_of(th, case, rec)
        print(case["name"], json.dumps(spread[case["name"]]), "counts", rec["counts"][-1].tolist(), "best", int(rec["best_epoch"]))
        assert max(spread[case["name"]][k] for k in ("param", "eval_states", "loss")) <= 1e-3, "shorten the case: the spread exceeds 1e-3"
        for k, a in rec.items():
            out["%s/%s" % (case["name"], k)] = a
    out["cases"] = np.array(json.dumps(list(iu.CASES)))
    out["torch_version"] = np.array(th.__version__)
    path = os.path.join(mg.OUT, "invfit_kats.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(mg.OUT, "invfit_spread.json"), "w") as f:
        json.dump({"cases": spread, "refused_above": 1e-3,
                   "metric": "the unmodified BaseInverseModel and inverseModelLoss under torch.optim.Adam in float32 on the CPU against "
                             "the float64 restatement of tests/invfit_util.py, same initial parameters, same minibatch tables: param = "
                             "worst tensor of tests/golden_util.py::endpoint_errors (|sum - ref| and |abs-sum - ref| over abs-sum + lr "
                             "* steps * numel), eval_states = its measure on the trained head's logits of the first validation "
                             "minibatch, loss = max relative error of the per-epoch train and val losses"}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s %.1f KB (%d arrays)" % (path, os.path.getsize(path) / 1024.0, len(out)))


if __name__ == "__main__":
    main()
