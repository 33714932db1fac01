"""The supervised baseline's step (GPU) against the unmodified reference (tools/make_golden_supervised.py): SupervisedLearning.trainStep
— the product's own loop body — on the inputs of step_sup_* (one training minibatch at B = 3: loss, predicted states, gradients,
BatchNorm running statistics; helpers and tolerance of tests/test_step_gpu.py, 1e-4 of the scale) and of trace_sup_cnn_b2 (3 Adam
steps at lr 1e-4, then one eval-mode validation minibatch without gradients): the first minibatch's loss, states, gradients and
BatchNorm statistics, every later loss, and the validation minibatch's loss and states, all at the same 1e-4.

The trace's end point is bounded like tests/test_trajectory_gpu.py bounds its own: the reference's rounding spread (1 against 8 CPU
threads, tests/golden/supervised_spread.json) x SPREAD_FACTOR, with that file's floors."""
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import test_trajectory_gpu as traj
from supervised_util import sup_inputs, STATE_DIM

pytestmark = pytest.mark.gpu
RTOL = 1e-4  # tests/test_step_gpu.py
LR = 1e-4


def make_learner(model_type, seed=1):
    import io
    import contextlib
    import preprocessing.preprocess as pre
    import srl_baselines.supervised as sup
    pre.N_CHANNELS = 3
    with contextlib.redirect_stdout(io.StringIO()):
        return sup.SupervisedLearning(STATE_DIM, model_type=model_type, seed=seed, learning_rate=LR, cuda=True, log_folder="/tmp")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def check_first_step(srl, loss, g, name):
    """Loss, predicted states, gradients and BatchNorm running statistics of the FIRST training minibatch against the fixture, with
    the helpers of tests/test_step_gpu.py at RTOL."""
    ref = float(g["loss/supervised"])
    print("%s: loss %.7g vs %.7g (rel %.2e)" % (name, loss, ref, abs(loss - ref) / ref))
    worst = {"states": gu.check_digest(srl.last_pred_states, g, "states", rtol=RTOL)}
    assert abs(loss - ref) <= RTOL * ref, (loss, ref)
    fails = []
    for k, p in srl.model.named_parameters():
        d, sub = gu.tensor_digest(p.grad), g["grad/" + k + "/sub"]
        if sub.size != d["sub"].size:  # (the dense fixtures keep at most 4096 samples: tools/make_golden.py::dense_subs)
            d["sub"] = d["sub"][::max(1, -(-len(d["sub"]) // 4096))]
        scale = max(float(np.abs(sub).max()), 1e-30)
        e = max(float(np.abs(d["sub"] - sub).max()) / scale, abs(float(d["l2"]) - float(g["grad/" + k + "/l2"])) / float(g["grad/" + k + "/l2"]),
                abs(float(d["sum"]) - float(g["grad/" + k + "/sum"])) / float(g["grad/" + k + "/abs"]))
        worst["grad " + k] = e
        if not e <= RTOL:
            fails.append("grad %s: %.3e" % (k, e))
    sd = srl.model.state_dict()
    for k in [f for f in g.files if f.startswith("bn/")]:
        key = k[len("bn/"):]
        if "num_batches_tracked" in key:
            assert int(sd[key]) == int(g[k]), key
            continue
        worst[key] = rel(sd[key], g[k])
        if not worst[key] <= RTOL:
            fails.append("%s: %.3e" % (key, worst[key]))
    print(name, json.dumps({k: float("%.3g" % v) for k, v in worst.items()}))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,model_type", [("step_sup_cnn_b3", "custom_cnn"), ("step_sup_mlp_b3", "mlp")])
def test_train_step_matches_reference(name, model_type):
    g = gu.load(name)
    srl = make_learner(model_type)
    obs, tgt = sup_inputs(3, 1234)
    if model_type == "mlp":
        torch.manual_seed(99)  # the reference's F.dropout draws its mask here; the product's redraw must be that mask
        np.testing.assert_array_equal(torch.empty(3, 64).bernoulli_(0.5).numpy().astype(np.uint8), g["dropout_mask/step0"])
        torch.manual_seed(99)
    loss = float(srl.trainStep(torch.from_numpy(obs), torch.from_numpy(tgt)))
    torch.cuda.synchronize()
    assert srl.optimizer.steps() == 1
    check_first_step(srl, loss, g, name)


def test_trace_follows_reference_and_validation_changes_nothing():
    name, n_steps, B = "trace_sup_cnn_b2", 3, 2
    g = gu.load(name)
    srl = make_learner("custom_cnn")
    fails = []
    for step in range(n_steps):
        obs, tgt = sup_inputs(B, 1234 + step)
        loss = float(srl.trainStep(torch.from_numpy(obs), torch.from_numpy(tgt)))
        ref = float(g["trace/values"][step])
        print("%s step %d: loss %.7g vs %.7g (rel %.2e)" % (name, step, loss, ref, abs(loss - ref) / ref))
        if not abs(loss - ref) <= RTOL * ref:
            fails.append("loss step %d: %.7g vs %.7g" % (step, loss, ref))
        if step == 0:  # (the fixture's states, gradients and BatchNorm statistics are those of the first minibatch)
            try:
                check_first_step(srl, loss, g, name)
            except AssertionError as e:
                fails.append("step 0: %s" % e)
    assert srl.optimizer.steps() == n_steps

    # ---- one validation minibatch: eval mode, no gradients; nothing that defines the trajectory may move
    fp, opt = srl.flat_params, srl.optimizer
    before = [t.clone() for t in (fp.flat, fp.bucket, fp.stage, opt.m, opt.v)] + [b.clone() for b in srl.model.buffers()]
    grad_ptrs = [p.grad.data_ptr() for p in fp.params]
    obs, tgt = sup_inputs(B, 1234 + n_steps)
    val = srl.validationStep(torch.from_numpy(obs), torch.from_numpy(tgt))
    torch.cuda.synchronize()
    assert not val.requires_grad and val.grad_fn is None and not srl.model.training
    after = [fp.flat, fp.bucket, fp.stage, opt.m, opt.v] + list(srl.model.buffers())
    assert all(torch.equal(a, b) for a, b in zip(after, before)) and opt.steps() == n_steps and not fp._dirty
    assert grad_ptrs == [p.grad.data_ptr() for p in fp.params]
    ref = float(g["val/loss"])
    print("%s validation: loss %.7g vs %.7g (rel %.2e)" % (name, float(val), ref, abs(float(val) - ref) / ref))
    if not abs(float(val) - ref) <= RTOL * ref:
        fails.append("validation loss: %.7g vs %.7g" % (float(val), ref))
    err = rel(srl.last_pred_states, g["val/states"])
    print("%s validation: states rel %.2e" % (name, err))
    if not err <= RTOL:
        fails.append("validation states: %.3e" % err)

    # ---- the end point, in the metric and with the margin of tests/test_trajectory_gpu.py
    sd = srl.model.state_dict()
    assert [str(k) for k in g["final/names"]] == list(sd.keys())
    with torch.no_grad():
        st = srl.model(torch.from_numpy(sup_inputs(B, 1234)[0]).cuda()).double().cpu().numpy()
    worst, table = gu.endpoint_errors(sd, g, LR, n_steps, st)
    with open(os.path.join(gu.GOLDEN_DIR, "supervised_spread.json")) as f:
        spread = json.load(f)["cases"][name]
    print(name, "end point", json.dumps(worst), "reference self-spread", json.dumps(spread))
    for kind, err in worst.items():
        tol = max(traj.ENDPOINT_FLOOR[kind], traj.SPREAD_FACTOR * spread[kind])
        if not err <= tol:
            fails.append("end point %s: %.3e > %.3e (reference self-spread %.3e)" % (kind, err, tol, spread[kind]))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("model_type", ["custom_cnn", "mlp"])
def test_byte_route_equals_float_route(model_type):
    """The loader's planar uint8 frames as they are (ops.EncInFn / ops.DenseInFn normalise while staging) against the same step on
    ops.frames_as_float's tensor."""
    from srlz import ops
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (3, 3, 224, 224)).astype(np.uint8))
    tgt = torch.from_numpy(sup_inputs(3, 5)[1])
    got = {}
    for read_bytes in (True, False):
        srl = make_learner(model_type)
        srl.read_bytes = read_bytes
        seen = []
        real = srl.model.forward
        srl.model.forward = lambda x, *a, **k: seen.append(x.dtype) or real(x, *a, **k)
        torch.manual_seed(99)
        got[read_bytes] = (float(srl.trainStep(frames, tgt)), srl.last_pred_states.cpu(), srl.flat_params.grad.cpu().clone())
        assert seen == [torch.uint8 if read_bytes else torch.float32]
    torch.cuda.synchronize()
    assert abs(got[True][0] - got[False][0]) <= RTOL * abs(got[False][0]), (got[True][0], got[False][0])
    assert rel(got[True][1], got[False][1]) <= RTOL and rel(got[True][2], got[False][2]) <= RTOL
    assert ops.is_u8_frames(frames)


@pytest.mark.parametrize("model_type", ["custom_cnn", "mlp"])
def test_ragged_minibatches_train(model_type):
    """B = 3, then the epoch's ragged tail B = 1, then B = 3 again, all in training mode (a BatchNorm batch of one image included)."""
    srl = make_learner(model_type)
    losses = []
    for i, B in enumerate((3, 1, 3)):
        obs, tgt = sup_inputs(B, 40 + i)
        losses.append(float(srl.trainStep(torch.from_numpy(obs), torch.from_numpy(tgt))))
        assert tuple(srl.last_pred_states.shape) == (B, STATE_DIM)
    torch.cuda.synchronize()
    assert srl.optimizer.steps() == 3 and all(np.isfinite(losses)), losses
    assert all(torch.isfinite(v).all() for v in srl.model.state_dict().values() if v.is_floating_point())
