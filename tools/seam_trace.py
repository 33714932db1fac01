"""Call trace of the Python seam (srlz/ops.py, srlz/hotpath.py) above the C ABI: which entry points a forward / backward / step enqueues,
in which order and with which descriptors, sizes and null / non-null pointers.  tests/test_seam_calls_gpu.py replays SCENARIOS and
compares with tests/golden/seam_calls.json; `python tools/seam_trace.py --record` (GPU box) writes that file — from the sources the
trace is meant to pin, BEFORE they are changed.

Every status-checked attribute of srlz._cabi (prototype returns c_int, not in _NOT_STATUS: the calls that enqueue work) is replaced by
a wrapper while a scenario runs; size queries and predicates are not logged (a correct change of the seam may reorder them) and no
address is: a pointer is "ptr" or "null", a structure its name and field values, an array its element type and length (+ the values
of a float array), numbers as they are.  Workspace sizes depend on the number of compute units: the fixture holds for MI355X only.
"""
import contextlib
import ctypes
import io
import json
import numbers
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "srl-zoo_amd"), REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(REPO, "tests", "golden", "seam_calls.json")

# Every enqueueing entry point called from the conv-block half of srlz/ops.py (everything above LinearFn) and from srlz/hotpath.py
# (bn_replay_many through ops.bn_replay_many) in the sources the fixture was recorded from: r"\bC\.(\w+)\(" over those two texts,
# intersected with enqueueing().  Each must occur in the fixture.
SEAM_ENTRY_POINTS = (
    "avgpool_nhwc", "bn_add_relu", "bn_bwd_finalize_partials", "bn_eval_params", "bn_eval_params_chunks", "bn_finalize",
    "bn_finalize_chunks", "bn_relu_bwd", "bn_relu_bwd_sums", "bn_relu_fwd", "bn_relu_pool_bwd", "bn_relu_pool_bwd_apply",
    "bn_relu_pool_bwd_sums", "bn_relu_pool_fwd", "bn_replay_many", "conv1_bwd_data", "conv1_bwd_weight", "conv1_bwd_weight_fused",
    "conv1_bwd_weight_fused_u8", "conv1_fwd", "conv1_fwd_u8", "conv64_bwd_data", "conv64_bwd_data_pool_sums", "conv64_bwd_fused",
    "conv64_bwd_weight", "conv64_fwd", "conv64_pack_weights", "conv64_wino_bwd_data", "conv64_wino_bwd_data_pool_sums",
    "conv64_wino_bwd_weight", "conv64_wino_fwd", "conv64_wino_pack_weights", "convT_out_bwd_data", "convT_out_bwd_fused",
    "convT_out_bwd_weight", "convT_out_fwd", "convT_out_fwd_loss", "convT_out_fwd_loss_u8", "convn_fwd", "convn_pack_weights",
    "normalize_lut", "normalize_u8_planar", "pair_loss_finalize", "scale_by_scalar")


def enqueueing():
    import torch  # noqa: F401  (before libsrlz_hip.so: the library must find the HIP runtime torch has loaded, not load a second one)
    from srlz import _cabi as C
    return sorted(n[len("srlz_"):] for n, (res, _) in C._PROTOS.items() if res is ctypes.c_int and n not in C._NOT_STATUS)


def _reduce(a, ctype=None):
    if isinstance(a, ctypes.Structure):
        return [type(a).__name__] + [_reduce(getattr(a, f), t) for f, t in a._fields_]
    if isinstance(a, ctypes.Array):
        floats = a._type_ in (ctypes.c_float, ctypes.c_double)
        return [a._type_.__name__, len(a)] + ([float(v) for v in a] if floats else [])
    if a is None:
        return "null"
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if ctype is not None and (ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer)):
        return "ptr" if a else "null"  # (an address given as a plain int, or byref(...))
    if isinstance(a, (bool, numbers.Integral)):
        return int(a)
    if isinstance(a, numbers.Real):
        return float(a)
    raise TypeError("seam_trace: argument %r of a kind the trace does not know" % (a,))


@contextlib.contextmanager
def recording(trace):
    from srlz import _cabi as C
    saved = {}
    for name in enqueueing():
        def wrapper(*a, _fn=getattr(C, name), _name=name, _types=C._PROTOS["srlz_" + name][1]):
            trace.append([_name] + [_reduce(x, t) for x, t in zip(a, _types)])
            return _fn(*a)
        saved[name] = getattr(C, name)
        setattr(C, name, wrapper)
    try:
        yield trace
    finally:
        for name, fn in saved.items():
            setattr(C, name, fn)


# ---- scenarios: each returns {"calls": [...]} (+ "timers" for the default route) -----------------------------------------------
B = 2  # the encoder and decoder are fixed at 224 x 224: the smallest step there is


def _frames(n, size=224, seed=31):
    import numpy as np
    import torch
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (n, 3, size, size), dtype=np.uint8))


def _learner(losses=("autoencoder",)):
    import models.learner as learner
    import preprocessing.preprocess as pre
    pre.N_CHANNELS = 3
    learner.BATCH_SIZE = B
    with contextlib.redirect_stdout(io.StringIO()):
        return learner.SRL4robotics(200, model_type="custom_cnn", seed=3, learning_rate=1e-3, cuda=True, losses=list(losses),
                                    n_actions=6, log_folder="/tmp")


def train_step(as_bytes=True, switch=None, timers=False):
    """SRL4robotics.trainStep of the auto-encoder as learn() runs it; `switch`: a hotpath fusion switch cleared for the step;
    `timers`: a second step with ops' timers on, its report's keys with their launch counts and flop."""
    import numpy as np
    import torch
    from losses.losses import LossManager
    from srlz import hotpath, ops
    srl = _learner()
    both = _frames(2 * B).cuda()
    if not as_bytes:
        both = ops.frames_as_float(both)
    act = torch.from_numpy(np.random.RandomState(1).randint(0, 6, (B,)).astype(np.int64)).view(-1, 1).cuda()
    out = {"calls": []}
    old = getattr(hotpath, switch) if switch else None
    if switch:
        setattr(hotpath, switch, False)
    try:
        with recording(out["calls"]):
            for timed in ((False, True) if timers else (False,)):
                ops.timers_enable(timed)
                obs, nxt = srl._toDevicePair(both[:B], both[B:])
                srl.trainStep(obs, nxt, act, LossManager(srl.model, None))
                if timed:
                    out["timers"] = {k: [v["launches"], v["flop"]] for k, v in sorted(ops.timers_report().items())}
        torch.cuda.synchronize()
    finally:
        ops.timers_enable(False)
        if switch:
            setattr(hotpath, switch, old)
    return out


def taps_step(case="step_ae_b2"):
    """The loop body of tests/test_step_gpu.py (hotpath.TAPS = {} around every forward: the plain chain — no links, materialised
    BatchNorm backward, two-launch last layer); "step_vae_perceptual_b2": its VAE + perceptual step, whose reconstruction carries a
    gradient into the frozen denoiser (Conv1Fn with conv1_bwd_data) and whose getStates replays the encoder's BatchNorm updates."""
    import torch
    import golden_util as gu
    import test_step_gpu as S
    cfg = gu.ext_defaults(dict(gu.ext_cases().get(case, dict(losses=["autoencoder"], B=B))))
    obs, nxt, act = (torch.from_numpy(a) for a in gu.golden_inputs(cfg["B"], 3, 6, seed=1234))
    model = S.build(cfg["losses"], S=cfg["S"]).to("cuda")
    eps = denoiser = None
    if "vae" in cfg["losses"]:
        torch.manual_seed(99)
        eps = [torch.randn(cfg["B"], cfg["S"]), torch.randn(cfg["B"], cfg["S"])]
    if cfg["dae_seed"] is not None:
        denoiser = S.build(["dae"], S=cfg["S"], seed=cfg["dae_seed"]).to("cuda").eval()
        for prm in denoiser.parameters():
            prm.requires_grad = False
    out = {"calls": []}
    with recording(out["calls"]):
        S.hip_step(model, cfg["losses"], obs, nxt, act, eps_list=eps, weights=cfg["weights"], denoiser=denoiser)
    return out


def eval_forward():
    import torch
    import golden_util as gu
    import test_step_gpu as S
    model = S.build(["autoencoder"]).to("cuda").eval()
    obs = torch.from_numpy(gu.golden_inputs(B, 3, 6, seed=1234)[0]).cuda()
    out = {"calls": []}
    with torch.no_grad(), recording(out["calls"]):
        model(obs)
    torch.cuda.synchronize()
    return out


def trunk_forward(size, training):
    """hotpath.resnet18_forward on a fresh trunk: layer 1 is 16 x 16 for size 64 (Winograd) and 13 x 13 for 52 (tile kernel)."""
    import torch
    from models.triplet import ResNet18Trunk
    from srlz import hotpath
    torch.manual_seed(11)
    trunk = ResNet18Trunk().to("cuda")
    trunk.train(training)
    x = torch.randn(2, 3, size, size).cuda()
    out = {"calls": []}
    with recording(out["calls"]):
        hotpath.resnet18_forward(trunk, x, training, groups=2 if training else 1)
    torch.cuda.synchronize()
    return out


def norm_table():
    """The first request for the uint8 normalisation table on a device (srlz_normalize_lut), and a conversion that uses it."""
    import torch
    from srlz import ops
    out = {"calls": []}
    ops._NORM_LUT.clear()
    with recording(out["calls"]):
        ops.frames_as_float(_frames(2, 8).cuda())
    torch.cuda.synchronize()
    return out


def dec_block_two_launches():
    """Kernel level: a decoder block whose BatchNorm backward is deferred to its producer (in_link) but whose own backward is the two
    launches (no out_link) — srlz_bn_relu_bwd_sums over (y_prev, dA).  No model-level step gets there: every block between two links
    takes srlz_conv64_bwd_fused at the decoder's sizes.  [2, 13, 13, 64] is the decoder's first map at n = 2
    (tests/test_kernels_gpu.py::test_fused_bn_backward_operand's smallest)."""
    import torch
    from srlz import ops
    g = torch.Generator().manual_seed(13)

    def rnd(*shape, scale=1.0, grad=False):
        return (torch.randn(*shape, generator=g) * scale).cuda().requires_grad_(grad)
    a, w0, b0 = rnd(2, 6, 6, 64), rnd(64, 64, 3, 3, scale=0.05), rnd(64, scale=0.1)
    gamma, beta = (torch.rand(64, generator=g) + 0.5).cuda().requires_grad_(), rnd(64, scale=0.2, grad=True)
    rm, rv = rnd(64, scale=0.1), (torch.rand(64, generator=g) + 0.5).cuda()
    w, bias = rnd(64, 64, 3, 3, scale=0.05, grad=True), rnd(64, scale=0.1, grad=True)
    out = {"calls": []}
    with recording(out["calls"]):
        y_prev, st = ops.Conv64Fn.apply(a, w0, b0, 2, 0, True, True)
        y, _ = ops.DecBlockFn.apply(y_prev, st, gamma, beta, rm, rv, True, w, bias, True, ops.BwdLink(), None)
        y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    return out


SCENARIOS = (
    ("a_default_u8", lambda: train_step(True, timers=True)),
    ("b_default_float", lambda: train_step(False)),
    ("c_taps_plain_chain", lambda: taps_step()),
    ("d_no_fuse_enc_in", lambda: train_step(True, "_FUSE_ENC_IN")),
    ("d_no_defer_bn_bwd", lambda: train_step(True, "_DEFER_BN_BWD")),
    ("d_no_fuse_recon", lambda: train_step(True, "_FUSE_RECON")),
    ("e_vae_perceptual", lambda: taps_step("step_vae_perceptual_b2")),
    ("f_eval_forward", eval_forward),
    ("g_trunk_train_64", lambda: trunk_forward(64, True)),
    ("g_trunk_train_52", lambda: trunk_forward(52, True)),
    ("g_trunk_eval_64", lambda: trunk_forward(64, False)),
    ("g_trunk_eval_52", lambda: trunk_forward(52, False)),
    ("k_norm_table", norm_table),
    ("k_dec_block_two_launches", dec_block_two_launches),
)


# ---- the fixture: every distinct call once, a scenario = indices into that table ---------------------------------------------------
def pack(results):
    table, index, packed = [], {}, {}
    for name, res in results.items():
        ids = []
        for call in res["calls"]:
            key = json.dumps(call)
            if key not in index:
                index[key] = len(table)
                table.append(call)
            ids.append(index[key])
        packed[name] = dict(res, calls=ids)
    return {"calls": table, "scenarios": packed}


def unpack(fixture):
    return {name: dict(res, calls=[fixture["calls"][i] for i in res["calls"]]) for name, res in fixture["scenarios"].items()}


def plain(result):
    """A scenario's result as JSON hands it back (lists for tuples, floats as their shortest round-trip text)."""
    return json.loads(json.dumps(result))


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        results = {}
        for name, fn in SCENARIOS:
            results[name] = plain(fn())
            print("%-28s %5d calls" % (name, len(results[name]["calls"])), flush=True)
        packed = pack(results)
        with open(FIXTURE, "w") as f:  # (one call per line: a diff of the fixture can be read)
            f.write("{\"calls\": [\n" + ",\n".join(json.dumps(c) for c in packed["calls"]) + "\n],\n\"scenarios\": "
                    + json.dumps(packed["scenarios"], sort_keys=True) + "}\n")
        seen = {c[0] for r in results.values() for c in r["calls"]}
        print("entry points never called:", sorted(set(SEAM_ENTRY_POINTS) - seen))
    else:
        sys.exit("usage: python tools/seam_trace.py --record   (on the GPU box, writes %s)" % FIXTURE)
