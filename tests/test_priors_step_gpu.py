"""Training steps with the reward-prior and episode-prior losses through the product's route (SRL4robotics.trainStep, the flat gradient
bucket, fused Adam) against the unmodified reference's numbers (tests/golden, tools/make_golden.py step_case): loss terms and every
gradient of the first step, the discriminator's included; the losses of an Adam trace with a validation step and the parameters of
model and discriminator it ends at.  Also: hipGraph replay (SRLZ_GRAPH=1) follows eager over steps with changing partner rows."""
import contextlib
import io
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-4
# biases in front of a BatchNorm: mathematically zero gradient, fp32 round-off only (skipped as in tests/test_step_gpu.py)
NOISE_GRADS = ("decoder_conv.0.bias", "decoder_conv.3.bias", "decoder_conv.6.bias", "decoder_conv.9.bias")
SPLIT = OrderedDict([("autoencoder", 120), ("inverse", 80), ("reward-prior", -1)])
# (name, losses, steps, validation steps, model type, split dimensions, balanced sampling)
GOLDEN = [("step_if_rp_ep_b4", ["inverse", "forward", "reward-prior", "episode-prior"], 1, (), "custom_cnn", None, False),
          ("step_ae_rp_b4", ["autoencoder", "reward-prior"], 1, (), "custom_cnn", None, False),
          ("step_mlp_vae_ep_bal_b4", ["vae", "episode-prior"], 1, (), "mlp", None, True),
          ("step_linear_if_ep_b4", ["inverse", "forward", "episode-prior"], 1, (), "linear", None, False),
          ("step_split_ae_rp_b4", list(SPLIT.keys()), 1, (), "custom_cnn", SPLIT, False),
          ("trace_if_rp_ep_b4", ["inverse", "forward", "reward-prior", "episode-prior"], 4, (2,), "custom_cnn", None, False)]


def learner(losses, S=200, lr=1e-4, model_type="custom_cnn", split=None):
    import preprocessing.preprocess as pre
    from models.learner import SRL4robotics
    pre.N_CHANNELS = 3
    with contextlib.redirect_stdout(io.StringIO()):
        return SRL4robotics(S, model_type=model_type, seed=1, learning_rate=lr, cuda=True, losses=losses, n_actions=6,
                            log_folder="/tmp", split_dimensions=split if split is not None else -1)


def _thin(sub):
    """The samples tools/make_golden.py keeps of a dense model's digest (dense_subs): v[::ceil(len / 4096)]."""
    return sub[::max(1, -(-len(sub) // 4096))]


def bucket_grads(srl):
    flat = srl.flat_params
    named = [("model/" + n, p) for n, p in srl.model.named_parameters() if p.requires_grad]
    if srl.discriminator is not None:
        named += [("disc/" + n, p) for n, p in srl.discriminator.named_parameters()]
    assert len(named) == len(flat.offsets)
    return OrderedDict((n, flat.grad[off:off + p.numel()].view(p.shape).double().cpu()) for (n, p), off in zip(named, flat.offsets))


def check_digest(t, g, prefix, rtol=RTOL):
    import golden_util as gu
    d = gu.tensor_digest(t)
    d["sub"] = _thin(d["sub"])
    ref_sub = g[prefix + "/sub"]
    assert d["sub"].shape == ref_sub.shape, prefix
    assert np.abs(d["sub"] - ref_sub).max() <= rtol * max(np.abs(ref_sub).max(), 1e-30), prefix
    l2 = float(g[prefix + "/l2"])
    assert abs(float(d["l2"]) - l2) <= rtol * max(l2, 1e-30), prefix


def step_inputs(srl, g, B, step, losses):
    """(obs, next_obs, actions, trainStep keywords) of step `step` of a golden case."""
    import golden_util as gu
    from losses.losses import episodeInputs
    obs_np, next_np, actions = gu.golden_inputs(B, 3, 6, seed=1234 + step)
    o, no = srl._toDevicePair(torch.from_numpy(obs_np), torch.from_numpy(next_np))
    kw = {}
    if "reward-prior" in losses:
        raw, _ = gu.golden_rewards(B, seed=1234 + step)
        kw["reward_prior_st"] = torch.from_numpy(raw.astype(np.float32)).cuda()
    if "episode-prior" in losses:
        ids, others = g["episode/ids"], g["episode/others"][step]
        assert (others >= 0).all() and (others < B).all()
        kw["episode_others"], kw["episode_same"] = episodeInputs(others, (ids == ids[others]).astype(np.float32), srl.device)
    return o, no, torch.from_numpy(actions).view(-1, 1).cuda(), kw


@pytest.mark.parametrize("name,losses,n_steps,val_steps,model_type,split,balanced", GOLDEN)
def test_priors_step_matches_reference_golden(name, losses, n_steps, val_steps, model_type, split, balanced, monkeypatch):
    import golden_util as gu
    import models.learner as learner_mod
    from losses.losses import LossManager
    g = gu.load(name)
    B, S = 4, 200
    monkeypatch.setattr(learner_mod, "BALANCED_SAMPLING", balanced)
    srl = learner(losses, model_type=model_type, split=split)
    disc0 = {k: v.detach().double().cpu().clone() for k, v in srl.discriminator.state_dict().items()} \
        if srl.discriminator is not None else {}
    trace = []
    for step in range(n_steps):
        o, no, act, kw = step_inputs(srl, g, B, step, losses)
        if n_steps == 1:  # the step's train-mode states (the states every loss of the step reads)
            with torch.no_grad():
                srl.model.train()
                check_digest(srl.model.getStates(o), g, "states")
                check_digest(srl.model.getStates(no), g, "next_states")
                if hasattr(srl.model.model, "forgetRecent"):
                    srl.model.model.forgetRecent()
        if "vae" in losses:
            torch.manual_seed(99 + step)  # the reference's two draws of this step (std.new(...).normal_())
            it = iter([torch.randn(B, S).cuda(), torch.randn(B, S).cuda()])
            srl.model.model.eps_fn = lambda mu: next(it)
        lm = LossManager(srl.model, None)
        loss = srl.trainStep(o, no, act, lm, validation_mode=step in val_steps, **kw)
        torch.cuda.synchronize()
        rec = dict(zip(lm.names, [float(v) for v in lm.losses]))
        rec["total"] = float(loss.detach())
        trace.append(rec)
        if step == 0:
            for k in [f for f in g.files if f.startswith("loss/")]:
                nm, v = k[len("loss/"):], float(g[k])
                assert abs(rec[nm] - v) <= RTOL * max(abs(v), 1e-6), (k, rec[nm], v)
            for k, gr in bucket_grads(srl).items():
                key = ("grad/" + k[len("model/"):]) if k.startswith("model/") else ("disc_grad/" + k[len("disc/"):])
                if (key + "/none") in g.files:
                    assert not gr.abs().max().item(), k
                elif k.endswith(NOISE_GRADS):
                    continue
                elif k.startswith("disc/") or model_type != "custom_cnn":
                    check_digest(gr, g, key)  # (the dense models make no pooling decisions: held as tests/test_dense_step_gpu.py holds them)
                else:
                    # the conv model's fp32 gradients carry the tie-break noise of its ReLU / max-pool decisions (tests/test_step_gpu.py
                    # module docstring): norm and strided subsample agree in the L2 sense, as there
                    import golden_util as gu
                    d = gu.tensor_digest(gr)
                    l2 = float(g[key + "/l2"])
                    assert abs(float(d["l2"]) - l2) <= 2e-2 * l2, key
                    assert np.linalg.norm(d["sub"] - g[key + "/sub"]) <= 5e-2 * max(np.linalg.norm(g[key + "/sub"]), 1e-30), key
    if n_steps > 1:
        names = [str(n) for n in g["trace/names"]]
        for step, row in enumerate(g["trace/values"]):
            for nm, v in zip(names, row):
                assert abs(trace[step][nm] - v) <= 1e-3 * max(abs(v), 1e-6), (step, nm, trace[step][nm], v)
        lr = 1e-4
        for prefix, sd in (("final", srl.model.state_dict()), ("final_disc", srl.discriminator.state_dict())):
            for k, ref_sum, ref_abs in zip(g[prefix + "/names"], g[prefix + "/sums"], g[prefix + "/abss"]):
                k = str(k)
                v = sd[k].double().cpu()
                if "num_batches_tracked" in k:
                    assert int(v) == int(ref_sum), k
                    continue
                e = max(abs(float(v.sum()) - ref_sum), abs(float(v.abs().sum()) - ref_abs)) / (ref_abs + lr * n_steps * v.numel())
                assert e <= 2e-2, (prefix, k, e)
                if prefix == "final_disc":
                    # Adam's movement of the discriminator, against the reference's: (final - initial) digests, the initial ones being
                    # the reference's too (tests/test_priors_host_cpu.py holds the seeded init)
                    v0 = disc0[k]
                    for got_d, ref_d in ((float(v.sum() - v0.sum()), ref_sum - float(v0.sum())),
                                         (float(v.abs().sum() - v0.abs().sum()), ref_abs - float(v0.abs().sum()))):
                        assert abs(got_d) > 0 and abs(ref_d) > 0, (k, got_d, ref_d)
                        assert abs(got_d - ref_d) <= 0.1 * abs(ref_d) + 1e-9 * ref_abs, (k, got_d, ref_d)


def test_priors_checkpoint_keys_and_regularisers():
    """The discriminator shares the flat bucket (after the model's parameters) but stays out of state_dict() and of the
    regularised parameters, as in the reference."""
    from losses.losses import LossManager
    srl = learner(["inverse", "reward-prior", "episode-prior"])
    keys = list(srl.model.state_dict().keys())
    assert not any(k.startswith("net.") or "discriminator" in k for k in keys)
    n_model = len([p for p in srl.model.parameters() if p.requires_grad])
    assert len(srl.flat_params.params) == n_model + 6
    for p, q in zip(srl.flat_params.params[n_model:], srl.discriminator.parameters()):
        assert p is q
    reg = LossManager(srl.model, None).reg_params
    assert not any(any(r is p for p in srl.discriminator.parameters()) for r in reg)


def test_priors_graph_replay_matches_eager(monkeypatch):
    """SRLZ_GRAPH=1: the partner rows and rewards are static graph inputs copied before every replay, not frozen at capture."""
    from losses.losses import LossManager, episodeInputs
    import golden_util as gu
    losses = ["inverse", "forward", "reward-prior", "episode-prior"]
    B = 8
    runs = []
    for graph in ("0", "1"):
        monkeypatch.setenv("SRLZ_GRAPH", graph)
        srl = learner(losses)
        assert srl._use_graph == (graph == "1")
        rng = np.random.RandomState(0)
        ids = np.array([0, 0, 1, 1, 1, 2, 3, 3])
        out = []
        for step in range(3):
            obs_np, next_np, actions = gu.golden_inputs(B, 3, 6, seed=1234 + step)
            o, no = srl._toDevicePair(torch.from_numpy(obs_np).cuda(), torch.from_numpy(next_np).cuda())
            others = rng.permutation(B)
            eo, es = episodeInputs(others, (ids == ids[others]).astype(np.float32), srl.device)
            rp = torch.from_numpy(rng.randint(-1, 2, B).astype(np.float32)).cuda()
            lm = LossManager(srl.model, None)
            loss = srl.trainStep(o, no, torch.from_numpy(actions).view(-1, 1).cuda(), lm, reward_prior_st=rp, episode_others=eo,
                                 episode_same=es)
            torch.cuda.synchronize()
            out.append([float(loss)] + [float(v) for v in lm.losses])
        out.append(srl.flat_params.flat.detach().cpu().clone())
        runs.append(out)
    for step in range(3):
        for a, b in zip(runs[0][step], runs[1][step]):
            assert abs(a - b) <= 1e-5 * max(abs(a), 1e-6), (step, runs[0][step], runs[1][step])
    assert len(set(round(r[-1], 6) for r in runs[0][:3])) > 1  # (the episode term changes with the draw)
    d = (runs[0][3] - runs[1][3]).abs().max().item()
    assert d <= 1e-5, d


def test_prior_step_launches_only_library_kernels():
    """A bs = 256 auto-encoder step with both losses runs the library's kernels plus fills and copies: no ATen compute kernel (the
    priors composed from torch ops would add about 40)."""
    from torch.profiler import profile, ProfilerActivity
    from losses.losses import LossManager, episodeInputs
    import golden_util as gu
    B = 256
    srl = learner(["autoencoder", "reward-prior", "episode-prior"])
    rng = np.random.RandomState(0)
    obs_np, next_np, actions = gu.golden_inputs(B, 3, 6, seed=1234)
    o8 = torch.from_numpy(np.clip(obs_np * 60 + 128, 0, 255).astype(np.uint8)).cuda()
    n8 = torch.from_numpy(np.clip(next_np * 60 + 128, 0, 255).astype(np.uint8)).cuda()
    ids = np.sort(rng.randint(0, 20, B))
    others = rng.permutation(B)

    def step():
        eo, es = episodeInputs(others, (ids == ids[others]).astype(np.float32), srl.device)
        rp = torch.from_numpy(rng.randint(-1, 2, B).astype(np.float32)).cuda()
        o, no = srl._toDevicePair(o8, n8)
        return srl.trainStep(o, no, torch.from_numpy(actions).view(-1, 1).cuda(), LossManager(srl.model, None), reward_prior_st=rp,
                             episode_others=eo, episode_same=es)
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert any("episode_prior_fwd_kernel" in n for n in names), sorted(set(names))[:40]
    for k in ("episode_prior_bwd_rows_kernel", "episode_prior_bwd_reduce_kernel", "reward_prior_fwd_kernel", "reward_prior_bwd_kernel"):
        assert any(k in n for n in names), k

    def allowed(n):
        low = n.lower()
        if any(w in low for w in ("fill", "copy", "memcpy", "memset")):
            return True
        # (torch's own kernels live in at:: / c10::; the BLAS and DNN libraries announce themselves by name)
        return not any(w in low for w in ("at::", "c10::", "aten", "cijk", "rocblas", "hipblas", "hipblaslt", "miopen", "triton"))
    bad = sorted(set(n for n in names if not allowed(n)))
    assert not bad, bad


def test_reverse_layer_identity_forward_negated_backward():
    from models.priors import ReverseLayerF
    x = torch.randn(5, 7, device="cuda", requires_grad=True)
    g = torch.randn(5, 7, device="cuda")
    y = ReverseLayerF.apply(x, 0.5)
    assert torch.equal(y, x)
    y.backward(g)
    torch.cuda.synchronize()
    assert torch.equal(x.grad, -0.5 * g)
