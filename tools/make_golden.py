#!/usr/bin/env python
"""Generate tests/golden/*.npz by running the UNMODIFIED reference (/root/reference) on CPU.

Runs only in the build container (the reference never travels to the GPU box).  The
reference is imported, never copied: four absent third-party modules are stubbed in
sys.modules (torchvision, cv2, termcolor, seaborn) exactly as SURVEY.md §8c describes.

Every fixture is DATA: inputs are regenerated from a seed by `golden_inputs()` (shared with
the tests through tests/golden_util.py), outputs are stored as sums, norms and strided
subsamples so the files stay small.

    python tools/make_golden.py            # writes tests/golden/*.npz
"""
from __future__ import print_function
import os
import sys
import types
import json

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))


def _stub_modules():
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvm.resnet18 = lambda *a, **k: None
    tv.models = tvm
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tvm
    tc = types.ModuleType("termcolor")
    tc.colored = lambda s, *a, **k: s
    sys.modules["termcolor"] = tc
    sb = types.ModuleType("seaborn")
    sb.set = lambda *a, **k: None
    sys.modules["seaborn"] = sb
    sys.modules["cv2"] = types.ModuleType("cv2")
    import matplotlib
    matplotlib.use("Agg")


def import_reference():
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # single-threaded: deterministic summation order
    import preprocessing.preprocess as ref_pre
    from models.modules import SRLModules
    import losses.losses as ref_losses
    return th, ref_pre, SRLModules, ref_losses


from golden_util import golden_inputs, golden_rewards, golden_noisy, tensor_digest  # noqa: E402


def digest_state_dict(sd):
    names, shapes, sums, abss = [], [], [], []
    for k, v in sd.items():
        names.append(k)
        shapes.append(list(v.shape))
        vv = v.double()
        sums.append(float(vv.sum()))
        abss.append(float(vv.abs().sum()))
    return dict(names=np.array(names), shapes=np.array([json.dumps(s) for s in shapes]),
                sums=np.array(sums), abss=np.array(abss))


def build(th, ref_pre, SRLModules, losses, S=200, A=6, C=3, seed=1, inverse="linear", split=None, model_type="custom_cnn"):
    ref_pre.N_CHANNELS = C
    np.random.seed(seed)
    th.manual_seed(seed)
    if split is not None:
        from models.modules import SRLModulesSplit  # the reference's
        return SRLModulesSplit(state_dim=S, action_dim=A, cuda=False, model_type="custom_cnn", losses=losses,
                               split_dimensions=split, inverse_model_type=inverse)
    return SRLModules(state_dim=S, action_dim=A, cuda=False, model_type=model_type,
                      losses=losses, inverse_model_type=inverse)


def grads_digest(model, out, prefix="grad/"):
    for name, p in model.named_parameters():
        if p.grad is None:
            out[prefix + name + "/none"] = np.array(1)
            continue
        for k, v in tensor_digest(p.grad).items():
            out[prefix + name + "/" + k] = v


def bn_digest(model, out, prefix="bn/"):
    for k, v in model.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out[prefix + k] = v.detach().double().numpy().copy()


def step_case(th, ref_pre, SRLModules, RL, losses, B, C=3, S=200, A=6, n_steps=1, lr=None,
              eps_seed=99, beta=1.0, inverse="linear", weights=None, split=None, l1_reg=0.0, l2_reg=0.0, val_steps=(),
              model_type="custom_cnn", balanced=False):
    """One (or several) loop bodies of models/learner.py:373-497 driven on the reference classes.
    `val_steps`: steps run as validation minibatches (learner.py:362-364,487-497: eval mode, forward + backward, no
    optimizer step).
    reward-prior / episode-prior: the raw golden rewards as float32; the episode prior's Discriminator is built right after the model
    (learner.py:189-190), its episodes are EPISODES[:B], np.random is seeded with 777 + step before the loss draws its partners
    (`balanced`: BALANCED_SAMPLING), and the drawn partner rows are recorded (episode/others)."""
    model = build(th, ref_pre, SRLModules, [l for l in losses if l != "perceptual"] if split is None else losses, S=S, A=A,
                  C=C, inverse=inverse, split=split, model_type=model_type)
    disc = None
    if "episode-prior" in losses:
        from models.priors import Discriminator  # the reference's
        disc = Discriminator(2 * S)
        disc_inputs = []
        disc.register_forward_pre_hook(lambda _m, inp: disc_inputs.append(inp[0].detach().clone()))
        episodes = np.array(EPISODES[:B])
        drawn = []
    denoiser = None
    if "perceptual" in losses:  # the frozen, eval-mode DAE of learner.py:317-326 (seed 7 stands in for "pre-trained")
        denoiser = build(th, ref_pre, SRLModules, ["dae"], S=S, A=A, C=C, seed=7)
        denoiser.eval()
        for param in denoiser.parameters():
            param.requires_grad = False
    w = {"forward": 1.0, "inverse": 2.0, "reward": 1.0, "autoencoder": 1.0, "dae": 1.0, "vae": 0.5e-6, "perceptual": 1e-6}
    if disc is not None or "reward-prior" in losses:
        w.update({"reward-prior": 10, "episode-prior": 1.0})
    if weights:
        w.update(weights)
    out = {}
    opt = None
    if lr is not None:
        opt = th.optim.Adam([p for p in model.parameters() if p.requires_grad] + ([p for p in disc.parameters()] if disc is not None
                                                                                   else []), lr=lr)
    history = {}
    lm = RL.LossManager(model, None)
    trace = []
    for step in range(n_steps):
        obs, next_obs, actions = golden_inputs(B, C, A, seed=1234 + step)
        obs, next_obs = th.from_numpy(obs), th.from_numpy(next_obs)
        act = th.from_numpy(actions).view(-1, 1)
        if step in val_steps:
            model.eval()
        else:
            model.train()
        if opt is not None:
            opt.zero_grad()
        lm.resetLosses()
        mu = logvar = None
        if l1_reg > 0:
            RL.l1Loss(lm.reg_params, l1_reg, lm)
        if l2_reg > 0:
            RL.l2Loss(lm.reg_params, l2_reg, lm)
        if "autoencoder" in losses:
            (states, dec), (next_states, next_dec) = model(obs), model(next_obs)
        elif "dae" in losses:
            noisy = th.from_numpy(golden_noisy(obs.numpy(), seed=1234 + step))
            next_noisy = th.from_numpy(golden_noisy(next_obs.numpy(), seed=4321 + step))
            (states, dec), (next_states, next_dec) = model(noisy), model(next_noisy)
        elif "vae" in losses:
            th.manual_seed(eps_seed + step)
            (dec, mu, logvar), (next_dec, next_mu, next_logvar) = model(obs), model(next_obs)
            states, next_states = model.getStates(obs), model.getStates(next_obs)
        else:
            states, next_states = model(obs), model(next_obs)
            dec = next_dec = None
        if "forward" in losses:
            pred = model.forwardModel(states, act)
            RL.forwardModelLoss(pred, next_states, weight=w["forward"], loss_manager=lm)
        if "inverse" in losses:
            logits = model.inverseModel(states, next_states)
            RL.inverseModelLoss(logits, act, weight=w["inverse"], loss_manager=lm)
        if "reward" in losses:
            _, rewards_st = golden_rewards(B, seed=1234 + step)
            rewards_pred = model.rewardModel(states, next_states)
            RL.rewardModelLoss(rewards_pred, th.from_numpy(rewards_st).long(), weight=w["reward"], loss_manager=lm)
        if "autoencoder" in losses or "dae" in losses:
            RL.autoEncoderLoss(obs, dec, next_obs, next_dec, weight=w["dae" if "dae" in losses else "autoencoder"],
                               loss_manager=lm)
        if "vae" in losses:
            RL.kullbackLeiblerLoss(mu, next_mu, logvar, next_logvar, loss_manager=lm, beta=beta)
            if denoiser is not None:
                (sd_real, _), (nsd_real, _) = denoiser(obs), denoiser(next_obs)
                (sd_pred, _), (nsd_pred, _) = denoiser(dec), denoiser(next_dec)
                RL.perceptualSimilarityLoss(sd_real, sd_pred, nsd_real, nsd_pred, weight=w["perceptual"], loss_manager=lm)
            else:
                RL.generationLoss(dec, next_dec, obs, next_obs, weight=w["vae"], loss_manager=lm)
        if "reward-prior" in losses:
            raw, _ = golden_rewards(B, seed=1234 + step)
            RL.rewardPriorLoss(states, th.from_numpy(raw.astype(np.float32)).view(-1, 1), weight=w["reward-prior"], loss_manager=lm)
        if disc is not None:
            np.random.seed(777 + step)
            RL.episodePriorLoss(0, [episodes], states, disc, balanced, weight=w["episode-prior"], loss_manager=lm)
            pairs = disc_inputs[-1][:, S:]
            drawn.append([int(np.flatnonzero((states.detach() == pairs[i]).all(1).numpy())[0]) for i in range(B)])
        loss = lm.computeTotalLoss()
        loss.backward()
        rec = {n: float(l.item()) for n, l in zip(lm.names, lm.losses)}
        rec["total"] = float(loss.item())
        trace.append(rec)
        if step == 0:
            for n, v in rec.items():
                out["loss/" + n] = np.array(v)
            for k, v in tensor_digest(states).items():
                out["states/" + k] = v
            for k, v in tensor_digest(next_states).items():
                out["next_states/" + k] = v
            if dec is not None:
                for k, v in tensor_digest(dec).items():
                    out["decoded/" + k] = v
                for k, v in tensor_digest(next_dec).items():
                    out["next_decoded/" + k] = v
            if mu is not None:
                for k, v in tensor_digest(logvar).items():
                    out["logvar/" + k] = v
                for k, v in tensor_digest(next_logvar).items():
                    out["next_logvar/" + k] = v
            grads_digest(model, out)
            bn_digest(model, out)
            if disc is not None:
                grads_digest(disc, out, prefix="disc_grad/")
        if opt is not None and step not in val_steps:
            opt.step()
    if n_steps > 1 or opt is not None:
        names = sorted(trace[0].keys())
        out["trace/names"] = np.array(names)
        out["trace/values"] = np.array([[t[n] for n in names] for t in trace])
        sd = digest_state_dict(model.state_dict())
        out["final/names"], out["final/sums"], out["final/abss"] = sd["names"], sd["sums"], sd["abss"]
        bn_digest(model, out, prefix="final_bn/")
        if disc is not None:
            sd = digest_state_dict(disc.state_dict())
            out["final_disc/names"], out["final_disc/sums"], out["final_disc/abss"] = sd["names"], sd["sums"], sd["abss"]
    if disc is not None:
        out["episode/ids"] = episodes
        out["episode/others"] = np.array(drawn, dtype=np.int64)
    # eval-mode states on the (possibly updated) model: the "learned states" output (learner.py:67-88)
    model.eval()
    with th.no_grad():
        obs, _, _ = golden_inputs(B, C, A, seed=1234)
        st = model.getStates(th.from_numpy(obs))
    out["eval_states/full"] = st.double().numpy()
    return out


EPISODES = [0, 0, 1, 1, 1, 2, 3, 3]  # episode ids of the rows of a prior step case (B <= 8)


def prior_kats(th):
    """The reference's episode-prior partner draws (losses.py:335-347) for a few episode vectors, seeds and both sampling modes,
    recovered from the rows its Discriminator receives; a single-episode minibatch under balanced sampling records the error; the
    seeded Discriminator(2 S) parameters (priors.py:155-175)."""
    import losses.losses as RL
    from models.priors import Discriminator
    out = {}
    cases = [[0, 0, 1, 1], [0, 1, 1, 1, 2, 2, 3], [3, 3, 3, 5, 5, 7, 7, 7, 7, 8], list(range(6))]
    for ci, eps in enumerate(cases):
        eps = np.array(eps)
        B = len(eps)
        states = th.arange(B * 3, dtype=th.float32).view(B, 3)
        seen = []

        def disc(x):
            seen.append(x.detach().clone())
            return th.full((x.shape[0], 1), 0.5)
        for balanced in (False, True):
            for seed in (0, 1, 2):
                np.random.seed(seed)
                draws = []
                for _ in range(3):  # three consecutive steps from one seed
                    RL.episodePriorLoss(0, [eps], states, disc, balanced, 1.0, RL.LossManager(th.nn.Linear(1, 1), None))
                    pairs = seen[-1][:, 3:]
                    draws.append([int(np.flatnonzero((states == pairs[i]).all(1).numpy())[0]) for i in range(B)])
                out["case%d/%s/seed%d" % (ci, "balanced" if balanced else "uniform", seed)] = np.array(draws, dtype=np.int64)
        out["case%d/episodes" % ci] = eps
    try:
        np.random.seed(0)
        RL.episodePriorLoss(0, [np.zeros(4, dtype=np.int64)], th.zeros(4, 3), lambda x: th.full((4, 1), 0.5), True, 1.0,
                            RL.LossManager(th.nn.Linear(1, 1), None))
        out["single_episode/error"] = np.array("none")
    except Exception as e:
        out["single_episode/error"] = np.array(type(e).__name__)
    for S in (2, 200):
        th.manual_seed(5)
        sd = digest_state_dict(Discriminator(2 * S).state_dict())
        out["disc_s%d/names" % S], out["disc_s%d/sums" % S], out["disc_s%d/abss" % S] = sd["names"], sd["sums"], sd["abss"]
    return out


def dense_subs(out):
    """Every */sub array of a digest thinned to at most 4096 samples, v[::ceil(len / 4096)] (tests/test_dense_step_gpu.py takes the
    same samples): the dense models' gradients and reconstructions have up to 60 M elements."""
    return {k: (v[::max(1, -(-len(v) // 4096))] if k.endswith("/sub") else v) for k, v in out.items()}


def layer_trace(th, ref_pre, SRLModules):
    """Per-layer forward digests of the AE (train mode, B=2) via forward hooks."""
    model = build(th, ref_pre, SRLModules, ["autoencoder"])
    obs, _, _ = golden_inputs(2, 3, 6, seed=1234)
    out = {}
    hooks = []

    def mk(name):
        def hook(_m, _i, o):
            for k, v in tensor_digest(o).items():
                out[name + "/" + k] = v
        return hook
    for name, mod in model.model.named_modules():
        if name.count(".") == 1 and (name.startswith("encoder_conv") or name.startswith("decoder_conv")
                                     or name.startswith("encoder_fc") or name.startswith("decoder_fc")):
            hooks.append(mod.register_forward_hook(mk(name)))
    model.train()
    model(th.from_numpy(obs))
    for h in hooks:
        h.remove()
    return out


def loss_kats(th, RL):
    """Known-answer vectors for the free loss functions (losses/losses.py:102-129,172-214,239-256)."""
    rs = np.random.RandomState(7)
    out = {}
    a = rs.randn(4, 3, 8, 8).astype(np.float32)
    b = rs.randn(4, 3, 8, 8).astype(np.float32)
    c = rs.randn(4, 3, 8, 8).astype(np.float32)
    d = rs.randn(4, 3, 8, 8).astype(np.float32)
    mu, nmu = rs.randn(4, 10).astype(np.float32), rs.randn(4, 10).astype(np.float32)
    lv, nlv = (0.3 * rs.randn(4, 10)).astype(np.float32), (0.3 * rs.randn(4, 10)).astype(np.float32)
    logits = rs.randn(4, 6).astype(np.float32)
    act = rs.randint(0, 6, (4, 1)).astype(np.int64)
    for k, v in dict(a=a, b=b, c=c, d=d, mu=mu, nmu=nmu, lv=lv, nlv=nlv, logits=logits, act=act).items():
        out["in/" + k] = v
    T = th.from_numpy

    class M(th.nn.Module):
        pass
    lm = RL.LossManager(M(), {})
    lm.loss_history = __import__("collections").defaultdict(list)
    out["reconstruction"] = np.array(RL.reconstructionLoss(T(a), T(b)).item())
    out["autoencoder_w1"] = np.array(RL.autoEncoderLoss(T(a), T(b), T(c), T(d), 1.0, lm).item())
    out["generation_w"] = np.array(RL.generationLoss(T(b), T(d), T(a), T(c), 0.5e-6, lm).item())
    out["kl_beta2"] = np.array(RL.kullbackLeiblerLoss(T(mu), T(nmu), T(lv), T(nlv), lm, beta=2.0).item())
    out["forward_w1"] = np.array(RL.forwardModelLoss(T(mu), T(nmu), 1.0, lm).item())
    out["inverse_w2"] = np.array(RL.inverseModelLoss(T(logits), T(act), 2.0, lm).item())
    sa, sp, sn = rs.randn(5, 7).astype(np.float32), rs.randn(5, 7).astype(np.float32), rs.randn(5, 7).astype(np.float32)
    out["in/tri_s"], out["in/tri_p"], out["in/tri_n"] = sa, sp, sn
    lm2 = RL.LossManager(M(), {})
    out["triplet_w1"] = np.array(RL.tripletLoss(T(sa), T(sp), T(sn), 1.0, lm2, alpha=0.2).item())
    out["total"] = np.array(lm.computeTotalLoss().item())
    lm.updateLossHistory()
    lm.updateLossHistory()
    out["history/names"] = np.array(list(lm.loss_history.keys()))
    out["history/values"] = np.array([lm.loss_history[k][-1] for k in lm.loss_history.keys()])
    out["names"] = np.array(lm.names)
    out["weights"] = np.array(lm.weights, dtype=np.float64)
    return out


def head_kats(th, ref_pre, SRLModules):
    """forwardModel / inverseModel (linear + mlp) outputs (models/forward_inverse.py:21-31,62-70)."""
    out = {}
    rs = np.random.RandomState(11)
    s = rs.randn(5, 200).astype(np.float32)
    ns = rs.randn(5, 200).astype(np.float32)
    act = rs.randint(0, 6, (5, 1)).astype(np.int64)
    out["in/s"], out["in/ns"], out["in/act"] = s, ns, act
    for inv in ("linear", "mlp"):
        m = build(th, ref_pre, SRLModules, ["autoencoder", "inverse", "forward"], inverse=inv)
        out[inv + "/forward"] = m.forwardModel(th.from_numpy(s), th.from_numpy(act)).detach().numpy()
        out[inv + "/inverse"] = m.inverseModel(th.from_numpy(s), th.from_numpy(ns)).detach().numpy()
    return out


def detach_kats(th):
    """SRLModulesSplit.detachSplit on an all-ones state for a list of split configurations: the kept-column mask per
    (configuration, index).  Uses the reference's method unbound on a minimal stand-in object (it only reads
    self.split_dimensions)."""
    from collections import OrderedDict as OD
    from models.modules import SRLModulesSplit
    configs = [OD([("dae", 20), ("reward", -1), ("forward", 60), ("inverse", 20)]),
               OD([("vae", 150), ("inverse", 50), ("forward", -1)]),
               OD([("autoencoder", 120), ("reward", 80), ("inverse", -1)]),
               OD([("autoencoder", 50), ("inverse", -1), ("forward", -1)]),
               OD([("autoencoder", 30), ("inverse", -1), ("forward", -1), ("reward", 20)]),
               OD([("inverse", 10), ("forward", 10), ("reward", 10)])]
    out = {"n_configs": np.array(len(configs))}

    class Holder(object):
        pass
    for ci, cfg in enumerate(configs):
        S = sum(v for v in cfg.values() if v > 0)
        h = Holder()
        h.split_dimensions = cfg
        out["cfg%d/keys" % ci] = np.array(list(cfg.keys()))
        out["cfg%d/dims" % ci] = np.array(list(cfg.values()))
        x = th.ones(2, S)
        for index in list(cfg.keys()) + ["autoencoder", "vae", "absent"]:
            try:
                y = SRLModulesSplit.detachSplit(h, x, index)
                out["cfg%d/mask/%s" % (ci, index)] = y[0].numpy().astype(np.int8)
            except Exception as e:  # e.g. torch.cat of an empty list when nothing is kept and nothing is zeroed
                out["cfg%d/error/%s" % (ci, index)] = np.array(type(e).__name__)
    return out


def _install_cv2_shim():
    """PIL-backed stand-in for the five cv2 symbols the reference loader touches (data_loader.py:48-51,212,238,247):
    imread -> BGR ndarray or None, resize (identity for 224x224 sources, the only case used), cvtColor(BGR2RGB),
    INTER_AREA, COLOR_BGR2RGB.  Everything downstream of the decoded uint8 frame is the reference's own code."""
    from PIL import Image
    cv2 = sys.modules["cv2"]

    def imread(path):
        try:
            with Image.open(path) as f:
                return np.ascontiguousarray(np.asarray(f.convert("RGB"))[..., ::-1])
        except (IOError, OSError):
            return None

    def resize(im, size, interpolation=None):
        assert (im.shape[1], im.shape[0]) == tuple(size), "shim: only already-sized frames"
        return im

    cv2.imread, cv2.resize = imread, resize
    cv2.cvtColor = lambda im, code: np.ascontiguousarray(im[..., ::-1])
    cv2.INTER_AREA, cv2.COLOR_BGR2RGB = 3, 4


def loop_case(th, losses, n_epochs=2, bs=8, S=12, seed=3, lr=1e-4, n_episodes=4, ep_len=26, model_type="custom_cnn", balanced=False,
              **ctor):
    """The UNMODIFIED SRL4robotics.learn() (models/learner.py:259-579: forked loader process, queue, train/validation
    split, best-model checkpoint, state prediction) on the tiny generated dataset of tests/dataset_util.py."""
    import tempfile
    import shutil
    from dataset_util import make_dataset
    _install_cv2_shim()
    import models.learner as RLn
    tmp = tempfile.mkdtemp(prefix="srlz_loop_")
    cwd = os.getcwd()
    try:
        name, paths, actions, rewards, starts = make_dataset(tmp, n_episodes=n_episodes, ep_len=ep_len)
        os.chdir(tmp)
        os.makedirs("logs/run", exist_ok=True)
        RLn.DISPLAY_PLOTS, RLn.N_EPOCHS, RLn.BATCH_SIZE, RLn.VALIDATION_SIZE = False, n_epochs, bs, 0.2
        RLn.BALANCED_SAMPLING = balanced  # (the episode prior's partner draw, train.py --balanced-sampling)
        srl = RLn.SRL4robotics(S, model_type=model_type, seed=seed, learning_rate=lr, cuda=False, losses=losses,
                               n_actions=6, log_folder="logs/run", **ctor)
        loss_history, states, pairs = srl.learn(paths, actions, rewards, starts)
        out = {"states/full": np.asarray(states, dtype=np.float64),
               "pairs/names": np.array([p[0] for p in pairs]), "pairs/weights": np.array([float(p[1]) for p in pairs]),
               "history/names": np.array(sorted(loss_history.keys())),
               "history/values": np.array([loss_history[k] for k in sorted(loss_history.keys())], dtype=np.float64)}
        sd = digest_state_dict(th.load("logs/run/srl_model.pth"))
        out["final/names"], out["final/sums"], out["final/abss"] = sd["names"], sd["sums"], sd["abss"]
        cfg = dict(losses=losses, n_epochs=n_epochs, bs=bs, S=S, seed=seed, lr=lr, n_episodes=n_episodes, ep_len=ep_len, ctor=ctor)
        if model_type != "custom_cnn":  # (the conv cases' config strings stay byte-identical)
            cfg["model_type"] = model_type
        if balanced:
            cfg["balanced"] = True
        out["config"] = np.array(json.dumps(cfg))
        return out
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


# whole-loop cases run in a FRESH interpreter each: learn() forks its loader processes, and a child forked from a parent
# that has already run OpenMP-parallel torch code dead-locks in its first parallel region
LOOP_CASES = {"loop_aeif": dict(losses=["autoencoder", "inverse", "forward"]),
              "loop_ae_reward": dict(losses=["autoencoder", "reward"], n_epochs=1, seed=5, l2_reg=1e-4),
              # --model-type mlp / linear (reference modules.py:53-69)
              "loop_mlp_ae": dict(losses=["autoencoder"], model_type="mlp"),
              "loop_linear_aeif": dict(losses=["autoencoder", "inverse", "forward"], model_type="linear"),
              # the reward-prior / episode-prior losses (losses.py:290-359): every step draws its partners from the global numpy RNG
              "loop_if_rp_ep": dict(losses=["inverse", "forward", "reward-prior", "episode-prior"]),
              "loop_mlp_rp_ep_bal": dict(losses=["inverse", "reward-prior", "episode-prior"], model_type="mlp", balanced=True)}


def run_loop_child(name):
    import subprocess
    import tempfile
    tmp = tempfile.mktemp(suffix=".npz")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--loop-child", name, tmp], timeout=1500)
    with np.load(tmp, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    os.remove(tmp)
    return d


def loop_child(name, path):
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # before anything runs: deterministic summation order, and nothing for a forked child to trip over
    np.savez_compressed(path, **loop_case(th, **LOOP_CASES[name]))


# ---------------------------------------------------------------------------------------------------------------------------------
# (9) evaluation/predict_reward.py, run as the script it is (it has no functions): runpy.run_path on the UNMODIFIED file, after
# th.manual_seed(preseed) (its model is built before it seeds anything).  A trace function reads the script's own variables where it
# prints them, so the losses are recorded at full precision next to the four decimals parsed from its output.
# ---------------------------------------------------------------------------------------------------------------------------------
REWARD_SCRIPT = os.path.join(REF, "evaluation", "predict_reward.py")
REWARD_LINE_MODEL_BUILT, REWARD_LINE_STEP, REWARD_LINE_PRINT = 66, 122, 149  # criterion = ...; optimizer.zero_grad(); print(loss)


def reward_probe_run(th, case):
    import contextlib
    import io
    import re
    import runpy
    import tempfile
    import dataset_util
    import reward_util as ru
    seen = {"init": None, "phases": [], "steps": 0}

    def local_trace(frame, event, arg):
        if event == "line":
            g = frame.f_globals
            if frame.f_lineno == REWARD_LINE_MODEL_BUILT and seen["init"] is None:
                seen["init"] = {k: v.detach().clone() for k, v in g["model"].state_dict().items()}
            elif frame.f_lineno == REWARD_LINE_STEP:
                seen["steps"] += 1
            elif frame.f_lineno == REWARD_LINE_PRINT and (g["epoch"], g["phase"]) != seen.get("last"):  # a two-line statement
                seen["last"] = (g["epoch"], g["phase"])
                seen["phases"].append(dict(epoch=g["epoch"], phase=g["phase"], loss=float(g["epoch_loss"]), acc=float(g["epoch_acc"]),
                                           per_class=[float(g["corrects"][0]), float(g["corrects"][1])],
                                           counts=[int(g["running_corrects"]), -1, -1, int(g["n_per_class"][0]),
                                                   int(g["n_per_class"][1])],
                                           running_loss=float(g["running_loss"]), n_batches=seen["steps"]))
                seen["steps"] = 0
        return local_trace

    def global_trace(frame, event, arg):
        return local_trace if frame.f_code.co_filename == REWARD_SCRIPT else None

    with tempfile.TemporaryDirectory() as root:
        # the arrays of tests/dataset_util.make_dataset, rewards rewritten as int64 (the script hands them to CrossEntropyLoss)
        arrays = ru.case_arrays(case)
        _, _, actions, rewards, starts = dataset_util.make_dataset(os.path.join(root, "check"), n_episodes=case["n_episodes"],
                                                                   ep_len=case["ep_len"], seed=case["data_seed"])
        assert np.array_equal(actions, arrays["actions"]) and np.array_equal(rewards, arrays["rewards"]) and \
            np.array_equal(starts, arrays["episode_starts"])
        with np.load(os.path.join(root, "check", "data", "tiny_test", "ground_truth.npz")) as gt:
            assert np.array_equal(gt["ground_truth_states"], arrays["ground_truth_states"])
            assert np.array_equal(gt["target_positions"], arrays["target_positions"])
        argv = ru.write_case(root, case, int_rewards=True)
        old_cwd, old_argv = os.getcwd(), list(sys.argv)
        os.chdir(root)
        out = io.StringIO()
        try:
            sys.argv = ["predict_reward.py"] + argv + ["--no-cuda"]
            th.manual_seed(case["preseed"])
            sys.settrace(global_trace)
            with contextlib.redirect_stdout(out):
                g = runpy.run_path(REWARD_SCRIPT, run_name="__main__")
        finally:
            sys.settrace(None)
            os.chdir(old_cwd)
            sys.argv = old_argv
    text = out.getvalue()
    epochs, bs = case["epochs"], case["bs"]
    assert seen["init"] is not None and len(seen["phases"]) == 2 * epochs, (seen["init"] is None, len(seen["phases"]))
    printed = re.findall(r"^(train|val) Loss: (\S+) Acc: (\S+)\nAccuracy per class: (\S+) (\S+)$", text, re.M)
    assert len(printed) == 2 * epochs, text
    best = re.search(r"^Best val Acc: (\S+)$", text, re.M)
    rec = {}
    for k in ru.KEYS:
        rec["init/" + k] = seen["init"][k].numpy()
        rec["final/" + k] = g["model"].state_dict()[k].detach().numpy()
    final = [g["model"].state_dict()[k].detach().double() for k in ru.KEYS]
    rec["final/names"] = np.array(ru.KEYS)
    rec["final/sums"] = np.array([float(t.sum()) for t in final])
    rec["final/abss"] = np.array([float(t.abs().sum()) for t in final])
    # the trained model's logits on the first validation minibatch
    idx = g["X_val"][:bs]
    st = g["states"]
    with th.no_grad():
        logits = g["model"].rewardModel(th.Tensor(st[idx, :]).float(), th.Tensor(st[idx + 1, :]).float())
    rec["eval_states/idx"] = idx.numpy()
    rec["eval_states/full"] = logits.double().numpy()
    shape = (epochs, 2)
    rec["loss"] = np.array([p["loss"] for p in seen["phases"]]).reshape(shape)
    rec["acc"] = np.array([p["acc"] for p in seen["phases"]]).reshape(shape)
    rec["acc_per_class"] = np.array([p["per_class"] for p in seen["phases"]]).reshape(shape + (2,))
    rec["counts"] = np.array([p["counts"] for p in seen["phases"]], dtype=np.int64).reshape(shape + (5,))
    for c in (0, 1):  # correct per class = accuracy per class * rows of the class (nan where the class is empty -> 0 rows)
        rec["counts"][..., 1 + c] = np.rint(np.nan_to_num(rec["acc_per_class"][..., c]) * rec["counts"][..., 3 + c])
    rec["running_loss"] = np.array([p["running_loss"] for p in seen["phases"]]).reshape(shape)
    rec["n_batches"] = np.array([p["n_batches"] for p in seen["phases"]], dtype=np.int64).reshape(shape)
    assert [p["phase"] for p in seen["phases"]] == ["train", "val"] * epochs
    rec["printed/loss"] = np.array([float(p[1]) for p in printed]).reshape(shape)
    rec["printed/acc"] = np.array([float(p[2]) for p in printed]).reshape(shape)
    rec["printed/acc_per_class"] = np.array([[float(p[3]), float(p[4])] for p in printed]).reshape(shape + (2,))
    rec["best_val_acc"] = np.array(float(g["best_acc"]))
    rec["printed/best_val_acc"] = np.array(float(best.group(1)))
    rec["phase_sizes"] = np.array([len(g["X_train"]), len(g["X_val"])], dtype=np.int64)
    rec["indices"] = g["indices"]
    assert (rec["counts"][..., 1] + rec["counts"][..., 2] == rec["counts"][..., 0]).all()
    assert np.abs(rec["printed/loss"] - rec["loss"]).max() <= 0.5001e-4
    return rec


def reward_probe_spread(th, case, rec):
    """The reference's float32 run against the float64 restatement (tests/reward_util.py) over the same minibatch order from the same
    initial parameters: its own float32-to-float64 spread, measured on the CPU."""
    import golden_util
    import reward_util as ru
    flat = ru.flatten_state_dict({k: rec["init/" + k] for k in ru.KEYS})
    states = np.asarray(ru.case_states(case), dtype=np.float32)  # the script feeds float32 rows
    labels = np.maximum(ru.case_arrays(case)["rewards"], 0).astype(np.int64)
    tables = ru.replay_tables(rec["indices"], case["seed"], case["bs"], case["epochs"])
    m, v, t = np.zeros_like(flat), np.zeros_like(flat), 0
    loss = np.zeros((case["epochs"], 2))
    for e, (train, val) in enumerate(tables):
        assert (len(train), len(val)) == tuple(rec["n_batches"][e]), (e, len(train), len(val), rec["n_batches"][e])
        flat, m, v, ph, _ = ru.fit(flat, m, v, t, states, labels, train, case["lr"])
        t += len(train)
        loss[e, 0] = ph.running_loss / rec["phase_sizes"][0]
        loss[e, 1] = ru.evaluate(flat, states, labels, val).running_loss / rec["phase_sizes"][1]
    S = states.shape[1]
    sd = {k: th.from_numpy(np.ascontiguousarray(a)) for k, a in zip(ru.KEYS, ru.unflatten(flat, S))}
    logits = ru.forward(flat, ru.rows(states, rec["eval_states/idx"]))[2]
    g = {k: rec[k] for k in ("final/names", "final/sums", "final/abss", "eval_states/full")}
    worst, _ = golden_util.endpoint_errors(sd, g, case["lr"], t, logits)
    return {"param": worst["param"], "eval_states": worst["eval_states"],
            "loss": float((np.abs(rec["loss"] - loss) / np.abs(loss)).max()), "loss_first_last": [float(rec["loss"][0, 0]),
                                                                                                  float(rec["loss"][-1, 0])]}


def reward_probe_child(path):
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)
    import reward_util as ru
    out, spread = {}, {}
    for case in ru.CASES:
        rec = reward_probe_run(th, case)
        spread[case["name"]] = reward_probe_spread(th, case, rec)
        print(case["name"], json.dumps(spread[case["name"]]), "train loss", rec["loss"][:, 0].round(4).tolist())
        assert max(spread[case["name"]][k] for k in ("param", "eval_states", "loss")) <= 1e-3, "shorten the case: the spread exceeds 1e-3"
        for k, a in rec.items():
            out["%s/%s" % (case["name"], k)] = a
    out["cases"] = np.array(json.dumps(list(ru.CASES)))
    out["torch_version"] = np.array(th.__version__)
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "reward_probe_spread.json"), "w") as f:
        json.dump({"cases": spread, "refused_above": 1e-3,
                   "metric": "the unmodified evaluation/predict_reward.py in float32 on the CPU against the float64 restatement of "
                             "tests/reward_util.py, same initial parameters, same minibatch order: param = worst tensor of "
                             "tests/golden_util.py::endpoint_errors (|sum - ref| and |abs-sum - ref| over abs-sum + lr * steps * "
                             "numel), eval_states = its measure on the trained model's logits of the first validation minibatch, "
                             "loss = max relative error of the per-epoch train and val losses"}, f, indent=1, sort_keys=True)
        f.write("\n")


def run_reward_probe_child():
    import subprocess
    import tempfile
    tmp = tempfile.mktemp(suffix=".npz")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--reward-probe-child", tmp], timeout=1500)
    with np.load(tmp, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    os.remove(tmp)
    return d


def main():
    os.makedirs(OUT, exist_ok=True)
    only = [a for a in sys.argv[1:] if not a.startswith("-")]
    if only and all(o.startswith("reward_probe") for o in only):  # a child process does all of it: nothing to import here
        d = run_reward_probe_child()
        path = os.path.join(OUT, "reward_probe.npz")
        np.savez_compressed(path, **d)
        print("wrote %-28s %6.1f KB  (%d arrays)" % ("reward_probe.npz", os.path.getsize(path) / 1024.0, len(d)))
        return
    th, ref_pre, SRLModules, RL = import_reference()

    only = [a for a in sys.argv[1:] if not a.startswith("-")]

    def save(name, fn):
        if only and not any(name.startswith(o) for o in only):
            return
        d = fn()
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        print("wrote %-28s %6.1f KB  (%d arrays)" % (name + ".npz", os.path.getsize(path) / 1024.0, len(d)))

    # (1) init KATs: same seed + same constructor order => identical parameters
    for tag, losses, C in (("ae_c3", ["autoencoder"], 3), ("vae_c3", ["vae"], 3), ("ae_c6", ["autoencoder"], 6),
                           ("cnn_c3", ["inverse"], 3)):
        save("init_" + tag, lambda: digest_state_dict(build(th, ref_pre, SRLModules, losses, C=C).state_dict()))
    # (1b) the dense models of --model-type mlp / linear (reference modules.py:53-69)
    for tag, mt, losses, C in (("mlp_ae_c3", "mlp", ["autoencoder"], 3), ("mlp_vae_c3", "mlp", ["vae"], 3),
                               ("mlp_net_c3", "mlp", ["inverse", "forward"], 3), ("linear_ae_c3", "linear", ["autoencoder"], 3),
                               ("linear_net_c3", "linear", ["inverse", "forward"], 3), ("mlp_ae_c6", "mlp", ["autoencoder"], 6)):
        save("init_" + tag, lambda: digest_state_dict(build(th, ref_pre, SRLModules, losses, C=C, model_type=mt).state_dict()))
    # (2) single train-mode steps
    save("step_ae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=2))
    save("step_ae_b4", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=4))
    save("step_vae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["vae"], B=2))
    save("step_vae_b4", lambda: step_case(th, ref_pre, SRLModules, RL, ["vae"], B=4))
    save("step_aeif_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder", "inverse", "forward"], B=2))
    save("step_aeif_mlp_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder", "inverse", "forward"], B=2,
                                       inverse="mlp"))
    save("step_ae_c6_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=2, C=6))
    save("step_vae_c6_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["vae"], B=2, C=6))
    save("step_cnn_if_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["inverse", "forward"], B=2))
    # (3) short optimisation traces (Adam, lr 1e-4)
    save("trace_ae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=2, n_steps=3, lr=1e-4))
    save("trace_vae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["vae"], B=2, n_steps=3, lr=1e-4))
    save("trace_aeif_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder", "inverse", "forward"], B=2,
                                    n_steps=3, lr=1e-4))
    # (3b) §8f-2/3: split representations (SRLModulesSplit), reward head + loss, l1/l2 regularisers, DAE inputs.
    # The first case is the reference's own stacked-model test configuration (tests/test_modules.py:8-19) at B=4.
    from collections import OrderedDict as OD
    stacked = OD([("dae", 20), ("reward", -1), ("forward", 60), ("inverse", 20)])
    stacked_w = {"dae": 1.0, "reward": 1.0, "forward": 1.0, "inverse": 5.0}
    save("step_split_dae_rfi_b4", lambda: step_case(th, ref_pre, SRLModules, RL, list(stacked.keys()), B=4, S=100, inverse="mlp",
                                            weights=stacked_w, split=stacked, l2_reg=0.0001))
    save("trace_split_dae_rfi_b4", lambda: step_case(th, ref_pre, SRLModules, RL, list(stacked.keys()), B=4, S=100, inverse="mlp",
                                             weights=stacked_w, split=stacked, l2_reg=0.0001, n_steps=3, lr=1e-4))
    vsplit = OD([("vae", 150), ("inverse", 50), ("forward", -1)])
    save("step_split_vae_if_b2", lambda: step_case(th, ref_pre, SRLModules, RL, list(vsplit.keys()), B=2, split=vsplit))
    asplit = OD([("autoencoder", 120), ("reward", 80), ("inverse", -1)])
    save("step_split_ae_ri_b2", lambda: step_case(th, ref_pre, SRLModules, RL, list(asplit.keys()), B=2, split=asplit))
    save("step_ae_reward_l1_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder", "reward"], B=2, l1_reg=1e-5))
    save("step_dae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["dae"], B=2))
    save("step_vae_perceptual_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["vae", "perceptual"], B=2,
                                             weights={"perceptual": 1.0}))
    save("detach_kats", lambda: detach_kats(th))
    # (4) per-layer forward digests, loss KATs, head KATs
    save("layers_ae_b2", lambda: layer_trace(th, ref_pre, SRLModules))
    save("loss_kats", lambda: loss_kats(th, RL))
    save("head_kats", lambda: head_kats(th, ref_pre, SRLModules))
    # (5) round 2: longer trajectories, a validation minibatch inside a trajectory, the whole learn() loop
    save("trace10_ae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=2, n_steps=10, lr=1e-4))
    save("trace10_vae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["vae"], B=2, n_steps=10, lr=1e-4))
    save("trace_val_aeif_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder", "inverse", "forward"], B=2,
                                                n_steps=4, lr=1e-4, val_steps=(1,)))
    save("trace_val_vae_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["vae"], B=2, n_steps=4, lr=1e-4,
                                               val_steps=(2,)))
    save("trace_ae_l1l2_b2", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=2, n_steps=3, lr=1e-4,
                                               l1_reg=1e-5, l2_reg=1e-4))
    # (6) round 3: a trajectory at the reference's DEFAULT minibatch (bs = 32, BASELINE.json configs[0]): with 16x the samples per
    # gradient, near-zero gradient elements (the ones Adam turns into +-lr steps of arbitrary sign) are far rarer than at B = 2,
    # so a free-running end point can be held much tighter (tests/test_trajectory_gpu.py, tools/measure_spread.py)
    save("trace10_ae_b32", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=32, n_steps=10, lr=1e-4))
    # (7) the dense models of --model-type mlp / linear (their image-sized tensors keep at most 4096 strided samples: dense_sub()): single steps, Adam traces (one with the l1 / l2 regularisers, which reach
    # the conv stacks these models build but never run)
    for tag, mt, losses, C in (("mlp_ae", "mlp", ["autoencoder"], 3), ("mlp_dae", "mlp", ["dae"], 3), ("mlp_vae", "mlp", ["vae"], 3),
                               ("linear_ae", "linear", ["autoencoder"], 3), ("mlp_if", "mlp", ["inverse", "forward"], 3),
                               ("linear_if", "linear", ["inverse", "forward"], 3), ("mlp_ae_c6", "mlp", ["autoencoder"], 6)):
        save("step_%s_b2" % tag, lambda: dense_subs(step_case(th, ref_pre, SRLModules, RL, losses, B=2, C=C, model_type=mt)))
    for tag, mt, losses in (("mlp_ae", "mlp", ["autoencoder"]), ("mlp_vae", "mlp", ["vae"]), ("linear_ae", "linear", ["autoencoder"])):
        save("trace_%s_b2" % tag, lambda: dense_subs(step_case(th, ref_pre, SRLModules, RL, losses, B=2, n_steps=3, lr=1e-4,
                                                               model_type=mt)))
    save("trace_mlp_ae_l1l2_b2", lambda: dense_subs(step_case(th, ref_pre, SRLModules, RL, ["autoencoder"], B=2, n_steps=3, lr=1e-4,
                                                              l1_reg=1e-5, l2_reg=1e-4, model_type="mlp")))
    # (8) the reward-prior and episode-prior losses (losses.py:290-359): partner draws, discriminator init, single steps, a trace
    save("prior_kats", lambda: prior_kats(th))
    save("step_if_rp_ep_b4", lambda: step_case(th, ref_pre, SRLModules, RL, ["inverse", "forward", "reward-prior", "episode-prior"],
                                               B=4))
    save("step_ae_rp_b4", lambda: step_case(th, ref_pre, SRLModules, RL, ["autoencoder", "reward-prior"], B=4))
    save("step_mlp_vae_ep_bal_b4", lambda: dense_subs(step_case(th, ref_pre, SRLModules, RL, ["vae", "episode-prior"], B=4,
                                                                model_type="mlp", balanced=True)))
    save("step_linear_if_ep_b4", lambda: dense_subs(step_case(th, ref_pre, SRLModules, RL, ["inverse", "forward", "episode-prior"],
                                                              B=4, model_type="linear")))
    rsplit = OD([("autoencoder", 120), ("inverse", 80), ("reward-prior", -1)])
    save("step_split_ae_rp_b4", lambda: step_case(th, ref_pre, SRLModules, RL, list(rsplit.keys()), B=4, split=rsplit))
    save("trace_if_rp_ep_b4", lambda: step_case(th, ref_pre, SRLModules, RL, ["inverse", "forward", "reward-prior", "episode-prior"],
                                                B=4, n_steps=4, lr=1e-4, val_steps=(2,)))
    for lname in LOOP_CASES:
        save(lname, lambda: run_loop_child(lname))
    # (9) evaluation/predict_reward.py as a script (also writes reward_probe_spread.json)
    save("reward_probe", run_reward_probe_child)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--loop-child":
        loop_child(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 3 and sys.argv[1] == "--reward-probe-child":
        reward_probe_child(sys.argv[2])
    else:
        main()
