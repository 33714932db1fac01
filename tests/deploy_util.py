"""Shared by the deployment-encoder tests and tools/make_golden_deploy.py: closed-form BatchNorm parameters, integer-formula camera
frames, and the fp64 restatement of one eval-mode encoder block.  Nothing here touches a GPU or reads a file."""
import numpy as np
import torch

# (kernel, stride, pad) of the three block kinds and the pool pad of the reference's block of that kind (models/models.py:47-63)
GEO = {0: (7, 2, 3), 1: (3, 1, 1), 2: (3, 2, 1)}
POOL_PAD = {0: 1, 1: 0, 2: 0}
BN_EPS = 1e-5


def bn_formula(layer, channels=64):
    """(gamma, beta, running_mean, running_var) of BatchNorm `layer` as fp32 tensors: gamma negative on every fifth channel, running
    variances spread over two decades (0.1 .. 10)."""
    c = np.arange(channels)
    gamma = (0.6 + 0.05 * ((c * 7 + layer * 3) % 11)) * np.where(c % 5 == 2, -1.0, 1.0)
    beta = 0.1 * (((c * 3 + layer) % 7) - 3)
    mean = 0.05 * (((c * 5 + 2 * layer) % 9) - 4)
    var = 10.0 ** (-1.0 + 2.0 * ((c * 13 + layer) % 17) / 16.0)
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (gamma, beta, mean, var))


def set_encoder_bn(stack):
    """Write bn_formula into the three BatchNorms of an encoder stack (indices 1, 5, 9), in place."""
    with torch.no_grad():
        for layer, idx in enumerate((1, 5, 9)):
            bn = stack[idx]
            for dst, src in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), bn_formula(layer)):
                dst.copy_(src.to(dst.dtype))


def frames_nhwc(n, h, w, c):
    """uint8 [n, h, w, c] camera frames from an integer formula (no stored picture): smooth ramps plus a hash-like term."""
    i, y, x, ch = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    v = (y * 3 + x * 5 + ch * 41 + i * 67 + ((y * x + 7 * i + 13 * ch) % 29) * 4 + ((y // 7) * (x // 5)) % 31) % 256
    return v.astype(np.uint8)


def to_planar(frames):
    """[N,H,W,C] bytes -> the reference's tensor layout [N,C,W,H] (preprocessing/data_loader.py:255), contiguous."""
    return np.ascontiguousarray(np.transpose(frames, (0, 3, 2, 1)))


def pooled_size(h, pad):
    return (h + 2 * pad - 3) // 2 + 1


def out_dims(kind, hi, wi, pool_pad):
    k, s, p = GEO[kind]
    hc, wc = (hi + 2 * p - k) // s + 1, (wi + 2 * p - k) // s + 1
    return hc, wc, pooled_size(hc, pool_pad), pooled_size(wc, pool_pad)


def ref_block(x, w, scale, shift, kind, pool_pad):
    """fp64: maxpool3x3s2(relu(conv2d(x, w) * scale + shift)); x [N,C,hi,wi], w [64,C,k,k], scale / shift [64] -> [N,64,hp,wp]."""
    k, s, p = GEO[kind]
    y = torch.nn.functional.conv2d(x.double(), w.double(), stride=s, padding=p)
    z = torch.relu(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return torch.nn.functional.max_pool2d(z, kernel_size=3, stride=2, padding=pool_pad)


# The five models of the golden test: constructor arguments shared by the reference's classes (tools/make_golden_deploy.py) and this
# build's (tests/test_deploy_golden_gpu.py).  "split": ordered (loss, dimensions) pairs of SRLModulesSplit.
CASES = {
    "cnn_inverse": dict(losses=["inverse"], state_dim=3, channels=3, split=None, seed=11),
    "ae": dict(losses=["autoencoder"], state_dim=8, channels=3, split=None, seed=12),
    "vae": dict(losses=["vae"], state_dim=8, channels=3, split=None, seed=13),
    "split_ae_inverse": dict(losses=["autoencoder", "inverse"], state_dim=8, channels=3, split=[("autoencoder", 4), ("inverse", 4)], seed=14),
    "ae_c6": dict(losses=["autoencoder"], state_dim=8, channels=6, split=None, seed=15),
}
N_FRAMES, FRAME_H, FRAME_W, N_ACTIONS = 3, 224, 224, 6


def build_case(name, modules, pre):
    """The model of CASES[name] from `modules` (a models.modules: the reference's or this build's) with `pre` its
    preprocessing.preprocess: seeded construction on the CPU, then the closed-form BatchNorm parameters.  Leaves pre.N_CHANNELS at 3."""
    from collections import OrderedDict
    case = CASES[name]
    pre.N_CHANNELS = case["channels"]
    try:
        np.random.seed(case["seed"])
        torch.manual_seed(case["seed"])
        if case["split"] is None:
            m = modules.SRLModules(state_dim=case["state_dim"], action_dim=N_ACTIONS, cuda=False, model_type="custom_cnn",
                                   losses=list(case["losses"]))
        else:
            m = modules.SRLModulesSplit(state_dim=case["state_dim"], action_dim=N_ACTIONS, cuda=False, model_type="custom_cnn",
                                        losses=list(case["losses"]), split_dimensions=OrderedDict(case["split"]))
    finally:
        pre.N_CHANNELS = 3
    set_encoder_bn(m.model.conv_layers if hasattr(m.model, "conv_layers") else m.model.encoder_conv)
    return m


def case_frames(name):
    return frames_nhwc(N_FRAMES, FRAME_H, FRAME_W, CASES[name]["channels"])


def checksums(state_dict):
    """(names, sums, abs-sums) of a state_dict in fp64: what a fixture stores instead of the weights."""
    names = list(state_dict.keys())
    sums = np.array([float(v.double().sum()) for v in state_dict.values()])
    abss = np.array([float(v.double().abs().sum()) for v in state_dict.values()])
    return names, sums, abss
