"""Shared by the deployment-decoder tests and tools/make_golden_decode.py: the decoder's closed-form BatchNorm parameters, states from
an integer formula, the fp64 restatement of the eval-mode decoder (per layer and from a state_dict) and the byte expression in numpy.
Nothing here touches a GPU or reads a file."""
import numpy as np
import torch

import deploy_util as du

CASES = ("ae", "vae", "split_ae_inverse", "ae_c6")  # the models of deploy_util.CASES that own a decoder
N_STATES = 3
DEC_BN = (1, 4, 7, 10)   # BatchNorms of decoder_conv (models/models.py:65-83)
DEC_CONV = (0, 3, 6, 9, 12)
BN_EPS = du.BN_EPS
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
# golden lattice: the four outermost rows / columns at every edge (ConvTranspose borders have fewer taps) and every 13th in between
LATTICE = np.array(list(range(4)) + list(range(8, 220, 13)) + list(range(220, 224)))


def set_decoder_bn(stack):
    """Write deploy_util.bn_formula(3..6) into the four BatchNorms of a decoder stack, in place."""
    with torch.no_grad():
        for layer, idx in enumerate(DEC_BN):
            bn = stack[idx]
            for dst, src in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), du.bn_formula(3 + layer)):
                dst.copy_(src.to(dst.dtype))


def build_case(name, modules, pre):
    """deploy_util.build_case plus the decoder's closed-form BatchNorm parameters."""
    m = du.build_case(name, modules, pre)
    set_decoder_bn(m.model.decoder_conv)
    return m


def states(n, s):
    """fp32 [n, s]: z[i][j] = 0.5 * (((5 i + 3 j) mod 7) - 3)."""
    i, j = np.meshgrid(np.arange(n), np.arange(s), indexing="ij")
    return (0.5 * (((5 * i + 3 * j) % 7) - 3)).astype(np.float32)


def case_states(name):
    return states(N_STATES, du.CASES[name]["state_dim"])


def ref_block(x, w, b, scale, shift):
    """fp64: relu((conv_transpose2d(x, w, stride 2) + b) * scale + shift); x [N,64,hi,wi], w [64,64,3,3] -> [N,64,2hi+1,2wi+1]."""
    y = torch.nn.functional.conv_transpose2d(x.double(), w.double(), b.double(), stride=2)
    return torch.relu(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))


def ref_out(x, w, b):
    """fp64: conv_transpose2d(x, w, stride 2) + b; x [N,64,hi,wi], w [64,C,4,4] -> [N,C,2hi+2,2wi+2]."""
    return torch.nn.functional.conv_transpose2d(x.double(), w.double(), b.double(), stride=2)


def ref_decode(state_dict, z):
    """fp64 restatement of the eval-mode decoder from a state_dict (any wrapper prefix): Linear, view [N,64,6,6], four blocks with the
    running statistics as an affine, the 4x4 layer -> [N,C,W,H] float64."""
    pre = [k[:-len("decoder_fc.0.weight")] for k in state_dict if k.endswith("decoder_fc.0.weight")]
    assert len(pre) == 1, pre
    sd = {k[len(pre[0]):]: v.detach().double().cpu() for k, v in state_dict.items() if k.startswith(pre[0])}
    z = torch.as_tensor(z).double()
    h = torch.nn.functional.linear(z, sd["decoder_fc.0.weight"], sd["decoder_fc.0.bias"]).view(z.shape[0], 64, 6, 6)
    for ci, bi in zip(DEC_CONV[:4], DEC_BN):
        p = "decoder_conv.%d." % bi
        scale = sd[p + "weight"] / torch.sqrt(sd[p + "running_var"] + BN_EPS)
        shift = sd[p + "bias"] - sd[p + "running_mean"] * scale
        h = ref_block(h, sd["decoder_conv.%d.weight" % ci], sd["decoder_conv.%d.bias" % ci], scale, shift)
    return ref_out(h, sd["decoder_conv.12.weight"], sd["decoder_conv.12.bias"])


def denormalize64(decoded):
    """fp64 [N,C,W,H] -> d * std[c % 3] + mean[c % 3], unclipped (numpy float64)."""
    d = np.asarray(decoded, np.float64)
    c = d.shape[1]
    std = STD.astype(np.float64)[np.arange(c) % 3].reshape(1, c, 1, 1)
    mean = MEAN.astype(np.float64)[np.arange(c) % 3].reshape(1, c, 1, 1)
    return d * std + mean


def bytes_expr(decoded32, layout="planar", bgr=False):
    """The byte expression on an fp32 decode tensor [N,C,W,H], in numpy fp32: v = clip(d * std + mean, 0, 1) with product and sum
    rounded separately, byte = rint(v * 255), NaN -> 0.  "planar": uint8 [N,C,W,H]; "nhwc": [N,H,W,C] (byte (n,y,x,c) =
    decoded[n][c][x][y]); bgr reverses the three channels of each camera."""
    d = np.asarray(decoded32)
    assert d.dtype == np.float32
    c = d.shape[1]
    v = d * STD[np.arange(c) % 3].reshape(1, c, 1, 1)
    v = v + MEAN[np.arange(c) % 3].reshape(1, c, 1, 1)
    with np.errstate(invalid="ignore"):
        v = np.clip(v, np.float32(0), np.float32(1))
        r = np.rint(v * np.float32(255))
    b = np.where(np.isnan(r), np.float32(0), r).astype(np.uint8)
    if bgr:
        b = b[:, [3 * (i // 3) + 2 - i % 3 for i in range(c)]]
    return np.ascontiguousarray(b.transpose(0, 3, 2, 1)) if layout == "nhwc" else np.ascontiguousarray(b)


def plane_sums(decoded64):
    """fp64 (sum, sum of squares) of every (image, channel) plane: [N,C] each."""
    d = np.asarray(decoded64, np.float64)
    return d.sum(axis=(2, 3)), (d * d).sum(axis=(2, 3))


def lattice(decoded):
    d = np.asarray(decoded)
    return d[:, :, LATTICE][:, :, :, LATTICE]
