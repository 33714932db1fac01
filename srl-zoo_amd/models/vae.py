"""VAEs of the reference (models/vae.py): CNNVAE — conv encoder + two Linear(2304, S) heads (mu, logvar), Linear(S, 2304) + conv
decoder (vae.py:43-75) — and DenseVAE (vae.py:6-40) of `--model-type mlp`, whose wide layers run on csrc/dense.hip."""
from __future__ import print_function, division, absolute_import

import torch.nn as nn

from .models import BaseModelVAE
from srlz import hotpath, ops


class CNNVAE(BaseModelVAE):
    """:param state_dim: (int)"""

    def __init__(self, state_dim=3):
        super(CNNVAE, self).__init__()
        self.encoder_fc1 = nn.Linear(6 * 6 * 64, state_dim)
        self.encoder_fc2 = nn.Linear(6 * 6 * 64, state_dim)
        self.decoder_fc = nn.Sequential(nn.Linear(state_dim, 6 * 6 * 64))

    def encode(self, x, stat_sink=None):
        e = self._encodeConv(x, stat_sink)
        return hotpath.linear(self.encoder_fc1, e), hotpath.linear(self.encoder_fc2, e)

    def decode(self, z):
        return self._decodeConv(hotpath.linear(self.decoder_fc[0], z))


class DenseVAE(BaseModelVAE):
    """fc1 Linear(input_dim, 50) + ReLU -> fc21, fc22 Linear(50, S) (mu, logvar); decoder Linear(S, 50)-ReLU-Linear(50, 50)-ReLU-
    Linear(50, input_dim).  The conv stacks of BaseModelAutoEncoder are built (RNG, state_dict) but never run.
    :param input_dim: (int)
    :param state_dim: (int)"""

    def __init__(self, input_dim, state_dim=3):
        super(DenseVAE, self).__init__()
        self.input_dim = input_dim
        self.encoder_fc1 = nn.Linear(input_dim, 50)
        self.encoder_fc21 = nn.Linear(50, state_dim)
        self.encoder_fc22 = nn.Linear(50, state_dim)
        self.decoder = nn.Sequential(nn.Linear(state_dim, 50), nn.ReLU(), nn.Linear(50, 50), nn.ReLU(), nn.Linear(50, input_dim))
        self.relu = nn.ReLU()
        self.sigmoid = nn.Sigmoid()

    def encode(self, x, stat_sink=None):
        h = hotpath.dense_in(self.encoder_fc1, x, ops.ACT_RELU)
        h21, h22 = ops.fan_out(h, 2)
        return hotpath.linear(self.encoder_fc21, h21), hotpath.linear(self.encoder_fc22, h22)

    def decode(self, z):
        d = self.decoder
        h = hotpath.linear(d[0], z, relu=True)
        h = hotpath.linear(d[2], h, relu=True)
        return hotpath.dense_out(d[4], h)

    def getStates(self, observations):
        # the reference re-encodes (learner.py:402); without BatchNorm that second pass only repeats mu: the forward's mu is handed out
        # (its fan-out routes the heads' gradient into the encoder as the second pass would)
        if self.training:
            for i, (x_ref, mu, _, _) in enumerate(self._recent):
                if x_ref is observations and x_ref._version == self._recent_versions[i]:
                    return mu
        return self.encode(observations)[0]
