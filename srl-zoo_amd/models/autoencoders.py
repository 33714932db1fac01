"""Auto-encoders of the reference (models/autoencoders.py): CNNAutoEncoder — conv encoder + Linear(2304, S), Linear(S, 2304) + conv
decoder (autoencoders.py:84-118) — and the dense ones of `--model-type linear | mlp`, LinearAutoEncoder (autoencoders.py:6-37) and
DenseAutoEncoder (autoencoders.py:40-81), whose wide layers (input_dim = C * 224 * 224 in or out) run on csrc/dense.hip.

The dense models inherit BaseModelAutoEncoder as in the reference: its conv stacks are built (they consume the RNG, sit in the
state_dict and in the regularisers' parameter list) but never run.
"""
from __future__ import print_function, division, absolute_import

import torch.nn as nn

from .models import BaseModelAutoEncoder
from srlz import hotpath, ops


class CNNAutoEncoder(BaseModelAutoEncoder):
    """:param state_dim: (int)"""

    def __init__(self, state_dim=3):
        super(CNNAutoEncoder, self).__init__()
        self.encoder_fc = nn.Sequential(nn.Linear(6 * 6 * 64, state_dim))
        self.decoder_fc = nn.Sequential(nn.Linear(state_dim, 6 * 6 * 64))

    def encode(self, x):
        return hotpath.linear(self.encoder_fc[0], self._encodeConv(x))

    def decode(self, x):
        return self._decodeConv(hotpath.linear(self.decoder_fc[0], x))


class LinearAutoEncoder(BaseModelAutoEncoder):
    """Linear(input_dim, S) / Linear(S, input_dim).
    :param input_dim: (int)
    :param state_dim: (int)"""

    def __init__(self, input_dim, state_dim=3):
        super(LinearAutoEncoder, self).__init__()
        self.encoder = nn.Sequential(nn.Linear(input_dim, state_dim))
        self.decoder = nn.Sequential(nn.Linear(state_dim, input_dim))

    def encode(self, x):
        return hotpath.dense_in(self.encoder[0], x)

    def decode(self, x):
        return hotpath.dense_out(self.decoder[0], x)


class DenseAutoEncoder(BaseModelAutoEncoder):
    """Linear(input_dim, 50)-Tanh-Linear(50, 50)-Tanh-Linear(50, S) / Linear(S, 50)-Tanh-Linear(50, 50)-Tanh-Linear(50, input_dim).
    :param input_dim: (int)
    :param state_dim: (int)"""

    def __init__(self, input_dim, state_dim=3):
        super(DenseAutoEncoder, self).__init__()
        self.encoder = nn.Sequential(nn.Linear(input_dim, 50), nn.Tanh(), nn.Linear(50, 50), nn.Tanh(), nn.Linear(50, state_dim))
        self.decoder = nn.Sequential(nn.Linear(state_dim, 50), nn.Tanh(), nn.Linear(50, 50), nn.Tanh(), nn.Linear(50, input_dim))

    def encode(self, x):
        e = self.encoder
        h = hotpath.dense_in(e[0], x, ops.ACT_TANH)
        h = hotpath.tanh(hotpath.linear(e[2], h))
        return hotpath.linear(e[4], h)

    def decode(self, x):
        d = self.decoder
        h = hotpath.tanh(hotpath.linear(d[0], x))
        h = hotpath.tanh(hotpath.linear(d[2], h))
        return hotpath.dense_out(d[4], h)
