"""The supervised baseline's dense network (reference models/supervised.py:6-28), MI355X-native.

DenseNetwork keeps the reference's constructor, parameter creation order and state_dict keys (fc1.*, fc2.*); its forward runs the HIP
blocks: fc1 + ReLU on the wide-input kernel (csrc/dense.hip, the loader's uint8 frames or the float tensor), dropout with a mask drawn
from torch's CPU generator where the reference's F.dropout draws its own (csrc/supervised.hip), fc2 on the small-GEMM kernel.
CustomCNN (reference models/supervised.py imports it from models/models.py) lives in models/models.py; the trainable ResNet-18 of
ConvolutionalNetwork is outside this build.
"""
from __future__ import print_function, division, absolute_import

import torch as th
import torch.nn as nn

from srlz import hotpath, ops
from .models import BaseModelSRL, CustomCNN  # noqa: F401


class DenseNetwork(BaseModelSRL):
    """
    Dense Neural Net for State Representation Learning (SRL)
    input shape : 3-channel RGB images of shape (3 x H x W) (to be consistent with CNN network)
    :param input_dim: (int) 3 x H x H
    :param state_dim: (int)
    :param n_hidden: (int)
    :param drop_p: (float) Dropout proba
    """

    def __init__(self, input_dim, state_dim=2, n_hidden=64, drop_p=0.5):
        super(DenseNetwork, self).__init__()
        self.fc1 = nn.Linear(input_dim, n_hidden)
        self.fc2 = nn.Linear(n_hidden, state_dim)
        self.drop_p = drop_p

    def forward(self, x, dropout_mask=None):
        """dropout_mask: (test hook, the product leaves it at None) a [B, n_hidden] tensor of zeros and ones used in place of the
        draw from torch's CPU generator."""
        hotpath.require_gpu(x, "DenseNetwork")
        h = hotpath.dense_in(self.fc1, x, ops.ACT_RELU)
        if self.training and self.drop_p > 0:
            if dropout_mask is None:
                # the reference's F.dropout draws empty_like(h).bernoulli_(1 - p) from the CPU generator at this point of the forward
                dropout_mask = th.empty(h.shape[0], h.shape[1]).bernoulli_(1 - self.drop_p)
            mask = dropout_mask.to(device=h.device, dtype=th.uint8)
            h = ops.DropoutFn.apply(h, mask, float(self.drop_p))
        return hotpath.linear(self.fc2, h)
