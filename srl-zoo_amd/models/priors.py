"""The plain dense encoders of the reference's models/priors.py (module name kept for the plugin surface): SRLDenseNetwork
(priors.py:71-102) and SRLLinear (priors.py:105-125), the `--model-type mlp | linear` models of the losses that need no decoder
(inverse / forward / reward).  Their nn.Linear(input_dim, .) runs on csrc/dense.hip.  Also the episode prior's Discriminator and
ReverseLayerF (priors.py:129-175): the discriminator holds the parameters, its forward and backward run inside ops.EpisodePriorFn
(csrc/priors.hip).  The robotic-priors loss (`priors`) is losses.losses.roboticPriorsLoss on csrc/robotic.hip and is fitted on a
recording by srlz/priorsfit.py; the trainer still rejects `--losses priors`."""
from __future__ import print_function, division, absolute_import

import torch as th
import torch.nn as nn

from .models import BaseModelSRL
from srlz import hotpath, ops


class GaussianNoiseVariant(nn.Module):
    """x + N(mean, std) drawn anew at every training-mode call (reference models/custom_layers.py:31-51); identity in eval mode.
    The noise is drawn on the device by torch's generator, one draw per model call of a batched pair (as the VAE's eps)."""

    def __init__(self, device, std, mean=0):
        super(GaussianNoiseVariant, self).__init__()
        self.std = std
        self.mean = mean
        self.device = device

    def forward(self, x):
        if self.training:
            noise = th.empty_like(x)
            for part in noise.chunk(ops.cur_groups(True)):
                part.normal_(self.mean, std=self.std)
            return ops.AddConstFn.apply(x, noise)
        return x


class SRLDenseNetwork(BaseModelSRL):
    """Linear(input_dim, n_hidden)-ReLU-Linear(n_hidden, S) + GaussianNoiseVariant(noise_std) in training.
    :param input_dim: (int) C * H * W
    :param state_dim: (int)
    :param cuda: (bool)
    :param n_hidden: (int)
    :param noise_std: (float) to avoid NaN (states must be different)"""

    def __init__(self, input_dim, state_dim=2, cuda=False, n_hidden=64, noise_std=1e-6):
        super(SRLDenseNetwork, self).__init__()
        self.fc = nn.Sequential(nn.Linear(input_dim, n_hidden), nn.ReLU(), nn.Linear(n_hidden, state_dim))
        self.device = th.device("cuda" if th.cuda.is_available() and cuda else "cpu")
        self.fc = self.fc.to(self.device)
        self.noise = GaussianNoiseVariant(self.device, noise_std)

    def forward(self, x):
        h = hotpath.dense_in(self.fc[0], x, ops.ACT_RELU)
        x = hotpath.linear(self.fc[2], h)
        if self.training:
            x = self.noise(x)
        return x


class SRLLinear(BaseModelSRL):
    """Linear(input_dim, S).
    :param input_dim: (int) C * H * W
    :param state_dim: (int)
    :param cuda: (bool)"""

    def __init__(self, input_dim, state_dim=2, cuda=False):
        super(SRLLinear, self).__init__()
        self.fc = nn.Linear(input_dim, state_dim)
        self.device = th.device("cuda" if th.cuda.is_available() and cuda else "cpu")
        self.fc = self.fc.to(self.device)

    def forward(self, x):
        return hotpath.dense_in(self.fc, x)


ReverseLayerF = ops.ReverseLayerF  # (reference priors.py:129-152: identity forward, -lambda * gradient backward)


class Discriminator(nn.Module):
    """Linear(input_dim, 64)-ReLU-Linear(64, 64)-ReLU-Linear(64, 1)-Sigmoid (reference priors.py:155-175), same keys (net.0 / net.2 /
    net.4) and the same initialisation order.  Parameters only: episodePriorLoss evaluates it through ops.EpisodePriorFn, which
    gathers its input pairs, runs the three layers and the BCE in one launch.
    :input_dim: (int) input_dim = 2 * state_dim"""

    def __init__(self, input_dim):
        super(Discriminator, self).__init__()
        self.net = nn.Sequential(
            nn.Linear(input_dim, 64),
            nn.ReLU(inplace=True),
            nn.Linear(64, 64),
            nn.ReLU(inplace=True),
            nn.Linear(64, 1),
            nn.Sigmoid()
        )

    def params(self):
        """(w1, b1, w2, b2, w3, b3), the order ops.EpisodePriorFn takes them in."""
        return (self.net[0].weight, self.net[0].bias, self.net[2].weight, self.net[2].bias, self.net[4].weight, self.net[4].bias)

    def forward(self, x):
        raise NotImplementedError("Discriminator runs inside the episode-prior loss (ops.EpisodePriorFn, csrc/priors.hip); "
                                  "call losses.losses.episodePriorLoss")
