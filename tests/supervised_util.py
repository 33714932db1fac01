"""Inputs of the supervised baseline's fixtures, shared by tools/make_golden_supervised.py and the tests: ONE frame per sample
(the `obs` half of golden_util.golden_inputs) and ground-truth states drawn from a seed.  Nothing is stored."""
import numpy as np

import golden_util as gu

STATE_DIM = 3  # the generated dataset's ground-truth states (tests/dataset_util.py)


def sup_inputs(B, seed, S=STATE_DIM):
    """(obs float32 [B, 3, 224, 224] in the reference's tensor layout, target states float32 [B, S])."""
    obs = gu.synthetic_obs(B, 3, seed)[0]
    targets = np.random.RandomState(seed + 11).randn(B, S).astype(np.float32)
    return obs, targets


def best_epoch(val_losses):
    """The epoch the reference checkpoints (srl_baselines/supervised.py:124-129): the first strict minimum of the epoch's mean
    validation loss, accumulated as the loop does."""
    best, best_error = -1, np.inf
    for epoch, values in enumerate(val_losses):
        val_loss = 0
        for v in values:
            val_loss += float(v)
        val_loss /= len(values)
        if val_loss < best_error:
            best, best_error = epoch, val_loss
    return best
