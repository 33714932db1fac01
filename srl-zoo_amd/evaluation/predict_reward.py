"""Predict the reward from (state, next_state) with a small classifier: how much of the reward a representation holds
(reference evaluation/predict_reward.py).

    python -m evaluation.predict_reward --data-folder data/<dataset> [-i logs/<dataset>/<experiment>/states_rewards.npz]

The reference's command line, printed lines and bookkeeping, quirks included: negative rewards count as 0, the 20 % / 80 % split of
the samples whose successor continues the episode (sklearn's train_test_split), the model built BEFORE the seeds are set, the
minibatch order of torch's own DataLoader objects, minibatches shorter than -bs skipped while the epoch's loss and accuracy are
divided by the full phase size, `Epoch k/n` counting to n - 1, nan for a class without rows.

What differs is where the work runs.  The reference launches about 30 small kernels per minibatch; here the states and labels are
uploaded once, an epoch's minibatch table is uploaded per phase, and the whole training phase is ONE launch
(srlz.ops.reward_probe_fit: forward, cross-entropy, backward, Adam and the statistics of every step, the parameters kept on chip),
the whole validation phase ONE more (srlz.ops.reward_probe_eval).  DESIGN.md §3.11.

Departures from the reference:
  * labels are cast to int64 before use (the reference hands float rewards to CrossEntropyLoss and fails with "expected scalar
    type Long but found Double" under current torch); a class index outside [0, 2) raises the ValueError of learn()'s reward head;
  * --no-cuda, or a machine without a GPU, raises: this build has no CPU fallback;
  * BaseRewardModel (models/forward_inverse.py) is the parameter container only — its layers are created in the reference's order
    (same RNG draws, same state_dict keys reward_net.{0,2,4}.{weight,bias}) and receive the trained values at the end.
"""
from __future__ import print_function, division, absolute_import

import argparse
import time
from collections import OrderedDict

import numpy as np
import torch as th
from torch.utils.data import TensorDataset, DataLoader

from models.forward_inverse import BaseRewardModel
from srlz import ops
from srlz._cabi import SrlzError
from utils import parseDataFolder, loadData

PHASES = ('train', 'val')


def build_parser():
    parser = argparse.ArgumentParser(description='Predict Reward from Ground Truth')
    parser.add_argument('--epochs', type=int, default=10, help='number of epochs to train (default: 10)')
    parser.add_argument('--seed', type=int, default=1, help='random seed (default: 1)')
    parser.add_argument('-bs', '--batch-size', type=int, default=32, help='batch_size (default: 256)')
    parser.add_argument('--training-set-size', type=int, default=-1,
                        help='Limit size (number of samples) of the training set (default: -1)')
    parser.add_argument('-lr', '--learning-rate', type=float, default=0.005, help='learning rate (default: 0.005)')
    parser.add_argument('--no-cuda', action='store_true', default=False, help='disables CUDA training')
    parser.add_argument('--data-folder', type=str, default="", help='Dataset folder', required=True)
    parser.add_argument('-i', '--input-file', type=str, default="", help='Path to a npz file containing states and rewards')
    return parser


def requireGpu(args):
    if args.no_cuda or not th.cuda.is_available():
        raise SrlzError("predict_reward runs on the GPU only ({}): the srl-zoo_amd build has no CPU fallback".format(
            "--no-cuda was given" if args.no_cuda else "torch.cuda.is_available() is False"))


def rewardClasses(rewards):
    """Rewards as stored -> class indices: negative rewards count as 0 (the reference predicts only positive or null rewards), then
    the int64 cast CrossEntropyLoss needs.  The class must lie in [0, 2)."""
    rewards = np.array(rewards).copy()
    rewards[rewards < 0] = 0
    classes = th.from_numpy(np.ascontiguousarray(rewards)).long().numpy()
    if classes.size and (classes.min() < 0 or classes.max() > 1):
        raise ValueError("the reward head has two classes: after mapping -1 to 0 and truncating to int64 (reference "
                         "learner.py:444-449) rewards must fall in [0, 2), found classes {}".format(sorted(set(classes.tolist()))))
    return classes


def prepare(args):
    """Everything the reference does before its model exists: the dataset, the states, the truncation, the sample indices.
    :return: (states [N, S], classes int64 [N'], indices int64) — host arrays, no GPU involved"""
    print('Loading data ... ')
    training_data, _, true_states, _ = loadData(parseDataFolder(args.data_folder))
    rewards, episode_starts = training_data['rewards'], training_data['episode_starts']
    classes = rewardClasses(rewards)
    if args.input_file != "":
        print("Loading {}...".format(args.input_file))
        states = np.load(args.input_file)['states']
    else:
        print("Using ground truth")
        states = true_states
    if args.training_set_size > 0:
        limit = min(args.training_set_size, len(states))
        classes, states, episode_starts = classes[:limit], states[:limit], episode_starts[:limit]
    num_samples = classes.shape[0] - 1
    print("{} samples".format(num_samples))
    # indices for all time steps where the episode continues
    indices = np.array([i for i in range(num_samples) if not episode_starts[i + 1]], dtype='int64')
    return states, classes, indices


def splitIndices(indices, seed):
    from sklearn.model_selection import train_test_split
    X_train, X_val = train_test_split(indices, test_size=0.8, random_state=seed)
    return th.from_numpy(X_train), th.from_numpy(X_val)


def makeLoaders(X_train, X_val, batch_size):
    """The reference's own loader objects: their RNG draws give the minibatch order."""
    datasets = {'train': TensorDataset(X_train), 'val': TensorDataset(X_val)}
    return datasets, {'train': DataLoader(datasets['train'], batch_size=batch_size, shuffle=True),
                      'val': DataLoader(datasets['val'], batch_size=batch_size, shuffle=False)}


def phaseTable(loader, batch_size):
    """One pass over a loader -> the phase's minibatch table, int32 [full minibatches, batch_size] on the host; a minibatch
    shorter than batch_size is skipped as the reference skips it (it is still drawn)."""
    full = [idx[0] for idx in loader if len(idx[0]) >= batch_size]
    if not full:
        return th.empty((0, batch_size), dtype=th.int32)
    return th.stack(full).to(th.int32).contiguous()


def flatParameters(model):
    """reward_net's parameters as one float32 vector in state_dict order."""
    return th.cat([p.detach().reshape(-1) for p in model.reward_net.parameters()]).float().contiguous()


def storeParameters(model, flat):
    o = 0
    with th.no_grad():
        for p in model.reward_net.parameters():
            p.copy_(flat[o:o + p.numel()].view_as(p))
            o += p.numel()


class ProbeResult(object):
    def __init__(self, records, best_acc, model, initial_state):
        self.records, self.best_acc, self.model, self.initial_state = records, best_acc, model, initial_state


def run(args):
    requireGpu(args)
    states, classes, indices = prepare(args)
    state_dim = states.shape[1]

    # the model exists BEFORE the seeds are set, as in the reference: its initial values come from the caller's RNG state
    model = BaseRewardModel()
    model.initRewardNet(state_dim, n_rewards=2, n_hidden=4)
    initial_state = OrderedDict((k, v.detach().clone()) for k, v in model.state_dict().items())
    num_epochs = args.epochs

    np.random.seed(args.seed)
    th.manual_seed(args.seed)
    th.cuda.manual_seed(args.seed)

    X_train, X_val = splitIndices(indices, args.seed)
    datasets, dataloaders = makeLoaders(X_train, X_val, args.batch_size)

    n = min(len(states), len(classes))
    data = ops.reward_probe_data(np.asarray(states[:n]), classes[:n])
    device = data.states.device
    params = flatParameters(model).to(device)
    m, v = th.zeros_like(params), th.zeros_like(params)
    steps_done = 0

    start_time = time.time()
    best_acc = 0.0
    records = []
    for epoch in range(num_epochs):
        print('Epoch {}/{}'.format(epoch + 1, num_epochs - 1))
        print('-' * 10)
        record = {'epoch': epoch}
        for phase in PHASES:
            table = phaseTable(dataloaders[phase], args.batch_size)
            running_loss, counts = ops.reward_probe_stats(device)
            if len(table):
                if phase == 'train':
                    ops.reward_probe_fit(data, table, params, m, v, steps_done, args.learning_rate, running_loss, counts)
                    steps_done += len(table)
                else:
                    ops.reward_probe_eval(data, table, params, running_loss, counts)
            running_loss = float(running_loss.item())
            counts = counts.cpu().numpy()
            epoch_loss = running_loss / len(datasets[phase])
            epoch_acc = float(counts[0]) / len(datasets[phase])
            with np.errstate(divide='ignore', invalid='ignore'):
                per_class = [np.float64(counts[1 + c]) / np.float64(counts[3 + c]) for c in range(2)]
            print('{} Loss: {:.4f} Acc: {:.4f}'.format(phase, epoch_loss, epoch_acc))
            print("Accuracy per class: {:.4f} {:.4f}".format(per_class[0], per_class[1]))
            record[phase] = {'loss': epoch_loss, 'acc': epoch_acc, 'acc_per_class': [float(a) for a in per_class],
                             'running_loss': running_loss, 'counts': [int(c) for c in counts], 'n_batches': int(len(table)),
                             'n_samples': len(datasets[phase])}
            if phase == 'val' and epoch_acc > best_acc:
                best_acc = epoch_acc
        records.append(record)
        print()

    storeParameters(model, params.cpu())
    time_elapsed = time.time() - start_time
    print('Training complete in {:.0f}m {:.0f}s'.format(time_elapsed // 60, time_elapsed % 60))
    print('Best val Acc: {:4f}'.format(best_acc))
    return ProbeResult(records, best_acc, model, initial_state)


def main(argv=None, full=False):
    """:return: the per-epoch records ({'epoch', 'train': {...}, 'val': {...}}), or the whole ProbeResult (records, best_acc, the
    trained model, its initial state_dict) with full=True"""
    result = run(build_parser().parse_args(argv))
    return result if full else result.records


if __name__ == '__main__':
    main()
