"""The supervised-learning baseline (reference srl_baselines/supervised.py:29-235), MI355X-native: an encoder regressed onto the
ground-truth states with an MSE loss — the number every other method is compared against.

    python -m srl_baselines.supervised --data-folder <dataset> --model-type custom_cnn --no-display-plots

Constructor arguments, module-level knobs, command line, log folder and the files written are the reference's.  Underneath, the
forward / backward run as HIP kernels (srlz/): ONE frame per sample and one BatchNorm group (no pair), the loss and its gradient in
one launch (srlz_mse_target_fwd), Adam fused over one flat parameter buffer; the validation pass runs in eval mode without gradients,
as the reference's does.  The minibatches are ragged (the last one of an epoch is shorter).
--model-type resnet (the reference's default: a trainable ResNet-18) is outside this build; there is no CPU path and no plotting.
"""
from __future__ import print_function, division, absolute_import

import argparse
import time
from collections import OrderedDict

import numpy as np
import torch as th

from models import DenseNetwork, CustomCNN
from models.learner import BaseLearner, _DeviceFeed, _requireGpu
from pipeline import saveConfig
from preprocessing.data_loader import SupervisedDataLoader
from preprocessing.preprocess import getInputDim
from srlz import hotpath, ops, optim
from utils import parseDataFolder, createFolder, loadData, buildConfig, printYellow

DISPLAY_PLOTS = True
EPOCH_FLAG = 1  # print every epoch
BATCH_SIZE = 32
TEST_BATCH_SIZE = 256
N_EPOCHS = 50  # (the command line's default; the reference binds it in its __main__ block only)
VALIDATION_SIZE = 0.33
# The reference builds its training loader with shuffle=True (srl_baselines/supervised.py:76-77), but the base DataLoader constructor
# runs after SupervisedDataLoader has stored the flag and resets it to is_training = False (preprocessing/data_loader.py:96,306-308):
# the reference trains on the minibatches IN ORDER, every epoch.  False follows it (and the fixtures recorded from it); True gives the
# per-epoch np.random.permutation the reference asks for.
SHUFFLE_MINIBATCHES = False


def trainValSplit(n_samples, seed, test_size=VALIDATION_SIZE):
    """(train indices, validation indices) of sklearn.model_selection.train_test_split(np.arange(n), ..., test_size=0.33,
    random_state=seed) (reference srl_baselines/supervised.py:73-74) without sklearn: one RandomState(seed).permutation, the test part
    first, n_test = ceil(test_size * n)."""
    n_test = int(np.ceil(test_size * n_samples))
    n_train = n_samples - n_test
    if n_train < 1 or n_test < 1:
        raise ValueError("With n_samples={} and test_size={} the train or the validation set would be empty".format(
            n_samples, test_size))
    permutation = np.random.RandomState(seed).permutation(n_samples)
    return permutation[n_test:n_test + n_train], permutation[:n_test]


class SupervisedLearning(BaseLearner):
    """
    :param state_dim: (int)
    :param model_type: (str) one of "custom_cnn" ("cnn") or "mlp" ("resnet" is outside this build)
    :param log_folder: (str)
    :param seed: (int)
    :param learning_rate: (float)
    :param cuda: (bool)
    """

    def __init__(self, state_dim, model_type="resnet", log_folder="logs/default",
                 seed=1, learning_rate=0.001, cuda=False):
        super(SupervisedLearning, self).__init__(state_dim, BATCH_SIZE, seed, cuda)

        if model_type == "resnet":
            raise NotImplementedError("model_type 'resnet' (the trainable ResNet-18 of ConvolutionalNetwork) is outside this build: "
                                      "use 'custom_cnn' or 'mlp'")
        elif model_type in ["cnn", "custom_cnn"]:
            self.model = CustomCNN(self.state_dim)
        elif model_type == "mlp":
            self.model = DenseNetwork(getInputDim(), self.state_dim)
        else:
            raise ValueError("Unknown model: {}".format(model_type))
        print("Using {} model".format(model_type))

        _requireGpu(cuda)
        if optim.world()[1] > 1:
            raise RuntimeError("the supervised baseline runs as a single process (world size {})".format(optim.world()[1]))
        self.device = th.device("cuda", th.cuda.current_device())
        self.model = self.model.to(self.device)
        self.model_type = model_type
        ops.norm_lut(self.device)
        self.flat_params = optim.FlatParams(self.model)
        self.optimizer = optim.FusedAdam(self.flat_params, lr=learning_rate)  # (torch.optim.Adam defaults)
        self.log_folder = log_folder
        self.read_bytes = True  # (False: every step gets the normalised float tensor; tests compare the two routes)

    def _readsBytes(self):
        """The only reader of the observations is conv1 (ops.EncInFn) / fc1 (ops.DenseInFn): the loader's bytes go in as they are."""
        return self.read_bytes and hotpath.input_reads_bytes(dense=self.model_type == "mlp")

    def _observations(self, frames):
        frames = frames.to(self.device, non_blocking=True)
        if ops.is_u8_frames(frames) and not (self._isPlanar(frames) and self._readsBytes()):
            return self._toDevice(frames)
        return frames

    def trainStep(self, obs, target_states):
        """One training minibatch (reference srl_baselines/supervised.py:98-105): forward in train mode, zero_grad, MSE, backward,
        Adam.  Returns the loss as a 0-dim device tensor."""
        self.model.train()
        pred_states = self.model(self._observations(obs))
        self.optimizer.zero_grad()
        loss = ops.mse_target(pred_states, target_states.to(self.device).detach())
        loss.backward()
        self.optimizer.step()
        self.last_pred_states = pred_states.detach()  # (of the parameters BEFORE the update, as the reference's pred_states)
        return loss.detach()

    def validationStep(self, obs, target_states):
        """One validation minibatch (reference :113-122): eval mode, no gradients, forward and loss only."""
        self.model.eval()
        with th.no_grad():
            self.last_pred_states = self.model(self._observations(obs))
            return ops.mse_target(self.last_pred_states, target_states.to(self.device))

    def saveModel(self, path):
        """th.save(state_dict) with the reference's keys and NCHW shapes, CPU tensors."""
        th.save(OrderedDict((k, v.detach().cpu().clone()) for k, v in self.model.state_dict().items()), path)

    def learn(self, true_states, images_path, rewards):
        """
        Learn a state representation
        :param images_path: (numpy 1D array)
        :param true_states: (np.ndarray)
        :param rewards: (numpy 1D array)
        :return: (np.ndarray) the learned states for the given observations
        """
        true_states = true_states.astype(np.float32)
        x_indices = np.arange(len(true_states)).astype(np.int64)

        # Split into train/validation set
        train_idx, val_idx = trainValSplit(len(x_indices), self.seed)
        x_train, x_val, y_train, y_val = x_indices[train_idx], x_indices[val_idx], true_states[train_idx], true_states[val_idx]

        train_loader = SupervisedDataLoader(x_train, y_train, images_path, batch_size=BATCH_SIZE, max_queue_len=4,
                                            shuffle=SHUFFLE_MINIBATCHES)
        val_loader = SupervisedDataLoader(x_val, y_val, images_path, batch_size=TEST_BATCH_SIZE, max_queue_len=1, shuffle=False)
        data_loader = SupervisedDataLoader(x_indices, true_states, images_path, no_targets=True, batch_size=TEST_BATCH_SIZE,
                                           max_queue_len=1, shuffle=False)
        printYellow("supervised: plotting is out of scope of the MI355X hot-path build: nothing is drawn, learned_states.png is not written")

        best_error = np.inf
        best_model_path = "{}/srl_supervised_model.pth".format(self.log_folder)
        self.best_epoch = -1

        start_time = time.time()
        epoch_train_loss = [[] for _ in range(N_EPOCHS)]
        epoch_val_loss = [[] for _ in range(N_EPOCHS)]
        try:
            for epoch in range(N_EPOCHS):
                train_loss, val_loss = 0, 0
                feed = _DeviceFeed(train_loader, self.device)
                for obs, target_states in feed:
                    loss = self.trainStep(obs, target_states)
                    feed.advance()  # the next minibatch's H2D copy overlaps this step
                    value = loss.item()
                    train_loss += value
                    epoch_train_loss[epoch].append(value)
                train_loss /= len(train_loader)

                for obs, target_states in _DeviceFeed(val_loader, self.device):
                    value = self.validationStep(obs, target_states).item()
                    val_loss += value
                    epoch_val_loss[epoch].append(value)
                val_loss /= len(val_loader)

                # Save best model
                if val_loss < best_error:
                    best_error = val_loss
                    self.best_epoch = epoch
                    self.saveModel(best_model_path)

                if (epoch + 1) % EPOCH_FLAG == 0:
                    print("Epoch {:3}/{}".format(epoch + 1, N_EPOCHS))
                    print("train_loss:{:.4f} val_loss:{:.4f}".format(train_loss, val_loss))
                    print("{:.2f}s/epoch".format((time.time() - start_time) / (epoch + 1)))

            # Load best model before predicting states
            self.model.load_state_dict(th.load(best_model_path, map_location=self.device))
            np.savez(self.log_folder + "/loss.npz", train=epoch_train_loss, val=epoch_val_loss)
            # return predicted states for training observations
            self.model.eval()
            with th.no_grad():
                pred_states = self.predStatesWithDataLoader(data_loader)
        finally:
            for loader in (train_loader, val_loader, data_loader):
                loader.shutdown()
        return pred_states


def getModelName(args):
    """
    :param args: (parsed args object)
    :return: (str)
    """
    name = "supervised_{}_SEED{}".format(args.model_type, args.seed)
    name += "_EPOCHS{}_BS{}".format(args.epochs, args.batch_size)
    return name


def buildParser():
    """The reference's command line (srl_baselines/supervised.py:166-181): flags, short forms, types and defaults."""
    parser = argparse.ArgumentParser(description='Supervised Learning')
    parser.add_argument('--epochs', type=int, default=50, metavar='N',
                        help='number of epochs to train (default: 50)')
    parser.add_argument('--seed', type=int, default=1, metavar='S',
                        help='random seed (default: 1)')
    parser.add_argument('-bs', '--batch-size', type=int, default=32, help='batch_size (default: 32)')
    parser.add_argument('-lr', '--learning-rate', type=float, default=0.005, help='learning rate (default: 0.005)')
    parser.add_argument('--no-cuda', action='store_true', default=False,
                        help='accepted for compatibility; this build has no CPU path')
    parser.add_argument('--no-display-plots', action='store_true', default=False,
                        help='accepted for compatibility; plotting is not part of this build')
    parser.add_argument('--model-type', type=str, default="resnet",
                        help='Model architecture: custom_cnn (cnn) or mlp (default: "resnet", which is outside this build)')
    parser.add_argument('--data-folder', type=str, default="", help='Dataset folder', required=True)
    parser.add_argument('--training-set-size', type=int, default=-1,
                        help='Limit size of the training set (default: -1)')
    parser.add_argument('--relative-pos', action='store_true', default=False,
                        help='Use relative position as ground_truth')
    parser.add_argument('--log-folder', type=str, default='', help='Override the default log-folder')
    return parser


def main(argv=None):
    global DISPLAY_PLOTS, N_EPOCHS, BATCH_SIZE
    args = buildParser().parse_args(argv)
    args.cuda = not args.no_cuda and th.cuda.is_available()
    DISPLAY_PLOTS = not args.no_display_plots
    N_EPOCHS = args.epochs
    BATCH_SIZE = args.batch_size
    args.data_folder = parseDataFolder(args.data_folder)
    log_folder = args.log_folder

    if log_folder == '':
        name = getModelName(args)
        log_folder = "logs/{}/baselines/{}".format(args.data_folder, name)

    createFolder(log_folder, "supervised folder already exist")
    createFolder('{}/NearestNeighbors/'.format(log_folder), "NearestNeighbors folder already exist")

    print('Log folder: {}'.format(log_folder))

    print('Loading data ... ')
    training_data, ground_truth, true_states, _ = loadData(args.data_folder)
    rewards = training_data['rewards']

    images_path = ground_truth['images_path']
    state_dim = true_states.shape[1]

    if args.training_set_size > 0:
        limit = args.training_set_size
        true_states = true_states[:limit]
        images_path = images_path[:limit]
        rewards = rewards[:limit]

    args.state_dim = state_dim
    args.losses = ["supervised"]
    exp_config = buildConfig(args)
    exp_config["log-folder"] = log_folder
    saveConfig(exp_config, print_config=True)

    print('Learning a state representation ... ')
    srl = SupervisedLearning(state_dim, model_type=args.model_type, seed=args.seed,
                             log_folder=log_folder, learning_rate=args.learning_rate,
                             cuda=args.cuda)

    learned_states = srl.learn(true_states, images_path, rewards)
    srl.saveStates(learned_states, images_path, rewards, log_folder)


if __name__ == '__main__':
    main()
