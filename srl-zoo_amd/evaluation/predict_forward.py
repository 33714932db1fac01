"""The k-step error of a trained forward model on the recorded dataset: does the latent dynamics that `LatentDynamics.plan` rolls
over a horizon still mean anything after that many steps?

    python -m evaluation.predict_forward --log-folder logs/<dataset>/<experiment>/ [--data-folder data/<dataset>]
                                         [-i states_rewards.npz] [--horizon 10] [--training-set-size N]

From every recorded frame i the recorded actions a_i .. a_{i+T-1} go through the model's forward head, open loop, as far as the
episode reaches; the imagined state after t + 1 steps is compared with the recorded state s_{i+t+1}, next to the error of "the state
stays s_i"; a trained reward head is asked, on the imagined pairs, for the recorded rewards (-1 read as 0).  The states come from the
log folder's states_rewards.npz (what train.py saved), actions, rewards and episode starts through utils.loadData from the data
folder named in exp_config.json, the model through srlz.deploy.LatentDynamics.from_log_folder.  One line per horizon is printed and
<log folder>/forward_horizon.json written: horizon, count, mse, baseline_mse, ratio (below 1: the model beats "nothing moves"),
reward_accuracy, majority_accuracy (null without a trained reward head).  DESIGN.md §3.18.

    python -m evaluation.predict_forward --log-folder logs/<dataset>/<experiment>/ --fit [-i states_rewards.npz | --ground-truth]
                                         [--ridge 1e-6] [--val-fraction 0.2] [--seed 0] [--horizon 10]

With --fit no model is loaded: the question is whether a LINEAR forward model is predictable in the space of these states — PCA
states, supervised or ground-truth states, a model trained without the forward loss.  The head is fitted in closed form
(srlz.dynfit) on the training episodes of srlz.dynfit.split_episodes(episode_starts, --val-fraction, --seed), and
the k-step error is measured twice, on the validation transitions (the printed lines) and on the training ones.  The states come
from -i, else from the log folder's states_rewards.npz, or with --ground-truth from the dataset's true states, as predict_reward
takes them without -i.  <log folder>/forward_horizon_fit.json holds the keys above for the validation side, the same keys under
"train", and "fit": ridge, count, val_fraction, seed, route, state_dim, n_actions.  --ground-truth, --ridge, --val-fraction and
--seed without --fit are an error.

    python -m evaluation.predict_forward --log-folder logs/<dataset>/<experiment>/ --fit --fit-reward
                                         [--reward-epochs 30] [--reward-batch-size 32] [--reward-lr 0.005]

With --fit --fit-reward the reward head is fitted too (srlz.headfit, DESIGN.md §3.21: Adam, one launch per epoch, on four fifths of
the training episodes, the epoch with the lowest loss on the remaining fifth kept — srlz.headfit.split_starts(train, ., 0.2, --seed);
the validation episodes take no part in it) and asked, on the imagined pairs, for the recorded
rewards: is the reward predictable from (s, s') in this space, on held-out episodes?  The printed lines and both sides of the JSON
gain reward_accuracy / majority_accuracy, and the JSON one object "reward_fit": route, hidden, epochs, batch_size, lr, seed,
best_epoch, count, val_count (the two shares of the training transitions) and the per-epoch train_loss, val_loss, train_accuracy, val_accuracy.  "fit" keeps its keys.
--fit-reward without --fit, and the --reward-* flags without --fit-reward, are an error.

    python -m evaluation.predict_forward --log-folder logs/<dataset>/<experiment>/ --fit --fit-inverse
                                         [--inverse-epochs 30] [--inverse-batch-size 32] [--inverse-lr 0.005]

With --fit --fit-inverse the inverse head Linear(2S, A) is fitted as well (srlz.invfit, DESIGN.md §3.22: Adam, one launch per epoch,
the same two shares of the training episodes) and asked for the recorded action of every validation transition: can the action be
read off (s, s') in this space, on held-out episodes?  One line is printed and the JSON gains one object "inverse_fit": accuracy,
majority_accuracy, recall (per action, null for an action the validation episodes never took), count (all four on the validation
transitions), best_epoch, route, and epochs, batch_size, lr, seed, fit_count, select_count.  Without the flag the file and the
printed lines are what they are without it.  --fit-inverse without --fit, and the --inverse-* flags without --fit-inverse, are an
error.

There is no reference counterpart: the reference has no metric for its dynamics heads.  --no-cuda, or a machine without a GPU,
raises: this build has no CPU fallback.
"""
from __future__ import print_function, division, absolute_import

import argparse
import json
import os

import numpy as np
import torch as th

from srlz._cabi import SrlzError
from utils import parseDataFolder, loadData

OUTPUT = "forward_horizon.json"
OUTPUT_FIT = "forward_horizon_fit.json"
FIT_KEYS = ("ridge", "count", "val_fraction", "seed", "route", "state_dim", "n_actions")
FIT_DEFAULTS = (("ridge", 1e-6), ("val_fraction", 0.2), ("seed", 0))  # what --fit uses for a flag that was not given
REWARD_DEFAULTS = (("reward_epochs", 30), ("reward_batch_size", 32), ("reward_lr", 0.005))  # train.py's own, with --fit-reward
INVERSE_DEFAULTS = (("inverse_epochs", 30), ("inverse_batch_size", 32), ("inverse_lr", 0.005))  # the same, with --fit-inverse
INVERSE_KEYS = ("accuracy", "majority_accuracy", "recall", "count", "best_epoch", "route", "epochs", "batch_size", "lr", "seed",
                "fit_count", "select_count")
KEYS = ("horizon", "count", "mse", "baseline_mse", "ratio", "reward_accuracy", "majority_accuracy")


class _Parser(argparse.ArgumentParser):
    """The flags of --fit are refused without it, and take their defaults with it."""

    def parse_args(self, args=None, namespace=None):
        ns = super(_Parser, self).parse_args(args, namespace)
        if not ns.fit_reward:
            given = [flag for flag, on in (("--reward-epochs", ns.reward_epochs is not None),
                                           ("--reward-batch-size", ns.reward_batch_size is not None),
                                           ("--reward-lr", ns.reward_lr is not None)) if on]
            if given:
                self.error("{} only with --fit-reward".format(", ".join(given)))
        if not ns.fit_inverse:
            given = [flag for flag, on in (("--inverse-epochs", ns.inverse_epochs is not None),
                                           ("--inverse-batch-size", ns.inverse_batch_size is not None),
                                           ("--inverse-lr", ns.inverse_lr is not None)) if on]
            if given:
                self.error("{} only with --fit-inverse".format(", ".join(given)))
        if not ns.fit:
            given = [flag for flag, on in (("--ground-truth", ns.ground_truth), ("--ridge", ns.ridge is not None),
                                           ("--val-fraction", ns.val_fraction is not None), ("--seed", ns.seed is not None),
                                           ("--fit-reward", ns.fit_reward), ("--fit-inverse", ns.fit_inverse)) if on]
            if given:
                self.error("{} only with --fit".format(", ".join(given)))
            return ns
        if ns.ground_truth and ns.input_file != "":
            self.error("--ground-truth and -i name two sources of states: give one")
        for name, default in FIT_DEFAULTS:
            if getattr(ns, name) is None:
                setattr(ns, name, default)
        if ns.fit_reward:
            for name, default in REWARD_DEFAULTS:
                if getattr(ns, name) is None:
                    setattr(ns, name, default)
        if ns.fit_inverse:
            for name, default in INVERSE_DEFAULTS:
                if getattr(ns, name) is None:
                    setattr(ns, name, default)
        return ns


def build_parser():
    parser = _Parser(description='k-step prediction error of the forward model on the recorded dataset')
    parser.add_argument('--log-folder', type=str, required=True, help='Experiment folder (exp_config.json, srl_model.pth)')
    parser.add_argument('--data-folder', type=str, default="", help='Dataset folder (default: the one named in exp_config.json)')
    parser.add_argument('-i', '--input-file', type=str, default="",
                        help='Path to a npz file containing the states (default: <log folder>/states_rewards.npz)')
    parser.add_argument('--horizon', type=int, default=10, help='number of open-loop steps (default: 10)')
    parser.add_argument('--training-set-size', type=int, default=-1,
                        help='Limit size (number of samples) of the evaluated set (default: -1)')
    parser.add_argument('--no-cuda', action='store_true', default=False, help='refused: there is no CPU path')
    parser.add_argument('--fit', action='store_true', default=False,
                        help='fit the forward head to the states in closed form instead of loading srl_model.pth')
    parser.add_argument('--ridge', type=float, default=None, help='with --fit: the penalty on the weights (default: 1e-6)')
    parser.add_argument('--val-fraction', type=float, default=None,
                        help='with --fit: the share of the episodes held out for validation (default: 0.2)')
    parser.add_argument('--seed', type=int, default=None, help='with --fit: the seed of the episode split (default: 0)')
    parser.add_argument('--ground-truth', action='store_true', default=False,
                        help="with --fit: take the dataset's true states instead of a states file")
    parser.add_argument('--fit-reward', action='store_true', default=False,
                        help='with --fit: fit the reward head too (Adam, one launch per epoch) and report its accuracy')
    parser.add_argument('--reward-epochs', type=int, default=None, help='with --fit-reward: epochs of the reward fit (default: 30)')
    parser.add_argument('--reward-batch-size', type=int, default=None,
                        help='with --fit-reward: minibatch size of the reward fit (default: 32)')
    parser.add_argument('--reward-lr', type=float, default=None, help='with --fit-reward: learning rate of the reward fit (default: 0.005)')
    parser.add_argument('--fit-inverse', action='store_true', default=False,
                        help='with --fit: fit the inverse head too (Adam, one launch per epoch) and report its held-out accuracy')
    parser.add_argument('--inverse-epochs', type=int, default=None, help='with --fit-inverse: epochs of the inverse fit (default: 30)')
    parser.add_argument('--inverse-batch-size', type=int, default=None,
                        help='with --fit-inverse: minibatch size of the inverse fit (default: 32)')
    parser.add_argument('--inverse-lr', type=float, default=None, help='with --fit-inverse: learning rate of the inverse fit (default: 0.005)')
    return parser


def requireGpu(args):
    if args.no_cuda or not th.cuda.is_available():
        raise SrlzError("predict_forward runs on the GPU only ({}): the srl-zoo_amd build has no CPU fallback".format(
            "--no-cuda was given" if args.no_cuda else "torch.cuda.is_available() is False"))


def prepare(args):
    """The recorded sequence: (states [N,S], actions [N], rewards [N], episode_starts [N]) — host arrays, no GPU involved."""
    log_folder = args.log_folder if args.log_folder.endswith("/") else args.log_folder + "/"
    data_folder = args.data_folder
    if data_folder == "":
        with open(os.path.join(log_folder, "exp_config.json"), "r") as f:
            data_folder = json.load(f)["data-folder"]
    print('Loading data ... ')
    training_data, _, true_states, _ = loadData(parseDataFolder(data_folder))
    actions, rewards = np.asarray(training_data['actions']).reshape(-1), np.asarray(training_data['rewards']).reshape(-1)
    episode_starts = np.asarray(training_data['episode_starts']).reshape(-1)
    if getattr(args, "ground_truth", False):
        print("Using ground truth")
        states = np.asarray(true_states)
    else:
        input_file = args.input_file if args.input_file != "" else os.path.join(log_folder, "states_rewards.npz")
        print("Loading {}...".format(input_file))
        states = np.load(input_file)['states']
    limit = min(len(states), len(actions))
    if args.training_set_size > 0:
        limit = min(limit, args.training_set_size)
    print("{} frames".format(limit))
    return states[:limit], actions[:limit], rewards[:limit], episode_starts[:limit]


def report(result):
    """The printed lines of a HorizonError, one per horizon."""
    lines = []
    for t in range(result.horizon):
        line = "t+{:<2d} n {:6d}  mse {:.6g}  baseline {:.6g}  ratio {:.4f}".format(
            t + 1, int(result.count[t]), result.mse[t], result.baseline_mse[t], result.ratio[t])
        if result.reward_accuracy is not None:
            line += "  reward acc {:.4f} (majority {:.4f})".format(result.reward_accuracy[t], result.majority_accuracy[t])
        lines.append(line)
    return lines


def run_fit(args):
    """--fit: the head fitted on the training episodes, the k-step error on the validation and on the training transitions."""
    states, actions, rewards, episode_starts = prepare(args)
    fit_reward = getattr(args, "fit_reward", False)
    from srlz import dynfit
    from srlz.deploy import LatentDynamics
    states = np.asarray(states, np.float32)
    if states.ndim != 2:
        raise ValueError("the states must be [N,S], got shape {}".format(states.shape))
    train, val = dynfit.split_episodes(episode_starts, args.val_fraction, args.seed)
    everyone = np.concatenate((train, val))
    n_actions = int(np.asarray(actions)[everyone].max()) + 1  # (an action the training episodes never took still has its column)
    dyn = LatentDynamics.from_recording(states, actions, episode_starts, n_actions=n_actions, ridge=args.ridge, starts=train,
                                        max_horizon=max(32, args.horizon))
    fit = dyn.fit
    asked = None
    if fit_reward:
        asked = rewards
        from srlz import headfit
        # the validation episodes stay out of the fit altogether: the kept epoch is picked on a fifth of the TRAINING episodes
        fit_side, select_side = headfit.split_starts(train, episode_starts, 0.2, args.seed)
        rfit = dyn.refit_reward(states, rewards, episode_starts, starts=fit_side, val_starts=select_side, seed=args.seed,
                                epochs=args.reward_epochs, batch_size=args.reward_batch_size, lr=args.reward_lr)
        print("Reward head fitted on {} transitions: route {}, epoch {} of {} kept on {} further training transitions "
              "(loss {:.6g}, accuracy {:.4f})".format(
                  rfit.count, rfit.route, rfit.best_epoch + 1, rfit.epochs, rfit.val_count, rfit.history[rfit.best_epoch]["val_loss"],
                  rfit.history[rfit.best_epoch]["val_accuracy"]))
    if getattr(args, "fit_inverse", False):
        from srlz import headfit
        fit_side, select_side = headfit.split_starts(train, episode_starts, 0.2, args.seed)  # as the reward fit: validation stays out
        ifit = dyn.refit_inverse(states, actions, episode_starts, starts=fit_side, val_starts=select_side, seed=args.seed,
                                 epochs=args.inverse_epochs, batch_size=args.inverse_batch_size, lr=args.inverse_lr)
        acc = dyn.action_accuracy(states, actions, episode_starts, starts=val)
        inverse = {"accuracy": acc.accuracy, "majority_accuracy": acc.majority_accuracy, "recall": acc.recall, "count": acc.count,
                   "best_epoch": ifit.best_epoch, "route": ifit.route, "epochs": ifit.epochs, "batch_size": ifit.batch_size,
                   "lr": ifit.lr, "seed": ifit.seed, "fit_count": ifit.count, "select_count": ifit.val_count}
        print("Inverse head fitted on {} transitions: route {}, epoch {} of {} kept on {} further training transitions; on {} "
              "validation transitions action acc {:.4f} (majority {:.4f}), recall {}".format(
                  ifit.count, ifit.route, ifit.best_epoch + 1, ifit.epochs, ifit.val_count, acc.count, acc.accuracy,
                  acc.majority_accuracy, " ".join("-" if r is None else "{:.2f}".format(r) for r in acc.recall)))
    on_val = dyn.horizon_error(states, actions, episode_starts, args.horizon, rewards=asked, starts=val)
    on_train = dyn.horizon_error(states, actions, episode_starts, args.horizon, rewards=asked, starts=train)
    print("Open-loop error of the fitted forward head over {} steps on {} validation transitions ({} fitted, fit route {}, route {})"
          .format(args.horizon, len(val), fit.count, fit.route, dyn.route))
    for line in report(on_val):
        print(line)
    out = on_val.as_dict()
    out["train"] = on_train.as_dict()
    out["fit"] = {"ridge": fit.ridge, "count": fit.count, "val_fraction": args.val_fraction, "seed": args.seed, "route": fit.route,
                  "state_dim": fit.state_dim, "n_actions": fit.n_actions}
    if fit_reward:
        out["reward_fit"] = rfit.as_dict()
    if getattr(args, "fit_inverse", False):
        out["inverse_fit"] = inverse
    log_folder = args.log_folder if args.log_folder.endswith("/") else args.log_folder + "/"
    with open(os.path.join(log_folder, OUTPUT_FIT), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


def run(args):
    requireGpu(args)
    if args.horizon < 1:
        raise ValueError("--horizon must be at least 1, got {}".format(args.horizon))
    if getattr(args, "fit", False):
        return run_fit(args)
    states, actions, rewards, episode_starts = prepare(args)
    from srlz.deploy import LatentDynamics
    dyn = LatentDynamics.from_log_folder(args.log_folder, max_horizon=max(32, args.horizon))
    result = dyn.horizon_error(np.asarray(states, np.float32), actions, episode_starts, args.horizon,
                               rewards=rewards if "reward" in dyn.heads else None)
    print("Open-loop error of the forward model over {} steps (route {})".format(args.horizon, dyn.route))
    for line in report(result):
        print(line)
    out = result.as_dict()
    log_folder = args.log_folder if args.log_folder.endswith("/") else args.log_folder + "/"
    with open(os.path.join(log_folder, OUTPUT), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


def main(argv=None):
    """:return: the dictionary written to forward_horizon.json (--fit: forward_horizon_fit.json)"""
    return run(build_parser().parse_args(argv))


if __name__ == '__main__':
    main()
