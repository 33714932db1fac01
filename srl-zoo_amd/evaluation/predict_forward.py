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
KEYS = ("horizon", "count", "mse", "baseline_mse", "ratio", "reward_accuracy", "majority_accuracy")


def build_parser():
    parser = argparse.ArgumentParser(description='k-step prediction error of the forward model on the recorded dataset')
    parser.add_argument('--log-folder', type=str, required=True, help='Experiment folder (exp_config.json, srl_model.pth)')
    parser.add_argument('--data-folder', type=str, default="", help='Dataset folder (default: the one named in exp_config.json)')
    parser.add_argument('-i', '--input-file', type=str, default="",
                        help='Path to a npz file containing the states (default: <log folder>/states_rewards.npz)')
    parser.add_argument('--horizon', type=int, default=10, help='number of open-loop steps (default: 10)')
    parser.add_argument('--training-set-size', type=int, default=-1,
                        help='Limit size (number of samples) of the evaluated set (default: -1)')
    parser.add_argument('--no-cuda', action='store_true', default=False, help='refused: there is no CPU path')
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
    training_data, _, _, _ = loadData(parseDataFolder(data_folder))
    actions, rewards = np.asarray(training_data['actions']).reshape(-1), np.asarray(training_data['rewards']).reshape(-1)
    episode_starts = np.asarray(training_data['episode_starts']).reshape(-1)
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


def run(args):
    requireGpu(args)
    if args.horizon < 1:
        raise ValueError("--horizon must be at least 1, got {}".format(args.horizon))
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
    """:return: the dictionary written to forward_horizon.json"""
    return run(build_parser().parse_args(argv))


if __name__ == '__main__':
    main()
