"""Ground-truth correlation (GTC) of a learned representation (reference plotting/representation_plot.py:259-309 and its command
line :312-406): for every dimension of the agent's position, then of the target's position, the largest absolute Pearson
correlation with any other column of [ground truth | learned states].  Written to gt_correlation.json next to the input file as
{'gt_corr': [...], 'gt_corr_mean': ...}.

The correlation rows come from the two-pass fp64 kernels on the GPU (srlz.ops.gt_correlation, csrc/gtc.hip) in place of
np.corrcoef over all (G + S)^2 pairs (:283); what is done with them — the epsilon added to both sides, the zeroed diagonal entry,
Python's max over the absolute row, the printed lines, the result file — is the reference's.  No figure is drawn, with or without
--print-corr, and nothing waits for a key; the flags that only draw parse and then stop with a message.

    python -m plotting.representation_plot -i logs/<dataset>/<experiment>/states_rewards.npz --data-folder data/<dataset> \
        --correlation --print-corr
"""
from __future__ import print_function, division, absolute_import

import argparse
import json
import os
import sys

import numpy as np

from utils import parseDataFolder, loadData, printYellow

PLOTS_MESSAGE = "representation_plot: plots are outside this build (only --correlation / --print-corr compute something)"


def plotCorrelation(states_rewards, ground_truth, target_positions, only_print=False):
    """
    Correlation: target position / ground truth states vs. predicted states (nothing is drawn, whatever only_print says)

    :param states_rewards: (numpy dict) 'states' [N, S] and 'rewards' [N]
    :param ground_truth: (numpy dict) 'ground_truth_states' (or 'arm_states'), at least N rows
    :param target_positions: (np.ndarray) per frame, at least N rows
    :param only_print: (bool) kept for the reference's signature
    :return: the max correlation for each of the ground truth's dimensions with the predicted states, and its mean
    """
    from srlz import ops
    np.set_printoptions(precision=2)
    correlation_max_vector = np.array([])
    n_frames = len(states_rewards['rewards'])

    for ground_truth_name in [" Agent's position ", "Target Position"]:
        if ground_truth_name == " Agent's position ":
            key = 'ground_truth_states' if 'ground_truth_states' in ground_truth.keys() else 'arm_states'
            x = ground_truth[key][:n_frames]
        else:
            x = target_positions[:n_frames]

        # adding epsilon in case of little variance in samples of X & Ys (as the reference does, in each side's own precision)
        eps = 1e-12
        corr = ops.gt_correlation(x + eps, states_rewards['states'] + eps)  # rows 0 .. G-1 of np.corrcoef(..., rowvar=0)

        # the vector of max correlation (a scalar for each of the ground truth's dimensions)
        ground_truth_dim = x.shape[1]
        for idx in range(ground_truth_dim):
            corr[idx, idx] = 0.0
            correlation_max_vector = np.append(correlation_max_vector, max(abs(corr[idx])))

    correlation_scalar = sum(correlation_max_vector)
    print("\nCorrelation value of the model's prediction with the Ground Truth:\n Max correlation vector (GTC): {}"
          "\n Mean : {:.2f}".format(correlation_max_vector, correlation_scalar / len(correlation_max_vector)))
    return correlation_max_vector, correlation_scalar / len(correlation_max_vector)


def buildParser():
    """The reference's flags and defaults (representation_plot.py:313-329)."""
    parser = argparse.ArgumentParser(description='Ground-truth correlation of a representation (no figures in this build)')
    parser.add_argument('-i', '--input-file', type=str, default="", help='Path to a npz file containing states and rewards')
    parser.add_argument('--data-folder', type=str, default="", help='Path to a dataset folder')
    parser.add_argument('--color-episode', action='store_true', default=False, help='(plots only) color states per episode')
    parser.add_argument('--plot-against', action='store_true', default=False, help='(plot: outside this build)')
    parser.add_argument('--pretty-plot-against', action='store_true', default=False, help='(plot: outside this build)')
    parser.add_argument('--correlation', action='store_true', default=False,
                        help='Correlation coefficients of the ground truth against each dimension')
    parser.add_argument('--projection', action='store_true', default=False, help='(plot: outside this build)')
    parser.add_argument('--print-corr', action='store_true', default=False, help='Only print correlation measurements')
    return parser


def parseArguments(argv=None):
    """Parse, then the reference's two assertions and its --print-corr rule (representation_plot.py:331-343)."""
    args = buildParser().parse_args(argv)
    assert not (args.color_episode and args.data_folder == ""), \
        "You must specify a datafolder when using per-episode color"
    assert not (args.correlation and args.data_folder == ""), \
        "You must specify a datafolder when using the correlation plot"
    # Force correlation when `--print-corr` is passed
    if args.print_corr:
        args.correlation = True
    args.data_folder = parseDataFolder(args.data_folder)
    return args


def main(argv=None):
    args = parseArguments(argv)
    if args.input_file == "" and args.data_folder == "":
        print("You must specify one of --input-file or --data-folder")
        return 0
    draws = args.plot_against or args.pretty_plot_against or args.projection
    if args.input_file == "" or draws or not args.correlation:
        printYellow(PLOTS_MESSAGE)
        return 2

    print("Loading {}...".format(args.input_file))
    states_rewards = np.load(args.input_file)
    training_data, ground_truth, true_states, target_positions = loadData(args.data_folder)
    # Compute Ground Truth Correlation
    gt_corr, gt_corr_mean = plotCorrelation(states_rewards, ground_truth, target_positions, only_print=args.print_corr)
    result_dict = {
        'gt_corr': gt_corr.tolist(),
        'gt_corr_mean': gt_corr_mean
    }
    # Write the results in a json file
    log_folder = os.path.dirname(args.input_file)
    with open("{}/gt_correlation.json".format(log_folder), 'w') as f:
        json.dump(result_dict, f)
    return 0


if __name__ == '__main__':
    sys.exit(main())
