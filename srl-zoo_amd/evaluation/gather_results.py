"""Create a csv report from a folder of experiments (reference evaluation/gather_results.py): one row per experiment of
logs/<dataset>/ (and of its baselines/ folder) with the keys of exp_config.json every results table carries, the KNN-MSE
(knn_mse.json) and the ground-truth correlation (gt_correlation.json).  A missing result file is computed first — through
pipeline.correlationCall / pipeline.knnCall, after evaluation.predict_dataset when states_rewards.npz is missing too — unless the
folder has no exp_config.json.  results.csv has the reference's columns in its order and is written with the csv module as pandas
writes a frame of these lists: an absent value as an empty cell, everything else by str().

    python -m evaluation.gather_results -i logs/<dataset>
"""
from __future__ import print_function, division, absolute_import

import argparse
import csv
import json
import os
import subprocess
import sys
from collections import OrderedDict

from pipeline import correlationCall, knnCall, _childEnv

# keys of exp_config.json that are saved in the csv report file, then the columns computed here: the reference's order
CONFIG_KEYS = ['training-set-size', 'split-dimensions', 'state-dim', 'seed', 'losses_weights']
COLUMNS = CONFIG_KEYS + ['experiments', 'knn_mse', 'gt_corr', 'gt_mean']


def getKnnMse(path):
    """
    Retrieve knn mse score
    :param path: (str)
    :return: (float)
    """
    try:
        with open(path) as f:
            return json.load(f)['knn_mse']
    except IOError:
        print("knn_mse.json not found for {}".format(path))
        return -1


def getCorrelation(path):
    """
    Retrieve Ground Truth Correlation
    :param path: (str)
    :return: (float, [float])
    """
    try:
        with open(path) as f:
            results = json.load(f)
            return results['gt_corr_mean'], results['gt_corr']
    except IOError:
        print("gt_correlation.json not found for {}".format(path))
        return -1, [-1]


def computeStates(exp_config, log_dir):
    """states_rewards.npz of an experiment that lacks it: evaluation.predict_dataset in a fresh child of this interpreter.
    :param exp_config: (dict)
    :param log_dir: (str)
    :return: (bool)
    """
    ok = subprocess.call([sys.executable, '-m', 'evaluation.predict_dataset', '--name-suffix', '',
                          '-n', str(exp_config['training-set-size']), '--log-dir', log_dir], env=_childEnv())
    return ok == 0


def findExperiments(log_dir):
    """The sub-folders of log_dir except baselines, then every entry of log_dir/baselines as 'baselines/<entry>', sorted."""
    experiments = []
    for item in os.listdir(log_dir):
        if 'baselines' not in item and os.path.isdir('{}/{}'.format(log_dir, item)):
            experiments.append(item)
    if os.path.isdir(log_dir + "/baselines"):
        for item in os.listdir(log_dir + "/baselines"):
            experiments.append('baselines/' + item)
    experiments.sort()
    return experiments


def _retrying(call, exp_config, folder):
    """call(exp_config); on RuntimeError — assumed to be a missing states_rewards.npz — predict the states and try once more."""
    try:
        call(exp_config)
    except RuntimeError:
        computeStates(exp_config, folder)
        try:
            call(exp_config)
        except RuntimeError:
            pass


def gatherResults(log_dir):
    """:return: (OrderedDict) column name -> list, one entry per experiment"""
    experiments = findExperiments(log_dir)
    print("Found {} experiments".format(len(experiments)))
    table = OrderedDict((key, []) for key in COLUMNS)
    table['experiments'] = experiments
    for experiment in experiments:
        folder = '{}/{}'.format(log_dir, experiment)
        skip = False
        try:
            with open('{}/exp_config.json'.format(folder)) as f:
                exp_config = json.load(f, object_pairs_hook=OrderedDict)
        except FileNotFoundError:
            print("exp_config not found for {}".format(experiment))
            skip = True
            exp_config = {}
        for key in CONFIG_KEYS:
            table[key].append(exp_config.get(key, None))

        get_corr_file = '{}/gt_correlation.json'.format(folder)
        if not os.path.isfile(get_corr_file) and not skip:
            _retrying(lambda cfg: correlationCall(cfg, plot=False), exp_config, folder)
        gt_mean, gt_corr = getCorrelation(get_corr_file)
        table['gt_mean'].append(gt_mean)
        table['gt_corr'].append(gt_corr)

        knn_mse_file = '{}/knn_mse.json'.format(folder)
        if not os.path.isfile(knn_mse_file) and not skip:
            _retrying(knnCall, exp_config, folder)
        table['knn_mse'].append(getKnnMse(knn_mse_file))
    return table


def writeCsv(table, path):
    """One header line, one line per experiment; None is an empty cell."""
    with open(path, 'w', newline='') as f:
        writer = csv.writer(f, lineterminator='\n')
        writer.writerow(COLUMNS)
        for row in zip(*[table[key] for key in COLUMNS]):
            writer.writerow(["" if cell is None else str(cell) for cell in row])


def main(argv=None):
    parser = argparse.ArgumentParser(description='Create a report file for a given dataset')
    parser.add_argument('-i', '--log-dir', type=str, default="", required=True, help='Path to a dataset log folder')
    args = parser.parse_args(argv)
    assert os.path.isdir(args.log_dir), "--log-dir must be a path to a valid folder"
    table = gatherResults(args.log_dir)
    writeCsv(table, '{}/results.csv'.format(args.log_dir))
    print("Saved results to {}/results.csv".format(args.log_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
