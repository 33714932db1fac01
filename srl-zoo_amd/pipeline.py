"""The helpers train.py imports from the reference's pipeline.py (getLogFolderName :28-51, saveConfig :223-236, correlationCall
:180-191) plus the exit-code constants (:23-25), the KNN-MSE evaluation call with its two helpers (knnCall :194-220,
createGroundTruthFolder :166-177, useRelativePosition :239-246) and the PCA baseline call (pcaCall :150-163).  Every evaluation runs
in a fresh child of this interpreter.  The grid-search driver itself is out of scope."""
from __future__ import print_function, division

import datetime
import json
import os
import subprocess
import sys
from collections import OrderedDict
from pprint import pprint

from utils import printBlue, printGreen, printRed, createFolder

MATPLOTLIB_WARNING_CODE = -11
NO_PAIRS_ERROR = 10  # no dissimilar/reference pairs found (robotic priors)
NAN_ERROR = 11       # training loss became NaN


def getLogFolderName(exp_config):
    """logs/<dataset>/<YY-MM-DD_HHhMM_SS>_<model>_ST_DIM<S>_<losses>; creates the folder.
    :return: (log_folder, experiment_name)"""
    date = datetime.datetime.now().strftime("%y-%m-%d_%Hh%M_%S")
    losses = exp_config["losses"]
    if not isinstance(losses, str):
        losses = "_".join(losses)
    experiment_name = "{}_{}_ST_DIM{}_{}".format(date, exp_config['model-type'], exp_config['state-dim'], losses)
    printBlue("\nExperiment: {}\n".format(experiment_name))
    log_folder = "logs/{}/{}".format(exp_config['data-folder'], experiment_name)
    createFolder(log_folder, "Experiment folder already exist")
    return log_folder, experiment_name


def saveConfig(exp_config, print_config=False):
    """Write <log-folder>/exp_config.json (keys sorted)."""
    if print_config:
        pprint(exp_config)
    exp_config = OrderedDict(sorted(exp_config.items()))
    with open("{}/exp_config.json".format(exp_config['log-folder']), "w") as f:
        json.dump(exp_config, f)
    print("Saved config to log folder: {}".format(exp_config['log-folder']))


def correlationArguments(exp_config, plot=False):
    """The reference's argument list for plotting.representation_plot (pipeline.py:186-190)."""
    log_folder = exp_config["log-folder"] + "/states_rewards.npz"
    data_folder = 'data/' + exp_config['data-folder']
    use_plot = [] if plot else ["--print-corr"]
    return ["-i", log_folder, "--data-folder", data_folder, "--correlation"] + use_plot


def correlationCall(exp_config, plot=False):
    """Ground-truth correlation of the representation in exp_config['log-folder'] (reference pipeline.py:180-191; writes
    gt_correlation.json there): plotting.representation_plot in a fresh child process — this interpreter, as knnCall starts its
    child.  No figure is drawn whatever `plot` says.
    :param exp_config: (dict)
    :param plot: (bool)"""
    ok = subprocess.call([sys.executable, '-m', 'plotting.representation_plot'] + correlationArguments(exp_config, plot),
                         env=_childEnv())
    printConfigOnError(ok, exp_config, "correlationCall")


def printConfigOnError(return_code, exp_config, step_name):
    """Reference pipeline.py:54-64."""
    if return_code != 0:
        printRed("An error occured, error code: {}".format(return_code))
        pprint(exp_config)
        raise RuntimeError("Error during {} (config file above)".format(step_name))
    print("End of " + step_name)


def createGroundTruthFolder(exp_config):
    """logs/<dataset>/baselines/ground_truth/ with its exp_config.json, so that KNN-MSE can be computed for the ground truth.
    :return: (dict) exp_config with 'log-folder' and 'ground-truth' set"""
    log_folder = "logs/{}/baselines/ground_truth/".format(exp_config['data-folder'])
    createFolder(log_folder, "")
    exp_config['log-folder'] = log_folder
    exp_config['ground-truth'] = True
    saveConfig(exp_config)
    return exp_config


def useRelativePosition(data_folder):
    """The dataset's 'relative_pos' setting (data/<folder>/dataset_config.json)."""
    with open('data/{}/dataset_config.json'.format(data_folder), 'r') as f:
        relative_pos = json.load(f).get('relative_pos', False)
    return relative_pos


def _childEnv():
    """The environment of a child interpreter that finds the package whatever the working directory."""
    env = dict(os.environ)
    package = os.path.dirname(os.path.abspath(__file__))
    env["PYTHONPATH"] = package + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def pcaArguments(exp_config):
    """The reference's argument list for srl_baselines.pca (pipeline.py:156-160)."""
    args = ['--no-display-plots']
    config_args = ['data-folder', 'training-set-size', 'state-dim']

    for arg in config_args:
        args.extend(['--{}'.format(arg), str(exp_config[arg])])
    return args


def pcaCall(exp_config):
    """The PCA baseline on exp_config's dataset (reference pipeline.py:150-163): srl_baselines.pca in a fresh child process — this
    interpreter, as knnCall starts its child.
    :param exp_config: (dict)"""
    printGreen("\n Baseline PCA...")
    ok = subprocess.call([sys.executable, '-m', 'srl_baselines.pca'] + pcaArguments(exp_config), env=_childEnv())
    printConfigOnError(ok, exp_config, "pcaCall")


def knnCall(exp_config):
    """KNN-MSE of the representation in exp_config['log-folder'] (writes knn_mse.json there): evaluation.knn_images in a fresh child
    process with the reference's argument list.  The child is this interpreter and finds the package whatever the working
    directory (the dataset is looked up under ./data, as everywhere)."""
    folder_path = '{}/NearestNeighbors/'.format(exp_config['log-folder'])
    createFolder(folder_path, "NearestNeighbors folder already exist")

    printGreen("\nEvaluating the state representation with KNN")

    args = ['--seed', str(exp_config['knn-seed']), '--n-samples', str(exp_config['knn-samples'])]

    if exp_config.get('ground-truth', False):
        args.extend(['--ground-truth'])

    if exp_config.get('multi-view', False):
        args.extend(['--multi-view'])

    if exp_config.get('relative-pos', False):
        args.extend(['--relative-pos'])

    for arg in ['log-folder', 'n-neighbors', 'n-to-plot']:
        args.extend(['--{}'.format(arg), str(exp_config[arg])])

    ok = subprocess.call([sys.executable, '-m', 'evaluation.knn_images'] + args, env=_childEnv())
    printConfigOnError(ok, exp_config, "knnCall")
