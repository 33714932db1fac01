"""The robotic-priors baseline: a LINEAR map from the features of a recording to a low-dimensional state, trained by the four
robotic priors alone (Jonschkowski & Brock) — srlz/priorsfit.py on csrc/robotic.hip.

    python -m srl_baselines.robotic_priors --data-folder <dataset> -i logs/<dataset>/baselines/pca_ST_DIM200/states_rewards.npz \
        --state-dim 3 --no-display-plots

The features are the 'states' of any experiment's states_rewards.npz (the PCA baseline's 200 components are the intended use);
actions, rewards and episode_starts come from data/<dataset>/preprocessed_data.npz, the image paths from ground_truth.npz, as
srl_baselines/pca.py and evaluation/predict_reward.py read them.  It writes logs/<dataset>/baselines/robotic_priors_ST_DIM<k>/
with exp_config.json (the PCA baseline's keys plus input-file, epochs, learning-rate, seed), robotic_priors.npz (weight, bias for the
raw features, history [epochs, 10] with the columns HISTORY_KEYS, best_epoch), states_rewards.npz and image_to_state.json (BaseLearner.saveStates) and the NearestNeighbors/
folder, so that knn_images, representation_plot --correlation and gather_results work on the folder unchanged.  A recording in
which a minibatch is left without a pair exits with pipeline.NO_PAIRS_ERROR.  No figure is drawn and there is no CPU path.
"""
from __future__ import print_function, division, absolute_import

import argparse
import io
import sys
import zipfile

import numpy as np
import torch as th

from losses.utils import NoPairsError
from models.learner import BaseLearner, _requireGpu
from pipeline import saveConfig, NO_PAIRS_ERROR
from srlz import priorsfit
from utils import parseDataFolder, createFolder, printYellow, printRed

HISTORY_KEYS = ("train_loss", "val_loss") + tuple("train_" + t for t in priorsfit.TERMS) + tuple("val_" + t for t in priorsfit.TERMS)


def getModelName(args):
    """
    :param args: (parsed args object)
    :return: (str)
    """
    return "{}_ST_DIM{}".format(args.method, args.state_dim)


def saveExpConfig(args, log_folder):
    """
    :param args: (parsed args object)
    :param log_folder: (str)
    """
    exp_config = {
        "batch-size": args.batch_size,
        "data-folder": args.data_folder,
        "training-set-size": args.training_set_size,
        "log-folder": log_folder,
        "state-dim": args.state_dim,
        "input-file": args.input_file,
        "epochs": args.epochs,
        "learning-rate": args.learning_rate,
        "seed": args.seed,
    }
    saveConfig(exp_config, print_config=True)


def buildParser():
    parser = argparse.ArgumentParser(description='A linear state map trained by the robotic priors on the features of a recording')
    parser.add_argument('--data-folder', type=str, default="", help='Dataset folder', required=True)
    parser.add_argument('-i', '--input-file', type=str, required=True, help="npz file with the features under 'states'")
    parser.add_argument('--state-dim', type=int, default=3, help='State dimension')
    parser.add_argument('--epochs', type=int, default=priorsfit.DEFAULT_EPOCHS, help='number of epochs to train (default: 30)')
    parser.add_argument('--seed', type=int, default=1, help='random seed (default: 1)')
    parser.add_argument('-bs', '--batch-size', type=int, default=priorsfit.DEFAULT_BATCH_SIZE, help='batch_size (default: 32)')
    parser.add_argument('-lr', '--learning-rate', type=float, default=priorsfit.DEFAULT_LR, help='learning rate (default: 0.005)')
    parser.add_argument('--val-size', type=float, default=0.2, help='share of the minibatches held out for validation (default: 0.2)')
    parser.add_argument('--training-set-size', type=int, default=-1, help='Limit size of the training set (default: -1)')
    parser.add_argument('--no-standardize', action='store_true', default=False, help='fit on the raw features')
    parser.add_argument('--no-display-plots', action='store_true', default=False,
                        help='accepted for compatibility; plotting is not part of this build')
    return parser


def historyArray(history):
    """The fit's history as one float64 [epochs, 10] array, columns HISTORY_KEYS."""
    return np.array([[h["train_loss"], h["val_loss"]] + list(h["train_terms"]) + list(h["val_terms"]) for h in history], np.float64)


def saveNpz(path, **arrays):
    """np.savez without the clock: the members carry a fixed date, so that two runs with the same seed write the same bytes
    (np.load reads the file like any other npz)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as archive:
        for key, value in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(value), allow_pickle=False)
            archive.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())


def main(argv=None):
    args = buildParser().parse_args(argv)
    args.data_folder = parseDataFolder(args.data_folder)
    args.method = "robotic_priors"
    log_folder = "logs/{}/baselines/{}".format(args.data_folder, getModelName(args))

    createFolder(log_folder, "{} folder already exist".format(args.method))
    createFolder('{}/NearestNeighbors/'.format(log_folder), "NearestNeighbors folder already exist")

    saveExpConfig(args, log_folder)
    print('Log folder: {}'.format(log_folder))
    _requireGpu(th.cuda.is_available())

    print('Loading data ... ')
    training_data = np.load("data/{}/preprocessed_data.npz".format(args.data_folder))
    actions, rewards, episode_starts = training_data['actions'], training_data['rewards'], training_data['episode_starts']
    images_path = np.load("data/{}/ground_truth.npz".format(args.data_folder))['images_path']
    features = np.load(args.input_file)['states']
    if len(features) != len(images_path):
        raise ValueError("{} holds {} rows, the dataset {} frames".format(args.input_file, len(features), len(images_path)))

    if args.training_set_size > 0:
        limit = args.training_set_size
        images_path, features = images_path[:limit], features[:limit]
        actions, rewards, episode_starts = actions[:limit], rewards[:limit], episode_starts[:limit]

    features = np.ascontiguousarray(features, dtype=np.float32)
    print("Fitting a {} -> {} map by the robotic priors".format(features.shape[1], args.state_dim))
    try:
        fit = priorsfit.fit_priors(features, actions, rewards, episode_starts, args.state_dim, epochs=args.epochs,
                                   batch_size=args.batch_size, lr=args.learning_rate, seed=args.seed, val_size=args.val_size,
                                   standardize=not args.no_standardize)
    except NoPairsError as e:
        printRed(str(e))
        sys.exit(NO_PAIRS_ERROR)
    for epoch, h in enumerate(fit.history):
        print("Epoch {:3}/{}, train_loss:{:.4f} val_loss:{:.4f}".format(epoch + 1, fit.epochs, h["train_loss"], h["val_loss"]))
    print("Kept epoch {} (route {}, {} minibatches resampled)".format(fit.best_epoch + 1, fit.route, fit.minibatches_resampled))

    saveNpz(log_folder + "/robotic_priors.npz", weight=fit.weight, bias=fit.bias, history=historyArray(fit.history),
            best_epoch=np.array(fit.best_epoch))
    print("Transforming features to states")
    predictions = fit.transform(features).cpu().numpy()
    BaseLearner.saveStates(predictions, images_path, rewards, log_folder)
    printYellow("robotic_priors: plotting is out of scope of the MI355X hot-path build: nothing is drawn, learned_states.png is not "
                "written")


if __name__ == '__main__':
    main()
