"""The PCA baseline (reference srl_baselines/pca.py:23-128), MI355X-native: the states are the projections of the frames onto the
principal components of an incremental PCA — the other number every results table carries beside the supervised baseline.

    python -m srl_baselines.pca --data-folder <dataset> --state-dim 3 --no-display-plots

Command line, log folder (logs/<dataset>/baselines/pca_ST_DIM<k>/ with its NearestNeighbors/ folder) and the files written
(exp_config.json, pca.pkl, states_rewards.npz, image_to_state.json) are the reference's.  Underneath, sklearn's IncrementalPCA —
one LAPACK SVD of a (k + bs + 1) x 150 528 matrix per minibatch on the host — is srl_baselines/ipca.py on csrc/pca.hip: an fp64
Gram matrix on the GPU, a host eigh of a few dozen rows, one skinny projection.  Every frame is decoded ONCE: the fit pass ships the
loader's planar bytes and leaves them in a ResidentFrames store (HBM if it fits the budget, pinned host memory otherwise, as
learn() does); the transform pass — for which the reference decodes the whole dataset a second time — reads the store.

Deviation: createTestMinibatchList ends with an empty range when the number of frames is a multiple of the batch size, and sklearn
raises on an empty array; here an empty minibatch is skipped.  pca.pkl holds srl_baselines.ipca.IncrementalPCA (sklearn's
attribute names, numpy arrays), not a sklearn object.  No figure is drawn and there is no CPU path.
"""
from __future__ import print_function, division, absolute_import

import argparse
import pickle as pkl

import numpy as np
import torch as th

from models.learner import BaseLearner, _requireGpu
from pipeline import saveConfig
from preprocessing.data_loader import DataLoader
from preprocessing.resident import ResidentFrames
from srl_baselines.ipca import IncrementalPCA
from utils import parseDataFolder, createFolder, printYellow


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
    }

    saveConfig(exp_config, print_config=True)


def buildParser():
    """The reference's command line (srl_baselines/pca.py:57-62): flags, short forms, types and defaults."""
    parser = argparse.ArgumentParser(description='Dimension Reduction using PCA')
    parser.add_argument('-bs', '--batch-size', type=int, default=16, help='batch_size for IncrementalPCA (default: 16)')
    parser.add_argument('--no-display-plots', action='store_true', default=False,
                        help='accepted for compatibility; plotting is not part of this build')
    parser.add_argument('--data-folder', type=str, default="", help='Dataset folder', required=True)
    parser.add_argument('--training-set-size', type=int, default=-1, help='Limit size of the training set (default: -1)')
    parser.add_argument('--state-dim', type=int, default=3, help='State dimension')
    return parser


def fitBatchSize(n_components, batch_size):
    """Avoid "Mean of empty slice." in sklearn (reference srl_baselines/pca.py:94-95)."""
    return max(n_components + 1, batch_size)


def fitAndTransform(images_path, n_components, batch_size, device=None, n_workers=4, budget=None):
    """The two loops of the reference (srl_baselines/pca.py:98-119) with ONE decode per frame: every minibatch of the loader is
    fitted and kept (ResidentFrames), the states are computed from the store.
    :return: (ipca, states float32 [N, k], info dict: frames decoded, store placement)"""
    _requireGpu(True)
    device = th.device("cuda", th.cuda.current_device()) if device is None else th.device(device)
    n_frames = len(images_path)
    minibatchlist = DataLoader.createTestMinibatchList(n_frames, batch_size)
    # Training = False -> outputs only the current observation, not a tuple
    data_loader = DataLoader(minibatchlist, images_path, n_workers=n_workers, is_training=False, infinite_loop=False,
                             raw_uint8="planar")
    print("Fitting PCA with n_components={}".format(n_components))
    ipca = IncrementalPCA(n_components=n_components)
    resident, decoded = None, 0
    try:
        for indices, frames in zip(minibatchlist, data_loader):
            if len(indices) == 0:  # the trailing empty range of createTestMinibatchList (sklearn would raise on it)
                continue
            if resident is None:
                resident = ResidentFrames(n_frames, tuple(frames.shape[1:]), device, np.arange(n_frames), budget=budget)
            on_device = frames.to(device, non_blocking=True)
            ipca.partial_fit(on_device)
            resident.absorb_range(int(indices[0]), on_device if resident.on_device else frames)
            decoded += int(frames.shape[0])
    finally:
        data_loader.shutdown()
    if resident is None or not resident.complete():
        raise RuntimeError("the fit pass left {} of {} frames out of the store".format(
            n_frames if resident is None else resident.missing, n_frames))

    print("Transforming observations to states")
    predictions = []
    for indices in minibatchlist:
        if len(indices) == 0:
            continue
        frames = resident.store[int(indices[0]):int(indices[-1]) + 1]
        predictions.append(ipca.transform(frames if resident.on_device else frames.to(device, non_blocking=True)))
    info = {"frames": n_frames, "decoded": decoded, "store": "device" if resident.on_device else "host"}
    return ipca, np.concatenate(predictions, axis=0), info


def main(argv=None):
    args = buildParser().parse_args(argv)
    args.data_folder = parseDataFolder(args.data_folder)
    args.method = "pca"
    log_folder = "logs/{}/baselines/{}".format(args.data_folder, getModelName(args))

    createFolder(log_folder, "{} folder already exist".format(args.method))
    folder_path = '{}/NearestNeighbors/'.format(log_folder)
    createFolder(folder_path, "NearestNeighbors folder already exist")

    saveExpConfig(args, log_folder)
    print('Log folder: {}'.format(log_folder))
    _requireGpu(th.cuda.is_available())

    print('Loading data ... ')
    rewards = np.load("data/{}/preprocessed_data.npz".format(args.data_folder))['rewards']
    images_path = np.load("data/{}/ground_truth.npz".format(args.data_folder))['images_path']

    if args.training_set_size > 0:
        limit = args.training_set_size
        images_path = images_path[:limit]
        rewards = rewards[:limit]

    n_components = args.state_dim
    batch_size = fitBatchSize(n_components, args.batch_size)
    print("batch_size = {}".format(batch_size))

    ipca, predictions, info = fitAndTransform(images_path, n_components, batch_size)
    print("Decoded {decoded} frames for {frames} observations (store: {store})".format(**info))
    # Save PCA transformation
    with open(log_folder + "/pca.pkl", "wb") as f:
        pkl.dump(ipca, f)

    BaseLearner.saveStates(predictions, images_path, rewards, log_folder)
    printYellow("pca: plotting is out of scope of the MI355X hot-path build: nothing is drawn, learned_states.png is not written")


if __name__ == '__main__':
    main()
