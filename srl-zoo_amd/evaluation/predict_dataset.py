"""States of a trained model on a dataset (reference evaluation/predict_dataset.py:22-61): loads <log-dir>/srl_model.pth with its
exp_config.json, predicts the states of the first -n images of the experiment's dataset and writes
states_rewards<suffix>.npz, image_to_state<suffix>.json and states_stats.npz into the log folder.

    python -m evaluation.predict_dataset -i logs/<dataset>/<experiment>/ [--name-suffix _test] [-n 1000]
"""
from __future__ import print_function, division, absolute_import

import argparse

import numpy as np
import torch as th

from models.learner import SRL4robotics, MAX_BATCH_SIZE_GPU
from preprocessing.data_loader import DataLoader

# the reference's list (predict_dataset.py:11-12) without "priors", which this build does not train
VALID_MODELS = ["forward", "inverse", "reward", "episode-prior", "reward-prior", "triplet", "autoencoder", "vae"]


def buildParser():
    parser = argparse.ArgumentParser(description="Predict states on a dataset for a trained model")
    parser.add_argument('-i', '--log-dir', default='', type=str, help='Directory to load model', required=True)
    parser.add_argument('--name-suffix', default='_test', type=str, help='Suffix to add to the filename of the output file')
    parser.add_argument('--no-cuda', default=False, action="store_true", help="Disable CUDA (this build then refuses to run)")
    parser.add_argument('-n', '--n-samples', type=int, default=-1,
                        help='Limit size (number of samples) for predicting the states (default: -1)')
    return parser


def statesStats(learned_states):
    """mean, std, min and max over axis 0 (predict_dataset.py:50-53)."""
    return {'mean': np.mean(learned_states, axis=0), 'std': np.std(learned_states, axis=0),
            'min': np.min(learned_states, axis=0), 'max': np.max(learned_states, axis=0)}


def predictDataset(log_dir, name_suffix='_test', cuda=True, n_samples=-1):
    """:return: (learned states np.ndarray [n, state_dim])"""
    if not log_dir.endswith('/'):
        log_dir += '/'
    srl_model, exp_config = SRL4robotics.loadSavedModel(log_dir, VALID_MODELS, cuda=cuda)

    images_path = np.load("data/{}/ground_truth.npz".format(exp_config['data-folder']))['images_path']
    rewards = np.load("data/{}/preprocessed_data.npz".format(exp_config['data-folder']))['rewards']
    limit = n_samples if n_samples > 0 else len(images_path)
    images_path = images_path[:limit]
    rewards = rewards[:limit]

    minibatchlist = DataLoader.createTestMinibatchList(len(images_path), MAX_BATCH_SIZE_GPU)
    data_loader = DataLoader(minibatchlist, images_path, n_workers=4, multi_view=exp_config.get('multi-view', False),
                             use_triplets='triplet' in exp_config['losses'], max_queue_len=1, is_training=False,
                             apply_occlusion=srl_model.use_dae, occlusion_percentage=srl_model.occlusion_percentage,
                             infinite_loop=False)

    print("Predicting states for {} observations...".format(len(images_path)))
    srl_model.model.eval()
    try:
        with th.no_grad():
            learned_states = srl_model.predStatesWithDataLoader(data_loader)
    finally:
        data_loader.shutdown()

    srl_model.saveStates(learned_states, images_path, rewards, log_dir, name=name_suffix)

    stats = statesStats(learned_states)
    print("Mean:", stats['mean'])
    print("Std:", stats['std'])
    print("Min:", stats['min'])
    print("Max:", stats['max'])
    print("Stats saved (states_stats.npz)")
    np.savez(log_dir + '/states_stats.npz', **stats)
    return learned_states


def main(argv=None):
    args = buildParser().parse_args(argv)
    predictDataset(args.log_dir, name_suffix=args.name_suffix, cuda=not args.no_cuda, n_samples=args.n_samples)
    return 0


if __name__ == '__main__':
    main()
