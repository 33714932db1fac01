"""KNN-MSE of a learned representation (reference evaluation/knn_images.py): for a random test set of images, the mean squared
ground-truth distance between each image and its k nearest neighbours in the learned state space.  Written to
<log-folder>/knn_mse.json as {'images': [...], 'knn_mse': ...}.

The neighbours come from the exact fp64 search on the GPU (srlz.ops.knn, csrc/knn.hip) for the sampled rows only, in place of the
reference's ball tree over all N states (knn_images.py:83-84); everything else — the sampled images, the error sum and its order, the
rounding, the titles — is the reference's.  Figures are not drawn (plotting is out of scope of this build).

    python -m evaluation.knn_images --log-folder logs/<dataset>/<experiment> [-k 5] [-n 5] [--ground-truth] [--relative-pos]
"""
from __future__ import print_function, division, absolute_import

import argparse
import json
import random

import numpy as np

from utils import printYellow


def buildParser():
    """The reference's flags and defaults (knn_images.py:33-41)."""
    parser = argparse.ArgumentParser(description='KNN MSE (no figures in this build)')
    parser.add_argument('--log-folder', type=str, default="", required=True, help='Path to a log folder')
    parser.add_argument('--seed', type=int, default=1, help='random seed (default: 1)')
    parser.add_argument('-k', '--n-neighbors', type=int, default=5, help='Number of nearest neighbors (default: 5)')
    parser.add_argument('-n', '--n-samples', type=int, default=5, help='Number of test samples (default: 5)')
    parser.add_argument('--n-to-plot', type=int, default=5, help='Number of samples to plot (default: 5; nothing is drawn)')
    parser.add_argument('--relative-pos', action='store_true', default=False, help='Use relative position as ground_truth')
    parser.add_argument('--ground-truth', action='store_true', default=False, help='Compute KNN-MSE for ground truth')
    parser.add_argument('--multi-view', action='store_true', default=False, help='To deal with multi view data format')
    return parser


def sampleIndices(n_images, n_samples, seed):
    """The reference's test images (knn_images.py:48,90-92): after random.seed(seed), random.sample over a list of length N consumes
    the generator as a function of (N, n) alone, so its picks are those of random.sample(range(N), n).
    :return: ([int]) min(n_images, n_samples) indices, in the order the reference visits them"""
    n_samples = min(n_images, n_samples)
    random.seed(seed)
    return random.sample(range(n_images), n_samples)


def loadGroundTruth(data_folder):
    """data/<folder>/ground_truth.npz with both key spellings (knn_images.py:55-59).
    :return: (true_states, images_path, ground_truth npz)"""
    ground_truth = np.load('data/{}/ground_truth.npz'.format(data_folder))
    keys = list(ground_truth.keys())
    true_states = ground_truth['ground_truth_states' if 'ground_truth_states' in keys else 'arm_states']
    return true_states, ground_truth['images_path'], ground_truth


def relativePositions(true_states, target_positions, episode_starts):
    """true_states[i] - target_positions[episode of i] (knn_images.py:62-71), on a copy."""
    true_states = np.array(true_states, copy=True)
    episode_idx = -1
    for i in range(len(episode_starts)):
        if episode_starts[i] == 1:
            episode_idx += 1
        true_states[i] -= target_positions[episode_idx]
    return true_states


def imageTitle(image_path):
    """'<record folder>/<frame name>' (knn_images.py:101-103)."""
    image_path = str(image_path)
    return '{}/{}'.format(image_path.split("/")[1], image_path.split("/")[-1].split(".")[0])


def knnMse(true_states, images_path, picks, neighbors_indices, n_neighbors):
    """The error loop of knn_images.py:95-169 without its figures.
    :param picks: the sampled image indices, in order
    :param neighbors_indices: one row per pick, the pick itself in position 0 (dropped, as the reference drops it) and its
        n_neighbors nearest neighbours behind it
    :return: (titles, mean_error) — mean_error unrounded; the result file holds round(mean_error, 5)"""
    n_images, total_error = 0, 0
    images_titles = []
    for image_idx, neigbour_indices in zip(picks, neighbors_indices):
        ref_coord = true_states[image_idx]
        images_titles.append(imageTitle(images_path[image_idx]))
        for i in range(0, n_neighbors):
            neighbor_coord = true_states[neigbour_indices[i + 1]]
            total_error += np.linalg.norm(neighbor_coord - ref_coord) ** 2
            n_images += 1
    return images_titles, total_error / n_images


def resultDict(images_titles, mean_error):
    return {'images': images_titles, 'knn_mse': round(mean_error, 5)}


def loadEvaluationInputs(log_folder, relative_pos=False, ground_truth=False):
    """What the reference reads (knn_images.py:51-77).
    :return: (states the search runs on, true_states, images_path)"""
    with open("{}/exp_config.json".format(log_folder), 'r') as f:
        data_folder = json.load(f)['data-folder']
    true_states, images_path, gt = loadGroundTruth(data_folder)
    if relative_pos:
        print("Using relative position")
        episode_starts = np.load('data/{}/preprocessed_data.npz'.format(data_folder))['episode_starts']
        keys = list(gt.keys())
        target_positions = gt['target_positions' if 'target_positions' in keys else 'button_positions']
        true_states = relativePositions(true_states, target_positions, episode_starts)
    if ground_truth:
        print("Using ground_truth")
        states = true_states.copy()
    else:
        states = np.load('{}/states_rewards.npz'.format(log_folder))['states']
    return states, true_states, images_path


def sampledNeighbors(states, picks, n_neighbors):
    """Rows `picks` of what kneighbors(states) returns with n_neighbors + 1 neighbours: the exact search on the GPU, the sampled
    rows as queries against all N states.  (float64 states — --ground-truth — are searched unrounded.)
    :return: (idx int64 [len(picks), n_neighbors + 1], distances float64, the same shape — Euclidean, as sklearn's)"""
    from srlz import ops
    states = np.asarray(states)
    if states.dtype not in (np.float32, np.float64):
        states = states.astype(np.float64)
    idx, dist2 = ops.knn(states, n_neighbors + 1, queries=states[np.asarray(picks, dtype=np.int64)])
    return idx, np.sqrt(dist2)


def main(argv=None):
    args = buildParser().parse_args(argv)
    states, true_states, images_path = loadEvaluationInputs(args.log_folder, args.relative_pos, args.ground_truth)
    printYellow("knn_images: no figure is drawn (--n-to-plot {} ignored): plotting is out of scope of this build".format(
        args.n_to_plot))
    print("Computing KNN... with k={}".format(args.n_neighbors))
    print('\nUsing a random test set of images for KNN MSE evaluation...')
    print('seed={}\n'.format(args.seed))
    picks = sampleIndices(len(images_path), args.n_samples, args.seed)
    neighbors_indices, _ = sampledNeighbors(states, picks, args.n_neighbors)
    images_titles, mean_error = knnMse(true_states, images_path, picks, neighbors_indices, args.n_neighbors)
    print("KNN MSE: {}".format(mean_error))
    with open("{}/knn_mse.json".format(args.log_folder), 'w') as f:
        json.dump(resultDict(images_titles, mean_error), f)
    return 0


if __name__ == '__main__':
    main()
