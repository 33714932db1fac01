"""Pair mining for the robotic priors (reference losses/utils.py:7-116): which rows of a minibatch took the same action, and which
of those were rewarded differently.  Same names, arguments, return values, printed lines and in-place effects as the reference:

    dissimilar_pairs, same_actions_pairs = findPriorsPairs(batch_size, minibatchlist, actions, rewards, n_actions, n_pairs_per_action)

Row i of a minibatch is the transition (frame m[i], frame m[i] + 1): its action is actions[m[i]], its reward rewards[m[i] + 1].
A pair [i, j] holds POSITIONS inside its minibatch, i < j, in generation order (i ascending, then j ascending).

What the reference does and this keeps, index for index (tests/golden/robotic_kats.npz is recorded from it):
  * overSampling runs for every minibatch k without a dissimilar pair.  It scans all minibatches m in list order, positions i
    ascending, and the positions j of findDissimilar(i, m_list[k], m_list[m]); at the first hit with j != i and m != k it overwrites
    m_list[k][j] = m_list[m][j] IN PLACE and that minibatch's dissimilar pairs become the single pair [[i, j]] (j < i is possible).
    The minibatch may then be unsorted and may hold a frame twice; later minibatches see the modified list.
  * the same-action pairs are computed after that modification; n_pairs_per_action is added to in place.
Where the reference does not reach what it means to do, the intended behaviour is built:
  * a minibatch left without a pair of either kind: the reference calls sys.exit without importing sys; here its message is printed
    and the process exits with pipeline.NO_PAIRS_ERROR;
  * a minibatch without a dissimilar pair to which no other minibatch can donate: the reference's loop never ends; here the same exit.

priors_pairs is the same function raising NoPairsError (a ValueError) instead of exiting; library code calls that one.
"""
from __future__ import print_function, division, absolute_import

import sys

import numpy as np

from pipeline import NO_PAIRS_ERROR
from utils import printRed


class NoPairsError(ValueError):
    """A minibatch has no same-action pair or no dissimilar pair, and none can be sampled for it."""


def _no_pairs_message(batch_size):
    return ("No same actions or dissimilar pairs found for at least one minibatch (currently is {})\n"
            "=> Consider increasing the batch_size or changing the seed".format(batch_size))


def findDissimilar(index, minibatch1, minibatch2, actions, rewards):
    """Positions of minibatch2 whose transition took the action of minibatch1[index] and was rewarded differently.
    :param index: (int)
    :param minibatch1: (np.ndarray)
    :param minibatch2: (np.ndarray)
    :param actions: (np.ndarray)
    :param rewards: (np.ndarray)
    :return: (np.ndarray)
    """
    frame = minibatch1[index]
    same_action = actions[minibatch2] == actions[frame]
    other_reward = rewards[minibatch2 + 1] != rewards[frame + 1]
    return np.where(same_action * other_reward)[0]


def findSameActions(index, minibatch, actions):
    """Positions of the minibatch whose transition took the action of minibatch[index] (itself included).
    :param index: (int)
    :param minibatch: (np.ndarray)
    :param actions: (np.ndarray)
    :return: (np.ndarray)
    """
    return np.where(actions[minibatch] == actions[minibatch[index]])[0]


def _donate(batch_size, m_list, k, function_on_pairs, actions, rewards):
    """The first (i, j) in scan order that another minibatch can donate to minibatch k, written into m_list[k]; None without one."""
    for m_id, minibatch in enumerate(m_list):
        if m_id == k:
            continue
        for i in range(batch_size):
            for j in function_on_pairs(i, m_list[k], minibatch, actions, rewards):
                if j != i:
                    m_list[k][j] = minibatch[j]
                    return i, int(j)
    return None


def _over_sampling(batch_size, m_list, pairs, function_on_pairs, actions, rewards):
    pair_name = 'dissimilar pairs' if function_on_pairs.__name__ == "findDissimilar" else 'Unknown pairs'
    counter, stuck = 0, []
    for k in range(len(pairs)):
        if len(pairs[k]) > 0:
            continue
        counter += 1
        hit = _donate(batch_size, m_list, k, function_on_pairs, actions, rewards)
        if hit is None:
            stuck.append(k)
        else:
            pairs[k] = np.array([list(hit)])
    print('Dealt with {} minibatches - {}'.format(counter, pair_name))
    return pairs, m_list, stuck


def overSampling(batch_size, m_list, pairs, function_on_pairs, actions, rewards):
    """For every minibatch without a pair, take one observation from another minibatch so that it has one (see the module's text).
    :param batch_size: (int)
    :param m_list: (list) mini-batch list, modified in place
    :param pairs: ([np.ndarray]) pairs per minibatch, modified in place
    :param function_on_pairs: (function) findDissimilar
    :param actions: (np.ndarray)
    :param rewards: (np.ndarray)
    :return: (list, list) pairs, mini-batch list
    """
    pairs, m_list, stuck = _over_sampling(batch_size, m_list, pairs, function_on_pairs, actions, rewards)
    if stuck:
        printRed(_no_pairs_message(batch_size))
        sys.exit(NO_PAIRS_ERROR)
    return pairs, m_list


def _pairs_of(batch_size, find):
    return np.array([[i, j] for i in range(batch_size) for j in find(i) if j > i], dtype='int64')


def priors_pairs(batch_size, minibatchlist, actions, rewards, n_actions, n_pairs_per_action):
    """findPriorsPairs, raising NoPairsError where that exits.  Arguments, return values, printed lines and in-place effects are
    findPriorsPairs's."""
    dissimilar_pairs = [_pairs_of(batch_size, lambda i, m=minibatch: findDissimilar(i, m, m, actions, rewards))
                        for minibatch in minibatchlist]
    dissimilar_pairs, minibatchlist, stuck = _over_sampling(batch_size, minibatchlist, dissimilar_pairs, findDissimilar, actions,
                                                            rewards)
    if stuck:
        raise NoPairsError(_no_pairs_message(batch_size))
    same_actions_pairs = [_pairs_of(batch_size, lambda i, m=minibatch: findSameActions(i, m, actions)) for minibatch in minibatchlist]

    for pair, minibatch in zip(same_actions_pairs, minibatchlist):
        if len(pair) == 0:
            continue
        first = actions[minibatch[pair[:, 0]]]
        for i in range(n_actions):
            n_pairs_per_action[i] += np.sum(first == i)

    print("Number of pairs per action:")
    print(n_pairs_per_action)
    print("Pairs of {} unique actions".format(np.sum(n_pairs_per_action > 0)))

    for item in same_actions_pairs + dissimilar_pairs:
        if len(item) == 0:
            raise NoPairsError(_no_pairs_message(batch_size))
    return dissimilar_pairs, same_actions_pairs


def findPriorsPairs(batch_size, minibatchlist, actions, rewards, n_actions, n_pairs_per_action):
    """
    :param batch_size: (int)
    :param minibatchlist: ([np.ndarray]) frame indices per minibatch, modified in place by the over-sampling
    :param actions: (np.ndarray)
    :param rewards: (np.ndarray)
    :param n_actions: (int)
    :param n_pairs_per_action: (np.ndarray) added to in place
    :return: ([np.ndarray], [np.ndarray]) dissimilar pairs, same-action pairs
    """
    try:
        return priors_pairs(batch_size, minibatchlist, actions, rewards, n_actions, n_pairs_per_action)
    except NoPairsError as e:
        printRed(str(e))
        sys.exit(NO_PAIRS_ERROR)
