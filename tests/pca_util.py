"""Shared by the PCA baseline's tests and tools/make_golden_pca.py: the matrix cases, the fixtures, and an fp64 numpy restatement of
one minibatch of the Gram route (srl_baselines/ipca.py on csrc/pca.hip)."""
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (N, C, W, H, bs, k)
CASES = [
    (37, 3, 7, 9, 4, 3),      # D = 189: less than one chunk of columns, no multiple of 4; r = 8 < 16; ragged last minibatch of 1 row
    (70, 3, 37, 29, 16, 5),   # D = 3 219; r = 22: two partial tiles
    (50, 6, 17, 13, 18, 17),  # r = 36: three tiles; six channels; last minibatch of 14 rows < k
    (32, 3, 7, 9, 16, 3),     # N a multiple of bs: the empty trailing range
]
PARITY = 1e-4  # the project's parity bound for outputs


def case_name(case):
    return "n%d_c%d_w%d_h%d_bs%d_k%d" % tuple(case)


def column_subsample(D):
    """Columns 0, s, 2 s, ... with the smallest stride s that leaves at most 64 of them."""
    return np.arange(0, D, max(1, -(-D // 64)))


def minibatches(n_samples, batch_size):
    """DataLoader.createTestMinibatchList of the reference (preprocessing/data_loader.py): the last range may be empty."""
    return [np.arange(i * batch_size, min(n_samples, (i + 1) * batch_size)) for i in range(n_samples // batch_size + 1)]


def load_kats():
    with np.load(os.path.join(GOLDEN_DIR, "pca_kats.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def load_spread():
    with open(os.path.join(GOLDEN_DIR, "pca_spread.json")) as f:
        return json.load(f)["cases"]


def tolerance(spread_of_case):
    """max(1e-4, 10 x the case's recorded spread): the parity bound, or ten times what float32 LAPACK moves sklearn's own result."""
    return max(PARITY, 10.0 * max(spread_of_case.values()))


def normalised(frames, lut):
    """uint8 planar [N, C, W, H] -> float64 [N, C * W * H] through the float32 table (channel c reads row c % 3)."""
    N, C = frames.shape[:2]
    return np.stack([lut[c % 3][frames[:, c]] for c in range(C)], axis=1).reshape(N, -1).astype(np.float64)


class NumpyIPCA(object):
    """sklearn's IncrementalPCA.partial_fit restated in fp64 numpy along the Gram route, one minibatch at a time; keeps every
    intermediate the kernels produce (bmean, corr, A, G, the new basis)."""

    def __init__(self, k):
        self.k, self.n = k, 0
        self.mean = self.var = self.basis = self.S = None

    def stats(self, X):
        """sklearn.utils.extmath._incremental_mean_and_var, the batch mean and the mean-correction row."""
        m, n = len(X), self.n
        new_sum = X.sum(0)
        T = new_sum / m
        temp = X - T
        new_unnorm = (temp ** 2).sum(0) - temp.sum(0) ** 2 / m
        if n == 0:
            mean, unnorm, corr = new_sum / m, new_unnorm, np.zeros_like(T)
        else:
            last_sum, ratio = self.mean * n, n / m
            mean = (last_sum + new_sum) / (n + m)
            unnorm = self.var * n + new_unnorm + ratio / (n + m) * (last_sum / ratio - new_sum) ** 2
            corr = np.sqrt(n / (n + m) * m) * (self.mean - T)
        return mean, unnorm / (n + m), T, corr

    def matrix(self, X, bmean, corr):
        if self.n == 0:
            return X - bmean
        return np.vstack([self.basis, X - bmean, corr])

    def partial_fit(self, X):
        X = np.asarray(X, dtype=np.float64)
        mean, var, bmean, corr = self.stats(X)
        A = self.matrix(X, bmean, corr)
        G = A.dot(A.T)
        w, U = np.linalg.eigh(G)
        order = np.argsort(w)[::-1][:self.k]
        W = U[:, order].T
        basis = W.dot(A)
        pick = np.abs(basis).argmax(1)
        basis = basis * np.sign(basis[np.arange(self.k), pick])[:, None]
        step = dict(bmean=bmean, corr=corr, A=A, G=G, W=W, old_basis=self.basis, first=self.n == 0, n_seen=self.n)
        self.mean, self.var, self.basis, self.S = mean, var, basis, np.sqrt(np.maximum(w[order], 0.0))
        self.n += len(X)
        step.update(mean=mean, var=var, basis=basis, S=self.S)
        return step

    def transform(self, X):
        return (np.asarray(X, dtype=np.float64) - self.mean).dot((self.basis / self.S[:, None]).T)
