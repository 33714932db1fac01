"""sklearn.decomposition.IncrementalPCA (what reference srl_baselines/pca.py:104-118 fits and applies), MI355X-native.

sklearn's partial_fit decomposes, per minibatch, the matrix A = [ S·V ; X - batch_mean ; mean_correction ] with one LAPACK SVD on
the host (r = k + bs + 1 rows, D = 150 528 columns, float32).  Here A is never written: csrc/pca.hip forms its rows where they are
read and accumulates the small Gram matrix G = A·Aᵀ in fp64 (srlz_pca_gram); the host takes numpy.linalg.eigh of the r x r matrix —
the only D2H copy of a minibatch — and the k leading eigenvectors come back as the new basis S·V = Uᵀ·A (srlz_pca_project).  The
algorithm is sklearn 1.7's step for step, including the truncation to k components after every minibatch (an exact PCA of all
frames gives different states): _incremental_mean_and_var (srlz_pca_stats), svd_flip(u_based_decision=False), and the attributes
derived from ALL r singular values.  See DESIGN.md 3.9 for the numerical limit of the Gram route.

Fitting needs the GPU (there is no CPU path).  The fitted object pickles as numpy arrays only, and `transform` of numpy frames runs on
the host, so that a pca.pkl can be used anywhere.
"""
from __future__ import print_function, division, absolute_import

import numpy as np

from utils import printYellow

_EPS = float(np.finfo(np.float64).eps)
_ATTRIBUTES = ("components_", "singular_values_", "mean_", "var_", "explained_variance_", "explained_variance_ratio_",
               "noise_variance_", "n_samples_seen_", "n_components_")
TRANSFORM_ROWS = 1024  # frames per srlz_pca_transform launch


def hostLut():
    """The srlz_normalize_lut table on the host: preprocessInput (preprocessing/utils.py) of v = 0..255 per channel, float32 [3, 256]."""
    from preprocessing.utils import preprocessInput
    x = np.repeat(np.arange(256, dtype=np.float32)[:, None, None], 3, axis=2)  # [256, 1, 3]
    return np.ascontiguousarray(preprocessInput(x)[:, 0, :].T)


def leadingEigenpairs(G, k, n_features):
    """What replaces linalg.svd(A): from G = A·Aᵀ (fp64, symmetric), the singular values of A, all of them, and the rows Uᵀ of the k
    leading left singular vectors.  An eigenvalue at or below the rounding floor of G (r * eps * w_max) is a singular value of zero:
    its row of W is zero (so is the component), never a division by it.
    :return: (S_all float64 [min(r, D)] descending, W float64 [k, r], zeroed (int) components without a singular value)"""
    r = G.shape[0]
    w, U = np.linalg.eigh(G)
    order = np.argsort(w)[::-1]
    w, U = w[order], U[:, order]
    floor = r * _EPS * max(w[0], 0.0)
    w = np.where(w > floor, w, 0.0)
    W = np.zeros((k, r), dtype=np.float64)
    top = min(k, r)
    W[:top] = U[:, :top].T
    W[:top][w[:top] <= 0.0] = 0.0
    return np.sqrt(w[:min(r, n_features)]), W, int((w[:top] <= 0.0).sum()) + (k - top)


class IncrementalPCA(object):
    """
    :param n_components: (int) components kept after every minibatch (sklearn's n_components; None is not supported)
    """

    def __init__(self, n_components):
        self.n_components = int(n_components)
        if self.n_components < 1:
            raise ValueError("n_components={} must be a positive integer".format(n_components))
        self._dev = None    # device state: mean, var, bmean, corr [D]; basis 2 x [k, D]; S [k]; which basis is current
        self._host = None   # the attributes as numpy arrays (filled on demand, dropped by the next partial_fit)

    # ---- frames ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _frameArgs(frames):
        """(x_u8, x_f32, lut, plane, m, D, the tensors to keep alive) of a device tensor: uint8 planar [m, C, W, H] or float [m, ...]."""
        import torch as th
        from srlz import ops
        if not isinstance(frames, th.Tensor) or frames.device.type != "cuda":
            raise RuntimeError("IncrementalPCA works on device tensors: there is no CPU path for fitting (use the reference on CPU)")
        if frames.dim() < 2:
            raise ValueError("frames must be [m, ...], got {}".format(tuple(frames.shape)))
        m = int(frames.shape[0])
        if ops.is_u8_frames(frames):
            frames = ops._check_u8(frames, "frames")
            plane = int(frames[0, 0].numel())
            return ops.ptr(frames), None, ops.ptr(ops.norm_lut(frames.device)), plane, m, int(frames[0].numel()), frames
        x = frames.reshape(m, -1)
        if x.dtype != th.float32 or not x.is_contiguous():
            x = x.to(th.float32).contiguous()
        return None, ops.ptr(x), None, 1, m, int(x.shape[1]), x

    # ---- fitting -----------------------------------------------------------------------------------------------------------------
    def partial_fit(self, frames):
        """One minibatch of sklearn's IncrementalPCA.partial_fit.  frames: device tensor, uint8 planar [m, C, W, H] (normalised
        through the table while it is read) or float [m, ...]."""
        import torch as th
        from srlz import _cabi as C
        from srlz import ops
        from models.learner import _requireGpu
        _requireGpu(True)
        x_u8, x_f32, lut, plane, m, D, keep = self._frameArgs(frames)
        k = self.n_components
        first = self._dev is None
        if first and self._host is not None:
            raise RuntimeError("an unpickled IncrementalPCA holds no device state: it transforms, it cannot be fitted further")
        if k > D:
            raise ValueError("n_components=%r invalid for n_features=%d, need more rows than columns for IncrementalPCA "
                             "processing" % (k, D))
        if first and k > m:
            raise ValueError("n_components={} must be less or equal to the batch number of samples {} for the first partial_fit "
                             "call.".format(k, m))
        device = keep.device
        if first:
            f64 = dict(dtype=th.float64, device=device)
            self._dev = {"D": D, "n": 0, "mean": th.zeros(D, **f64), "var": th.zeros(D, **f64), "bmean": th.empty(D, **f64),
                         "corr": th.empty(D, **f64), "basis": [th.zeros(k, D, **f64), th.zeros(k, D, **f64)], "cur": 0,
                         "S": th.zeros(k, **f64), "batches": 0}
        d = self._dev
        if D != d["D"]:
            raise ValueError("Number of input features has changed from {} to {} between calls to partial_fit".format(d["D"], D))
        n = d["n"]
        s = ops.stream()
        C.pca_stats(x_u8, x_f32, lut, plane, m, D, n, ops.ptr(d["mean"]), ops.ptr(d["var"]), ops.ptr(d["bmean"]), ops.ptr(d["corr"]), s)
        r = m if first else k + m + 1
        nbytes = C.pca_workspace(r, D)
        ws = th.empty(max(nbytes, 1), dtype=th.uint8, device=device)
        G = th.empty((r, r), dtype=th.float64, device=device)
        old, new = d["basis"][d["cur"]], d["basis"][1 - d["cur"]]
        C.pca_gram(ops.ptr(old), k, int(first), x_u8, x_f32, lut, plane, m, ops.ptr(d["bmean"]), ops.ptr(d["corr"]), D, ops.ptr(G),
                   ops.ptr(ws), nbytes, s)
        # the minibatch's one D2H copy (and its synchronisation): G, and behind it the sum of the column variances
        G_host = th.cat((G.reshape(-1), d["var"].sum().reshape(1))).cpu().numpy()
        G_host, var_sum = G_host[:-1].reshape(r, r), float(G_host[-1])
        S_all, W, zeroed = leadingEigenpairs(G_host, k, D)
        if zeroed:
            printYellow("IncrementalPCA: {} of {} components have no singular value (fewer distinct frames than components): "
                        "they are zero rows".format(zeroed, k))
        W_dev = th.from_numpy(W).to(device)
        C.pca_project(ops.ptr(W_dev), ops.ptr(old), k, int(first), x_u8, x_f32, lut, plane, m, ops.ptr(d["bmean"]), ops.ptr(d["corr"]),
                      D, ops.ptr(new), s)
        # svd_flip(u_based_decision=False): the entry of largest magnitude of every row of V (of S·V alike) is positive
        pick = new.abs().argmax(dim=1, keepdim=True)
        new.mul_(th.sign(new.gather(1, pick)))
        S = np.zeros(k, dtype=np.float64)
        S[:min(k, len(S_all))] = S_all[:k]
        d["S"].copy_(th.from_numpy(S))
        d["cur"] = 1 - d["cur"]
        n_total = n + m
        d["n"] = n_total
        d["batches"] += 1
        # the attributes sklearn derives from ALL singular values (partial_fit: explained_variance ... noise_variance_)
        with np.errstate(divide="ignore", invalid="ignore"):
            explained_variance = S_all ** 2 / (n_total - 1)
            explained_variance_ratio = S_all ** 2 / (var_sum * n_total)
        pad = np.zeros(max(0, k - len(S_all)))
        noise = float(explained_variance[k:].mean()) if k not in (m, D) and len(explained_variance) > k else 0.0
        d["scalars"] = {"singular_values_": S, "explained_variance_": np.concatenate((explained_variance, pad))[:k],
                        "explained_variance_ratio_": np.concatenate((explained_variance_ratio, pad))[:k], "noise_variance_": noise}
        self._host = None
        return self

    def _attributes(self):
        """The fitted attributes under sklearn's names, as numpy arrays in the dtypes sklearn gives float32 input."""
        if self._host is None:
            if self._dev is None:
                raise AttributeError("This IncrementalPCA instance is not fitted yet")
            d = self._dev
            S = d["scalars"]["singular_values_"]
            basis = d["basis"][d["cur"]].cpu().numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                components = np.where(S[:, None] > 0.0, basis / S[:, None], 0.0)
            # sklearn's dtypes for float32 frames: its SVD runs in float32 on the first minibatch only — from the second one np.vstack
            # with the float64 correction row makes the matrix, and everything derived from it, float64; mean_, var_ and the ratio
            # (divided by a float64 sum) are float64 throughout
            svd = np.float32 if d["batches"] == 1 else np.float64
            self._host = {"components_": components.astype(svd), "singular_values_": S.astype(svd),
                          "mean_": d["mean"].cpu().numpy(), "var_": d["var"].cpu().numpy(),
                          "explained_variance_": d["scalars"]["explained_variance_"].astype(svd),
                          "explained_variance_ratio_": d["scalars"]["explained_variance_ratio_"].astype(np.float64),
                          "noise_variance_": svd(d["scalars"]["noise_variance_"]), "n_samples_seen_": int(d["n"]),
                          "n_components_": self.n_components}
        return self._host

    def __getattr__(self, name):
        if name in _ATTRIBUTES:
            return self._attributes()[name]
        raise AttributeError(name)

    # ---- transform ---------------------------------------------------------------------------------------------------------------
    def transform(self, frames):
        """(X - mean_)·components_ᵀ, accumulated in fp64 and returned as float32 numpy [M, k] (what states_rewards.npz holds for every
        other method of this build; sklearn returns float64 here).  Device tensors (uint8 planar or float) go through srlz_pca_transform
        and need the fitted state on the device; numpy frames (float [M, ...], or uint8 planar [M, C, W, H]) are transformed on the
        host from the numpy attributes — the only CPU code of the baseline, for an unpickled pca.pkl."""
        if isinstance(frames, np.ndarray):
            return self._transformHost(frames)
        import torch as th
        from srlz import _cabi as C
        from srlz import ops
        if self._dev is None:
            raise RuntimeError("transform of device tensors needs the fitted state on the device (an unpickled object transforms "
                               "numpy frames on the host)")
        d = self._dev
        k = self.n_components
        out = []
        for a in range(0, int(frames.shape[0]), TRANSFORM_ROWS):
            x_u8, x_f32, lut, plane, M, D, keep = self._frameArgs(frames[a:a + TRANSFORM_ROWS])
            if D != d["D"]:
                raise ValueError("frames have {} features, the fitted PCA {}".format(D, d["D"]))
            nbytes = C.pca_transform_workspace(M, k, D)
            ws = th.empty(max(nbytes, 1), dtype=th.uint8, device=keep.device)
            states = th.empty((M, k), dtype=th.float32, device=keep.device)
            C.pca_transform(x_u8, x_f32, lut, plane, M, ops.ptr(d["mean"]), ops.ptr(d["basis"][d["cur"]]), ops.ptr(d["S"]), k, D,
                            ops.ptr(states), ops.ptr(ws), nbytes, ops.stream())
            out.append(states.cpu().numpy())
        return np.concatenate(out, axis=0) if out else np.zeros((0, k), dtype=np.float32)

    def _transformHost(self, frames):
        at = self._attributes()
        if frames.dtype == np.uint8:
            if frames.ndim != 4 or frames.shape[1] not in (3, 6, 9):
                raise ValueError("uint8 frames must be [M, C, W, H] planar with C in (3, 6, 9), got {}".format(frames.shape))
            lut = hostLut()
            frames = np.stack([lut[c % 3][frames[:, c]] for c in range(frames.shape[1])], axis=1)
        X = np.asarray(frames, dtype=np.float64).reshape(len(frames), -1)
        if X.shape[1] != at["mean_"].shape[0]:
            raise ValueError("frames have {} features, the fitted PCA {}".format(X.shape[1], at["mean_"].shape[0]))
        return ((X - at["mean_"]) @ at["components_"].astype(np.float64).T).astype(np.float32)

    # ---- pickling: numpy arrays only -----------------------------------------------------------------------------------------------
    def __getstate__(self):
        return {"n_components": self.n_components, "fitted": dict(self._attributes()) if (self._dev or self._host) else None}

    def __setstate__(self, state):
        self.n_components = state["n_components"]
        self._dev = None
        self._host = state["fitted"]

    @classmethod
    def fromAttributes(cls, **fitted):
        """An object that transforms on the host, from the fitted attributes (sklearn's names) — e.g. the fields of a pca.pkl."""
        missing = [a for a in ("components_", "mean_") if a not in fitted]
        if missing:
            raise ValueError("fromAttributes needs {}".format(missing))
        self = cls(int(np.asarray(fitted["components_"]).shape[0]))
        self._host = {"n_components_": self.n_components}
        self._host.update({k: (np.asarray(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in fitted.items()})
        return self
