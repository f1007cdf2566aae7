"""KMeans for the SAL pose clusters -- drop-in for the reference's ``sklearn.cluster.KMeans(NUM_CLUSTERS,
random_state=RANDOM_SEED).fit(kp_values)`` (strategy.py:38-52) and ``kmeans.predict`` (strategy.py:981-989).

The fit runs on the device (csrc/kmeans.hip: k-means++ seeding, Lloyd iterations, empty-cluster relocation, all in
float64 with a fixed reduction order).  Only the random draws stay on the host, in sklearn 1.7.2's order, so that
a given ``random_state`` picks the same initial centres as sklearn does.
"""
from __future__ import annotations

import numbers
import warnings

import numpy as np
import torch

from .. import _lib

try:  # the same warning class as sklearn's, when sklearn is installed (filters written for it keep working)
    from sklearn.exceptions import ConvergenceWarning
except ImportError:  # pragma: no cover - depends on the environment
    class ConvergenceWarning(UserWarning):
        """Fewer distinct clusters than requested (sklearn.exceptions.ConvergenceWarning)."""


def check_random_state(seed):
    """sklearn.utils.check_random_state: None -> numpy's global RandomState, int -> a new RandomState(seed),
    a RandomState -> itself."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError("%r cannot be used to seed a numpy.random.RandomState instance" % (seed,))


def n_local_trials(n_clusters):
    """Candidates per greedy k-means++ step (sklearn: 2 + int(log(n_clusters)))."""
    return 2 + int(np.log(n_clusters))


def draw_plusplus(random_state, n_samples, n_clusters):
    """The random numbers of one k-means++ initialisation, drawn in sklearn's stream order (``_kmeans_plusplus``
    with unit sample weights): the first centre's index, then ``n_local_trials`` uniforms per further centre.
    Returns (first_idx, rand_u of shape ((n_clusters - 1) * n_local_trials,))."""
    trials = n_local_trials(n_clusters)
    first = int(random_state.choice(n_samples, p=np.full(n_samples, 1.0 / n_samples)))
    u = [random_state.uniform(size=trials) for _ in range(n_clusters - 1)]
    return first, (np.concatenate(u) if u else np.zeros(0, dtype=np.float64))


def _is_same_clustering(labels1, labels2, n_clusters):
    """sklearn's _is_same_clustering: the two labelings are equal up to a permutation of the labels."""
    mapping = np.full(n_clusters, -1, dtype=np.int64)
    for a, b in zip(labels1.tolist(), labels2.tolist()):
        if mapping[a] == -1:
            mapping[a] = b
        elif mapping[a] != b:
            return False
    return True


def _device():
    return torch.device("cuda", torch.cuda.current_device())


class KMeans:
    """sklearn.cluster.KMeans (1.7.2) with Lloyd's algorithm on the device.

    ``X`` may be a numpy array (or anything ``np.asarray`` takes) or a torch tensor, on the host or on the device.
    Every other dtype is converted to float64: the fit always runs in float64.  Supported: ``init`` =
    "k-means++" or an (n_clusters, n_features) array, ``n_init`` = "auto" or an int, ``max_iter``, ``tol`` and
    ``random_state`` (None, an int or a numpy RandomState).  ``sample_weight`` and ``algorithm="elkan"`` raise
    NotImplementedError.

    After ``fit``: ``cluster_centers_`` (K, D) float64, ``labels_`` (n,) int32, ``inertia_``, ``n_iter_`` (numpy /
    python values, as sklearn's) and ``init_indices_`` (one row of k-means++ picks per initialisation, -1 for an
    array ``init``)."""

    def __init__(self, n_clusters=8, *, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, random_state=None,
                 algorithm="lloyd"):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.random_state = random_state
        self.algorithm = algorithm

    # ---- checks that need no device ---------------------------------------------------------------------
    def _check_params(self, n_samples, n_features):
        if self.algorithm == "elkan":
            raise NotImplementedError("KMeans: algorithm='elkan' is not implemented (use 'lloyd')")
        if self.algorithm != "lloyd":
            raise ValueError("KMeans: algorithm must be 'lloyd', got %r" % (self.algorithm,))
        if not isinstance(self.n_clusters, numbers.Integral) or self.n_clusters < 1:
            raise ValueError("n_clusters must be an int >= 1, got %r" % (self.n_clusters,))
        if not isinstance(self.max_iter, numbers.Integral) or self.max_iter < 1:
            raise ValueError("max_iter must be an int >= 1, got %r" % (self.max_iter,))
        if not self.tol >= 0:
            raise ValueError("tol must be >= 0, got %r" % (self.tol,))
        if n_samples < self.n_clusters:
            raise ValueError(f"n_samples={n_samples} should be >= n_clusters={self.n_clusters}.")
        init_is_array = not isinstance(self.init, str)
        if not init_is_array and self.init != "k-means++":
            raise NotImplementedError("KMeans: init=%r is not implemented (use 'k-means++' or an array)" % (self.init,))
        if callable(self.init):
            raise NotImplementedError("KMeans: a callable init is not implemented")
        init = None
        if init_is_array:
            init = np.array(self.init, dtype=np.float64, copy=True)
            if init.shape != (self.n_clusters, n_features):
                raise ValueError(
                    f"The shape of the initial centers {init.shape} does not match the number of clusters "
                    f"{self.n_clusters} or the number of features {n_features}.")
            if not np.isfinite(init).all():
                raise ValueError("init contains NaN or infinity.")
        if self.n_init == "auto":
            n_init = 1
        elif isinstance(self.n_init, numbers.Integral) and self.n_init >= 1:
            n_init = int(self.n_init)
        else:
            raise ValueError("n_init must be 'auto' or an int >= 1, got %r" % (self.n_init,))
        if init_is_array and n_init != 1:
            warnings.warn(
                "Explicit initial center position passed: performing only one init in KMeans instead of "
                f"n_init={n_init}.", RuntimeWarning, stacklevel=3)
            n_init = 1
        return init, n_init

    @staticmethod
    def _host_array(X):
        """X as a float64 numpy array when it is not a tensor (checked here, before any device work)."""
        if torch.is_tensor(X):
            return None
        x = np.asarray(X, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("Expected a 2D array, got an array of shape %s" % (x.shape,))
        if not np.isfinite(x).all():
            raise ValueError("Input X contains NaN or infinity.")
        return np.ascontiguousarray(x)

    @staticmethod
    def _to_device(X, host):
        if host is not None:
            return torch.from_numpy(host).to(_device())
        if X.dim() != 2:
            raise ValueError("Expected a 2D tensor, got shape %s" % (tuple(X.shape),))
        x = X.to(_device() if not X.is_cuda else X.device, torch.float64).contiguous()
        if not bool(torch.isfinite(x).all().item()):
            raise ValueError("Input X contains NaN or infinity.")
        return x

    # ---- public API -------------------------------------------------------------------------------------
    def fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("KMeans: sample_weight is not implemented (unit weights only)")
        host = self._host_array(X)
        if host is None and X.dim() != 2:
            raise ValueError("Expected a 2D tensor, got shape %s" % (tuple(X.shape),))
        n, d = host.shape if host is not None else tuple(X.shape)
        init, n_init = self._check_params(n, d)
        random_state = check_random_state(self.random_state)
        x = self._to_device(X, host)
        k = int(self.n_clusters)
        trials = n_local_trials(k)
        init_dev = None if init is None else torch.from_numpy(init).to(x.device)
        best = None
        picks = []
        for _ in range(n_init):
            if init_dev is None:
                first, u = draw_plusplus(random_state, n, k)
                u_dev = torch.from_numpy(u).to(x.device) if u.size else None
                res = _lib.kmeans_fit(x, k, None, first, u_dev, trials, int(self.max_iter), float(self.tol))
            else:
                res = _lib.kmeans_fit(x, k, init_dev, 0, None, 1, int(self.max_iter), float(self.tol))
            centers, labels, inertia, n_iter, init_idx = res
            labels_h = labels.cpu().numpy()
            inertia_h = float(inertia.item())
            picks.append(init_idx.cpu().numpy())
            # sklearn: a later run wins only with a lower inertia AND a different clustering (rounding can give a
            # slightly lower inertia for the same clustering)
            if best is None or (inertia_h < best[2] and not _is_same_clustering(labels_h, best[1], k)):
                best = (centers, labels_h, inertia_h, int(n_iter.item()))
        self._centers_dev = best[0]
        self.cluster_centers_ = best[0].cpu().numpy()
        self.labels_ = best[1]
        self.inertia_ = best[2]
        self.n_iter_ = best[3]
        self.init_indices_ = np.stack(picks)
        self.n_features_in_ = d
        distinct = len(np.unique(self.labels_))
        if distinct < k:
            warnings.warn(
                "Number of distinct clusters ({}) found smaller than n_clusters ({}). Possibly due to duplicate "
                "points in X.".format(distinct, k), ConvergenceWarning, stacklevel=2)
        return self

    def predict(self, X):
        """Index of the nearest centre of every row (first minimum of |c|^2 - 2 x.c, as sklearn) -> (n,) int32."""
        if not hasattr(self, "cluster_centers_"):
            raise ValueError("This KMeans instance is not fitted yet. Call 'fit' first.")
        host = self._host_array(X)
        x = self._to_device(X, host)
        if x.shape[1] != self.n_features_in_:
            raise ValueError("X has %d features, but KMeans is expecting %d features as input."
                             % (x.shape[1], self.n_features_in_))
        centers = self._centers_dev
        if centers.device != x.device:
            centers = centers.to(x.device)
        return _lib.nearest_center(x, centers).cpu().numpy()

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_
