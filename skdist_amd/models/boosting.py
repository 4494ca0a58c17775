"""
Gradient-boosted trees on the batched histogram builder.

The reference's answer to boosting was a pass-through: an xgboost/catboost
estimator riding the task fan-out (reference README.rst:158-166,
test_spark.py:165-187 — xgboost is NOT vendored).  This module gives the
engine a native boosted family with the sklearn GradientBoosting API so
boosted workloads exist without external packages, built on the SAME
binned dataset + level-synchronous tree builder as the forests
(models/forest.py; HIP kernels on GPU, eager torch mirror on CPU):

  * X is quantile-binned ONCE; every boosting round fits its tree(s)
    against the same HBM-resident codes — only the per-row gradient
    vector changes between rounds (updated in place in ``ds.y_f``);
  * trees are least-squares HistTrees on the loss gradients; leaf values
    are then refit with the one-step Newton update sklearn's
    BinomialDeviance / MultinomialDeviance uses (Σ residual / Σ p(1-p)),
    so classification quality tracks sklearn's GradientBoosting to
    tolerance rather than plain gradient-fitting;
  * ``subsample`` < 1 uses an exact 0/1 row mask through the builder's
    weight plane (stochastic gradient boosting).
  * ``n_iter_no_change`` holds out ``validation_fraction`` rows (weight 0
    through the same plane) and stops when their loss stalls for that
    many rounds (sklearn's early-stopping semantics).
  * ``fit(X, y, sample_weight=...)`` (and the classifier's
    ``class_weight=None | "balanced" | dict``, expanded per row and
    multiplied in) rides a real-valued f32 row-weight plane next to the
    codes (``BinnedDataset.row_w``; k_tree_hist_w / k_tree_split_w on
    GPU): every histogram cell holds (Σw, Σw·g, Σw·g², row count), so
    weight sums drive impurity, gain and leaf values while
    ``min_samples_split`` / ``min_samples_leaf`` stay ROW counts
    (sklearn's GradientBoosting semantics).  The initial score is the
    weighted mean / weighted class priors, the Newton leaf refit is
    Σw·g / Σw·h, the validation loss is the weighted mean over the
    held-out rows, and rows of weight 0 are folded into the 0/1 mask so
    they enter no node segment and no count.  A fit without weights
    takes exactly the unweighted code path and kernels.  Not supported:
    ``min_weight_fraction_leaf``; the forests keep their own quantised
    uint8 weight plane.
  * ``allow_nan=True`` lets a dense X hold NaN (never ±inf), at fit and
    at predict.  The binned dataset then keeps its top code for the
    missing cells, every split learns which child they go to (the scan
    weighs both directions of that bin; sklearn's rule, the majority side,
    where a node saw none), and each tree carries the per-node flags
    (``HistTree.missing_left``) that every traversal honours.  On NaN-free
    data such a fit grows the trees of ``allow_nan=False`` with the same
    kernels.  The default keeps raising on NaN, and so does a sparse X
    with a stored NaN in either mode.

The CPU path runs the builder's eager torch mirror — correct and
usable (50 trees on 100k x 20 in ~8 s) but, like the rest of the CPU
tier, a fallback: the production path is the HIP builder on the GPU
(sklearn's dedicated C `HistGradientBoosting*` remains the right tool
for CPU-only deployments).

Fitted state is host numpy only (HistTrees + priors): models pickle and
predict like sklearn estimators and ride every meta-estimator's task
fan-out (DistGridSearchCV and friends) exactly as the reference's
xgboost pass-through did.  Boosting itself is sequential by nature — the
reference never distributed a single boost fit either; parallelism comes
from the within-round device kernels and from fanning out independent
fits (search candidates, OvR classes).
"""

import numpy as np
import torch
from sklearn.base import BaseEstimator, ClassifierMixin, RegressorMixin

from ._sgd import as_dense_f32
from .forest import (BinnedDataset, ForestBuilder, HistTree, canonical_csr,
                     forest_walk)


def _leaf_rows(tree, X):
    """Per-row index into ``tree.value`` (leaf payload row)."""
    return tree.left[tree.apply(X)]


def _leaf_value_rows(tree, X, Xdev, dev):
    """Device int64 [n] of each row's leaf-payload index.  On GPU this
    is one k_forest_apply traversal of the RESIDENT X (no host
    round-trip); on CPU the numpy traversal."""
    if Xdev is None:
        return torch.as_tensor(_leaf_rows(tree, X), dtype=torch.int64,
                               device=dev)
    # a resident CSR X is the tuple (indptr, indices, data)
    n = len(Xdev[0]) - 1 if isinstance(Xdev, tuple) else len(Xdev)
    from ..ops import require_hip

    ext = require_hip()
    as_t = lambda a, dt: torch.as_tensor(
        np.ascontiguousarray(a), dtype=dt, device=dev)
    feat = as_t(tree.feature, torch.int32)
    thr = as_t(tree.threshold, torch.float32)
    left = as_t(tree.left, torch.int32)
    right = as_t(tree.right, torch.int32)
    roots = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(n, 1, dtype=torch.int32, device=dev)
    ml = getattr(tree, "missing_left", None)
    forest_walk(ext, "apply", Xdev, feat, thr, left, right, roots, out,
                mleft=None if ml is None else as_t(ml, torch.uint8))
    return left.index_select(
        0, out[:, 0].to(torch.int64)).to(torch.int64)


def _seg_sum(vrow, vals, nl):
    """Deterministic per-leaf sums: stable sort by leaf + fp64 cumsum
    differencing (GPU scatter_add atomics would be order-dependent)."""
    dev = vals.device
    order = torch.argsort(vrow, stable=True)
    vs = vrow.index_select(0, order)
    xs = vals.index_select(0, order).to(torch.float64)
    cs = torch.zeros(len(xs) + 1, dtype=torch.float64, device=dev)
    torch.cumsum(xs, 0, out=cs[1:])
    ends = torch.searchsorted(
        vs, torch.arange(nl + 1, dtype=vs.dtype, device=dev))
    return cs.index_select(0, ends[1:]) - cs.index_select(0, ends[:-1])


def _wmean(v, w):
    """Mean of ``v``, weighted by ``w`` when given (device fp64)."""
    if w is None:
        return float(v.mean())
    return float((v * w).sum() / w.sum())


class _BaseHistGB(BaseEstimator):
    """NAMING NOTE: despite the ``HistGradientBoosting*`` class names
    (they ARE histogram-binned boosters), the parameter surface is
    sklearn's ``GradientBoosting*`` API (``n_estimators``, ``subsample``,
    ``max_depth=3`` semantics), NOT sklearn's HGB API
    (``l2_regularization``, ``max_leaf_nodes``).  ``max_iter`` is accepted
    as an alias for ``n_estimators`` so HGB-style grids still work; the
    classes are also exported as ``GradientBoostingClassifier`` /
    ``GradientBoostingRegressor``."""

    _is_classifier = False

    def __init__(self, n_estimators=100, learning_rate=0.1, max_depth=3,
                 subsample=1.0, min_samples_split=2, min_samples_leaf=1,
                 max_features=None, n_iter_no_change=None,
                 validation_fraction=0.1, tol=1e-4, random_state=None,
                 max_iter=None, sc=None, allow_nan=False):
        self.max_iter = max_iter
        self.n_estimators = n_estimators
        self.learning_rate = learning_rate
        self.max_depth = max_depth
        self.subsample = subsample
        self.min_samples_split = min_samples_split
        self.min_samples_leaf = min_samples_leaf
        self.max_features = max_features
        self.n_iter_no_change = n_iter_no_change
        self.validation_fraction = validation_fraction
        self.tol = tol
        self.random_state = random_state
        self.sc = sc
        self.allow_nan = allow_nan

    # ------------------------------------------------------------------ #
    def _row_weights(self, y, sample_weight, n):
        """Validated fp64 [n] row weights, or None for an unweighted fit
        (the classifier multiplies its class_weight expansion in)."""
        if sample_weight is None:
            return None
        sw = np.asarray(sample_weight, dtype=np.float64)
        if sw.shape != (n,):
            raise ValueError(
                f"sample_weight must have shape ({n},), got {sw.shape}")
        if not np.isfinite(sw).all():
            raise ValueError("sample_weight must be finite")
        if (sw < 0).any():
            raise ValueError("sample_weight must be non-negative")
        if not sw.sum() > 0:
            raise ValueError("sample_weight must have a positive sum")
        return sw

    def fit(self, X, y, sample_weight=None):
        import scipy.sparse as sp

        sparse = sp.issparse(X)
        if sparse:
            # binned, traversed and kept resident as CSR; never densified
            X = canonical_csr(X)
        else:
            X = as_dense_f32(X)
        n = X.shape[0]
        sc = getattr(self, "sc", None)
        device = (
            sc.device if sc is not None
            else ("cuda" if torch.cuda.is_available() else "cpu")
        )
        # sklearn semantics: random_state=None draws fresh entropy per
        # fit (check_random_state), an int seed is deterministic
        from sklearn.utils import check_random_state

        rng = check_random_state(self.random_state)
        n_rounds = (
            int(self.max_iter) if self.max_iter is not None
            else int(self.n_estimators)
        )

        sw = self._row_weights(y, sample_weight, n)
        if sw is not None:
            # the builder's plane is f32; use the same rounded values in
            # the Newton refit, the priors and the validation loss
            sw = sw.astype(np.float32).astype(np.float64)
            if not sw.sum() > 0:
                raise ValueError("sample_weight must have a positive sum")
        F, K = self._init_raw(y, n, sw)   # raw scores [n, K]; K columns
        ds = BinnedDataset(
            X, np.zeros(n, dtype=np.float32), device, is_cls=False,
            seed=int(rng.randint(1 << 31)),
            row_weight=sw,
            # getattr: estimators pickled before the parameter existed
            allow_missing=bool(getattr(self, "allow_nan", False)),
        )
        builder = ForestBuilder(
            ds, "squared_error", max_depth=self.max_depth,
            min_samples_split=self.min_samples_split,
            min_samples_leaf=self.min_samples_leaf,
            max_features=self.max_features, extra_mode=False,
            bootstrap=False,
        )

        # early stopping: hold out a validation slice whose rows train no
        # tree (weight 0 through the builder's weight plane) and track
        # its loss (sklearn's n_iter_no_change semantics)
        train_mask = None
        val_idx = None
        if self.n_iter_no_change is not None:
            vn = max(1, int(round(self.validation_fraction * n)))
            if vn >= n:
                raise ValueError("validation_fraction leaves no train rows")
            val_idx = rng.permutation(n)[:vn]
            train_mask = np.ones(n, dtype=np.float32)
            train_mask[val_idx] = 0.0
            if sw is not None and not sw[val_idx].sum() > 0:
                raise ValueError(
                    "the validation slice held out for n_iter_no_change "
                    "has zero total sample_weight; early stopping cannot "
                    "score it")
        if sw is not None and (sw == 0).any():
            # zero-weight rows enter no node segment and no count
            nz = (sw > 0).astype(np.float32)
            train_mask = nz if train_mask is None else train_mask * nz
        best_loss = np.inf
        stall = 0

        # the boosting loop runs on DEVICE tensors end to end (round 1
        # re-traversed X on the host twice per round — the measured fit
        # was 75% host time, profiles/r02_boosting_profile.txt): raw
        # scores F, gradients, leaf assignment (k_forest_apply against
        # the resident X) and the Newton leaf sums all stay on ds.device
        dev = ds.device
        Ft = torch.as_tensor(F, dtype=torch.float64, device=dev)
        self._to_device_targets(dev)
        Xdev = None
        if dev.type == "cuda" and sparse:
            Xdev = tuple(
                torch.as_tensor(a, device=dev)
                for a in (X.indptr, X.indices, X.data))
        elif dev.type == "cuda":
            Xdev = torch.as_tensor(
                np.ascontiguousarray(X), device=dev)
        val_t = (
            torch.as_tensor(val_idx, dtype=torch.int64, device=dev)
            if val_idx is not None else None
        )
        sw_t = (
            torch.as_tensor(sw, dtype=torch.float64, device=dev)
            if sw is not None else None
        )
        val_w = (
            sw_t.index_select(0, val_t)
            if sw_t is not None and val_t is not None else None
        )

        stages = []
        for _ in range(n_rounds):
            if self.subsample < 1.0:
                mask = (
                    rng.random_sample(n) < self.subsample
                ).astype(np.float32)
                if mask.sum() < 2:
                    mask[:] = 1.0
            else:
                mask = None
            if train_mask is not None:
                mask = train_mask if mask is None else mask * train_mask
            mask_t = (
                torch.as_tensor(mask, device=dev) if mask is not None
                else None
            )
            if sw_t is not None:
                # Newton sums weigh each row by mask * sample_weight
                mask_t = sw_t if mask_t is None else mask_t * sw_t
            grad, hess = self._gradients_t(Ft)   # [n, K] device fp64
            round_trees = []
            for k in range(K):
                ds.y_f = grad[:, k].to(torch.float32).contiguous()
                seed = int(rng.randint(1 << 31))
                tree = builder.build([seed], sample_weight=mask)[0]
                vrow = _leaf_value_rows(tree, X, Xdev, dev)
                self._newton_leaves_t(tree, vrow, grad[:, k], hess[:, k],
                                      mask_t, K)
                val_col = torch.as_tensor(
                    tree.value[:, 0], dtype=torch.float64, device=dev)
                Ft[:, k] += self.learning_rate * val_col.index_select(
                    0, vrow)
                round_trees.append(tree)
            stages.append(round_trees)
            if val_t is not None:
                loss = self._loss_t(val_t, Ft, val_w)
                if loss < best_loss - self.tol:
                    best_loss = loss
                    stall = 0
                else:
                    stall += 1
                    if stall >= self.n_iter_no_change:
                        break

        self.stages_ = stages
        self.n_features_in_ = X.shape[1]
        self.n_estimators_ = len(stages)
        # training labels / device tensors don't belong in the pickle
        for a in ("_enc", "_yv", "_enc_t", "_yv_t"):
            if hasattr(self, a):
                delattr(self, a)
        _strip(self)
        return self

    def _newton_leaves_t(self, tree, vrow, g, h, mask_t, K):
        """Refit leaf payloads with the one-step Newton update over the
        (subsampled) rows: value = scale * Σg / Σh per leaf — computed
        on device with a deterministic sort + cumsum segment sum."""
        scale = self._newton_scale(K)
        if scale is None:  # squared loss: (weighted) mean residual is
            return         # already the Newton step
        if mask_t is not None:
            g = g * mask_t
            h = h * mask_t
        nl = len(tree.value)
        num = _seg_sum(vrow, g, nl)
        den = _seg_sum(vrow, h, nl)
        val = scale * num / den.clamp_min(1e-8)
        tree.value = val.to(torch.float32).cpu().numpy()[:, None]

    # ------------------------------------------------------------------ #
    def _raw_scores(self, X):
        import scipy.sparse as sp

        if not hasattr(self, "stages_"):
            from sklearn.exceptions import NotFittedError

            raise NotFittedError(
                f"This {type(self).__name__} instance is not fitted yet. "
                "Call 'fit' before using this estimator.")

        if sp.issparse(X):
            X = canonical_csr(X, self.n_features_in_)
        else:
            X = np.asarray(X, dtype=np.float32)
        K = len(self.stages_[0])
        out = np.tile(self._base_raw(), (X.shape[0], 1))
        for round_trees in self.stages_:
            for k, tree in enumerate(round_trees):
                out[:, k] += (
                    self.learning_rate * tree.value[_leaf_rows(tree, X), 0]
                )
        return out

    def _staged_raw(self, X):
        """Yield raw scores after each boosting round (sklearn's
        staged_* protocol; one traversal per stage, accumulated)."""
        import scipy.sparse as sp

        if sp.issparse(X):
            X = canonical_csr(X, self.n_features_in_)
        else:
            X = np.asarray(X, dtype=np.float32)
        out = np.tile(self._base_raw(), (X.shape[0], 1))
        for round_trees in self.stages_:
            for k, tree in enumerate(round_trees):
                out[:, k] += (
                    self.learning_rate * tree.value[_leaf_rows(tree, X), 0]
                )
            yield out.copy()

    @property
    def estimators_(self):
        """[n_stages, K] object array of HistTrees (sklearn-shaped)."""
        arr = np.empty((len(self.stages_), len(self.stages_[0])),
                       dtype=object)
        for i, ts in enumerate(self.stages_):
            for k, t in enumerate(ts):
                arr[i, k] = t
        return arr

    @property
    def feature_importances_(self):
        imp = np.zeros(self.n_features_in_)
        for ts in self.stages_:
            for t in ts:
                if t.feature_importances_ is not None:
                    imp += t.feature_importances_
        s = imp.sum()
        return imp / s if s > 0 else imp

    # device inference hook (DistPredictor): the lr-scaled stage trees
    # flatten onto the GPU-validated FlatForest traversal kernel, one
    # flat per raw-score column (same scheme as FlatGBT for sklearn GBTs)
    def _device_predict_fn(self, method, device):
        if method not in ("predict", "predict_proba"):
            return None
        if method == "predict_proba" and not self._is_classifier:
            return None
        from .forest import FlatForest

        K = len(self.stages_[0])
        flats = []
        for k in range(K):
            trees = []
            for ts in self.stages_:
                t = ts[k]
                trees.append(HistTree(
                    t.feature, t.threshold, t.left, t.right,
                    t.value * self.learning_rate, None,
                    t.n_features_in_, t.feature_importances_,
                    getattr(t, "missing_left", None)))
            flats.append(FlatForest(trees, device))
        base = self._base_raw()

        def raw(X):
            cols = [
                f.predict_value(X)[:, 0] * f.n_trees for f in flats
            ]  # undo the kernel's mean -> sum
            return np.column_stack(cols) + base[None, :]

        def fn(X):
            r = raw(X)
            if method == "predict":
                if not self._is_classifier:
                    return r[:, 0]
                if r.shape[1] == 1:
                    return self.classes_[(r[:, 0] > 0).astype(np.int64)]
                return self.classes_[r.argmax(axis=1)]
            if r.shape[1] == 1:
                p = 1.0 / (1.0 + np.exp(-r[:, 0]))
                return np.column_stack([1.0 - p, p])
            e = np.exp(r - r.max(axis=1, keepdims=True))
            return e / e.sum(axis=1, keepdims=True)

        return fn


def _strip(est):
    if getattr(est, "sc", None) is not None:
        est.sc = None


class HistGradientBoostingRegressor(RegressorMixin, _BaseHistGB):
    """Least-squares gradient boosting on binned HistTrees."""

    def _init_raw(self, y, n, sw=None):
        self._yv = np.asarray(y, dtype=np.float64)
        self.init_raw_ = float(
            self._yv.mean() if sw is None
            else np.average(self._yv, weights=sw))
        return np.full((n, 1), self.init_raw_), 1

    def _to_device_targets(self, dev):
        self._yv_t = torch.as_tensor(self._yv, dtype=torch.float64,
                                     device=dev)

    def _loss_t(self, idx, Ft, w=None):
        d = self._yv_t.index_select(0, idx) - Ft.index_select(0, idx)[:, 0]
        return _wmean(d * d, w)

    def _base_raw(self):
        return np.array([self.init_raw_])

    def _gradients_t(self, Ft):
        g = (self._yv_t - Ft[:, 0]).unsqueeze(1)
        return g, torch.ones_like(g)

    def _newton_scale(self, K):
        return None  # leaf mean of residuals IS the Newton step

    def predict(self, X):
        return self._raw_scores(X)[:, 0]

    def staged_predict(self, X):
        for r in self._staged_raw(X):
            yield r[:, 0]


class HistGradientBoostingClassifier(ClassifierMixin, _BaseHistGB):
    """Binomial / multinomial deviance gradient boosting on binned
    HistTrees (leaf values via sklearn's one-step Newton update)."""

    _is_classifier = True

    def __init__(self, n_estimators=100, learning_rate=0.1, max_depth=3,
                 subsample=1.0, min_samples_split=2, min_samples_leaf=1,
                 max_features=None, n_iter_no_change=None,
                 validation_fraction=0.1, tol=1e-4, random_state=None,
                 max_iter=None, sc=None, class_weight=None,
                 allow_nan=False):
        super().__init__(
            n_estimators=n_estimators, learning_rate=learning_rate,
            max_depth=max_depth, subsample=subsample,
            min_samples_split=min_samples_split,
            min_samples_leaf=min_samples_leaf, max_features=max_features,
            n_iter_no_change=n_iter_no_change,
            validation_fraction=validation_fraction, tol=tol,
            random_state=random_state, max_iter=max_iter, sc=sc,
            allow_nan=allow_nan)
        self.class_weight = class_weight

    def _row_weights(self, y, sample_weight, n):
        sw = super()._row_weights(y, sample_weight, n)
        cw = getattr(self, "class_weight", None)
        if cw is None:
            return sw
        from sklearn.utils.class_weight import compute_sample_weight

        cwv = np.asarray(compute_sample_weight(cw, np.asarray(y)),
                         dtype=np.float64)
        return super()._row_weights(
            y, cwv if sw is None else sw * cwv, n)

    def _init_raw(self, y, n, sw=None):
        self.classes_, enc = np.unique(np.asarray(y), return_inverse=True)
        self._enc = enc
        k = len(self.classes_)
        if k < 2:
            raise ValueError("need at least 2 classes")
        eps = 1e-12
        if k == 2:
            p = np.clip(
                enc.mean() if sw is None else np.average(enc, weights=sw),
                eps, 1 - eps)
            self.init_raw_ = np.array([np.log(p / (1 - p))])
            return np.tile(self.init_raw_, (n, 1)), 1
        if sw is not None:
            cnt = np.bincount(enc, weights=sw, minlength=k)
            pri = np.clip(cnt / cnt.sum(), eps, None)
            self.init_raw_ = np.log(pri)
            return np.tile(self.init_raw_, (n, 1)), k
        pri = np.clip(np.bincount(enc, minlength=k) / n, eps, None)
        self.init_raw_ = np.log(pri)
        return np.tile(self.init_raw_, (n, 1)), k

    def _base_raw(self):
        return self.init_raw_

    def _to_device_targets(self, dev):
        self._enc_t = torch.as_tensor(self._enc, dtype=torch.int64,
                                      device=dev)

    def _gradients_t(self, Ft):
        if Ft.shape[1] == 1:
            p = torch.sigmoid(Ft[:, 0])
            g = (self._enc_t.to(torch.float64) - p).unsqueeze(1)
            h = (p * (1.0 - p)).unsqueeze(1)
            return g, h
        P = torch.softmax(Ft, dim=1)
        Y = torch.zeros_like(P)
        Y[torch.arange(len(self._enc_t), device=Ft.device),
          self._enc_t] = 1.0
        return Y - P, P * (1.0 - P)

    def _newton_scale(self, K):
        return 1.0 if K == 1 else (K - 1.0) / K

    def _loss_t(self, idx, Ft, w=None):
        # (weighted) mean deviance (neg log-likelihood) on the validation
        # slice
        z = Ft.index_select(0, idx)
        t = self._enc_t.index_select(0, idx)
        if Ft.shape[1] == 1:
            z0 = z[:, 0]
            return _wmean(
                torch.nn.functional.softplus(z0)
                - t.to(torch.float64) * z0, w)
        lse = torch.logsumexp(z, dim=1)
        return _wmean(lse - z.gather(1, t.unsqueeze(1))[:, 0], w)

    def decision_function(self, X):
        r = self._raw_scores(X)
        return r[:, 0] if r.shape[1] == 1 else r

    def predict_proba(self, X):
        return self._proba_from_raw(self._raw_scores(X))

    def predict_log_proba(self, X):
        return np.log(np.clip(self.predict_proba(X), 1e-300, None))

    def predict(self, X):
        r = self._raw_scores(X)
        if r.shape[1] == 1:
            return self.classes_[(r[:, 0] > 0).astype(np.int64)]
        return self.classes_[r.argmax(axis=1)]

    def _proba_from_raw(self, r):
        if r.shape[1] == 1:
            p = 1.0 / (1.0 + np.exp(-r[:, 0]))
            return np.column_stack([1.0 - p, p])
        e = np.exp(r - r.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    def staged_predict_proba(self, X):
        for r in self._staged_raw(X):
            yield self._proba_from_raw(r)

    def staged_predict(self, X):
        for r in self._staged_raw(X):
            if r.shape[1] == 1:
                yield self.classes_[(r[:, 0] > 0).astype(np.int64)]
            else:
                yield self.classes_[r.argmax(axis=1)]

    def staged_decision_function(self, X):
        for r in self._staged_raw(X):
            yield r[:, 0] if r.shape[1] == 1 else r


# honest-name aliases: the parameter surface IS sklearn's
# GradientBoosting* API (see _BaseHistGB docstring)
GradientBoostingClassifier = HistGradientBoostingClassifier
GradientBoostingRegressor = HistGradientBoostingRegressor
