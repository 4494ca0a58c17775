"""
Batched histogram decision-tree / forest builder (MI355X device path).

Replaces the per-tree sklearn Cython builder the reference fans out
(reference worker ``_build_trees``, skdist/distribute/ensemble.py:68-109;
inventory SURVEY.md §2.4 row 2) with a level-synchronous GPU builder:

  * X is quantile-binned ONCE into uint8 codes resident in HBM
    (row-major ``[n, fp]``, feature stride padded to a multiple of 4 so
    the histogram kernel reads 4 codes per uchar4 load);
  * a batch of TB trees grows together, breadth-first: one fused
    LDS-staged histogram kernel per level covers every (tree, node)
    frontier entry, a split kernel scans all (feature, bin) candidates
    with exact ``max_features`` subsampling (hash-ranked m-of-f) and
    ExtraTrees random-threshold mode, and a stable two-phase partition
    reorders each node's sample segment in place;
  * finished trees land on the host as plain numpy arrays (``HistTree``)
    that pickle and predict with no GPU/scheduler handles, per sk-dist's
    contract (reference search.py:568-570).

The same level loop runs two engines: the HIP kernels
(skdist_amd/ops/csrc/tree_kernels.hip — the production path, mandatory on
GPU) and a pure-torch eager mirror (CPU tests + the numerics reference the
kernels are asserted against; identical trees for classification, where
histogram sums are exact integer-valued f32).

Algorithmic notes / divergences from sklearn's exact splitter (documented,
deliberate):
  * split thresholds come from <=256 quantile bins (LightGBM/XGBoost-hist
    style), not exact midpoints;
  * ``min_samples_split`` / ``min_samples_leaf`` count bootstrap-weighted
    samples (integer multiplicities; equal to row counts when
    ``bootstrap=False``);
  * ``max_leaf_nodes`` / ``min_weight_fraction_leaf`` / ``class_weight``
    are not supported by the device path — callers fall back to the CPU
    per-tree path for those.
"""

import numpy as np
import torch

CRIT_GINI, CRIT_ENTROPY, CRIT_MSE = 0, 1, 2
_CRITERIA = {
    "gini": CRIT_GINI,
    "entropy": CRIT_ENTROPY,
    "log_loss": CRIT_ENTROPY,
    "squared_error": CRIT_MSE,
    "mse": CRIT_MSE,
}

# widest class-count vector the tree kernels take (tree_kernels.hip WIDE_S,
# predict_kernels.hip MAXVS_WIDE); up to NARROW_STATS the thread-per-feature
# / thread-per-row kernels run, above it the wave-per-feature / wave-per-row
# ones
MAX_DEVICE_CLASSES = 256
NARROW_STATS = 32
_U32 = np.uint32


def _wang_hash(s):
    """numpy uint32 mirror of the kernel's wang_hash (tree_kernels.hip)."""
    s = np.asarray(s, dtype=_U32)
    with np.errstate(over="ignore"):
        s = (s ^ _U32(61)) ^ (s >> _U32(16))
        s = s * _U32(9)
        s = s ^ (s >> _U32(4))
        s = s * _U32(0x27D4EB2D)
        s = s ^ (s >> _U32(15))
    return s


def _feat_hashes(seed, f):
    j = np.arange(f, dtype=np.int64)
    with np.errstate(over="ignore"):
        x = (_U32(seed) ^ (j * 2654435761 % (1 << 32)).astype(_U32))
    return _wang_hash(x)


def resolve_max_features(max_features, f):
    if max_features in (None, "auto", 1.0):
        return f
    if max_features == "sqrt":
        return max(1, int(np.sqrt(f)))
    if max_features == "log2":
        return max(1, int(np.log2(f)))
    if isinstance(max_features, float):
        return max(1, min(f, int(max_features * f)))
    return max(1, min(f, int(max_features)))


# --------------------------------------------------------------------- #
# fitted tree container (host-only, pickle-safe)
# --------------------------------------------------------------------- #

class HistTree:
    """One fitted histogram tree: flat numpy arrays, sklearn-like API.

    ``feature[i] == -1`` marks a leaf; its ``left[i]`` indexes ``value``
    (leaf payload: class distribution [k] or mean [1]).  Internal nodes
    send ``x[feature] <= threshold`` left.  ``missing_left`` (uint8
    ``[node_count]`` or None) marks the nodes that send a NaN left as well;
    without it a NaN goes right everywhere (``NaN <= t`` is false).
    """

    def __init__(self, feature, threshold, left, right, value, classes,
                 n_features, importances, missing_left=None):
        self.feature = feature
        self.threshold = threshold
        self.left = left
        self.right = right
        self.value = value
        self.classes_ = classes
        self.n_features_in_ = n_features
        self.feature_importances_ = importances
        self.missing_left = missing_left

    @property
    def node_count(self):
        return len(self.feature)

    def apply(self, X):
        """Leaf NODE index per row (vectorized host traversal).

        A scipy-sparse X is read cell by cell through CSR paired
        indexing (absent cell = 0.0); it is never densified."""
        import scipy.sparse as sp

        sparse = sp.issparse(X)
        if sparse:
            X = X.tocsr()
        else:
            X = np.asarray(X, dtype=np.float32)
        node = np.zeros(X.shape[0], dtype=np.int64)
        active = self.feature[node] >= 0
        while active.any():
            idx = np.flatnonzero(active)
            nd = node[idx]
            f = self.feature[nd]
            if sparse:
                xv = np.asarray(X[idx, f]).ravel().astype(np.float32)
            else:
                xv = X[idx, f]
            go_left = xv <= self.threshold[nd]
            # getattr: trees pickled before missing_left existed
            ml = getattr(self, "missing_left", None)
            if ml is not None:
                go_left |= np.isnan(xv) & (ml[nd] != 0)
            node[idx] = np.where(go_left, self.left[nd], self.right[nd])
            active[idx] = self.feature[node[idx]] >= 0
        return node

    def _leaf_values(self, X):
        leaves = self.apply(X)
        return self.value[self.left[leaves]]

    def predict_proba(self, X):
        return self._leaf_values(X)

    def predict(self, X):
        v = self._leaf_values(X)
        if self.classes_ is not None:
            return self.classes_[v.argmax(axis=1)]
        return v[:, 0]


# --------------------------------------------------------------------- #
# binned dataset (built once per forest fit, shared by every tree)
# --------------------------------------------------------------------- #

def canonical_csr(X, n_features=None):
    """Canonical CSR COPY of a scipy-sparse X for the sparse tree kernels
    (k_bin_csr, k_forest_predict_csr / k_forest_apply_csr): float32 data,
    duplicates summed, indices sorted, int32 column indices, int64 indptr.
    The caller's matrix is never mutated.  Raises before any launch on a
    malformed ``indptr``, a column index outside ``[0, f)`` or a width
    other than ``n_features``."""
    import scipy.sparse as sp

    n, f = X.shape
    if n_features is not None and f != n_features:
        raise ValueError(
            f"X has {f} features, but the model was fitted with "
            f"{n_features}")
    if f >= 2 ** 31:
        raise ValueError("sparse X wider than 2^31-1 columns")
    A = X.tocsr() if not sp.isspmatrix_csr(X) else X
    # duplicates are summed in X's own dtype and cast afterwards, the
    # order toarray() followed by a float32 cast uses
    data = np.array(A.data, copy=True)
    indices = np.array(A.indices, dtype=np.int64, copy=True)
    indptr = np.array(A.indptr, dtype=np.int64, copy=True)
    if (len(indptr) != n + 1 or indptr[0] != 0
            or indptr[-1] != len(indices) or len(indices) != len(data)
            or (n and np.any(np.diff(indptr) < 0))):
        raise ValueError("sparse X has an inconsistent indptr")
    if len(indices) and (indices.min() < 0 or indices.max() >= f):
        raise ValueError(
            f"sparse X holds a column index outside [0, {f})")
    C = sp.csr_matrix((data, indices.astype(np.int32), indptr),
                      shape=(n, f))
    C.sum_duplicates()
    C.sort_indices()
    C.indices = np.ascontiguousarray(C.indices, dtype=np.int32)
    C.indptr = np.ascontiguousarray(C.indptr, dtype=np.int64)
    C.data = np.ascontiguousarray(C.data, dtype=np.float32)
    return C


def _sparse_quantile_edges(C, nbins, device):
    """``torch.quantile(C.toarray(), qs, dim=0).t()`` without the dense
    matrix: [f, nbins-1] float32, bit-identical to the dense result.

    The order statistics of a virtual dense column are its sorted
    negatives, then (rows - nnz_col) zeros, then its sorted positives.
    torch.quantile reads ranks floor/ceil(q·(rows-1)) and joins them with
    ``lerp(lo, hi, q·(rows-1) - floor)``; the same float32 rank
    arithmetic runs here on the same device, the two order statistics are
    gathered from the per-column sorted nonzeros, and ``torch.lerp``
    joins them."""
    ns, f = C.shape
    qs = torch.linspace(0, 1, nbins + 1, device=device)[1:-1]
    ranks = qs * (ns - 1)
    r_lo = ranks.floor().to(torch.int64)
    w = ranks - r_lo
    r_hi = ranks.ceil().to(torch.int64).cpu().numpy()
    r_lo = r_lo.cpu().numpy()

    # stored nonzeros, sorted by (column, value)
    nz = C.data != 0
    cols = C.indices[nz].astype(np.int64)
    vals = C.data[nz]
    order = np.lexsort((vals, cols))
    cols = cols[order]
    vals = vals[order]
    colptr = np.zeros(f + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=f), out=colptr[1:])
    n_neg = np.bincount(cols[vals < 0], minlength=f).astype(np.int64)
    n_zero = ns - (colptr[1:] - colptr[:-1])    # implicit + stored zeros
    # one trailing pad so masked-out gathers stay in range
    vals = np.concatenate([vals, np.zeros(1, dtype=np.float32)])

    def order_stat(r, j0, j1):
        # r: [nq] ranks; columns j0:j1 → [j1-j0, nq] float32
        neg = n_neg[j0:j1, None]
        zero = n_zero[j0:j1, None]
        base = colptr[j0:j1, None]
        rr = r[None, :]
        in_neg = rr < neg
        in_pos = rr >= neg + zero
        pos = np.where(in_neg, base + rr, base + rr - zero)
        pos = np.where(in_neg | in_pos, pos, len(vals) - 1)
        return vals[pos]

    edges = torch.empty(f, nbins - 1, dtype=torch.float32, device=device)
    step = max(1, (1 << 24) // max(nbins - 1, 1))
    for j0 in range(0, f, step):
        j1 = min(f, j0 + step)
        lo = torch.as_tensor(order_stat(r_lo, j0, j1), device=device)
        hi = torch.as_tensor(order_stat(r_hi, j0, j1), device=device)
        edges[j0:j1] = torch.lerp(lo, hi, w.unsqueeze(0))
    return edges


def _csr_row_chunks(indptr, max_rows, max_nnz):
    """Row ranges [lo, hi) holding at most ``max_rows`` rows and, unless
    a single row is larger, at most ``max_nnz`` stored entries."""
    n = len(indptr) - 1
    lo = 0
    while lo < n:
        hi = int(np.searchsorted(indptr, indptr[lo] + max_nnz,
                                 side="right")) - 1
        hi = min(max(hi, lo + 1), lo + max_rows, n)
        yield lo, hi
        lo = hi


def _bin_csr_eager(indptr, indices, data, edges, zc, n):
    """Torch mirror of k_bin_csr (CPU tier / SKDIST_AMD_ALLOW_EAGER):
    every row starts as the zero-code pattern, then each stored entry is
    overwritten with the number of its feature's edges strictly below
    its value."""
    codes = zc.unsqueeze(0).repeat(n, 1).contiguous()
    nnz = len(data)
    if nnz == 0:
        return codes
    rows = torch.repeat_interleave(
        torch.arange(n, device=data.device), indptr[1:] - indptr[:-1])
    cols = indices.to(torch.int64)
    step = max(1, (1 << 24) // max(edges.shape[1], 1))
    for k0 in range(0, nnz, step):
        sl = slice(k0, k0 + step)
        c = (edges[cols[sl]] < data[sl].unsqueeze(1)).sum(dim=1)
        codes[rows[sl], cols[sl]] = c.to(torch.uint8)
    return codes


class BinnedDataset:
    """Quantile-binned (X, y) resident on one device.

    A scipy-sparse X is binned from its CSR arrays (k_bin_csr on GPU, a
    torch mirror on CPU) into the same ``edges`` and ``codes`` the dense
    constructor computes for ``X.toarray()``; only the uint8 code matrix
    is dense.

    ``row_weight`` (regression mode only) puts a real-valued f32 [n]
    weight plane ``row_w`` next to the codes.  The builder then keeps four
    statistics per histogram cell, (W, Wy, Wyy, C): weight sums drive
    impurity, gain and leaf values while the row count C keeps
    ``min_samples_*`` counts.  Without it nothing changes.

    ``allow_missing`` lets a dense X hold NaN (never ±inf).  If it holds
    any, the top code ``missing_bin = nbins - 1`` is reserved for them and
    the real values share ``nbins - 1`` bins whose last edge is ``+inf``;
    if it holds none, edges and codes are the ones of ``allow_missing=
    False`` and ``missing_bin`` is None.  A sparse X with a stored NaN
    still raises."""

    def __init__(self, X, y, device, is_cls, classes=None, nbins=256,
                 max_bin_sample=200_000, seed=0, row_weight=None,
                 allow_missing=False):
        import scipy.sparse as sp

        self.device = torch.device(device)
        self.allow_missing = bool(allow_missing)
        self.missing_bin = None
        if sp.issparse(X):
            self._init_codes_csr(X, nbins, max_bin_sample, seed)
        else:
            self._init_codes_dense(X, nbins, max_bin_sample, seed)
        self._init_targets(y, is_cls, classes)
        self.row_w = None
        if row_weight is not None:
            self.set_row_weight(row_weight)

    def set_row_weight(self, row_weight):
        """Attach the f32 row-weight plane (before a ForestBuilder is
        constructed on this dataset: the builder sizes its LDS feature
        groups from ``S``)."""
        if self.is_cls:
            raise ValueError(
                "row_weight is supported for regression targets only "
                "(classification forests use the uint8 weight plane)")
        rw = np.ascontiguousarray(row_weight, dtype=np.float32)
        if rw.shape != (self.n,):
            raise ValueError(
                f"row_weight must have shape ({self.n},), got {rw.shape}")
        if not np.isfinite(rw).all() or (rw < 0).any():
            raise ValueError("row_weight must be finite and non-negative")
        self.row_w = torch.as_tensor(rw, device=self.device)
        self.S = 4  # (W, Wy, Wyy, C)

    def _init_codes_csr(self, X, nbins, max_bin_sample, seed):
        import os

        from ._sgd import check_finite

        self.n, self.f = X.shape
        self.nbins = nbins
        self.fp = (self.f + 3) // 4 * 4
        gb = self.n * self.fp / 1e9
        limit = float(os.environ.get("SKDIST_AMD_DENSIFY_GB", "64"))
        if gb > limit:
            raise ValueError(
                f"the uint8 code matrix of sparse X ({self.n} x {self.fp}) "
                f"would take {gb:.1f} GB (> {limit:.0f} GB; set "
                "SKDIST_AMD_DENSIFY_GB to raise the limit)")
        C = canonical_csr(X)
        if self.allow_missing and np.isnan(C.data).any():
            raise ValueError(
                "Input X contains NaN: a sparse (CSR) X with a stored NaN "
                "cannot be fitted, missing values are binned for dense X "
                "only (pass a dense array, or impute the stored NaN)")
        check_finite(torch.from_numpy(C.data), "X")
        dev = self.device

        if self.n > max_bin_sample:
            g = torch.Generator(device="cpu")
            g.manual_seed(seed)
            sub = torch.randperm(self.n, generator=g)[:max_bin_sample]
            Cs = C[sub.numpy()]
        else:
            Cs = C
        self.edges = _sparse_quantile_edges(Cs, nbins, dev)
        del Cs

        # a cell with no stored entry holds 0.0: its code is the number
        # of edges strictly below zero; pad columns stay 0
        zc = torch.zeros(self.fp, dtype=torch.uint8, device=dev)
        zc[: self.f] = (self.edges < 0).sum(dim=1).to(torch.uint8)
        indptr = torch.as_tensor(C.indptr, device=dev)
        indices = torch.as_tensor(C.indices, device=dev)
        data = torch.as_tensor(C.data, device=dev)
        use_hip = dev.type == "cuda"
        if use_hip and _allow_eager():
            from ..ops import hip_available

            use_hip = hip_available()
        if use_hip:
            from ..ops import require_hip

            self.codes = torch.empty(self.n, self.fp, dtype=torch.uint8,
                                     device=dev)
            require_hip().bin_csr(indptr, indices, data, self.edges, zc,
                                  self.codes, self.f)
        else:
            self.codes = _bin_csr_eager(indptr, indices, data, self.edges,
                                        zc, self.n)

    def _init_codes_dense(self, X, nbins, max_bin_sample, seed):
        X = np.ascontiguousarray(X, dtype=np.float32)
        self.n, self.f = X.shape
        self.nbins = nbins
        Xt = torch.as_tensor(X, device=self.device)
        from ._sgd import check_finite

        nan = None
        if self.allow_missing:
            nan = torch.isnan(Xt)
            if not bool(nan.any()):
                nan = None
        if nan is None:
            check_finite(Xt, "X")
        elif bool(torch.isinf(Xt).any()):
            raise ValueError(
                "Input X contains infinity; missing values are NaN only")

        # per-feature quantile edges from a (seeded) row subsample
        if self.n > max_bin_sample:
            g = torch.Generator(device="cpu")
            g.manual_seed(seed)
            sub = torch.randperm(self.n, generator=g)[:max_bin_sample]
            Xs = Xt[sub.to(self.device)]
        else:
            Xs = Xt
        if nan is None:
            qs = torch.linspace(0, 1, nbins + 1, device=self.device)[1:-1]
            edges = torch.quantile(Xs.to(torch.float32), qs, dim=0)
            self.edges = edges.t().contiguous()                  # [f, nb-1]
        else:
            # the top code is the missing bin: nbins-1 bins for the real
            # values, cut at the quantiles of each column's non-NaN values,
            # and a closing +inf edge so that no real value passes it.  An
            # all-NaN column (quantile = NaN) gets +inf everywhere.
            self.missing_bin = nbins - 1
            qs = torch.linspace(0, 1, nbins, device=self.device)[1:-1]
            edges = torch.nanquantile(Xs.to(torch.float32), qs, dim=0)
            edges = torch.where(torch.isnan(edges),
                                torch.full_like(edges, float("inf")), edges)
            self.edges = torch.cat(
                [edges.t(), torch.full((self.f, 1), float("inf"),
                                       device=self.device)],
                dim=1).contiguous()                              # [f, nb-1]
            # NaN cells are masked explicitly: bin a stand-in value, then
            # overwrite their codes below
            Xt = torch.where(nan, torch.zeros_like(Xt), Xt)

        # codes[n][fp]: count of edges < x  →  (code <= b) ⟺ (x <= edges[b])
        # row-major with the feature stride padded to a multiple of 4 so
        # the histogram kernel reads 4 feature codes per uchar4 load
        self.fp = (self.f + 3) // 4 * 4
        XT = Xt.t().contiguous()
        codes_fm = torch.searchsorted(self.edges, XT, right=False)
        self.codes = torch.zeros(self.n, self.fp, dtype=torch.uint8,
                                 device=self.device)
        self.codes[:, : self.f] = codes_fm.to(torch.uint8).t()
        if nan is not None:
            self.codes[:, : self.f][nan] = self.missing_bin
        self.codes = self.codes.contiguous()
        del XT, Xt, Xs, codes_fm

    def _init_targets(self, y, is_cls, classes):
        self.is_cls = is_cls
        if is_cls:
            y_np = np.asarray(y)
            if classes is None:
                classes, enc = np.unique(y_np, return_inverse=True)
            else:
                enc = np.searchsorted(classes, y_np)
            self.classes_ = np.asarray(classes)
            self.S = len(self.classes_)
            if self.S > MAX_DEVICE_CLASSES:
                raise ValueError(
                    f"device forest supports <= {MAX_DEVICE_CLASSES} "
                    f"classes, got {self.S}")
            self.y_int = torch.as_tensor(
                np.ascontiguousarray(enc, dtype=np.int32),
                device=self.device)
            self.y_f = None
        else:
            self.classes_ = None
            self.S = 3  # (w, wy, wyy)
            self.y_int = None
            self.y_f = torch.as_tensor(
                np.ascontiguousarray(y, dtype=np.float32),
                device=self.device)

    def edges_np(self):
        if not hasattr(self, "_edges_np"):
            self._edges_np = self.edges.cpu().numpy()
        return self._edges_np


# --------------------------------------------------------------------- #
# the level-synchronous builder
# --------------------------------------------------------------------- #


class _NodeStore:
    """Flat growing node table for one tree batch (host, numpy).

    Nodes of every tree in the batch share one store; per-tree node ids
    (``nid``) are assigned densely in creation order so ``assemble``
    reproduces exactly the per-tree layout the scalar builder used.
    All level bookkeeping is vectorized over this store — the builder's
    wall time was host-bound before (kernels ~125 ms vs ~1.2 s wall for
    a 32-tree batch), dominated by per-node Python loops.
    """

    def __init__(self, TB, s_out):
        self.s_out = s_out
        self.cap = 1024
        self.n = 0
        self.tree = np.empty(self.cap, dtype=np.int64)
        self.nid = np.empty(self.cap, dtype=np.int64)
        self.feature = np.empty(self.cap, dtype=np.int64)
        self.bin = np.empty(self.cap, dtype=np.int64)
        self.left = np.empty(self.cap, dtype=np.int64)
        self.right = np.empty(self.cap, dtype=np.int64)
        self.leafrow = np.empty(self.cap, dtype=np.int64)
        self.mleft = np.empty(self.cap, dtype=np.int64)
        self.tree_counts = np.zeros(TB, dtype=np.int64)
        self.leaf_blocks = []
        self.n_leaves = 0

    def _ensure(self, extra):
        need = self.n + extra
        if need <= self.cap:
            return
        while self.cap < need:
            self.cap *= 2
        for name in ("tree", "nid", "feature", "bin", "left", "right",
                     "leafrow", "mleft"):
            old = getattr(self, name)
            new = np.empty(self.cap, dtype=np.int64)
            new[: self.n] = old[: self.n]
            setattr(self, name, new)

    def append(self, tree, nid):
        m = len(tree)
        self._ensure(m)
        lo = self.n
        self.n += m
        sl = slice(lo, self.n)
        self.tree[sl] = tree
        self.nid[sl] = nid
        self.feature[sl] = -1
        self.bin[sl] = -1
        self.left[sl] = -1
        self.right[sl] = -1
        self.leafrow[sl] = -1
        self.mleft[sl] = 0
        return np.arange(lo, self.n)

    def make_leaves(self, rows, values):
        """Mark store rows as leaves with the given [m, s_out] payloads."""
        m = len(rows)
        if m == 0:
            return
        self.feature[rows] = -1
        self.leafrow[rows] = self.n_leaves + np.arange(m)
        self.n_leaves += m
        self.leaf_blocks.append(
            np.ascontiguousarray(values, dtype=np.float32))

    def assemble(self, ds, importances):
        """Per-tree HistTree list (nid-ordered arrays, leaf re-indexed)."""
        n = self.n
        vals = (
            np.concatenate(self.leaf_blocks, axis=0)
            if self.leaf_blocks
            else np.zeros((0, self.s_out), dtype=np.float32)
        )
        edges = ds.edges_np()
        order = np.lexsort((self.nid[:n], self.tree[:n]))
        tree_sorted = self.tree[:n][order]
        bounds = np.searchsorted(
            tree_sorted, np.arange(len(self.tree_counts) + 1))
        out = []
        for t in range(len(self.tree_counts)):
            rows = order[bounds[t]: bounds[t + 1]]
            feature = self.feature[rows].astype(np.int32)
            bins = self.bin[rows]
            thr = np.zeros(len(rows), dtype=np.float32)
            internal = feature >= 0
            if internal.any():
                thr[internal] = edges[feature[internal], bins[internal]]
            left = self.left[rows].astype(np.int32)
            right = self.right[rows].astype(np.int32)
            leaf = ~internal
            lrows = self.leafrow[rows][leaf]
            value = (
                vals[lrows] if len(lrows)
                else np.zeros((1, self.s_out), dtype=np.float32)
            )
            left[leaf] = np.arange(leaf.sum())
            imp = importances[t]
            ssum = imp.sum()
            # a dataset binned with allow_missing yields trees that carry
            # the per-node direction of a missing value (0 at leaves)
            mleft = (self.mleft[rows].astype(np.uint8)
                     if ds.allow_missing else None)
            out.append(HistTree(
                feature, thr, left, right, value, ds.classes_, ds.f,
                (imp / ssum if ssum > 0 else imp).astype(np.float64),
                mleft))
        return out


def hist_groups(f, nbins, S, budget):
    """(fg, cg) of the class-grouped histogram kernel: features and
    classes per LDS tile with ``fg * nbins * cg * 4 <= budget`` bytes.

    The classes are cut first, and only as far as it takes to keep four
    features (one uchar4 code load) in a tile where the data has four:
    every class group scans the node's rows again, while a narrow feature
    group loses the vector load.  What is left of the budget then widens
    the feature group, in steps of four."""
    cells = budget // (nbins * 4)              # (feature, class) pairs
    cg = min(S, max(1, cells // min(f, 4)))
    fg = max(1, min(f, cells // cg))
    return (fg // 4 * 4 if fg >= 4 else fg), cg


class ForestBuilder:
    """Grows a batch of trees level-by-level against one BinnedDataset.

    engine: 'hip' (mandatory on GPU) or 'eager' (CPU / numerics mirror).
    """

    CHUNK_ROWS = 32768
    HIST_BUDGET_BYTES = 1 << 30
    LDS_BUDGET_BYTES = 64 * 1024

    def __init__(self, ds, criterion, max_depth=None, min_samples_split=2,
                 min_samples_leaf=1, min_impurity_decrease=0.0,
                 max_features=None, extra_mode=False, bootstrap=True,
                 tree_batch=32, engine=None, subtract=True):
        self.ds = ds
        self.crit = _CRITERIA[criterion]
        self.max_depth = 10**9 if max_depth is None else int(max_depth)
        self.mss = float(min_samples_split)
        self.msl = float(min_samples_leaf)
        self.mid = float(min_impurity_decrease)
        self.m_features = resolve_max_features(max_features, ds.f)
        self.extra_mode = bool(extra_mode)
        # the dataset reserved its top code for NaN: the split scan weighs
        # both directions of that bin and the partition follows the winner
        self.missing = ds.missing_bin is not None
        if self.missing and self.extra_mode:
            raise ValueError(
                "extra_mode (random thresholds) is not supported on a "
                "dataset with a missing bin")
        self.bootstrap = bool(bootstrap)
        self.tree_batch = int(tree_batch)
        self.subtract = bool(subtract)
        if engine is None:
            engine = "hip" if ds.device.type == "cuda" else "eager"
        if engine == "hip":
            from ..ops import require_hip

            self._ext = require_hip()
        elif ds.device.type == "cuda" and not _allow_eager():
            raise RuntimeError(
                "eager forest engine on a GPU device requires "
                "SKDIST_AMD_ALLOW_EAGER=1 (the HIP kernels are the "
                "production path)")
        self.engine = engine
        # index of the row-count stat (datasets with a row-weight plane)
        self.cnt_stat = 3 if ds.row_w is not None else -1
        # scale of the uint8 weight plane and the min_samples thresholds
        # in that scale (make_weights / _build_batch set them per batch)
        self._w_scale = 1.0
        self._mss_eff = self.mss
        self._msl_eff = self.msl
        # features per LDS group for the hist kernel; above NARROW_STATS
        # classes also the classes per group (hist_groups), None = one
        # tile over all S stats
        self.cg = None
        if ds.is_cls and ds.S > NARROW_STATS:
            self.fg, self.cg = hist_groups(ds.f, ds.nbins, ds.S,
                                           self.LDS_BUDGET_BYTES)
        else:
            per_feat = ds.nbins * ds.S * 4
            fg = max(1, min(ds.f, self.LDS_BUDGET_BYTES // per_feat))
            self.fg = fg // 4 * 4 if fg >= 4 else fg

    # -------------------------------------------------------------- #
    def build(self, seeds, sample_weight=None):
        """Fit one tree per seed; returns list of HistTree."""
        trees = []
        for s0 in range(0, len(seeds), self.tree_batch):
            trees.extend(
                self._build_batch(seeds[s0:s0 + self.tree_batch],
                                  sample_weight))
        return trees

    def make_weights(self, seeds, sample_weight=None):
        """Bootstrap multiplicities [TB, n] uint8 (torch RNG per seed)."""
        ds = self.ds
        TB = len(seeds)
        if not self.bootstrap:
            w = torch.ones(TB, ds.n, dtype=torch.uint8, device=ds.device)
        else:
            w = torch.empty(TB, ds.n, dtype=torch.uint8, device=ds.device)
            for t, seed in enumerate(seeds):
                g = torch.Generator(device=ds.device)
                g.manual_seed(int(seed))
                idx = torch.randint(0, ds.n, (ds.n,), generator=g,
                                    device=ds.device)
                w[t] = torch.bincount(idx, minlength=ds.n).clamp_(
                    max=255).to(torch.uint8)
        self._w_scale = 1.0
        if sample_weight is not None:
            sw = torch.as_tensor(
                np.ascontiguousarray(sample_weight, dtype=np.float32),
                device=ds.device)
            wf = w.to(torch.float32) * sw.unsqueeze(0)
            mx = float(wf.max())
            if mx <= 0:
                raise ValueError("sample_weight leaves no weighted rows")
            if mx <= 255 and bool((wf == wf.round()).all()):
                # integer-valued weights (bootstrap counts, 0/1 masks,
                # integer class weights): exact, as in round 1
                w = wf.round_().to(torch.uint8)
            else:
                # real-valued weights quantize into the uint8 plane at
                # 192 levels (~0.5% relative granularity).  A uniform
                # weight scale is mathematically free for splits and
                # leaf values; the min_samples/min-leaf thresholds are
                # scaled to match (_build_batch).
                self._w_scale = 192.0 / mx
                w = (wf * self._w_scale).round_().clamp_(0, 255).to(
                    torch.uint8)
        return w

    # -------------------------------------------------------------- #
    def _build_batch(self, seeds, sample_weight):
        ds = self.ds
        TB = len(seeds)
        f, nbins, S = ds.f, ds.nbins, ds.S
        s_out = S if ds.is_cls else 1

        weights = self.make_weights(seeds, sample_weight)
        # weighted-count thresholds live in the (possibly quantized)
        # weight-plane scale
        self._mss_eff = self.mss * self._w_scale
        self._msl_eff = self.msl * self._w_scale
        si_a, counts = self._initial_sample_idx(weights)
        si_b = torch.empty_like(si_a)

        st = _NodeStore(TB, s_out)
        importances = np.zeros((TB, f))
        root_w = np.ones(TB)

        fr_tree = np.arange(TB, dtype=np.int64)
        fr_grow = st.append(fr_tree, np.zeros(TB, dtype=np.int64))
        st.tree_counts[:] = 1
        fr_start = np.zeros(TB, dtype=np.int64)
        fr_count = counts.astype(np.int64)
        fr_parent = np.full(TB, -1, dtype=np.int64)
        fr_sib_start = np.zeros(TB, dtype=np.int64)
        fr_sib_count = np.zeros(TB, dtype=np.int64)
        fr_left = np.zeros(TB, dtype=np.int64)
        prev_hist = None
        depth = 0
        hist_nodes_cap = max(
            1, self.HIST_BUDGET_BYTES // (f * nbins * S * 4))

        while len(fr_tree) and depth <= self.max_depth:
            dec, prev_hist = self._level_decisions(
                seeds, fr_tree, st.nid[fr_grow], fr_start, fr_count,
                weights, si_a, hist_nodes_cap, prev_hist=prev_hist,
                fr_parent=fr_parent, fr_sib_start=fr_sib_start,
                fr_sib_count=fr_sib_count, fr_left=fr_left)
            (bfeat, bbin, bgain, bimp, bwl, pstats, lstats, bml) = dec

            wp = pstats.sum(axis=1) if ds.is_cls else pstats[:, 0]
            if not self.missing:
                # no missing bin in this dataset: a NaN met at predict time
                # follows the majority of the split (ties to the right)
                bml = (bwl + bwl > wp).astype(np.int64)
            counted = self.cnt_stat >= 0
            # min_samples_split compares row counts when the weights are
            # real numbers; the weight sums drive everything else
            cp = pstats[:, self.cnt_stat] if counted else wp
            if depth == 0:
                root_w[fr_tree] = (
                    np.where(wp > 0, wp, 1.0) if counted
                    else np.maximum(wp, 1.0))
            ok = (
                (bfeat >= 0)
                & (depth < self.max_depth)
                & (cp >= self._mss_eff)
                & (bgain > 0)
                & ((wp / root_w[fr_tree]) * bgain >= self.mid - 1e-12)
            )

            part_idx = np.flatnonzero(ok)
            leaf_idx = np.flatnonzero(~ok)
            st.make_leaves(fr_grow[leaf_idx],
                           self._leaf_values_vec(pstats[leaf_idx]))

            if not len(part_idx):
                fr_tree = np.empty(0, dtype=np.int64)
                depth += 1
                continue

            nl = self._partition(
                fr_tree[part_idx], fr_start[part_idx],
                fr_count[part_idx], bfeat[part_idx], bbin[part_idx],
                bml[part_idx], si_a, si_b)
            si_a, si_b = si_b, si_a

            t_p = fr_tree[part_idx]
            # per-tree dense child-id assignment in part order
            order = np.argsort(t_p, kind="stable")
            ts = t_p[order]
            starts = np.flatnonzero(np.r_[True, ts[1:] != ts[:-1]])
            seg_len = np.diff(np.r_[starts, len(ts)])
            ranks = np.empty(len(t_p), dtype=np.int64)
            ranks[order] = np.arange(len(ts)) - np.repeat(starts, seg_len)
            lid = st.tree_counts[t_p] + 2 * ranks
            rid = lid + 1
            st.tree_counts += 2 * np.bincount(t_p, minlength=TB)

            gl = st.append(t_p, lid)
            gr = st.append(t_p, rid)
            pg = fr_grow[part_idx]
            st.feature[pg] = bfeat[part_idx]
            st.bin[pg] = bbin[part_idx]
            st.mleft[pg] = bml[part_idx]
            st.left[pg] = lid
            st.right[pg] = rid
            np.add.at(
                importances, (t_p, bfeat[part_idx]),
                wp[part_idx] * bgain[part_idx] / root_w[t_p])

            ls = lstats[part_idx]
            rs = pstats[part_idx] - ls
            if ds.is_cls:
                wl = ls.sum(axis=1)
                wr = rs.sum(axis=1)
            else:
                wl = ls[:, 0]
                wr = rs[:, 0]
            cl = ls[:, self.cnt_stat] if counted else wl
            cr = rs[:, self.cnt_stat] if counted else wr
            nrows_l = nl.astype(np.int64)
            nrows_r = fr_count[part_idx] - nrows_l
            st_l = fr_start[part_idx]
            st_r = st_l + nrows_l

            can_grow = depth + 1 < self.max_depth
            grow_l = (can_grow & (cl >= self._mss_eff) & (nrows_l > 1)
                      & (self._impurity_vec(ls, wl) > 1e-12))
            grow_r = (can_grow & (cr >= self._mss_eff) & (nrows_r > 1)
                      & (self._impurity_vec(rs, wr) > 1e-12))
            st.make_leaves(gl[~grow_l], self._leaf_values_vec(ls[~grow_l]))
            st.make_leaves(gr[~grow_r], self._leaf_values_vec(rs[~grow_r]))

            fr_tree = np.concatenate([t_p[grow_l], t_p[grow_r]])
            fr_grow = np.concatenate([gl[grow_l], gr[grow_r]])
            fr_start = np.concatenate([st_l[grow_l], st_r[grow_r]])
            fr_count = np.concatenate([nrows_l[grow_l], nrows_r[grow_r]])
            fr_parent = np.concatenate(
                [part_idx[grow_l], part_idx[grow_r]])
            fr_sib_start = np.concatenate([st_r[grow_l], st_l[grow_r]])
            fr_sib_count = np.concatenate(
                [nrows_r[grow_l], nrows_l[grow_r]])
            fr_left = np.concatenate([
                np.ones(int(grow_l.sum()), dtype=np.int64),
                np.zeros(int(grow_r.sum()), dtype=np.int64),
            ])
            depth += 1

        return st.assemble(ds, importances)

    def _leaf_values_vec(self, stats):
        """[m, S] stats -> [m, s_out] leaf payloads (vectorized)."""
        stats = np.atleast_2d(stats)
        if self.ds.is_cls:
            tot = np.clip(stats.sum(axis=1, keepdims=True), 1e-30, None)
            return stats / tot
        return (stats[:, 1] / np.clip(stats[:, 0], 1e-30, None))[:, None]

    def _impurity_vec(self, stats, w):
        """Vectorized impurity over [m, S] stats rows."""
        w = np.clip(np.asarray(w, dtype=np.float64), 1e-30, None)
        if self.ds.is_cls:
            if self.crit == CRIT_GINI:
                return 1.0 - (stats ** 2).sum(axis=1) / (w * w)
            p = stats / w[:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                e = np.where(p > 0, p * np.log2(p, where=p > 0), 0.0)
            return -e.sum(axis=1)
        mean = stats[:, 1] / w
        return np.maximum(stats[:, 2] / w - mean * mean, 0.0)

    def _initial_sample_idx(self, weights):
        """Pack rows with weight > 0 to the front of each tree's row
        (one vectorized nonzero over the whole batch)."""
        ds = self.ds
        TB = weights.shape[0]
        si = torch.zeros(TB, ds.n, dtype=torch.int32, device=ds.device)
        nz = torch.nonzero(weights > 0)          # [(t, i)] sorted
        t_idx = nz[:, 0]
        counts_t = torch.bincount(t_idx, minlength=TB)
        offs = torch.cumsum(counts_t, 0) - counts_t
        pos = torch.arange(len(nz), device=ds.device) - offs[t_idx]
        si[t_idx, pos] = nz[:, 1].to(torch.int32)
        return si, counts_t.cpu().numpy().astype(np.int64)

    def _impurity_np(self, stats, w):
        if w <= 0:
            return 0.0
        if self.ds.is_cls:
            if self.crit == CRIT_GINI:
                return 1.0 - float((stats ** 2).sum()) / (w * w)
            p = stats[stats > 0] / w
            return float(-(p * np.log2(p)).sum())
        mean = stats[1] / w
        return max(float(stats[2] / w - mean * mean), 0.0)

    # -------------------------------------------------------------- #
    # level primitives: hist + split (sliced to the hist budget)
    # -------------------------------------------------------------- #
    def _level_decisions(self, seeds, fr_tree, fr_node, fr_start, fr_count,
                         weights, si, cap, prev_hist=None, fr_parent=None,
                         fr_sib_start=None, fr_sib_count=None,
                         fr_left=None):
        """Per-frontier-node split decisions.

        Returns (8-tuple of decision arrays, hist_or_None).  When the
        previous level's histogram tensor is available (``prev_hist``,
        slot = previous frontier index) the HIP path uses the LightGBM
        subtraction trick: only the smaller child of each split parent is
        histogrammed; its sibling's histogram is ``parent − child``
        (exact for classification — integer-valued f32).  The returned
        hist tensor feeds the NEXT level's subtraction.
        """
        NF = len(fr_tree)
        if (
            self.engine == "hip"
            and self.subtract
            and prev_hist is not None
            and fr_parent is not None
            and len(fr_parent) == NF
            and NF > 0
            and (fr_parent >= 0).all()
        ):
            out = self._subtract_level(
                seeds, fr_tree, fr_node, fr_start, fr_count, weights, si,
                cap, prev_hist, fr_parent, fr_sib_start, fr_sib_count,
                fr_left)
            if out is not None:
                return out
        if self.engine == "hip" and 0 < NF <= cap:
            dec, hist = self._hist_and_split(
                seeds, fr_tree, fr_node, fr_start, fr_count, weights, si,
                return_hist=True)
            return dec, hist
        outs = []
        for s0 in range(0, NF, cap):
            sl = slice(s0, min(NF, s0 + cap))
            outs.append(self._hist_and_split(
                seeds, fr_tree[sl], fr_node[sl], fr_start[sl],
                fr_count[sl], weights, si))
        return (
            tuple(np.concatenate(parts) for parts in zip(*outs)),
            None,
        )

    def _subtract_level(self, seeds, fr_tree, fr_node, fr_start, fr_count,
                        weights, si, cap, prev_hist, fr_parent,
                        fr_sib_start, fr_sib_count, fr_left):
        """One level with sibling-subtraction; None -> caller falls back."""
        ds = self.ds
        NF = len(fr_tree)
        f, nbins, S = ds.f, ds.nbins, ds.S
        dev = ds.device
        direct = (fr_count < fr_sib_count) | (
            (fr_count == fr_sib_count) & (fr_left == 1))
        # sibling hist source per derived node: the co-frontier sibling
        # (same parent slot) when present, else an extra slot for the
        # leaf sibling's rows
        sib_src = np.full(NF, -1, dtype=np.int64)
        order = np.argsort(fr_parent, kind="stable")
        ps = fr_parent[order]
        starts = np.flatnonzero(np.r_[True, ps[1:] != ps[:-1]])
        seg = np.diff(np.r_[starts, NF])
        pair_at = starts[seg == 2]
        a = order[pair_at]
        b = order[pair_at + 1]
        da = direct[a]
        sib_src[np.where(da, b, a)] = np.where(da, a, b)
        singles = order[starts[seg == 1]]
        need = singles[~direct[singles]]  # derive from a leaf sibling
        sib_src[need] = NF + np.arange(len(need))
        extras = need
        total = NF + len(extras)
        if total > cap:
            return None

        hist = torch.zeros(total, f, nbins, S, dtype=torch.float32,
                           device=dev)
        d_slots = np.flatnonzero(~direct)
        dir_slots = np.flatnonzero(direct)
        h_slot = np.concatenate([dir_slots, NF + np.arange(len(extras))])
        h_tree = np.concatenate([fr_tree[dir_slots], fr_tree[extras]])
        h_start = np.concatenate(
            [fr_start[dir_slots], fr_sib_start[extras]])
        h_count = np.concatenate(
            [fr_count[dir_slots], fr_sib_count[extras]])
        self._run_hist_kernel(hist, h_slot, h_tree, h_start, h_count,
                              weights, si)
        if len(d_slots):
            d_idx = torch.as_tensor(d_slots, device=dev)
            p_idx = torch.as_tensor(
                fr_parent[d_slots].astype(np.int64), device=dev)
            s_idx = torch.as_tensor(sib_src[d_slots], device=dev)
            hist[d_idx] = prev_hist.index_select(0, p_idx) - \
                hist.index_select(0, s_idx)
        dec = self._run_split_kernel(
            hist, self._node_seeds(seeds, fr_tree, fr_node), NF)
        return dec, hist

    def _node_seeds(self, seeds, fr_tree, fr_node):
        s = np.asarray([seeds[t] for t in fr_tree], dtype=np.int64)
        with np.errstate(over="ignore"):
            x = (s * 2654435761 + fr_node * 97531) % (1 << 32)
        return _wang_hash(x.astype(_U32)).astype(np.uint32)

    def _chunk_table(self, fr_tree, fr_start, fr_count, slot_ids):
        """[n_chunks, 4] = {slot, tree_slot, row_start, row_count}
        (vectorized; a node always yields >= 1 chunk)."""
        CH = self.CHUNK_ROWS
        fr_count = np.asarray(fr_count, dtype=np.int64)
        nch = np.maximum(1, (fr_count + CH - 1) // CH)
        rep = np.repeat(np.arange(len(fr_tree)), nch)
        firsts = np.cumsum(nch) - nch
        within = np.arange(len(rep)) - np.repeat(firsts, nch)
        off = within * CH
        out = np.empty((len(rep), 4), dtype=np.int32)
        out[:, 0] = np.asarray(slot_ids)[rep]
        out[:, 1] = np.asarray(fr_tree)[rep]
        out[:, 2] = np.asarray(fr_start)[rep] + off
        out[:, 3] = np.minimum(CH, fr_count[rep] - off)
        return out

    def _run_hist_kernel(self, hist, slot, tree, start, count, weights,
                         si):
        """Histogram the given segments (parallel arrays) into ``hist``
        (zero-initialized [n_slots, f, nbins, S])."""
        ds = self.ds
        dev = ds.device
        if not len(slot):
            return
        chunks_np = self._chunk_table(tree, start, count, slot)
        chunks = torch.as_tensor(chunks_np, device=dev)
        absent = torch.empty(0, device=dev)   # the binding's "not given"
        self._ext.tree_hist(
            ds.codes, ds.y_int if ds.is_cls else absent,
            absent if ds.is_cls else ds.y_f,
            absent if ds.row_w is None else ds.row_w,
            weights, si, chunks, hist, ds.n, ds.f, ds.nbins, self.fg,
            *(() if self.cg is None else (self.cg,)))

    def _run_split_kernel(self, hist, node_seed, NF):
        ds = self.ds
        dev = ds.device
        S = ds.S
        seed_t = torch.as_tensor(node_seed.astype(np.int32), device=dev)
        # outputs packed into two buffers -> two D2H transfers per level
        # (the third int plane, the missing direction, is written in
        # missing mode only)
        ibuf = torch.empty(3 * NF, dtype=torch.int32, device=dev)
        fbuf = torch.empty((3 + 2 * S) * NF, dtype=torch.float32,
                           device=dev)
        out_feat = ibuf[:NF]
        out_bin = ibuf[NF: 2 * NF]
        out_mleft = ibuf[2 * NF:]
        out_wl = fbuf[:NF]
        out_gain = fbuf[NF: 2 * NF]
        out_imp = fbuf[2 * NF: 3 * NF]
        out_stats = fbuf[3 * NF: (3 + S) * NF].view(NF, S)
        out_lstats = fbuf[(3 + S) * NF:].view(NF, S)
        self._ext.tree_split(
            hist, seed_t, ds.f, ds.nbins, S, int(ds.is_cls), self.crit,
            self.m_features, int(self.extra_mode), self._msl_eff,
            out_feat, out_bin, out_wl, out_gain, out_imp, out_stats,
            out_lstats, self.cnt_stat,
            *((1, out_mleft) if self.missing else ()))
        ih = ibuf.cpu().numpy()
        fh = fbuf.cpu().numpy().astype(np.float64)
        return (ih[:NF].astype(np.int64),
                ih[NF: 2 * NF].astype(np.int64),
                fh[NF: 2 * NF],
                fh[2 * NF: 3 * NF],
                fh[:NF],
                fh[3 * NF: (3 + S) * NF].reshape(NF, S),
                fh[(3 + S) * NF:].reshape(NF, S),
                ih[2 * NF:].astype(np.int64) if self.missing
                else np.zeros(NF, dtype=np.int64))

    def _hist_and_split(self, seeds, fr_tree, fr_node, fr_start, fr_count,
                        weights, si, return_hist=False):
        ds = self.ds
        NF = len(fr_tree)
        f, nbins, S = ds.f, ds.nbins, ds.S
        dev = ds.device
        node_seed = self._node_seeds(seeds, fr_tree, fr_node)

        if self.engine == "hip":
            hist = torch.zeros(NF, f, nbins, S, dtype=torch.float32,
                               device=dev)
            self._run_hist_kernel(hist, np.arange(NF), fr_tree, fr_start,
                                  fr_count, weights, si)
            dec = self._run_split_kernel(hist, node_seed, NF)
            if return_hist:
                return dec, hist
            return dec

        return self._hist_and_split_eager(
            fr_tree, fr_start, fr_count, weights, si, node_seed)

    # ---------------- eager (torch) mirror of K1+K2 ---------------- #
    def _hist_and_split_eager(self, fr_tree, fr_start, fr_count, weights,
                              si, node_seed):
        ds = self.ds
        f, nbins, S = ds.f, ds.nbins, ds.S
        NF = len(fr_tree)
        bfeat = np.full(NF, -1, dtype=np.int64)
        bbin = np.full(NF, -1, dtype=np.int64)
        bgain = np.zeros(NF)
        bimp = np.zeros(NF)
        bwl = np.zeros(NF)
        pstats = np.zeros((NF, S))
        lstats = np.zeros((NF, S))
        bml = np.zeros(NF, dtype=np.int64)
        for k in range(NF):
            t = int(fr_tree[k])
            rows = si[t, int(fr_start[k]): int(fr_start[k] + fr_count[k])]
            rows = rows.to(torch.int64)
            w = weights[t, rows].to(torch.float32)
            codes = ds.codes[rows][:, : f].t().to(torch.int64)  # [f, m]
            hist = torch.zeros(f, nbins, S, device=ds.device)
            if ds.is_cls:
                stat = ds.y_int[rows].to(torch.int64)          # [m]
                flat = (torch.arange(f, device=ds.device)[:, None]
                        * nbins + codes) * S + stat[None, :]
                hist.view(-1).scatter_add_(
                    0, flat.reshape(-1),
                    w.unsqueeze(0).expand(f, -1).reshape(-1))
            else:
                yv = ds.y_f[rows]
                base = (torch.arange(f, device=ds.device)[:, None]
                        * nbins + codes) * S
                hv = hist.view(-1)
                if self.cnt_stat >= 0:
                    # (W, Wy, Wyy, C): C counts the uint8 multiplicity m,
                    # the weight is m * row_w (k_tree_hist_w)
                    hv.scatter_add_(0, (base + self.cnt_stat).reshape(-1),
                                    w.unsqueeze(0).expand(f, -1).reshape(-1))
                    w = w * ds.row_w[rows]
                hv.scatter_add_(0, base.reshape(-1),
                                w.unsqueeze(0).expand(f, -1).reshape(-1))
                hv.scatter_add_(0, (base + 1).reshape(-1),
                                (w * yv).unsqueeze(0).expand(
                                    f, -1).reshape(-1))
                hv.scatter_add_(0, (base + 2).reshape(-1),
                                (w * yv * yv).unsqueeze(0).expand(
                                    f, -1).reshape(-1))
            res = self._split_eager(hist, int(node_seed[k]))
            (bfeat[k], bbin[k], bgain[k], bimp[k], bwl[k], pstats[k],
             lstats[k], bml[k]) = res
        return bfeat, bbin, bgain, bimp, bwl, pstats, lstats, bml

    def _split_eager(self, hist, seed):
        ds = self.ds
        f, nbins, S = ds.f, ds.nbins, ds.S
        h = hist.cpu().numpy().astype(np.float64)      # [f, nbins, S]
        parent = h[0].sum(axis=0)                      # [S]
        wp = parent.sum() if ds.is_cls else parent[0]
        imp_p = self._impurity_np(parent, wp)

        sel = np.ones(f, dtype=bool)
        if self.m_features < f:
            hv = _feat_hashes(seed, f)
            thresh = np.sort(hv)[self.m_features - 1]
            sel = hv <= thresh

        cum = h.cumsum(axis=1)[:, :-1, :]              # left stats [f,nb-1,S]

        def scan(cum):
            """(wl, gain, valid) of the cuts whose left stats are ``cum``,
            each [f, nbins-1]."""
            if ds.is_cls:
                wl = cum.sum(axis=2)
            else:
                wl = cum[:, :, 0]
            wr = wp - wl
            if ds.is_cls:
                if self.crit == CRIT_GINI:
                    q = (cum ** 2).sum(axis=2)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        imp_l = 1.0 - q / (wl * wl)
                    rq = ((parent[None, None, :] - cum) ** 2).sum(axis=2)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        imp_r = 1.0 - rq / (wr * wr)
                else:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        pl = cum / wl[:, :, None]
                        pr = (parent[None, None, :] - cum) / wr[:, :, None]
                    imp_l = -np.nansum(
                        np.where(pl > 0, pl * np.log2(pl, where=pl > 0),
                                 0.0), axis=2)
                    imp_r = -np.nansum(
                        np.where(pr > 0, pr * np.log2(pr, where=pr > 0),
                                 0.0), axis=2)
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    ml = cum[:, :, 1] / wl
                    imp_l = np.maximum(cum[:, :, 2] / wl - ml * ml, 0.0)
                    mr = (parent[1] - cum[:, :, 1]) / wr
                    imp_r = np.maximum(
                        (parent[2] - cum[:, :, 2]) / wr - mr * mr, 0.0)
            with np.errstate(invalid="ignore"):
                gain = imp_p - (wl * imp_l + wr * imp_r) / max(wp, 1e-30)
            msl = self._msl_eff
            if self.cnt_stat >= 0:
                # k_tree_split_w: min-leaf on row counts, weight on both
                # sides
                cl = cum[:, :, self.cnt_stat]
                cr = parent[self.cnt_stat] - cl
                valid = ((cl >= msl) & (cr >= msl) & (wl > 0) & (wr > 0)
                         & sel[:, None])
            else:
                valid = (wl >= msl) & (wr >= msl) & sel[:, None]
            return wl, gain, valid

        wl, gain, valid = scan(cum)
        if self.extra_mode:
            extra_ok = np.zeros_like(valid)
            wbin = h.sum(axis=2) if ds.is_cls else h[:, :, 0]
            occupied = wbin > 0
            for j in np.flatnonzero(sel):
                occ = np.flatnonzero(occupied[j])
                if len(occ) < 2:
                    continue
                lo, hi = int(occ[0]), int(occ[-1])
                if hi <= lo:
                    continue
                with np.errstate(over="ignore"):
                    r = int(_wang_hash(
                        _U32(seed) ^ _U32(0x9E3779B9)
                        ^ _U32((j * 40503) % (1 << 32))))
                rb = lo + (r % (hi - lo))
                extra_ok[j, rb] = True
            valid &= extra_ok
        gain = np.where(valid & np.isfinite(gain), gain, -1.0)
        if not self.missing:
            best = float(gain.max(initial=-1.0))
            if best <= 0.0:
                return (-1, -1, best, imp_p, 0.0, parent, np.zeros(S), 0)
            cands = np.argwhere(gain >= best - 1e-12)
            jf, jb = cands[np.lexsort((cands[:, 1], cands[:, 0]))][0]
            return (int(jf), int(jb), float(gain[jf, jb]), imp_p,
                    float(wl[jf, jb]), parent, cum[jf, jb].copy(), 0)

        # missing mode (k_tree_split_m / _wm): the top bin holds the
        # missing rows.  R candidates are the prefixes above (the missing
        # bin stays right); L candidates add its stats to the left side,
        # for the features whose missing bin holds weight in this node.
        miss = h[:, nbins - 1, :]                      # [f, S]
        wm = miss.sum(axis=1) if ds.is_cls else miss[:, 0]
        cum_l = cum + miss[:, None, :]
        wl_l, gain_l, valid_l = scan(cum_l)
        valid_l &= (wm > 0)[:, None]
        gain_l = np.where(valid_l & np.isfinite(gain_l), gain_l, -1.0)
        both = np.stack([gain, gain_l], axis=2)        # [f, nb-1, (R, L)]
        best = float(both.max(initial=-1.0))
        if best <= 0.0:
            return (-1, -1, best, imp_p, 0.0, parent, np.zeros(S), 0)
        # equal gains: lower feature, then lower bin, then R before L
        cands = np.argwhere(both >= best - 1e-12)
        jf, jb, jd = cands[np.lexsort(
            (cands[:, 2], cands[:, 1], cands[:, 0]))][0]
        if jd == 1:
            return (int(jf), int(jb), float(gain_l[jf, jb]), imp_p,
                    float(wl_l[jf, jb]), parent, cum_l[jf, jb].copy(), 1)
        w_left = float(wl[jf, jb])
        # nothing missing under this feature here: majority side
        mleft = int(not wm[jf] > 0 and w_left + w_left > wp)
        return (int(jf), int(jb), float(gain[jf, jb]), imp_p, w_left,
                parent, cum[jf, jb].copy(), mleft)

    # -------------------------------------------------------------- #
    # partition (K3 count + host scan + K4 scatter, or eager)
    # -------------------------------------------------------------- #
    def _partition(self, p_tree, p_start, p_count, p_feat, p_bin, p_mleft,
                   si_in, si_out):
        """Stable-partition each listed node's segment; returns per-node
        left-row counts.  On a dataset with a missing bin a row goes left
        iff ``code <= bin or (mleft and code == missing_bin)``."""
        ds = self.ds
        dev = ds.device
        NP = len(p_tree)
        if self.engine != "hip":
            nl = np.empty(NP, dtype=np.int64)
            for k in range(NP):
                t = int(p_tree[k])
                st, cnt = int(p_start[k]), int(p_count[k])
                rows = si_in[t, st:st + cnt].to(torch.int64)
                code = ds.codes[rows, int(p_feat[k])]
                go_left = code <= int(p_bin[k])
                if self.missing and int(p_mleft[k]):
                    go_left |= code == ds.missing_bin
                lrows = rows[go_left]
                rrows = rows[~go_left]
                nl[k] = len(lrows)
                si_out[t, st:st + len(lrows)] = lrows.to(torch.int32)
                si_out[t, st + len(lrows):st + cnt] = rrows.to(torch.int32)
            return nl

        chunks_np = self._chunk_table(p_tree, p_start, p_count,
                                      np.arange(NP))
        chunks = torch.as_tensor(chunks_np, device=dev)
        feat_t = torch.as_tensor(p_feat.astype(np.int32), device=dev)
        bin_t = torch.as_tensor(p_bin.astype(np.int32), device=dev)
        nch = len(chunks_np)
        counts = torch.empty(nch, dtype=torch.int32, device=dev)
        # trailing arguments of the two partition entries in missing mode
        miss_args = ()
        if self.missing:
            miss_args = (
                torch.as_tensor(p_mleft.astype(np.int32), device=dev),
                ds.missing_bin)
        self._ext.part_count(ds.codes, si_in, chunks, feat_t, bin_t,
                             ds.n, counts, *miss_args)
        counts_np = counts.cpu().numpy().astype(np.int64)

        # per-node prefix over its chunks → absolute left/right bases
        # (vectorized: the chunk table is ordered per node, so group
        # prefixes are global cumsums minus each group's start value)
        slot = chunks_np[:, 0].astype(np.int64)
        rows_np = chunks_np[:, 3].astype(np.int64)
        nl = np.bincount(slot, weights=counts_np,
                         minlength=NP).astype(np.int64)
        starts = np.flatnonzero(np.r_[True, slot[1:] != slot[:-1]])
        seg_len = np.diff(np.r_[starts, nch])
        ex_l = np.cumsum(counts_np) - counts_np
        run_l = ex_l - np.repeat(ex_l[starts], seg_len)
        rminusc = rows_np - counts_np
        ex_r = np.cumsum(rminusc) - rminusc
        run_r = ex_r - np.repeat(ex_r[starts], seg_len)
        lbase = p_start[slot] + run_l
        rbase = p_start[slot] + nl[slot] + run_r
        lb = torch.as_tensor(lbase.astype(np.int32), device=dev)
        rb = torch.as_tensor(rbase.astype(np.int32), device=dev)
        self._ext.part_scatter(ds.codes, si_in, chunks, feat_t, bin_t,
                               lb, rb, ds.n, si_out, *miss_args)
        return nl


def _allow_eager():
    import os

    return os.environ.get("SKDIST_AMD_ALLOW_EAGER") == "1"


# --------------------------------------------------------------------- #
# flattened device forest (batched inference kernel)
# --------------------------------------------------------------------- #

def forest_walk(ext, op, xdev, *args, mleft=None):
    """The one entry to the inference kernels: ``op`` is "predict" or
    "apply", ``xdev`` a device f32 ``[rows, f]`` block or a device CSR
    ``(indptr, indices, data)``; ``args`` go on to the binding.  ``mleft``
    (device uint8 per node, or None) selects the kernels that send a NaN
    left where the flag is set; without it the call is the flag-free one."""
    if mleft is not None:
        args = args + (mleft,)
    if isinstance(xdev, tuple):
        getattr(ext, f"forest_{op}_csr")(*xdev, *args)
    else:
        getattr(ext, f"forest_{op}")(xdev, *args)


def _missing_left_of(tree):
    """A tree's per-node missing direction or None (trees pickled before
    the attribute existed have none)."""
    return getattr(tree, "missing_left", None)


class FlatForest:
    """A list of HistTrees flattened into device arrays for the batched
    inference kernels (k_forest_predict / k_forest_apply,
    predict_kernels.hip) — the device analog of the reference's
    executor-side ``model.predict`` inside a pandas UDF
    (skdist/distribute/predict.py:160-178).

    Ephemeral: built next to a prediction call, never pickled inside a
    fitted estimator.
    """

    def __init__(self, trees, device):
        from ..ops import require_hip

        self._ext = require_hip()
        self.device = torch.device(device)
        feats, thrs, lefts, rights, roots, vals = [], [], [], [], [], []
        mlefts = []
        off = voff = 0
        for t in trees:
            internal = t.feature >= 0
            left = t.left.astype(np.int64)
            right = t.right.astype(np.int64)
            left = np.where(internal, left + off, left + voff)
            right = np.where(internal, right + off, 0)
            feats.append(t.feature)
            thrs.append(t.threshold)
            lefts.append(left)
            rights.append(right)
            vals.append(t.value)
            ml = _missing_left_of(t)
            mlefts.append(np.zeros(t.node_count, dtype=np.uint8)
                          if ml is None else np.asarray(ml, dtype=np.uint8))
            roots.append(off)
            off += t.node_count
            voff += len(t.value)
        dev = self.device
        as_t = lambda a, dt: torch.as_tensor(
            np.ascontiguousarray(np.concatenate(a)), dtype=dt, device=dev)
        self.feat = as_t(feats, torch.int32)
        self.thr = as_t(thrs, torch.float32)
        self.left = as_t(lefts, torch.int32)
        self.right = as_t(rights, torch.int32)
        # missing-direction flags ride along only when some tree has them;
        # a forest without any takes the flag-free kernels
        self.mleft = (
            as_t(mlefts, torch.uint8)
            if any(_missing_left_of(t) is not None for t in trees) else None)
        self.values = torch.as_tensor(
            np.ascontiguousarray(np.concatenate(vals, axis=0)),
            dtype=torch.float32, device=dev)
        self.roots = torch.as_tensor(
            np.asarray(roots, dtype=np.int32), device=dev)
        self.n_trees = len(trees)
        self.vs = self.values.shape[1]
        self.classes_ = trees[0].classes_
        self.n_features = trees[0].n_features_in_

    # stored entries uploaded per CSR chunk (12 bytes each on device)
    CSR_CHUNK_NNZ = 1 << 27

    def _chunks(self, X, chunk_rows):
        """Yield ``(rows, xdev)`` per chunk of X for ``forest_walk``: a
        device f32 block of an array, or of a scipy-sparse X (canonical
        copy, never densified) a device CSR triple with ``indptr`` rebased
        to 0, bounded by a row count and a stored-entry count."""
        import scipy.sparse as sp

        dev = self.device
        if not sp.issparse(X):
            X = np.ascontiguousarray(X, dtype=np.float32)
            for lo in range(0, len(X), chunk_rows):
                xb = torch.as_tensor(X[lo: lo + chunk_rows], device=dev)
                yield len(xb), xb
            return
        C = canonical_csr(X, self.n_features)
        # a sparse X without rows is one empty chunk -> [0, width] output
        for lo, hi in list(_csr_row_chunks(
                C.indptr, chunk_rows, self.CSR_CHUNK_NNZ)) or [(0, 0)]:
            a, b = int(C.indptr[lo]), int(C.indptr[hi])
            yield hi - lo, (
                torch.as_tensor(C.indptr[lo: hi + 1] - a, device=dev),
                torch.as_tensor(C.indices[a:b], device=dev),
                torch.as_tensor(C.data[a:b], device=dev),
            )

    def predict_value(self, X, chunk_rows=1 << 22):
        """Mean leaf payload over trees: [rows, vs] numpy."""
        outs = []
        for rows, xdev in self._chunks(X, chunk_rows):
            out = torch.empty(rows, self.vs, dtype=torch.float32,
                              device=self.device)
            forest_walk(self._ext, "predict", xdev, self.feat, self.thr,
                        self.left, self.right, self.roots, self.values, out,
                        mleft=self.mleft)
            outs.append(out.cpu().numpy())
        return np.concatenate(outs, axis=0)

    def predict_proba(self, X):
        return self.predict_value(X)

    def predict(self, X):
        v = self.predict_value(X)
        if self.classes_ is not None:
            return self.classes_[v.argmax(axis=1)]
        return v[:, 0]

    def apply(self, X, chunk_rows=1 << 21):
        """Leaf node id per (row, tree): [rows, n_trees] int32 — ids are
        tree-local (matching HistTree.apply) for embedding parity."""
        roots_np = self.roots.cpu().numpy().astype(np.int64)
        outs = []
        for rows, xdev in self._chunks(X, chunk_rows):
            out = torch.empty(rows, self.n_trees, dtype=torch.int32,
                              device=self.device)
            forest_walk(self._ext, "apply", xdev, self.feat, self.thr,
                        self.left, self.right, self.roots, out,
                        mleft=self.mleft)
            outs.append(out.cpu().numpy() - roots_np[None, :])
        return np.concatenate(outs, axis=0)


def _sklearn_tree_to_hist_tree(tree, kind):
    """Flatten one fitted sklearn tree (its ``tree_`` arrays) into the
    HistTree layout the device traversal kernel walks.

    kind: 'proba' (classifier: leaf = class distribution),
          'value' (regressor / boosting stage: leaf = raw value).
    """
    t = tree.tree_
    n = t.node_count
    feature = t.feature.astype(np.int32).copy()
    threshold = t.threshold.astype(np.float32)
    left = t.children_left.astype(np.int32).copy()
    right = t.children_right.astype(np.int32).copy()
    leaves = np.flatnonzero(feature < 0)
    feature[leaves] = -1
    v = t.value[leaves]                      # [n_leaves, n_out, k]
    if kind == "proba":
        v = v[:, 0, :]
        v = v / np.clip(v.sum(axis=1, keepdims=True), 1e-30, None)
    else:
        v = v.reshape(len(leaves), -1)[:, :1]
    left[leaves] = np.arange(len(leaves), dtype=np.int32)
    # sklearn >= 1.3 learns, per split, the side a NaN goes to
    mleft = getattr(t, "missing_go_to_left", None)
    if mleft is not None:
        mleft = np.ascontiguousarray(mleft, dtype=np.uint8)
    return HistTree(
        feature, threshold, left, right,
        np.ascontiguousarray(v, dtype=np.float32),
        getattr(tree, "classes_", None),
        t.n_features, None, mleft,
    )


class FlatGBT:
    """sklearn GradientBoosting{Classifier,Regressor} flattened for the
    device traversal kernel: raw score = prior + lr·Σ stage-tree values,
    then the sigmoid/softmax link — the GBT batch-inference path of
    BASELINE config 5 (reference analog: executor-side model.predict in
    the pandas UDF, predict.py:160-178)."""

    def __init__(self, model, device):
        from sklearn.ensemble import (
            GradientBoostingClassifier,
            GradientBoostingRegressor,
        )

        self.is_cls = isinstance(model, GradientBoostingClassifier)
        if not self.is_cls and not isinstance(
                model, GradientBoostingRegressor):
            raise TypeError(model)
        self.classes_ = getattr(model, "classes_", None)
        ests = model.estimators_            # [n_stages, k_trees]
        self.k_trees = ests.shape[1]
        lr = model.learning_rate
        flats = []
        for j in range(self.k_trees):
            trees = []
            for i in range(ests.shape[0]):
                ht = _sklearn_tree_to_hist_tree(ests[i, j], "value")
                ht.value = ht.value * lr
                trees.append(ht)
            flats.append(FlatForest(trees, device))
        self.flats = flats
        # prior (raw init) from the model's initial estimator via its
        # public decision path on a single dummy row is model-dependent;
        # use the training prior stored on the loss/init estimator
        init = model.init_
        probe = np.zeros((1, model.n_features_in_), dtype=np.float64)
        if hasattr(init, "predict_proba"):
            p = np.clip(init.predict_proba(probe)[0], 1e-12, 1 - 1e-12)
            if len(p) == 2:
                self.base = np.array([np.log(p[1] / p[0])])
            else:
                self.base = np.log(p)
        elif hasattr(init, "predict"):
            self.base = np.atleast_1d(
                np.asarray(init.predict(probe), dtype=np.float64).ravel())
        else:  # 'zero'
            self.base = np.zeros(max(self.k_trees, 1))

    def _raw(self, X):
        cols = [
            f.predict_value(X)[:, 0] * f.n_trees for f in self.flats
        ]  # undo the kernel's mean -> sum
        return np.column_stack(cols) + self.base[None, :]

    def predict_proba(self, X):
        raw = self._raw(X)
        if raw.shape[1] == 1:
            p1 = 1.0 / (1.0 + np.exp(-raw[:, 0]))
            return np.column_stack([1 - p1, p1])
        e = np.exp(raw - raw.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    def predict(self, X):
        if self.is_cls:
            raw = self._raw(X)
            if raw.shape[1] == 1:
                return self.classes_[(raw[:, 0] > 0).astype(np.int64)]
            return self.classes_[raw.argmax(axis=1)]
        return self._raw(X)[:, 0]


def flat_forest_for(model, device):
    """Device scorer for a fitted tree ensemble: HIP-fitted HistTree
    forests, host-fitted sklearn forests (DecisionTree estimators_), and
    sklearn GradientBoosting models all flatten onto the same traversal
    kernel; returns None for anything else (host path)."""
    try:
        from sklearn.ensemble import (
            GradientBoostingClassifier,
            GradientBoostingRegressor,
        )

        if isinstance(model, (GradientBoostingClassifier,
                              GradientBoostingRegressor)):
            return FlatGBT(model, device)
    except Exception:
        pass
    trees = getattr(model, "estimators_", None)
    if trees is None or len(trees) == 0 or getattr(trees, "ndim", 1) != 1:
        return None  # (a boosted model's [n_stages, K] array is not a
        # flat forest — those models expose _device_predict_fn instead)
    trees = list(trees)
    # the traversal kernels carry <= MAX_DEVICE_CLASSES payload values per
    # leaf (predict_kernels.hip MAXVS_WIDE); wider-class forests score on
    # the host path instead of erroring at launch.  So do the forests
    # above NARROW_STATS classes when the device is not a GPU.
    widest = (MAX_DEVICE_CLASSES if torch.device(device).type == "cuda"
              else NARROW_STATS)
    if all(isinstance(t, HistTree) for t in trees):
        if trees[0].value.shape[1] > widest:
            return None
        return FlatForest(trees, device)
    if all(hasattr(t, "tree_") for t in trees):
        is_cls = hasattr(trees[0], "predict_proba") and hasattr(
            model, "classes_")
        if is_cls and len(model.classes_) > widest:
            return None
        flat = FlatForest(
            [
                _sklearn_tree_to_hist_tree(
                    t, "proba" if is_cls else "value")
                for t in trees
            ],
            device,
        )
        flat.classes_ = getattr(model, "classes_", None)
        return flat
    return None
