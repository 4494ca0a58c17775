"""
HIP/CDNA4 kernel extension loader.

The extension (`_skdist_hip`) is built IN-TREE for gfx950 by
``__graft_entry__.build()`` / ``python setup.py build_ext --inplace`` and
ships with the repo snapshot.  Policy on a GPU box: the HIP kernels ARE the
compute path — if the extension is missing, ops raise instead of silently
falling back to eager torch (set SKDIST_AMD_ALLOW_EAGER=1 to waive, for
debugging only).
"""

import os

import torch

_ext = None
_ext_err = None


def _load():
    global _ext, _ext_err
    if _ext is not None or _ext_err is not None:
        return _ext
    try:
        from . import _skdist_hip  # built in-tree, travels with the repo

        _ext = _skdist_hip
    except ImportError as e:
        _ext_err = e
    return _ext


def hip_available():
    return torch.cuda.is_available() and _load() is not None


def require_hip():
    if not torch.cuda.is_available():
        raise RuntimeError("require_hip(): no HIP device visible")
    if _load() is None:
        raise RuntimeError(
            "skdist_amd HIP extension is not built — run "
            "`python -c 'import __graft_entry__; __graft_entry__.build()'` "
            f"(import error: {_ext_err})"
        )
    return _ext


GRAM_MAX_BYTES = 768  # csrc/hash_kernels.hip: GRAM_MAX
CHAR_WB_MAX_CHARS = 32  # csrc/hash_kernels.hip: WIN_CHARS


class HashGramOverflow(ValueError):
    """An n-gram did not fit the UTF-8 hashing kernel's buffer."""


def hash_vectorize(docs, n_features=2 ** 20, analyzer="word",
                   ngram_range=(1, 1), alternate_sign=True, binary=False,
                   norm="l2", lowercase=True, dtype="float64",
                   device="cuda"):
    """Device hashing vectorizer: tokenize + murmur3 + CSR, sklearn-exact
    for any Unicode text under the default ``word`` / ``char_wb``
    analyzers (kernels: csrc/hash_kernels.hip; reference analog: sklearn
    HashingVectorizer inside skdist/preprocessing.py:264-310).

    Documents are lowercased on the host (``str.lower()``, so the Unicode
    case mapping is Python's own), packed into ONE UTF-8 byte buffer and
    uploaded to HBM.  A pure-ASCII buffer goes to the byte-oriented
    ``k_hash_vectorize``; any other buffer goes to
    ``k_hash_vectorize_utf8``, which walks code points with Python's
    ``\\w`` / ``\\s`` classes (ops/unicode_tables.py).  The kernel emits
    (doc*F + feature, ±1) COO pairs; torch sorts + segment-sums them and
    the result returns as a scipy CSR (same dtype/norm contract as
    sklearn's transform).

    Raises ``UnicodeEncodeError`` for a document that cannot be encoded
    (lone surrogate) and ``HashGramOverflow`` (a ``ValueError``) when a
    non-ASCII buffer holds a word n-gram (n >= 2) longer than
    ``GRAM_MAX_BYTES`` bytes.  Known deviation: on a pure-ASCII buffer
    such an n-gram is skipped without an error (docs/PARITY.md).
    """
    import numpy as np
    import scipy.sparse as sp

    ext = require_hip()
    mode = {"word": 0, "char_wb": 1}[analyzer]
    min_n, max_n = ngram_range
    if len(docs) == 0:
        return sp.csr_matrix((0, n_features), dtype=dtype)
    enc = [
        (d.lower() if lowercase else d).encode("utf-8") for d in docs
    ]
    lens = np.fromiter((len(b) for b in enc), dtype=np.int64,
                       count=len(enc))
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    blob = np.frombuffer(b"".join(enc), dtype=np.uint8)
    n_docs = len(enc)
    dev = torch.device(device)
    bytes_t = torch.as_tensor(blob, device=dev)
    off_t = torch.as_tensor(off, device=dev)
    # routing: an all-ASCII buffer keeps the byte-oriented kernel.  One
    # reduction over the uploaded buffer: the same reduction in numpy
    # costs ~16 ms per 130 MB on the host, which showed in the ASCII
    # throughput (profiles/r03_hash_unicode.txt)
    utf8 = bool(len(blob)) and int(bytes_t.max().item()) >= 0x80
    if utf8:
        from .unicode_tables import device_tables

        word_tbl, ws_list = device_tables(bytes_t.device)
    orders = max_n - min_n + 1
    if mode == 0:
        cap = int(len(blob) // 3 + n_docs + 64) * orders
    else:
        cap = int(2 * len(blob) + 2 * n_docs + 64) * orders
    while True:
        keys = torch.empty(max(cap, 64), dtype=torch.int64, device=dev)
        vals = torch.empty(max(cap, 64), dtype=torch.float32, device=dev)
        # ctr[0]: pairs emitted; ctr[1]: overflow flag (UTF-8 kernel only)
        ctr = torch.zeros(2, dtype=torch.int64, device=dev)
        if utf8:
            ext.hash_vectorize_utf8(bytes_t, off_t, mode, min_n, max_n,
                                    n_features, int(alternate_sign),
                                    word_tbl, ws_list, keys, vals, ctr)
        else:
            ext.hash_vectorize(bytes_t, off_t, mode, min_n, max_n,
                               n_features, int(alternate_sign), keys,
                               vals, ctr)
        total, overflow = ctr.tolist()
        if overflow:
            raise HashGramOverflow(
                "hash_vectorize: an n-gram does not fit the kernel's "
                f"buffer (word n-grams with n >= 2: {GRAM_MAX_BYTES} "
                f"bytes; char_wb: {CHAR_WB_MAX_CHARS} characters); "
                "use sklearn's HashingVectorizer for these documents"
            )
        if total <= cap:
            break
        cap = total  # exact size known now; one retry
    keys = keys[:total]
    vals = vals[:total]
    if total:
        keys, order = torch.sort(keys)
        vals = vals[order]
        uniq, inverse = torch.unique_consecutive(keys,
                                                 return_inverse=True)
        sums = torch.zeros(len(uniq), dtype=torch.float32, device=dev)
        sums.scatter_add_(0, inverse, vals)
        rows = (uniq // n_features).cpu().numpy()
        cols = (uniq % n_features).cpu().numpy().astype(np.int64)
        data = sums.cpu().numpy().astype(dtype)
    else:
        rows = np.empty(0, dtype=np.int64)
        cols = np.empty(0, dtype=np.int64)
        data = np.empty(0, dtype=dtype)
    if binary:
        data = np.ones_like(data)
    indptr = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_docs), out=indptr[1:])
    out = sp.csr_matrix((data, cols, indptr),
                        shape=(n_docs, n_features))
    if norm is not None:
        from sklearn.preprocessing import normalize

        out = normalize(out, norm=norm, copy=False)
    return out


def _pad_cols(t, ncols_pad, fill):
    import torch as _t

    out = _t.full((ncols_pad,), fill, dtype=t.dtype, device=t.device)
    out[: t.shape[0]] = t
    return out.contiguous()


SOFTMAX_LOSS_ID = 3       # models/_sgd.py LOSS_SOFTMAX, csrc/common.h
SOFTMAX_MAX_CLASSES = 128  # one group must fit a 128-column kernel tile


def softmax_columns(n_models, gk):
    """Kernel column of every (model, class) of a multinomial solve, and
    the padded column count.

    k_fwd_gt_softmax reduces over the ``gk`` columns of a model inside
    one 128-column tile, so a group never straddles a tile: a tile holds
    ``gpt = 128 // gk`` groups in its first ``gpt * gk`` columns and the
    rest of the tile is dead (``128 % gk`` columns: none for gk = 64,
    2 for gk = 3, 63 for gk = 65).  Model j, class c lives at column
    ``(j // gpt) * 128 + (j % gpt) * gk + c``.
    """
    import numpy as np

    gpt = 128 // gk
    j = np.arange(n_models)
    base = (j // gpt) * 128 + (j % gpt) * gk
    cols = (base[:, None] + np.arange(gk)[None, :]).ravel()
    ncp = (n_models + gpt - 1) // gpt * 128
    return cols, ncp


def pack_bit_plane(a, perm, n_pad, ncols_pad, chunk=1 << 15):
    """Bit plane of a 0/1 matrix for k_fwd_gt_bits.

    ``a`` [n, ncols] uint8 on the device, original row order; ``perm`` [n]
    int64, the shuffled row order of ``Xs``.  Returns int32
    [n_pad, ncols_pad / 32]: bit ``c & 31`` of word ``[r, c >> 5]`` is
    ``a[perm[r], c]``; rows >= n and columns >= ncols are 0.  Packed
    ``chunk`` rows at a time, so the int32 scratch stays at
    ``chunk * ncols_pad * 4`` bytes.
    """
    n, ncols = a.shape
    assert ncols_pad % 32 == 0 and ncols <= ncols_pad and n <= n_pad
    dev = a.device
    out = torch.zeros(n_pad, ncols_pad // 32, dtype=torch.int32, device=dev)
    # bit 31 is the sign bit of an int32 word: it enters as -2^31
    weights = torch.tensor([1 << k for k in range(31)] + [-(1 << 31)],
                           dtype=torch.int32, device=dev)
    for lo in range(0, n, chunk):
        rows = a.index_select(0, perm[lo: lo + chunk])
        blk = torch.zeros(rows.shape[0], ncols_pad, dtype=torch.int32,
                          device=dev)
        blk[:, :ncols] = rows != 0
        out[lo: lo + rows.shape[0]] = (
            blk.view(rows.shape[0], ncols_pad // 32, 32) * weights
        ).sum(dim=2, dtype=torch.int32)
    return out


def hip_sgd_solve(ds, spec, loss_id, epochs, batch_size, seed, momentum,
                  lr_decay, splitk=8):
    """Full batched SGD solve on the HIP kernels (K1+K2+K3 per step).

    Walks the same per-epoch host-RNG permutations as the torch reference
    (minibatch = slab of the epoch-shuffled copy), so the two paths are
    comparable to bf16 tolerance.  Returns W [fa, ncols] fp32.

    ``spec.col_l1`` set (some column with l1 > 0) switches K3 to
    k_reduce_update_l1 through the ``*_l1`` entries; it costs two more
    [fa, ncols_pad] fp32 tables (the per-weight L1 credits).  Without it
    the calls below are the L2-only ones, unchanged.

    The softmax loss (``spec.group_k`` set) spreads the columns into the
    tile layout of ``softmax_columns`` -- dead columns are pad columns --
    and gathers W back, so the caller sees compact model-major columns
    like for every other loss.

    ``spec.targets`` set switches K1 to k_fwd_gt_bits through the ``*_bits``
    entries (L2-only and L1 alike): ``spec.targets`` and, if set,
    ``spec.train_mask`` are packed on the device into int32 bit planes,
    columns padded to ``ncols_pad``, rows gathered by the solve's
    permutation and zero-filled to ``n_pad``.  Each plane takes
    ``n_pad * ncols_pad / 8`` bytes.
    """
    import numpy as np

    ext = require_hip()
    device = ds.device
    n, fa = ds.Xaug.shape
    assert fa % 32 == 0
    ncols = spec.ncols
    ncp = (ncols + 127) // 128 * 128
    gk = getattr(spec, "group_k", None)
    if (int(loss_id) == SOFTMAX_LOSS_ID) != (gk is not None):
        raise ValueError(
            "the softmax loss and ColumnSpec.group_k go together")
    place = None    # kernel column of each spec column (softmax only)
    if gk is not None:
        if gk > SOFTMAX_MAX_CLASSES:
            raise ValueError(
                f"multi_class='multinomial' on the HIP path takes at most "
                f"{SOFTMAX_MAX_CLASSES} classes, got {gk}")
        cols_np, ncp = softmax_columns(ncols // gk, gk)
        place = torch.as_tensor(cols_np, dtype=torch.int64, device=device)
    gk_arg = int(gk) if gk is not None else 0

    def pad_cols(t, fill):
        if place is None:
            return _pad_cols(t, ncp, fill)
        out = torch.full((ncp,), fill, dtype=t.dtype, device=t.device)
        out[place] = t
        return out.contiguous()
    bs = min(batch_size, (n + 127) // 128 * 128)
    bs = max(128, bs - bs % 128)
    gts = (bs + 127) // 128 * 128

    W = torch.zeros(fa, ncp, dtype=torch.float32, device=device)
    V = (
        torch.zeros_like(W) if momentum > 0.0
        else torch.empty(0, device=device)
    )
    WbfT = torch.zeros(ncp, fa, dtype=torch.bfloat16, device=device)
    GT = torch.empty(ncp, gts, dtype=torch.bfloat16, device=device)
    partial = torch.empty(splitk, fa, ncp, dtype=torch.float32,
                          device=device)
    cls_p = pad_cols(spec.col_class, -99)
    cfold_p = pad_cols(spec.col_fold, -9)
    cls2_p = pad_cols(spec.col_class2, -1)
    lr_p = pad_cols(spec.col_lr, 0.0)
    l2_p = pad_cols(spec.col_l2, 0.0)
    if getattr(spec, "feat_mask", None) is not None:
        fmask = torch.ones(fa, ncp, dtype=torch.uint8, device=device)
        if place is None:
            fmask[:, :ncols] = spec.feat_mask
        else:
            fmask[:, place] = spec.feat_mask
        fmask = fmask.contiguous()
    else:
        fmask = torch.empty(0, dtype=torch.uint8, device=device)

    # one seeded shuffle (minibatch composition then stays fixed across
    # epochs — standard for convex SGD; matches the torch reference path)
    rng = np.random.default_rng(seed)
    perm = torch.as_tensor(
        rng.permutation(n), dtype=torch.int64, device=device
    )
    Xs, XsT, ys, folds, rw = ds.shuffled_views(perm)
    targets = getattr(spec, "targets", None)
    tbits = mbits = None
    if targets is not None:
        if gk is not None:
            raise ValueError("targets do not go with the softmax loss")
        tmask = getattr(spec, "train_mask", None)
        for a in (targets, tmask):
            if a is not None and tuple(a.shape) != (n, ncols):
                raise ValueError(
                    f"targets / train_mask must be [{n}, {ncols}], got "
                    f"{tuple(a.shape)}")
        tbits = pack_bit_plane(targets, perm, Xs.shape[0], ncp)
        mbits = (
            pack_bit_plane(tmask, perm, Xs.shape[0], ncp)
            if tmask is not None
            else torch.empty(0, dtype=torch.int32, device=device)
        )
    if rw is None:
        rw_t = torch.empty(0, dtype=torch.float32, device=device)
        inv_m = torch.tensor(
            [1.0 / min(bs, n - s) for s in range(0, n, bs)],
            dtype=torch.float32)
    else:
        rw_t = rw
        sums = [
            float(rw[s: s + bs].sum()) for s in range(0, n, bs)
        ]
        inv_m = torch.tensor(
            [1.0 / max(v, 1e-30) for v in sums], dtype=torch.float32)
    col_l1 = getattr(spec, "col_l1", None)
    if tbits is not None:
        l1_args = ()
        if col_l1 is not None:
            if not 0.0 <= momentum < 1.0:
                raise ValueError("the L1 update needs momentum in [0, 1)")
            l1_args = (pad_cols(col_l1, 0.0), torch.zeros_like(W),
                       torch.zeros_like(W))
        if lr_decay == 0.0:
            ext.sgd_solve_bits(
                Xs, XsT, GT, W, V, WbfT, partial, ys, folds,
                cls_p, cfold_p, cls2_p, lr_p, l2_p, fmask, rw_t, inv_m,
                bs, int(loss_id), float(momentum), int(ds.intercept_row),
                int(epochs), tbits, mbits, *l1_args,
            )
        else:
            for epoch in range(epochs):
                lr_scale = 1.0 / (1.0 + lr_decay * epoch)
                ext.sgd_epoch_bits(
                    Xs, XsT, GT, W, V, WbfT, partial, ys, folds,
                    cls_p, cfold_p, cls2_p, lr_p, l2_p, fmask, rw_t,
                    inv_m, bs, int(loss_id), float(lr_scale),
                    float(momentum), int(ds.intercept_row),
                    tbits, mbits, *l1_args,
                )
    elif col_l1 is not None:
        if not 0.0 <= momentum < 1.0:
            raise ValueError("the L1 update needs momentum in [0, 1)")
        l1_p = pad_cols(col_l1, 0.0)
        cpos = torch.zeros_like(W)
        cneg = torch.zeros_like(W)
        if lr_decay == 0.0:
            ext.sgd_solve_l1(
                Xs, XsT, GT, W, V, WbfT, partial, ys, folds,
                cls_p, cfold_p, cls2_p, lr_p, l2_p, fmask, rw_t, inv_m,
                bs, int(loss_id), float(momentum), int(ds.intercept_row),
                int(epochs), l1_p, cpos, cneg, gk_arg,
            )
        else:
            for epoch in range(epochs):
                lr_scale = 1.0 / (1.0 + lr_decay * epoch)
                ext.sgd_epoch_l1(
                    Xs, XsT, GT, W, V, WbfT, partial, ys, folds,
                    cls_p, cfold_p, cls2_p, lr_p, l2_p, fmask, rw_t,
                    inv_m, bs, int(loss_id), float(lr_scale),
                    float(momentum), int(ds.intercept_row),
                    l1_p, cpos, cneg, gk_arg,
                )
    elif lr_decay == 0.0:
        # constant lr_scale: every epoch launches the identical
        # sequence — one C++ call, epochs 2..N replay a hipGraph
        ext.sgd_solve(
            Xs, XsT, GT, W, V, WbfT, partial, ys, folds,
            cls_p, cfold_p, cls2_p, lr_p, l2_p, fmask, rw_t, inv_m,
            bs, int(loss_id), float(momentum), int(ds.intercept_row),
            int(epochs), gk_arg,
        )
    else:
        for epoch in range(epochs):
            lr_scale = 1.0 / (1.0 + lr_decay * epoch)
            ext.sgd_epoch(
                Xs, XsT, GT, W, V, WbfT, partial, ys, folds,
                cls_p, cfold_p, cls2_p, lr_p, l2_p, fmask, rw_t, inv_m,
                bs, int(loss_id), float(lr_scale), float(momentum),
                int(ds.intercept_row), gk_arg,
            )
    if place is not None:
        return W.index_select(1, place)
    return W[:, :ncols]
