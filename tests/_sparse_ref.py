"""
Float64 numpy references of the sparse text-scale SGD step, kernel by
kernel (skdist_amd/ops/csrc/sparse_sgd_kernels.hip).  Every function takes
the buffers its kernel takes, as numpy arrays holding the VALUES of those
buffers (the bf16 G as float64 of its bf16 values), and returns float64.
Rounding G to bf16 is left to the caller (``bf16_rne``).

Besides the references: an independent batch-CSC builder, ``make_case``
(hand-built buffers of one solve, dyadic or random), the table of single-
step cases the GPU test runs (``STEP_CASES``) and the interval a log-loss
G element must fall into (``g_interval``), shared so that the CPU suite
can check the inputs' near-boundary share (tests/test_sparse_ref.py).

A plain helper module, not a conftest.
"""

import numpy as np

from _dense_ref import (EPS32, LOSS_HINGE, LOSS_LOG, LOSS_SQUARED,  # noqa
                        bf16_rne, bf16_step, ceil_to, dloss)

H_EPS = 1e-12   # the kernels' Adagrad epsilon (1e-12f)


def pad_cols(c):
    return ceil_to(c, 64)


def chunk_rule(m):
    """Rows per k_sp_colsum chunk as the host picks it: ceil(m/256)
    rounded up to 32, at least 32.  Returns (chunk, n_chunks)."""
    chunk = max(32, ceil_to((m + 255) // 256, 32))
    return chunk, (m + chunk - 1) // chunk


def csr_rows_dense(crow, cidx, cval, rows, f):
    """The CSR rows ``rows`` as a dense float64 [len(rows), f]."""
    X = np.zeros((len(rows), f))
    for i, r in enumerate(rows):
        k0, k1 = int(crow[r]), int(crow[r + 1])
        np.add.at(X[i], cidx[k0:k1], cval[k0:k1])
    return X


# ------------------------------------------------------------------ #
# kernels
# ------------------------------------------------------------------ #

def ref_fwd(crow, cidx, cval, W, Wb, s, y, fold, row_w, col_class,
            col_fold, col_class2, rows, loss_id):
    """K1 (k_sp_fwd) on the rows ``rows`` (global row ids).

    z = s[c] * sum_k val_k W[j_k, c] + Wb[c]; target y for a regression
    column (col_class < 0), else [y == col_class]; g = dloss * row_w
    where the element trains, else 0.  An element trains when the row's
    fold differs from the column's and, for a one-vs-one column
    (col_class2 >= 0), y is one of the pair.

    Returns dict: z, g (unrounded), train, absz = sum |val| |s W| and
    nnz (per row), the two the rounding bound of z is built from."""
    rows = np.asarray(rows, np.int64)
    W = np.asarray(W, np.float64)
    s = np.asarray(s, np.float64)
    X = csr_rows_dense(crow, cidx, np.asarray(cval, np.float64), rows,
                       W.shape[0])
    z = s[None, :] * (X @ W) + np.asarray(Wb, np.float64)[None, :]
    absz = np.abs(X) @ np.abs(s[None, :] * W)
    nnz = (np.asarray(crow)[rows + 1] - np.asarray(crow)[rows])
    yv = np.asarray(y, np.float64)[rows][:, None]
    cls = np.asarray(col_class).astype(np.int64)[None, :]
    c2 = np.asarray(col_class2).astype(np.int64)[None, :]
    is_cls = yv == cls.astype(np.float64)
    t = np.where(cls < 0, yv, is_cls.astype(np.float64))
    g = dloss(loss_id, z, t)
    if row_w is not None:
        g = g * np.asarray(row_w, np.float64)[rows][:, None]
    train = np.asarray(fold)[rows][:, None] != np.asarray(col_fold)[None, :]
    pair = is_cls | (yv == c2.astype(np.float64))
    train = train & ((c2 < 0) | pair)
    return dict(z=z, g=np.where(train, g, 0.0), train=train, absz=absz,
                nnz=nnz.astype(np.int64))


def ref_colsum(G, m, chunk):
    """K2a (k_sp_colsum): [n_chunks, cp] sums of G[:m] over row chunks."""
    G = np.asarray(G, np.float64)
    nch = (m + chunk - 1) // chunk
    return np.stack([G[z * chunk: min(m, (z + 1) * chunk)].sum(axis=0)
                     for z in range(nch)])


def ref_bias_scale(part, Wb, s, hb, col_lr, col_l2, inv_m, lr_scale,
                   col_l1=None, U=None):
    """K2b (k_sp_bias_scale[_l1]).  part [n_chunks, cp]; hb None = plain
    SGD intercept step, else Adagrad.  s' = s (1 - lr l2); with col_l1
    U += lr l1 / s'.  Returns dict Wb, s, hb, U and g, step, lr, r."""
    g = np.asarray(part, np.float64).sum(axis=0) * float(inv_m)
    lr = np.asarray(col_lr, np.float64) * float(lr_scale)
    hbn, r = None, np.ones_like(g)
    if hb is not None:
        hbn = np.asarray(hb, np.float64) + g * g
        r = 1.0 / np.sqrt(hbn + H_EPS)
    step = lr * g * r
    sn = np.asarray(s, np.float64) * (1.0 - lr * np.asarray(col_l2,
                                                            np.float64))
    Un = None
    if col_l1 is not None:
        Un = np.asarray(U, np.float64) + lr * np.asarray(
            col_l1, np.float64) / sn
    return dict(Wb=np.asarray(Wb, np.float64) - step, s=sn, hb=hbn, U=Un,
                g=g, step=step, lr=lr, r=r)


def ref_l1_touch(w, h, U, q, uw, ul):
    """sp_l1_touch on weight rows w [k, cp]: bring the L1 credit up to the
    column's U, clip towards 0, book what was applied.  h / uw / ul None =
    adaptive off (u = U); otherwise credit accrues at rsqrt(h + 1e-12)
    and not at all while h == 0.  Returns dict w, q, uw, ul and u, t (the
    amount subtracted from |w|), pre (the weight before the clamp)."""
    w = np.asarray(w, np.float64)
    q = np.asarray(q, np.float64)
    Uc = np.broadcast_to(np.asarray(U, np.float64)[None, :], w.shape)
    uwn = uln = None
    if uw is not None:
        h = np.asarray(h, np.float64)
        credit = (Uc - np.asarray(ul, np.float64)) / np.sqrt(h + H_EPS)
        u = np.asarray(uw, np.float64) + np.where(h > 0, credit, 0.0)
        uwn, uln = u.copy(), Uc.copy()
    else:
        u = Uc
    t = np.where(w > 0, u + q, u - q)
    pre = np.where(w > 0, w - t, np.where(w < 0, w + t, w))
    wn = np.where(w > 0, np.maximum(pre, 0.0),
                  np.where(w < 0, np.minimum(pre, 0.0), w))
    return dict(w=wn, q=q + (wn - w), uw=uwn, ul=uln, u=u, t=t, pre=pre)


def ref_update(ufeat, cptr, ridx, bval, G, W, h, s_new, col_lr, inv_m,
               lr_scale, U_new=None, q=None, uw=None, ul=None):
    """K3 (k_sp_update[_l1]) on one batch's CSC slice: ufeat [uf], cptr
    [uf+1] (offsets into ridx / bval), G [m, cp] bf16 values, W and the
    per-weight tables [f, cp].  s_new / U_new are K2b's outputs.  h None =
    plain SGD.  Returns dict of the full updated tables W, h, q, uw, ul
    and, for the touched rows [uf, cp]: a = sum bval G, absa = sum
    |bval G|, cnt (rows per slot), g, r, step, w1 (the weight after the
    gradient step, before the L1 touch) and the touch's own dict."""
    ufeat = np.asarray(ufeat, np.int64)
    cptr = np.asarray(cptr, np.int64)
    G = np.asarray(G, np.float64)
    uf = len(ufeat)
    cnt = cptr[1:] - cptr[:-1]
    slot = np.repeat(np.arange(uf), cnt)
    k = np.arange(int(cptr[0]), int(cptr[-1])) if uf else np.zeros(0, int)
    terms = np.asarray(bval, np.float64)[k][:, None] * G[
        np.asarray(ridx, np.int64)[k]]
    a = np.zeros((uf, G.shape[1]))
    absa = np.zeros_like(a)
    np.add.at(a, slot, terms)
    np.add.at(absa, slot, np.abs(terms))
    g = a * float(inv_m)
    lr = (np.asarray(col_lr, np.float64) * float(lr_scale))[None, :]
    Wn = np.array(W, np.float64)
    out = dict(a=a, absa=absa, cnt=cnt, g=g, h=None, q=None, uw=None,
               ul=None, touch=None)
    r = np.ones_like(g)
    if h is not None:
        hn = np.array(h, np.float64)
        hn[ufeat] = hn[ufeat] + g * g
        r = 1.0 / np.sqrt(hn[ufeat] + H_EPS)
        out["h"] = hn
    step = lr * g * r
    w1 = Wn[ufeat] - step / np.asarray(s_new, np.float64)[None, :]
    out.update(r=r, step=step, w1=w1)
    if U_new is not None:
        adaptive = uw is not None
        t = ref_l1_touch(w1, out["h"][ufeat] if adaptive else None, U_new,
                         np.asarray(q, np.float64)[ufeat],
                         np.asarray(uw, np.float64)[ufeat] if adaptive
                         else None,
                         np.asarray(ul, np.float64)[ufeat] if adaptive
                         else None)
        w1 = t["w"]
        out["touch"] = t
        out["q"] = np.array(q, np.float64)
        out["q"][ufeat] = t["q"]
        if adaptive:
            out["uw"] = np.array(uw, np.float64)
            out["ul"] = np.array(ul, np.float64)
            out["uw"][ufeat] = t["uw"]
            out["ul"][ufeat] = t["ul"]
    Wn[ufeat] = w1
    out["W"] = Wn
    return out


def ref_renorm(W, s):
    """k_sp_renorm: fold the lazy scale into W."""
    return np.asarray(W, np.float64) * np.asarray(s, np.float64)[None, :]


def ref_renorm_l1(W, s, q, uw, ul):
    """k_sp_renorm_l1: W and every stored-unit L1 table change units."""
    sc = np.asarray(s, np.float64)[None, :]
    f = lambda t: None if t is None else np.asarray(t, np.float64) * sc
    return f(W), f(q), f(uw), f(ul)


# ------------------------------------------------------------------ #
# batch CSC, written independently of SparseDeviceDataset.shuffled
# ------------------------------------------------------------------ #

def batch_csc(crow, cidx, cval, n, batch_size):
    """Per-batch CSC of a CSR whose rows are already in training order.
    Batch b holds rows [b*batch_size, ...); within it the features present
    are listed in increasing order and each feature's entries in
    increasing row order.  Returns ufeat [U] i32, cptr [U+1] i64 (global
    offsets into ridx / bval), ridx i32 (row within the batch), bval,
    ub_ptr [n_batches+1] i64 (slices ufeat; cptr is read at ub_ptr[b] +
    slot)."""
    ufeat, cptr, ridx, bval, ub_ptr = [], [0], [], [], [0]
    for start in range(0, n, batch_size):
        m = min(batch_size, n - start)
        by_feat = {}
        for i in range(m):
            for k in range(int(crow[start + i]), int(crow[start + i + 1])):
                by_feat.setdefault(int(cidx[k]), []).append((i, cval[k]))
        for j in sorted(by_feat):
            ufeat.append(j)
            for i, v in by_feat[j]:
                ridx.append(i)
                bval.append(v)
            cptr.append(len(ridx))
        ub_ptr.append(len(ufeat))
    return (np.asarray(ufeat, np.int32), np.asarray(cptr, np.int64),
            np.asarray(ridx, np.int32), np.asarray(bval, np.float64),
            np.asarray(ub_ptr, np.int64))


# ------------------------------------------------------------------ #
# cases
# ------------------------------------------------------------------ #

NNZ_CYCLE = (0, 1, 3, 4, 5, 7, 8, 9)     # both unroll-by-4 tails, empty
SLOT_ROWS = (1, 3, 4, 5, 9)              # rows per reserved CSC slot


def _make_csr(rng, n, f, dyadic, nnz_cycle, every_row, layout):
    """CSR with a prescribed nnz per row.  ``random``: row i holds
    nnz_cycle[i % len] features; the last len(SLOT_ROWS) features are
    reserved and placed in exactly 1, 3, 4, 5 and 9 rows (where n allows);
    ``every_row`` puts feature 0 into every row.  ``blocks``: row i holds
    the next nnz_cycle[...] features in sequence, so no two rows share a
    feature until the sequence wraps (many unique features per batch)."""
    sets = [set() for _ in range(n)]
    target = [nnz_cycle[i % len(nnz_cycle)] for i in range(n)]
    if layout == "blocks":
        j = 0
        for i in range(n):
            for _ in range(target[i]):
                sets[i].add(j % f)
                j += 1
    else:
        n_res = len(SLOT_ROWS) if f >= 20 else 0
        pool = np.arange(1 if every_row else 0, f - n_res)
        if every_row:
            for st in sets:
                st.add(0)
            target = [max(t, 1) for t in target]
        # reserved features go to the rows with the most room
        roomy = [i for i in np.argsort(-np.asarray(target), kind="stable")
                 if target[i] >= 3]
        for k in range(n_res):
            cnt = SLOT_ROWS[k]
            if cnt > len(roomy):
                continue
            for i in rng.choice(len(roomy), size=cnt, replace=False):
                sets[roomy[i]].add(f - 1 - k)
        for i in range(n):
            need = target[i] - len(sets[i])
            if need > 0:
                free = np.setdiff1d(pool, list(sets[i]))
                sets[i].update(rng.choice(free, size=need,
                                          replace=False).tolist())
    crow = np.zeros(n + 1, np.int64)
    cidx, cval = [], []
    for i, st in enumerate(sets):
        js = sorted(st)
        cidx += js
        crow[i + 1] = crow[i] + len(js)
    nnz = len(cidx)
    if dyadic:
        cval = rng.choice([-1.0, -0.5, 0.5, 1.0], size=nnz)
    else:
        v = rng.standard_normal(nnz)
        cval = bf16_rne(v)
    return crow, np.asarray(cidx, np.int32), np.asarray(cval, np.float64)


def make_case(seed, n, f, ncols, loss_id, dyadic=True, adaptive=False,
              l1=False, midfit=False, row_w=False, ovo=False,
              regress=False, batch_size=None, nnz_cycle=NNZ_CYCLE,
              every_row=False, layout="random", lr_scale=0.5):
    """Hand-built buffers of one sparse solve, as numpy arrays of buffer
    values (float64 holding fp32 / bf16 values).

    dyadic: val in {+-.5, +-1}, W and Wb multiples of 1/8 in [-.5, .5], s
    in {1, .5, .25}, row_w in {.5, 1, 2}, U a multiple of 1/16, q of 1/16,
    lr, lr_scale, l1 and inv_m powers of two, and l2 either 0 or 1/(2 lr)
    so that 1 - lr l2 is 1 or 1/2: every product, every sum in any order
    and the division by s' are then exact in fp32 as long as the sums stay
    below 2^24 grid units, which the test asserts per case.  inv_m is
    2^-min(6, ceil(log2 m)), not 1/m.
    Otherwise val is a bf16-rounded normal, W / Wb fp32 normals of size
    1/4 (one column 256x larger to reach the +-30 clamp of the log loss),
    the per-weight tables random fp32 and inv_m the solver's fp32
    1/m or 1/sum(row_w); lr, lr_scale, l2, l1 and s stay powers of two (so
    s' and every division by it are exact and the derived bounds of the
    later kernels stay short).

    midfit: s at .5 or .25 per column, non-zero W / Wb / h / hb / U / q /
    uw / ul with ul < U, some h == 0 (batches of up to 128 rows), weights of
    both signs, exact zeros,
    and weights that the L1 clip takes exactly to 0 (dyadic: W = U + q).
    Otherwise the state a fit starts from (zeros, s = 1).

    Columns cycle through CV columns of folds 0..2 (class 1), a full-data
    column (fold -2), one-vs-one columns (class 0 vs 2) when ``ovo`` and
    regression columns (class -1) when ``regress`` (squared loss).  Pad
    columns carry what sparse_sgd_fit pads with (class -99, fold -9,
    lr = l2 = l1 = 0) and zero state with s = 1."""
    rng = np.random.default_rng(seed)
    cp = pad_cols(ncols)
    bs = n if batch_size is None else batch_size
    crow, cidx, cval = _make_csr(rng, n, f, dyadic, nnz_cycle, every_row,
                                 layout)
    y = rng.integers(0, 3, size=n).astype(np.float64)
    fold = rng.integers(0, 3, size=n).astype(np.int32)
    rw = None
    if row_w:
        rw = np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, size=n)]

    kinds = [(1, 0, -1), (1, 1, -1), (1, 2, -1), (1, -2, -1)]
    if ovo:
        kinds += [(0, 0, 2), (0, -2, 2), (2, 1, 0)]
    if regress:
        assert loss_id == LOSS_SQUARED
        kinds += [(-1, 0, -1), (-1, -2, -1)]
    col_class = np.full(cp, -99, np.int32)
    col_fold = np.full(cp, -9, np.int32)
    col_class2 = np.full(cp, -1, np.int32)
    for c in range(ncols):
        col_class[c], col_fold[c], col_class2[c] = kinds[c % len(kinds)]
    col_lr = np.zeros(cp)
    col_l2 = np.zeros(cp)
    col_l1 = np.zeros(cp)
    col_lr[:ncols] = 2.0 ** -rng.integers(1, 4, size=ncols)
    halve = rng.random(ncols) < 0.5
    col_l2[:ncols] = np.where(halve, 0.5 / (col_lr[:ncols] * lr_scale), 0.0)
    col_l1[:ncols] = np.array([0.0, 2.0 ** -3, 2.0 ** -2])[
        rng.integers(0, 3, size=ncols)]

    z2 = lambda: np.zeros((f, cp))
    W, Wb, s = z2(), np.zeros(cp), np.ones(cp)
    h, hb = (z2(), np.zeros(cp)) if adaptive else (None, None)
    U, q = (np.zeros(cp), z2()) if l1 else (None, None)
    uw, ul = (z2(), z2()) if (l1 and adaptive) else (None, None)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    if midfit:
        s[:ncols] = rng.choice([0.5, 0.25], size=ncols)
        if dyadic:
            W[:, :ncols] = rng.integers(-4, 5, size=(f, ncols)) / 8.0
            Wb[:ncols] = rng.integers(-4, 5, size=ncols) / 8.0
        else:
            w = rng.standard_normal((f, ncols)) / 4.0
            w *= np.where(rng.random((f, ncols)) < 0.1, 0.01, 1.0)
            w[rng.random((f, ncols)) < 0.15] = 0.0
            if ncols > 5:
                w[:, 5] *= 256.0
            W[:, :ncols] = f32(w)
            Wb[:ncols] = f32(rng.standard_normal(ncols) / 4.0)
        if adaptive:
            hv = rng.uniform(0.0, 4.0, size=(f, ncols))
            if n <= 128:
                # with 1/m small, gradients of a large batch reach the
                # 1e-6 scale where, at h == 0, g rsqrt(h + g g + 1e-12)
                # turns from g 1e6 into sign(g): ill-conditioned by
                # design, so no derived bound stays near an ulp there
                hv[rng.random((f, ncols)) < 0.2] = 0.0
            if ncols > 5:
                # the saturating column's gradients are tiny: with h == 0
                # they would sit where g rsqrt(h + g g + 1e-12) turns from
                # g 1e6 into sign(g), ill-conditioned by design
                hv[:, 5] = np.maximum(hv[:, 5], 0.25)
            h[:, :ncols] = f32(hv)
            hb[:ncols] = f32(rng.uniform(0.1, 4.0, size=ncols))
        if l1:
            if dyadic:
                U[:ncols] = rng.integers(1, 5, size=ncols) / 16.0
                q[:, :ncols] = rng.integers(-2, 3, size=(f, ncols)) / 16.0
                # some positive weights sit exactly at their debt U + q:
                # the clip takes them to 0 with nothing to spare
                debt = U[None, :ncols] + q[:, :ncols]
                at = (rng.random((f, ncols)) < 0.1) & (debt > 0)
                W[:, :ncols] = np.where(at, debt, W[:, :ncols])
            else:
                U[:ncols] = f32(rng.uniform(0.01, 0.05, size=ncols))
                q[:, :ncols] = f32(rng.standard_normal((f, ncols)) * 0.01)
            if adaptive:
                uw[:, :ncols] = f32(rng.uniform(0.0, 0.05, size=(f, ncols)))
                ul[:, :ncols] = f32(U[None, :ncols] * rng.uniform(
                    0.3, 1.0, size=(f, ncols)))
                ul[:, :ncols] = np.minimum(ul[:, :ncols], U[None, :ncols])

    ufeat, cptr, ridx, bval, ub_ptr = batch_csc(crow, cidx, cval, n, bs)
    inv_m = []
    for start in range(0, n, bs):
        m = min(bs, n - start)
        if dyadic:
            inv_m.append(2.0 ** -min(6, int(np.ceil(np.log2(m)))))
        elif rw is None:
            inv_m.append(np.float32(1.0 / m))
        else:
            inv_m.append(np.float32(1.0 / float(rw[start:start + m].sum())))
    return dict(
        n=n, f=f, ncols=ncols, cp=cp, loss_id=loss_id, batch_size=bs,
        lr_scale=lr_scale, dyadic=dyadic, adaptive=adaptive, l1=l1,
        midfit=midfit,
        crow=crow, cidx=cidx, cval=cval, y=y, fold=fold, row_w=rw,
        col_class=col_class, col_fold=col_fold, col_class2=col_class2,
        col_lr=col_lr, col_l2=col_l2, col_l1=col_l1 if l1 else None,
        W=W, Wb=Wb, s=s, h=h, hb=hb, U=U, q=q, uw=uw, ul=ul,
        ufeat=ufeat, cptr=cptr, ridx=ridx, bval=bval, ub_ptr=ub_ptr,
        inv_m=np.asarray(inv_m, np.float64))


STATE_KEYS = ("W", "Wb", "s", "h", "hb", "U", "q", "uw", "ul")


def state_of(c):
    return {k: (None if c[k] is None else np.array(c[k], np.float64))
            for k in STATE_KEYS}


def batch_slices(c, bi):
    """(start, m, ufeat, cptr) of batch bi; cptr holds global offsets."""
    start = bi * c["batch_size"]
    m = min(c["batch_size"], c["n"] - start)
    u0, u1 = int(c["ub_ptr"][bi]), int(c["ub_ptr"][bi + 1])
    return start, m, c["ufeat"][u0:u1], c["cptr"][u0:u1 + 1]


def catchup(c, st, ufeat):
    """k_sp_l1_catchup: one touch of every (batch feature, column).
    Returns the touched state and the touch's dict."""
    st = dict(st)
    if not c["l1"] or len(ufeat) == 0:
        return st, None
    j = np.asarray(ufeat, np.int64)
    ad = c["adaptive"]
    t = ref_l1_touch(st["W"][j], st["h"][j] if ad else None, st["U"],
                     st["q"][j], st["uw"][j] if ad else None,
                     st["ul"][j] if ad else None)
    for k in ("W", "q") + (("uw", "ul") if ad else ()):
        st[k] = st[k].copy()
        st[k][j] = t["w" if k == "W" else k]
    return st, t


def composed_step(c, st, bi, round_g=True):
    """catch-up -> K1 -> K2a -> K2b -> K3 of batch bi from state ``st``,
    each reference fed by the one before (G rounded to bf16 between K1
    and the rest unless ``round_g`` is off).  Returns (state', G)."""
    start, m, ufeat, cptr = batch_slices(c, bi)
    st, _ = catchup(c, st, ufeat)
    fw = ref_fwd(c["crow"], c["cidx"], c["cval"], st["W"], st["Wb"],
                 st["s"], c["y"], c["fold"], c["row_w"], c["col_class"],
                 c["col_fold"], c["col_class2"], start + np.arange(m),
                 c["loss_id"])
    G = bf16_rne(fw["g"]) if round_g else fw["g"]
    chunk, _ = chunk_rule(m)
    b = ref_bias_scale(ref_colsum(G, m, chunk), st["Wb"], st["s"],
                       st["hb"], c["col_lr"], c["col_l2"], c["inv_m"][bi],
                       c["lr_scale"], c["col_l1"], st["U"])
    u = ref_update(ufeat, cptr, c["ridx"], c["bval"], G, st["W"], st["h"],
                   b["s"], c["col_lr"], c["inv_m"][bi], c["lr_scale"],
                   b["U"], st["q"], st["uw"], st["ul"])
    new = dict(W=u["W"], Wb=b["Wb"], s=b["s"], h=u["h"], hb=b["hb"],
               U=b["U"], q=u["q"], uw=u["uw"], ul=u["ul"])
    return new, G


def flush(c, st):
    """k_sp_l1_flush: one touch of every (feature, column)."""
    return catchup(c, st, np.arange(c["f"]))[0]


def g_interval(c, fw, rows):
    """[lo, hi] of bf16 values a log-loss G element may take, and the
    mask of elements with lo != hi (the reference lies within delta of a
    bf16 rounding boundary).  dz = nnz_row * eps * sum |val| |s W| bounds
    the fp32 accumulation of z (each of at most nnz_row adds rounds a
    running sum of at most sum |val| |s W|); sigmoid' <= 1/4 carries dz/4
    into g; 2^-20 is the project's allowance for __expf and the fp32
    roundings after it; row_w scales both."""
    dz = fw["nnz"][:, None] * EPS32 * fw["absz"]
    rw = np.ones(len(rows)) if c["row_w"] is None else c["row_w"][rows]
    delta = np.where(fw["train"], (dz / 4 + 2.0 ** -20) * rw[:, None], 0.0)
    lo, hi = bf16_rne(fw["g"] - delta), bf16_rne(fw["g"] + delta)
    return lo, hi, lo != hi, delta


def grid_of(x):
    """Largest power of two that every element of x is a multiple of (1.0
    for an all-zero x)."""
    x = np.ascontiguousarray(x, np.float64).ravel()
    x = x[x != 0]
    if x.size == 0:
        return 1.0
    mant, exp = np.frexp(np.abs(x))              # |x| = mant 2^exp
    k = (mant * 2.0 ** 53).astype(np.uint64)     # integer, exact
    low = k & (~k + np.uint64(1))                # lowest set bit
    return float(2.0 ** (np.log2(low.astype(np.float64)) + exp - 53).min())


def is_f32(x):
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(x.astype(np.float32).astype(np.float64), x))


def assert_exact_step(c, st_c, fw, G, part, b, u):
    """What makes a dyadic case exact on the device whatever the order of
    its fp32 sums: terms on a grid 2^-k whose magnitudes sum to less than
    2^24 grid units give partial sums that are integers below 2^24 in
    grid units, hence fp32 values; and every elementwise result of the
    float64 reference is itself an fp32 value, so the one fp32 operation
    that produces it from exact operands does not round.  Arguments: the
    caught-up state, ref_fwd's dict, the bf16 G, ref_colsum's part and
    the dicts of ref_bias_scale and ref_update."""
    lim = 2.0 ** 24
    g1 = grid_of(c["cval"]) * grid_of(st_c["W"]) * grid_of(st_c["s"])
    assert fw["absz"].max() / g1 < lim, ("K1 sum", fw["absz"].max() / g1)
    assert is_f32(fw["z"]) and is_f32(fw["g"])
    assert np.abs(G).sum(axis=0).max() / grid_of(G) < lim
    assert is_f32(part) and is_f32(part.sum(axis=0))
    for k in ("g", "step", "Wb", "s"):
        assert is_f32(b[k]), ("K2b", k)
    if b["U"] is not None:
        assert is_f32(b["U"]) and is_f32(b["U"] - st_c["U"])
    g3 = grid_of(c["bval"]) * grid_of(G)
    assert u["absa"].max(initial=0.0) / g3 < lim, "K3 sum"
    for k in ("g", "step", "w1"):
        assert is_f32(u[k]), ("K3", k)
    assert is_f32(u["step"] / b["s"][None, :])
    if u["touch"] is not None:
        for k in ("t", "pre", "w", "q"):
            assert is_f32(u["touch"][k]), ("K3 touch", k)
        assert is_f32(u["touch"]["w"] - u["w1"])


# Single-step cases of tests/test_sparse_sgd_kernels_gpu.py: name ->
# make_case arguments (n == batch_size == m: one step).  What each reaches
# is in that file's table.  exact = hinge / squared loss, adaptive off;
# the others are log loss with adaptive on.
def _sc(n, f, ncols, loss, **kw):
    exact = loss != LOSS_LOG
    return dict(n=n, f=f, ncols=ncols, loss_id=loss, dyadic=exact,
                adaptive=not exact, **kw)


STEP_CASES = {
    "c64-m5": _sc(5, 40, 24, 1),
    "c64-m1-l1-mid": _sc(1, 40, 24, 2, l1=True, midfit=True, regress=True,
                         nnz_cycle=(5,)),
    "c128-m31-mid": _sc(31, 60, 100, 2, midfit=True, row_w=True, ovo=True),
    "c192-m33-l1-mid": _sc(33, 60, 150, 1, l1=True, midfit=True,
                           row_w=True, ovo=True),
    "c192-m96-mid": _sc(96, 60, 150, 2, midfit=True, every_row=True,
                        regress=True),
    "c256-m128-l1": _sc(128, 60, 200, 1, l1=True),
    "c320-m33-l1-mid": _sc(33, 60, 290, 2, l1=True, midfit=True, ovo=True,
                           row_w=True, regress=True),
    "c320-m96": _sc(96, 60, 290, 1, every_row=True),
    "c256-m2100-mid": _sc(2100, 300, 200, 2, midfit=True),
    "c256-uf2400-l1-mid": _sc(300, 2400, 200, 1, l1=True, midfit=True,
                              nnz_cycle=(8,), layout="blocks"),
    "c64-m8200-mid": _sc(8200, 50, 24, 1, midfit=True),
    "c64-empty-l1-mid": _sc(32, 40, 24, 2, l1=True, midfit=True,
                            nnz_cycle=(0,)),
    "log-c64-m33-fresh": _sc(33, 60, 24, 0, row_w=True),
    "log-c192-m96-l1-mid": _sc(96, 60, 150, 0, l1=True, midfit=True,
                               ovo=True, row_w=True),
    "log-c320-m31-l1-mid": _sc(31, 60, 290, 0, l1=True, midfit=True),
    "log-c256-m2100-mid": _sc(2100, 300, 200, 0, midfit=True),
    "log-c128-m5-l1": _sc(5, 40, 100, 0, l1=True),
    "log-c192-m33-mid": _sc(33, 60, 150, 0, midfit=True, every_row=True),
}


def step_case(name):
    return make_case(sum(map(ord, name)), **STEP_CASES[name])
