"""Missing values (NaN) in the tree stack, GPU tier: the MISSING
instantiations of the split scan (k_tree_split_m / k_tree_split_wm), the
partition predicate with a per-slot direction flag, the MISS traversal
kernels, and the device fits built on them.

As in test_boosting_weights_gpu.py the kernel tests use values whose every
partial sum is exactly representable in f32 (integer y in [-4, 4], integer
multiplicities in {1, 2, 3}, row weights in quarters), so stats compare
bitwise with the fp64 host reference whatever the order of the sums."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_missing_values import (
    holes,
    missing_vs_rest_data,
    stump_data,
    trees_of,
)

pytestmark = pytest.mark.gpu

from skdist_amd.models import (
    HistGradientBoostingClassifier,
    HistGradientBoostingRegressor,
)
from skdist_amd.models.forest import (
    BinnedDataset,
    FlatForest,
    ForestBuilder,
    HistTree,
    _feat_hashes,
    flat_forest_for,
)

if torch.cuda.is_available():
    from skdist_amd.ops import require_hip

NBINS = 256
MISS = NBINS - 1
CRIT_GINI, CRIT_MSE = 0, 2
CHUNK_ROWS = 32768
MARGIN = 1e-4

# (S, is_cls, cnt_stat): regression (w, wy, wyy); regression with a row
# weight plane and the count stat; 3-class gini
KINDS = {"reg3": (3, 0, -1), "reg4": (4, 0, 3), "cls3": (3, 1, -1)}


# ---------------------------------------------------------------------- #
# tree_split in missing mode against an fp64 brute force over (j, b, d)
# ---------------------------------------------------------------------- #
def make_node(rng, f, kind, shape, m=400, nan=True):
    """One frontier node's histogram [f, NBINS, S] (fp64, exact small
    numbers) built from m synthetic rows with a planted best cut;
    ``nan=False`` leaves the top bin of every feature empty."""
    S, is_cls, _ = KINDS[kind]
    if shape == "single":
        m = 1
    codes = rng.integers(0, MISS, (m, f))              # present: 0..254
    if nan:
        codes[rng.random((m, f)) < 0.15] = MISS
    js = int(rng.integers(f))
    c = rng.integers(0, MISS, m)
    gone = np.zeros(m, dtype=bool)
    if shape in ("L", "R"):
        bs = int(rng.integers(60, 190))
        gone = rng.random(m) < 0.3
        left_like = (c <= bs) | gone if shape == "L" else (c <= bs) & ~gone
    elif shape == "top":            # all present | all missing
        gone = rng.random(m) < 0.4
        c[np.flatnonzero(~gone)[:3]] = MISS - 1        # bin 254 is occupied
        # ... and so is bin 0: no cut has the missing rows alone on the
        # left, the mirror image of the planted one with the same gain
        c[np.flatnonzero(~gone)[3:6]] = 0
        left_like = ~gone
    elif shape in ("maj_left", "maj_right"):           # nothing missing
        bs = int(rng.integers(180, 230) if shape == "maj_left"
                 else rng.integers(20, 70))
        left_like = c <= bs
    elif shape == "minleaf":
        # 20 present rows below the cut, 100 missing rows that belong with
        # them: only the missing rows lift the left side over min_leaf = 50
        bs = 99
        c = np.r_[rng.integers(0, bs + 1, 20), rng.integers(bs + 1, MISS,
                                                            m - 120),
                  np.zeros(100, dtype=np.int64)]
        c[0] = bs                                      # bin 99 is occupied
        gone = np.r_[np.zeros(m - 100, dtype=bool), np.ones(100, dtype=bool)]
        left_like = (c <= bs) | gone
    else:
        assert shape == "single"
        left_like = np.ones(m, dtype=bool)
    c[gone] = MISS
    codes[:, js] = c
    if f > 1 and shape != "single" and nan:
        codes[:, (js + 1) % f] = MISS                  # entirely missing
    mult = (np.ones(m) if shape in ("minleaf", "single")
            else rng.integers(1, 4, m).astype(np.float64))
    H = np.zeros((f, NBINS, S))
    jj = np.broadcast_to(np.arange(f), (m, f))
    if is_cls:
        cls = np.where(left_like, 0, 1)
        flip = rng.random(m) < 0.1
        cls[flip] = 2
        np.add.at(H, (jj, codes, np.broadcast_to(cls[:, None], (m, f))),
                  np.broadcast_to(mult[:, None], (m, f)))
        return H
    y = np.where(left_like, 3.0, -3.0) + rng.integers(-1, 2, m)
    w = mult * rng.integers(1, 9, m) / 4.0 if S == 4 else mult
    for s, v in enumerate((w, w * y, w * y * y, mult)[:S]):
        np.add.at(H[:, :, s], (jj, codes),
                  np.broadcast_to(v[:, None], (m, f)))
    return H


def brute_split(H, kind, min_leaf, sel=None, missing=True):
    """fp64 reference of one node: every (feature, bin <= NBINS-2,
    direction) candidate, best gain, ties to the lower (j, b, d)."""
    S, is_cls, cnt_stat = KINDS[kind]
    f = H.shape[0]
    parent = H[0].sum(axis=0)
    wp = parent.sum() if is_cls else parent[0]

    def imp(s, w):
        with np.errstate(all="ignore"):
            if is_cls:
                r = 1.0 - (s ** 2).sum(axis=-1) / (w * w)
            else:
                mean = s[..., 1] / w
                r = np.maximum(s[..., 2] / w - mean * mean, 0.0)
        return np.where(w > 0, r, 0.0)

    imp_p = float(imp(parent, wp))
    cum = H.cumsum(axis=1)[:, :-1]                     # [f, nb-1, S]
    miss = H[:, MISS]
    wm = miss.sum(axis=-1) if is_cls else miss[:, 0]
    left = np.stack([cum, cum + miss[:, None, :]] if missing else [cum],
                    axis=2)                            # [f, nb-1, D, S]
    wl = left.sum(axis=-1) if is_cls else left[..., 0]
    wr = wp - wl
    with np.errstate(all="ignore"):                    # an empty node
        gain = imp_p - (wl * imp(left, wl)
                        + wr * imp(parent - left, wr)) / wp
    if cnt_stat >= 0:
        cl = left[..., cnt_stat]
        cr = parent[cnt_stat] - cl
        valid = (cl >= min_leaf) & (cr >= min_leaf) & (wl > 0) & (wr > 0)
    else:
        valid = (wl >= min_leaf) & (wr >= min_leaf)
    if missing:
        valid[:, :, 1] &= (wm > 0)[:, None]            # L needs missing rows
    if sel is not None:
        valid &= sel[:, None, None]
    gain = np.where(valid, gain, -1.0)
    best = float(gain.max())
    out = dict(feat=-1, bin=-1, mleft=0, wl=0.0, gain=-1.0, imp=imp_p,
               stats=parent, lstats=np.zeros(S), d=-1, wm=wm)
    if not valid.any():
        return out
    assert best > 0, "degenerate node: a valid cut without gain"
    tied = np.argwhere(gain == best)                   # (j, b, d) ascending
    j, b, d = (int(v) for v in tied[0])
    # a condition on the INPUTS: candidates that tie exactly are the same
    # partition, every other one trails by a relative margin f32 keeps
    for jj, bb, dd in tied:
        assert np.array_equal(left[jj, bb, dd], left[j, b, d])
    rest = gain[gain < best]
    assert not len(rest) or rest.max() <= best * (1 - MARGIN), (
        "runner-up within the margin", best, rest.max())
    w_left = float(wl[j, b, d])
    mleft = 1 if d == 1 else int(not wm[j] > 0 and 2 * w_left > wp)
    out.update(feat=j, bin=b, mleft=mleft, wl=w_left, gain=best,
               lstats=left[j, b, d], d=d)
    return out


def run_split(H, kind, min_leaf, m_features, seeds, missing):
    """ext.tree_split on [NF, f, NBINS, S]; missing=None is the call with
    the argument list from before the missing mode."""
    S, is_cls, cnt_stat = KINDS[kind]
    ext = require_hip()
    dev = "cuda"
    NF, f = H.shape[:2]
    hist = torch.as_tensor(np.ascontiguousarray(H, dtype=np.float32),
                           device=dev)
    assert np.array_equal(hist.cpu().numpy().astype(np.float64), H)
    seed = torch.as_tensor(np.asarray(seeds, dtype=np.uint32).view(np.int32),
                           device=dev)
    oi = lambda: torch.full((NF,), -7, dtype=torch.int32, device=dev)
    of = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    out = (oi(), oi(), of(NF), of(NF), of(NF), of(NF, S), of(NF, S))
    mleft = oi()
    args = (hist, seed, f, NBINS, S, is_cls,
            CRIT_GINI if is_cls else CRIT_MSE, m_features, 0,
            float(min_leaf), *out, cnt_stat)
    if missing is None:
        ext.tree_split(*args)
    else:
        ext.tree_split(*args, 1, mleft)
    torch.cuda.synchronize()
    names = ("feat", "bin", "wl", "gain", "imp", "stats", "lstats")
    got = {k: o.cpu().numpy() for k, o in zip(names, out)}
    got["mleft"] = mleft.cpu().numpy()
    return got


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_split(got, refs):
    for k, ref in enumerate(refs):
        where = f"node {k}"
        assert got["feat"][k] == ref["feat"], where
        assert got["bin"][k] == ref["bin"], where
        if "mleft" in got:
            assert got["mleft"][k] == ref["mleft"], where
        assert np.array_equal(bits(got["stats"][k]), bits(ref["stats"])), where
        assert np.array_equal(bits(got["lstats"][k]),
                              bits(ref["lstats"])), where
        assert got["wl"][k] == np.float32(ref["wl"]), where
        # f32 rounding of a gain scales with the impurities it is the
        # difference of, not with the gain itself
        np.testing.assert_allclose(got["gain"][k], ref["gain"], rtol=0,
                                   atol=1e-5 * max(ref["imp"], 1e-30))
        np.testing.assert_allclose(got["imp"][k], ref["imp"], rtol=1e-5)


SHAPES = ("L", "R", "top", "maj_left", "maj_right", "single")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("f", [3, 7, 300])
def test_tree_split_missing_matches_brute_force(f, kind):
    rng = np.random.default_rng(1000 + f)
    H = np.stack([make_node(rng, f, kind, s) for s in SHAPES])
    refs = [brute_split(H[k], kind, 1) for k in range(len(SHAPES))]
    by = dict(zip(SHAPES, refs))
    # the node shapes are the ones meant
    assert by["L"]["d"] == 1 and by["L"]["mleft"] == 1
    assert by["R"]["d"] == 0 and by["R"]["mleft"] == 0
    assert by["R"]["wm"][by["R"]["feat"]] > 0
    assert by["top"]["bin"] == NBINS - 2 and by["top"]["d"] == 0
    for name, flag in (("maj_left", 1), ("maj_right", 0)):
        assert by[name]["wm"][by[name]["feat"]] == 0
        assert (by[name]["d"], by[name]["mleft"]) == (0, flag)
    assert by["single"]["feat"] == -1
    if f > 1:   # a feature that holds nothing but missing rows
        assert (H[0, :, :MISS].sum(axis=(1, 2)) == 0).any()
    got = run_split(H, kind, 1, f, np.zeros(len(SHAPES)), missing=1)
    check_split(got, refs)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("f", [3, 7, 300])
def test_tree_split_missing_feature_subsample(f, kind):
    # a node that loses its planted feature is decided among noise cuts;
    # these seeds leave every such winner clear of its runner-up
    rng = np.random.default_rng(2100 + f)
    shapes = ("L", "R", "top", "maj_left", "L", "R")
    H = np.stack([make_node(rng, f, kind, s) for s in shapes])
    seeds = rng.integers(1, 2 ** 32, len(shapes), dtype=np.uint64)
    m_features = max(1, f // 2)
    refs = []
    for k in range(len(shapes)):
        hv = _feat_hashes(int(seeds[k]), f)
        sel = hv <= np.sort(hv)[m_features - 1]
        assert sel.sum() == m_features
        refs.append(brute_split(H[k], kind, 1, sel=sel))
        assert refs[-1]["feat"] < 0 or sel[refs[-1]["feat"]]
    full = [brute_split(H[k], kind, 1)["feat"] for k in range(len(shapes))]
    # the subsample took some node's best feature away
    assert any(a != r["feat"] for a, r in zip(full, refs))
    got = run_split(H, kind, 1, m_features, seeds, missing=1)
    check_split(got, refs)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("f", [3, 7, 300])
def test_tree_split_min_leaf_met_by_missing_rows_only(f, kind):
    rng = np.random.default_rng(3000 + f)
    shapes = ("minleaf", "L", "R", "top", "maj_left", "maj_right")
    H = np.stack([make_node(rng, f, kind, s) for s in shapes])
    refs = [brute_split(H[k], kind, 50) for k in range(len(shapes))]
    a = refs[0]
    assert (a["bin"], a["d"], a["mleft"]) == (99, 1, 1)
    S, is_cls, cnt_stat = KINDS[kind]
    present_left = H[0, a["feat"], :100].sum(axis=0)
    n_left = (present_left.sum() if is_cls
              else present_left[max(cnt_stat, 0)])
    assert n_left == 20 < 50                 # R at this cut is not valid
    got = run_split(H, kind, 50, f, np.zeros(len(shapes)), missing=1)
    check_split(got, refs)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("f", [3, 300])
def test_tree_split_old_call_on_empty_top_bin(f, kind):
    """The argument list from before the missing mode still works and is
    the plain prefix scan; on a histogram whose top bin is empty the missing
    mode finds the same split, bit for bit, and adds the majority flag."""
    rng = np.random.default_rng(4000 + f)
    shapes = ("maj_left", "maj_right") * 2 + ("maj_left", "single")
    H = np.stack([make_node(rng, f, kind, s, nan=False) for s in shapes])
    assert not H[:, :, MISS, :].any()
    plain = [brute_split(H[k], kind, 1, missing=False)
             for k in range(len(shapes))]
    refs = [brute_split(H[k], kind, 1) for k in range(len(shapes))]
    assert {r["mleft"] for r in refs} == {0, 1}
    old = run_split(H, kind, 1, f, np.zeros(len(shapes)), missing=None)
    assert (old.pop("mleft") == -7).all()     # not given, not written
    check_split(old, plain)
    new = run_split(H, kind, 1, f, np.zeros(len(shapes)), missing=1)
    check_split(new, refs)
    for name in old:
        assert np.array_equal(old[name].view(np.uint32),
                              new[name].view(np.uint32)), name


def test_tree_split_rejects_bad_missing_arguments():
    H = np.stack([make_node(np.random.default_rng(0), 3, "reg3", "L")])
    ext = require_hip()
    dev = "cuda"
    hist = torch.as_tensor(H.astype(np.float32), device=dev)
    seed = torch.zeros(1, dtype=torch.int32, device=dev)
    oi = lambda n=1: torch.zeros(n, dtype=torch.int32, device=dev)
    of = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)

    def call(extra_mode, *tail):
        ext.tree_split(hist, seed, 3, NBINS, 3, 0, CRIT_MSE, 3, extra_mode,
                       1.0, oi(), oi(), of(1), of(1), of(1), of(1, 3),
                       of(1, 3), -1, *tail)

    with pytest.raises(RuntimeError, match="out_mleft"):
        call(0, 1)                                        # flag, no output
    with pytest.raises(RuntimeError, match="out_mleft"):
        call(0, 0, oi())                                  # output, no flag
    with pytest.raises(RuntimeError, match="out_mleft"):
        call(0, 1, oi(2))                                 # wrong length
    with pytest.raises(RuntimeError, match="out_mleft"):
        call(0, 1, of(1))                                 # wrong dtype
    with pytest.raises(RuntimeError, match="out_mleft"):
        call(0, 1, oi().cpu())                            # wrong device
    with pytest.raises(RuntimeError, match="extra_mode"):
        call(1, 1, oi())


# ---------------------------------------------------------------------- #
# part_count / part_scatter with a per-slot direction flag
# ---------------------------------------------------------------------- #
def _chunks(segments):
    out = []
    for slot, tree, start, count in segments:
        for off in range(0, count, CHUNK_ROWS):
            out.append((slot, tree, start + off,
                        min(CHUNK_ROWS, count - off)))
    return np.asarray(out, dtype=np.int32)


def _run_partition(codes, si, segments, feat, bin_, tail):
    """K3 + the host prefix + K4, as ForestBuilder._partition does them;
    ``tail`` holds the trailing (split_mleft, missing_code) or nothing."""
    ext = require_hip()
    dev = "cuda"
    n = codes.shape[0]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    ch = _chunks(segments)
    counts = torch.full((len(ch),), -1, dtype=torch.int32, device=dev)
    args = (t(codes), t(si), t(ch), t(feat), t(bin_))
    ext.part_count(*args, n, counts, *tail)
    cnt = counts.cpu().numpy().astype(np.int64)
    slot = ch[:, 0]
    nl = np.bincount(slot, weights=cnt, minlength=len(segments)).astype(
        np.int64)
    lbase = np.zeros(len(ch), dtype=np.int32)
    rbase = np.zeros(len(ch), dtype=np.int32)
    run_l = np.zeros(len(segments), dtype=np.int64)
    run_r = np.zeros(len(segments), dtype=np.int64)
    for k, (s, _, start, count) in enumerate(ch):
        seg_start = segments[s][2]
        lbase[k] = seg_start + run_l[s]
        rbase[k] = seg_start + nl[s] + run_r[s]
        run_l[s] += cnt[k]
        run_r[s] += count - cnt[k]
    out = torch.full_like(t(si), -1)
    ext.part_scatter(*args, t(lbase), t(rbase), n, out, *tail)
    torch.cuda.synchronize()
    return nl, out.cpu().numpy()


def test_partition_with_missing_direction():
    sizes = [1, 63, 64, 257, 1000, 33_000]
    n = sum(sizes)
    f, fp = 5, 8
    rng = np.random.default_rng(11)
    codes = np.zeros((n, fp), dtype=np.uint8)
    codes[:, :f] = rng.integers(0, 256, (n, f), dtype=np.uint8)
    codes[rng.random((n, fp)) < 0.2] = MISS
    codes[:, f:] = 0
    si = rng.permutation(n).astype(np.int32)[None, :]
    codes[si[0, 0], :f] = MISS             # the 1-row segment holds a 255
    starts = np.cumsum([0] + sizes[:-1])
    segments = [(k, 0, int(starts[k]), sizes[k]) for k in range(len(sizes))]
    assert len(_chunks(segments)) == len(sizes) + 1     # 33 000: two chunks
    feat = np.array([0, 1, 2, 3, 4, 2], dtype=np.int32)
    bin_ = np.array([100, 30, 200, 128, 254, 77], dtype=np.int32)
    mleft = np.array([1, 0, 1, 0, 1, 1], dtype=np.int32)
    dev = "cuda"
    tail = (torch.as_tensor(mleft, device=dev), MISS)

    def reference(flags):
        ref = np.full(n, -1, dtype=np.int32)
        nl = np.zeros(len(sizes), dtype=np.int64)
        for k, _, start, count in segments:
            rows = si[0, start:start + count]
            c = codes[rows, feat[k]]
            go = (c <= bin_[k]) | ((flags[k] != 0) & (c == MISS))
            nl[k] = go.sum()
            ref[start:start + count] = np.r_[rows[go], rows[~go]]   # stable
        return nl, ref

    nl, out = _run_partition(codes, si, segments, feat, bin_, tail)
    ref_nl, ref = reference(mleft)
    np.testing.assert_array_equal(nl, ref_nl)
    np.testing.assert_array_equal(out[0], ref)
    # the flags moved rows, and the 1-row segment went left through its flag
    nl0, out0 = _run_partition(codes, si, segments, feat, bin_, ())
    ref_nl0, ref0 = reference(np.zeros_like(mleft))
    np.testing.assert_array_equal(nl0, ref_nl0)
    np.testing.assert_array_equal(out0[0], ref0)
    assert (nl[mleft == 1] > nl0[mleft == 1]).all() and nl[0] == 1
    np.testing.assert_array_equal(nl[mleft == 0], nl0[mleft == 0])
    # all-zero flags are the flag-free call
    nlz, outz = _run_partition(
        codes, si, segments, feat, bin_,
        (torch.zeros(len(sizes), dtype=torch.int32, device=dev), MISS))
    np.testing.assert_array_equal(nlz, nl0)
    np.testing.assert_array_equal(outz, out0)

    with pytest.raises(RuntimeError, match="split_mleft"):
        _run_partition(codes, si, segments, feat, bin_,
                       (tail[0][:-1], MISS))
    with pytest.raises(RuntimeError, match="split_mleft"):
        _run_partition(codes, si, segments, feat, bin_,
                       (tail[0].to(torch.uint8), MISS))
    with pytest.raises(RuntimeError, match="missing_code"):
        _run_partition(codes, si, segments, feat, bin_, (tail[0], 256))


# ---------------------------------------------------------------------- #
# traversal
# ---------------------------------------------------------------------- #
def random_tree(rng, f, vs, max_depth):
    feature, thr, left, right, mleft, values = [], [], [], [], [], []

    def grow(depth):
        i = len(feature)
        for a in (feature, thr, left, right, mleft):
            a.append(0)
        if depth == max_depth or (depth > 0 and rng.random() < 0.2):
            feature[i] = -1
            left[i] = len(values)
            values.append(rng.integers(0, 65, vs) / 64.0)
            return i
        feature[i] = int(rng.integers(f))
        thr[i] = float(rng.integers(-4, 5)) / 4.0
        mleft[i] = int(rng.integers(2))
        left[i] = grow(depth + 1)
        right[i] = grow(depth + 1)
        return i

    grow(0)
    return HistTree(
        np.asarray(feature, dtype=np.int32), np.asarray(thr, np.float32),
        np.asarray(left, dtype=np.int32), np.asarray(right, dtype=np.int32),
        np.asarray(values, dtype=np.float32), None, f, None,
        np.asarray(mleft, dtype=np.uint8))


@pytest.mark.parametrize("vs", [1, 32])
@pytest.mark.parametrize("n_trees", [1, 65])
@pytest.mark.parametrize("rows", [1, 257])
def test_traversal_follows_missing_left(rows, n_trees, vs):
    f = 9
    rng = np.random.default_rng(rows * 1000 + n_trees * 10 + vs)
    trees = [random_tree(rng, f, vs, int(rng.integers(1, 7)))
             for _ in range(n_trees)]
    X = holes(np.round(rng.standard_normal((rows, f)) * 4) / 4, 0.2,
              rows + n_trees)
    X[0, :] = np.nan                     # a row that is missing everywhere
    Xs = sp.csr_matrix(X)                # every NaN is a stored entry
    assert np.isnan(Xs.data).sum() == np.isnan(X).sum()

    ff = FlatForest(trees, "cuda")
    assert ff.mleft is not None
    host_ids = np.column_stack([t.apply(X) for t in trees])
    ids_d, ids_s = ff.apply(X), ff.apply(Xs)
    np.testing.assert_array_equal(ids_d, host_ids)
    np.testing.assert_array_equal(ids_s, host_ids)
    pd, ps = ff.predict_value(X), ff.predict_value(Xs)
    assert np.array_equal(pd.view(np.uint32), ps.view(np.uint32))
    host = np.mean([t.predict_proba(X).astype(np.float64) for t in trees],
                   axis=0)
    np.testing.assert_allclose(pd, host, atol=1e-5, rtol=0)

    # without flags the same forest walks as before: NaN goes right
    bare = [HistTree(t.feature, t.threshold, t.left, t.right, t.value, None,
                     f, None) for t in trees]
    fb = FlatForest(bare, "cuda")
    assert fb.mleft is None
    bare_ids = np.column_stack([t.apply(X) for t in bare])
    np.testing.assert_array_equal(fb.apply(X), bare_ids)
    np.testing.assert_array_equal(fb.apply(Xs), bare_ids)
    if any(t.missing_left[0] == 1 for t in trees):
        # row 0 is NaN everywhere: it leaves such a root on the other side
        assert (bare_ids[0] != host_ids[0]).any()
    pb = fb.predict_value(X)
    assert np.array_equal(pb.view(np.uint32),
                          fb.predict_value(Xs).view(np.uint32))
    host_b = np.mean([t.predict_proba(X).astype(np.float64) for t in bare],
                     axis=0)
    np.testing.assert_allclose(pb, host_b, atol=1e-5, rtol=0)


def test_traversal_rejects_bad_flags():
    rng = np.random.default_rng(5)
    trees = [random_tree(rng, 4, 1, 3)]
    ff = FlatForest(trees, "cuda")
    X = np.zeros((3, 4), dtype=np.float32)
    ff.mleft = ff.mleft[:-1].contiguous()
    with pytest.raises(RuntimeError, match="mleft"):
        ff.apply(X)
    with pytest.raises(RuntimeError, match="mleft"):
        ff.predict_value(sp.csr_matrix(X))
    ff.mleft = torch.zeros(len(ff.feat), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="mleft"):
        ff.predict_value(X)


# ---------------------------------------------------------------------- #
# builder: HIP engine against the eager mirror on a NaN dataset
# ---------------------------------------------------------------------- #
def _nan_dataset(n=2000, f=7, seed=21):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f)).astype(np.float32)
    t = 2 * X[:, 0] + 1.5 * X[:, 1] * (X[:, 2] > 0) - X[:, 3]
    X = holes(X, 0.15, seed + 1)
    gone = np.isnan(X[:, 0])
    t = np.where(gone, 3.0, np.where(np.isnan(t), 0.0, t))
    y = np.clip(np.round(t), -4, 4)
    return X, y


@pytest.mark.parametrize("case", ["reg", "cls3", "row_weight"])
def test_hip_builder_matches_eager_on_nan_data(case, monkeypatch):
    monkeypatch.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
    X, y = _nan_dataset()
    kw = {}
    if case == "cls3":
        target, crit = np.digitize(y, [-1.5, 1.5]), "gini"
    else:
        target, crit = y.astype(np.float32), "squared_error"
    if case == "row_weight":
        kw["row_weight"] = (np.random.default_rng(3).integers(
            1, 9, len(y)) / 4.0).astype(np.float32)
    ds = BinnedDataset(X, target, "cuda", is_cls=case == "cls3",
                       allow_missing=True, **kw)
    assert ds.missing_bin == MISS and ds.S == (4 if kw else 3)
    bkw = dict(max_depth=4, bootstrap=False, min_samples_leaf=5)
    th = ForestBuilder(ds, crit, engine="hip", **bkw).build([7])[0]
    te = ForestBuilder(ds, crit, engine="eager", **bkw).build([7])[0]
    assert th.node_count >= 15
    for name in ("feature", "threshold", "left", "right", "value",
                 "missing_left"):
        np.testing.assert_array_equal(getattr(th, name), getattr(te, name),
                                      name)
    inner = th.feature >= 0
    assert set(th.missing_left[inner]) == {0, 1}


# ---------------------------------------------------------------------- #
# end to end on the device
# ---------------------------------------------------------------------- #
def test_device_stump_learns_missing_left():
    X, y = stump_data()
    m = HistGradientBoostingRegressor(
        n_estimators=1, learning_rate=1, max_depth=1, allow_nan=True,
        random_state=0).fit(X, y)
    t = m.stages_[0][0]
    assert t.feature[0] == 0 and t.missing_left[0] == 1
    pred = m.predict(X)
    assert np.abs(pred - y).max() < 2e-4       # f32 sums of 3000 residuals
    np.testing.assert_array_equal(np.round(pred), y)
    dev_pred = m._device_predict_fn("predict", "cuda")(X)
    np.testing.assert_allclose(dev_pred, pred, atol=1e-5, rtol=0)


def test_device_missing_vs_rest_split():
    X, y = missing_vs_rest_data()
    m = HistGradientBoostingClassifier(
        n_estimators=20, max_depth=3, allow_nan=True,
        random_state=0).fit(X[:2000], y[:2000])
    Xh, yh = X[2000:], y[2000:]
    assert (m.predict(Xh) == yh).mean() >= 0.99
    t = m.stages_[0][0]
    assert ((t.feature == 0) & np.isposinf(t.threshold)).any()
    np.testing.assert_array_equal(
        m._device_predict_fn("predict", "cuda")(Xh), m.predict(Xh))
    np.testing.assert_allclose(
        m._device_predict_fn("predict_proba", "cuda")(Xh),
        m.predict_proba(Xh), atol=1e-5, rtol=0)


def test_device_no_nan_fit_is_identical():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((1500, 5)).astype(np.float32)
    y = (X[:, 0] + X[:, 1] ** 2 > 0.5).astype(np.int64)
    # one round: both fits bin the same codes and scan the same two
    # gradient values (later rounds inherit the rounding of the f32 atomic
    # sums, which two runs of ONE configuration do not share either)
    kw = dict(n_estimators=1, random_state=3)
    a = HistGradientBoostingClassifier(**kw).fit(X, y)
    b = HistGradientBoostingClassifier(allow_nan=True, **kw).fit(X, y)
    ta, tb = trees_of(a)[0], trees_of(b)[0]
    for name in ("feature", "threshold", "left", "right"):
        np.testing.assert_array_equal(getattr(ta, name), getattr(tb, name))
    assert ta.missing_left is None and tb.missing_left is not None


def test_sklearn_forest_with_nan_scores_like_sklearn():
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(0)
    X = rng.standard_normal((800, 6)).astype(np.float32)
    y = ((X[:, 0] > 0) ^ (X[:, 2] > 0.5)).astype(np.int64)
    X = holes(X, 0.2, 1)
    y[np.isnan(X[:, 0])] = 1
    rf = RandomForestClassifier(n_estimators=6, max_depth=5,
                                random_state=0).fit(X, y)
    assert any(e.tree_.missing_go_to_left[e.tree_.feature >= 0].any()
               for e in rf.estimators_)
    ff = flat_forest_for(rf, "cuda")
    np.testing.assert_array_equal(ff.apply(X), rf.apply(X))
    np.testing.assert_allclose(ff.predict_proba(X), rf.predict_proba(X),
                               atol=1e-5, rtol=0)
