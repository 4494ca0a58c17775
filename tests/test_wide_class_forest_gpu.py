"""GPU tests of the wide-class (32 < S <= 256) tree kernels: the
class-grouped histogram, the wave-per-feature split scan, the wave-per-row
traversal, and the forest estimators on top of them.

The histogram is compared exactly (class counts are integers).  The split
scan is compared against float64 gains of the same histogram: the kernel's
pick must be a valid candidate whose float64 gain is within ``tol`` of the
best one, with

    tol = 8 * S * 2**-24        (gini),   times log2(S) for entropy.

It bounds the f32 rounding of an S-term sum of squares of exactly
represented counts (each term and each partial sum rounds by at most
2**-24 relative, and q / w**2 <= 1), with room for the handful of roundings
that turn the two impurities into a gain.
"""

import pickle
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skdist_amd import Cluster
    from skdist_amd.distribute.ensemble import (
        DistExtraTreesClassifier,
        DistRandomForestClassifier,
    )
    from skdist_amd.models.forest import (
        CRIT_ENTROPY,
        CRIT_GINI,
        BinnedDataset,
        FlatForest,
        ForestBuilder,
        HistTree,
        _feat_hashes,
        _wang_hash,
        flat_forest_for,
        hist_groups,
    )
    from skdist_amd.ops import require_hip

DEV = "cuda"
LDS_BYTES = 64 * 1024


# ---------------------------------------------------------------------- #
# 1. histogram
# ---------------------------------------------------------------------- #
def _run_hist(S, nbins, f, fg, cg, seed, skip_classes=()):
    """3000 rows in two chunks of unequal length on node slot 1 of 3 (the
    two blocks meet in the global atomics; slots 0 and 2 must stay zero).
    cg=None is the call without the trailing argument."""
    n, fp = 3000, (f + 3) // 4 * 4
    rng = np.random.default_rng(seed)
    codes = np.zeros((n, fp), dtype=np.uint8)
    codes[:, :f] = rng.integers(0, nbins, (n, f))
    allowed = np.setdiff1d(np.arange(S), np.asarray(skip_classes, dtype=int))
    y = rng.choice(allowed, n).astype(np.int32)
    y[: len(allowed)] = allowed                  # every allowed class occurs
    w = np.minimum(rng.poisson(1.0, n), 255).astype(np.uint8)
    assert (w == 0).any() and (w > 1).any()
    si = rng.permutation(n).astype(np.int32)
    chunks = np.array([[1, 0, 0, 1900], [1, 0, 1900, 1100]], dtype=np.int32)

    t = lambda a: torch.as_tensor(a, device=DEV)
    hist = torch.zeros(3, f, nbins, S, dtype=torch.float32, device=DEV)
    absent = torch.empty(0, device=DEV)
    require_hip().tree_hist(
        t(codes), t(y), absent, absent, t(w[None, :]), t(si[None, :]),
        t(chunks), hist, n, f, nbins, fg, *(() if cg is None else (cg,)))
    torch.cuda.synchronize()

    ref = np.zeros((3, f, nbins, S), dtype=np.float64)
    rows = np.repeat(si, f)
    feat = np.tile(np.arange(f), n)
    np.add.at(ref, (1, feat, codes[rows, feat], y[rows]), w[rows])
    return hist.cpu().numpy(), ref.astype(np.float32)


HIST_CASES = [
    # (S, nbins, f, fg, cg); fg = None: the builder's own (fg, cg)
    (33, 16, 12, None, None), (64, 16, 12, None, None),
    (65, 16, 12, None, None), (200, 16, 12, None, None),
    (256, 16, 12, None, None),
    (200, 256, 12, None, None), (256, 256, 12, None, None),   # cg < S
    (200, 256, 5, None, None), (256, 256, 5, None, None),     # tail group
    (200, 256, 5, 3, 21),     # g0 = 3: the byte-wise code loads; 200 % 21
    (65, 16, 12, 4, 7),       # ten class groups, the last one 2 wide
    (33, 16, 5, 3, 32),       # a 1-class tail group
    (64, 16, 12, 12, 500),    # cg past S: one group
    (33, 16, 12, 4, -1),      # -1, the default, is "not grouped"
]


@pytest.mark.parametrize("S,nbins,f,fg,cg", HIST_CASES)
def test_hist_class_groups_exact(S, nbins, f, fg, cg):
    if fg is None:
        fg, cg = hist_groups(f, nbins, S, LDS_BYTES)
        assert f < 4 or fg >= 4
        if nbins == 256:
            assert cg < S
    got, ref = _run_hist(S, nbins, f, fg, cg, seed=S + nbins + f)
    assert ref[1].sum() > 0 and (ref[1].sum(axis=(0, 1)) > 0).all()
    np.testing.assert_array_equal(got, ref)


def test_hist_ungrouped_call_is_unchanged():
    """The call without cg, at a width whose tile fits: S = 33, 16 bins."""
    got, ref = _run_hist(33, 16, 12, 4, None, seed=5)
    np.testing.assert_array_equal(got, ref)


def test_hist_class_group_without_rows():
    """Classes 16..31 never occur: class group 1 of cg = 16 adds nothing."""
    got, ref = _run_hist(70, 64, 6, 4, 16, seed=9,
                         skip_classes=range(16, 32))
    assert not ref[..., 16:32].any() and ref[..., 32:48].any()
    np.testing.assert_array_equal(got, ref)


def test_hist_rejects_bad_class_groups():
    ext = require_hip()
    t = lambda a: torch.as_tensor(a, device=DEV)
    n, f, nbins, S = 8, 4, 256, 100
    codes = torch.zeros(n, 4, dtype=torch.uint8, device=DEV)
    y = torch.zeros(n, dtype=torch.int32, device=DEV)
    yf = torch.zeros(n, dtype=torch.float32, device=DEV)
    w = torch.ones(1, n, dtype=torch.uint8, device=DEV)
    si = t(np.arange(n, dtype=np.int32)[None, :])
    chunks = t(np.array([[0, 0, 0, n]], dtype=np.int32))
    absent = torch.empty(0, device=DEV)
    hist = torch.zeros(1, f, nbins, S, device=DEV)

    def call(y_int, y_f, row_w, h, fg, *cg):
        ext.tree_hist(codes, y_int, y_f, row_w, w, si, chunks, h, n, f,
                      nbins, fg, *cg)

    with pytest.raises(RuntimeError, match="64 KiB"):
        call(y, absent, absent, hist, 1)            # 256 * 100 * 4 B
    with pytest.raises(RuntimeError, match="64 KiB"):
        call(y, absent, absent, hist, 4, 17)        # 4 * 256 * 17 * 4 B
    with pytest.raises(RuntimeError, match="cg must be > 0"):
        call(y, absent, absent, hist, 4, 0)
    h3 = torch.zeros(1, f, nbins, 3, device=DEV)
    with pytest.raises(RuntimeError, match="class counts only"):
        call(absent, yf, absent, h3, 4, 2)
    h4 = torch.zeros(1, f, nbins, 4, device=DEV)
    with pytest.raises(RuntimeError):
        call(absent, yf, yf, h4, 4, 2)
    torch.cuda.synchronize()
    assert not hist.any()                           # nothing was launched
    call(y, absent, absent, hist, 4, 16)
    assert float(hist.sum()) == n * f


# ---------------------------------------------------------------------- #
# 2. split scan
# ---------------------------------------------------------------------- #
def _tol(S, crit):
    return 8 * S * 2.0 ** -24 * (np.log2(S) if crit == CRIT_ENTROPY else 1.0)


def _node_hist(rng, f, nbins, S, m, informative=0.6, top_bin=None):
    """[f, nbins, S] class counts of m rows with Poisson(1) weights: a
    feature's code follows the row's class with probability `informative`,
    else it is random, so features and cuts differ in gain.  top_bin: the
    number of usable bins (the rest stay empty)."""
    nb = top_bin or nbins
    y = rng.integers(0, S, m)
    w = np.minimum(rng.poisson(1.0, m), 255)
    H = np.zeros((f, nbins, S))
    for j in range(f):
        centre = rng.permutation(S)[y] * nb // S
        code = np.where(rng.random(m) < informative * rng.random(),
                        centre, rng.integers(0, nb, m))
        np.add.at(H[j], (code, y), w)
    return H


def _extra_bins(H, seed, sel):
    """Per feature the eager mirror's hashed bin (-1: no candidate)."""
    f = H.shape[0]
    out = np.full(f, -1)
    occupied = H.sum(axis=2) > 0
    for j in np.flatnonzero(sel):
        occ = np.flatnonzero(occupied[j])
        if len(occ) < 2:
            continue
        lo, hi = int(occ[0]), int(occ[-1])
        with np.errstate(over="ignore"):
            r = int(_wang_hash(np.uint32(seed) ^ np.uint32(0x9E3779B9)
                               ^ np.uint32((j * 40503) % (1 << 32))))
        out[j] = lo + r % (hi - lo)
    return out


def _ref_split(H, crit, min_leaf, sel, extra_bins=None, missing=False):
    """float64 view of one node: gain [f, nbins-1, D] over (feature, bin,
    direction R/L), -inf where the candidate is not valid."""
    f, nbins, S = H.shape
    parent = H[0].sum(axis=0)
    wp = parent.sum()

    def imp(s, w):
        with np.errstate(divide="ignore", invalid="ignore"):
            if crit == CRIT_GINI:
                r = 1.0 - (s ** 2).sum(axis=-1) / (w * w)
            else:
                p = s / np.asarray(w)[..., None]
                r = -(np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)),
                               0.0)).sum(axis=-1)
        return np.where(np.asarray(w) > 0, r, 0.0)

    imp_p = float(imp(parent, wp))
    cum = H.cumsum(axis=1)[:, :-1]
    left = cum[:, :, None, :]
    wm = H[:, -1].sum(axis=-1)
    if missing:
        left = np.concatenate([left, left + H[:, -1][:, None, None, :]],
                              axis=2)
    wl = left.sum(axis=-1)
    wr = wp - wl
    gain = imp_p - (wl * imp(left, wl) + wr * imp(parent - left, wr)) / wp
    valid = (wl >= min_leaf) & (wr >= min_leaf) & sel[:, None, None]
    if missing:
        valid[:, :, 1] &= (wm > 0)[:, None]
    if extra_bins is not None:
        valid &= (np.arange(nbins - 1)[None, :]
                  == extra_bins[:, None])[:, :, None]
    gain = np.where(valid, gain, -np.inf)
    return dict(parent=parent, wp=wp, imp=imp_p, gain=gain, wl=wl,
                left=left, wm=wm)


def _run_split(H, crit, min_leaf, m_features, extra, seeds, missing=False,
               is_cls=1, cnt_stat=-1):
    NF, f, nbins, S = H.shape
    hist = torch.as_tensor(np.ascontiguousarray(H, dtype=np.float32),
                           device=DEV)
    seed = torch.as_tensor(np.asarray(seeds, dtype=np.uint32).view(np.int32),
                           device=DEV)
    oi = lambda: torch.full((NF,), -7, dtype=torch.int32, device=DEV)
    of = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=DEV)
    out = (oi(), oi(), of(NF), of(NF), of(NF), of(NF, S), of(NF, S))
    mleft = oi()
    require_hip().tree_split(
        hist, seed, f, nbins, S, is_cls, crit, m_features, int(extra),
        float(min_leaf), *out, cnt_stat, *((1, mleft) if missing else ()))
    torch.cuda.synchronize()
    names = ("feat", "bin", "wl", "gain", "imp", "stats", "lstats")
    got = {k: o.cpu().numpy() for k, o in zip(names, out)}
    got["mleft"] = mleft.cpu().numpy()
    return got


def _check_split(H, crit, min_leaf, m_features, extra, seeds,
                 missing=False):
    """Every node of H against its float64 view; returns the per-node
    (ref, feat, bin, direction) for further assertions."""
    NF, f, nbins, S = H.shape
    assert H.max() < 2 ** 24 and np.array_equal(H, np.round(H))
    got = _run_split(H, crit, min_leaf, m_features, extra, seeds, missing)
    tol = _tol(S, crit)
    picks = []
    for k in range(NF):
        where = f"node {k}"
        sel = np.ones(f, dtype=bool)
        if m_features < f:
            hv = _feat_hashes(int(seeds[k]), f)
            sel = hv <= np.sort(hv)[m_features - 1]
            assert sel.sum() == m_features
        eb = _extra_bins(H[k], int(seeds[k]), sel) if extra else None
        ref = _ref_split(H[k], crit, min_leaf, sel, eb, missing)
        best = ref["gain"].max()
        np.testing.assert_array_equal(got["stats"][k], ref["parent"], where)
        assert abs(got["imp"][k] - ref["imp"]) <= tol, where
        jf, jb = int(got["feat"][k]), int(got["bin"][k])
        if not best > 0:
            assert jf == -1, where
            assert not got["lstats"][k].any(), where
            picks.append((ref, -1, -1, 0))
            continue
        # the data of this test keeps real splits clear of the noise floor
        assert best > 4 * tol, (where, best)
        assert 0 <= jf < f and 0 <= jb < nbins - 1, (where, jf, jb)
        assert sel[jf], (where, "feature outside the hashed subsample")
        if extra:
            assert jb == eb[jf], (where, "not the hashed bin")
        d = 0
        if missing:
            ml = int(got["mleft"][k])
            if ref["wm"][jf] > 0:
                d = ml                           # the learned direction
            else:                                # the majority side
                assert ml == int(2 * ref["wl"][jf, jb, 0] > ref["wp"]), where
        g64 = ref["gain"][jf, jb, d]
        assert np.isfinite(g64), (where, "not a valid candidate", jf, jb, d)
        assert g64 >= best - tol, (where, g64, best)
        np.testing.assert_array_equal(got["lstats"][k], ref["left"][jf, jb, d],
                                      where)
        assert got["wl"][k] == ref["wl"][jf, jb, d], where
        assert abs(got["gain"][k] - g64) <= tol, (where, got["gain"][k], g64)
        picks.append((ref, jf, jb, d))
    return picks


def _split_nodes(S, f, nbins, seed):
    """Six random nodes, a pure node and a three-row node."""
    rng = np.random.default_rng(seed)
    nodes = [_node_hist(rng, f, nbins, S, m) for m in (3000, 2000, 1500,
                                                       1000, 700, 400)]
    pure = np.zeros((f, nbins, S))
    pure[:, :, S - 1] = rng.multinomial(500, np.ones(nbins) / nbins, f)
    tiny = np.zeros((f, nbins, S))
    for c, b in ((0, 1), (S // 2, 5), (S - 1, 9)):
        tiny[:, b, c] = 1
    return np.stack(nodes + [pure, tiny])


@pytest.mark.parametrize("crit", [0, 1], ids=["gini", "entropy"])
@pytest.mark.parametrize("S", [33, 65, 256])
@pytest.mark.parametrize("f", [3, 70])
def test_split_wide_matches_float64(f, S, crit):
    H = _split_nodes(S, f, 16, seed=S * 100 + f)
    seeds = 1000 + 77 * np.arange(len(H))
    picks = _check_split(H, crit, 1.0, f, False, seeds)
    assert [p[1] for p in picks[-2:-1]] == [-1]          # the pure node
    assert all(p[1] >= 0 for p in picks[:-2])


@pytest.mark.parametrize("crit", [0, 1], ids=["gini", "entropy"])
@pytest.mark.parametrize("S", [33, 256])
def test_split_wide_feature_subsample(S, crit):
    """m_features < f: the same node under 12 seeds; each pick lies in its
    seed's hashed subsample and is the best one there."""
    f, m = 70, 8
    rng = np.random.default_rng(S)
    H = np.repeat(_node_hist(rng, f, 16, S, 2500)[None], 12, axis=0)
    seeds = rng.integers(0, 2 ** 32, 12, dtype=np.uint64)
    picks = _check_split(H, crit, 1.0, m, False, seeds)
    assert len({p[1] for p in picks}) > 3       # the subsample moves the pick


@pytest.mark.parametrize("S", [33, 65, 256])
@pytest.mark.parametrize("f", [3, 70])
def test_split_wide_min_leaf(f, S):
    """min_leaf = 400 weighted rows: the outer cuts of the larger nodes and
    every cut of the nodes under 800 rows are invalid."""
    H = _split_nodes(S, f, 16, seed=S * 7 + f)
    seeds = 5 + np.arange(len(H))
    ref = _ref_split(H[0], CRIT_GINI, 400.0, np.ones(f, dtype=bool))
    assert np.isinf(ref["gain"]).any() and np.isfinite(ref["gain"]).any()
    picks = _check_split(H, CRIT_GINI, 400.0, f, False, seeds)
    assert [p[1] >= 0 for p in picks] == [True] * 4 + [False] * 4


@pytest.mark.parametrize("crit", [0, 1], ids=["gini", "entropy"])
@pytest.mark.parametrize("S,f", [(33, 70), (65, 3), (256, 70)])
def test_split_wide_extra_mode(S, f, crit):
    """ExtraTrees: one hashed bin per feature in its occupied range; four
    bins stay empty so the range is not the whole axis."""
    rng = np.random.default_rng(S + f)
    H = np.stack([_node_hist(rng, f, 16, S, m, top_bin=12)
                  for m in (3000, 1500, 800, 300)])
    H = np.roll(H, 2, axis=2)                   # occupied bins 2..13
    const = np.zeros_like(H[0])
    const[:, 7, :] = H[0].sum(axis=1)           # one occupied bin: no cut
    H = np.concatenate([H, const[None]])
    seeds = 31 * np.arange(1, len(H) + 1)
    picks = _check_split(H, crit, 1.0, f, True, seeds)
    assert picks[-1][1] == -1 and picks[0][1] >= 0
    _check_split(H, crit, 1.0, min(f, 2), True, seeds)


@pytest.mark.parametrize("extra", [False, True], ids=["best", "extra"])
def test_split_wide_exact_ties_take_lowest_feature(extra):
    """All 70 features carry one and the same histogram (four of its bins
    empty), so candidates with equal left stats have exactly equal gains in
    any arithmetic: among them the kernel must return the lowest feature of
    the node's hashed subsample, and the lowest bin.  Deep nodes of
    separable classes are full of such ties."""
    f, m, S = 70, 3, 40
    rng = np.random.default_rng(70)
    one = np.roll(_node_hist(rng, 1, 16, S, 1500, top_bin=12), 2, axis=1)
    one[0, 6] = 0                                # an empty bin inside
    H = np.repeat(np.repeat(one, f, axis=0)[None], 12, axis=0)
    seeds = rng.integers(0, 2 ** 32, 12, dtype=np.uint64)
    picks = _check_split(H, CRIT_GINI, 1.0, m, extra, seeds)
    firsts = set()
    for (ref, jf, jb, _), seed in zip(picks, seeds):
        tied = np.flatnonzero(np.isfinite(ref["gain"][:, jb, 0]))
        assert len(tied) == (m if not extra else len(tied)) and jf in tied
        assert jf == tied.min(), (jf, tied)
        if not extra and jb > 0:                 # not after an empty bin
            assert ref["wl"][jf, jb, 0] > ref["wl"][jf, jb - 1, 0]
        firsts.add(int(jf))
    # the subsample's lowest feature falls into every wave's range
    assert len({j * 4 // f for j in firsts}) > 1 or extra


def _missing_node(rng, kind, S=40, nbins=16, m=1600):
    """Two features over 15 present bins and the missing bin 15.  The
    classes below S/2 sit in bins 0..6 of the informative feature, the rest
    in bins 8..14; the other feature is noise.
      L / R:         feature 0 informative, a fifth of the rows of its left
                     / right classes missing; feature 1 has nothing missing
      majL / majR:   feature 1 informative with nothing missing and 70 % of
                     the rows on its left / right; noisy feature 0 has
                     missing rows"""
    heavy_left = kind in ("L", "majL")
    p_left = 0.7 if kind.startswith("maj") else 0.5
    side = rng.random(m) < (p_left if heavy_left else 1 - p_left)
    y = np.where(side, rng.integers(0, S // 2, m),
                 rng.integers(S // 2, S, m))
    info = np.where(side, rng.integers(0, 7, m), rng.integers(8, 15, m))
    noise = rng.integers(0, 15, m)
    if kind in ("L", "R"):
        gone = (side == (kind == "L")) & (rng.random(m) < 0.2)
        codes = [np.where(gone, 15, info), noise]
    else:
        codes = [np.where(rng.random(m) < 0.1, 15, noise), info]
    w = np.minimum(rng.poisson(1.0, m), 255)
    H = np.zeros((2, nbins, S))
    for j in range(2):
        np.add.at(H[j], (codes[j], y), w)
    return H


@pytest.mark.parametrize("crit", [0, 1], ids=["gini", "entropy"])
def test_split_wide_missing_directions(crit):
    rng = np.random.default_rng(40)
    kinds = ("L", "R", "majL", "majR")
    H = np.stack([_missing_node(rng, k) for k in kinds])
    assert H[:2, 0, 15].any() and not H[:2, 1, 15].any()
    got = _run_split(H, crit, 1.0, 2, False, [1, 2, 3, 4], missing=True)
    picks = _check_split(H, crit, 1.0, 2, False, [1, 2, 3, 4], missing=True)
    # learned: the missing rows rejoin their classes
    assert [p[1] for p in picks] == [0, 0, 1, 1]
    assert list(got["mleft"]) == [1, 0, 1, 0]
    assert picks[0][3] == 1 and picks[1][3] == 0


def test_split_wide_single_best_cut():
    """Hand-built: 40 classes x 16 rows; every feature spreads each class
    evenly over the bins except feature 3, which keeps classes 0..19 in bins
    0..6 and the others in bins 7..15: (3, 6) is the one perfect cut."""
    f, nbins, S = 5, 16, 40
    H = np.ones((f, nbins, S))
    H[3] = 0
    for c in range(S):
        bins = np.arange(16) % 7 if c < 20 else 7 + np.arange(16) % 9
        np.add.at(H[3, :, c], bins, 1)
    assert (H.sum(axis=1) == 16).all()
    for crit in (CRIT_GINI, CRIT_ENTROPY):
        got = _run_split(H[None], crit, 1.0, f, False, [11])
        assert (got["feat"][0], got["bin"][0]) == (3, 6)
        assert got["wl"][0] == 320.0
        child = 1 - 1 / 20 if crit == CRIT_GINI else np.log2(20)
        parent = 1 - 1 / 40 if crit == CRIT_GINI else np.log2(40)
        assert abs(got["imp"][0] - parent) <= _tol(S, crit)
        assert abs(got["gain"][0] - (parent - child)) <= _tol(S, crit)
        _check_split(H[None], crit, 1.0, f, False, [11])


@pytest.mark.parametrize("S,is_cls,cnt_stat", [(257, 1, -1), (40, 0, -1),
                                               (40, 1, 3)])
def test_split_wide_guards(S, is_cls, cnt_stat):
    H = np.ones((2, 3, 16, S))
    with pytest.raises(RuntimeError, match="tree_split"):
        _run_split(H, CRIT_GINI, 1.0, 3, False, [1, 2], is_cls=is_cls,
                   cnt_stat=cnt_stat)


# ---------------------------------------------------------------------- #
# the 100-blob data shared by the builder, predict and estimator tests
# ---------------------------------------------------------------------- #
def _blobs(n=4000, f=10, k=100, seed=0):
    """k unit-variance Gaussian blobs with centres drawn uniformly from
    [0, 40]^f, any two at least 10 sigma apart.  The centres are in general
    position on purpose: on a grid every feature takes a few values only, all
    features offer the same few cuts, and with equal class sizes their gains
    tie to within 1 / w**2 — f32 and f64 then pick different features."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.0, 40.0, (k, f))
    gaps = np.linalg.norm(centres[:, None] - centres[None], axis=2)
    assert gaps[~np.eye(k, dtype=bool)].min() >= 10.0
    y = rng.permutation(np.arange(n) % k)
    X = (centres[y] + rng.standard_normal((n, f))).astype(np.float32)
    return X, y.astype(np.int64)


@pytest.fixture(scope="module")
def blobs():
    return _blobs()


@pytest.fixture(scope="module")
def blob_forest(blobs):
    """Eight device-built trees on the blobs (built once, never changed)."""
    X, y = blobs
    ds = BinnedDataset(X, y, DEV, is_cls=True)
    b = ForestBuilder(ds, "gini", max_features="sqrt", bootstrap=True,
                      tree_batch=8, engine="hip")
    assert b.cg is not None and b.cg < 100 and b.fg >= 4
    trees = b.build(list(range(8)))
    assert all(t.value.shape[1] == 100 for t in trees)
    return trees


def _host_mean(trees, X):
    """The estimator's host path: f32 payloads summed in tree order."""
    p = None
    for t in trees:
        q = t.predict_proba(X)
        p = q if p is None else p + q
    return p / len(trees)


# ---------------------------------------------------------------------- #
# 4. builder: HIP against the eager mirror
# ---------------------------------------------------------------------- #
@pytest.mark.parametrize("extra_mode", [False, True], ids=["best", "extra"])
def test_hip_builder_matches_eager_100_classes(blobs, extra_mode,
                                               monkeypatch):
    monkeypatch.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
    X, y = blobs
    ds = BinnedDataset(X, y, DEV, is_cls=True)
    assert ds.S == 100
    kw = dict(max_depth=8, max_features="sqrt", bootstrap=True,
              tree_batch=4, extra_mode=extra_mode)
    th = ForestBuilder(ds, "gini", engine="hip", **kw).build([3, 17, 42])
    te = ForestBuilder(ds, "gini", engine="eager", **kw).build([3, 17, 42])
    for a, b in zip(th, te):
        pa, pb = a.predict(X), b.predict(X)
        assert (pa == pb).mean() > 0.99, (a.node_count, b.node_count)
        assert abs(a.node_count - b.node_count) <= 0.1 * b.node_count


# ---------------------------------------------------------------------- #
# 5. traversal
# ---------------------------------------------------------------------- #
def test_flat_forest_wide_matches_host(blobs, blob_forest):
    X, _ = blobs
    trees = blob_forest
    ff = FlatForest(trees, DEV)
    assert ff.vs == 100
    host = _host_mean(trees, X)
    dev = ff.predict_proba(X)
    assert dev.shape == (len(X), 100)
    np.testing.assert_allclose(dev, host, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(ff.predict(X),
                                  trees[0].classes_[host.argmax(axis=1)])
    np.testing.assert_array_equal(
        ff.apply(X), np.column_stack([t.apply(X) for t in trees]))
    # CSR rows: the same walk and the same accumulation order -> same bits
    Xs = sp.csr_matrix(X)
    dev_s = ff.predict_proba(Xs)
    assert np.array_equal(dev_s.view(np.uint32), dev.view(np.uint32))
    np.testing.assert_array_equal(ff.predict(Xs), ff.predict(X))
    np.testing.assert_array_equal(ff.apply(Xs), ff.apply(X))


def _random_tree(rng, f, vs, max_depth):
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


@pytest.mark.parametrize("vs", [33, 65, 256])
@pytest.mark.parametrize("n_trees", [1, 9])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_wide_traversal_synthetic(rows, n_trees, vs):
    """Synthetic trees with payloads k/64 (exact sums): 4 rows per block, so
    5 and 257 rows end in a block with one row.  With missing_left flags
    and NaN cells the _m instantiations run, without them the plain ones;
    dense and CSR give the same bits."""
    f = 9
    rng = np.random.default_rng(rows * 1000 + n_trees * 10 + vs)
    trees = [_random_tree(rng, f, vs, int(rng.integers(1, 7)))
             for _ in range(n_trees)]
    X = np.round(rng.standard_normal((rows, f)) * 4) / 4
    X[rng.random(X.shape) < 0.2] = np.nan
    X[0, :] = np.nan
    Xs = sp.csr_matrix(X)
    assert np.isnan(Xs.data).sum() == np.isnan(X).sum()
    bare = [HistTree(t.feature, t.threshold, t.left, t.right, t.value, None,
                     f, None) for t in trees]
    for forest in (trees, bare):
        ff = FlatForest(forest, DEV)
        assert (ff.mleft is not None) == (forest is trees)
        host = np.mean([t.predict_proba(X).astype(np.float64)
                        for t in forest], axis=0)
        pd, ps = ff.predict_value(X), ff.predict_value(Xs)
        assert pd.shape == (rows, vs)
        np.testing.assert_allclose(pd, host, rtol=0, atol=1e-5)
        assert np.array_equal(pd.view(np.uint32), ps.view(np.uint32))
        ids = np.column_stack([t.apply(X) for t in forest])
        np.testing.assert_array_equal(ff.apply(X), ids)
        np.testing.assert_array_equal(ff.apply(Xs), ids)


def test_wide_traversal_rejects_257_values():
    t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=DEV)
    X = torch.zeros(5, 2, device=DEV)
    nodes = (t([0, -1, -1], torch.int32), t([0.0, 0.0, 0.0], torch.float32),
             t([1, 0, 1], torch.int32), t([2, 0, 0], torch.int32),
             t([0], torch.int32))
    values = torch.zeros(2, 257, device=DEV)
    out = torch.empty(5, 257, device=DEV)
    with pytest.raises(RuntimeError, match="vs <= 256"):
        require_hip().forest_predict(X, *nodes, values, out)


def test_sklearn_forest_40_classes_on_device(blobs):
    from sklearn.ensemble import RandomForestClassifier

    X, y = blobs
    keep = y < 40
    X, y = X[keep], y[keep]
    rf = RandomForestClassifier(n_estimators=10, max_depth=6,
                                random_state=0).fit(X, y)
    assert len(rf.classes_) == 40
    assert flat_forest_for(rf, "cpu") is None
    ff = flat_forest_for(rf, DEV)
    assert ff is not None and ff.vs == 40
    np.testing.assert_allclose(ff.predict_proba(X), rf.predict_proba(X),
                               rtol=0, atol=1e-5)


# ---------------------------------------------------------------------- #
# 6. estimators
# ---------------------------------------------------------------------- #
@pytest.mark.parametrize("kind", ["rf", "extra"])
def test_dist_forest_100_classes_end_to_end(blobs, kind):
    from sklearn.ensemble import RandomForestClassifier

    X, y = blobs
    Xtr, Xte, ytr, yte = X[:3000], X[3000:], y[:3000], y[3000:]
    assert len(np.unique(ytr)) == 100
    Est = DistRandomForestClassifier if kind == "rf" \
        else DistExtraTreesClassifier
    clf = Est(sc=Cluster(require_gpu=True), n_estimators=16, random_state=0)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        clf.fit(Xtr, ytr)
    assert not any("falling back" in str(r.message) for r in rec)
    assert all(isinstance(t, HistTree) for t in clf.estimators_)
    proba = clf.predict_proba(Xte)
    assert proba.shape == (len(Xte), 100)
    np.testing.assert_allclose(proba.sum(axis=1), 1.0, atol=1e-5)
    clf2 = pickle.loads(pickle.dumps(clf))
    np.testing.assert_array_equal(clf2.predict_proba(Xte), proba)
    np.testing.assert_array_equal(clf2.predict(Xte), clf.predict(Xte))

    ref = RandomForestClassifier(n_estimators=16, random_state=0)
    ref.fit(Xtr, ytr)
    acc_ref = (ref.predict(Xte) == yte).mean()
    acc = (clf.predict(Xte) == yte).mean()
    print(f"held-out accuracy: device {kind} {acc:.4f}, sklearn {acc_ref:.4f}")
    assert acc_ref > 0.97, acc_ref          # the blobs are separable
    assert acc >= acc_ref - 0.03, (acc, acc_ref)


def test_dist_forest_100_classes_oob_warm_start_class_weight(blobs):
    X, y = blobs
    Xtr, ytr = X[:3000], y[:3000]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        clf = DistRandomForestClassifier(
            sc=Cluster(require_gpu=True), n_estimators=16, oob_score=True,
            random_state=0).fit(Xtr, ytr)
        assert 0.0 < clf.oob_score_ <= 1.0
        assert clf.oob_decision_function_.shape == (3000, 100)

        ws = DistRandomForestClassifier(
            sc=Cluster(require_gpu=True), n_estimators=8, warm_start=True,
            random_state=0).fit(Xtr, ytr)
        ws.set_params(n_estimators=12, sc=Cluster(require_gpu=True))
        ws.fit(Xtr, ytr)
        assert len(ws.estimators_) == 12

        cw = DistRandomForestClassifier(
            sc=Cluster(require_gpu=True), n_estimators=8,
            class_weight="balanced", random_state=0).fit(Xtr, ytr)
    assert not any("falling back" in str(r.message) for r in rec)
    for m in (clf, ws, cw):
        assert all(isinstance(t, HistTree) for t in m.estimators_)
        assert (m.predict(X[3000:]) == y[3000:]).mean() > 0.9
