"""GPU tests: UTF-8 hashing-vectorizer kernel vs sklearn on Unicode text.

Reference everywhere: sklearn's HashingVectorizer.  Criterion as in
tests/test_hash_gpu.py: identical shape and abs(out - ref).max() < 1e-12;
with norm=None additionally identical indices, indptr and data.
"""

import random

import numpy as np
import pytest
from sklearn.feature_extraction.text import HashingVectorizer

pytestmark = pytest.mark.gpu

# every document is here for one specific way the kernel can go wrong
CORPUS = [
    # byte width against character count
    "é",                        # 2 bytes, 1 character: not a token
    "éa",                       # 2 characters: a token
    "日 本",                    # two 1-character runs: no tokens
    "日本",                     # one token
    "𝒳",                        # lone 4-byte letter
    "𝒳𝒳",                       # two of them: a token
    # word class outside ASCII
    "٣٤ ٣",                     # Arabic-Indic digits
    "x² y",                     # superscript two is \w
    "½a ½",                     # vulgar fraction is \w
    "Ⅷi Ⅷ",                     # Roman numeral (lowercases to ⅷ)
    "日本語のテキスト 中文字符",  # CJK
    "привет мир снова привет",  # Cyrillic
    "naïve_é _日_ é_ _é",       # underscore next to non-ASCII letters
    # non-word characters
    "alpha—beta – gamma",       # em-dash, en-dash
    "“quoted” ‘single’ it’s",   # curly quotes
    "¿qué? 100€ €uro",
    "smile😀face 😀 ab😀",        # 4-byte non-word between letters
    "zero\u200dwidth soft\xadhyphen",  # ZWJ, soft hyphen inside a word
    "İstanbul İİ",              # lower() produces i + U+0307
    # host lowercasing
    "ÉCOLE École",
    "ΟΔΟΣ ΟΔΟΣ.",               # final sigma
    "STRASSE Straße ǅ",
    # whitespace
    "nb\xa0sp em\u2003sp cjk\u3000sp nel\u0085x ls\u2028y",
    "a\x1fbb é",                # ASCII separator in a non-ASCII document
    "é\xa0\u2003 \u3000\t\u2028b  \u205f\u1680cc\u202f",  # mixed runs
    "\xa0\u3000",             # whitespace only
    "tab\tnew\nline\rcr\x0bvt\x0cff\x1cfs\x1dgs\x1ers é",
    # edges
    "",
    "😀😀 😀",                    # emoji only
    "ends with 日本語",          # non-ASCII token at document end
    "ends with é",              # 1-character run at document end
    "𝒳" * 40,                   # one word of 40 four-byte letters
    "日本",                     # char_wb with n > word length (multi-byte)
    "é b 日",                   # 1-character words
    "über straße ñandú çedilla ångström",
    "mixed ASCII words and 日本語 tokens and more ascii",
    "a1 b2 c3 _ __ ___ 9",
    "plain ascii document in a mixed chunk",
    "e\u0301 combining acute cafe\u0301",
    "ﬁnance ﬂow ǆ",             # ligatures
]

ASCII_DOCS = [
    "The quick brown fox jumps over the lazy dog",
    "a ab abc abcd _under_score_ 1234 mixedCASE Token99",
    "",
    "   leading and trailing   spaces   ",
    "punctuation, should; split: tokens! right? (yes) [ok] {fine}",
    "tabs\tand\nnew\rlines\x0bmix\x0c end",
]

CASES = [
    dict(analyzer="word", ngram_range=(1, 1), alternate_sign=False),
    dict(analyzer="word", ngram_range=(1, 2), alternate_sign=False),
    dict(analyzer="word", ngram_range=(2, 3), alternate_sign=False),
    dict(analyzer="word", ngram_range=(1, 3), norm=None),
    dict(analyzer="word", ngram_range=(1, 2), binary=True),
    dict(analyzer="word", ngram_range=(1, 2), n_features=4096),
    dict(analyzer="char_wb", ngram_range=(2, 5)),
    dict(analyzer="char_wb", ngram_range=(3, 4)),
    dict(analyzer="char_wb", ngram_range=(1, 3), norm=None),
]


def _id(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items()).replace(" ", "")


def _device(docs, kw):
    from skdist_amd.ops import hash_vectorize

    return hash_vectorize(
        docs,
        n_features=kw.get("n_features", 2 ** 20),
        analyzer=kw.get("analyzer", "word"),
        ngram_range=kw.get("ngram_range", (1, 1)),
        alternate_sign=kw.get("alternate_sign", True),
        binary=kw.get("binary", False),
        norm=kw.get("norm", "l2"),
    )


def _assert_same(out, ref, exact):
    assert out.shape == ref.shape
    d = out - ref
    assert (abs(d).max() if d.nnz else 0.0) < 1e-12
    if exact:
        out = out.tocsr()
        ref = ref.tocsr()
        out.sort_indices()
        ref.sort_indices()
        assert np.array_equal(out.indptr, ref.indptr)
        assert np.array_equal(out.indices, ref.indices)
        assert np.array_equal(out.data, ref.data)


def _check(docs, kw):
    ref = HashingVectorizer(**kw).transform(docs)
    out = _device(docs, kw)
    _assert_same(out, ref, exact=kw.get("norm", "l2") is None)


@pytest.mark.parametrize("kw", CASES, ids=_id)
def test_corpus_matches_sklearn(kw):
    _check(CORPUS, kw)


@pytest.mark.parametrize("kw", CASES, ids=_id)
def test_corpus_per_document(kw):
    # one launch, but a mismatch names the document
    ref = HashingVectorizer(**kw).transform(CORPUS).tocsr()
    out = _device(CORPUS, kw).tocsr()
    bad = [
        CORPUS[i] for i in range(len(CORPUS))
        if abs(out[i] - ref[i]).sum() >= 1e-12
    ]
    assert bad == []


@pytest.mark.parametrize("kw", CASES, ids=_id)
def test_several_blocks(kw):
    docs = CORPUS * 8  # > 256 documents: more than one block
    assert len(docs) > 256
    _check(docs, kw)


@pytest.mark.parametrize("kw", CASES, ids=_id)
def test_ascii_chunk_and_mixed_chunk(kw):
    assert all(d.isascii() for d in ASCII_DOCS)
    _check(ASCII_DOCS, kw)               # routed to the ASCII kernel
    _check(ASCII_DOCS + CORPUS[:12], kw)  # routed to the UTF-8 kernel


# pool: several code points per (class x UTF-8 width) cell, uppercase
# included; classes are word / whitespace / other
_POOL = {
    ("word", 1): "abzAZ09_",
    ("word", 2): "éÉñßΣσяЖ٣²",
    ("word", 3): "日本語あ한Ⅷⅷ",
    ("word", 4): "𝒳𝒴𐐀𐐨𠀀",
    ("space", 1): " \t\n\x1c\x1f",
    ("space", 2): "\u0085\xa0",
    ("space", 3): "\u1680\u2003\u2028\u202f\u3000",
    ("other", 1): ".,-!'",
    ("other", 2): "¿«\xad\u0301\u0307",
    ("other", 3): "—“”€\u200d",
    ("other", 4): "😀🙂🎉",
}


def _fuzz_docs():
    rng = random.Random(20240607)
    cells = sorted(_POOL)
    docs = []
    for _ in range(200):
        n = rng.randint(0, 60)
        chars = []
        for _ in range(n):
            cls = rng.choices(["word", "space", "other"], [6, 2, 1])[0]
            width = rng.choice([w for c, w in cells if c == cls])
            chars.append(rng.choice(_POOL[(cls, width)]))
        docs.append("".join(chars))
    return docs


def test_fuzz_pool_is_what_it_claims():
    import re

    for (cls, width), chars in _POOL.items():
        for ch in chars:
            assert len(ch.encode("utf-8")) == width, (cls, width, ch)
            got = ("word" if re.fullmatch(r"\w", ch) else
                   "space" if ch.isspace() else "other")
            assert got == cls, (cls, width, hex(ord(ch)))


@pytest.mark.parametrize("kw", [
    dict(analyzer="word", ngram_range=(1, 2), norm=None),
    dict(analyzer="char_wb", ngram_range=(2, 4), norm=None),
], ids=_id)
def test_seeded_fuzz(kw):
    docs = _fuzz_docs()
    assert len(docs) == 200
    _check(docs, kw)


def _overflow_docs():
    return ["short doc", "日" * 300 + " 本語", "after the long one é"]


def test_overflow_raises():
    from skdist_amd.ops import (
        GRAM_MAX_BYTES, HashGramOverflow, hash_vectorize,
    )

    docs = _overflow_docs()
    assert len(docs[1].split()[0].encode("utf-8")) > GRAM_MAX_BYTES
    with pytest.raises(ValueError, match=str(GRAM_MAX_BYTES)) as ei:
        hash_vectorize(docs, analyzer="word", ngram_range=(1, 2))
    assert isinstance(ei.value, HashGramOverflow)
    # the unigram path hashes from the document buffer: no limit
    _check(docs, dict(analyzer="word", ngram_range=(1, 1), norm=None))


def test_overflow_chunk_falls_back_to_sklearn():
    from skdist_amd.preprocessing import HashingVectorizerChunked

    docs = _overflow_docs()
    v = HashingVectorizerChunked(ngram_range=(1, 2))
    assert v._try_device_transform(docs) is None
    out = v.transform(np.asarray(docs, dtype=object))
    ref = HashingVectorizer(ngram_range=(1, 2)).transform(docs)
    _assert_same(out, ref, exact=False)


def test_public_interface_takes_device_path():
    from skdist_amd.preprocessing import HashingVectorizerChunked

    v = HashingVectorizerChunked(ngram_range=(1, 2))
    assert v._try_device_transform(CORPUS) is not None
    out = v.transform(np.asarray(CORPUS, dtype=object))
    ref = HashingVectorizer(ngram_range=(1, 2)).transform(CORPUS)
    _assert_same(out, ref, exact=False)
    # chunked: the ASCII chunk and the mixed chunks take different kernels
    docs = ASCII_DOCS + CORPUS
    v = HashingVectorizerChunked(chunksize=len(ASCII_DOCS),
                                 analyzer="char_wb", ngram_range=(2, 4))
    out = v.transform(np.asarray(docs, dtype=object))
    ref = HashingVectorizer(analyzer="char_wb",
                            ngram_range=(2, 4)).transform(docs)
    _assert_same(out, ref, exact=False)


@pytest.mark.parametrize("strip", ["unicode", "ascii"])
@pytest.mark.parametrize("analyzer,ngram_range",
                         [("word", (1, 2)), ("char_wb", (2, 4))])
def test_strip_accents(strip, analyzer, ngram_range):
    from skdist_amd.preprocessing import HashingVectorizerChunked

    kw = dict(strip_accents=strip, analyzer=analyzer,
              ngram_range=ngram_range, norm=None)
    docs = CORPUS
    if analyzer == "char_wb":
        # strip_accents="ascii" leaves a pure-ASCII chunk, which takes the
        # ASCII kernel; its char_wb whitespace set lacks U+001C..U+001F
        # (known deviation of that kernel, docs/PARITY.md), so the
        # documents with those separators are checked under "word" only
        docs = [d for d in CORPUS
                if not any("\x1c" <= ch <= "\x1f" for ch in d)]
        assert len(docs) == len(CORPUS) - 2
    v = HashingVectorizerChunked(**kw)
    assert v._try_device_transform(docs) is not None
    out = v.transform(np.asarray(docs, dtype=object))
    ref = HashingVectorizer(**kw).transform(docs)
    _assert_same(out, ref, exact=True)


def test_lone_surrogate_keeps_sklearn_path():
    from skdist_amd.ops import hash_vectorize
    from skdist_amd.preprocessing import HashingVectorizerChunked

    docs = ["fine é", "bad \ud83d doc"]
    with pytest.raises(UnicodeEncodeError):
        hash_vectorize(docs)
    assert HashingVectorizerChunked()._try_device_transform(docs) is None


def test_lowercase_false():
    from skdist_amd.preprocessing import HashingVectorizerChunked

    kw = dict(lowercase=False, ngram_range=(1, 2), norm=None)
    out = HashingVectorizerChunked(**kw).transform(
        np.asarray(CORPUS, dtype=object))
    ref = HashingVectorizer(**kw).transform(CORPUS)
    _assert_same(out, ref, exact=True)


def test_encoderizer_unicode_text(monkeypatch):
    import pandas as pd

    import skdist_amd.ops as ops
    from skdist_amd.distribute.encoder import Encoderizer

    df = pd.DataFrame({
        "txt": CORPUS,
        "num": np.arange(len(CORPUS), dtype=float),
    })
    calls = []
    real = ops.hash_vectorize

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "hash_vectorize", counting)
    on = Encoderizer(size="small").fit_transform(df)
    assert calls, "the device path was not taken"
    monkeypatch.setattr(ops, "hip_available", lambda: False)
    n_calls = len(calls)
    off = Encoderizer(size="small").fit_transform(df)
    assert len(calls) == n_calls, "the device path was not disabled"
    assert on.shape == off.shape
    d = abs(on - off)
    assert (d.max() if d.shape[0] else 0.0) < 1e-12
