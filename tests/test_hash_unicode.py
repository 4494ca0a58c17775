"""CPU tests: Unicode class tables and the device-path gate of
HashingVectorizerChunked (no GPU needed; the kernel itself is covered by
tests/test_hash_unicode_gpu.py)."""

import re

import numpy as np
import pytest
from sklearn.feature_extraction.text import (
    HashingVectorizer, strip_accents_ascii, strip_accents_unicode,
)

UNICODE_DOCS = [
    "café — 日本語",
    "ÉCOLE İstanbul ΟΔΟΣ",
    "nb\xa0sp em\u2003sp a\x1fbb é",
    "",
    "plain ascii words here",
    "smile😀face x² ٣٤ 𝒳𝒳",
]


def _non_surrogates():
    return (cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF)


def test_word_bitmap_matches_re():
    from skdist_amd.ops.unicode_tables import BITMAP_WORDS, word_bitmap

    bm = word_bitmap()
    assert bm.dtype == np.uint32
    assert bm.shape == (0x110000 // 32,) == (BITMAP_WORDS,)
    bits = np.unpackbits(bm.view(np.uint8), bitorder="little")
    word = re.compile(r"\w")
    wrong = [
        cp for cp in _non_surrogates()
        if bool(bits[cp]) != (word.fullmatch(chr(cp)) is not None)
    ]
    assert wrong == []
    # surrogates are class 0
    assert not bits[0xD800:0xE000].any()
    # the kernel's lookup expression
    for ch in "a_9é日𝒳٣²½ⅷ":
        cp = ord(ch)
        assert (int(bm[cp >> 5]) >> (cp & 31)) & 1
    for ch in " -—😀\u200d\xad\u0307€":
        cp = ord(ch)
        assert not (int(bm[cp >> 5]) >> (cp & 31)) & 1


def test_whitespace_list_matches_python():
    from skdist_amd.ops.unicode_tables import (
        MAX_WHITESPACE, whitespace_codepoints,
    )

    ws = whitespace_codepoints()
    assert ws.dtype == np.int32
    assert list(ws) == sorted(set(ws.tolist()))
    assert len(ws) <= MAX_WHITESPACE
    assert set(ws.tolist()) == {
        cp for cp in _non_surrogates() if chr(cp).isspace()
    }
    # ... which is what str.split() splits on
    assert set(ws.tolist()) == {
        cp for cp in _non_surrogates()
        if ("a" + chr(cp) + "b").split() == ["a", "b"]
    }
    for cp in (0x1C, 0x1F, 0x85, 0xA0, 0x1680, 0x2003, 0x2028, 0x3000):
        assert cp in ws


def test_tables_are_cached():
    from skdist_amd.ops import unicode_tables as ut

    assert ut.host_tables()[0] is ut.host_tables()[0]
    assert ut.word_bitmap() is ut.host_tables()[0]


@pytest.fixture
def recorder(monkeypatch):
    """Pretend HIP is there; record what reaches ops.hash_vectorize.

    Like the real function, the stand-in packs the documents as UTF-8
    first (which is where an unencodable document raises, before anything
    reaches the device) and records only what it could pack."""
    import skdist_amd.ops as ops

    seen = []

    def fake(docs, **kw):
        for d in docs:
            d.encode("utf-8")
        seen.append((list(docs), kw))
        return "sentinel"

    monkeypatch.setattr(ops, "hip_available", lambda: True)
    monkeypatch.setattr(ops, "hash_vectorize", fake)
    return seen


def test_gate_forwards_unicode(recorder):
    from skdist_amd.preprocessing import HashingVectorizerChunked

    v = HashingVectorizerChunked(ngram_range=(1, 2))
    assert v._try_device_transform(list(UNICODE_DOCS)) == "sentinel"
    docs, kw = recorder[-1]
    assert docs == UNICODE_DOCS
    assert kw["lowercase"] is True
    assert kw["ngram_range"] == (1, 2)


@pytest.mark.parametrize("name,func", [
    ("unicode", strip_accents_unicode), ("ascii", strip_accents_ascii),
])
def test_gate_strips_accents_on_host(recorder, name, func):
    from skdist_amd.preprocessing import HashingVectorizerChunked

    v = HashingVectorizerChunked(strip_accents=name)
    assert v._try_device_transform(list(UNICODE_DOCS)) == "sentinel"
    docs, kw = recorder[-1]
    # sklearn's order: lower(), then strip; nothing left for the callee
    assert docs == [func(d.lower()) for d in UNICODE_DOCS]
    assert kw["lowercase"] is False
    assert "cafe" in docs[0]

    v = HashingVectorizerChunked(strip_accents=name, lowercase=False)
    assert v._try_device_transform(list(UNICODE_DOCS)) == "sentinel"
    docs, kw = recorder[-1]
    assert docs == [func(d) for d in UNICODE_DOCS]
    assert kw["lowercase"] is False


def test_gate_rejects_callable_strip_accents(recorder):
    from skdist_amd.preprocessing import HashingVectorizerChunked

    v = HashingVectorizerChunked(strip_accents=strip_accents_unicode)
    assert v._try_device_transform(list(UNICODE_DOCS)) is None
    assert recorder == []


def test_gate_rejects_lone_surrogate(recorder):
    from skdist_amd.preprocessing import HashingVectorizerChunked

    v = HashingVectorizerChunked()
    assert v._try_device_transform(["fine", "bad \ud83d doc"]) is None
    assert v._try_device_transform(["fine", b"bytes"]) is None
    assert recorder == []


def test_gate_keeps_other_fallbacks(recorder):
    from skdist_amd.preprocessing import HashingVectorizerChunked

    docs = list(UNICODE_DOCS)
    for kw in (
        dict(token_pattern=r"\w+"), dict(stop_words=["the"]),
        dict(tokenizer=str.split), dict(preprocessor=str.lower),
        dict(input="file"), dict(analyzer="char"),
        dict(ngram_range=(1, 9)),
        dict(analyzer="char_wb", ngram_range=(1, 33)),
    ):
        assert HashingVectorizerChunked(**kw)._try_device_transform(
            docs) is None, kw
    assert recorder == []


def test_gate_falls_back_on_gram_overflow(monkeypatch):
    import skdist_amd.ops as ops
    from skdist_amd.preprocessing import HashingVectorizerChunked

    def overflowing(docs, **kw):
        raise ops.HashGramOverflow("too long")

    monkeypatch.setattr(ops, "hip_available", lambda: True)
    monkeypatch.setattr(ops, "hash_vectorize", overflowing)
    v = HashingVectorizerChunked(ngram_range=(1, 2))
    assert v._try_device_transform(list(UNICODE_DOCS)) is None
    out = v.transform(np.asarray(UNICODE_DOCS, dtype=object))
    ref = HashingVectorizer(ngram_range=(1, 2)).transform(UNICODE_DOCS)
    assert abs(out - ref).max() < 1e-12
    assert issubclass(ops.HashGramOverflow, ValueError)


@pytest.mark.parametrize("kw", [
    dict(ngram_range=(1, 2)),
    dict(analyzer="char_wb", ngram_range=(2, 4)),
    dict(strip_accents="unicode"),
])
def test_fallback_path_equals_sklearn(monkeypatch, kw):
    import skdist_amd.ops as ops
    from skdist_amd.preprocessing import HashingVectorizerChunked

    monkeypatch.setattr(ops, "hip_available", lambda: False)
    out = HashingVectorizerChunked(**kw).transform(
        np.asarray(UNICODE_DOCS, dtype=object))
    ref = HashingVectorizer(**kw).transform(UNICODE_DOCS)
    assert out.shape == ref.shape
    assert abs(out - ref).max() < 1e-12
