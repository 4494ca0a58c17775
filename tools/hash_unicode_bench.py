"""Throughput of HashingVectorizerChunked on ASCII, mixed and non-ASCII
text (documents/s, warm, best of 3 after one warm-up).

Seeded synthetic corpus: 1M documents of about 20 words, n_features=2**20,
word analyzer, ngram_range=(1, 2), default chunksize (100,000).

  (a) ascii     every document pure ASCII
  (b) mixed     the same corpus, 1 document in 1,000 carries one
                non-ASCII word
  (c) unicode   every word non-ASCII (Latin-1, Cyrillic, CJK), timed on
                the device path and on sklearn's HashingVectorizer

Run it on two checkouts on the same box to compare commits:

    python tools/hash_unicode_bench.py                  # this tree
    python tools/hash_unicode_bench.py --root ../other  # another tree
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))),
    help="checkout whose skdist_amd package is measured")
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--cases", default="ascii,mixed,unicode")
ap.add_argument("--no-sklearn", action="store_true",
                help="skip the sklearn timing of case (c)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np
import torch
from sklearn.feature_extraction.text import HashingVectorizer

import skdist_amd
from skdist_amd.preprocessing import HashingVectorizerChunked

KW = dict(n_features=2 ** 20, analyzer="word", ngram_range=(1, 2))
WORDS_PER_DOC = 20
VOCAB = 50_000


def _vocab(rng, alphabet):
    letters = np.array(list(alphabet))
    lens = rng.integers(2, 10, size=VOCAB)
    return np.array(
        ["".join(rng.choice(letters, size=n)) for n in lens], dtype=object
    )


def _corpus(rng, vocab, n):
    idx = rng.integers(0, VOCAB, size=(n, WORDS_PER_DOC))
    nw = rng.integers(WORDS_PER_DOC - 5, WORDS_PER_DOC + 1, size=n)
    return [" ".join(vocab[row[:k]]) for row, k in zip(idx, nw)]


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _time(fn, docs, repeats=3, warmup=1):
    for _ in range(warmup):
        fn(docs)
    ts = []
    for _ in range(repeats):
        _sync()
        t0 = time.perf_counter()
        out = fn(docs)
        _sync()
        ts.append(time.perf_counter() - t0)
    return ts, out


def _report(name, path, ts, n):
    best = min(ts)
    print(f"{name:<8} {path:<8} {n / best:12.0f} docs/s  best {best:.3f}s  "
          f"runs {[round(t, 3) for t in ts]}", flush=True)


def main():
    rng = np.random.default_rng(20240607)
    n = args.docs
    ascii_vocab = _vocab(rng, "abcdefghijklmnopqrstuvwxyz")
    uni_vocab = _vocab(rng, "àéîõüñçßøåабвгдежзиклмнопрстуяю日本語中文字符한글")
    print(f"package: {os.path.dirname(skdist_amd.__file__)}")
    dev = (torch.cuda.get_device_name(0) if torch.cuda.is_available()
           else "none (sklearn fallback everywhere)")
    print(f"device: {dev}  docs: {n}  {KW}")
    vec = HashingVectorizerChunked(**KW)
    cases = args.cases.split(",")
    docs = _corpus(rng, ascii_vocab, n)
    docs_arr = np.asarray(docs, dtype=object)

    def device_path(d):
        return vec._try_device_transform(list(d[:1000])) is not None

    if "ascii" in cases:
        path = "device" if device_path(docs) else "sklearn"
        ts, _ = _time(vec.transform, docs_arr)
        _report("ascii", path, ts, n)
    if "mixed" in cases:
        mixed = list(docs)
        for i in range(0, n, 1000):
            mixed[i] = mixed[i] + " " + uni_vocab[i % VOCAB]
        path = "device" if device_path(mixed) else "sklearn"
        ts, _ = _time(vec.transform, np.asarray(mixed, dtype=object))
        _report("mixed", path, ts, n)
        del mixed
    if "unicode" in cases:
        del docs, docs_arr
        udocs = _corpus(rng, uni_vocab, n)
        path = "device" if device_path(udocs) else "sklearn"
        ts, out = _time(vec.transform, np.asarray(udocs, dtype=object))
        _report("unicode", path, ts, n)
        if not args.no_sklearn:
            ts, ref = _time(HashingVectorizer(**KW).transform, udocs)
            _report("unicode", "sklearn*", ts, n)
            d = abs(out - ref)
            print(f"unicode  max |device - sklearn| = "
                  f"{d.max() if d.nnz else 0.0:.3g}  nnz {ref.nnz}")


if __name__ == "__main__":
    main()
