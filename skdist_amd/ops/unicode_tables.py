"""
Unicode class tables for the UTF-8 hashing-vectorizer kernel
(csrc/hash_kernels.hip: k_hash_vectorize_utf8).

Both tables are generated at run time from the running interpreter's own
``re`` module, so they are exact for whatever Python (and Unicode database)
runs the package; nothing is hard-coded or shipped:

* ``word_bitmap()``: ``\\w`` over U+0000..U+10FFFF as a bitmap, bit
  ``cp & 31`` of word ``cp >> 5`` (0x110000 / 32 ``uint32`` words, 136 KB);
* ``whitespace_codepoints()``: the sorted code points of ``\\s`` (what
  ``str.split()`` splits on).

Surrogates cannot be encoded to UTF-8 and are absent from both (class 0).
Host tables are built once per process, device copies once per device.
"""

import re

import numpy as np

N_CODEPOINTS = 0x110000
BITMAP_WORDS = N_CODEPOINTS // 32
MAX_WHITESPACE = 64  # kernel-side capacity of the whitespace list (WS_MAX)

_host = None
_device = {}


def _build():
    text = "".join(
        chr(cp) for cp in range(N_CODEPOINTS) if not 0xD800 <= cp <= 0xDFFF
    )
    word = np.fromiter(map(ord, re.findall(r"\w", text)), dtype=np.int64)
    space = np.fromiter(map(ord, re.findall(r"\s", text)), dtype=np.int64)
    bits = np.zeros(N_CODEPOINTS, dtype=np.uint8)
    bits[word] = 1
    bitmap = np.packbits(bits, bitorder="little").view("<u4")
    bitmap = np.ascontiguousarray(bitmap, dtype=np.uint32)
    ws = np.sort(space).astype(np.int32)
    if len(ws) > MAX_WHITESPACE:
        raise RuntimeError(
            f"{len(ws)} whitespace code points exceed the kernel's "
            f"capacity of {MAX_WHITESPACE}"
        )
    bitmap.setflags(write=False)
    ws.setflags(write=False)
    return bitmap, ws


def host_tables():
    """(word bitmap uint32[0x110000/32], sorted whitespace int32[n])."""
    global _host
    if _host is None:
        _host = _build()
    return _host


def word_bitmap():
    return host_tables()[0]


def whitespace_codepoints():
    return host_tables()[1]


def device_tables(device):
    """Device copies (int32 views, as the binding expects), cached per
    device."""
    import torch

    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    hit = _device.get(dev)
    if hit is None:
        bitmap, ws = host_tables()
        hit = (
            torch.from_numpy(bitmap.view(np.int32).copy()).to(dev),
            torch.from_numpy(ws.copy()).to(dev),
        )
        _device[dev] = hit
    return hit
