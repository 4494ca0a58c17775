// HIP hashing vectorizer — CDNA4 (gfx950) kernels.
//
// Device replacement for the murmurhash3/CSR core of sklearn's
// HashingVectorizer that the reference's Encoderizer text pipelines call
// (reference skdist/preprocessing.py:264-310, _defaults.py:91-198;
// SURVEY.md §2.4 "HashingVectorizer" row).  The documents travel to HBM
// ONCE as a packed byte buffer; tokenization + murmur3 + feature hashing
// run on-device and emit (doc*F + feature, ±1) COO pairs through a
// global bump allocator; the torch side sorts + segment-sums them into a
// CSR (skdist_amd/ops/__init__.py:hash_vectorize).
//
// Analyzer parity with sklearn.  Two kernels share murmur3_32 and emit:
//   k_hash_vectorize       byte-oriented, exact for pure-ASCII buffers;
//   k_hash_vectorize_utf8  walks UTF-8 code points with Python's own \w
//                          and \s classes (tables generated at run time
//                          by ops/unicode_tables.py), exact for any
//                          well-formed UTF-8 buffer.
// The host wrapper lowercases (and strips accents) first, then routes an
// all-ASCII buffer to the first kernel and anything else to the second.
//   * word:    token_pattern \w\w+ (runs of word-class characters,
//              length >= 2 CHARACTERS), n-grams joined by single spaces;
//   * char_wb: whitespace-split words padded with one space each side,
//              sliding char n-grams; a word shorter than n yields the
//              whole padded word once (sklearn's offset==0 break).
// Long n-grams: the ASCII kernel silently skips a word n-gram (n >= 2)
// longer than GRAM_MAX bytes (known deviation, docs/PARITY.md); the UTF-8
// kernel raises an overflow flag in ctr[1] instead and the host refuses
// the result.
// Hash: MurmurHash3_x86_32(token_bytes, seed=0), signed;
//   index = abs(h) % n_features, value = +1 / -1 (alternate_sign).
#include "common.h"

#define GRAM_MAX 768

static __device__ __forceinline__ unsigned rotl32(unsigned x, int r) {
    return (x << r) | (x >> (32 - r));
}

static __device__ int murmur3_32(const unsigned char* data, int len,
                                 unsigned seed) {
    const unsigned c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    unsigned h1 = seed;
    const int nblocks = len / 4;
    for (int i = 0; i < nblocks; ++i) {
        unsigned k1 = (unsigned)data[i * 4] |
                      ((unsigned)data[i * 4 + 1] << 8) |
                      ((unsigned)data[i * 4 + 2] << 16) |
                      ((unsigned)data[i * 4 + 3] << 24);
        k1 *= c1;
        k1 = rotl32(k1, 15);
        k1 *= c2;
        h1 ^= k1;
        h1 = rotl32(h1, 13);
        h1 = h1 * 5u + 0xe6546b64u;
    }
    unsigned k1 = 0;
    switch (len & 3) {
        case 3: k1 ^= (unsigned)data[nblocks * 4 + 2] << 16;
        case 2: k1 ^= (unsigned)data[nblocks * 4 + 1] << 8;
        case 1:
            k1 ^= (unsigned)data[nblocks * 4];
            k1 *= c1;
            k1 = rotl32(k1, 15);
            k1 *= c2;
            h1 ^= k1;
    }
    h1 ^= (unsigned)len;
    h1 ^= h1 >> 16;
    h1 *= 0x85ebca6bu;
    h1 ^= h1 >> 13;
    h1 *= 0xc2b2ae35u;
    h1 ^= h1 >> 16;
    return (int)h1;
}

static __device__ __forceinline__ void
emit(unsigned long long doc, const unsigned char* buf, int len, unsigned F,
     int alt_sign, unsigned long long* keys, float* vals,
     unsigned long long* ctr, long long cap) {
    const int h = murmur3_32(buf, len, 0u);
    const unsigned idx =
        (h < 0 ? (unsigned)(-(long long)h) : (unsigned)h) % F;
    const float v = (!alt_sign || h >= 0) ? 1.f : -1.f;
    const unsigned long long pos = atomicAdd(ctr, 1ull);
    if (pos < (unsigned long long)cap) {
        keys[pos] = doc * (unsigned long long)F + idx;
        vals[pos] = v;
    }
}

static __device__ __forceinline__ bool is_word_char(unsigned char c) {
    // ASCII \w; bytes >= 0x80 (utf-8 continuation/lead) are treated as
    // word chars — exact for pure-ASCII docs (host gates on that)
    return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') ||
           (c >= '0' && c <= '9') || c == '_' || c >= 0x80;
}

static __device__ __forceinline__ bool is_space(unsigned char c) {
    return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' ||
           c == '\v';
}

#define MAX_NGRAM_TOKENS 8

extern "C" __global__ __launch_bounds__(256) void k_hash_vectorize(
    const unsigned char* __restrict__ bytes,
    const long long* __restrict__ doc_off,  // [n_docs + 1]
    long long n_docs, int mode,             // 0 = word, 1 = char_wb
    int min_n, int max_n, int n_features, int alt_sign,
    unsigned long long* __restrict__ out_keys,
    float* __restrict__ out_vals, unsigned long long* __restrict__ ctr,
    long long cap) {
    const unsigned F = (unsigned)n_features;
    for (long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         d < n_docs; d += (long long)gridDim.x * blockDim.x) {
        const long long lo = doc_off[d], hi = doc_off[d + 1];
        if (mode == 0) {
            // ---- word analyzer ----
            long long tok_start[MAX_NGRAM_TOKENS];
            int tok_len[MAX_NGRAM_TOKENS];
            int n_tok = 0;
            long long p = lo;
            while (p < hi) {
                while (p < hi && !is_word_char(bytes[p])) ++p;
                const long long s = p;
                while (p < hi && is_word_char(bytes[p])) ++p;
                const int len = (int)(p - s);
                if (len < 2) continue;  // token_pattern \w\w+
                // shift ring
                if (n_tok == MAX_NGRAM_TOKENS) {
                    for (int i = 1; i < MAX_NGRAM_TOKENS; ++i) {
                        tok_start[i - 1] = tok_start[i];
                        tok_len[i - 1] = tok_len[i];
                    }
                    --n_tok;
                }
                tok_start[n_tok] = s;
                tok_len[n_tok] = len;
                ++n_tok;
                // n-grams ending at this token
                unsigned char gram[GRAM_MAX];
                for (int n = min_n; n <= max_n && n <= n_tok; ++n) {
                    if (n == 1) {
                        // unigram: hash straight from the global buffer
                        emit((unsigned long long)d, bytes + s, len, F,
                             alt_sign, out_keys, out_vals, ctr, cap);
                        continue;
                    }
                    int glen = 0;
                    bool ok = true;
                    for (int t = n_tok - n; t < n_tok; ++t) {
                        if (glen + tok_len[t] + 1 > GRAM_MAX) {
                            ok = false;
                            break;
                        }
                        if (glen) gram[glen++] = ' ';
                        for (int b = 0; b < tok_len[t]; ++b)
                            gram[glen++] = bytes[tok_start[t] + b];
                    }
                    if (ok)
                        emit((unsigned long long)d, gram, glen, F,
                             alt_sign, out_keys, out_vals, ctr, cap);
                }
            }
        } else {
            // ---- char_wb analyzer ----
            long long p = lo;
            unsigned char win[64];
            while (p < hi) {
                while (p < hi && is_space(bytes[p])) ++p;
                const long long s = p;
                while (p < hi && !is_space(bytes[p])) ++p;
                const int wlen = (int)(p - s);
                if (wlen == 0) continue;
                const int plen = wlen + 2;  // ' ' + word + ' '
                for (int n = min_n; n <= max_n; ++n) {
                    if (n >= plen) {
                        // short word: whole padded word, once
                        win[0] = ' ';
                        for (int b = 0; b < wlen && b < 62; ++b)
                            win[b + 1] = bytes[s + b];
                        win[wlen + 1] = ' ';
                        emit((unsigned long long)d, win, plen, F,
                             alt_sign, out_keys, out_vals, ctr, cap);
                        break;
                    }
                    for (int off = 0; off + n <= plen; ++off) {
                        for (int b = 0; b < n; ++b) {
                            const int q = off + b;
                            win[b] = (q == 0 || q == plen - 1)
                                         ? (unsigned char)' '
                                         : bytes[s + q - 1];
                        }
                        emit((unsigned long long)d, win, n, F, alt_sign,
                             out_keys, out_vals, ctr, cap);
                    }
                }
            }
        }
    }
}

extern "C" hipError_t skdist_hash_vectorize(
    const void* bytes, const void* doc_off, long long n_docs, int mode,
    int min_n, int max_n, int n_features, int alt_sign, void* out_keys,
    void* out_vals, void* ctr, long long cap, hipStream_t stream) {
    const int blocks =
        (int)std::min<long long>((n_docs + 255) / 256, 16384);
    hipLaunchKernelGGL(k_hash_vectorize, dim3(blocks), dim3(256), 0,
                       stream, (const unsigned char*)bytes,
                       (const long long*)doc_off, n_docs, mode, min_n,
                       max_n, n_features, alt_sign,
                       (unsigned long long*)out_keys, (float*)out_vals,
                       (unsigned long long*)ctr, cap);
    return hipGetLastError();
}

// ======================================================================
// UTF-8 tokenizer: same launch shape, COO output and bump allocator as
// k_hash_vectorize, but the analyzers walk code points.
//   word_tbl  bitmap of Python's \w over U+0000..U+10FFFF, bit cp&31 of
//             word cp>>5 (0x110000/32 words);
//   ws_list   sorted code points of Python's \s (n_ws <= WS_MAX).
// ctr[0] is the bump allocator, ctr[1] the overflow flag: nonzero when an
// n-gram did not fit its per-thread buffer (nothing is dropped silently).
#define WS_MAX 64
#define WIN_CHARS 32
#define WIN_BYTES (WIN_CHARS * 4)
#define CP_LIMIT 0x110000u
#define CP_INVALID 0xffffffffu

// Byte length announced by a UTF-8 lead byte (1 for a stray continuation
// byte, so a malformed buffer still makes progress).
static __device__ __forceinline__ int u8_len(unsigned c) {
    return c < 0xC0 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
}

// Decode the code point at p (p < hi).  Never reads at or past hi: a
// sequence cut off by the document end decodes to CP_INVALID and spans
// the bytes that are left.
static __device__ __forceinline__ int
u8_decode(const unsigned char* __restrict__ bytes, long long p,
          long long hi, unsigned& cp) {
    const unsigned c = bytes[p];
    if (c < 0x80) {
        cp = c;
        return 1;
    }
    const int len = u8_len(c);
    if (len == 1) {
        cp = CP_INVALID;
        return 1;
    }
    if (p + len > hi) {
        cp = CP_INVALID;
        return (int)(hi - p);
    }
    unsigned v = c & (0xFFu >> (len + 1));
    for (int i = 1; i < len; ++i) v = (v << 6) | (bytes[p + i] & 0x3Fu);
    cp = v;
    return len;
}

// 128-bit ASCII class mask held in two registers
struct AsciiMask {
    unsigned long long lo, hi;
    __device__ __forceinline__ bool test(unsigned cp) const {
        return ((cp < 64 ? lo : hi) >> (cp & 63)) & 1ull;
    }
};

static __device__ __forceinline__ bool
u8_is_word(unsigned cp, const AsciiMask& am,
           const unsigned* __restrict__ word_tbl) {
    if (cp < 0x80) return am.test(cp);
    if (cp >= CP_LIMIT) return false;
    return (word_tbl[cp >> 5] >> (cp & 31)) & 1u;
}

static __device__ __forceinline__ bool
u8_is_space(unsigned cp, const AsciiMask& am, const int* s_ws, int n_ws) {
    if (cp < 0x80) return am.test(cp);
    if (n_ws == 0 || cp > (unsigned)s_ws[n_ws - 1]) return false;
    int a = 0, b = n_ws;
    while (a < b) {
        const int m = (a + b) >> 1;
        if ((unsigned)s_ws[m] < cp) a = m + 1; else b = m;
    }
    return a < n_ws && (unsigned)s_ws[a] == cp;
}

extern "C" __global__ __launch_bounds__(256) void k_hash_vectorize_utf8(
    const unsigned char* __restrict__ bytes,
    const long long* __restrict__ doc_off,  // [n_docs + 1]
    long long n_docs, int mode,             // 0 = word, 1 = char_wb
    int min_n, int max_n, int n_features, int alt_sign,
    const unsigned* __restrict__ word_tbl,  // [CP_LIMIT / 32]
    const int* __restrict__ ws_list, int n_ws,
    unsigned long long* __restrict__ out_keys,
    float* __restrict__ out_vals, unsigned long long* __restrict__ ctr,
    long long cap) {
    __shared__ int s_ws[WS_MAX];
    if (n_ws > WS_MAX) n_ws = WS_MAX;  // launcher rejects this
    for (int i = threadIdx.x; i < n_ws; i += blockDim.x)
        s_ws[i] = ws_list[i];
    __syncthreads();
    // ASCII fast path: the first 128 bits of the class in registers
    AsciiMask am = {0ull, 0ull};
    if (mode == 0) {
        am.lo = (unsigned long long)word_tbl[0] |
                ((unsigned long long)word_tbl[1] << 32);
        am.hi = (unsigned long long)word_tbl[2] |
                ((unsigned long long)word_tbl[3] << 32);
    } else {
        for (int i = 0; i < n_ws; ++i) {
            const int c = s_ws[i];
            if (c < 64) am.lo |= 1ull << c;
            else if (c < 128) am.hi |= 1ull << (c - 64);
        }
    }
    const unsigned F = (unsigned)n_features;
    for (long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         d < n_docs; d += (long long)gridDim.x * blockDim.x) {
        const long long lo = doc_off[d], hi = doc_off[d + 1];
        if (mode == 0) {
            // ---- word analyzer: maximal runs of \w, >= 2 characters ----
            long long tok_start[MAX_NGRAM_TOKENS];
            int tok_len[MAX_NGRAM_TOKENS];
            int n_tok = 0;
            long long p = lo, s = lo;
            int nch = 0;  // characters in the run that started at s
            while (true) {
                int clen = 0;
                bool w = false;
                if (p < hi) {
                    unsigned cp;
                    clen = u8_decode(bytes, p, hi, cp);
                    w = u8_is_word(cp, am, word_tbl);
                }
                if (w) {
                    if (nch == 0) s = p;
                    ++nch;
                    p += clen;
                    continue;
                }
                // run boundary: a non-word character or the document end
                const int run = nch;
                const int len = (int)(p - s);
                nch = 0;
                const bool at_end = p >= hi;
                p += clen;
                if (run >= 2) {
                    if (n_tok == MAX_NGRAM_TOKENS) {
                        for (int i = 1; i < MAX_NGRAM_TOKENS; ++i) {
                            tok_start[i - 1] = tok_start[i];
                            tok_len[i - 1] = tok_len[i];
                        }
                        --n_tok;
                    }
                    tok_start[n_tok] = s;
                    tok_len[n_tok] = len;
                    ++n_tok;
                    // n-grams ending at this token
                    unsigned char gram[GRAM_MAX];
                    for (int n = min_n; n <= max_n && n <= n_tok; ++n) {
                        if (n == 1) {
                            // unigram: hash straight from the global
                            // buffer, no length limit
                            emit((unsigned long long)d, bytes + s, len, F,
                                 alt_sign, out_keys, out_vals, ctr, cap);
                            continue;
                        }
                        int glen = 0;
                        bool ok = true;
                        for (int t = n_tok - n; t < n_tok; ++t) {
                            if (glen + tok_len[t] + 1 > GRAM_MAX) {
                                ok = false;
                                break;
                            }
                            if (glen) gram[glen++] = ' ';
                            for (int b = 0; b < tok_len[t]; ++b)
                                gram[glen++] = bytes[tok_start[t] + b];
                        }
                        if (ok)
                            emit((unsigned long long)d, gram, glen, F,
                                 alt_sign, out_keys, out_vals, ctr, cap);
                        else
                            atomicOr(ctr + 1, 1ull);
                    }
                }
                if (at_end) break;
            }
        } else {
            // ---- char_wb analyzer: windows slide in characters ----
            long long p = lo;
            unsigned char win[WIN_BYTES];
            while (p < hi) {
                unsigned cp;
                while (p < hi) {
                    const int clen = u8_decode(bytes, p, hi, cp);
                    if (!u8_is_space(cp, am, s_ws, n_ws)) break;
                    p += clen;
                }
                const long long s = p;
                int wch = 0;  // characters in the word [s, e)
                while (p < hi) {
                    const int clen = u8_decode(bytes, p, hi, cp);
                    if (u8_is_space(cp, am, s_ws, n_ws)) break;
                    p += clen;
                    ++wch;
                }
                const long long e = p;
                if (wch == 0) continue;
                const int plen = wch + 2;  // ' ' + word + ' '
                for (int n = min_n; n <= max_n; ++n) {
                    if (n >= plen) {
                        // short word: whole padded word, once
                        if (e - s + 2 > WIN_BYTES) {
                            atomicOr(ctr + 1, 1ull);
                            break;
                        }
                        int glen = 0;
                        win[glen++] = ' ';
                        for (long long q = s; q < e; ++q)
                            win[glen++] = bytes[q];
                        win[glen++] = ' ';
                        emit((unsigned long long)d, win, glen, F,
                             alt_sign, out_keys, out_vals, ctr, cap);
                        break;
                    }
                    // ws: byte offset of padded character max(off, 1)
                    long long ws = s;
                    for (int off = 0; off + n <= plen; ++off) {
                        int glen = 0;
                        bool ok = true;
                        long long q = ws;
                        for (int b = 0; b < n; ++b) {
                            const int idx = off + b;
                            if (idx == 0 || idx == plen - 1) {
                                if (glen + 1 > WIN_BYTES) {
                                    ok = false;
                                    break;
                                }
                                win[glen++] = ' ';
                                continue;
                            }
                            int clen = q < e ? u8_len(bytes[q]) : 0;
                            if (q + clen > e) clen = (int)(e - q);
                            if (clen == 0 || glen + clen > WIN_BYTES) {
                                ok = false;
                                break;
                            }
                            for (int k = 0; k < clen; ++k)
                                win[glen++] = bytes[q + k];
                            q += clen;
                        }
                        if (ok)
                            emit((unsigned long long)d, win, glen, F,
                                 alt_sign, out_keys, out_vals, ctr, cap);
                        else
                            atomicOr(ctr + 1, 1ull);
                        if (off >= 1 && ws < e) {
                            int clen = u8_len(bytes[ws]);
                            if (ws + clen > e) clen = (int)(e - ws);
                            ws += clen;
                        }
                    }
                }
            }
        }
    }
}

extern "C" hipError_t skdist_hash_vectorize_utf8(
    const void* bytes, const void* doc_off, long long n_docs, int mode,
    int min_n, int max_n, int n_features, int alt_sign,
    const void* word_tbl, const void* ws_list, int n_ws, void* out_keys,
    void* out_vals, void* ctr, long long cap, hipStream_t stream) {
    if (n_ws < 0 || n_ws > WS_MAX) return hipErrorInvalidValue;
    const int blocks =
        (int)std::min<long long>((n_docs + 255) / 256, 16384);
    hipLaunchKernelGGL(k_hash_vectorize_utf8, dim3(blocks), dim3(256), 0,
                       stream, (const unsigned char*)bytes,
                       (const long long*)doc_off, n_docs, mode, min_n,
                       max_n, n_features, alt_sign,
                       (const unsigned*)word_tbl, (const int*)ws_list,
                       n_ws, (unsigned long long*)out_keys,
                       (float*)out_vals, (unsigned long long*)ctr, cap);
    return hipGetLastError();
}
