// Batched histogram decision-tree builder — CDNA4 (gfx950) kernels.
//
// MI355X-native replacement for the per-tree sklearn Cython builder the
// reference fans out (reference worker
// skdist/distribute/ensemble.py:68-109).  A batch of TB trees grows
// level-synchronously against ONE HBM-resident binned copy of X:
//
//   K0 k_bin_csr:      CSR -> uint8 codes (scipy-sparse X)
//   K1 k_tree_hist:    per-(node,feature,bin) weighted stats, LDS-staged
//      k_tree_hist_w:  the regression stats with a real-valued f32 row-weight
//                      plane on top of the uint8 one, plus a row-count slot
//      k_tree_hist_cg: class counts with the classes split into groups of
//                      cg, one LDS tile per (feature group, class group)
//   K2 k_tree_split:   best (feature,bin) per frontier node — gini /
//                      entropy / mse scan with exact max_features
//                      subsampling and ExtraTrees random-threshold mode
//      k_tree_split_w: same scan; the min-leaf test reads a count slot
//      k_tree_split_wide: the classification scan for 32 < S <= 256, one
//                      wave per feature with the classes across its lanes
//   K3 k_part_count:   per-chunk left-row counts for the stable partition
//   K4 k_part_scatter: stable partition of each node's sample segment
//
// K1 has ONE body (tree_hist_body<ROW_W, GROUPED>); K2 has one per register
// layout (tree_split_body<COUNTED, MISSING>: a thread per feature, S <= 32;
// tree_split_wide_body<MISSING>: a wave per feature, S <= 256) that share
// the feature subsample and the block-level ending.  ONE checked launcher
// each (tree_api.h) picks the instantiation: skdist_tree_hist by
// row_w != nullptr and cg > 0, skdist_tree_split by S > 32, cnt_stat >= 0
// and its `missing` flag.
//
// Missing values: a dataset binned with a missing bin keeps code nbins-1
// for NaN cells.  K1 is unchanged (missing is one more bin); the MISSING
// split scan evaluates every (feature, bin) cut twice, with the missing
// bin's stats on the right (R) and on the left (L), and reports the learned
// direction per node; K3/K4 send code nbins-1 left where that flag is set.
//
// Host orchestration + torch eager reference: skdist_amd/models/forest.py.
//
// Layouts:
//   codes      [n][fp]   uint8   row-major quantile bin codes (fp = f
//                                     padded to a multiple of 4 for uchar4 loads)
//   sample_idx [TB][n]   int32   per-tree row ids, node segments contiguous
//   weights    [TB][n]   uint8   bootstrap multiplicities (0 = out of bag)
//   row_w      [n]       f32     real-valued row weights, shared by all trees
//                                     of the batch (ROW_W instantiation only)
//   hist       [NF][f][nbins][S] f32   S = n_classes (cls) | 3 (w,wy,wyy)
//                                       | 4 (W,Wy,Wyy,C) with row_w, where
//                                       w = weights*row_w and C = Σ weights
//   hist LDS   [fg][nbins][S] f32      one tile per (chunk, feature group);
//              [fg][nbins][cg]         class-grouped: per (chunk, feature
//                                      group, class group), the block of
//                                      group z owning classes [z*cg, z*cg+cg)
//   chunks     [n_chunks][4] int32     {node_slot, tree_slot, row_start,
//                                       row_count}
//
// Determinism: classification stats are integer-valued f32 atomics (exact,
// order-independent); regression wy/wyy sums are fp32 atomics whose
// rounding depends on arrival order — ties between split candidates are
// broken by (feature, bin) so only near-exact-tie splits can differ.  With
// row_w the W slot is a real-valued sum too and rounds the same way; the
// count slot C is integer-valued like the class counts, so it is exact and
// the min_samples_* tests that read it do not depend on arrival order.
#include "common.h"
#include "tree_api.h"

#define WAVE 64

static __device__ __forceinline__ unsigned wang_hash(unsigned s) {
    s = (s ^ 61u) ^ (s >> 16);
    s *= 9u;
    s ^= s >> 4;
    s *= 0x27d4eb2du;
    s ^= s >> 15;
    return s;
}

// ---------------------------------------------------------------------- //
// K1: histogram build
// grid: (n_chunks, n_feature_groups[, n_class_groups]), block 256
// dynamic LDS: fg * nbins * S floats (class-grouped: fg * nbins * cg)
// ---------------------------------------------------------------------- //
typedef __attribute__((ext_vector_type(4))) unsigned char uchar4v;

// one row's contribution to one (feature, bin) cell — cls: one atomic on
// the row's class slot; reg: (w, wy, wyy); reg + row_w: the count m as well
template <bool ROW_W>
static __device__ __forceinline__ void hist_cell_add(
    float* h, int is_cls, int stat, float w, float v1, float v2, float m) {
    if (is_cls) {
        atomicAdd(h + stat, w);
    } else {
        atomicAdd(h + 0, w);
        atomicAdd(h + 1, v1);
        atomicAdd(h + 2, v2);
        if (ROW_W) atomicAdd(h + 3, m);
    }
}

// ROW_W: a real-valued f32 row-weight plane on top of the uint8 one
// (regression / gradient stats only, so is_cls is the constant false and
// S the constant 4 there).  m = the tree's uint8 multiplicity; the cell
// weight is w = m (no row_w) or m * row_w, and with row_w a fourth stat
// keeps the row count C = Σ m.  The __restrict__ qualifiers stay on the
// kernel wrappers' own parameters: repeated here they only add per-call
// alias scopes on top of the same facts.
//
// GROUPED (classification only): the block with blockIdx.z = z keeps the
// classes [z*cg, z*cg + cg) and skips every row of another class, so its
// tile is fg * nbins * cg floats whatever S is.  Each row is still counted
// once across the class groups; only the row scan repeats per group.
template <bool ROW_W, bool GROUPED>
static __device__ __forceinline__ void tree_hist_body(
    const unsigned char* codes,    // [n][fp] row-major
    const int* y_int,              // [n] (cls) or nullptr
    const float* y_f,              // [n] (reg) or nullptr
    const float* row_w,            // [n] (ROW_W) or nullptr
    const unsigned char* weights,  // [TB][n]
    const int* sample_idx,         // [TB][n]
    const int* chunks,             // [n_chunks][4]
    float* hist,                   // [NF][f][nbins][S]
    long long n, int f, int fp, int nbins, int S, int is_cls, int fg,
    int cg) {
    extern __shared__ float lds[];
    const int chunk = blockIdx.x;
    const int g0 = blockIdx.y * fg;
    const int nf_g = min(fg, f - g0);
    // first class and stat width of this block's tile
    const int c0 = GROUPED ? (int)blockIdx.z * cg : 0;
    const int cw = GROUPED ? min(cg, S - c0) : S;
    const int node_slot = chunks[chunk * 4 + 0];
    const int tree_slot = chunks[chunk * 4 + 1];
    const int row_start = chunks[chunk * 4 + 2];
    const int row_count = chunks[chunk * 4 + 3];

    const int lds_sz = nf_g * nbins * cw;
    for (int i = threadIdx.x; i < lds_sz; i += blockDim.x) lds[i] = 0.f;
    __syncthreads();

    const int* si = sample_idx + (long long)tree_slot * n + row_start;
    const unsigned char* wrow = weights + (long long)tree_slot * n;
    // vector path: 4 feature codes per uchar4 load (codes rows are
    // padded to fp, a multiple of 4, so over-reads land in zero pad)
    const bool vec = (g0 & 3) == 0;
    for (int r = threadIdx.x; r < row_count; r += blockDim.x) {
        const int i = si[r];
        const float m = (float)wrow[i];
        const float w = ROW_W ? m * row_w[i] : m;
        int stat = 0;
        float v1 = 0.f, v2 = 0.f;
        if (is_cls) {
            stat = y_int[i];
            if (GROUPED) {
                stat -= c0;
                if ((unsigned)stat >= (unsigned)cw) continue;
            }
        } else {
            const float yv = y_f[i];
            v1 = w * yv;
            v2 = w * yv * yv;
        }
        const unsigned char* crow = codes + (long long)i * fp + g0;
        if (vec) {
            const uchar4v* c4 = (const uchar4v*)crow;
            for (int q = 0; q * 4 < nf_g; ++q) {
                const uchar4v b4 = c4[q];
                #pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int jj = q * 4 + t;
                    if (jj >= nf_g) break;
                    hist_cell_add<ROW_W>(
                        lds + ((jj * nbins + (int)b4[t]) * cw), is_cls, stat,
                        w, v1, v2, m);
                }
            }
        } else {
            for (int jj = 0; jj < nf_g; ++jj)
                hist_cell_add<ROW_W>(
                    lds + ((jj * nbins + (int)crow[jj]) * cw), is_cls, stat,
                    w, v1, v2, m);
        }
    }
    __syncthreads();

    float* gh = hist + ((long long)node_slot * f + g0) * nbins * S;
    for (int i = threadIdx.x; i < lds_sz; i += blockDim.x) {
        const float v = lds[i];
        if (v == 0.f) continue;
        if (GROUPED) {
            const int cell = i / cw;   // (feature, bin) of the tile
            atomicAdd(gh + (long long)cell * S + c0 + (i - cell * cw), v);
        } else {
            atomicAdd(gh + i, v);
        }
    }
}

extern "C" __global__ __launch_bounds__(256) void k_tree_hist(
    const unsigned char* __restrict__ codes, const int* __restrict__ y_int,
    const float* __restrict__ y_f, const unsigned char* __restrict__ weights,
    const int* __restrict__ sample_idx, const int* __restrict__ chunks,
    float* __restrict__ hist, long long n, int f, int fp, int nbins, int S,
    int is_cls, int fg) {
    tree_hist_body<false, false>(codes, y_int, y_f, nullptr, weights,
                                 sample_idx, chunks, hist, n, f, fp, nbins,
                                 S, is_cls, fg, 0);
}

// grid.z = class groups of cg; dynamic LDS: fg * nbins * min(cg, S) floats
extern "C" __global__ __launch_bounds__(256) void k_tree_hist_cg(
    const unsigned char* __restrict__ codes, const int* __restrict__ y_int,
    const unsigned char* __restrict__ weights,
    const int* __restrict__ sample_idx, const int* __restrict__ chunks,
    float* __restrict__ hist, long long n, int f, int fp, int nbins, int S,
    int fg, int cg) {
    tree_hist_body<false, true>(codes, y_int, nullptr, nullptr, weights,
                                sample_idx, chunks, hist, n, f, fp, nbins,
                                S, 1, fg, cg);
}

// dynamic LDS: fg * nbins * 4 floats
extern "C" __global__ __launch_bounds__(256) void k_tree_hist_w(
    const unsigned char* __restrict__ codes, const float* __restrict__ y_f,
    const float* __restrict__ row_w,
    const unsigned char* __restrict__ weights,
    const int* __restrict__ sample_idx, const int* __restrict__ chunks,
    float* __restrict__ hist, long long n, int f, int fp, int nbins,
    int fg) {
    tree_hist_body<true, false>(codes, nullptr, y_f, row_w, weights,
                                sample_idx, chunks, hist, n, f, fp, nbins,
                                4, 0, fg, 0);
}

// ---------------------------------------------------------------------- //
// K2: split finding — one 256-thread block per frontier node
// ---------------------------------------------------------------------- //
#define CRIT_GINI 0
#define CRIT_ENTROPY 1
#define CRIT_MSE 2

// impurity from a stats vector (cls: weighted class counts; reg: w,wy,wyy)
static __device__ __forceinline__ float
impurity(const float* s, float w, int S, int is_cls, int crit) {
    if (w <= 0.f) return 0.f;
    if (is_cls) {
        if (crit == CRIT_GINI) {
            float q = 0.f;
            for (int c = 0; c < S; ++c) q += s[c] * s[c];
            return 1.f - q / (w * w);
        }
        float e = 0.f;
        for (int c = 0; c < S; ++c) {
            if (s[c] > 0.f) {
                const float p = s[c] / w;
                e -= p * __log2f(p);
            }
        }
        return e;
    }
    // mse: variance
    const float mean = s[1] / w;
    float v = s[2] / w - mean * mean;
    return v > 0.f ? v : 0.f;
}

// COUNTED: min_samples_leaf stays a ROW count when the weights are real
// numbers — the min-leaf test reads the integer-valued stat cnt_stat
// instead of the weight sums, and a candidate also needs weight on both
// sides.  Impurity, gain, tie-break and outputs are the same either way.
//
// MISSING: the top bin nbins-1 holds the rows whose feature value is
// missing.  Candidates are (feature, bin b <= nbins-2, direction): R is the
// plain prefix (the missing bin is the top bin, so it is already on the
// right; b = nbins-2 cuts "all present | all missing"), L adds the missing
// bin's stats to the left side.  L is scanned only where the feature's
// missing bin holds weight in this node; elsewhere the direction is the
// majority side (wl > wr, ties to the right).  Order among equal gains:
// lower feature, lower bin, R before L.  Validity, impurity and gain are
// the non-MISSING ones.
template <bool COUNTED>
static __device__ __forceinline__ bool split_candidate(
    const float* left, float wl, const float* s_parent, float wp,
    float imp_p, int S, int is_cls, int crit, float min_leaf_w, int cnt_stat,
    float* gain_out) {
    const float wr = wp - wl;
    if (COUNTED) {
        const float cl = left[cnt_stat];
        const float cr = s_parent[cnt_stat] - cl;
        if (cl < min_leaf_w || cr < min_leaf_w) return false;
        if (!(wl > 0.f && wr > 0.f)) return false;
    } else {
        if (wl < min_leaf_w || wr < min_leaf_w) return false;
    }
    const float imp_l = impurity(left, wl, S, is_cls, crit);
    float right[36];
    for (int c = 0; c < S; ++c) right[c] = s_parent[c] - left[c];
    const float imp_r = impurity(right, wr, S, is_cls, crit);
    *gain_out = imp_p - (wl * imp_l + wr * imp_r) / wp;
    return true;
}

// exact m-of-f feature subsample: a feature is kept when its hash ranks in
// the m smallest.  Returns the m-th smallest hash value (binary search, the
// whole block counts per step); every thread of the block calls it.
static __device__ __forceinline__ unsigned feat_hash_threshold(
    unsigned seed, int f, int m_features) {
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    unsigned lo = 0u, hi = 0xffffffffu;
    for (int it = 0; it < 32; ++it) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        int cnt = 0;
        for (int j = tid; j < f; j += blockDim.x)
            if (wang_hash(seed ^ (unsigned)(j * 2654435761u)) <= mid)
                ++cnt;
        atomicAdd(&s_cnt, cnt);
        __syncthreads();
        const int total = s_cnt;
        __syncthreads();
        if (total >= m_features) hi = mid; else lo = mid + 1;
        if (lo >= hi) break;
    }
    return hi;
}

// The ending both scans share.  Lane 0 of every wave brings its wave's best
// candidate; thread 0 merges them (larger gain, then lower feature, lower
// bin) and writes the node's decision, then the block writes the parent
// totals and the winning split's left stats.
template <bool MISSING>
static __device__ __forceinline__ void split_block_finish(
    float best_gain, int best_feat, int best_bin, float best_wl, int best_ml,
    const float* s_parent, float imp_p, const float* H, int node, int nbins,
    int S, int* __restrict__ out_feat, int* __restrict__ out_bin,
    float* __restrict__ out_wl, float* __restrict__ out_gain,
    float* __restrict__ out_imp, float* __restrict__ out_stats,
    float* __restrict__ out_lstats, int* __restrict__ out_mleft) {
    __shared__ float s_best_gain[256 / WAVE];
    __shared__ int s_best_feat[256 / WAVE];
    __shared__ int s_best_bin[256 / WAVE];
    __shared__ float s_best_wl[256 / WAVE];
    __shared__ int s_best_ml[MISSING ? 256 / WAVE : 1];
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
    if (lane == 0) {
        s_best_gain[wid] = best_gain;
        s_best_feat[wid] = best_feat;
        s_best_bin[wid] = best_bin;
        s_best_wl[wid] = best_wl;
        if (MISSING) s_best_ml[wid] = best_ml;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w2 = 1; w2 < (int)(blockDim.x / WAVE); ++w2) {
            const float og = s_best_gain[w2];
            const int of = s_best_feat[w2];
            const bool take = (og > s_best_gain[0] + 1e-12f) ||
                              (og > s_best_gain[0] - 1e-12f && of >= 0 &&
                               (s_best_feat[0] < 0 ||
                                of < s_best_feat[0] ||
                                (of == s_best_feat[0] &&
                                 s_best_bin[w2] < s_best_bin[0])));
            if (take) {
                s_best_gain[0] = og;
                s_best_feat[0] = of;
                s_best_bin[0] = s_best_bin[w2];
                s_best_wl[0] = s_best_wl[w2];
                if (MISSING) s_best_ml[0] = s_best_ml[w2];
            }
        }
        out_feat[node] = s_best_gain[0] > 0.f ? s_best_feat[0] : -1;
        out_bin[node] = s_best_bin[0];
        out_wl[node] = s_best_wl[0];
        out_gain[node] = s_best_gain[0];
        out_imp[node] = imp_p;
        if (MISSING)
            out_mleft[node] = s_best_gain[0] > 0.f ? s_best_ml[0] : 0;
    }
    for (int c = tid; c < S; c += blockDim.x)
        out_stats[(long long)node * S + c] = s_parent[c];
    __syncthreads();
    // left stats of the winning split (prefix sum over its bins, then the
    // missing bin when it goes left: all zeros there on a majority flag)
    const int wf = (s_best_gain[0] > 0.f) ? s_best_feat[0] : -1;
    for (int c = tid; c < S; c += blockDim.x) {
        float acc = 0.f;
        if (wf >= 0) {
            const float* Hw = H + (long long)wf * nbins * S;
            const int wb = s_best_bin[0];
            for (int b = 0; b <= wb; ++b) acc += Hw[b * S + c];
            if (MISSING && s_best_ml[0]) acc += Hw[(nbins - 1) * S + c];
        }
        out_lstats[(long long)node * S + c] = acc;
    }
}

template <bool COUNTED, bool MISSING>
static __device__ __forceinline__ void tree_split_body(
    const float* __restrict__ hist,        // [NF][f][nbins][S]
    const unsigned* __restrict__ node_seed,  // [NF]
    int f, int nbins, int S, int is_cls, int crit, int m_features,
    int extra_mode, float min_leaf_w,
    int* __restrict__ out_feat,   // [NF]  (-1 = no valid split)
    int* __restrict__ out_bin,    // [NF]
    float* __restrict__ out_wl,   // [NF]  left weighted count
    float* __restrict__ out_gain, // [NF]  impurity improvement (unscaled)
    float* __restrict__ out_imp,  // [NF]  parent impurity
    float* __restrict__ out_stats,  // [NF][S] parent stat totals
    float* __restrict__ out_lstats, // [NF][S] winning split's left stats
    int cnt_stat,
    int* __restrict__ out_mleft) {  // [NF] (MISSING) 1 = missing rows go left
    const int node = blockIdx.x;
    const unsigned seed = node_seed[node];
    const float* H = hist + (long long)node * f * nbins * S;
    const int tid = threadIdx.x;

    __shared__ float s_parent[36];     // S <= 32 stats + pad

    // parent totals from feature 0's histogram
    for (int c = tid; c < S; c += blockDim.x) s_parent[c] = 0.f;
    __syncthreads();
    for (int i = tid; i < nbins * S; i += blockDim.x)
        atomicAdd(&s_parent[i % S], H[i]);
    __syncthreads();
    float wp = 0.f;
    if (is_cls) {
        for (int c = 0; c < S; ++c) wp += s_parent[c];
    } else {
        wp = s_parent[0];
    }
    const float imp_p = impurity(s_parent, wp, S, is_cls, crit);

    unsigned h_thresh = 0xffffffffu;
    if (m_features < f) h_thresh = feat_hash_threshold(seed, f, m_features);

    // per-thread best over its features
    float best_gain = -1.f;
    int best_feat = -1, best_bin = -1;
    float best_wl = 0.f;
    int best_ml = 0;
    float left[36];
    float miss[MISSING ? 36 : 1];   // the feature's missing-bin stats
    float lm[MISSING ? 36 : 1];     // left + miss: the L candidate
    for (int j = tid; j < f; j += blockDim.x) {
        if (m_features < f &&
            wang_hash(seed ^ (unsigned)(j * 2654435761u)) > h_thresh)
            continue;
        const float* Hj = H + (long long)j * nbins * S;
        // ExtraTrees: pick one random bin in the node's occupied range
        int rand_bin = -1;
        if (extra_mode) {
            int lo = -1, hi = -1;
            for (int b = 0; b < nbins; ++b) {
                float wb = 0.f;
                if (is_cls) {
                    for (int c = 0; c < S; ++c) wb += Hj[b * S + c];
                } else {
                    wb = Hj[b * S];
                }
                if (wb > 0.f) {
                    if (lo < 0) lo = b;
                    hi = b;
                }
            }
            if (lo < 0 || hi <= lo) continue;  // constant feature here
            const unsigned r = wang_hash(seed ^ 0x9e3779b9u ^
                                         (unsigned)(j * 40503u));
            rand_bin = lo + (int)(r % (unsigned)(hi - lo));  // in [lo, hi)
        }
        for (int c = 0; c < S; ++c) left[c] = 0.f;
        float wl = 0.f;
        float wm = 0.f;
        if (MISSING) {
            // read once per feature, not per bin
            for (int c = 0; c < S; ++c) miss[c] = Hj[(nbins - 1) * S + c];
            if (is_cls) {
                for (int c = 0; c < S; ++c) wm += miss[c];
            } else {
                wm = miss[0];
            }
        }
        for (int b = 0; b < nbins - 1; ++b) {
            for (int c = 0; c < S; ++c) left[c] += Hj[b * S + c];
            if (is_cls) {
                wl = 0.f;
                for (int c = 0; c < S; ++c) wl += left[c];
            } else {
                wl = left[0];
            }
            if (extra_mode && b != rand_bin) continue;
            float gain;
            if (split_candidate<COUNTED>(left, wl, s_parent, wp, imp_p, S,
                                         is_cls, crit, min_leaf_w, cnt_stat,
                                         &gain)) {
                // deterministic tie-break: larger gain, then lower
                // feature/bin
                if (gain > best_gain + 1e-12f) {
                    best_gain = gain;
                    best_feat = j;
                    best_bin = b;
                    best_wl = wl;
                    // no missing weight here: majority side
                    if (MISSING) best_ml = (!(wm > 0.f) && wl + wl > wp);
                }
            }
            if (MISSING && wm > 0.f) {
                float wlm = 0.f;
                for (int c = 0; c < S; ++c) lm[c] = left[c] + miss[c];
                if (is_cls) {
                    for (int c = 0; c < S; ++c) wlm += lm[c];
                } else {
                    wlm = lm[0];
                }
                if (split_candidate<COUNTED>(lm, wlm, s_parent, wp, imp_p,
                                             S, is_cls, crit, min_leaf_w,
                                             cnt_stat, &gain) &&
                    gain > best_gain + 1e-12f) {
                    best_gain = gain;
                    best_feat = j;
                    best_bin = b;
                    best_wl = wlm;
                    best_ml = 1;
                }
            }
        }
    }

    // wave then block argmax reduce (lower (feat,bin) wins ties)
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const float og = __shfl_down(best_gain, off);
        const int of = __shfl_down(best_feat, off);
        const int ob = __shfl_down(best_bin, off);
        const float owl = __shfl_down(best_wl, off);
        const int oml = MISSING ? __shfl_down(best_ml, off) : 0;
        const bool take = (og > best_gain + 1e-12f) ||
                          (og > best_gain - 1e-12f && of >= 0 &&
                           (best_feat < 0 || of < best_feat ||
                            (of == best_feat && ob < best_bin)));
        if (take) {
            best_gain = og; best_feat = of; best_bin = ob; best_wl = owl;
            best_ml = oml;
        }
    }
    split_block_finish<MISSING>(best_gain, best_feat, best_bin, best_wl,
                                best_ml, s_parent, imp_p, H, node, nbins, S,
                                out_feat, out_bin, out_wl, out_gain, out_imp,
                                out_stats, out_lstats, out_mleft);
}

// ---------------------------------------------------------------------- //
// K2 wide: classification with 32 < S <= 256 — 256 threads per frontier
// node, ONE WAVE PER FEATURE.  Wave w scans the w-th contiguous quarter of
// the features, in order: the block ending keeps the earlier wave's
// candidate when two gains are exactly equal, which is then the lower
// feature, as in the narrow scan (features identical within the node are
// common once a node holds two or three separable classes).  Lane l owns
// the classes l, l+64, l+128, l+192: at most WIDE_K running left counts (and
// missing-bin counts) per lane, and per bin one coalesced load of
// H[j][b][.] along S.  Everything summed over the classes is a wave
// reduction (xor butterfly: a fixed order, the same value in every lane), so
// the scan's control flow is wave-uniform.  Candidates, validity, gain,
// subsample, ExtraTrees bin and tie order are tree_split_body's.
// ---------------------------------------------------------------------- //
#define WIDE_S 256
#define WIDE_K (WIDE_S / WAVE)

static __device__ __forceinline__ float wave_sum(float v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// impurity() over a stats vector spread across the wave (s = this lane's
// WIDE_K classes, zero past S); w is the vector's total
static __device__ __forceinline__ float
impurity_wide(const float* s, float w, int crit) {
    if (w <= 0.f) return 0.f;
    float a = 0.f;
    if (crit == CRIT_GINI) {
#pragma unroll
        for (int k = 0; k < WIDE_K; ++k) a += s[k] * s[k];
        return 1.f - wave_sum(a) / (w * w);
    }
#pragma unroll
    for (int k = 0; k < WIDE_K; ++k) {
        if (s[k] > 0.f) {
            const float p = s[k] / w;
            a -= p * __log2f(p);
        }
    }
    return wave_sum(a);
}

// split_candidate<false> on lane-sliced stats
static __device__ __forceinline__ bool split_candidate_wide(
    const float* left, float wl, const float* parent, float wp, float imp_p,
    int crit, float min_leaf_w, float* gain_out) {
    const float wr = wp - wl;
    if (wl < min_leaf_w || wr < min_leaf_w) return false;
    const float imp_l = impurity_wide(left, wl, crit);
    float right[WIDE_K];
#pragma unroll
    for (int k = 0; k < WIDE_K; ++k) right[k] = parent[k] - left[k];
    const float imp_r = impurity_wide(right, wr, crit);
    *gain_out = imp_p - (wl * imp_l + wr * imp_r) / wp;
    return true;
}

template <bool MISSING>
static __device__ __forceinline__ void tree_split_wide_body(
    const float* __restrict__ hist,        // [NF][f][nbins][S]
    const unsigned* __restrict__ node_seed,  // [NF]
    int f, int nbins, int S, int crit, int m_features, int extra_mode,
    float min_leaf_w, int* __restrict__ out_feat, int* __restrict__ out_bin,
    float* __restrict__ out_wl, float* __restrict__ out_gain,
    float* __restrict__ out_imp, float* __restrict__ out_stats,
    float* __restrict__ out_lstats, int* __restrict__ out_mleft) {
    const int node = blockIdx.x;
    const unsigned seed = node_seed[node];
    const float* H = hist + (long long)node * f * nbins * S;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;

    __shared__ float s_parent[WIDE_S];

    // parent totals from feature 0's histogram: thread c sums class c
    for (int c = tid; c < WIDE_S; c += blockDim.x) {
        float acc = 0.f;
        if (c < S)
            for (int b = 0; b < nbins; ++b) acc += H[b * S + c];
        s_parent[c] = acc;
    }
    __syncthreads();
    float parent[WIDE_K];
    float wsum = 0.f;
#pragma unroll
    for (int k = 0; k < WIDE_K; ++k) {
        parent[k] = s_parent[lane + k * WAVE];
        wsum += parent[k];
    }
    const float wp = wave_sum(wsum);
    const float imp_p = impurity_wide(parent, wp, crit);

    unsigned h_thresh = 0xffffffffu;
    if (m_features < f) h_thresh = feat_hash_threshold(seed, f, m_features);

    // per-wave best over its features (the same value in every lane)
    float best_gain = -1.f;
    int best_feat = -1, best_bin = -1;
    float best_wl = 0.f;
    int best_ml = 0;
    float left[WIDE_K];
    float miss[MISSING ? WIDE_K : 1];   // the feature's missing-bin stats
    float lm[MISSING ? WIDE_K : 1];     // left + miss: the L candidate
    const int n_waves = blockDim.x / WAVE;
    const int per_wave = (f + n_waves - 1) / n_waves;
    const int j_end = min(f, (wid + 1) * per_wave);
    for (int j = wid * per_wave; j < j_end; ++j) {
        if (m_features < f &&
            wang_hash(seed ^ (unsigned)(j * 2654435761u)) > h_thresh)
            continue;
        const float* Hj = H + (long long)j * nbins * S;
        // ExtraTrees: pick one random bin in the node's occupied range (a
        // bin of non-negative counts holds weight iff some class does)
        int rand_bin = -1;
        if (extra_mode) {
            int lo = -1, hi = -1;
            for (int b = 0; b < nbins; ++b) {
                bool occ = false;
#pragma unroll
                for (int k = 0; k < WIDE_K; ++k) {
                    const int c = lane + k * WAVE;
                    if (c < S && Hj[b * S + c] > 0.f) occ = true;
                }
                if (__any(occ)) {
                    if (lo < 0) lo = b;
                    hi = b;
                }
            }
            if (lo < 0 || hi <= lo) continue;  // constant feature here
            const unsigned r = wang_hash(seed ^ 0x9e3779b9u ^
                                         (unsigned)(j * 40503u));
            rand_bin = lo + (int)(r % (unsigned)(hi - lo));  // in [lo, hi)
        }
#pragma unroll
        for (int k = 0; k < WIDE_K; ++k) left[k] = 0.f;
        float wm = 0.f;
        if (MISSING) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < WIDE_K; ++k) {
                const int c = lane + k * WAVE;
                miss[k] = c < S ? Hj[(nbins - 1) * S + c] : 0.f;
                s += miss[k];
            }
            wm = wave_sum(s);
        }
        // the ExtraTrees cut needs the prefix up to its one bin only
        const int b_end = extra_mode ? rand_bin + 1 : nbins - 1;
        for (int b = 0; b < b_end; ++b) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < WIDE_K; ++k) {
                const int c = lane + k * WAVE;
                if (c < S) left[k] += Hj[b * S + c];
                s += left[k];
            }
            if (extra_mode && b != rand_bin) continue;
            const float wl = wave_sum(s);
            float gain;
            if (split_candidate_wide(left, wl, parent, wp, imp_p, crit,
                                     min_leaf_w, &gain)) {
                if (gain > best_gain + 1e-12f) {
                    best_gain = gain;
                    best_feat = j;
                    best_bin = b;
                    best_wl = wl;
                    // no missing weight here: majority side
                    if (MISSING) best_ml = (!(wm > 0.f) && wl + wl > wp);
                }
            }
            if (MISSING && wm > 0.f) {
                float sm = 0.f;
#pragma unroll
                for (int k = 0; k < WIDE_K; ++k) {
                    lm[k] = left[k] + miss[k];
                    sm += lm[k];
                }
                const float wlm = wave_sum(sm);
                if (split_candidate_wide(lm, wlm, parent, wp, imp_p, crit,
                                         min_leaf_w, &gain) &&
                    gain > best_gain + 1e-12f) {
                    best_gain = gain;
                    best_feat = j;
                    best_bin = b;
                    best_wl = wlm;
                    best_ml = 1;
                }
            }
        }
    }
    split_block_finish<MISSING>(best_gain, best_feat, best_bin, best_wl,
                                best_ml, s_parent, imp_p, H, node, nbins, S,
                                out_feat, out_bin, out_wl, out_gain, out_imp,
                                out_stats, out_lstats, out_mleft);
}

extern "C" __global__ __launch_bounds__(256) void k_tree_split_wide(
    const float* __restrict__ hist, const unsigned* __restrict__ node_seed,
    int f, int nbins, int S, int crit, int m_features, int extra_mode,
    float min_leaf_w, int* __restrict__ out_feat, int* __restrict__ out_bin,
    float* __restrict__ out_wl, float* __restrict__ out_gain,
    float* __restrict__ out_imp, float* __restrict__ out_stats,
    float* __restrict__ out_lstats) {
    tree_split_wide_body<false>(hist, node_seed, f, nbins, S, crit,
                                m_features, extra_mode, min_leaf_w, out_feat,
                                out_bin, out_wl, out_gain, out_imp,
                                out_stats, out_lstats, nullptr);
}

extern "C" __global__ __launch_bounds__(256) void k_tree_split_wide_m(
    const float* __restrict__ hist, const unsigned* __restrict__ node_seed,
    int f, int nbins, int S, int crit, int m_features, float min_leaf_w,
    int* __restrict__ out_feat, int* __restrict__ out_bin,
    float* __restrict__ out_wl, float* __restrict__ out_gain,
    float* __restrict__ out_imp, float* __restrict__ out_stats,
    float* __restrict__ out_lstats, int* __restrict__ out_mleft) {
    tree_split_wide_body<true>(hist, node_seed, f, nbins, S, crit,
                               m_features, 0, min_leaf_w, out_feat, out_bin,
                               out_wl, out_gain, out_imp, out_stats,
                               out_lstats, out_mleft);
}

extern "C" __global__ __launch_bounds__(256) void k_tree_split(
    const float* __restrict__ hist, const unsigned* __restrict__ node_seed,
    int f, int nbins, int S, int is_cls, int crit, int m_features,
    int extra_mode, float min_leaf_w, int* __restrict__ out_feat,
    int* __restrict__ out_bin, float* __restrict__ out_wl,
    float* __restrict__ out_gain, float* __restrict__ out_imp,
    float* __restrict__ out_stats, float* __restrict__ out_lstats) {
    tree_split_body<false, false>(hist, node_seed, f, nbins, S, is_cls,
                                  crit, m_features, extra_mode, min_leaf_w,
                                  out_feat, out_bin, out_wl, out_gain,
                                  out_imp, out_stats, out_lstats, -1,
                                  nullptr);
}

// min_leaf_w is a row-count threshold here; cnt_stat in [0, S)
extern "C" __global__ __launch_bounds__(256) void k_tree_split_w(
    const float* __restrict__ hist, const unsigned* __restrict__ node_seed,
    int f, int nbins, int S, int is_cls, int crit, int m_features,
    int extra_mode, float min_leaf_w, int* __restrict__ out_feat,
    int* __restrict__ out_bin, float* __restrict__ out_wl,
    float* __restrict__ out_gain, float* __restrict__ out_imp,
    float* __restrict__ out_stats, float* __restrict__ out_lstats,
    int cnt_stat) {
    tree_split_body<true, false>(hist, node_seed, f, nbins, S, is_cls, crit,
                                 m_features, extra_mode, min_leaf_w,
                                 out_feat, out_bin, out_wl, out_gain,
                                 out_imp, out_stats, out_lstats, cnt_stat,
                                 nullptr);
}

// the MISSING instantiations: bin nbins-1 is the missing bin, no ExtraTrees
extern "C" __global__ __launch_bounds__(256) void k_tree_split_m(
    const float* __restrict__ hist, const unsigned* __restrict__ node_seed,
    int f, int nbins, int S, int is_cls, int crit, int m_features,
    float min_leaf_w, int* __restrict__ out_feat,
    int* __restrict__ out_bin, float* __restrict__ out_wl,
    float* __restrict__ out_gain, float* __restrict__ out_imp,
    float* __restrict__ out_stats, float* __restrict__ out_lstats,
    int* __restrict__ out_mleft) {
    tree_split_body<false, true>(hist, node_seed, f, nbins, S, is_cls, crit,
                                 m_features, 0, min_leaf_w, out_feat,
                                 out_bin, out_wl, out_gain, out_imp,
                                 out_stats, out_lstats, -1, out_mleft);
}

extern "C" __global__ __launch_bounds__(256) void k_tree_split_wm(
    const float* __restrict__ hist, const unsigned* __restrict__ node_seed,
    int f, int nbins, int S, int is_cls, int crit, int m_features,
    float min_leaf_w, int* __restrict__ out_feat,
    int* __restrict__ out_bin, float* __restrict__ out_wl,
    float* __restrict__ out_gain, float* __restrict__ out_imp,
    float* __restrict__ out_stats, float* __restrict__ out_lstats,
    int cnt_stat, int* __restrict__ out_mleft) {
    tree_split_body<true, true>(hist, node_seed, f, nbins, S, is_cls, crit,
                                m_features, 0, min_leaf_w, out_feat,
                                out_bin, out_wl, out_gain, out_imp,
                                out_stats, out_lstats, cnt_stat, out_mleft);
}

// ---------------------------------------------------------------------- //
// K3: per-chunk left counts (split nodes only)
// chunks here carry {part_slot, tree_slot, row_start, row_count}
// ---------------------------------------------------------------------- //
// The one partition predicate of K3 and K4: a row goes left iff
// code <= b || (mleft && code == missing_code).  split_mleft is nullable
// (no slot sends its missing rows left); a slot whose flag is 0 gets the
// impossible code -1, so the row test stays two compares.
struct PartSplit {
    int jf, b, miss;
    __device__ __forceinline__ PartSplit(const int* split_feat,
                                         const int* split_bin,
                                         const int* split_mleft,
                                         int part_slot, int missing_code)
        : jf(split_feat[part_slot]), b(split_bin[part_slot]),
          miss((split_mleft != nullptr && split_mleft[part_slot] != 0)
                   ? missing_code : -1) {}
    __device__ __forceinline__ bool left(const unsigned char* codes,
                                         long long i, int fp) const {
        const int c = codes[i * fp + jf];
        return c <= b || c == miss;
    }
};

extern "C" __global__ __launch_bounds__(256) void k_part_count(
    const unsigned char* __restrict__ codes, const int* __restrict__ sample_idx,
    const int* __restrict__ chunks, const int* __restrict__ split_feat,
    const int* __restrict__ split_bin, const int* __restrict__ split_mleft,
    int missing_code, long long n, int fp, int* __restrict__ out_counts) {
    const int chunk = blockIdx.x;
    const int part_slot = chunks[chunk * 4 + 0];
    const int tree_slot = chunks[chunk * 4 + 1];
    const int row_start = chunks[chunk * 4 + 2];
    const int row_count = chunks[chunk * 4 + 3];
    const PartSplit sp(split_feat, split_bin, split_mleft, part_slot,
                       missing_code);
    const int* si = sample_idx + (long long)tree_slot * n + row_start;
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int cnt = 0;
    for (int r = threadIdx.x; r < row_count; r += blockDim.x)
        if (sp.left(codes, si[r], fp)) ++cnt;
    atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) out_counts[chunk] = s_cnt;
}

// ---------------------------------------------------------------------- //
// K4: stable partition scatter
// left_base/right_base: absolute output offsets (into the tree's row of
// sample_idx_out) for this chunk's first left / right element.
// ---------------------------------------------------------------------- //
extern "C" __global__ __launch_bounds__(256) void k_part_scatter(
    const unsigned char* __restrict__ codes,
    const int* __restrict__ sample_idx_in, const int* __restrict__ chunks,
    const int* __restrict__ split_feat, const int* __restrict__ split_bin,
    const int* __restrict__ split_mleft, int missing_code,
    const int* __restrict__ left_base, const int* __restrict__ right_base,
    long long n, int fp, int* __restrict__ sample_idx_out) {
    const int chunk = blockIdx.x;
    const int part_slot = chunks[chunk * 4 + 0];
    const int tree_slot = chunks[chunk * 4 + 1];
    const int row_start = chunks[chunk * 4 + 2];
    const int row_count = chunks[chunk * 4 + 3];
    const PartSplit sp(split_feat, split_bin, split_mleft, part_slot,
                       missing_code);
    const int* si = sample_idx_in + (long long)tree_slot * n + row_start;
    int* so = sample_idx_out + (long long)tree_slot * n;

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
    __shared__ int s_wave_tot[256 / WAVE];
    __shared__ int s_run[2];  // running left / right within this chunk
    if (tid == 0) { s_run[0] = 0; s_run[1] = 0; }
    __syncthreads();

    for (int tile = 0; tile < row_count; tile += blockDim.x) {
        const int r = tile + tid;
        const bool valid = r < row_count;
        int i = 0;
        bool p = false;
        if (valid) {
            i = si[r];
            p = sp.left(codes, i, fp);
        }
        const unsigned long long mask = __ballot(p);
        const int before =
            __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == WAVE - 1) s_wave_tot[wid] = before + (p ? 1 : 0);
        __syncthreads();
        int wave_off = 0;
        for (int w2 = 0; w2 < wid; ++w2) wave_off += s_wave_tot[w2];
        int tile_l = 0;
        for (int w2 = 0; w2 < (int)(blockDim.x / WAVE); ++w2)
            tile_l += s_wave_tot[w2];
        const int lpre = before + wave_off;
        if (valid) {
            if (p)
                so[left_base[chunk] + s_run[0] + lpre] = i;
            else
                so[right_base[chunk] + s_run[1] + (tid - lpre)] = i;
        }
        __syncthreads();
        if (tid == 0) {
            const int vcnt = min((int)blockDim.x, row_count - tile);
            s_run[0] += tile_l;
            s_run[1] += vcnt - tile_l;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------- //
// C launchers
// ---------------------------------------------------------------------- //
extern "C" hipError_t skdist_tree_hist(
    const void* codes, const void* y_int, const void* y_f,
    const void* row_w, const void* weights, const void* sample_idx,
    const void* chunks, void* hist, long long n, int f, int fp, int nbins,
    int S, int fg, int cg, int n_chunks, hipStream_t stream) {
    if (n_chunks <= 0) return hipSuccess;
    if (cg < 0 || S <= 0) return hipErrorInvalidValue;
    // the tile's stat width: all S stats, or one class group
    const int tile_s = cg > 0 && cg < S ? cg : S;
    const size_t lds = (size_t)fg * nbins * tile_s * sizeof(float);
    if (fg <= 0 || f <= 0 || fp % 4 != 0 || f > fp || nbins <= 0 ||
        nbins > 256 || lds > 64 * 1024)
        return hipErrorInvalidValue;
    // exactly one target; row_w rides the regression stats only (S = 4)
    if ((y_int != nullptr) == (y_f != nullptr) ||
        (row_w != nullptr && (y_f == nullptr || S != 4)))
        return hipErrorInvalidValue;
    // class groups split class counts only
    const int n_cg = cg > 0 ? (S + cg - 1) / cg : 1;
    if (cg > 0 && (y_int == nullptr || row_w != nullptr || n_cg > 65535))
        return hipErrorInvalidValue;
    const dim3 grid(n_chunks, (f + fg - 1) / fg, n_cg);
    if (cg > 0)
        hipLaunchKernelGGL(k_tree_hist_cg, grid, dim3(256), lds, stream,
                           (const unsigned char*)codes, (const int*)y_int,
                           (const unsigned char*)weights,
                           (const int*)sample_idx, (const int*)chunks,
                           (float*)hist, n, f, fp, nbins, S, fg, cg);
    else if (row_w != nullptr)
        hipLaunchKernelGGL(k_tree_hist_w, grid, dim3(256), lds, stream,
                           (const unsigned char*)codes, (const float*)y_f,
                           (const float*)row_w,
                           (const unsigned char*)weights,
                           (const int*)sample_idx, (const int*)chunks,
                           (float*)hist, n, f, fp, nbins, fg);
    else
        hipLaunchKernelGGL(k_tree_hist, grid, dim3(256), lds, stream,
                           (const unsigned char*)codes, (const int*)y_int,
                           (const float*)y_f,
                           (const unsigned char*)weights,
                           (const int*)sample_idx, (const int*)chunks,
                           (float*)hist, n, f, fp, nbins, S,
                           (int)(y_int != nullptr), fg);
    return hipGetLastError();
}

extern "C" hipError_t skdist_tree_split(
    const void* hist, const void* node_seed, int n_frontier, int f,
    int nbins, int S, int is_cls, int crit, int m_features, int extra_mode,
    float min_leaf, int cnt_stat, void* out_feat, void* out_bin,
    void* out_wl, void* out_gain, void* out_imp, void* out_stats,
    void* out_lstats, int missing, void* out_mleft, hipStream_t stream) {
    if (n_frontier <= 0) return hipSuccess;
    if (S <= 0 || S > WIDE_S || cnt_stat >= S) return hipErrorInvalidValue;
    // above 32 stats only the class-count scan exists (the counted variant
    // is a regression one)
    const bool wide = S > 32;
    if (wide && (!is_cls || cnt_stat >= 0)) return hipErrorInvalidValue;
    // the missing scan needs a present bin below the missing one, its own
    // output, and has no ExtraTrees mode
    if (missing && (nbins < 2 || out_mleft == nullptr || extra_mode))
        return hipErrorInvalidValue;
    if (wide) {
        // one wave per feature, four waves with a quarter of them each
        const dim3 grid(n_frontier), block(256);
        if (missing)
            hipLaunchKernelGGL(k_tree_split_wide_m, grid, block, 0, stream,
                               (const float*)hist,
                               (const unsigned*)node_seed, f, nbins, S, crit,
                               m_features, min_leaf, (int*)out_feat,
                               (int*)out_bin, (float*)out_wl,
                               (float*)out_gain, (float*)out_imp,
                               (float*)out_stats, (float*)out_lstats,
                               (int*)out_mleft);
        else
            hipLaunchKernelGGL(k_tree_split_wide, grid, block, 0, stream,
                               (const float*)hist,
                               (const unsigned*)node_seed, f, nbins, S, crit,
                               m_features, extra_mode, min_leaf,
                               (int*)out_feat, (int*)out_bin, (float*)out_wl,
                               (float*)out_gain, (float*)out_imp,
                               (float*)out_stats, (float*)out_lstats);
        return hipGetLastError();
    }
    // per-node parallelism is one thread per feature: size the block to
    // f so low-f datasets don't idle 3/4 of each workgroup
    const int threads = f >= 192 ? 256 : (f >= 96 ? 128 : 64);
    const dim3 grid(n_frontier), block(threads);
    if (missing && cnt_stat < 0)
        hipLaunchKernelGGL(k_tree_split_m, grid, block, 0, stream,
                           (const float*)hist, (const unsigned*)node_seed,
                           f, nbins, S, is_cls, crit, m_features, min_leaf,
                           (int*)out_feat, (int*)out_bin, (float*)out_wl,
                           (float*)out_gain, (float*)out_imp,
                           (float*)out_stats, (float*)out_lstats,
                           (int*)out_mleft);
    else if (missing)
        hipLaunchKernelGGL(k_tree_split_wm, grid, block, 0, stream,
                           (const float*)hist, (const unsigned*)node_seed,
                           f, nbins, S, is_cls, crit, m_features, min_leaf,
                           (int*)out_feat, (int*)out_bin, (float*)out_wl,
                           (float*)out_gain, (float*)out_imp,
                           (float*)out_stats, (float*)out_lstats, cnt_stat,
                           (int*)out_mleft);
    else if (cnt_stat < 0)
        hipLaunchKernelGGL(k_tree_split, grid, block, 0,
                           stream, (const float*)hist,
                           (const unsigned*)node_seed, f, nbins, S, is_cls,
                           crit, m_features, extra_mode, min_leaf,
                           (int*)out_feat, (int*)out_bin, (float*)out_wl,
                           (float*)out_gain, (float*)out_imp,
                           (float*)out_stats, (float*)out_lstats);
    else
        hipLaunchKernelGGL(k_tree_split_w, grid, block,
                           0, stream, (const float*)hist,
                           (const unsigned*)node_seed, f, nbins, S, is_cls,
                           crit, m_features, extra_mode, min_leaf,
                           (int*)out_feat, (int*)out_bin, (float*)out_wl,
                           (float*)out_gain, (float*)out_imp,
                           (float*)out_stats, (float*)out_lstats, cnt_stat);
    return hipGetLastError();
}

// split_mleft == nullptr: no slot sends its missing rows left (then
// missing_code is not read); else missing_code is a uint8 code
extern "C" hipError_t skdist_part_count(
    const void* codes, const void* sample_idx, const void* chunks,
    const void* split_feat, const void* split_bin, const void* split_mleft,
    int missing_code, long long n, int fp, int n_chunks, void* out_counts,
    hipStream_t stream) {
    if (n_chunks <= 0) return hipSuccess;
    if (split_mleft != nullptr && (missing_code < 0 || missing_code > 255))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_part_count, dim3(n_chunks), dim3(256), 0, stream,
                       (const unsigned char*)codes, (const int*)sample_idx,
                       (const int*)chunks, (const int*)split_feat,
                       (const int*)split_bin, (const int*)split_mleft,
                       missing_code, n, fp, (int*)out_counts);
    return hipGetLastError();
}

extern "C" hipError_t skdist_part_scatter(
    const void* codes, const void* sample_idx_in, const void* chunks,
    const void* split_feat, const void* split_bin, const void* split_mleft,
    int missing_code, const void* left_base, const void* right_base,
    long long n, int fp, int n_chunks, void* sample_idx_out,
    hipStream_t stream) {
    if (n_chunks <= 0) return hipSuccess;
    if (split_mleft != nullptr && (missing_code < 0 || missing_code > 255))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_part_scatter, dim3(n_chunks), dim3(256), 0,
                       stream, (const unsigned char*)codes,
                       (const int*)sample_idx_in, (const int*)chunks,
                       (const int*)split_feat, (const int*)split_bin,
                       (const int*)split_mleft, missing_code,
                       (const int*)left_base, (const int*)right_base, n,
                       fp, (int*)sample_idx_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------- //
// K0: CSR -> uint8 codes (BinnedDataset on a scipy-sparse X)
// grid: grid-stride over rows, one row per workgroup pass; block 256
//
//   zc4    [fp/4]       the row pattern of a cell with no stored entry
//                       (zero_code[j] = #edges[j] < 0.0, pad columns 0),
//                       packed 4 codes per 32-bit word
//   edges  [f][nbins-1] f32 ascending per feature
//   indptr [n+1] int64, indices [nnz] int32, data [nnz] f32 (no duplicate
//   (row, col) pairs: the host sums them before upload)
//
// Pass 1 fills the row with the zero pattern in 4-byte stores (fp % 4 == 0
// keeps every row base aligned); after the barrier pass 2 overwrites each
// stored cell with its own code = #edges[col] strictly less than the value
// (lower bound), so a stored 0.0 lands on zero_code again.
// ---------------------------------------------------------------------- //
extern "C" __global__ __launch_bounds__(256) void k_bin_csr(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const float* __restrict__ edges,
    const unsigned* __restrict__ zc4, unsigned char* __restrict__ codes,
    long long n, long long nnz, int f, int fp, int nedges) {
    const int fp4 = fp >> 2;
    for (long long r = blockIdx.x; r < n; r += gridDim.x) {
        unsigned char* crow = codes + r * (long long)fp;
        unsigned* crow4 = (unsigned*)crow;
        for (int q = threadIdx.x; q < fp4; q += blockDim.x)
            crow4[q] = zc4[q];
        __syncthreads();
        long long lo = indptr[r], hi = indptr[r + 1];
        if (lo < 0) lo = 0;
        if (hi > nnz) hi = nnz;
        for (long long k = lo + threadIdx.x; k < hi; k += blockDim.x) {
            const int col = indices[k];
            if ((unsigned)col >= (unsigned)f) continue;
            const float v = data[k];
            const float* e = edges + (long long)col * nedges;
            int a = 0, b = nedges;       // first index with e[idx] >= v
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (e[mid] < v) a = mid + 1; else b = mid;
            }
            crow[col] = (unsigned char)a;
        }
        // the next row of this workgroup is a different address range,
        // so no second barrier is needed
    }
}

extern "C" hipError_t skdist_bin_csr(
    const void* indptr, const void* indices, const void* data,
    const void* edges, const void* zc4, void* codes, long long n,
    long long nnz, int f, int fp, int nedges, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (fp % 4 != 0 || f > fp || nedges < 0 || nedges > 255)
        return hipErrorInvalidValue;
    const int blocks = (int)(n < 16384 ? n : 16384);
    hipLaunchKernelGGL(k_bin_csr, dim3(blocks), dim3(256), 0, stream,
                       (const long long*)indptr, (const int*)indices,
                       (const float*)data, (const float*)edges,
                       (const unsigned*)zc4, (unsigned char*)codes, n, nnz,
                       f, fp, nedges);
    return hipGetLastError();
}
