// C launchers of the tree family: included by tree_kernels.hip and
// predict_kernels.hip, which define them, and by bindings.cpp, which calls
// them, so the compiler checks each signature on both sides.
#pragma once

#include <hip/hip_runtime.h>

extern "C" {
// row_w == nullptr: class counts (y_int) or (w, wy, wyy) (y_f);
// row_w != nullptr: (W, Wy, Wyy, C) over y_f, S must be 4.
// cg == 0: one LDS tile of fg * nbins * S floats per block; cg > 0 (class
// counts only): the classes go in groups of cg over grid.z and the tile is
// fg * nbins * min(cg, S) floats.  The tile must fit 64 KiB either way
hipError_t skdist_tree_hist(
    const void* codes, const void* y_int, const void* y_f,
    const void* row_w, const void* weights, const void* sample_idx,
    const void* chunks, void* hist, long long n, int f, int fp, int nbins,
    int S, int fg, int cg, int n_chunks, hipStream_t stream);
// cnt_stat < 0: min-leaf on the weight sums; else on the stat cnt_stat.
// S <= 32: any stats; 32 < S <= 256: class counts only (is_cls, cnt_stat
// < 0), scanned by the wave-per-feature kernels.
// missing != 0: bin nbins-1 is the missing bin, both directions are
// scanned and out_mleft [n_frontier] int32 gets the learned one (no
// extra_mode); missing == 0: out_mleft is not touched and may be null
hipError_t skdist_tree_split(
    const void* hist, const void* node_seed, int n_frontier, int f,
    int nbins, int S, int is_cls, int crit, int m_features, int extra_mode,
    float min_leaf, int cnt_stat, void* out_feat, void* out_bin,
    void* out_wl, void* out_gain, void* out_imp, void* out_stats,
    void* out_lstats, int missing, void* out_mleft, hipStream_t stream);
// split_mleft: nullable int32 per part_slot; a set flag sends the rows
// whose code is missing_code left as well
hipError_t skdist_part_count(
    const void* codes, const void* sample_idx, const void* chunks,
    const void* split_feat, const void* split_bin, const void* split_mleft,
    int missing_code, long long n, int fp, int n_chunks, void* out_counts,
    hipStream_t stream);
hipError_t skdist_part_scatter(
    const void* codes, const void* sample_idx_in, const void* chunks,
    const void* split_feat, const void* split_bin, const void* split_mleft,
    int missing_code, const void* left_base, const void* right_base,
    long long n, int fp, int n_chunks, void* sample_idx_out,
    hipStream_t stream);
hipError_t skdist_bin_csr(
    const void* indptr, const void* indices, const void* data,
    const void* edges, const void* zc4, void* codes, long long n,
    long long nnz, int f, int fp, int nedges, hipStream_t stream);
// mleft: nullable uint8 [total_nodes]; given, a NaN value goes left at the
// nodes whose flag is set (the MISS instantiation of the same kernel)
hipError_t skdist_forest_predict(
    const void* X, const void* feat, const void* thr, const void* left,
    const void* right, const void* roots, const void* values,
    const void* mleft, void* out, long long rows, int f, int n_trees,
    int vs, hipStream_t stream);
hipError_t skdist_forest_apply(
    const void* X, const void* feat, const void* thr, const void* left,
    const void* right, const void* roots, const void* mleft,
    void* out_leaf, long long rows, int f, int n_trees,
    hipStream_t stream);
hipError_t skdist_forest_predict_csr(
    const void* indptr, const void* indices, const void* data,
    const void* feat, const void* thr, const void* left, const void* right,
    const void* roots, const void* values, const void* mleft, void* out,
    long long rows, long long nnz, int n_trees, int vs,
    hipStream_t stream);
hipError_t skdist_forest_apply_csr(
    const void* indptr, const void* indices, const void* data,
    const void* feat, const void* thr, const void* left, const void* right,
    const void* roots, const void* mleft, void* out_leaf, long long rows,
    long long nnz, int n_trees, hipStream_t stream);
}  // extern "C"
