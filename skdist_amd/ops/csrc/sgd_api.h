// C launchers of the dense SGD family: included by sgd_kernels.hip and
// auc_kernels.hip, which define them, and by bindings.cpp, which calls
// them, so the compiler checks each signature on both sides.
#pragma once

#include <hip/hip_runtime.h>

// One mini-batch step (K1 + K2 + K3) of the batched dense solver.  Device
// pointers, row-major, K-contiguous; nothing is owned.
struct SgdStep {
    const void* Xs = nullptr;    // [n_pad][fa] bf16, epoch-shuffled, rows
                                 // n..n_pad zero
    const void* XsT = nullptr;   // [fa_store][n_pad] bf16, rows fa.. zero
    void* GT = nullptr;          // [ncols_pad][gt_stride] bf16, K1 -> K2
    void* W = nullptr;           // [fa][ncols_pad] f32
    void* V = nullptr;           // like W: momentum buffer, null without
    void* WbfT = nullptr;        // [ncols_pad][fa] bf16: K1 reads, K3 writes
    void* partial = nullptr;     // [splitk][fa][ncols_pad] f32, K2 -> K3
    const void* y = nullptr;     // [n] f32
    const void* fold = nullptr;  // [n] int32
    const void* col_class = nullptr;   // [ncols_pad] int32, < 0: t = y
    const void* col_fold = nullptr;    // [ncols_pad] int32
    const void* col_class2 = nullptr;  // [ncols_pad] int32, >= 0: one-vs-one
    const void* col_lr = nullptr;      // [ncols_pad] f32
    const void* col_l2 = nullptr;      // [ncols_pad] f32
    const void* fmask = nullptr;  // [fa][ncols_pad] uint8 or null; 0 pins W
    const void* row_w = nullptr;  // [n] f32 sample weights or null
    float inv_m = 0.f;            // 1 / m, or 1 / sum(row_w) of the batch
    long long start = 0, m = 0;   // the batch: rows start .. start + m
    long long n = 0, n_pad = 0, fa_store = 0;
    int fa = 0, ncols_pad = 0, gt_stride = 0, splitk = 0;
    int loss_id = 0;              // LOSS_* of common.h
    float lr_scale = 1.f, momentum = 0.f;
    int intercept_row = 0;        // the row of W that takes no penalty
    // L1 (k_reduce_update_l1 as K3), all three or none: the per-column
    // coefficient and the [fa][ncols_pad] f32 credit tables
    const void* col_l1 = nullptr;
    void* cpos = nullptr;
    void* cneg = nullptr;
    // per-element targets (k_fwd_gt_bits as K1), not with the softmax loss:
    // int32 [n_pad][ncols_pad / 32] bit planes; Mbits null trains every
    // element the fold and row tests let through, and needs Tbits
    const void* Tbits = nullptr;
    const void* Mbits = nullptr;
    // LOSS_SOFTMAX (k_fwd_gt_softmax as K1): columns per group, 2..128;
    // every other loss takes 0
    int group_k = 0;
};

// a combination the comments above rule out returns hipErrorInvalidValue
// before anything is launched
hipError_t skdist_sgd_step(const SgdStep& s, hipStream_t stream);

extern "C" {
// K2 alone; variant: 0 the launcher's rule, 1 / 2 the 128- / 96-row tile,
// 3 the whole-fa kernel
hipError_t skdist_grad_partial(
    const void* XsT, const void* GT, void* partial, long long start,
    long long m, long long n_pad, long long fa_store, int fa, int ncols_pad,
    int gt_stride, int splitk, int variant, hipStream_t stream);
hipError_t skdist_score(
    const void* Xf, const void* WbfT, const void* yf, void* out,
    long long m_pad, int fa, int ncols_pad, int mode, hipStream_t stream);
hipError_t skdist_score_groups(
    const void* Xf, const void* WbfT, const void* yf, void* part,
    long long m_pad, int fa, int ncols_pad, int gk, int mode,
    hipStream_t stream);
// gk: 1 (binary) or 3..128; cnt [2][ncols_pad] int32, zeroed by the caller
hipError_t skdist_score_counts(
    const void* Xf, const void* WbfT, const void* yf, void* cnt,
    long long m_pad, int fa, int ncols_pad, int gk, hipStream_t stream);
// exact ROC AUC counts (auc_kernels.hip).  ZT [nm][M] f32, the n_neg
// negatives of each row first; scratch [nm][n_neg] int32; out [nm] int64
// U2.  ZT is consumed: the sort ping-pongs between scratch and the
// negatives' part of ZT.  0 <= n_neg <= M < 2^31
hipError_t skdist_auc_counts(
    void* ZT, void* scratch, void* out, long long nm, long long M,
    long long n_neg, hipStream_t stream);
// average precision sums (auc_kernels.hip).  ZT as above; scratch [nm][M]
// int32; out [nm] f64 S = sum over positives of TP / (TP + FP), AP = S / P.
// All of ZT is consumed: both halves are sorted, each between its own part
// of ZT and of scratch.  0 <= n_neg <= M < 2^31
hipError_t skdist_ap_sums(
    void* ZT, void* scratch, void* out, long long nm, long long M,
    long long n_neg, hipStream_t stream);
hipError_t skdist_standardize(
    const void* X, const void* mean, const void* inv_std, void* out,
    long long n, int f, int fa, hipStream_t stream);
}
