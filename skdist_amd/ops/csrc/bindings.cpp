// Python bindings for the skdist_amd HIP kernels (built with hipcc against
// the ROCm torch in this image; no CUDA shims, no hipify).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <hip/hip_runtime.h>

#include <optional>

#include "tree_api.h"

extern "C" hipError_t skdist_sgd_step(
    const void* Xs, const void* XsT, const void* WbfT_in,
    void* GT, void* W, void* V, void* WbfT, void* partial,
    const void* y, const void* fold,
    const void* col_class, const void* col_fold, const void* col_class2,
    const void* col_lr, const void* col_l2, const void* fmask,
    const void* row_w, float inv_m,
    long long start, long long m, long long n, long long n_pad,
    long long fa_store, int fa, int ncols_pad,
    int gt_stride, int splitk, int loss_id,
    float lr_scale, float momentum, int intercept_row, int group_k,
    hipStream_t stream);
// same step with the cumulative-penalty L1 update (k_reduce_update_l1)
extern "C" hipError_t skdist_sgd_step_l1(
    const void* Xs, const void* XsT, const void* WbfT_in,
    void* GT, void* W, void* V, void* WbfT, void* partial,
    const void* y, const void* fold,
    const void* col_class, const void* col_fold, const void* col_class2,
    const void* col_lr, const void* col_l2, const void* fmask,
    const void* row_w, float inv_m,
    long long start, long long m, long long n, long long n_pad,
    long long fa_store, int fa, int ncols_pad,
    int gt_stride, int splitk, int loss_id,
    float lr_scale, float momentum, int intercept_row,
    const void* col_l1, void* cpos, void* cneg, int group_k,
    hipStream_t stream);
// same step with per-element targets from bit planes (k_fwd_gt_bits as K1);
// col_l1 null is the L2-only update, Mbits null means every element trains
extern "C" hipError_t skdist_sgd_step_bits(
    const void* Xs, const void* XsT, const void* WbfT_in,
    void* GT, void* W, void* V, void* WbfT, void* partial,
    const void* y, const void* fold,
    const void* col_class, const void* col_fold, const void* col_class2,
    const void* col_lr, const void* col_l2, const void* fmask,
    const void* row_w, float inv_m,
    long long start, long long m, long long n, long long n_pad,
    long long fa_store, int fa, int ncols_pad,
    int gt_stride, int splitk, int loss_id,
    float lr_scale, float momentum, int intercept_row,
    const void* col_l1, void* cpos, void* cneg,
    const void* Tbits, const void* Mbits, hipStream_t stream);
// K2 alone; variant: 0 the launcher's rule, 1 / 2 the 128- / 96-row tile,
// 3 the whole-fa kernel
extern "C" hipError_t skdist_grad_partial(
    const void* XsT, const void* GT, void* partial, long long start,
    long long m, long long n_pad, long long fa_store, int fa, int ncols_pad,
    int gt_stride, int splitk, int variant, hipStream_t stream);

namespace {

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be on the GPU")
#define CHECK_CONT(t) TORCH_CHECK((t).is_contiguous(), #t " not contiguous")

// ---- argument checks of the bindings.  The launchers take void*, so
// every tensor that reaches one is first pinned to the device, layout and
// dtype its kernel reads; a binding launches nothing on empty work.
void check_t(const torch::Tensor& t, torch::ScalarType dt,
             const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
    TORCH_CHECK(t.is_contiguous(), name, " not contiguous");
    TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt);
}

void check_vec(const torch::Tensor& t, torch::ScalarType dt, int64_t len,
               const char* name) {
    check_t(t, dt, name);
    TORCH_CHECK(t.numel() == len, name, " must have ", len, " elements");
}

void check_2d(const torch::Tensor& t, torch::ScalarType dt, int64_t rows,
              int64_t cols, const char* name) {
    check_t(t, dt, name);
    TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols,
                name, " must be [", rows, ", ", cols, "]");
}

struct StepArgs {
    int64_t n_pad, fa, fa_store, ncols_pad, gt_stride, splitk, n;
};

// Every tensor of one dense SGD step (K1+K2+K3), checked against what the
// kernels index: shared by sgd_step and the epoch / solve entries with and
// without L1.  `rows` is the largest row count one step covers (m for
// sgd_step, the batch size otherwise); V, fmask and row_w may be empty.
// loss_id 3 (softmax) trains groups of group_k columns (2..128) with
// k_fwd_gt_softmax; every other loss takes group_k == 0.
StepArgs check_step_tensors(
    const torch::Tensor& Xs, const torch::Tensor& XsT,
    const torch::Tensor& GT, const torch::Tensor& W, const torch::Tensor& V,
    const torch::Tensor& WbfT, const torch::Tensor& partial,
    const torch::Tensor& y, const torch::Tensor& fold,
    const torch::Tensor& col_class, const torch::Tensor& col_fold,
    const torch::Tensor& col_class2, const torch::Tensor& col_lr,
    const torch::Tensor& col_l2, const torch::Tensor& fmask,
    const torch::Tensor& row_w, int64_t rows, double momentum,
    int64_t intercept_row, int64_t loss_id, int64_t group_k) {
    TORCH_CHECK(loss_id >= 0 && loss_id <= 3, "loss_id must be 0..3");
    if (loss_id == 3) {
        TORCH_CHECK(group_k >= 2 && group_k <= 128,
                    "the softmax loss needs group_k in [2, 128], got ",
                    group_k);
    } else {
        TORCH_CHECK(group_k == 0,
                    "group_k is for the softmax loss (loss_id 3) only");
    }
    const auto bf16 = torch::kBFloat16;
    const auto f32 = torch::kFloat32;
    const auto i32 = torch::kInt32;
    check_t(Xs, bf16, "Xs");
    check_t(XsT, bf16, "XsT");
    check_t(GT, bf16, "GT");
    check_t(W, f32, "W");
    check_t(partial, f32, "partial");
    TORCH_CHECK(Xs.dim() == 2 && XsT.dim() == 2 && GT.dim() == 2 &&
                W.dim() == 2, "Xs, XsT, GT and W must be 2-D");
    TORCH_CHECK(partial.dim() == 3, "partial must be [splitk, fa, ncols_pad]");
    StepArgs a;
    a.n_pad = Xs.size(0);
    a.fa = Xs.size(1);
    a.fa_store = XsT.size(0);
    a.ncols_pad = W.size(1);
    a.gt_stride = GT.size(1);
    a.splitk = partial.size(0);
    a.n = y.numel();
    TORCH_CHECK(a.fa >= 32 && a.fa % 32 == 0,
                "fa must be a multiple of 32");
    TORCH_CHECK(a.n_pad >= 128 && a.n_pad % 128 == 0,
                "n_pad must be a multiple of 128");
    TORCH_CHECK(a.fa_store % 128 == 0, "fa_store must be a multiple of 128");
    TORCH_CHECK(a.fa_store >= a.fa, "XsT must have at least fa rows");
    TORCH_CHECK(a.ncols_pad >= 128 && a.ncols_pad % 128 == 0,
                "ncols_pad must be a mult of 128");
    TORCH_CHECK(XsT.size(1) == a.n_pad, "XsT shape mismatch");
    TORCH_CHECK(W.size(0) == a.fa, "W rows != fa");
    TORCH_CHECK(a.splitk >= 1, "splitk must be >= 1");
    TORCH_CHECK(partial.size(1) == a.fa && partial.size(2) == a.ncols_pad,
                "partial must be [splitk, fa, ncols_pad]");
    check_2d(WbfT, bf16, a.ncols_pad, a.fa, "WbfT");
    TORCH_CHECK(rows >= 1, "a step needs at least one row");
    const int64_t rows_pad = (rows + 127) / 128 * 128;
    TORCH_CHECK(GT.size(0) == a.ncols_pad && a.gt_stride >= rows_pad &&
                a.gt_stride % 8 == 0,
                "GT must be [ncols_pad, gt_stride >= ", rows_pad,
                "] with gt_stride a multiple of 8");
    TORCH_CHECK(a.n >= 1 && a.n <= a.n_pad, "y must have 1..n_pad elements");
    check_vec(y, f32, a.n, "y");
    check_vec(fold, i32, a.n, "fold");
    check_vec(col_class, i32, a.ncols_pad, "col_class");
    check_vec(col_fold, i32, a.ncols_pad, "col_fold");
    check_vec(col_class2, i32, a.ncols_pad, "col_class2");
    check_vec(col_lr, f32, a.ncols_pad, "col_lr");
    check_vec(col_l2, f32, a.ncols_pad, "col_l2");
    if (row_w.numel() > 0) check_vec(row_w, f32, a.n, "row_w");
    if (fmask.numel() > 0)
        check_2d(fmask, torch::kUInt8, a.fa, a.ncols_pad, "fmask");
    if (V.numel() > 0) {
        check_t(V, f32, "V");
        TORCH_CHECK(V.sizes() == W.sizes(), "V must be empty or match W");
    } else {
        TORCH_CHECK(!(momentum > 0.0), "momentum > 0 needs V");
    }
    TORCH_CHECK(intercept_row >= 0 && intercept_row < a.fa,
                "intercept_row must be in [0, fa)");
    return a;
}

// the epoch / solve entries walk y in batches of batch_size rows and read
// one 1/m (or 1/sum(w)) per batch from a CPU f32 tensor
void check_batches(const StepArgs& a, int64_t batch_size,
                   const torch::Tensor& inv_m_cpu) {
    TORCH_CHECK(batch_size >= 128 && batch_size % 128 == 0,
                "batch_size must be a mult of 128");
    TORCH_CHECK(!inv_m_cpu.is_cuda(), "inv_m must be a CPU tensor");
    TORCH_CHECK(inv_m_cpu.scalar_type() == torch::kFloat32 &&
                inv_m_cpu.is_contiguous(),
                "inv_m must be a contiguous f32 tensor");
    TORCH_CHECK(inv_m_cpu.numel() >= (a.n + batch_size - 1) / batch_size,
                "inv_m shorter than the batch count");
}

void sgd_step(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
              torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
              torch::Tensor partial, torch::Tensor y, torch::Tensor fold,
              torch::Tensor col_class, torch::Tensor col_fold,
              torch::Tensor col_class2,
              torch::Tensor col_lr, torch::Tensor col_l2,
              torch::Tensor fmask, torch::Tensor row_w,
              int64_t start, int64_t m, int64_t loss_id, double lr_scale,
              double momentum, int64_t intercept_row, double inv_m,
              int64_t group_k) {
    TORCH_CHECK(m >= 1, "m must be >= 1");
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, m, momentum,
                                intercept_row, loss_id, group_k);
    // K2 stages 16 B chunks of XsT from column `start` on
    TORCH_CHECK(start >= 0 && start % 8 == 0,
                "start must be a non-negative multiple of 8");
    TORCH_CHECK(start + (m + 127) / 128 * 128 <= a.n_pad,
                "start + m_pad must be <= n_pad");
    const bool has_V = V.numel() > 0;
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_sgd_step(
        Xs.data_ptr(), XsT.data_ptr(), WbfT.data_ptr(), GT.data_ptr(),
        W.data_ptr(), has_V ? V.data_ptr() : nullptr, WbfT.data_ptr(),
        partial.data_ptr(), y.data_ptr(), fold.data_ptr(),
        col_class.data_ptr(), col_fold.data_ptr(), col_class2.data_ptr(),
        col_lr.data_ptr(), col_l2.data_ptr(),
        fmask.numel() ? fmask.data_ptr() : nullptr,
        row_w.numel() ? row_w.data_ptr() : nullptr, (float)inv_m,
        start, m, a.n, a.n_pad, a.fa_store, (int)a.fa,
        (int)a.ncols_pad, (int)a.gt_stride, (int)a.splitk, (int)loss_id,
        (float)lr_scale, (float)momentum, (int)intercept_row, (int)group_k,
        stream);
    TORCH_CHECK(err == hipSuccess, "skdist_sgd_step: ",
                hipGetErrorString(err));
}

// K2 of one step on its own (tests, timing under a kernel trace): the
// checks sgd_step makes on XsT, GT and partial, then one launch of the
// kernel `variant` names
void grad_partial(torch::Tensor XsT, torch::Tensor GT, torch::Tensor partial,
                  int64_t start, int64_t m, int64_t variant) {
    const auto bf16 = torch::kBFloat16;
    check_t(XsT, bf16, "XsT");
    check_t(GT, bf16, "GT");
    check_t(partial, torch::kFloat32, "partial");
    TORCH_CHECK(XsT.dim() == 2 && GT.dim() == 2, "XsT and GT must be 2-D");
    TORCH_CHECK(partial.dim() == 3, "partial must be [splitk, fa, ncols_pad]");
    const int64_t fa_store = XsT.size(0), n_pad = XsT.size(1);
    const int64_t splitk = partial.size(0), fa = partial.size(1);
    const int64_t ncols_pad = partial.size(2), gt_stride = GT.size(1);
    TORCH_CHECK(fa >= 32 && fa % 32 == 0, "fa must be a multiple of 32");
    TORCH_CHECK(n_pad >= 128 && n_pad % 128 == 0,
                "n_pad must be a multiple of 128");
    TORCH_CHECK(fa_store % 128 == 0, "fa_store must be a multiple of 128");
    TORCH_CHECK(fa_store >= fa, "XsT must have at least fa rows");
    TORCH_CHECK(ncols_pad >= 128 && ncols_pad % 128 == 0,
                "ncols_pad must be a mult of 128");
    TORCH_CHECK(splitk >= 1, "splitk must be >= 1");
    TORCH_CHECK(m >= 1, "m must be >= 1");
    const int64_t m_pad = (m + 127) / 128 * 128;
    TORCH_CHECK(GT.size(0) == ncols_pad && gt_stride >= m_pad &&
                gt_stride % 8 == 0,
                "GT must be [ncols_pad, gt_stride >= ", m_pad,
                "] with gt_stride a multiple of 8");
    TORCH_CHECK(start >= 0 && start % 8 == 0,
                "start must be a non-negative multiple of 8");
    TORCH_CHECK(start + m_pad <= n_pad, "start + m_pad must be <= n_pad");
    TORCH_CHECK(variant >= 0 && variant <= 3, "variant must be 0..3");
    TORCH_CHECK(variant != 3 || fa <= 288,
                "the whole-fa kernel takes fa <= 288");
    TORCH_CHECK(variant != 2 || (fa + 95) / 96 * 96 <= fa_store,
                "96-row tiles would read XsT rows past fa_store");
    hipError_t err = skdist_grad_partial(
        XsT.data_ptr(), GT.data_ptr(), partial.data_ptr(), start, m, n_pad,
        fa_store, (int)fa, (int)ncols_pad, (int)gt_stride, (int)splitk,
        (int)variant, c10::hip::getCurrentHIPStream().stream());
    TORCH_CHECK(err == hipSuccess, "skdist_grad_partial: ",
                hipGetErrorString(err));
}

// Run `body(stream)` for `epochs` epochs with hipGraph capture: epoch 0
// executes eagerly on a dedicated non-blocking stream (the legacy
// default stream cannot capture), one epoch is then recorded into a
// graph and replayed for the rest — one launch per epoch instead of
// hundreds (the per-epoch launch sequence is identical by construction:
// fixed batches, fixed buffers).  Falls back to the eager loop on any
// capture error.
template <typename Body>
static void run_epochs_graphed(int64_t epochs, hipStream_t torch_stream,
                               Body&& body) {
    if (epochs <= 0) return;
    hipStream_t s2 = nullptr;
    if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking)
            != hipSuccess || s2 == nullptr) {
        for (int64_t e = 0; e < epochs; ++e) body(torch_stream);
        return;
    }
    hipEvent_t ev = nullptr;
    hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    hipEventRecord(ev, torch_stream);
    hipStreamWaitEvent(s2, ev, 0);

    body(s2);  // epoch 0 executes (and warms any lazy module state)
    int64_t done = 1;
    if (epochs > 1) {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        bool ok = hipStreamBeginCapture(
                      s2, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            try {
                body(s2);  // recorded, not executed
            } catch (...) {
                // never leave the stream in capture mode
                hipStreamEndCapture(s2, &graph);
                if (graph) hipGraphDestroy(graph);
                hipEventDestroy(ev);
                hipStreamDestroy(s2);
                throw;
            }
            ok = hipStreamEndCapture(s2, &graph) == hipSuccess;
        }
        if (ok)
            ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)
                 == hipSuccess;
        if (ok) {
            for (int64_t e = 1; e < epochs; ++e)
                hipGraphLaunch(exec, s2);
            done = epochs;
        }
        if (exec) hipGraphExecDestroy(exec);
        if (graph) hipGraphDestroy(graph);
    }
    for (int64_t e = done; e < epochs; ++e) body(s2);  // capture fallback

    hipEventRecord(ev, s2);
    hipStreamWaitEvent(torch_stream, ev, 0);
    hipEventDestroy(ev);
    hipStreamDestroy(s2);
}

// L1 state of one dense solve: per-column coefficient plus the two
// per-weight credit tables, all-or-nothing
struct L1Args {
    const void* col_l1 = nullptr;
    void* cpos = nullptr;
    void* cneg = nullptr;
};

L1Args check_l1(torch::Tensor& col_l1, torch::Tensor& cpos,
                torch::Tensor& cneg, torch::Tensor& W, double momentum) {
    for (auto* t : {&col_l1, &cpos, &cneg}) {
        CHECK_DEV(*t);
        CHECK_CONT(*t);
        TORCH_CHECK(t->scalar_type() == torch::kFloat32, "L1 state is f32");
    }
    TORCH_CHECK(col_l1.numel() == W.size(1), "col_l1 must be [ncols_pad]");
    TORCH_CHECK(cpos.sizes() == W.sizes() && cneg.sizes() == W.sizes(),
                "L1 credit tables must match W");
    TORCH_CHECK(momentum >= 0.0 && momentum < 1.0,
                "momentum must be in [0, 1)");
    L1Args l1;
    l1.col_l1 = col_l1.data_ptr();
    l1.cpos = cpos.data_ptr();
    l1.cneg = cneg.data_ptr();
    return l1;
}

// the bit planes of a solve with per-element targets: Tbits and, optionally,
// Mbits, both int32 [n_pad, ncols_pad / 32]; tbits == nullptr is a solve
// with class targets
struct BitArgs {
    const void* tbits = nullptr;
    const void* mbits = nullptr;
};

BitArgs check_bits(const StepArgs& a, const torch::Tensor& tbits,
                   const torch::Tensor& mbits, int64_t loss_id) {
    TORCH_CHECK(loss_id != 3,
                "per-element targets do not go with the softmax loss");
    check_2d(tbits, torch::kInt32, a.n_pad, a.ncols_pad / 32, "tbits");
    BitArgs b;
    b.tbits = tbits.data_ptr();
    if (mbits.numel() > 0) {
        check_2d(mbits, torch::kInt32, a.n_pad, a.ncols_pad / 32, "mbits");
        b.mbits = mbits.data_ptr();
    }
    return b;
}

// the optional L1 tensors of the *_bits entries: all three empty is the
// L2-only update
L1Args check_l1_opt(torch::Tensor& col_l1, torch::Tensor& cpos,
                    torch::Tensor& cneg, torch::Tensor& W, double momentum) {
    if (col_l1.numel() == 0 && cpos.numel() == 0 && cneg.numel() == 0)
        return L1Args{};
    TORCH_CHECK(col_l1.numel() > 0 && cpos.numel() > 0 && cneg.numel() > 0,
                "col_l1, cpos and cneg (the L1 state) go together");
    return check_l1(col_l1, cpos, cneg, W, momentum);
}

// every mini-batch step of one epoch on `st`; `l1.col_l1 == nullptr`
// launches the L2-only step, `bits.tbits != nullptr` the step with
// per-element targets
void enqueue_epoch(const StepArgs& a, torch::Tensor& Xs, torch::Tensor& XsT,
                   torch::Tensor& GT, torch::Tensor& W, torch::Tensor& V,
                   torch::Tensor& WbfT, torch::Tensor& partial,
                   torch::Tensor& y, torch::Tensor& fold,
                   torch::Tensor& col_class, torch::Tensor& col_fold,
                   torch::Tensor& col_class2, torch::Tensor& col_lr,
                   torch::Tensor& col_l2, torch::Tensor& fmask,
                   torch::Tensor& row_w, const float* inv_p,
                   int64_t batch_size, int64_t loss_id, float lr_scale,
                   double momentum, int64_t intercept_row,
                   const L1Args& l1, int64_t group_k, hipStream_t st,
                   const char* who, const BitArgs& bits = BitArgs{}) {
    const bool has_V = V.numel() > 0;
    int64_t bi = 0;
    for (int64_t start = 0; start < a.n; start += batch_size, ++bi) {
        const int64_t m = std::min(batch_size, a.n - start);
        void* Vp = has_V ? V.data_ptr() : nullptr;
        const void* fm = fmask.numel() ? fmask.data_ptr() : nullptr;
        const void* rw = row_w.numel() ? row_w.data_ptr() : nullptr;
        hipError_t err;
        if (bits.tbits != nullptr) {
            err = skdist_sgd_step_bits(
                Xs.data_ptr(), XsT.data_ptr(), WbfT.data_ptr(),
                GT.data_ptr(), W.data_ptr(), Vp, WbfT.data_ptr(),
                partial.data_ptr(), y.data_ptr(), fold.data_ptr(),
                col_class.data_ptr(), col_fold.data_ptr(),
                col_class2.data_ptr(), col_lr.data_ptr(),
                col_l2.data_ptr(), fm, rw, inv_p[bi],
                start, m, a.n, a.n_pad, a.fa_store,
                (int)a.fa, (int)a.ncols_pad, (int)a.gt_stride,
                (int)a.splitk, (int)loss_id, lr_scale, (float)momentum,
                (int)intercept_row, l1.col_l1, l1.cpos, l1.cneg,
                bits.tbits, bits.mbits, st);
        } else if (l1.col_l1 == nullptr) {
            err = skdist_sgd_step(
                Xs.data_ptr(), XsT.data_ptr(), WbfT.data_ptr(),
                GT.data_ptr(), W.data_ptr(), Vp, WbfT.data_ptr(),
                partial.data_ptr(), y.data_ptr(), fold.data_ptr(),
                col_class.data_ptr(), col_fold.data_ptr(),
                col_class2.data_ptr(), col_lr.data_ptr(),
                col_l2.data_ptr(), fm, rw, inv_p[bi],
                start, m, a.n, a.n_pad, a.fa_store,
                (int)a.fa, (int)a.ncols_pad, (int)a.gt_stride,
                (int)a.splitk, (int)loss_id, lr_scale, (float)momentum,
                (int)intercept_row, (int)group_k, st);
        } else {
            err = skdist_sgd_step_l1(
                Xs.data_ptr(), XsT.data_ptr(), WbfT.data_ptr(),
                GT.data_ptr(), W.data_ptr(), Vp, WbfT.data_ptr(),
                partial.data_ptr(), y.data_ptr(), fold.data_ptr(),
                col_class.data_ptr(), col_fold.data_ptr(),
                col_class2.data_ptr(), col_lr.data_ptr(),
                col_l2.data_ptr(), fm, rw, inv_p[bi],
                start, m, a.n, a.n_pad, a.fa_store,
                (int)a.fa, (int)a.ncols_pad, (int)a.gt_stride,
                (int)a.splitk, (int)loss_id, lr_scale, (float)momentum,
                (int)intercept_row, l1.col_l1, l1.cpos, l1.cneg,
                (int)group_k, st);
        }
        TORCH_CHECK(err == hipSuccess, who, ": ", hipGetErrorString(err));
    }
}

// one whole epoch: the minibatch loop runs in C++ so the hot path costs
// one pybind crossing per epoch instead of one per step
void sgd_epoch(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
               torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
               torch::Tensor partial, torch::Tensor y, torch::Tensor fold,
               torch::Tensor col_class, torch::Tensor col_fold,
               torch::Tensor col_class2,
               torch::Tensor col_lr, torch::Tensor col_l2,
               torch::Tensor fmask, torch::Tensor row_w,
               torch::Tensor inv_m_cpu,  // [n_batches] f32 on CPU
               int64_t batch_size, int64_t loss_id, double lr_scale,
               double momentum, int64_t intercept_row, int64_t group_k) {
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, batch_size, momentum,
                                intercept_row, loss_id, group_k);
    check_batches(a, batch_size, inv_m_cpu);
    enqueue_epoch(a, Xs, XsT, GT, W, V, WbfT, partial, y, fold, col_class,
                  col_fold, col_class2, col_lr, col_l2, fmask, row_w,
                  (const float*)inv_m_cpu.data_ptr(), batch_size, loss_id,
                  (float)lr_scale, momentum, intercept_row, L1Args{},
                  group_k, c10::hip::getCurrentHIPStream().stream(),
                  "sgd_epoch");
}

// all epochs in one call; lr_scale is constant (lr_decay=0), so every
// epoch launches the identical sequence -> hipGraph replay
void sgd_solve(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
               torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
               torch::Tensor partial, torch::Tensor y, torch::Tensor fold,
               torch::Tensor col_class, torch::Tensor col_fold,
               torch::Tensor col_class2,
               torch::Tensor col_lr, torch::Tensor col_l2,
               torch::Tensor fmask, torch::Tensor row_w,
               torch::Tensor inv_m_cpu, int64_t batch_size,
               int64_t loss_id, double momentum, int64_t intercept_row,
               int64_t epochs, int64_t group_k) {
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, batch_size, momentum,
                                intercept_row, loss_id, group_k);
    check_batches(a, batch_size, inv_m_cpu);
    const float* inv_p = (const float*)inv_m_cpu.data_ptr();
    auto torch_stream = c10::hip::getCurrentHIPStream().stream();
    auto body = [&](hipStream_t st) {
        enqueue_epoch(a, Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                      col_class, col_fold, col_class2, col_lr, col_l2,
                      fmask, row_w, inv_p, batch_size, loss_id, 1.0f,
                      momentum, intercept_row, L1Args{}, group_k, st,
                      "sgd_solve");
    };
    run_epochs_graphed(epochs, torch_stream, body);
}

// L1 / elastic-net twins of sgd_epoch and sgd_solve: same positional
// arguments, then col_l1 [ncols_pad] and the credit tables cpos / cneg
// [fa][ncols_pad] (zero-initialised by the caller, carried across epochs)
void sgd_epoch_l1(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
                  torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
                  torch::Tensor partial, torch::Tensor y,
                  torch::Tensor fold, torch::Tensor col_class,
                  torch::Tensor col_fold, torch::Tensor col_class2,
                  torch::Tensor col_lr, torch::Tensor col_l2,
                  torch::Tensor fmask, torch::Tensor row_w,
                  torch::Tensor inv_m_cpu, int64_t batch_size,
                  int64_t loss_id, double lr_scale, double momentum,
                  int64_t intercept_row, torch::Tensor col_l1,
                  torch::Tensor cpos, torch::Tensor cneg,
                  int64_t group_k) {
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, batch_size, momentum,
                                intercept_row, loss_id, group_k);
    check_batches(a, batch_size, inv_m_cpu);
    auto l1 = check_l1(col_l1, cpos, cneg, W, momentum);
    enqueue_epoch(a, Xs, XsT, GT, W, V, WbfT, partial, y, fold, col_class,
                  col_fold, col_class2, col_lr, col_l2, fmask, row_w,
                  (const float*)inv_m_cpu.data_ptr(), batch_size, loss_id,
                  (float)lr_scale, momentum, intercept_row, l1, group_k,
                  c10::hip::getCurrentHIPStream().stream(), "sgd_epoch_l1");
}

void sgd_solve_l1(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
                  torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
                  torch::Tensor partial, torch::Tensor y,
                  torch::Tensor fold, torch::Tensor col_class,
                  torch::Tensor col_fold, torch::Tensor col_class2,
                  torch::Tensor col_lr, torch::Tensor col_l2,
                  torch::Tensor fmask, torch::Tensor row_w,
                  torch::Tensor inv_m_cpu, int64_t batch_size,
                  int64_t loss_id, double momentum, int64_t intercept_row,
                  int64_t epochs, torch::Tensor col_l1, torch::Tensor cpos,
                  torch::Tensor cneg, int64_t group_k) {
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, batch_size, momentum,
                                intercept_row, loss_id, group_k);
    check_batches(a, batch_size, inv_m_cpu);
    auto l1 = check_l1(col_l1, cpos, cneg, W, momentum);
    const float* inv_p = (const float*)inv_m_cpu.data_ptr();
    auto torch_stream = c10::hip::getCurrentHIPStream().stream();
    auto body = [&](hipStream_t st) {
        enqueue_epoch(a, Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                      col_class, col_fold, col_class2, col_lr, col_l2,
                      fmask, row_w, inv_p, batch_size, loss_id, 1.0f,
                      momentum, intercept_row, l1, group_k, st,
                      "sgd_solve_l1");
    };
    run_epochs_graphed(epochs, torch_stream, body);
}

// ---- per-element targets (k_fwd_gt_bits as K1): the argument lists of
// sgd_step / sgd_epoch / sgd_solve, then tbits and mbits (int32
// [n_pad, ncols_pad / 32]; an empty mbits means no mask), then the optional
// L1 tensors col_l1, cpos, cneg (all empty: the L2-only update)
void sgd_step_bits(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
                   torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
                   torch::Tensor partial, torch::Tensor y,
                   torch::Tensor fold, torch::Tensor col_class,
                   torch::Tensor col_fold, torch::Tensor col_class2,
                   torch::Tensor col_lr, torch::Tensor col_l2,
                   torch::Tensor fmask, torch::Tensor row_w,
                   int64_t start, int64_t m, int64_t loss_id,
                   double lr_scale, double momentum, int64_t intercept_row,
                   double inv_m, torch::Tensor tbits, torch::Tensor mbits,
                   torch::Tensor col_l1, torch::Tensor cpos,
                   torch::Tensor cneg) {
    TORCH_CHECK(m >= 1, "m must be >= 1");
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, m, momentum,
                                intercept_row, loss_id, 0);
    TORCH_CHECK(start >= 0 && start % 8 == 0,
                "start must be a non-negative multiple of 8");
    TORCH_CHECK(start + (m + 127) / 128 * 128 <= a.n_pad,
                "start + m_pad must be <= n_pad");
    auto bits = check_bits(a, tbits, mbits, loss_id);
    auto l1 = check_l1_opt(col_l1, cpos, cneg, W, momentum);
    const bool has_V = V.numel() > 0;
    hipError_t err = skdist_sgd_step_bits(
        Xs.data_ptr(), XsT.data_ptr(), WbfT.data_ptr(), GT.data_ptr(),
        W.data_ptr(), has_V ? V.data_ptr() : nullptr, WbfT.data_ptr(),
        partial.data_ptr(), y.data_ptr(), fold.data_ptr(),
        col_class.data_ptr(), col_fold.data_ptr(), col_class2.data_ptr(),
        col_lr.data_ptr(), col_l2.data_ptr(),
        fmask.numel() ? fmask.data_ptr() : nullptr,
        row_w.numel() ? row_w.data_ptr() : nullptr, (float)inv_m,
        start, m, a.n, a.n_pad, a.fa_store, (int)a.fa,
        (int)a.ncols_pad, (int)a.gt_stride, (int)a.splitk, (int)loss_id,
        (float)lr_scale, (float)momentum, (int)intercept_row,
        l1.col_l1, l1.cpos, l1.cneg, bits.tbits, bits.mbits,
        c10::hip::getCurrentHIPStream().stream());
    TORCH_CHECK(err == hipSuccess, "skdist_sgd_step_bits: ",
                hipGetErrorString(err));
}

void sgd_epoch_bits(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
                    torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
                    torch::Tensor partial, torch::Tensor y,
                    torch::Tensor fold, torch::Tensor col_class,
                    torch::Tensor col_fold, torch::Tensor col_class2,
                    torch::Tensor col_lr, torch::Tensor col_l2,
                    torch::Tensor fmask, torch::Tensor row_w,
                    torch::Tensor inv_m_cpu, int64_t batch_size,
                    int64_t loss_id, double lr_scale, double momentum,
                    int64_t intercept_row, torch::Tensor tbits,
                    torch::Tensor mbits, torch::Tensor col_l1,
                    torch::Tensor cpos, torch::Tensor cneg) {
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, batch_size, momentum,
                                intercept_row, loss_id, 0);
    check_batches(a, batch_size, inv_m_cpu);
    auto bits = check_bits(a, tbits, mbits, loss_id);
    auto l1 = check_l1_opt(col_l1, cpos, cneg, W, momentum);
    enqueue_epoch(a, Xs, XsT, GT, W, V, WbfT, partial, y, fold, col_class,
                  col_fold, col_class2, col_lr, col_l2, fmask, row_w,
                  (const float*)inv_m_cpu.data_ptr(), batch_size, loss_id,
                  (float)lr_scale, momentum, intercept_row, l1, 0,
                  c10::hip::getCurrentHIPStream().stream(),
                  "sgd_epoch_bits", bits);
}

void sgd_solve_bits(torch::Tensor Xs, torch::Tensor XsT, torch::Tensor GT,
                    torch::Tensor W, torch::Tensor V, torch::Tensor WbfT,
                    torch::Tensor partial, torch::Tensor y,
                    torch::Tensor fold, torch::Tensor col_class,
                    torch::Tensor col_fold, torch::Tensor col_class2,
                    torch::Tensor col_lr, torch::Tensor col_l2,
                    torch::Tensor fmask, torch::Tensor row_w,
                    torch::Tensor inv_m_cpu, int64_t batch_size,
                    int64_t loss_id, double momentum, int64_t intercept_row,
                    int64_t epochs, torch::Tensor tbits,
                    torch::Tensor mbits, torch::Tensor col_l1,
                    torch::Tensor cpos, torch::Tensor cneg) {
    auto a = check_step_tensors(Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                                col_class, col_fold, col_class2, col_lr,
                                col_l2, fmask, row_w, batch_size, momentum,
                                intercept_row, loss_id, 0);
    check_batches(a, batch_size, inv_m_cpu);
    auto bits = check_bits(a, tbits, mbits, loss_id);
    auto l1 = check_l1_opt(col_l1, cpos, cneg, W, momentum);
    const float* inv_p = (const float*)inv_m_cpu.data_ptr();
    auto torch_stream = c10::hip::getCurrentHIPStream().stream();
    auto body = [&](hipStream_t st) {
        enqueue_epoch(a, Xs, XsT, GT, W, V, WbfT, partial, y, fold,
                      col_class, col_fold, col_class2, col_lr, col_l2,
                      fmask, row_w, inv_p, batch_size, loss_id, 1.0f,
                      momentum, intercept_row, l1, 0, st,
                      "sgd_solve_bits", bits);
    };
    run_epochs_graphed(epochs, torch_stream, body);
}

}  // namespace

// ------------------------------------------------------------------ //
// sparse text-scale solver (sparse_sgd_kernels.hip)
// ------------------------------------------------------------------ //

extern "C" hipError_t skdist_sp_sgd_step(
    const void* crow, const void* cidx, const void* cval,
    void* W, void* Wb, void* s, void* h, void* hb, void* G, void* part,
    const void* y, const void* fold, const void* row_w,
    const void* col_class, const void* col_fold, const void* col_class2,
    const void* col_lr, const void* col_l2,
    const void* ufeat, const void* cptr, const void* ridx,
    const void* bval, long long uf,
    long long start, long long m, int cp, int loss_id,
    float inv_m, float lr_scale, hipStream_t stream);
extern "C" hipError_t skdist_sp_sgd_step_l1(
    const void* crow, const void* cidx, const void* cval,
    void* W, void* Wb, void* s, void* h, void* hb, void* G, void* part,
    const void* y, const void* fold, const void* row_w,
    const void* col_class, const void* col_fold, const void* col_class2,
    const void* col_lr, const void* col_l2,
    const void* ufeat, const void* cptr, const void* ridx,
    const void* bval, long long uf,
    long long start, long long m, int cp, int loss_id,
    float inv_m, float lr_scale,
    const void* col_l1, void* U, void* q, void* uw, void* ul,
    hipStream_t stream);
extern "C" hipError_t skdist_sp_l1_flush(
    void* W, const void* h, const void* U, void* q, void* uw, void* ul,
    long long f, int cp, hipStream_t stream);
extern "C" hipError_t skdist_sp_renorm_l1(
    void* W, const void* s, void* q, void* uw, void* ul, long long f,
    int cp, hipStream_t stream);
extern "C" hipError_t skdist_sp_forward(
    const void* crow, const void* cidx, const void* cval,
    const void* W, const void* Wb, const void* s, const void* rows,
    void* Z, long long m, int cp, hipStream_t stream);
extern "C" hipError_t skdist_sp_renorm(
    void* W, const void* s, long long f, int cp, hipStream_t stream);

namespace {

static void check_cp(int64_t cp) {
    TORCH_CHECK(cp % 64 == 0, "cp must be a multiple of 64");
}

// one epoch of the sparse solver: the per-batch loop runs in C++.
// CSC arrays are the concatenation over batches; ub_ptr (CPU int64,
// [n_batches+1]) slices ufeat/cptr per batch, cptr values are GLOBAL
// offsets into ridx/bval.
void sp_sgd_epoch(torch::Tensor crow, torch::Tensor cidx,
                  torch::Tensor cval, torch::Tensor W, torch::Tensor Wb,
                  torch::Tensor s, torch::Tensor h, torch::Tensor hb,
                  torch::Tensor G, torch::Tensor part,
                  torch::Tensor y, torch::Tensor fold, torch::Tensor row_w,
                  torch::Tensor col_class, torch::Tensor col_fold,
                  torch::Tensor col_class2, torch::Tensor col_lr,
                  torch::Tensor col_l2, torch::Tensor ufeat,
                  torch::Tensor cptr, torch::Tensor ridx,
                  torch::Tensor bval, torch::Tensor ub_ptr_cpu,
                  torch::Tensor inv_m_cpu, int64_t batch_size,
                  int64_t loss_id, double lr_scale) {
    for (auto* t : {&crow, &cidx, &cval, &W, &Wb, &s, &G, &part, &y,
                    &fold, &col_class, &col_fold, &col_class2, &col_lr,
                    &col_l2, &ufeat, &cptr, &ridx, &bval}) {
        CHECK_DEV(*t);
        CHECK_CONT(*t);
    }
    TORCH_CHECK(!ub_ptr_cpu.is_cuda() && !inv_m_cpu.is_cuda(),
                "ub_ptr/inv_m must be CPU tensors");
    TORCH_CHECK(crow.scalar_type() == torch::kInt64, "crow must be i64");
    TORCH_CHECK(cidx.scalar_type() == torch::kInt32, "cidx must be i32");
    TORCH_CHECK(G.scalar_type() == torch::kBFloat16, "G must be bf16");
    const int64_t cp = W.size(1);
    check_cp(cp);
    const int64_t n = crow.size(0) - 1;
    TORCH_CHECK(G.size(0) >= std::min<int64_t>(batch_size, n) &&
                G.size(1) == cp, "G buffer too small");
    const int64_t* ub = (const int64_t*)ub_ptr_cpu.data_ptr();
    const float* inv_p = (const float*)inv_m_cpu.data_ptr();
    auto stream = c10::hip::getCurrentHIPStream().stream();
    int64_t bi = 0;
    for (int64_t start = 0; start < n; start += batch_size, ++bi) {
        const int64_t m = std::min(batch_size, n - start);
        const int64_t ub0 = ub[bi], uf = ub[bi + 1] - ub[bi];
        hipError_t err = skdist_sp_sgd_step(
            crow.data_ptr(), cidx.data_ptr(), cval.data_ptr(),
            W.data_ptr(), Wb.data_ptr(), s.data_ptr(),
            h.numel() ? h.data_ptr() : nullptr,
            hb.numel() ? hb.data_ptr() : nullptr, G.data_ptr(),
            part.data_ptr(), y.data_ptr(), fold.data_ptr(),
            row_w.numel() ? row_w.data_ptr() : nullptr,
            col_class.data_ptr(), col_fold.data_ptr(),
            col_class2.data_ptr(), col_lr.data_ptr(), col_l2.data_ptr(),
            (const int*)ufeat.data_ptr() + ub0,
            (const long long*)cptr.data_ptr() + ub0,
            ridx.data_ptr(), bval.data_ptr(), uf,
            start, m, (int)cp, (int)loss_id, inv_p[bi],
            (float)lr_scale, stream);
        TORCH_CHECK(err == hipSuccess, "sp_sgd_epoch: ",
                    hipGetErrorString(err));
    }
}

// all epochs of the sparse solver in one call (constant lr_scale);
// identical per-epoch launch sequence -> hipGraph replay
void sp_sgd_solve(torch::Tensor crow, torch::Tensor cidx,
                  torch::Tensor cval, torch::Tensor W, torch::Tensor Wb,
                  torch::Tensor s, torch::Tensor h, torch::Tensor hb,
                  torch::Tensor G, torch::Tensor part,
                  torch::Tensor y, torch::Tensor fold, torch::Tensor row_w,
                  torch::Tensor col_class, torch::Tensor col_fold,
                  torch::Tensor col_class2, torch::Tensor col_lr,
                  torch::Tensor col_l2, torch::Tensor ufeat,
                  torch::Tensor cptr, torch::Tensor ridx,
                  torch::Tensor bval, torch::Tensor ub_ptr_cpu,
                  torch::Tensor inv_m_cpu, int64_t batch_size,
                  int64_t loss_id, int64_t epochs) {
    const int64_t cp = W.size(1);
    check_cp(cp);
    const int64_t n = crow.size(0) - 1;
    const int64_t* ub = (const int64_t*)ub_ptr_cpu.data_ptr();
    const float* inv_p = (const float*)inv_m_cpu.data_ptr();
    auto torch_stream = c10::hip::getCurrentHIPStream().stream();
    auto body = [&](hipStream_t st) {
        int64_t bi = 0;
        for (int64_t start = 0; start < n; start += batch_size, ++bi) {
            const int64_t m = std::min(batch_size, n - start);
            const int64_t ub0 = ub[bi], uf = ub[bi + 1] - ub[bi];
            hipError_t err = skdist_sp_sgd_step(
                crow.data_ptr(), cidx.data_ptr(), cval.data_ptr(),
                W.data_ptr(), Wb.data_ptr(), s.data_ptr(),
                h.numel() ? h.data_ptr() : nullptr,
                hb.numel() ? hb.data_ptr() : nullptr, G.data_ptr(),
                part.data_ptr(), y.data_ptr(), fold.data_ptr(),
                row_w.numel() ? row_w.data_ptr() : nullptr,
                col_class.data_ptr(), col_fold.data_ptr(),
                col_class2.data_ptr(), col_lr.data_ptr(),
                col_l2.data_ptr(),
                (const int*)ufeat.data_ptr() + ub0,
                (const long long*)cptr.data_ptr() + ub0,
                ridx.data_ptr(), bval.data_ptr(), uf,
                start, m, (int)cp, (int)loss_id, inv_p[bi], 1.0f, st);
            TORCH_CHECK(err == hipSuccess, "sp_sgd_solve: ",
                        hipGetErrorString(err));
        }
    };
    run_epochs_graphed(epochs, torch_stream, body);
}

// L1 state of one sparse solve: col_l1 / U [CP], q [f][CP], and with
// the Adagrad accumulator h also uw / ul [f][CP]
struct SpL1Args {
    void* U; void* q; void* uw; void* ul;
};

// `vec` is the per-column f32 vector that goes with the tables (U, or
// the scale s in the renorm); uw / ul are present exactly when `adaptive`
SpL1Args check_sp_l1(torch::Tensor& W, bool adaptive, torch::Tensor& vec,
                     torch::Tensor& q, torch::Tensor& uw,
                     torch::Tensor& ul) {
    for (auto* t : {&W, &vec, &q, &uw, &ul}) {
        if (t->numel() == 0) continue;
        CHECK_DEV(*t);
        CHECK_CONT(*t);
        TORCH_CHECK(t->scalar_type() == torch::kFloat32,
                    "W and the L1 state are f32");
    }
    TORCH_CHECK(W.dim() == 2 && vec.numel() == W.size(1),
                "per-column vector must be [cp]");
    TORCH_CHECK(q.sizes() == W.sizes(), "q must match W");
    if (adaptive) {
        TORCH_CHECK(uw.sizes() == W.sizes() && ul.sizes() == W.sizes(),
                    "adaptive L1 tables must match W");
    } else {
        TORCH_CHECK(uw.numel() == 0 && ul.numel() == 0,
                    "adaptive L1 tables need the Adagrad accumulator");
    }
    return {vec.data_ptr(), q.data_ptr(),
            adaptive ? uw.data_ptr() : nullptr,
            adaptive ? ul.data_ptr() : nullptr};
}

// the Adagrad accumulator decides the mode: empty, or f32 shaped like W
bool check_adagrad(torch::Tensor& W, torch::Tensor& h) {
    if (h.numel() == 0) return false;
    CHECK_DEV(h);
    CHECK_CONT(h);
    TORCH_CHECK(h.scalar_type() == torch::kFloat32 &&
                h.sizes() == W.sizes(), "h must be f32 and match W");
    return true;
}

// L1 / elastic-net twin of sp_sgd_epoch: same positional arguments, then
// col_l1 [CP] and the L1 state (zero-initialised by the caller, carried
// across epochs).  One call per epoch, no graph capture.
void sp_sgd_epoch_l1(torch::Tensor crow, torch::Tensor cidx,
                     torch::Tensor cval, torch::Tensor W, torch::Tensor Wb,
                     torch::Tensor s, torch::Tensor h, torch::Tensor hb,
                     torch::Tensor G, torch::Tensor part,
                     torch::Tensor y, torch::Tensor fold,
                     torch::Tensor row_w,
                     torch::Tensor col_class, torch::Tensor col_fold,
                     torch::Tensor col_class2, torch::Tensor col_lr,
                     torch::Tensor col_l2, torch::Tensor ufeat,
                     torch::Tensor cptr, torch::Tensor ridx,
                     torch::Tensor bval, torch::Tensor ub_ptr_cpu,
                     torch::Tensor inv_m_cpu, int64_t batch_size,
                     int64_t loss_id, double lr_scale,
                     torch::Tensor col_l1, torch::Tensor U,
                     torch::Tensor q, torch::Tensor uw, torch::Tensor ul) {
    for (auto* t : {&crow, &cidx, &cval, &W, &Wb, &s, &G, &part, &y,
                    &fold, &col_class, &col_fold, &col_class2, &col_lr,
                    &col_l2, &ufeat, &cptr, &ridx, &bval, &col_l1}) {
        CHECK_DEV(*t);
        CHECK_CONT(*t);
    }
    TORCH_CHECK(!ub_ptr_cpu.is_cuda() && !inv_m_cpu.is_cuda(),
                "ub_ptr/inv_m must be CPU tensors");
    TORCH_CHECK(crow.scalar_type() == torch::kInt64, "crow must be i64");
    TORCH_CHECK(cidx.scalar_type() == torch::kInt32, "cidx must be i32");
    TORCH_CHECK(G.scalar_type() == torch::kBFloat16, "G must be bf16");
    const int64_t cp = W.size(1);
    check_cp(cp);
    TORCH_CHECK(col_l1.numel() == cp &&
                col_l1.scalar_type() == torch::kFloat32,
                "col_l1 must be f32 [cp]");
    auto l1 = check_sp_l1(W, check_adagrad(W, h), U, q, uw, ul);
    const int64_t n = crow.size(0) - 1;
    TORCH_CHECK(G.size(0) >= std::min<int64_t>(batch_size, n) &&
                G.size(1) == cp, "G buffer too small");
    const int64_t nb = (n + batch_size - 1) / batch_size;
    TORCH_CHECK(ub_ptr_cpu.numel() >= nb + 1 && inv_m_cpu.numel() >= nb,
                "ub_ptr/inv_m shorter than the batch count");
    const int64_t* ub = (const int64_t*)ub_ptr_cpu.data_ptr();
    TORCH_CHECK(ub[nb] <= ufeat.numel() && ub[nb] + 1 <= cptr.numel(),
                "ub_ptr runs past ufeat/cptr");
    const float* inv_p = (const float*)inv_m_cpu.data_ptr();
    auto stream = c10::hip::getCurrentHIPStream().stream();
    int64_t bi = 0;
    for (int64_t start = 0; start < n; start += batch_size, ++bi) {
        const int64_t m = std::min(batch_size, n - start);
        const int64_t ub0 = ub[bi], uf = ub[bi + 1] - ub[bi];
        hipError_t err = skdist_sp_sgd_step_l1(
            crow.data_ptr(), cidx.data_ptr(), cval.data_ptr(),
            W.data_ptr(), Wb.data_ptr(), s.data_ptr(),
            h.numel() ? h.data_ptr() : nullptr,
            hb.numel() ? hb.data_ptr() : nullptr, G.data_ptr(),
            part.data_ptr(), y.data_ptr(), fold.data_ptr(),
            row_w.numel() ? row_w.data_ptr() : nullptr,
            col_class.data_ptr(), col_fold.data_ptr(),
            col_class2.data_ptr(), col_lr.data_ptr(), col_l2.data_ptr(),
            (const int*)ufeat.data_ptr() + ub0,
            (const long long*)cptr.data_ptr() + ub0,
            ridx.data_ptr(), bval.data_ptr(), uf,
            start, m, (int)cp, (int)loss_id, inv_p[bi],
            (float)lr_scale, col_l1.data_ptr(), l1.U, l1.q, l1.uw, l1.ul,
            stream);
        TORCH_CHECK(err == hipSuccess, "sp_sgd_epoch_l1: ",
                    hipGetErrorString(err));
    }
}

// end-of-fit L1 flush over all (feature, column)
void sp_l1_flush(torch::Tensor W, torch::Tensor h, torch::Tensor U,
                 torch::Tensor q, torch::Tensor uw, torch::Tensor ul) {
    auto l1 = check_sp_l1(W, check_adagrad(W, h), U, q, uw, ul);
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_sp_l1_flush(
        W.data_ptr(), h.numel() ? h.data_ptr() : nullptr, l1.U, l1.q,
        l1.uw, l1.ul, W.size(0), (int)W.size(1), stream);
    TORCH_CHECK(err == hipSuccess, "sp_l1_flush: ", hipGetErrorString(err));
}

// L1-mode renorm: W and the per-weight L1 tables change units together
// (the caller scales the per-column U and resets s)
void sp_renorm_l1(torch::Tensor W, torch::Tensor s, torch::Tensor q,
                  torch::Tensor uw, torch::Tensor ul) {
    auto l1 = check_sp_l1(W, uw.numel() > 0, s, q, uw, ul);
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_sp_renorm_l1(
        W.data_ptr(), l1.U, l1.q, l1.uw, l1.ul, W.size(0), (int)W.size(1),
        stream);
    TORCH_CHECK(err == hipSuccess, "sp_renorm_l1: ",
                hipGetErrorString(err));
}

void sp_forward(torch::Tensor crow, torch::Tensor cidx,
                torch::Tensor cval, torch::Tensor W, torch::Tensor Wb,
                torch::Tensor s, torch::Tensor rows, torch::Tensor Z) {
    for (auto* t : {&crow, &cidx, &cval, &W, &Wb, &s, &rows, &Z}) {
        CHECK_DEV(*t);
        CHECK_CONT(*t);
    }
    TORCH_CHECK(rows.scalar_type() == torch::kInt64, "rows must be i64");
    const int64_t cp = W.size(1);
    check_cp(cp);
    TORCH_CHECK(Z.size(0) == rows.size(0) && Z.size(1) == cp,
                "Z shape mismatch");
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_sp_forward(
        crow.data_ptr(), cidx.data_ptr(), cval.data_ptr(), W.data_ptr(),
        Wb.data_ptr(), s.data_ptr(), rows.data_ptr(), Z.data_ptr(),
        rows.size(0), (int)cp, stream);
    TORCH_CHECK(err == hipSuccess, "sp_forward: ", hipGetErrorString(err));
}

void sp_renorm(torch::Tensor W, torch::Tensor s) {
    CHECK_DEV(W);
    CHECK_CONT(W);
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_sp_renorm(W.data_ptr(), s.data_ptr(),
                                      W.size(0), (int)W.size(1), stream);
    TORCH_CHECK(err == hipSuccess, "sp_renorm: ", hipGetErrorString(err));
}

}  // namespace

// ------------------------------------------------------------------ //
// tree family (tree_kernels.hip, predict_kernels.hip: launchers declared
// in tree_api.h), scoring, standardize and hashing
// ------------------------------------------------------------------ //

extern "C" hipError_t skdist_score(
    const void* Xf, const void* WbfT, const void* yf, void* out,
    long long m_pad, int fa, int ncols_pad, int mode,
    hipStream_t stream);
extern "C" hipError_t skdist_standardize(
    const void* X, const void* mean, const void* inv_std, void* out,
    long long n, int f, int fa, hipStream_t stream);
extern "C" hipError_t skdist_hash_vectorize(
    const void* bytes, const void* doc_off, long long n_docs, int mode,
    int min_n, int max_n, int n_features, int alt_sign, void* out_keys,
    void* out_vals, void* ctr, long long cap, hipStream_t stream);
extern "C" hipError_t skdist_hash_vectorize_utf8(
    const void* bytes, const void* doc_off, long long n_docs, int mode,
    int min_n, int max_n, int n_features, int alt_sign,
    const void* word_tbl, const void* ws_list, int n_ws, void* out_keys,
    void* out_vals, void* ctr, long long cap, hipStream_t stream);

namespace {

// codes [n, fp] u8 with fp a multiple of 4 (uchar4 loads); returns fp
int64_t check_codes(const torch::Tensor& codes, int64_t n) {
    check_t(codes, torch::kUInt8, "codes");
    TORCH_CHECK(codes.dim() == 2 && codes.size(0) == n &&
                    codes.size(1) % 4 == 0 && codes.size(1) < (1LL << 31),
                "codes must be [n, fp] with fp % 4 == 0");
    return codes.size(1);
}

// chunk table [n_chunks, 4] i32; returns n_chunks
int64_t check_chunks(const torch::Tensor& chunks) {
    check_t(chunks, torch::kInt32, "chunks");
    TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 4 &&
                    chunks.size(0) < (1LL << 31),
                "chunks must be [n_chunks, 4]");
    return chunks.size(0);
}

// per-tree row plane [TB, n]; returns TB
int64_t check_plane(const torch::Tensor& t, torch::ScalarType dt, int64_t n,
                    const char* name) {
    check_t(t, dt, name);
    TORCH_CHECK(t.dim() == 2 && t.size(1) == n, name, " must be [TB, n]");
    return t.size(0);
}

// CSR inputs shared by the sparse tree kernels: indptr int64 [rows+1],
// indices int32 [nnz], data f32 [nnz], all contiguous on the GPU
void check_csr(const torch::Tensor& indptr, const torch::Tensor& indices,
               const torch::Tensor& data, int64_t rows) {
    TORCH_CHECK(rows >= 0, "output must be 2-D");
    check_vec(indptr, torch::kInt64, rows + 1, "indptr");
    check_vec(indices, torch::kInt32, data.numel(), "indices");
    check_t(data, torch::kFloat32, "data");
    for (auto* t : {&indptr, &indices, &data})
        TORCH_CHECK(t->dim() == 1, "CSR arrays must be 1-D");
}

// node arrays of a flattened forest: int32 / f32, equal lengths
void check_nodes(const torch::Tensor& feat, const torch::Tensor& thr,
                 const torch::Tensor& left, const torch::Tensor& right,
                 const torch::Tensor& roots) {
    const int64_t nodes = feat.numel();
    check_t(feat, torch::kInt32, "feat");
    check_vec(thr, torch::kFloat32, nodes, "thr");
    check_vec(left, torch::kInt32, nodes, "left");
    check_vec(right, torch::kInt32, nodes, "right");
    check_t(roots, torch::kInt32, "roots");
    TORCH_CHECK(roots.numel() >= 1 && nodes >= 1, "empty forest");
    TORCH_CHECK(roots.numel() < (1LL << 31), "too many trees");
}

// leaf payloads values [n_values, vs] and out [rows, vs]; returns vs
int64_t check_payload(const torch::Tensor& values, const torch::Tensor& out,
                      int64_t rows) {
    check_t(values, torch::kFloat32, "values");
    TORCH_CHECK(values.dim() == 2 && values.size(1) >= 1 &&
                    values.size(1) <= 256,
                "values must be [n_values, vs] with vs <= 256 (MAXVS_WIDE)");
    check_2d(out, torch::kFloat32, rows, values.size(1), "out");
    return values.size(1);
}

int64_t rows_of(const torch::Tensor& out) {
    return out.dim() == 2 ? out.size(0) : -1;
}

// an optional trailing tensor: None and an empty tensor both mean "not
// given" (the convention tree_hist uses for its absent tensors)
using OptTensor = std::optional<torch::Tensor>;
bool given(const OptTensor& t) { return t.has_value() && t->numel() > 0; }

// per-node missing-direction flags of a flattened forest, uint8
// [total_nodes]; returns the pointer a launcher takes (null = not given)
const void* check_mleft(const OptTensor& mleft, const torch::Tensor& feat) {
    if (!given(mleft)) return nullptr;
    check_vec(*mleft, torch::kUInt8, feat.numel(), "mleft");
    return mleft->data_ptr();
}

// the current stream, and a launcher's verdict as an exception
hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }
void launched(hipError_t err, const char* what) {
    TORCH_CHECK(err == hipSuccess, what, ": ", hipGetErrorString(err));
}

// absent tensors (y_int / y_f / row_w) are passed empty
void tree_hist(torch::Tensor codes, torch::Tensor y_int, torch::Tensor y_f,
               torch::Tensor row_w, torch::Tensor weights,
               torch::Tensor sample_idx, torch::Tensor chunks,
               torch::Tensor hist, int64_t n, int64_t f, int64_t nbins,
               int64_t fg, int64_t cg) {
    const int64_t fp = check_codes(codes, n);
    const int64_t n_chunks = check_chunks(chunks);
    const int64_t TB = check_plane(weights, torch::kUInt8, n, "weights");
    TORCH_CHECK(check_plane(sample_idx, torch::kInt32, n, "sample_idx") ==
                    TB, "weights and sample_idx differ in TB");
    check_t(hist, torch::kFloat32, "hist");
    TORCH_CHECK(f >= 1 && f <= fp, "f must be in [1, fp]");
    TORCH_CHECK(nbins >= 1 && nbins <= 256, "nbins must be in [1, 256]");
    TORCH_CHECK(hist.dim() == 4 && hist.size(1) == f &&
                    hist.size(2) == nbins && hist.size(3) >= 1,
                "hist must be [NF, f, nbins, S]");
    const int64_t S = hist.size(3);
    const bool cls = y_int.numel() > 0, has_w = row_w.numel() > 0;
    TORCH_CHECK(cls != (y_f.numel() > 0),
                "exactly one of y_int / y_f must be given");
    if (cls) {
        check_vec(y_int, torch::kInt32, n, "y_int");
        TORCH_CHECK(!has_w, "row_w rides the regression stats (y_f) only");
    } else {
        check_vec(y_f, torch::kFloat32, n, "y_f");
        if (has_w) check_vec(row_w, torch::kFloat32, n, "row_w");
        TORCH_CHECK(S == (has_w ? 4 : 3),
                    "hist must be [NF, f, nbins, 4] with row_w and "
                    "[NF, f, nbins, 3] without");
    }
    // cg = -1 (the default): not grouped; else the class-group width
    const bool grouped = cg != -1;
    if (grouped) {
        TORCH_CHECK(cg > 0, "cg must be > 0 (leave it out for one tile "
                            "over all S stats)");
        TORCH_CHECK(cls && !has_w,
                    "class groups (cg) split class counts only: y_int and "
                    "no row_w");
    }
    const int64_t tile_s = grouped && cg < S ? cg : S;
    TORCH_CHECK(fg >= 1 && fg <= fp && fg * nbins * tile_s * 4 <= 64 * 1024,
                grouped ? "fg * nbins * min(cg, S) * 4 bytes must fit 64 "
                          "KiB of LDS"
                        : "fg * nbins * S * 4 bytes must fit 64 KiB of LDS");
    TORCH_CHECK(!grouped || (S + cg - 1) / cg <= 65535,
                "too many class groups");
    if (n_chunks == 0) return;
    launched(skdist_tree_hist(
        codes.data_ptr(), cls ? y_int.data_ptr() : nullptr,
        cls ? nullptr : y_f.data_ptr(),
        has_w ? row_w.data_ptr() : nullptr, weights.data_ptr(),
        sample_idx.data_ptr(), chunks.data_ptr(), hist.data_ptr(), n,
        (int)f, (int)fp, (int)nbins, (int)S, (int)fg,
        grouped ? (int)std::min<int64_t>(cg, S) : 0, (int)n_chunks,
        cur_stream()), "tree_hist");
}

// cnt_stat = -1: min-leaf on the weight sums; else on that (count) stat.
// missing != 0: bin nbins-1 is the missing bin; out_mleft int32 [NF] gets
// the learned direction (1 = missing rows go left)
void tree_split(torch::Tensor hist, torch::Tensor node_seed, int64_t f,
                int64_t nbins, int64_t S, int64_t is_cls, int64_t crit,
                int64_t m_features, int64_t extra_mode, double min_leaf,
                torch::Tensor out_feat, torch::Tensor out_bin,
                torch::Tensor out_wl, torch::Tensor out_gain,
                torch::Tensor out_imp, torch::Tensor out_stats,
                torch::Tensor out_lstats, int64_t cnt_stat, int64_t missing,
                OptTensor out_mleft) {
    const int64_t NF = node_seed.numel();
    check_t(hist, torch::kFloat32, "hist");
    check_t(node_seed, torch::kInt32, "node_seed");
    check_vec(out_feat, torch::kInt32, NF, "out_feat");
    check_vec(out_bin, torch::kInt32, NF, "out_bin");
    check_vec(out_wl, torch::kFloat32, NF, "out_wl");
    check_vec(out_gain, torch::kFloat32, NF, "out_gain");
    check_vec(out_imp, torch::kFloat32, NF, "out_imp");
    check_vec(out_stats, torch::kFloat32, NF * S, "out_stats");
    check_vec(out_lstats, torch::kFloat32, NF * S, "out_lstats");
    TORCH_CHECK(S >= 1 && S <= 256, "tree_split supports <= 256 stats");
    TORCH_CHECK(cnt_stat >= -1 && cnt_stat < S,
                "cnt_stat must be -1 or a stat index");
    TORCH_CHECK(S <= 32 || is_cls != 0,
                "tree_split: more than 32 stats are class counts only "
                "(is_cls = 1)");
    TORCH_CHECK(S <= 32 || cnt_stat == -1,
                "tree_split: more than 32 stats have no counted variant "
                "(cnt_stat must be -1)");
    TORCH_CHECK(f >= 1 && nbins >= 1 && NF < (1LL << 31) &&
                    hist.numel() >= NF * f * nbins * S, "hist too small");
    TORCH_CHECK(missing == 0 || missing == 1, "missing must be 0 or 1");
    TORCH_CHECK((missing != 0) == given(out_mleft) || NF == 0,
                "out_mleft goes with missing = 1, and only with it");
    if (missing) {
        if (NF > 0) check_vec(*out_mleft, torch::kInt32, NF, "out_mleft");
        TORCH_CHECK(nbins >= 2, "missing mode needs nbins >= 2");
        TORCH_CHECK(extra_mode == 0,
                    "missing mode has no extra_mode (random thresholds)");
    }
    if (NF == 0) return;
    launched(skdist_tree_split(
        hist.data_ptr(), node_seed.data_ptr(), (int)NF, (int)f, (int)nbins,
        (int)S, (int)is_cls, (int)crit, (int)m_features, (int)extra_mode,
        (float)min_leaf, (int)cnt_stat, out_feat.data_ptr(),
        out_bin.data_ptr(), out_wl.data_ptr(), out_gain.data_ptr(),
        out_imp.data_ptr(), out_stats.data_ptr(), out_lstats.data_ptr(),
        (int)missing, missing ? out_mleft->data_ptr() : nullptr,
        cur_stream()), "tree_split");
}

// split_feat / split_bin / split_mleft are indexed by the chunk table's
// part_slot; split_mleft (int32 [n_parts], optional) sends the rows whose
// code is missing_code left as well
int64_t check_part(const torch::Tensor& codes, const torch::Tensor& si,
                   const torch::Tensor& chunks,
                   const torch::Tensor& split_feat,
                   const torch::Tensor& split_bin,
                   const OptTensor& split_mleft, int64_t missing_code,
                   int64_t n) {
    check_codes(codes, n);
    check_plane(si, torch::kInt32, n, "sample_idx");
    check_t(split_feat, torch::kInt32, "split_feat");
    check_vec(split_bin, torch::kInt32, split_feat.numel(), "split_bin");
    if (given(split_mleft)) {
        check_vec(*split_mleft, torch::kInt32, split_feat.numel(),
                  "split_mleft");
        TORCH_CHECK(missing_code >= 0 && missing_code <= 255,
                    "missing_code must be a uint8 code with split_mleft");
    }
    return check_chunks(chunks);
}

void part_count(torch::Tensor codes, torch::Tensor sample_idx,
                torch::Tensor chunks, torch::Tensor split_feat,
                torch::Tensor split_bin, int64_t n,
                torch::Tensor out_counts, OptTensor split_mleft,
                int64_t missing_code) {
    const int64_t n_chunks = check_part(codes, sample_idx, chunks,
                                        split_feat, split_bin, split_mleft,
                                        missing_code, n);
    check_vec(out_counts, torch::kInt32, n_chunks, "out_counts");
    if (n_chunks == 0) return;
    launched(skdist_part_count(
        codes.data_ptr(), sample_idx.data_ptr(), chunks.data_ptr(),
        split_feat.data_ptr(), split_bin.data_ptr(),
        given(split_mleft) ? split_mleft->data_ptr() : nullptr,
        (int)missing_code, n, (int)codes.size(1), (int)n_chunks,
        out_counts.data_ptr(), cur_stream()), "part_count");
}

void part_scatter(torch::Tensor codes, torch::Tensor sample_idx_in,
                  torch::Tensor chunks, torch::Tensor split_feat,
                  torch::Tensor split_bin, torch::Tensor left_base,
                  torch::Tensor right_base, int64_t n,
                  torch::Tensor sample_idx_out, OptTensor split_mleft,
                  int64_t missing_code) {
    const int64_t n_chunks = check_part(codes, sample_idx_in, chunks,
                                        split_feat, split_bin, split_mleft,
                                        missing_code, n);
    check_2d(sample_idx_out, torch::kInt32, sample_idx_in.size(0), n,
             "sample_idx_out");
    check_vec(left_base, torch::kInt32, n_chunks, "left_base");
    check_vec(right_base, torch::kInt32, n_chunks, "right_base");
    if (n_chunks == 0) return;
    launched(skdist_part_scatter(
        codes.data_ptr(), sample_idx_in.data_ptr(), chunks.data_ptr(),
        split_feat.data_ptr(), split_bin.data_ptr(),
        given(split_mleft) ? split_mleft->data_ptr() : nullptr,
        (int)missing_code, left_base.data_ptr(), right_base.data_ptr(), n,
        (int)codes.size(1), (int)n_chunks, sample_idx_out.data_ptr(),
        cur_stream()), "part_scatter");
}

// dense X [rows, f] f32; returns rows
int64_t check_dense_x(const torch::Tensor& X) {
    check_t(X, torch::kFloat32, "X");
    TORCH_CHECK(X.dim() == 2 && X.size(1) >= 1 && X.size(1) < (1LL << 31),
                "X must be [rows, f]");
    return X.size(0);
}

void forest_predict(torch::Tensor X, torch::Tensor feat, torch::Tensor thr,
                    torch::Tensor left, torch::Tensor right,
                    torch::Tensor roots, torch::Tensor values,
                    torch::Tensor out, OptTensor mleft) {
    const int64_t rows = check_dense_x(X);
    check_nodes(feat, thr, left, right, roots);
    const void* ml = check_mleft(mleft, feat);
    const int64_t vs = check_payload(values, out, rows);
    if (rows == 0) return;
    launched(skdist_forest_predict(
        X.data_ptr(), feat.data_ptr(), thr.data_ptr(), left.data_ptr(),
        right.data_ptr(), roots.data_ptr(), values.data_ptr(), ml,
        out.data_ptr(), rows, (int)X.size(1), (int)roots.numel(), (int)vs,
        cur_stream()), "forest_predict");
}

void forest_apply(torch::Tensor X, torch::Tensor feat, torch::Tensor thr,
                  torch::Tensor left, torch::Tensor right,
                  torch::Tensor roots, torch::Tensor out_leaf,
                  OptTensor mleft) {
    const int64_t rows = check_dense_x(X);
    check_nodes(feat, thr, left, right, roots);
    const void* ml = check_mleft(mleft, feat);
    check_2d(out_leaf, torch::kInt32, rows, roots.numel(), "out_leaf");
    if (rows == 0) return;
    launched(skdist_forest_apply(
        X.data_ptr(), feat.data_ptr(), thr.data_ptr(), left.data_ptr(),
        right.data_ptr(), roots.data_ptr(), ml, out_leaf.data_ptr(), rows,
        (int)X.size(1), (int)roots.numel(), cur_stream()), "forest_apply");
}

void forest_predict_csr(torch::Tensor indptr, torch::Tensor indices,
                        torch::Tensor data, torch::Tensor feat,
                        torch::Tensor thr, torch::Tensor left,
                        torch::Tensor right, torch::Tensor roots,
                        torch::Tensor values, torch::Tensor out,
                        OptTensor mleft) {
    const int64_t rows = rows_of(out);
    check_csr(indptr, indices, data, rows);
    check_nodes(feat, thr, left, right, roots);
    const void* ml = check_mleft(mleft, feat);
    const int64_t vs = check_payload(values, out, rows);
    if (rows == 0) return;
    launched(skdist_forest_predict_csr(
        indptr.data_ptr(), indices.data_ptr(), data.data_ptr(),
        feat.data_ptr(), thr.data_ptr(), left.data_ptr(),
        right.data_ptr(), roots.data_ptr(), values.data_ptr(), ml,
        out.data_ptr(), rows, indices.numel(), (int)roots.numel(),
        (int)vs, cur_stream()), "forest_predict_csr");
}

void forest_apply_csr(torch::Tensor indptr, torch::Tensor indices,
                      torch::Tensor data, torch::Tensor feat,
                      torch::Tensor thr, torch::Tensor left,
                      torch::Tensor right, torch::Tensor roots,
                      torch::Tensor out_leaf, OptTensor mleft) {
    const int64_t rows = rows_of(out_leaf);
    check_csr(indptr, indices, data, rows);
    check_nodes(feat, thr, left, right, roots);
    const void* ml = check_mleft(mleft, feat);
    check_2d(out_leaf, torch::kInt32, rows, roots.numel(), "out_leaf");
    if (rows == 0) return;
    launched(skdist_forest_apply_csr(
        indptr.data_ptr(), indices.data_ptr(), data.data_ptr(),
        feat.data_ptr(), thr.data_ptr(), left.data_ptr(),
        right.data_ptr(), roots.data_ptr(), ml, out_leaf.data_ptr(), rows,
        indices.numel(), (int)roots.numel(), cur_stream()),
        "forest_apply_csr");
}

void bin_csr(torch::Tensor indptr, torch::Tensor indices,
             torch::Tensor data, torch::Tensor edges, torch::Tensor zc,
             torch::Tensor codes, int64_t f) {
    const int64_t n = rows_of(codes);
    check_csr(indptr, indices, data, n);
    const int64_t fp = check_codes(codes, n);
    check_vec(zc, torch::kUInt8, fp, "zc");
    TORCH_CHECK(f >= 1 && f <= fp, "fp must be f padded to a multiple of 4");
    check_t(edges, torch::kFloat32, "edges");
    TORCH_CHECK(edges.dim() == 2 && edges.size(0) == f &&
                    edges.size(1) <= 255,
                "edges must be f32 [f, nbins-1] with nbins <= 256");
    if (n == 0) return;
    launched(skdist_bin_csr(
        indptr.data_ptr(), indices.data_ptr(), data.data_ptr(),
        edges.data_ptr(), zc.data_ptr(), codes.data_ptr(), n,
        indices.numel(), (int)f, (int)fp, (int)edges.size(1), cur_stream()),
        "bin_csr");
}

// stats: [ncols_pad * 2] (mode 0: hits, rows) or [ncols_pad] (mode 1: sse),
// zeroed by the caller; the kernel adds into it
void score_fold(torch::Tensor Xf, torch::Tensor WbfT, torch::Tensor yf,
                torch::Tensor out, int64_t mode) {
    TORCH_CHECK(mode == 0 || mode == 1, "mode must be 0 or 1");
    check_t(Xf, torch::kBFloat16, "Xf");
    TORCH_CHECK(Xf.dim() == 2 && Xf.size(0) >= 128 &&
                Xf.size(0) % 128 == 0, "m_pad must be a mult of 128");
    const int64_t m_pad = Xf.size(0), fa = Xf.size(1);
    TORCH_CHECK(fa >= 32 && fa % 32 == 0, "fa must be a multiple of 32");
    check_t(WbfT, torch::kBFloat16, "WbfT");
    TORCH_CHECK(WbfT.dim() == 2 && WbfT.size(1) == fa &&
                WbfT.size(0) >= 128 && WbfT.size(0) % 128 == 0,
                "WbfT must be [ncols_pad, fa], ncols_pad a mult of 128");
    const int64_t ncols_pad = WbfT.size(0);
    check_vec(yf, torch::kFloat32, m_pad, "yf");
    check_vec(out, torch::kFloat32, ncols_pad * (mode == 0 ? 2 : 1),
              "stats");
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_score(
        Xf.data_ptr(), WbfT.data_ptr(), yf.data_ptr(), out.data_ptr(),
        m_pad, (int)fa, (int)ncols_pad, (int)mode, stream);
    TORCH_CHECK(err == hipSuccess, "score_fold: ", hipGetErrorString(err));
}

void standardize(torch::Tensor X, torch::Tensor mean,
                 torch::Tensor inv_std, torch::Tensor out, int64_t f) {
    check_t(out, torch::kBFloat16, "out");
    TORCH_CHECK(out.dim() == 2, "out must be [n, fa]");
    const int64_t n = out.size(0), fa = out.size(1);
    TORCH_CHECK(fa % 8 == 0, "fa must be a multiple of 8");
    TORCH_CHECK(f >= 1 && f < fa, "f must be in [1, fa)");
    check_2d(X, torch::kFloat32, n, f, "X");
    check_vec(mean, torch::kFloat32, f, "mean");
    check_vec(inv_std, torch::kFloat32, f, "inv_std");
    if (n == 0) return;
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_standardize(
        X.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), out.data_ptr(),
        n, (int)f, (int)fa, stream);
    TORCH_CHECK(err == hipSuccess, "standardize: ",
                hipGetErrorString(err));
}

void hash_vectorize(torch::Tensor bytes, torch::Tensor doc_off,
                    int64_t mode, int64_t min_n, int64_t max_n,
                    int64_t n_features, int64_t alt_sign,
                    torch::Tensor out_keys, torch::Tensor out_vals,
                    torch::Tensor ctr) {
    for (auto* t : {&bytes, &doc_off, &out_keys, &out_vals, &ctr}) {
        CHECK_DEV(*t);
        CHECK_CONT(*t);
    }
    TORCH_CHECK(bytes.scalar_type() == torch::kUInt8, "bytes must be u8");
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_hash_vectorize(
        bytes.data_ptr(), doc_off.data_ptr(), doc_off.size(0) - 1,
        (int)mode, (int)min_n, (int)max_n, (int)n_features, (int)alt_sign,
        out_keys.data_ptr(), out_vals.data_ptr(), ctr.data_ptr(),
        out_keys.size(0), stream);
    TORCH_CHECK(err == hipSuccess, "hash_vectorize: ",
                hipGetErrorString(err));
}

// UTF-8 tokenizer: word_tbl is the \w bitmap over U+0000..U+10FFFF
// (0x110000/32 int32 words), ws_list the sorted \s code points, and ctr
// holds {pair count, overflow flag}.
void hash_vectorize_utf8(torch::Tensor bytes, torch::Tensor doc_off,
                         int64_t mode, int64_t min_n, int64_t max_n,
                         int64_t n_features, int64_t alt_sign,
                         torch::Tensor word_tbl, torch::Tensor ws_list,
                         torch::Tensor out_keys, torch::Tensor out_vals,
                         torch::Tensor ctr) {
    for (auto* t : {&bytes, &doc_off, &word_tbl, &ws_list, &out_keys,
                    &out_vals, &ctr}) {
        CHECK_DEV(*t);
        CHECK_CONT(*t);
    }
    TORCH_CHECK(bytes.scalar_type() == torch::kUInt8, "bytes must be u8");
    TORCH_CHECK(doc_off.scalar_type() == torch::kInt64 &&
                    doc_off.numel() >= 1,
                "doc_off must be int64 [n_docs + 1]");
    TORCH_CHECK(word_tbl.scalar_type() == torch::kInt32 &&
                    word_tbl.numel() == 0x110000 / 32,
                "word_tbl must be int32 [0x110000 / 32]");
    TORCH_CHECK(ws_list.scalar_type() == torch::kInt32 &&
                    ws_list.numel() <= 64,
                "ws_list must be int32 with at most 64 entries");
    TORCH_CHECK(ctr.scalar_type() == torch::kInt64 && ctr.numel() >= 2,
                "ctr must be int64 [2]: {count, overflow}");
    TORCH_CHECK(out_vals.numel() >= out_keys.numel(),
                "out_vals shorter than out_keys");
    TORCH_CHECK(mode == 0 || mode == 1, "mode must be 0 or 1");
    TORCH_CHECK(min_n >= 1 && max_n <= (mode == 0 ? 8 : 32),
                "ngram_range outside the kernel's limits "
                "(word: 1..8 tokens, char_wb: 1..32 characters)");
    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipError_t err = skdist_hash_vectorize_utf8(
        bytes.data_ptr(), doc_off.data_ptr(), doc_off.size(0) - 1,
        (int)mode, (int)min_n, (int)max_n, (int)n_features, (int)alt_sign,
        word_tbl.data_ptr(), ws_list.data_ptr(), (int)ws_list.numel(),
        out_keys.data_ptr(), out_vals.data_ptr(), ctr.data_ptr(),
        out_keys.size(0), stream);
    TORCH_CHECK(err == hipSuccess, "hash_vectorize_utf8: ",
                hipGetErrorString(err));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    // the tensors every dense step entry takes first, in order; naming
    // the arguments lets the trailing group_k (softmax group width)
    // default to 0, so positional calls without it keep working
    #define STEP_TENSORS                                                    \
        py::arg("Xs"), py::arg("XsT"), py::arg("GT"), py::arg("W"),         \
        py::arg("V"), py::arg("WbfT"), py::arg("partial"), py::arg("y"),    \
        py::arg("fold"), py::arg("col_class"), py::arg("col_fold"),         \
        py::arg("col_class2"), py::arg("col_lr"), py::arg("col_l2"),        \
        py::arg("fmask"), py::arg("row_w")
    m.def("sgd_step", &sgd_step, "fused batched SGD step (K1+K2+K3)",
          STEP_TENSORS, py::arg("start"), py::arg("m"), py::arg("loss_id"),
          py::arg("lr_scale"), py::arg("momentum"),
          py::arg("intercept_row"), py::arg("inv_m"),
          py::arg("group_k") = 0);
    m.def("sgd_epoch", &sgd_epoch, "one epoch of fused SGD steps",
          STEP_TENSORS, py::arg("inv_m"), py::arg("batch_size"),
          py::arg("loss_id"), py::arg("lr_scale"), py::arg("momentum"),
          py::arg("intercept_row"), py::arg("group_k") = 0);
    m.def("grad_partial", &grad_partial,
          "K2 of one dense SGD step alone (variant: 0 rule, 1 128-row, "
          "2 96-row, 3 whole-fa)");
    m.def("sp_sgd_epoch", &sp_sgd_epoch,
          "one epoch of the sparse text-scale solver");
    m.def("sgd_epoch_l1", &sgd_epoch_l1,
          "one epoch of fused SGD steps with the L1 update",
          STEP_TENSORS, py::arg("inv_m"), py::arg("batch_size"),
          py::arg("loss_id"), py::arg("lr_scale"), py::arg("momentum"),
          py::arg("intercept_row"), py::arg("col_l1"), py::arg("cpos"),
          py::arg("cneg"), py::arg("group_k") = 0);
    m.def("sgd_solve_l1", &sgd_solve_l1,
          "all epochs with the L1 update (hipGraph replay)",
          STEP_TENSORS, py::arg("inv_m"), py::arg("batch_size"),
          py::arg("loss_id"), py::arg("momentum"), py::arg("intercept_row"),
          py::arg("epochs"), py::arg("col_l1"), py::arg("cpos"),
          py::arg("cneg"), py::arg("group_k") = 0);
    m.def("sgd_solve", &sgd_solve,
          "all epochs of the dense solver (hipGraph-replayed)",
          STEP_TENSORS, py::arg("inv_m"), py::arg("batch_size"),
          py::arg("loss_id"), py::arg("momentum"), py::arg("intercept_row"),
          py::arg("epochs"), py::arg("group_k") = 0);
    #define BITS_TAIL                                                       \
        py::arg("tbits"), py::arg("mbits"),                                 \
        py::arg("col_l1") = torch::empty({0}),                              \
        py::arg("cpos") = torch::empty({0}),                                \
        py::arg("cneg") = torch::empty({0})
    m.def("sgd_step_bits", &sgd_step_bits,
          "fused SGD step with per-element targets (k_fwd_gt_bits)",
          STEP_TENSORS, py::arg("start"), py::arg("m"), py::arg("loss_id"),
          py::arg("lr_scale"), py::arg("momentum"),
          py::arg("intercept_row"), py::arg("inv_m"), BITS_TAIL);
    m.def("sgd_epoch_bits", &sgd_epoch_bits,
          "one epoch of SGD steps with per-element targets",
          STEP_TENSORS, py::arg("inv_m"), py::arg("batch_size"),
          py::arg("loss_id"), py::arg("lr_scale"), py::arg("momentum"),
          py::arg("intercept_row"), BITS_TAIL);
    m.def("sgd_solve_bits", &sgd_solve_bits,
          "all epochs with per-element targets (hipGraph replay)",
          STEP_TENSORS, py::arg("inv_m"), py::arg("batch_size"),
          py::arg("loss_id"), py::arg("momentum"), py::arg("intercept_row"),
          py::arg("epochs"), BITS_TAIL);
    #undef BITS_TAIL
    #undef STEP_TENSORS
    m.def("sp_sgd_solve", &sp_sgd_solve,
          "all epochs of the sparse solver (hipGraph-replayed)");
    m.def("sp_sgd_epoch_l1", &sp_sgd_epoch_l1,
          "one epoch of sparse SGD steps with the lazy L1 update");
    m.def("sp_l1_flush", &sp_l1_flush, "end-of-fit L1 flush");
    m.def("sp_renorm_l1", &sp_renorm_l1,
          "fold the lazy-L2 scale into W and the L1 tables");
    m.def("sp_forward", &sp_forward, "sparse decision values (scoring)");
    m.def("sp_renorm", &sp_renorm, "fold the lazy-L2 scale into W");
    m.def("score_fold", &score_fold,
          "fused fold-scoring GEMM + per-column stats");
    m.def("standardize", &standardize,
          "fused standardize + augment + bf16 cast");
    m.def("hash_vectorize", &hash_vectorize,
          "tokenize + murmur3 feature hashing -> COO pairs");
    m.def("hash_vectorize_utf8", &hash_vectorize_utf8,
          "UTF-8 tokenize + murmur3 feature hashing -> COO pairs");
    // the trailing arguments with defaults are the class-group width and
    // the missing-value ones; every entry keeps its earlier positional
    // argument list
    namespace py = pybind11;
    m.def("tree_hist", &tree_hist,
          "per-(node,feature,bin) stats: class counts, (w,wy,wyy), or "
          "(W,Wy,Wyy,C) with f32 row weights; cg > 0 splits the class "
          "counts into class groups of cg, one LDS tile each",
          py::arg("codes"), py::arg("y_int"), py::arg("y_f"),
          py::arg("row_w"), py::arg("weights"), py::arg("sample_idx"),
          py::arg("chunks"), py::arg("hist"), py::arg("n"), py::arg("f"),
          py::arg("nbins"), py::arg("fg"), py::arg("cg") = -1);
    m.def("tree_split", &tree_split,
          "best split per frontier node; min-leaf on the weight sums "
          "(cnt_stat = -1) or on a count stat; missing = 1 scans both "
          "directions of the missing bin nbins-1 and fills out_mleft",
          py::arg("hist"), py::arg("node_seed"), py::arg("f"),
          py::arg("nbins"), py::arg("S"), py::arg("is_cls"),
          py::arg("crit"), py::arg("m_features"), py::arg("extra_mode"),
          py::arg("min_leaf"), py::arg("out_feat"), py::arg("out_bin"),
          py::arg("out_wl"), py::arg("out_gain"), py::arg("out_imp"),
          py::arg("out_stats"), py::arg("out_lstats"), py::arg("cnt_stat"),
          py::arg("missing") = 0, py::arg("out_mleft") = py::none());
    m.def("part_count", &part_count, "partition phase A: left counts",
          py::arg("codes"), py::arg("sample_idx"), py::arg("chunks"),
          py::arg("split_feat"), py::arg("split_bin"), py::arg("n"),
          py::arg("out_counts"), py::arg("split_mleft") = py::none(),
          py::arg("missing_code") = -1);
    m.def("part_scatter", &part_scatter, "partition phase B: scatter",
          py::arg("codes"), py::arg("sample_idx_in"), py::arg("chunks"),
          py::arg("split_feat"), py::arg("split_bin"),
          py::arg("left_base"), py::arg("right_base"), py::arg("n"),
          py::arg("sample_idx_out"), py::arg("split_mleft") = py::none(),
          py::arg("missing_code") = -1);
    m.def("forest_predict", &forest_predict, "batched forest inference",
          py::arg("X"), py::arg("feat"), py::arg("thr"), py::arg("left"),
          py::arg("right"), py::arg("roots"), py::arg("values"),
          py::arg("out"), py::arg("mleft") = py::none());
    m.def("forest_apply", &forest_apply, "leaf ids per (row, tree)",
          py::arg("X"), py::arg("feat"), py::arg("thr"), py::arg("left"),
          py::arg("right"), py::arg("roots"), py::arg("out_leaf"),
          py::arg("mleft") = py::none());
    m.def("forest_predict_csr", &forest_predict_csr,
          "batched forest inference over CSR rows", py::arg("indptr"),
          py::arg("indices"), py::arg("data"), py::arg("feat"),
          py::arg("thr"), py::arg("left"), py::arg("right"),
          py::arg("roots"), py::arg("values"), py::arg("out"),
          py::arg("mleft") = py::none());
    m.def("forest_apply_csr", &forest_apply_csr,
          "leaf ids per (row, tree) over CSR rows", py::arg("indptr"),
          py::arg("indices"), py::arg("data"), py::arg("feat"),
          py::arg("thr"), py::arg("left"), py::arg("right"),
          py::arg("roots"), py::arg("out_leaf"),
          py::arg("mleft") = py::none());
    m.def("bin_csr", &bin_csr, "CSR -> uint8 quantile codes");
}
