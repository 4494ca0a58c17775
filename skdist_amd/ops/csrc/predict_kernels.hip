// Batched forest inference — CDNA4 (gfx950) kernels.
//
// Device analog of the reference's executor-side model.predict inside the
// pandas UDF (skdist/distribute/predict.py:160-178) for tree ensembles:
// the fitted forest is flattened into four node arrays + a leaf-value
// table resident in HBM (small enough to sit in L2/L3), and every thread
// walks all trees for one row, accumulating leaf payloads in registers.
//
// There is ONE walk (descend) and ONE apply body, templated on a row
// accessor with a single `float at(int jf)` and on a bool MISS (NaN
// follows a per-node direction flag), and two predict bodies by payload
// width: predict_row (vs <= 32, one thread per row, the payload in
// registers) and predict_row_wide (32 < vs <= 256, one wave per row, the
// payload across the lanes).  The twelve kernels are {predict, predict
// wide, apply} x dense/CSR x MISS instantiations of them.  Trees go in
// order t = 0..T-1 in every body, so the accumulation order — and
// therefore every output bit — is the same for a CSR row and for its
// dense copy.
//
// Layouts:
//   X       [rows][f]  f32 row-major
//   feat    [total_nodes] int32   (-1 = leaf; leaf's `left` indexes values)
//   thr     [total_nodes] f32     (x[feat] <= thr  → left)
//   left/right [total_nodes] int32 (absolute node ids, pre-offset per tree)
//   roots   [n_trees] int32
//   values  [n_values][vs] f32
//   mleft   [total_nodes] uint8   (MISS kernels: 1 = NaN goes left here)
//
// CSR rows (scipy-sparse X, never densified):
//   indptr  [rows+1] int64   (rebased so indptr[0] == 0 for the chunk)
//   indices [nnz]    int32   ascending within each row, no duplicates
//   data    [nnz]    f32
#include "common.h"
#include "tree_api.h"

#define MAXVS 32        // widest payload of the thread-per-row predict
#define MAXVS_WIDE 256  // widest payload of the wave-per-row predict
#define WAVE 64

struct DenseRow {
    const float* __restrict__ x;
    __device__ __forceinline__ DenseRow(const float* X, long long r, int f)
        : x(X + r * f) {}
    __device__ __forceinline__ float at(int jf) const { return x[jf]; }
};

static __device__ __forceinline__ float csr_lookup(
    const int* __restrict__ indices, const float* __restrict__ data,
    long long lo, long long hi, int jf) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        const int c = indices[mid];
        if (c < jf) lo = mid + 1;
        else if (c > jf) hi = mid;
        else return data[mid];
    }
    return 0.f;
}

// x[jf] is a binary search of the row's index range [lo, hi): the stored
// value when column jf is present, 0.0f otherwise.  Any nnz per row from 0
// to f takes this one path.
struct CsrRow {
    const int* __restrict__ indices;
    const float* __restrict__ data;
    long long lo, hi;
    __device__ __forceinline__ CsrRow(const long long* indptr,
                                      const int* indices_,
                                      const float* data_, long long r,
                                      long long nnz)
        : indices(indices_), data(data_), lo(indptr[r]), hi(indptr[r + 1]) {
        if (lo < 0) lo = 0;
        if (hi > nnz) hi = nnz;
    }
    __device__ __forceinline__ float at(int jf) const {
        return csr_lookup(indices, data, lo, hi, jf);
    }
};

// root-to-leaf descent of tree t; returns the leaf's node id.
// MISS: a NaN value (x <= thr is false for it) goes left at the nodes whose
// mleft flag is set; without MISS mleft is not read and NaN goes right.
template <bool MISS, typename Row>
static __device__ __forceinline__ int descend(
    const Row& row, const int* __restrict__ feat,
    const float* __restrict__ thr, const int* __restrict__ left,
    const int* __restrict__ right, const int* __restrict__ roots,
    const unsigned char* __restrict__ mleft, int t) {
    int node = roots[t];
    int jf = feat[node];
    while (jf >= 0) {
        const float x = row.at(jf);
        bool go_left = x <= thr[node];
        if (MISS) go_left = go_left || (x != x && mleft[node] != 0);
        node = go_left ? left[node] : right[node];
        jf = feat[node];
    }
    return node;
}

// mean leaf payload over the trees -> out[r][0..vs)
template <bool MISS, typename Row>
static __device__ __forceinline__ void predict_row(
    const Row& row, const int* __restrict__ feat,
    const float* __restrict__ thr, const int* __restrict__ left,
    const int* __restrict__ right, const int* __restrict__ roots,
    const float* __restrict__ values,
    const unsigned char* __restrict__ mleft, float* __restrict__ out,
    long long r, int n_trees, int vs) {
    float acc[MAXVS];
#pragma unroll
    for (int c = 0; c < MAXVS; ++c) acc[c] = 0.f;
    for (int t = 0; t < n_trees; ++t) {
        const int node =
            descend<MISS>(row, feat, thr, left, right, roots, mleft, t);
        const float* v = values + (long long)left[node] * vs;
#pragma unroll
        for (int c = 0; c < MAXVS; ++c)
            if (c < vs) acc[c] += v[c];
    }
    const float inv = 1.f / (float)n_trees;
#pragma unroll
    for (int c = 0; c < MAXVS; ++c)
        if (c < vs) out[r * vs + c] = acc[c] * inv;
}

// predict_row for MAXVS < vs <= MAXVS_WIDE, called by a whole wave for ONE
// row: all 64 lanes walk the same root-to-leaf path (uniform control flow,
// every node load a broadcast), then lane l adds the leaf's payload values
// l, l+64, l+128, l+192 — coalesced along vs, at most 4 accumulators.
template <bool MISS, typename Row>
static __device__ __forceinline__ void predict_row_wide(
    const Row& row, const int* __restrict__ feat,
    const float* __restrict__ thr, const int* __restrict__ left,
    const int* __restrict__ right, const int* __restrict__ roots,
    const float* __restrict__ values,
    const unsigned char* __restrict__ mleft, float* __restrict__ out,
    long long r, int n_trees, int vs) {
    const int lane = threadIdx.x & (WAVE - 1);
    float acc[MAXVS_WIDE / WAVE];
#pragma unroll
    for (int k = 0; k < MAXVS_WIDE / WAVE; ++k) acc[k] = 0.f;
    for (int t = 0; t < n_trees; ++t) {
        const int node =
            descend<MISS>(row, feat, thr, left, right, roots, mleft, t);
        const float* v = values + (long long)left[node] * vs;
#pragma unroll
        for (int k = 0; k < MAXVS_WIDE / WAVE; ++k)
            if (lane + k * WAVE < vs) acc[k] += v[lane + k * WAVE];
    }
    const float inv = 1.f / (float)n_trees;
#pragma unroll
    for (int k = 0; k < MAXVS_WIDE / WAVE; ++k)
        if (lane + k * WAVE < vs) out[r * vs + lane + k * WAVE] = acc[k] * inv;
}

// leaf node id per tree -> out_leaf[r][0..n_trees)
template <bool MISS, typename Row>
static __device__ __forceinline__ void apply_row(
    const Row& row, const int* __restrict__ feat,
    const float* __restrict__ thr, const int* __restrict__ left,
    const int* __restrict__ right, const int* __restrict__ roots,
    const unsigned char* __restrict__ mleft, int* __restrict__ out_leaf,
    long long r, int n_trees) {
    for (int t = 0; t < n_trees; ++t)
        out_leaf[r * n_trees + t] =
            descend<MISS>(row, feat, thr, left, right, roots, mleft, t);
}

// The twelve kernels: {predict, predict wide, apply} x {dense, CSR} x
// {plain, _m}.  The plain ones are the MISS = false instantiations and take
// no mleft.  ROW is the row a thread works on: its own (THREAD_ROW), or its
// wave's with 4 rows per 256-thread block (WAVE_ROW, the wide body).
#define THREAD_ROW ((long long)blockIdx.x * blockDim.x + threadIdx.x)
#define WAVE_ROW                                                            \
    ((long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE)

#define FOREST_PREDICT_KERNEL(NAME, BODY, ROW, MISS, MLEFT_PARAM, MLEFT)    \
    extern "C" __global__ __launch_bounds__(256) void NAME(                 \
        const float* __restrict__ X, const int* __restrict__ feat,          \
        const float* __restrict__ thr, const int* __restrict__ left,        \
        const int* __restrict__ right, const int* __restrict__ roots,       \
        const float* __restrict__ values, MLEFT_PARAM                       \
        float* __restrict__ out, long long rows, int f, int n_trees,        \
        int vs) {                                                           \
        const long long r = ROW;                                            \
        if (r >= rows) return;                                              \
        BODY<MISS>(DenseRow(X, r, f), feat, thr, left, right, roots,        \
                   values, MLEFT, out, r, n_trees, vs);                     \
    }

#define FOREST_APPLY_KERNEL(NAME, MISS, MLEFT_PARAM, MLEFT)                 \
    extern "C" __global__ __launch_bounds__(256) void NAME(                 \
        const float* __restrict__ X, const int* __restrict__ feat,          \
        const float* __restrict__ thr, const int* __restrict__ left,        \
        const int* __restrict__ right, const int* __restrict__ roots,       \
        MLEFT_PARAM int* __restrict__ out_leaf, long long rows, int f,      \
        int n_trees) {                                                      \
        const long long r =                                                 \
            (long long)blockIdx.x * blockDim.x + threadIdx.x;               \
        if (r >= rows) return;                                              \
        apply_row<MISS>(DenseRow(X, r, f), feat, thr, left, right, roots,   \
                        MLEFT, out_leaf, r, n_trees);                       \
    }

#define FOREST_PREDICT_CSR_KERNEL(NAME, BODY, ROW, MISS, MLEFT_PARAM,       \
                                  MLEFT)                                    \
    extern "C" __global__ __launch_bounds__(256) void NAME(                 \
        const long long* __restrict__ indptr,                               \
        const int* __restrict__ indices, const float* __restrict__ data,    \
        const int* __restrict__ feat, const float* __restrict__ thr,        \
        const int* __restrict__ left, const int* __restrict__ right,        \
        const int* __restrict__ roots, const float* __restrict__ values,    \
        MLEFT_PARAM float* __restrict__ out, long long rows,                \
        long long nnz, int n_trees, int vs) {                               \
        const long long r = ROW;                                            \
        if (r >= rows) return;                                              \
        BODY<MISS>(CsrRow(indptr, indices, data, r, nnz), feat, thr, left,  \
                   right, roots, values, MLEFT, out, r, n_trees, vs);       \
    }

#define FOREST_APPLY_CSR_KERNEL(NAME, MISS, MLEFT_PARAM, MLEFT)             \
    extern "C" __global__ __launch_bounds__(256) void NAME(                 \
        const long long* __restrict__ indptr,                               \
        const int* __restrict__ indices, const float* __restrict__ data,    \
        const int* __restrict__ feat, const float* __restrict__ thr,        \
        const int* __restrict__ left, const int* __restrict__ right,        \
        const int* __restrict__ roots, MLEFT_PARAM                          \
        int* __restrict__ out_leaf, long long rows, long long nnz,          \
        int n_trees) {                                                      \
        const long long r =                                                 \
            (long long)blockIdx.x * blockDim.x + threadIdx.x;               \
        if (r >= rows) return;                                              \
        apply_row<MISS>(CsrRow(indptr, indices, data, r, nnz), feat, thr,   \
                        left, right, roots, MLEFT, out_leaf, r, n_trees);   \
    }

#define NO_MLEFT_PARAM
#define MLEFT_PARAM_ const unsigned char* __restrict__ mleft,
FOREST_PREDICT_KERNEL(k_forest_predict, predict_row, THREAD_ROW, false,
                      NO_MLEFT_PARAM, nullptr)
FOREST_PREDICT_KERNEL(k_forest_predict_m, predict_row, THREAD_ROW, true,
                      MLEFT_PARAM_, mleft)
FOREST_PREDICT_KERNEL(k_forest_predict_wide, predict_row_wide, WAVE_ROW,
                      false, NO_MLEFT_PARAM, nullptr)
FOREST_PREDICT_KERNEL(k_forest_predict_wide_m, predict_row_wide, WAVE_ROW,
                      true, MLEFT_PARAM_, mleft)
FOREST_APPLY_KERNEL(k_forest_apply, false, NO_MLEFT_PARAM, nullptr)
FOREST_APPLY_KERNEL(k_forest_apply_m, true, MLEFT_PARAM_, mleft)
FOREST_PREDICT_CSR_KERNEL(k_forest_predict_csr, predict_row, THREAD_ROW,
                          false, NO_MLEFT_PARAM, nullptr)
FOREST_PREDICT_CSR_KERNEL(k_forest_predict_csr_m, predict_row, THREAD_ROW,
                          true, MLEFT_PARAM_, mleft)
FOREST_PREDICT_CSR_KERNEL(k_forest_predict_csr_wide, predict_row_wide,
                          WAVE_ROW, false, NO_MLEFT_PARAM, nullptr)
FOREST_PREDICT_CSR_KERNEL(k_forest_predict_csr_wide_m, predict_row_wide,
                          WAVE_ROW, true, MLEFT_PARAM_, mleft)
FOREST_APPLY_CSR_KERNEL(k_forest_apply_csr, false, NO_MLEFT_PARAM, nullptr)
FOREST_APPLY_CSR_KERNEL(k_forest_apply_csr_m, true, MLEFT_PARAM_, mleft)

// ---------------------------------------------------------------------- //
// C launchers: block 256, one thread per row (predict with vs <= MAXVS,
// apply) or one wave per row (predict with MAXVS < vs <= MAXVS_WIDE);
// mleft != nullptr picks the MISS instantiation
// ---------------------------------------------------------------------- //
static inline dim3 row_grid(long long rows) {
    return dim3((unsigned)((rows + 255) / 256));
}
// rows_per_block = 256 / WAVE; false where the grid would pass 2^31 - 1
static inline bool wave_grid(long long rows, dim3* grid) {
    const long long blocks = (rows + 256 / WAVE - 1) / (256 / WAVE);
    *grid = dim3((unsigned)blocks);
    return blocks <= 0x7fffffffLL;
}

extern "C" hipError_t skdist_forest_predict(
    const void* X, const void* feat, const void* thr, const void* left,
    const void* right, const void* roots, const void* values,
    const void* mleft, void* out, long long rows, int f, int n_trees,
    int vs, hipStream_t stream) {
    if (vs <= 0 || vs > MAXVS_WIDE) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    if (vs > MAXVS) {
        dim3 grid;
        if (!wave_grid(rows, &grid)) return hipErrorInvalidValue;
        if (mleft != nullptr)
            hipLaunchKernelGGL(k_forest_predict_wide_m, grid, dim3(256), 0,
                               stream, (const float*)X, (const int*)feat,
                               (const float*)thr, (const int*)left,
                               (const int*)right, (const int*)roots,
                               (const float*)values,
                               (const unsigned char*)mleft, (float*)out,
                               rows, f, n_trees, vs);
        else
            hipLaunchKernelGGL(k_forest_predict_wide, grid, dim3(256), 0,
                               stream, (const float*)X, (const int*)feat,
                               (const float*)thr, (const int*)left,
                               (const int*)right, (const int*)roots,
                               (const float*)values, (float*)out, rows, f,
                               n_trees, vs);
        return hipGetLastError();
    }
    if (mleft != nullptr)
        hipLaunchKernelGGL(k_forest_predict_m, row_grid(rows), dim3(256), 0,
                           stream, (const float*)X, (const int*)feat,
                           (const float*)thr, (const int*)left,
                           (const int*)right, (const int*)roots,
                           (const float*)values,
                           (const unsigned char*)mleft, (float*)out, rows,
                           f, n_trees, vs);
    else
        hipLaunchKernelGGL(k_forest_predict, row_grid(rows), dim3(256), 0,
                           stream, (const float*)X, (const int*)feat,
                           (const float*)thr, (const int*)left,
                           (const int*)right, (const int*)roots,
                           (const float*)values, (float*)out, rows, f,
                           n_trees, vs);
    return hipGetLastError();
}

extern "C" hipError_t skdist_forest_apply(
    const void* X, const void* feat, const void* thr, const void* left,
    const void* right, const void* roots, const void* mleft,
    void* out_leaf, long long rows, int f, int n_trees,
    hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (mleft != nullptr)
        hipLaunchKernelGGL(k_forest_apply_m, row_grid(rows), dim3(256), 0,
                           stream, (const float*)X, (const int*)feat,
                           (const float*)thr, (const int*)left,
                           (const int*)right, (const int*)roots,
                           (const unsigned char*)mleft, (int*)out_leaf,
                           rows, f, n_trees);
    else
        hipLaunchKernelGGL(k_forest_apply, row_grid(rows), dim3(256), 0,
                           stream, (const float*)X, (const int*)feat,
                           (const float*)thr, (const int*)left,
                           (const int*)right, (const int*)roots,
                           (int*)out_leaf, rows, f, n_trees);
    return hipGetLastError();
}

extern "C" hipError_t skdist_forest_predict_csr(
    const void* indptr, const void* indices, const void* data,
    const void* feat, const void* thr, const void* left, const void* right,
    const void* roots, const void* values, const void* mleft, void* out,
    long long rows, long long nnz, int n_trees, int vs,
    hipStream_t stream) {
    if (vs <= 0 || vs > MAXVS_WIDE) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    if (vs > MAXVS) {
        dim3 grid;
        if (!wave_grid(rows, &grid)) return hipErrorInvalidValue;
        if (mleft != nullptr)
            hipLaunchKernelGGL(k_forest_predict_csr_wide_m, grid, dim3(256),
                               0, stream, (const long long*)indptr,
                               (const int*)indices, (const float*)data,
                               (const int*)feat, (const float*)thr,
                               (const int*)left, (const int*)right,
                               (const int*)roots, (const float*)values,
                               (const unsigned char*)mleft, (float*)out,
                               rows, nnz, n_trees, vs);
        else
            hipLaunchKernelGGL(k_forest_predict_csr_wide, grid, dim3(256),
                               0, stream, (const long long*)indptr,
                               (const int*)indices, (const float*)data,
                               (const int*)feat, (const float*)thr,
                               (const int*)left, (const int*)right,
                               (const int*)roots, (const float*)values,
                               (float*)out, rows, nnz, n_trees, vs);
        return hipGetLastError();
    }
    if (mleft != nullptr)
        hipLaunchKernelGGL(k_forest_predict_csr_m, row_grid(rows),
                           dim3(256), 0, stream, (const long long*)indptr,
                           (const int*)indices, (const float*)data,
                           (const int*)feat, (const float*)thr,
                           (const int*)left, (const int*)right,
                           (const int*)roots, (const float*)values,
                           (const unsigned char*)mleft, (float*)out, rows,
                           nnz, n_trees, vs);
    else
        hipLaunchKernelGGL(k_forest_predict_csr, row_grid(rows), dim3(256),
                           0, stream, (const long long*)indptr,
                           (const int*)indices, (const float*)data,
                           (const int*)feat, (const float*)thr,
                           (const int*)left, (const int*)right,
                           (const int*)roots, (const float*)values,
                           (float*)out, rows, nnz, n_trees, vs);
    return hipGetLastError();
}

extern "C" hipError_t skdist_forest_apply_csr(
    const void* indptr, const void* indices, const void* data,
    const void* feat, const void* thr, const void* left, const void* right,
    const void* roots, const void* mleft, void* out_leaf, long long rows,
    long long nnz, int n_trees, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (mleft != nullptr)
        hipLaunchKernelGGL(k_forest_apply_csr_m, row_grid(rows), dim3(256),
                           0, stream, (const long long*)indptr,
                           (const int*)indices, (const float*)data,
                           (const int*)feat, (const float*)thr,
                           (const int*)left, (const int*)right,
                           (const int*)roots, (const unsigned char*)mleft,
                           (int*)out_leaf, rows, nnz, n_trees);
    else
        hipLaunchKernelGGL(k_forest_apply_csr, row_grid(rows), dim3(256), 0,
                           stream, (const long long*)indptr,
                           (const int*)indices, (const float*)data,
                           (const int*)feat, (const float*)thr,
                           (const int*)left, (const int*)right,
                           (const int*)roots, (int*)out_leaf, rows, nnz,
                           n_trees);
    return hipGetLastError();
}
