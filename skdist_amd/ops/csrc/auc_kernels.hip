// Exact ROC AUC fold scoring for gfx950: per column (model) of a fold, an
// LSD radix sort of the negatives' decision values and a tie-aware rank
// count of the positives against them.
//
// ZT [nm][M] fp32, one row per model: the fold's M decision values with the
// n_neg negatives first and the P = M - n_neg positives after them.
// scratch [nm][n_neg] int32.  out [nm] int64:
//   U2[c] = sum over positives p of  #{negatives z < z_p} + #{negatives z <= z_p}
// so that auc = U2 / (2 P N); U2 / 2 is the tie-aware rank sum.  U2 is an
// integer, so the result does not depend on any order of execution and is
// tested for equality.
//
// ZT IS CONSUMED: the sort ping-pongs between scratch and the negatives'
// part of the model's own row of ZT (ZT -> scratch -> ZT -> scratch -> ZT),
// which is why one scratch buffer is enough; afterwards that part holds the
// sorted keys, not decision values.  The positives' part is only read.
//
// One 256-lane workgroup owns one column from the first load to the one
// store of out[c]; nothing crosses workgroups, there are no global atomics.
//
//   key     -0.0 becomes +0.0 (what z + 0.0f does, done on the bits so that
//           no float mode can change it), then the order-preserving map of
//           the bit pattern: all bits of a negative flipped, the sign bit of
//           a non-negative set.  +-inf order by themselves, a NaN orders as
//           its bit pattern does.
//   hist    one sweep over the negatives adds into four 256-bin digit
//           histograms in LDS; wave w then turns table w into exclusive
//           base offsets (4 bins per lane, a shuffle scan over the wave).
//   passes  four stable passes, low byte first, keys only.  A tile is 256
//           consecutive keys, one per lane, the next tile's key already in
//           flight.  Within a wave a lane finds the lanes holding its digit
//           with eight 64-bit ballots, one per digit bit (lanes past the end
//           of the column are outside every mask); the first of them posts
//           the wave's count of the digit in wcnt[buf][wave][digit].  A
//           key's place is  base[digit] + counts of the waves before it +
//           its rank among its wave's equals.  Thread t then adds the
//           tile's four counts of digit t to base[t] and clears them.  wcnt
//           is double-buffered over tiles, which leaves two barriers per
//           tile.  A pass reads what the pass before scattered to global
//           memory from this same workgroup: a __syncthreads() separates
//           them.
//   count   a lane takes positives strided by 256, four at a time, and runs
//           a lower-bound and an upper-bound binary search over the sorted
//           keys for each in one loop of uniform length (eight independent
//           loads per step), adding both results to a 64-bit accumulator
//           (U2 passes 2^32 at 40,000 x 40,000 rows).  Lanes combine
//           through LDS in a fixed tree, lane 0 stores.
//
// k_ap_sums (average precision, described above the kernel) shares the key,
// the histograms and the passes, sorts both halves of the row and searches
// both.
//
// n_neg == 0 or P == 0 gives U2 = 0 and touches neither ZT nor scratch.
// Indices are 32-bit inside a column (M < 2^31, checked by the launcher);
// the column's base address is 64-bit.
//
// grid: nm workgroups of 256.  __launch_bounds__(256): see the resource
// line above the kernel.
#include "common.h"
#include "sgd_api.h"

#define AUC_TILE 256       // keys per tile = lanes per workgroup
#define AUC_ILP 4          // positives a lane searches for at a time
#define AUC_WCNT (4 * 256) // one buffer of per-wave digit counts

static __device__ __forceinline__ unsigned auc_key(unsigned u)
{
    if (u == 0x80000000u) u = 0u;  // -0.0 ties with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One stable pass over digit (key >> shift) & 255 of src[0..n) into dst.
// base: this pass's exclusive digit offsets, advanced tile by tile; wcnt:
// [2][4][256], all zero on entry and on return.  FROM_Z: src holds decision
// values, not keys yet.
template <bool FROM_Z>
static __device__ __forceinline__ void auc_radix_pass(
    const unsigned* src, unsigned* dst, unsigned n, int shift, int* base,
    int* wcnt, int tid)
{
    const int lane = tid & 63;
    const int w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned nxt = 0u;
    if ((unsigned)tid < n) nxt = src[tid];
    int buf = 0;
    for (unsigned t0 = 0; t0 < n; t0 += AUC_TILE, buf ^= 1) {
        const unsigned i = t0 + tid;
        const bool valid = i < n;
        const unsigned key = FROM_Z ? auc_key(nxt) : nxt;
        if (i + AUC_TILE < n) nxt = src[i + AUC_TILE];
        const unsigned d = (key >> shift) & 255u;
        // the valid lanes of this wave that hold digit d
        unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(bit);
            same &= bit ? bal : ~bal;
        }
        const int rank = __popcll(same & below);
        int* wc = wcnt + buf * AUC_WCNT;
        if (valid && rank == 0) wc[w * 256 + d] = __popcll(same);
        __syncthreads();
        if (valid) {
            unsigned pos = (unsigned)(base[d] + rank);
#pragma unroll
            for (int v = 0; v < 3; ++v)
                if (v < w) pos += (unsigned)wc[v * 256 + d];
            // the histograms make pos < n; the test keeps a wrong offset
            // from ever leaving the column
            if (pos < n) dst[pos] = key;
        }
        __syncthreads();
        // thread t is digit t: advance its offset past this tile, clear the
        // counts for the tile after next (which reuses this buffer)
        int tot = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            tot += wc[v * 256 + tid];
            wc[v * 256 + tid] = 0;
        }
        base[tid] += tot;
    }
    // the scattered keys are visible to the next reader, wcnt is all zero
    __syncthreads();
}

// The whole sort of one segment: A[0..n) decision values become their keys
// in ascending order, in place; B[0..n) is the other buffer of the
// ping-pong (A -> B -> A -> B -> A).  hist [4][256] is cleared and used
// here; wcnt is all zero on entry and on return.  Every lane of the
// workgroup calls it, behind a barrier after the last use of hist, A and B;
// n == 0 does nothing.
static __device__ __forceinline__ void auc_sort_keys(
    unsigned* A, unsigned* B, unsigned n, int* hist, int* wcnt, int tid)
{
    const int lane = tid & 63;
    const int w = tid >> 6;
#pragma unroll
    for (int v = 0; v < 4; ++v) hist[v * 256 + tid] = 0;
    __syncthreads();

    // all four digit histograms in one sweep
    for (unsigned i = tid; i < n; i += AUC_TILE) {
        const unsigned key = auc_key(A[i]);
        atomicAdd(&hist[key & 255u], 1);
        atomicAdd(&hist[256 + ((key >> 8) & 255u)], 1);
        atomicAdd(&hist[512 + ((key >> 16) & 255u)], 1);
        atomicAdd(&hist[768 + (key >> 24)], 1);
    }
    __syncthreads();
    {   // wave w: exclusive scan of table w, 4 bins per lane
        int* h = hist + w * 256 + 4 * lane;
        const int v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
        const int s = v0 + v1 + v2 + v3;
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        const int ex = inc - s;
        h[0] = ex;
        h[1] = ex + v0;
        h[2] = ex + v0 + v1;
        h[3] = ex + v0 + v1 + v2;
    }
    __syncthreads();

    auc_radix_pass<true>(A, B, n, 0, hist, wcnt, tid);
    auc_radix_pass<false>(B, A, n, 8, hist + 256, wcnt, tid);
    auc_radix_pass<false>(A, B, n, 16, hist + 512, wcnt, tid);
    auc_radix_pass<false>(B, A, n, 24, hist + 768, wcnt, tid);
}

// 30 VGPRs, 0 AGPRs, no scratch, 14336 B of LDS (gfx950, -O3): 8 waves per
// SIMD by registers, 8 workgroups per CU
extern "C" __global__ __launch_bounds__(256)
void k_auc_counts(
    float* ZT,            // [nm][M], negatives first; consumed
    int* scratch,         // [nm][n_neg]
    long long* out,       // [nm] U2
    unsigned M, unsigned n_neg)
{
    __shared__ int hist[4 * 256];            // digit counts, then offsets
    __shared__ int wcnt[2 * AUC_WCNT];       // [buf][wave][digit]
    __shared__ unsigned long long red[256];

    const int tid = threadIdx.x;
    const unsigned n = n_neg;
    const unsigned P = M - n_neg;
    if (n == 0u || P == 0u) {
        if (tid == 0) out[blockIdx.x] = 0;
        return;
    }
    unsigned* A = (unsigned*)(ZT + (size_t)blockIdx.x * M);
    unsigned* B = (unsigned*)(scratch + (size_t)blockIdx.x * n);

#pragma unroll
    for (int v = 0; v < 8; ++v) wcnt[v * 256 + tid] = 0;
    auc_sort_keys(A, B, n, hist, wcnt, tid);

    // A[0..n): the negatives' keys, ascending; A[n..M): the positives' z
    const unsigned* keys = A;
    const unsigned* zp = A + n;
    unsigned long long acc = 0ull;
    for (unsigned j0 = 0; j0 < P; j0 += AUC_TILE * AUC_ILP) {
        unsigned kp[AUC_ILP], lo[AUC_ILP], hi[AUC_ILP];
        bool ok[AUC_ILP];
#pragma unroll
        for (int u = 0; u < AUC_ILP; ++u) {
            const unsigned j = j0 + u * AUC_TILE + tid;
            ok[u] = j < P;
            kp[u] = ok[u] ? auc_key(zp[j]) : 0u;
            lo[u] = hi[u] = 0u;
        }
        // lo: first key >= kp, hi: first key > kp; the answer stays in
        // [lo, lo + len], so lo + half - 1 < n
        unsigned len = n;
        while (len > 1u) {
            const unsigned half = len >> 1;
#pragma unroll
            for (int u = 0; u < AUC_ILP; ++u) {
                const unsigned a = keys[lo[u] + half - 1u];
                const unsigned b = keys[hi[u] + half - 1u];
                lo[u] += a < kp[u] ? half : 0u;
                hi[u] += b <= kp[u] ? half : 0u;
            }
            len -= half;
        }
#pragma unroll
        for (int u = 0; u < AUC_ILP; ++u) {
            lo[u] += keys[lo[u]] < kp[u] ? 1u : 0u;
            hi[u] += keys[hi[u]] <= kp[u] ? 1u : 0u;
            if (ok[u]) acc += (unsigned long long)lo[u] + hi[u];
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = (long long)red[0];
}

// Average precision of one fold, per model:
//   S[c] = sum over positives i of TP(i) / (TP(i) + FP(i)),  AP = S / P
//   TP(i) = #positives with z >= z_i, FP(i) = #negatives with z >= z_i
// (sklearn's step-wise average_precision_score: thresholds at the distinct
// values, ties grouped).  ZT [nm][M] as above, scratch [nm][M], out [nm]
// fp64.  Both halves of the row are sorted with auc_sort_keys, each
// between its own part of ZT and the same part of scratch, so all of ZT is
// consumed.  A lane then takes SORTED positives strided by 256, AUC_ILP at
// a time (neighbouring lanes hold neighbouring keys, so their probes land
// close together), and runs one lower-bound search over the negatives' keys
// and one over the positives' keys in a single loop: a segment's half
// length is 0 once its search is down to one candidate, and no probe is
// issued for it, so every probe index stays inside its own segment:
//   TP = P - lower_bound_pos(k),  FP = n - lower_bound_neg(k)
// The ratio is one correctly rounded fp64 division of exact integers; a
// lane adds its ratios in ascending index, the lanes combine in the fixed
// LDS tree and lane 0 stores, so S does not depend on the launch order.
// P == 0 stores 0.0 and touches no memory; n == 0 sorts the positives
// alone and gives S = P exactly.
//
// 30 VGPRs, 0 AGPRs, no scratch, 14336 B of LDS (gfx950, -O3): 8 waves per
// SIMD by registers, 8 workgroups per CU
extern "C" __global__ __launch_bounds__(256)
void k_ap_sums(
    float* ZT,            // [nm][M], negatives first; consumed
    int* scratch,         // [nm][M]
    double* out,          // [nm] S
    unsigned M, unsigned n_neg)
{
    __shared__ int hist[4 * 256];            // digit counts, then offsets
    __shared__ int wcnt[2 * AUC_WCNT];       // [buf][wave][digit]
    __shared__ double red[256];

    const int tid = threadIdx.x;
    const unsigned n = n_neg;
    const unsigned P = M - n_neg;
    if (P == 0u) {
        if (tid == 0) out[blockIdx.x] = 0.0;
        return;
    }
    unsigned* A = (unsigned*)(ZT + (size_t)blockIdx.x * M);
    unsigned* B = (unsigned*)(scratch + (size_t)blockIdx.x * M);

#pragma unroll
    for (int v = 0; v < 8; ++v) wcnt[v * 256 + tid] = 0;
    auc_sort_keys(A, B, n, hist, wcnt, tid);
    auc_sort_keys(A + n, B + n, P, hist, wcnt, tid);

    // ascending keys: the negatives' in A[0..n), the positives' in A[n..M)
    const unsigned* nk = A;
    const unsigned* pk = A + n;
    double acc = 0.0;
    for (unsigned j0 = 0; j0 < P; j0 += AUC_TILE * AUC_ILP) {
        unsigned kp[AUC_ILP], ln[AUC_ILP], lp[AUC_ILP];
        bool ok[AUC_ILP];
#pragma unroll
        for (int u = 0; u < AUC_ILP; ++u) {
            const unsigned j = j0 + u * AUC_TILE + tid;
            ok[u] = j < P;
            kp[u] = ok[u] ? pk[j] : 0u;
            ln[u] = lp[u] = 0u;
        }
        // ln / lp: first negative / positive key >= kp.  An answer stays in
        // [l, l + len] with l + len <= the segment's length, so
        // l + half - 1 is inside the segment whenever half >= 1
        unsigned lenn = n, lenp = P;
        while (lenn > 1u || lenp > 1u) {
            const unsigned hn = lenn >> 1, hp = lenp >> 1;
#pragma unroll
            for (int u = 0; u < AUC_ILP; ++u) {
                if (hn) ln[u] += nk[ln[u] + hn - 1u] < kp[u] ? hn : 0u;
                if (hp) lp[u] += pk[lp[u] + hp - 1u] < kp[u] ? hp : 0u;
            }
            lenn -= hn;
            lenp -= hp;
        }
#pragma unroll
        for (int u = 0; u < AUC_ILP; ++u) {
            // ln <= n - 1 when n >= 1, lp <= P - 1
            if (n) ln[u] += nk[ln[u]] < kp[u] ? 1u : 0u;
            lp[u] += pk[lp[u]] < kp[u] ? 1u : 0u;
            const unsigned tp = P - lp[u];
            const unsigned fp = n - ln[u];
            if (ok[u]) acc += (double)tp / (double)(tp + fp);
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0];
}

extern "C" hipError_t skdist_auc_counts(
    void* ZT, void* scratch, void* out, long long nm, long long M,
    long long n_neg, hipStream_t stream)
{
    if (nm < 0 || nm > 0x7fffffffLL || M < 0 || M > 0x7fffffffLL ||
        n_neg < 0 || n_neg > M)
        return hipErrorInvalidValue;
    if (nm == 0 || M == 0) return hipSuccess;
    hipLaunchKernelGGL(k_auc_counts, dim3((unsigned)nm), dim3(256), 0, stream,
                       (float*)ZT, (int*)scratch, (long long*)out,
                       (unsigned)M, (unsigned)n_neg);
    return hipGetLastError();
}

extern "C" hipError_t skdist_ap_sums(
    void* ZT, void* scratch, void* out, long long nm, long long M,
    long long n_neg, hipStream_t stream)
{
    if (nm < 0 || nm > 0x7fffffffLL || M < 0 || M > 0x7fffffffLL ||
        n_neg < 0 || n_neg > M)
        return hipErrorInvalidValue;
    if (nm == 0 || M == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ap_sums, dim3((unsigned)nm), dim3(256), 0, stream,
                       (float*)ZT, (int*)scratch, (double*)out,
                       (unsigned)M, (unsigned)n_neg);
    return hipGetLastError();
}
