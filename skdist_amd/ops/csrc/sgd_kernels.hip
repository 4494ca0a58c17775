// Batched mini-batch-SGD linear solver — CDNA4 (gfx950) kernels.
//
// One SGD step over a minibatch of m rows trains ncols independent linear
// models (columns) at once (math + torch reference: skdist_amd/models/_sgd.py;
// reference inventory: SURVEY.md §2.4 row 1).
//
//   K1 k_fwd_gt:        GT[c][i] = mask*dloss( (Xs·W)[i][c], target )
//      k_fwd_gt_softmax (multinomial): GT = mask*(softmax over a group - t)
//   K2 k_grad_partial:  partial[z] = Xᵀ·G  (split-K, deterministic slabs)
//   K3 k_reduce_update: W -= lr * (Σz partial / m + λ∘W); refresh WbfT
//
// GEMM structure (K1, K5 and K2's legacy tiles; K2's whole-fa kernel has
// its own comment block): 128×128 tile, 4 waves (2×2 of 64×64), MFMA bf16
// 16x16x32, BK=32, double-buffered LDS staged by global_load_lds_dwordx4
// (wave-uniform LDS chunk base + lane×16B, per-lane swizzled SOURCE
// address).  LDS image is lane-linear [128][32] bf16; the 16B slot of each
// row is XOR-swizzled by ((row>>2)&3) so ds_read_b128 fragment loads are
// bank-conflict-free (guide §5.4 rule 21 / T2).
//
// Layouts (row-major, K-contiguous):
//   Xs    [n_pad][fa]        bf16  epoch-shuffled, rows n..n_pad zero
//   XsT   [fa_store][n_pad]  bf16  transpose (fa_store = ceil(fa/128)*128;
//                                rows fa..fa_store zero)
//   WbfT  [ncols_pad][fa]    bf16
//   W, V  [fa][ncols_pad]    f32
//   GT    [ncols_pad][gts]   bf16
//   partial [SPLITK][fa][ncols_pad] f32
#include "common.h"

#include <atomic>

#define BM 128
#define BN 128
#define BK 32
#define LDC 132  // LDS row stride for the epilogue transpose tile
// double-buffered LDS tiles carved from the extern-shared base `sm`
// (one __shared__ object only — guide §5 'Three .s-level traps' (a))

// stage one 128x32 bf16 tile (8 KiB) into linear LDS via 8 glds chunks;
// each of the 4 waves issues 2. src_row(row) must return the global
// pointer to the row's k-offset base (element units).
#define STAGE_TILE(ldsbase, SRC_EXPR)                                       \
    do {                                                                    \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                     \
            const int c = w + 4 * i;                                        \
            const int row = 16 * c + (lane >> 2);                           \
            const int slot = (lane & 3) ^ ((row >> 2) & 3);                 \
            const __bf16* _src = (SRC_EXPR) + slot * 8;                     \
            __builtin_amdgcn_global_load_lds(                               \
                (const unsigned int*)_src,                                  \
                (unsigned int*)((ldsbase) + c * 512), 16, 0, 0);            \
        }                                                                   \
    } while (0)

// swizzled ds_read_b128 of one 8-elem fragment at (row, k-slot fk/8)
static __device__ __forceinline__ bf16x8
frag_load(const __bf16* lds, int row, int fk) {
    const int phys = (fk >> 3) ^ ((row >> 2) & 3);
    return *(const bf16x8*)(lds + row * BK + phys * 8);
}

// ---------------------------------------------------------------------- //
// K1: fused forward GEMM + loss gradient + transposed store
// grid: (m_pad/BM, ncols_pad/BN), block 256
//
// The epilogue (64 accumulators per lane -> masked dloss -> bf16) costs
// more issue slots than the GEMM loop, so it is instantiated per loss and
// per path and the kernel branches once, workgroup-uniformly:
//   PLAIN   every column of the tile has col_class < 0 and col_class2 < 0
//           (pad columns included) and there is no row_w: t = y, g is not
//           scaled, and an element trains when its row may train and the
//           row's fold differs from the column's.
//   general class targets, one-vs-one pairs, row_w.
// Both paths run the same arithmetic on an element both can express
// (dropping a multiply by 1.0f is exact), so GT does not depend on which
// path a tile took.  ok_s holds, per row, whether bm + row < m.
//
// __launch_bounds__(256, 4): 4 waves per SIMD, i.e. 4 workgroups per CU.
// Within 128 registers the accumulators stay in VGPRs (121 VGPRs, no
// AGPRs, no scratch); unbounded, the kernel took 121 + 64 and ran 2.
// ---------------------------------------------------------------------- //
template <int LOSS, bool PLAIN>
static __device__ __forceinline__ void fwd_epilogue(
    const f32x4 (&acc)[4][4], __bf16* ldsC, const float* y_s,
    const int* fold_s, const int* ok_s, const float* rw_s,
    const int* cls_s, const int* cfold_s, const int* cls2_s,
    int wr, int wc, int fr, int rw)
{
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int rowb = wr + mi * 16 + rw * 4;
        const f32x4 y4 = *(const f32x4*)&y_s[rowb];
        const int4v fo4 = *(const int4v*)&fold_s[rowb];
        const int4v ok4 = *(const int4v*)&ok_s[rowb];
        f32x4 rw4 = {1.f, 1.f, 1.f, 1.f};
        if (!PLAIN) rw4 = *(const f32x4*)&rw_s[rowb];
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int colb = wc + ni * 16 + fr;
            const int cfo = cfold_s[colb];
            const int cls = PLAIN ? -1 : cls_s[colb];
            const int c2 = PLAIN ? -1 : cls2_s[colb];
            short4v g4;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = acc[mi][ni][r];
                const float yv = y4[r];
                bool train = (fo4[r] != cfo) && (ok4[r] != 0);
                float g;
                if (PLAIN) {
                    g = dloss(LOSS, z, yv);
                } else {
                    const float t =
                        (cls < 0) ? yv : (yv == (float)cls ? 1.f : 0.f);
                    g = dloss(LOSS, z, t) * rw4[r];
                    if (c2 >= 0)  // one-vs-one: only the pair's rows train
                        train = train &&
                                (yv == (float)cls || yv == (float)c2);
                }
                g4[r] = __builtin_bit_cast(short,
                                           f32_to_bf16(train ? g : 0.f));
            }
            *(short4v*)&ldsC[colb * LDC + rowb] = g4;
        }
    }
}

extern "C" __global__ __launch_bounds__(256, 4) void k_fwd_gt(
    const __bf16* __restrict__ Xs,    // [n_pad][fa]
    const __bf16* __restrict__ WbfT,  // [ncols_pad][fa]
    __bf16* __restrict__ GT,          // [ncols_pad][gt_stride]
    const float* __restrict__ y,      // [n]
    const int* __restrict__ fold,     // [n]
    const int* __restrict__ col_class,
    const int* __restrict__ col_fold,
    const int* __restrict__ col_class2,  // >=0: one-vs-one partner class
    const float* __restrict__ row_w,     // per-row sample weights or null
    int start, int m, long long n, int fa, int ncols_pad, int gt_stride,
    int loss_id)
{
    extern __shared__ __attribute__((aligned(16))) char sm[];
    #define bufA(b) ((__bf16*)(sm + (b) * 16384))
    #define bufB(b) ((__bf16*)(sm + 8192 + (b) * 16384))
    __bf16* ldsC = (__bf16*)sm;             // [BN][LDC], aliases the bufs
    char* meta = sm + BN * LDC * 2;
    float* y_s = (float*)meta;              // [BM]
    int* fold_s = (int*)(meta + 512);       // [BM]
    int* cls_s = (int*)(meta + 1024);       // [BN]
    int* cfold_s = (int*)(meta + 1536);     // [BN]
    int* cls2_s = (int*)(meta + 2048);      // [BN]
    float* rw_s = (float*)(meta + 2560);    // [BM]
    int* ok_s = (int*)(meta + 3072);        // [BM] row may train (< m)
    int* gen_s = (int*)(meta + 3584);       // [2] a wave saw a class column

    const int tid = threadIdx.x;
    const int bm = blockIdx.x * BM;
    const int bn = blockIdx.y * BN;
    const int lane = tid & 63;
    const int w = tid >> 6;

    if (tid < BM) {
        const long long r = (long long)start + bm + tid;
        const bool ok = r < n;
        y_s[tid] = ok ? y[r] : 0.f;
        fold_s[tid] = ok ? fold[r] : -9;
        rw_s[tid] = (row_w != nullptr && ok) ? row_w[r] : 1.f;
        ok_s[tid] = (bm + tid < m) ? 1 : 0;
    } else {
        const int c = tid - BM;
        const int cl = col_class[bn + c];
        const int c2 = col_class2[bn + c];
        cls_s[c] = cl;
        cfold_s[c] = col_fold[bn + c];
        cls2_s[c] = c2;
        const bool general = __ballot(cl >= 0 || c2 >= 0) != 0ull;
        if (lane == 0) gen_s[w - 2] = general ? 1 : 0;
    }

    const __bf16* Abase = Xs + (long long)(start + bm) * fa;
    const __bf16* Bbase = WbfT + (long long)bn * fa;

    const int wr = ((w >> 1) & 1) * 64;
    const int wc = (w & 1) * 64;
    const int fr = lane & 15;
    const int fk = (lane >> 4) * 8;

    f32x4 acc[4][4] = {};
    const int nk = fa / BK;
    int cur = 0;
    STAGE_TILE(bufA(0), Abase + (long long)row * fa);
    STAGE_TILE(bufB(0), Bbase + (long long)row * fa);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // staged tile (glds) complete for buf[cur]
        if (kt + 1 < nk) {
            STAGE_TILE(bufA(cur ^ 1),
                       Abase + (long long)row * fa + (kt + 1) * BK);
            STAGE_TILE(bufB(cur ^ 1),
                       Bbase + (long long)row * fa + (kt + 1) * BK);
        }
        bf16x8 af[4], bfr[4];
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            af[mi] = frag_load(bufA(cur), wr + mi * 16 + fr, fk);
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
            bfr[ni] = frag_load(bufB(cur), wc + ni * 16 + fr, fk);
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] =
                    MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        cur ^= 1;
    }

    // epilogue: z -> masked dloss -> bf16, transposed through LDS.  The
    // barrier also orders the prologue's metadata writes (nk >= 1 put
    // another one in between) before the reads below.
    __syncthreads();
    const int rw = lane >> 4;
    const bool plain = __builtin_amdgcn_readfirstlane(
        (gen_s[0] | gen_s[1]) == 0 && row_w == nullptr);
    #define FWD_EPILOGUE(L)                                                 \
        do {                                                                \
            if (plain)                                                      \
                fwd_epilogue<L, true>(acc, ldsC, y_s, fold_s, ok_s, rw_s,   \
                                      cls_s, cfold_s, cls2_s, wr, wc, fr,   \
                                      rw);                                  \
            else                                                            \
                fwd_epilogue<L, false>(acc, ldsC, y_s, fold_s, ok_s, rw_s,  \
                                       cls_s, cfold_s, cls2_s, wr, wc, fr,  \
                                       rw);                                 \
        } while (0)
    switch (loss_id) {
    case LOSS_LOG: FWD_EPILOGUE(LOSS_LOG); break;
    case LOSS_HINGE: FWD_EPILOGUE(LOSS_HINGE); break;
    default: FWD_EPILOGUE(LOSS_SQUARED); break;
    }
    #undef FWD_EPILOGUE
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tid + 256 * i;
        const int col = p >> 3;
        const int ch = (p & 7) * 16;
        int4v v0 = *(int4v*)&ldsC[col * LDC + ch];
        int4v v1 = *(int4v*)&ldsC[col * LDC + ch + 8];
        __bf16* dst = GT + (long long)(bn + col) * gt_stride + bm + ch;
        *(int4v*)dst = v0;
        *(int4v*)(dst + 8) = v1;
    }
}

// ---------------------------------------------------------------------- //
// K1, per-element targets: forward GEMM + loss gradient, with the target
// and the train mask of every (row, column) read from bit planes
// grid: (m_pad/BM, ncols_pad/BN), block 256 -- k_fwd_gt's grid, GEMM main
// loop, GT layout, transposed store and per-loss epilogue instantiation.
//
//   Tbits [n_pad][ncols_pad/32] int32: bit (c & 31) of word [r][c >> 5] is
//         the target of kernel column c on shuffled row r
//   Mbits same shape: the element trains only where the bit is set; a null
//         pointer means all ones, costs no loads and selects, workgroup-
//         uniformly, an epilogue without the mask test
// Rows >= n and pad columns hold 0 in both planes (rows >= n are not even
// read).  col_class / col_class2 do not exist here: the target is the bit,
// and there is no one-vs-one test.  fold / col_fold / row_w / m keep
// k_fwd_gt's meaning, and on a given element the arithmetic is that of
// k_fwd_gt's general path: g = dloss(z, t) * row_w, stored as 0 where the
// element does not train.
//
// A 128-column tile needs words bn/32 .. bn/32+3 of each of its 128 rows:
// one aligned 16-byte load per row and plane (ncols_pad and bn are multiples
// of 128), staged in the prologue word-major ([4][BM]) so that the epilogue
// fetches one word of 4 consecutive rows with one ds_read_b128.  The 64
// columns of a wave span two words; the bit of column colb is bit
// (colb & 31) of word colb >> 5.
//
// LDS: BN*LDC*2 = 33792 (the transpose tile, aliasing the GEMM buffers)
// + 4 * 512 (fold_s, cfold_s, rw_s, ok_s) + 2 * 2048 (the plane slabs)
// = 39936 B <= 40960, so 4 workgroups per CU fit in 160 KiB as for k_fwd_gt
// (y_s, cls_s, cls2_s and gen_s are gone).
// __launch_bounds__(256, 4): 128 VGPRs, no AGPRs, no scratch (k_fwd_gt: 121).
// ---------------------------------------------------------------------- //
#define BITS_LDS (BN * LDC * 2 + 4 * 512 + 2 * 2048)

template <int LOSS, bool HASM>
static __device__ __forceinline__ void fwd_epilogue_bits(
    const f32x4 (&acc)[4][4], __bf16* ldsC, const int* fold_s,
    const int* ok_s, const float* rw_s, const int* cfold_s,
    const int* tb_s, const int* mb_s, int wr, int wc, int fr, int rw)
{
    const int wq = wc >> 5;  // first of the two plane words of this wave
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int rowb = wr + mi * 16 + rw * 4;
        const int4v fo4 = *(const int4v*)&fold_s[rowb];
        const int4v ok4 = *(const int4v*)&ok_s[rowb];
        const f32x4 rw4 = *(const f32x4*)&rw_s[rowb];
        int4v tw[2], mw[2];
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            tw[h] = *(const int4v*)&tb_s[(wq + h) * BM + rowb];
            if (HASM) mw[h] = *(const int4v*)&mb_s[(wq + h) * BM + rowb];
        }
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int colb = wc + ni * 16 + fr;
            const int cfo = cfold_s[colb];
            const int sh = (ni & 1) * 16 + fr;  // colb & 31
            short4v g4;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = acc[mi][ni][r];
                bool train = (fo4[r] != cfo) && (ok4[r] != 0);
                if (HASM)
                    train = train &&
                            (((unsigned)mw[ni >> 1][r] >> sh) & 1u) != 0u;
                const float t =
                    (((unsigned)tw[ni >> 1][r] >> sh) & 1u) ? 1.f : 0.f;
                const float g = dloss(LOSS, z, t) * rw4[r];
                g4[r] = __builtin_bit_cast(short,
                                           f32_to_bf16(train ? g : 0.f));
            }
            *(short4v*)&ldsC[colb * LDC + rowb] = g4;
        }
    }
}

extern "C" __global__ __launch_bounds__(256, 4) void k_fwd_gt_bits(
    const __bf16* __restrict__ Xs,    // [n_pad][fa]
    const __bf16* __restrict__ WbfT,  // [ncols_pad][fa]
    __bf16* __restrict__ GT,          // [ncols_pad][gt_stride]
    const int* __restrict__ fold,     // [n]
    const int* __restrict__ col_fold,
    const float* __restrict__ row_w,  // per-row sample weights or null
    const int* __restrict__ Tbits,    // [n_pad][ncols_pad/32]
    const int* __restrict__ Mbits,    // same, or null: every element trains
    int start, int m, long long n, int fa, int ncols_pad, int gt_stride,
    int loss_id)
{
    extern __shared__ __attribute__((aligned(16))) char sm[];
    __bf16* ldsC = (__bf16*)sm;             // [BN][LDC], aliases the bufs
    char* meta = sm + BN * LDC * 2;
    int* fold_s = (int*)meta;               // [BM]
    int* cfold_s = (int*)(meta + 512);      // [BN]
    float* rw_s = (float*)(meta + 1024);    // [BM]
    int* ok_s = (int*)(meta + 1536);        // [BM] row may train (< m)
    int* tb_s = (int*)(meta + 2048);        // [4][BM] target words
    int* mb_s = (int*)(meta + 4096);        // [4][BM] mask words

    const int tid = threadIdx.x;
    const int bm = blockIdx.x * BM;
    const int bn = blockIdx.y * BN;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int wpr = ncols_pad >> 5;         // plane words per row

    if (tid < BM) {
        const long long r = (long long)start + bm + tid;
        const bool ok = r < n;
        fold_s[tid] = ok ? fold[r] : -9;
        rw_s[tid] = (row_w != nullptr && ok) ? row_w[r] : 1.f;
        ok_s[tid] = (bm + tid < m) ? 1 : 0;
        int4v tv = {0, 0, 0, 0};
        if (ok) tv = *(const int4v*)(Tbits + r * wpr + (bn >> 5));
        #pragma unroll
        for (int k = 0; k < 4; ++k) tb_s[k * BM + tid] = tv[k];
    } else {
        const int c = tid - BM;
        cfold_s[c] = col_fold[bn + c];
        if (Mbits != nullptr) {             // workgroup-uniform
            const long long r = (long long)start + bm + c;
            int4v mv = {0, 0, 0, 0};
            if (r < n) mv = *(const int4v*)(Mbits + r * wpr + (bn >> 5));
            #pragma unroll
            for (int k = 0; k < 4; ++k) mb_s[k * BM + c] = mv[k];
        }
    }

    const __bf16* Abase = Xs + (long long)(start + bm) * fa;
    const __bf16* Bbase = WbfT + (long long)bn * fa;

    const int wr = ((w >> 1) & 1) * 64;
    const int wc = (w & 1) * 64;
    const int fr = lane & 15;
    const int fk = (lane >> 4) * 8;

    // the GEMM main loop of k_fwd_gt
    f32x4 acc[4][4] = {};
    const int nk = fa / BK;
    int cur = 0;
    STAGE_TILE(bufA(0), Abase + (long long)row * fa);
    STAGE_TILE(bufB(0), Bbase + (long long)row * fa);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // staged tile (glds) complete for buf[cur]
        if (kt + 1 < nk) {
            STAGE_TILE(bufA(cur ^ 1),
                       Abase + (long long)row * fa + (kt + 1) * BK);
            STAGE_TILE(bufB(cur ^ 1),
                       Bbase + (long long)row * fa + (kt + 1) * BK);
        }
        bf16x8 af[4], bfr[4];
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            af[mi] = frag_load(bufA(cur), wr + mi * 16 + fr, fk);
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
            bfr[ni] = frag_load(bufB(cur), wc + ni * 16 + fr, fk);
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] =
                    MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        cur ^= 1;
    }

    // epilogue, as k_fwd_gt: the barrier ends the reads of the GEMM buffers
    // and orders the prologue's metadata writes before the reads below
    __syncthreads();
    const int rw = lane >> 4;
    #define FWD_EPILOGUE_BITS(L)                                            \
        do {                                                                \
            if (Mbits != nullptr)                                           \
                fwd_epilogue_bits<L, true>(acc, ldsC, fold_s, ok_s, rw_s,   \
                                           cfold_s, tb_s, mb_s, wr, wc, fr, \
                                           rw);                             \
            else                                                            \
                fwd_epilogue_bits<L, false>(acc, ldsC, fold_s, ok_s, rw_s,  \
                                            cfold_s, tb_s, mb_s, wr, wc,    \
                                            fr, rw);                        \
        } while (0)
    switch (loss_id) {
    case LOSS_LOG: FWD_EPILOGUE_BITS(LOSS_LOG); break;
    case LOSS_HINGE: FWD_EPILOGUE_BITS(LOSS_HINGE); break;
    default: FWD_EPILOGUE_BITS(LOSS_SQUARED); break;
    }
    #undef FWD_EPILOGUE_BITS
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tid + 256 * i;
        const int col = p >> 3;
        const int ch = (p & 7) * 16;
        int4v v0 = *(int4v*)&ldsC[col * LDC + ch];
        int4v v1 = *(int4v*)&ldsC[col * LDC + ch + 8];
        __bf16* dst = GT + (long long)(bn + col) * gt_stride + bm + ch;
        *(int4v*)dst = v0;
        *(int4v*)(dst + 8) = v1;
    }
}

// ---------------------------------------------------------------------- //
// K1, multinomial: forward GEMM + softmax cross-entropy gradient
// grid: (m_pad/BM, ncols_pad/BN), block 256 -- k_fwd_gt's grid, GEMM tile,
// GT layout and transposed store; `gk` stands where k_fwd_gt has loss_id.
//
// The gk columns of one model form a group.  A group never straddles a
// 128-column tile: a tile holds gpt = 128 / gk groups in its first
// gpt * gk columns (model j, class c at column
// (j / gpt) * 128 + (j % gpt) * gk + c; ops.hip_sgd_solve lays the columns
// out), the rest of the tile is dead.  Per row i and live group:
//     p_c = exp(z_c - max_c z) / sum_c exp(z_c - max_c z)
//     g_c = (p_c - [y_i == col_class[c]]) * row_w[i]
// and g = 0 where the element does not train: row >= m, row >= n, or the
// row's fold is the group's fold (col_fold of the group's first column).
// A group whose first column has col_class < 0 (pad columns) is dead too;
// dead columns enter no max or sum and store 0.
//
// First-cut epilogue: z goes through LDS as fp32, 64 rows at a time (the
// [64][129] fp32 image aliases the GEMM buffers), and one lane owns one
// (row, group): it walks the group's gk columns three times (max; exp and
// sum, leaving e in place; divide, subtract, scale), in ascending column
// order, so the result is deterministic and there are no atomics.  Lanes
// of a wave hold consecutive rows, stride 129 words: conflict-free.  A
// wave takes groups w, w + 4, ...: with gk > 32 some waves idle, and a
// 128-wide group is one wave's work.  The tile is then read back
// column-wise, rounded to bf16 and stored as k_fwd_gt stores it.
//
// __launch_bounds__(256, 4): 115 VGPRs, no AGPRs, no scratch, 36096 B of
// LDS: 4 workgroups per CU (4 waves per SIMD), as k_fwd_gt.
// ---------------------------------------------------------------------- //
#define SMX_ZLD 129                    // fp32 row stride of the z image
#define SMX_ZBYTES (64 * SMX_ZLD * 4)  // 33024, covers the 32 KiB of bufs
#define SMX_LDS (SMX_ZBYTES + 6 * 512)

extern "C" __global__ __launch_bounds__(256, 4) void k_fwd_gt_softmax(
    const __bf16* __restrict__ Xs,    // [n_pad][fa]
    const __bf16* __restrict__ WbfT,  // [ncols_pad][fa]
    __bf16* __restrict__ GT,          // [ncols_pad][gt_stride]
    const float* __restrict__ y,      // [n]
    const int* __restrict__ fold,     // [n]
    const int* __restrict__ col_class,
    const int* __restrict__ col_fold,
    const int* __restrict__ col_class2,  // unused: groups have no partner
    const float* __restrict__ row_w,     // per-row sample weights or null
    int start, int m, long long n, int fa, int ncols_pad, int gt_stride,
    int gk)
{
    extern __shared__ __attribute__((aligned(16))) char sm[];
    float* zS = (float*)sm;                 // [64][SMX_ZLD], aliases the bufs
    char* meta = sm + SMX_ZBYTES;
    float* y_s = (float*)meta;              // [BM]
    int* fold_s = (int*)(meta + 512);       // [BM]
    int* cls_s = (int*)(meta + 1024);       // [BN]
    int* cfold_s = (int*)(meta + 1536);     // [BN]
    float* rw_s = (float*)(meta + 2048);    // [BM]
    int* ok_s = (int*)(meta + 2560);        // [BM] row may train

    const int tid = threadIdx.x;
    const int bm = blockIdx.x * BM;
    const int bn = blockIdx.y * BN;
    const int lane = tid & 63;
    const int w = tid >> 6;

    if (tid < BM) {
        const long long r = (long long)start + bm + tid;
        const bool ok = r < n;
        y_s[tid] = ok ? y[r] : 0.f;
        fold_s[tid] = ok ? fold[r] : -9;
        rw_s[tid] = (row_w != nullptr && ok) ? row_w[r] : 1.f;
        ok_s[tid] = (ok && bm + tid < m) ? 1 : 0;
    } else {
        const int c = tid - BM;
        cls_s[c] = col_class[bn + c];
        cfold_s[c] = col_fold[bn + c];
    }

    const __bf16* Abase = Xs + (long long)(start + bm) * fa;
    const __bf16* Bbase = WbfT + (long long)bn * fa;

    const int wr = ((w >> 1) & 1) * 64;
    const int wc = (w & 1) * 64;
    const int fr = lane & 15;
    const int fk = (lane >> 4) * 8;

    // the GEMM main loop of k_fwd_gt
    f32x4 acc[4][4] = {};
    const int nk = fa / BK;
    int cur = 0;
    STAGE_TILE(bufA(0), Abase + (long long)row * fa);
    STAGE_TILE(bufB(0), Bbase + (long long)row * fa);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // staged tile (glds) complete for buf[cur]
        if (kt + 1 < nk) {
            STAGE_TILE(bufA(cur ^ 1),
                       Abase + (long long)row * fa + (kt + 1) * BK);
            STAGE_TILE(bufB(cur ^ 1),
                       Bbase + (long long)row * fa + (kt + 1) * BK);
        }
        bf16x8 af[4], bfr[4];
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            af[mi] = frag_load(bufA(cur), wr + mi * 16 + fr, fk);
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
            bfr[ni] = frag_load(bufB(cur), wc + ni * 16 + fr, fk);
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] =
                    MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        cur ^= 1;
    }

    // every wave is done reading the GEMM buffers, and the prologue's
    // metadata is visible
    __syncthreads();
    const int rw = lane >> 4;
    const int gpt = BN / gk;
    const int ncl = gpt * gk;   // live columns of the tile
    for (int h = 0; h < 2; ++h) {
        if (wr == h * 64) {     // the two waves holding rows 64h .. 64h+63
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    #pragma unroll
                    for (int r = 0; r < 4; ++r)
                        zS[(mi * 16 + rw * 4 + r) * SMX_ZLD + wc + ni * 16 +
                           fr] = acc[mi][ni][r];
        }
        __syncthreads();
        {
            const int R = h * 64 + lane;  // this lane's row of the tile
            const float yv = y_s[R];
            const float rwv = rw_s[R];
            const int fo = fold_s[R];
            const bool rok = ok_s[R] != 0;
            float* zrow = zS + lane * SMX_ZLD;
            for (int g = w; g < gpt; g += 4) {
                float* zr = zrow + g * gk;
                const int* cl = cls_s + g * gk;
                const bool train =
                    rok && cl[0] >= 0 && fo != cfold_s[g * gk];
                if (!train) {
                    for (int c = 0; c < gk; ++c) zr[c] = 0.f;
                    continue;
                }
                float mx = zr[0];
                for (int c = 1; c < gk; ++c) mx = fmaxf(mx, zr[c]);
                float s = 0.f;
                for (int c = 0; c < gk; ++c) {
                    const float e = __expf(zr[c] - mx);
                    zr[c] = e;
                    s += e;
                }
                for (int c = 0; c < gk; ++c) {
                    const float t = (yv == (float)cl[c]) ? 1.f : 0.f;
                    zr[c] = (zr[c] / s - t) * rwv;
                }
            }
            for (int c = ncl + w; c < BN; c += 4) zrow[c] = 0.f;
        }
        __syncthreads();
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i;
            const int col = p >> 2;
            const int ch = (p & 3) * 16;
            int4v v[2];
            #pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned lo = (unsigned short)__builtin_bit_cast(
                    short, f32_to_bf16(zS[(ch + 2 * k) * SMX_ZLD + col]));
                const unsigned hi = (unsigned short)__builtin_bit_cast(
                    short, f32_to_bf16(zS[(ch + 2 * k + 1) * SMX_ZLD + col]));
                v[k >> 2][k & 3] = (int)(lo | (hi << 16));
            }
            __bf16* dst =
                GT + (long long)(bn + col) * gt_stride + bm + h * 64 + ch;
            *(int4v*)dst = v[0];
            *(int4v*)(dst + 8) = v[1];
        }
        if (h == 0) __syncthreads();  // zS is rewritten for rows 64..127
    }
}

// ---------------------------------------------------------------------- //
// K2: Grad partial slabs, split-K over minibatch rows
//
// partial[z][r][c] = sum over the slab's k of XsT[r][start + k] * GT[c][k],
// slab z = [z * k_chunk, min(m_pad, (z + 1) * k_chunk)), accumulated by one
// MFMA 16x16x32 per 32-deep k-step in ascending k.  Every kernel below
// computes an element by that same chain, so which one ran cannot be told
// from the result.
//
// fa <= K2F_MAX_FA (288): k_grad_partial_fullm, the whole-fa tile.
//   grid (SPLITK, ncols_pad / K2F_BN), block 512.  One workgroup owns all
//   fa feature rows of one column tile and one slab, so GT is fetched once
//   per step.  The slab is the fast grid dimension: consecutive workgroups
//   go to different XCDs, so with SPLITK = 8 an XCD sees one slab of XsT
//   (fa x 1024 bf16, L2-resident) and its 24 column tiles.  8 waves as
//   2 (rows) x 4 (columns); the 16-row fragments of the tile are dealt to
//   the two wave rows alternately (fragment 2*mi + r), so both halves
//   carry fa/32 fragments whatever fa is, and the kernel is instantiated
//   per fa/32.  Both operands are staged by global_load_lds into a ring of
//   K2F_NS stages of BK = 32; the loads of K2F_NS - 2 stages stay in flight
//   across each raw s_barrier and are retired by a counted s_waitcnt vmcnt
//   (see grad_partial_fullm_body).
//
// fa > K2F_MAX_FA: the legacy tiles, grid (ceil(fa/rows), ncols_pad/BN,
//   SPLITK), block 256.  The tile is rows x 128 with rows = 32 * MI: 2x2
//   waves, each holding MI fragments of 16 feature rows by 4 of 16 columns.
//   MI = 4 is the 128-row tile; MI = 3 is a 96-row tile for fa that 96
//   covers with fewer padded rows.  Double-buffered LDS, __syncthreads()
//   per k-step.
// ---------------------------------------------------------------------- //
template <int MI>
static __device__ __forceinline__ void grad_partial_body(
    const __bf16* __restrict__ XsT,  // [fa_store][n_pad]
    const __bf16* __restrict__ GT,   // [ncols_pad][gt_stride]
    float* __restrict__ partial,     // [SPLITK][fa][ncols_pad]
    int start, int m_pad, long long n_pad, int fa, int ncols_pad,
    int gt_stride, int k_chunk)
{
    extern __shared__ __attribute__((aligned(16))) char sm[];

    // stage the (32 * MI) x 32 A tile: 2 * MI chunks of 16 rows, chunk c
    // by wave c & 3 (wave-uniform guard)
    #define STAGE_A(ldsbase, SRC_EXPR)                                      \
        do {                                                                \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) {                 \
                const int c = w + 4 * i;                                    \
                if (c < 2 * MI) {                                           \
                    const int row = 16 * c + (lane >> 2);                   \
                    const int slot = (lane & 3) ^ ((row >> 2) & 3);         \
                    const __bf16* _src = (SRC_EXPR) + slot * 8;             \
                    __builtin_amdgcn_global_load_lds(                       \
                        (const unsigned int*)_src,                          \
                        (unsigned int*)((ldsbase) + c * 512), 16, 0, 0);    \
                }                                                           \
            }                                                               \
        } while (0)

    const int tid = threadIdx.x;
    const int bf = blockIdx.x * (32 * MI);  // feature-row offset
    const int bn = blockIdx.y * BN;         // col offset
    const int z = blockIdx.z;
    const int lane = tid & 63;
    const int w = tid >> 6;

    const __bf16* Abase = XsT + (long long)bf * n_pad + start;
    const __bf16* Bbase = GT + (long long)bn * gt_stride;

    const int k0 = z * k_chunk;
    const int k1 = min(m_pad, k0 + k_chunk);

    const int wr = ((w >> 1) & 1) * (16 * MI);
    const int wc = (w & 1) * 64;
    const int fr = lane & 15;
    const int fk = (lane >> 4) * 8;

    f32x4 acc[MI][4] = {};
    int cur = 0;
    if (k0 < k1) {
        STAGE_A(bufA(0), Abase + (long long)row * n_pad + k0);
        STAGE_TILE(bufB(0), Bbase + (long long)row * gt_stride + k0);
    }
    for (int kt = k0; kt < k1; kt += BK) {
        __syncthreads();
        if (kt + BK < k1) {
            STAGE_A(bufA(cur ^ 1),
                    Abase + (long long)row * n_pad + kt + BK);
            STAGE_TILE(bufB(cur ^ 1),
                       Bbase + (long long)row * gt_stride + kt + BK);
        }
        bf16x8 af[MI], bfr[4];
        #pragma unroll
        for (int mi = 0; mi < MI; ++mi)
            af[mi] = frag_load(bufA(cur), wr + mi * 16 + fr, fk);
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
            bfr[ni] = frag_load(bufB(cur), wc + ni * 16 + fr, fk);
        #pragma unroll
        for (int mi = 0; mi < MI; ++mi)
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] =
                    MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        cur ^= 1;
    }
    #undef STAGE_A

    float* out = partial + (long long)z * fa * ncols_pad;
    const int rw = lane >> 4;
    #pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int rowb = bf + wr + mi * 16 + rw * 4;
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = bn + wc + ni * 16 + fr;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (rowb + r < fa)
                    out[(long long)(rowb + r) * ncols_pad + col] =
                        acc[mi][ni][r];
            }
        }
    }
}

extern "C" __global__ __launch_bounds__(256) void k_grad_partial(
    const __bf16* __restrict__ XsT, const __bf16* __restrict__ GT,
    float* __restrict__ partial,
    int start, int m_pad, long long n_pad, int fa, int ncols_pad,
    int gt_stride, int k_chunk)
{
    grad_partial_body<4>(XsT, GT, partial, start, m_pad, n_pad, fa,
                         ncols_pad, gt_stride, k_chunk);
}

extern "C" __global__ __launch_bounds__(256) void k_grad_partial_96(
    const __bf16* __restrict__ XsT, const __bf16* __restrict__ GT,
    float* __restrict__ partial,
    int start, int m_pad, long long n_pad, int fa, int ncols_pad,
    int gt_stride, int k_chunk)
{
    grad_partial_body<3>(XsT, GT, partial, start, m_pad, n_pad, fa,
                         ncols_pad, gt_stride, k_chunk);
}

// ---------------------------------------------------------------------- //
// K2, whole-fa tile (fa <= K2F_MAX_FA).
//
// LDS, all in the one extern array: NS stages of [A: 18 chunks][B: BNT/16
// chunks] followed by one spare chunk; a chunk is 16 rows x 32 k of bf16
// (1 KiB), one global_load_lds_dwordx4 of one wave, in the XOR-swizzled
// image frag_load reads.  MI = fa / 32 is a template parameter: only the
// 2 * MI A chunks below fa are staged and multiplied, so XsT rows at or
// past fa are never touched, and nothing in the loop is guarded.
//
// Staging: the chunks of a stage are dealt round-robin to the 8 waves,
// chunk c = w + 8*s for slot s < G, G = ceil(chunks / 8).  A wave whose
// last slot falls past the stage's chunks re-loads the first B chunk into
// the spare chunk instead, so every wave issues exactly G loads per stage
// and one vmcnt count is right for all of them.
//
// Ring: stage t lives in buffer t % NS and is issued D = NS - 1 steps
// ahead.  Step t:
//     s_waitcnt vmcnt(G * min(D - 1, T - 1 - t))   this wave's loads of
//                                                  stage t have landed
//     s_barrier        every wave's have, and every wave has finished
//                      reading stage t - 1
//     issue stage t + D into the buffer of stage t - 1
//     fragments + MFMAs of stage t
// so D - 1 stages stay in flight across the barrier; the count reaches 0
// only in the last step of a slab.  No VGPR-destination global load is
// issued anywhere in the kernel.
// ---------------------------------------------------------------------- //
#define K2F_MAX_FA 288
#define K2F_A_BYTES (K2F_MAX_FA * BK * 2)

static __device__ __forceinline__ void wait_vmcnt(int n) {
    #define K2F_W(N) \
        case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    switch (n) {
    K2F_W(1) K2F_W(2) K2F_W(3) K2F_W(4) K2F_W(5) K2F_W(6) K2F_W(7) K2F_W(8)
    K2F_W(9) K2F_W(10) K2F_W(11) K2F_W(12) K2F_W(13) K2F_W(14) K2F_W(15)
    K2F_W(16)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
    #undef K2F_W
}

template <int BNT, int NS, int MI>
static __device__ __forceinline__ void grad_partial_fullm_body(
    const __bf16* __restrict__ XsT,  // [fa_store][n_pad]
    const __bf16* __restrict__ GT,   // [ncols_pad][gt_stride]
    float* __restrict__ partial,     // [SPLITK][fa][ncols_pad]
    int start, int m_pad, long long n_pad, int fa, int ncols_pad,
    int gt_stride, int k_chunk)
{
    extern __shared__ __attribute__((aligned(16))) char sm[];
    constexpr int NCB = BNT / 16;            // B chunks per stage
    constexpr int NI = BNT / 64;             // column fragments per wave
    constexpr int NCA = 2 * MI;              // A chunks (MI = fa / 32)
    constexpr int STAGE = K2F_A_BYTES + NCB * 1024;
    constexpr int SPARE = NS * STAGE;
    constexpr int G = (NCA + NCB + 7) / 8;   // loads per wave per stage
    constexpr int D = NS - 1;
    static_assert(G * (D - 1) <= 16, "wait_vmcnt covers 0..16");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int z = blockIdx.x;   // slab first: see the K2 comment block
    const int bn = blockIdx.y * BNT;

    const int k0 = z * k_chunk;
    const int k1 = min(m_pad, k0 + k_chunk);
    const int T = (k1 > k0) ? (k1 - k0) / BK : 0;

    // per slot: source of this lane's 16 B at k0, LDS offset of the chunk,
    // and whether the offset moves with the stage (the spare does not)
    const int lr = lane >> 2;
    const int slot = (lane & 3) ^ ((lr >> 2) & 3);
    const __bf16* src[G];
    int dst[G], per_stage[G];
    #pragma unroll
    for (int s = 0; s < G; ++s) {
        const int c = w + 8 * s;
        if (c < NCA) {
            src[s] = XsT + (long long)(16 * c + lr) * n_pad + start + k0 +
                     slot * 8;
            dst[s] = c * 1024;
            per_stage[s] = STAGE;
        } else {
            const bool real = c < NCA + NCB;
            const int cb = real ? c - NCA : 0;
            src[s] = GT + (long long)(bn + 16 * cb + lr) * gt_stride + k0 +
                     slot * 8;
            dst[s] = real ? K2F_A_BYTES + cb * 1024 : SPARE;
            per_stage[s] = real ? STAGE : 0;
        }
    }
    #define K2F_ISSUE(buf, kt)                                              \
        do {                                                                \
            _Pragma("unroll") for (int s = 0; s < G; ++s)                   \
                __builtin_amdgcn_global_load_lds(                           \
                    (const unsigned int*)(src[s] + (kt) * BK),              \
                    (unsigned int*)(sm + (buf) * per_stage[s] + dst[s]),    \
                    16, 0, 0);                                              \
        } while (0)

    const int r = w >> 2;
    const int wc = (w & 3) * (BNT / 4);
    const int fr = lane & 15;
    const int fk = (lane >> 4) * 8;

    f32x4 acc[MI][NI] = {};
    for (int t = 0; t < D && t < T; ++t) K2F_ISSUE(t, t);
    int cur = 0;      // buffer of stage t
    int nxt = D % NS; // buffer of stage t + D
    for (int t = 0; t < T; ++t) {
        wait_vmcnt(G * min(D - 1, T - 1 - t));
        __builtin_amdgcn_s_barrier();
        if (t + D < T) K2F_ISSUE(nxt, t + D);
        const __bf16* A = (const __bf16*)(sm + cur * STAGE);
        const __bf16* B = (const __bf16*)(sm + cur * STAGE + K2F_A_BYTES);
        bf16x8 bfr[NI];
        #pragma unroll
        for (int ni = 0; ni < NI; ++ni)
            bfr[ni] = frag_load(B, wc + ni * 16 + fr, fk);
        bf16x8 af[MI];
        #pragma unroll
        for (int mi = 0; mi < MI; ++mi)
            af[mi] = frag_load(A, (2 * mi + r) * 16 + fr, fk);
        #pragma unroll
        for (int mi = 0; mi < MI; ++mi)
            #pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[mi][ni] =
                    MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        cur = (cur + 1 == NS) ? 0 : cur + 1;
        nxt = (nxt + 1 == NS) ? 0 : nxt + 1;
    }
    #undef K2F_ISSUE

    float* out = partial + (long long)z * fa * ncols_pad;
    const int rw = lane >> 4;
    #pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int rowb = (2 * mi + r) * 16 + rw * 4;
        #pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int col = bn + wc + ni * 16 + fr;
            #pragma unroll
            for (int j = 0; j < 4; ++j)
                out[(long long)(rowb + j) * ncols_pad + col] =
                    acc[mi][ni][j];
        }
    }
}

#define K2F_BN 128
#define K2F_NS 3
#define K2F_LDS (K2F_NS * (K2F_A_BYTES + K2F_BN / 16 * 1024) + 1024)

// one instantiation per fa / 32, chosen workgroup-uniformly.
// __launch_bounds__(512): 103 VGPRs, no AGPRs, no scratch, 80896 B of LDS:
// two workgroups fit a CU, and the flagship's grid (8 x 24 = 192) puts one
// on each of 192 CUs, 2 waves per SIMD.
extern "C" __global__ __launch_bounds__(512) void k_grad_partial_fullm(
    const __bf16* __restrict__ XsT, const __bf16* __restrict__ GT,
    float* __restrict__ partial,
    int start, int m_pad, long long n_pad, int fa, int ncols_pad,
    int gt_stride, int k_chunk)
{
    #define K2F_CASE(MI)                                                    \
        case MI:                                                            \
            grad_partial_fullm_body<K2F_BN, K2F_NS, MI>(                    \
                XsT, GT, partial, start, m_pad, n_pad, fa, ncols_pad,       \
                gt_stride, k_chunk);                                        \
            break;
    switch (fa >> 5) {
    K2F_CASE(1) K2F_CASE(2) K2F_CASE(3) K2F_CASE(4) K2F_CASE(5)
    K2F_CASE(6) K2F_CASE(7) K2F_CASE(8) K2F_CASE(9)
    default: break;
    }
    #undef K2F_CASE
}

// ---------------------------------------------------------------------- //
// K2 launcher.  variant 0 is the rule sgd_step uses: the whole-fa kernel
// for fa <= K2F_MAX_FA, else the 96-row tile where it pads fa with fewer
// rows than the 128-row tile.  1 / 2 / 3 force the 128-row tile, the
// 96-row tile and the whole-fa kernel (tests, timing).
// ---------------------------------------------------------------------- //
static hipError_t launch_grad_partial(
    const void* XsT, const void* GT, void* partial, int start, int m_pad,
    long long n_pad, long long fa_store, int fa, int ncols_pad,
    int gt_stride, int splitk, int variant, hipStream_t stream)
{
    const int k_chunk = (int)((m_pad / splitk + BK - 1) / BK) * BK;
    const long long r96 = (fa + 95LL) / 96 * 96;
    const long long r128 = (fa + 127LL) / 128 * 128;
    if (variant == 0)
        variant = fa <= K2F_MAX_FA ? 3 : (r96 < r128 ? 2 : 1);
    if (variant == 3) {
        if (fa > K2F_MAX_FA || fa > fa_store) return hipErrorInvalidValue;
        const size_t lds = K2F_LDS;
        // more than 64 KiB of dynamic LDS has to be allowed once per
        // device; the first launch on a device is never a captured one
        // (run_epochs_graphed runs epoch 0 eagerly)
        static std::atomic<bool> allowed[64];
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        std::atomic<bool>& ok = allowed[dev & 63];
        if (!ok.load(std::memory_order_acquire)) {
            HIP_CHECK(hipFuncSetAttribute(
                (const void*)k_grad_partial_fullm,
                hipFuncAttributeMaxDynamicSharedMemorySize,
                (int)lds));
            ok.store(true, std::memory_order_release);
        }
        dim3 grid(splitk, ncols_pad / K2F_BN);
        hipLaunchKernelGGL(k_grad_partial_fullm, grid, dim3(512), lds,
                           stream,
                           (const __bf16*)XsT, (const __bf16*)GT,
                           (float*)partial, start, m_pad, n_pad, fa,
                           ncols_pad, gt_stride, k_chunk);
        return hipGetLastError();
    }
    if (variant != 1 && variant != 2) return hipErrorInvalidValue;
    const bool t96 = variant == 2;
    const long long rows = t96 ? r96 : r128;
    if (rows > fa_store) return hipErrorInvalidValue;  // XsT rows read
    dim3 grid((unsigned)(rows / (t96 ? 96 : 128)), ncols_pad / BN, splitk);
    hipLaunchKernelGGL(t96 ? k_grad_partial_96 : k_grad_partial, grid,
                       dim3(256), 32768, stream,
                       (const __bf16*)XsT, (const __bf16*)GT,
                       (float*)partial, start, m_pad, n_pad, fa, ncols_pad,
                       gt_stride, k_chunk);
    return hipGetLastError();
}

extern "C" hipError_t skdist_grad_partial(
    const void* XsT, const void* GT, void* partial, long long start,
    long long m, long long n_pad, long long fa_store, int fa, int ncols_pad,
    int gt_stride, int splitk, int variant, hipStream_t stream)
{
    const int m_pad = (int)((m + BM - 1) / BM) * BM;
    return launch_grad_partial(XsT, GT, partial, (int)start, m_pad, n_pad,
                               fa_store, fa, ncols_pad, gt_stride, splitk,
                               variant, stream);
}

// ---------------------------------------------------------------------- //
// K3: reduce partials, update W (+momentum), refresh WbfT
// grid: (ncols_pad/128, fa), block 128
//
// L1 = true adds the cumulative-penalty L1 step (Tsuruoka et al. 2009;
// eager twin: _sgd._l1_clip_torch) after the gradient step.  Per weight
// two credits live in [fa][ncols_pad] f32 tables: cpos = u + q is what a
// positive weight still owes, cneg = u - q what a negative one owes
// (u: penalty that could have been applied so far, q: signed penalty
// actually applied).  Both advance by lr * lr_scale * l1 * l1_gain per
// step, l1_gain = 1 / (1 - momentum); a weight is clipped towards 0 by
// its credit, never across 0, and a weight at exactly 0 stays there.
// Every lane reads and writes only its own (row, col) entries, so no
// lane depends on what another block writes in the same launch.
// ---------------------------------------------------------------------- //
template <bool L1>
static __device__ __forceinline__ void reduce_update_body(
    const float* __restrict__ partial,
    float* __restrict__ W,
    float* __restrict__ V,
    __bf16* __restrict__ WbfT,
    const float* __restrict__ col_lr,
    const float* __restrict__ col_l2,
    const unsigned char* __restrict__ fmask,  // [fa][ncols_pad] or null:
    float inv_m, float lr_scale, float momentum,  // 0 pins W to 0 (the
    int intercept_row, int splitk, int fa, int ncols_pad,  // per-column
    const float* __restrict__ col_l1,         // feature-subset device path)
    float* __restrict__ cpos, float* __restrict__ cneg, float l1_gain)
{
    const int col = blockIdx.x * 128 + threadIdx.x;
    const int row = blockIdx.y;
    const long long e = (long long)row * ncols_pad + col;

    float s = 0.f;
    for (int z = 0; z < splitk; ++z)
        s += partial[(long long)z * fa * ncols_pad + e];

    float wv = W[e];
    const float l2 = (row == intercept_row) ? 0.f : col_l2[col];
    const float grad = s * inv_m + l2 * wv;
    float step = col_lr[col] * lr_scale * grad;
    if (momentum > 0.f) {
        const float v = V[e] * momentum + step;
        V[e] = v;
        step = v;
    }
    wv -= step;
    if (L1 && row != intercept_row) {
        const float delta = col_lr[col] * lr_scale * col_l1[col] * l1_gain;
        float cp = cpos[e] + delta;
        float cn = cneg[e] + delta;
        float wn = wv;
        if (wv > 0.f) wn = fmaxf(wv - cp, 0.f);
        else if (wv < 0.f) wn = fminf(wv + cn, 0.f);
        const float d = wn - wv;
        cp += d;
        cn -= d;
        wv = wn;
        if (fmask != nullptr && fmask[e] == 0) { cp = 0.f; cn = 0.f; }
        cpos[e] = cp;
        cneg[e] = cn;
    }
    if (fmask != nullptr && fmask[e] == 0) {
        wv = 0.f;
        if (momentum > 0.f) V[e] = 0.f;
    }
    W[e] = wv;
    WbfT[(long long)col * fa + row] = f32_to_bf16(wv);
}

extern "C" __global__ __launch_bounds__(128) void k_reduce_update(
    const float* __restrict__ partial, float* __restrict__ W,
    float* __restrict__ V, __bf16* __restrict__ WbfT,
    const float* __restrict__ col_lr, const float* __restrict__ col_l2,
    const unsigned char* __restrict__ fmask,
    float inv_m, float lr_scale, float momentum,
    int intercept_row, int splitk, int fa, int ncols_pad)
{
    reduce_update_body<false>(partial, W, V, WbfT, col_lr, col_l2, fmask,
                              inv_m, lr_scale, momentum, intercept_row,
                              splitk, fa, ncols_pad, nullptr, nullptr,
                              nullptr, 0.f);
}

extern "C" __global__ __launch_bounds__(128) void k_reduce_update_l1(
    const float* __restrict__ partial, float* __restrict__ W,
    float* __restrict__ V, __bf16* __restrict__ WbfT,
    const float* __restrict__ col_lr, const float* __restrict__ col_l2,
    const unsigned char* __restrict__ fmask,
    float inv_m, float lr_scale, float momentum,
    int intercept_row, int splitk, int fa, int ncols_pad,
    const float* __restrict__ col_l1, float* __restrict__ cpos,
    float* __restrict__ cneg, float l1_gain)
{
    reduce_update_body<true>(partial, W, V, WbfT, col_lr, col_l2, fmask,
                             inv_m, lr_scale, momentum, intercept_row,
                             splitk, fa, ncols_pad, col_l1, cpos, cneg,
                             l1_gain);
}

// ---------------------------------------------------------------------- //
// host launcher.  col_l1 == null is the L2-only step (k_reduce_update);
// otherwise cpos/cneg are the [fa][ncols_pad] L1 credit tables and K3 is
// k_reduce_update_l1.  K1 and K2 are shared.  loss_id == LOSS_SOFTMAX
// launches k_fwd_gt_softmax with group width group_k (2..128) as K1; every
// other loss launches k_fwd_gt and takes group_k == 0.  Tbits != null
// launches k_fwd_gt_bits as K1 (not with the softmax loss), with Mbits the
// optional mask plane; null Tbits launches the kernels above, unchanged.
// ---------------------------------------------------------------------- //
static hipError_t sgd_step_impl(
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
    const void* Tbits, const void* Mbits, hipStream_t stream)
{
    const int m_pad = (int)((m + BM - 1) / BM) * BM;
    {
        dim3 grid(m_pad / BM, ncols_pad / BN);
        size_t lds = (size_t)BN * LDC * 2 + 3600;
        if (Tbits != nullptr) {
            if (loss_id == LOSS_SOFTMAX || group_k != 0)
                return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_fwd_gt_bits, grid, dim3(256), BITS_LDS,
                               stream,
                               (const __bf16*)Xs, (const __bf16*)WbfT_in,
                               (__bf16*)GT, (const int*)fold,
                               (const int*)col_fold, (const float*)row_w,
                               (const int*)Tbits, (const int*)Mbits,
                               (int)start, (int)m, n, fa, ncols_pad,
                               gt_stride, loss_id);
        } else if (Mbits != nullptr) {
            return hipErrorInvalidValue;  // a mask plane needs targets
        } else if (loss_id == LOSS_SOFTMAX) {
            if (group_k < 2 || group_k > BN) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_fwd_gt_softmax, grid, dim3(256), SMX_LDS,
                               stream,
                               (const __bf16*)Xs, (const __bf16*)WbfT_in,
                               (__bf16*)GT, (const float*)y,
                               (const int*)fold, (const int*)col_class,
                               (const int*)col_fold, (const int*)col_class2,
                               (const float*)row_w, (int)start, (int)m, n,
                               fa, ncols_pad, gt_stride, group_k);
        } else {
            if (group_k != 0) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_fwd_gt, grid, dim3(256), lds, stream,
                               (const __bf16*)Xs, (const __bf16*)WbfT_in,
                               (__bf16*)GT, (const float*)y,
                               (const int*)fold, (const int*)col_class,
                               (const int*)col_fold, (const int*)col_class2,
                               (const float*)row_w, (int)start, (int)m, n,
                               fa, ncols_pad, gt_stride, loss_id);
        }
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(launch_grad_partial(XsT, GT, partial, (int)start, m_pad, n_pad,
                                  fa_store, fa, ncols_pad, gt_stride, splitk,
                                  0, stream));
    {
        dim3 grid(ncols_pad / 128, fa);
        if (col_l1 == nullptr) {
            hipLaunchKernelGGL(k_reduce_update, grid, dim3(128), 0, stream,
                               (const float*)partial, (float*)W, (float*)V,
                               (__bf16*)WbfT, (const float*)col_lr,
                               (const float*)col_l2,
                               (const unsigned char*)fmask, inv_m,
                               lr_scale, momentum, intercept_row, splitk,
                               fa, ncols_pad);
        } else {
            hipLaunchKernelGGL(k_reduce_update_l1, grid, dim3(128), 0,
                               stream,
                               (const float*)partial, (float*)W, (float*)V,
                               (__bf16*)WbfT, (const float*)col_lr,
                               (const float*)col_l2,
                               (const unsigned char*)fmask, inv_m,
                               lr_scale, momentum, intercept_row, splitk,
                               fa, ncols_pad, (const float*)col_l1,
                               (float*)cpos, (float*)cneg,
                               1.f / (1.f - momentum));
        }
        HIP_CHECK(hipGetLastError());
    }
    return hipSuccess;
}

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
    hipStream_t stream)
{
    return sgd_step_impl(Xs, XsT, WbfT_in, GT, W, V, WbfT, partial, y,
                         fold, col_class, col_fold, col_class2, col_lr,
                         col_l2, fmask, row_w, inv_m, start, m, n, n_pad,
                         fa_store, fa, ncols_pad, gt_stride, splitk,
                         loss_id, lr_scale, momentum, intercept_row,
                         nullptr, nullptr, nullptr, group_k, nullptr,
                         nullptr, stream);
}

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
    hipStream_t stream)
{
    if (col_l1 == nullptr || cpos == nullptr || cneg == nullptr)
        return hipErrorInvalidValue;
    return sgd_step_impl(Xs, XsT, WbfT_in, GT, W, V, WbfT, partial, y,
                         fold, col_class, col_fold, col_class2, col_lr,
                         col_l2, fmask, row_w, inv_m, start, m, n, n_pad,
                         fa_store, fa, ncols_pad, gt_stride, splitk,
                         loss_id, lr_scale, momentum, intercept_row,
                         col_l1, cpos, cneg, group_k, nullptr, nullptr,
                         stream);
}

// the step with per-element targets (k_fwd_gt_bits as K1).  col_l1 == null
// is the L2-only update, otherwise cpos / cneg are the L1 credit tables;
// Mbits == null trains every element the fold and row tests let through.
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
    const void* Tbits, const void* Mbits, hipStream_t stream)
{
    if (Tbits == nullptr) return hipErrorInvalidValue;
    if (col_l1 != nullptr && (cpos == nullptr || cneg == nullptr))
        return hipErrorInvalidValue;
    return sgd_step_impl(Xs, XsT, WbfT_in, GT, W, V, WbfT, partial, y,
                         fold, col_class, col_fold, col_class2, col_lr,
                         col_l2, fmask, row_w, inv_m, start, m, n, n_pad,
                         fa_store, fa, ncols_pad, gt_stride, splitk,
                         loss_id, lr_scale, momentum, intercept_row,
                         col_l1, cpos, cneg, 0, Tbits, Mbits, stream);
}

// ---------------------------------------------------------------------- //
// K4: fused standardize + intercept/pad augment + bf16 cast
// out[i][j] = (X[i][j] - mean[j]) * inv_std[j]   for j <  f
//           = 1.0                                 for j == f (intercept)
//           = 0.0                                 for j >  f (K-pad)
// One pass over X instead of the eager sub/div/cat/cast chain
// (DeviceDataset build, skdist_amd/models/_sgd.py).
// grid: ceil(n*fa/8/256), block 256; each thread emits one 16 B chunk.
// ---------------------------------------------------------------------- //
extern "C" __global__ __launch_bounds__(256) void k_standardize(
    const float* __restrict__ X, const float* __restrict__ mean,
    const float* __restrict__ inv_std, __bf16* __restrict__ out,
    long long n, int f, int fa)
{
    const long long chunk =
        (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = n * (long long)fa / 8;
    if (chunk >= total) return;
    const long long e0 = chunk * 8;
    const long long row = e0 / fa;
    const int c0 = (int)(e0 - row * fa);
    const float* xr = X + row * (long long)f;
    short4v lo, hi;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        float v;
        if (c < f)
            v = (xr[c] - mean[c]) * inv_std[c];
        else
            v = (c == f) ? 1.f : 0.f;
        const short b = __builtin_bit_cast(short, f32_to_bf16(v));
        if (j < 4) lo[j] = b; else hi[j - 4] = b;
    }
    *(short4v*)(out + e0) = lo;
    *(short4v*)(out + e0 + 4) = hi;
}

extern "C" hipError_t skdist_standardize(
    const void* X, const void* mean, const void* inv_std, void* out,
    long long n, int f, int fa, hipStream_t stream)
{
    if (fa % 8 != 0) return hipErrorInvalidValue;
    const long long chunks = n * (long long)fa / 8;
    const int blocks = (int)((chunks + 255) / 256);
    hipLaunchKernelGGL(k_standardize, dim3(blocks), dim3(256), 0, stream,
                       (const float*)X, (const float*)mean,
                       (const float*)inv_std, (__bf16*)out, n, f, fa);
    return hipGetLastError();
}

// ---------------------------------------------------------------------- //
// K5: fused test-fold scoring — GEMM tile + per-column sufficient stats
// (the k-fold CV scoring kernel; SURVEY.md §2.4 "k-fold split + score").
// The caller gathers ONE fold's test rows into a 128-padded bf16 buffer
// (pad rows zero, y pad = -1e30 sentinel -> excluded), so no masks are
// needed: every row scores every column.
//   mode 0 (binary accuracy): out[col*2]   += #(sign(z) == y)
//                             out[col*2+1] += #rows           (valid)
//   mode 1 (regression):      out[col]     += (z-y)^2
// (r2's total sum of squares depends on y alone, not on the column: the
// caller takes it from the fold's y in float64, _sgd._score_fold_hip)
// grid: (m_pad/128, ncols_pad/128), block 256 (4 waves of 64x64).
// ---------------------------------------------------------------------- //
extern "C" __global__ __launch_bounds__(256) void k_score(
    const __bf16* __restrict__ Xf,    // [m_pad][fa] gathered fold rows
    const __bf16* __restrict__ WbfT,  // [ncols_pad][fa]
    const float* __restrict__ yf,     // [m_pad] (-1e30 pad sentinel)
    float* __restrict__ out,          // [ncols_pad * (2|1)]
    int fa, int ncols_pad, int mode)
{
    extern __shared__ __attribute__((aligned(16))) char sm[];
    #define sbufA(b) ((__bf16*)(sm + (b) * 16384))
    #define sbufB(b) ((__bf16*)(sm + 8192 + (b) * 16384))
    float* y_s = (float*)(sm + 32768);        // [128]
    float* red = (float*)(sm + 33280);        // [132] per-col partials

    const int tid = threadIdx.x;
    const int bm = blockIdx.x * 128;
    const int bn = blockIdx.y * 128;
    const int lane = tid & 63;
    const int w = tid >> 6;
    if (tid < 128) y_s[tid] = yf[bm + tid];

    const __bf16* Abase = Xf + (long long)bm * fa;
    const __bf16* Bbase = WbfT + (long long)bn * fa;
    const int wr = ((w >> 1) & 1) * 64;
    const int wc = (w & 1) * 64;
    const int fr = lane & 15;
    const int fk = (lane >> 4) * 8;

    f32x4 acc[4][4] = {};
    const int nk = fa / BK;
    int cur = 0;
    {   // stage first tiles (STAGE_TILE expects `row`, `lane`, `w`)
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {
            const int c = w + 4 * i;
            const int row = 16 * c + (lane >> 2);
            const int slot = (lane & 3) ^ ((row >> 2) & 3);
            __builtin_amdgcn_global_load_lds(
                (const unsigned int*)(Abase + (long long)row * fa +
                                      slot * 8),
                (unsigned int*)(sbufA(0) + c * 512), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(
                (const unsigned int*)(Bbase + (long long)row * fa +
                                      slot * 8),
                (unsigned int*)(sbufB(0) + c * 512), 16, 0, 0);
        }
    }
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        if (kt + 1 < nk) {
            _Pragma("unroll") for (int i = 0; i < 2; ++i) {
                const int c = w + 4 * i;
                const int row = 16 * c + (lane >> 2);
                const int slot = (lane & 3) ^ ((row >> 2) & 3);
                __builtin_amdgcn_global_load_lds(
                    (const unsigned int*)(Abase + (long long)row * fa +
                                          (kt + 1) * BK + slot * 8),
                    (unsigned int*)(sbufA(cur ^ 1) + c * 512), 16, 0, 0);
                __builtin_amdgcn_global_load_lds(
                    (const unsigned int*)(Bbase + (long long)row * fa +
                                          (kt + 1) * BK + slot * 8),
                    (unsigned int*)(sbufB(cur ^ 1) + c * 512), 16, 0, 0);
            }
        }
        bf16x8 af[4], bfr[4];
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            af[mi] = frag_load(sbufA(cur), wr + mi * 16 + fr, fk);
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
            bfr[ni] = frag_load(sbufB(cur), wc + ni * 16 + fr, fk);
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] =
                    MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        cur ^= 1;
    }
    __syncthreads();

    // per-lane partials over this wave's 16 rows x 4 col-groups
    const int rw = lane >> 4;
    float s0[4] = {}, s1[4] = {};
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr + mi * 16 + rw * 4 + r;
                const float yv = y_s[row];
                if (yv < -1e29f) continue;   // pad row
                const float z = acc[mi][ni][r];
                if (mode == 0) {
                    s0[ni] += ((z >= 0.f) == (yv != 0.f)) ? 1.f : 0.f;
                    s1[ni] += 1.f;
                } else {
                    const float e = z - yv;
                    s0[ni] += e * e;
                }
            }
        }
    }
    // reduce across the 16 lanes-groups sharing a column (rows axis):
    // lanes with same (lane&15, wc) hold different rows; use LDS.
    const int nstat = (mode == 0) ? 2 : 1;
    for (int st = 0; st < nstat; ++st) {
        __syncthreads();
        for (int i = tid; i < 132; i += 256) red[i] = 0.f;
        __syncthreads();
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const float v = (st == 0) ? s0[ni] : s1[ni];
            atomicAdd(&red[wc + ni * 16 + fr], v);
        }
        __syncthreads();
        for (int c = tid; c < 128; c += 256)
            atomicAdd(&out[(long long)(bn + c) * nstat + st], red[c]);
    }
}

extern "C" hipError_t skdist_score(
    const void* Xf, const void* WbfT, const void* yf, void* out,
    long long m_pad, int fa, int ncols_pad, int mode,
    hipStream_t stream)
{
    dim3 grid((unsigned)(m_pad / 128), ncols_pad / 128);
    hipLaunchKernelGGL(k_score, grid, dim3(256), 33280 + 132 * 4, stream,
                       (const __bf16*)Xf, (const __bf16*)WbfT,
                       (const float*)yf, (float*)out, fa, ncols_pad,
                       mode);
    return hipGetLastError();
}
