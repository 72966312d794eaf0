// "Because you watched" evidence for recommended items on gfx950 (lgcn_explain_topr): per query a
// list of k recommended candidates and a history row of a CSR in, per (query, slot) the r history
// items with the largest contribution w * (Cn[i] . Cn[j]) to the slot's candidate j out, with their
// count and the sum of all contributions.
//
//   explain_query    the work of one query, by W waves of one workgroup. The k candidate rows are
//                    staged in LDS once (float4 loads, the rows of empty slots zero), then the
//                    history is streamed in rounds of 16 entries per wave, wave w of W taking the
//                    rounds w, w + W, ... A round is the 16 x D by D x 16 product of its entries'
//                    rows with 16 slots' rows, on v_mfma_f32_16x16x4_f32 (f32 in, f32 out, a
//                    k-ordered fma chain): entry c of the round is row c of the A operand, slot
//                    s * 16 + c column c of B, so lane (g, c) loads float4 g, g + 4, g + 8, g + 12
//                    of every 64-column block of its entry's row (the four lanes of an entry read
//                    64 consecutive bytes per instruction) and of its slot's LDS row, component
//                    x, y, z, w of float4 j being k-step 4 j + 0 .. 3 for both operands. The tile
//                    comes out with column c on lane c: lane (g, c) holds the dots of ITS slot
//                    with entries 4 g .. 4 g + 3 of the round, no exchange between lanes. The loads
//                    run two rounds ahead of the arithmetic: a round issues the item indices of
//                    the round after next and the rows of the next one (their indices arrived a
//                    round ago) before it touches its own rows. Each lane keeps its slot's running
//                    top-8 in registers as 64-bit words, ordered value image above, inverted item
//                    index below (the larger word is the larger contribution, then the lower
//                    index), so insertion is a compare-exchange chain behind one comparison and
//                    ties are exact; the slot's sum rides in the same lane. Slots 16 .. 63 use
//                    further accumulators and register sets (template KS = ceil(k / 16)); with up
//                    to two sets the first 64 columns of the slots' rows stay in registers (all of
//                    a row at D = 64), otherwise they are read from LDS every round. At the end the
//                    four lanes' lists of a slot are merged by two exchange rounds, the W waves'
//                    lists through LDS (over the rows, which nobody needs any more), and wave 0
//                    stores.
//   k_explain_topr       one wave per query, one query per 64-thread workgroup (W = 1): every
//                        query whose history has at most kExplainLong entries.
//   k_explain_topr_long  a 512-thread workgroup per eight consecutive queries: those among them
//                        with a longer history, one after the other, by all eight waves (W = 8).
//                        A workgroup without one ends after reading eight row lengths.
//
// Why this shape. A query's work is len(history) * k short dot products against k rows that never
// change: the k rows belong in LDS (k * D * 4 bytes, unpadded: at most 64 KiB at the limits k = 64,
// D = 256, which the default dynamic-LDS ceiling admits), the history rows are read once each, and
// nothing is shared with another query. The first version formed the dots on the vector ALU, a row
// per 16-lane group, and moved slot t's sum to lane t with a transposing butterfly: about 1,500
// vector instructions per 16 entries, and issue-bound at that. The matrix core takes the products
// AND leaves the result in the layout the lists want. A slot's row is read by one lane as four
// float4 at a stride of the row length, a 16-way bank conflict on ds_read_b128; it is paid once per
// query where the rows stay in registers, every round above two slot sets or 64 columns.
// Histories are heavy-tailed (ML-25M-shaped: mean 77, longest 31,703): with one wave per query
// whatever its length the longest history alone ran 8.0 ms of the 8.5 ms all 162,541 users took, so
// long histories get eight waves, and the short ones, which are nearly all, keep the 64-thread
// workgroup whose occupancy does not pay for seven idle waves. The two launches write disjoint
// queries. No atomics, no waiting on other workgroups, nothing allocated, stream-ordered.
#include "lgcn_common.h"
#include "lgcn_ragged.h"

#include <cmath>

#pragma clang fp contract(off)

namespace lgcn {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kExplainList = LGCN_EXPLAIN_MAX_R;  // words of a slot's running list
constexpr int kExplainWaves = 8;                  // waves that share a long history
constexpr int kExplainLong = 512;                 // history entries above which they do
constexpr int kExplainMergeBytes = kExplainList * 8 + 4;  // a wave's list and sum of one slot, in LDS

// value image (NaN as -inf, -0 as +0) | inverted item index (31 bits) | "the value is a number" (a NaN decodes as NaN again)
__device__ __forceinline__ unsigned long long explain_word(float v, int32_t i) {
    const uint32_t low = (0x7FFFFFFFu - static_cast<uint32_t>(i)) << 1 | (v == v ? 1u : 0u);
    return static_cast<unsigned long long>(ordered_key_nan_last(v)) << 32 | low;
}

// keep the kExplainList largest words, descending (0 = empty)
__device__ __forceinline__ void explain_insert(unsigned long long (&L)[kExplainList], unsigned long long w) {
    if (w > L[kExplainList - 1]) {
#pragma unroll
        for (int p = 0; p < kExplainList; ++p) {
            const unsigned long long hi = w > L[p] ? w : L[p];
            w = w > L[p] ? L[p] : w;
            L[p] = hi;
        }
    }
}

// Query q by the W waves of the calling workgroup (64 * W threads, all of them call); smem holds
// max(k * D * 4, (W - 1) * k * kExplainMergeBytes) bytes.
template <int KS, int W>
__device__ __forceinline__ void explain_query(char* smem, int64_t q, int64_t beg, int64_t end,
                                              const int32_t* __restrict__ rec_idx, int64_t ld, int32_t k,
                                              const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w,
                                              const float* __restrict__ Cn, int64_t M, int32_t D, int32_t r,
                                              int32_t* __restrict__ out_idx, float* __restrict__ out_val,
                                              int32_t* __restrict__ out_n, float* __restrict__ out_sum) {
    constexpr int kRound = 16;  // history entries per wave and round: one MFMA tile
    float4* rows = reinterpret_cast<float4*>(smem);
    const float4* Cn4 = reinterpret_cast<const float4*>(Cn);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int c4 = D >> 2;  // float4 per row

    // this lane's slots: t = s * 16 + c, its candidate (-1: an empty slot)
    int32_t recj[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = s * 16 + c;
        recj[s] = -1;
        if (t < k) {
            const int32_t j = rec_idx[q * ld + t];
            if (j >= 0 && static_cast<int64_t>(j) < M) recj[s] = j;
        }
    }
    if (W > 1) __syncthreads();  // the workgroup's previous query is done with the LDS
    // stage the k candidate rows: float4 e of the image is column e % c4 of slot e / c4
    for (int e = tid; e < k * c4; e += 64 * W) {
        const int t = e / c4, cc = e - t * c4;
        const int32_t j = rec_idx[q * ld + t];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j >= 0 && static_cast<int64_t>(j) < M) v = Cn4[static_cast<int64_t>(j) * c4 + cc];
        rows[e] = v;
    }
    __syncthreads();

    unsigned long long L[KS][kExplainList];
    float sum[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        sum[s] = 0.f;
#pragma unroll
        for (int p = 0; p < kExplainList; ++p) L[s][p] = 0ull;
    }

    // A round is 16 history entries, one v_mfma_f32_16x16x4_f32 tile: entry e0 + c is row c of the A
    // operand (this lane loads four float4 of its row), slot s * 16 + c column c of B, and the result
    // leaves this lane with the dots of ITS slot and entries e0 + 4 g .. 4 g + 3. So a lane needs the
    // item of entry e0 + c for the rows, and item and weight of its four result entries
    // (-1: none, or outside [0, M) and never read).
    auto entries = [&](int64_t e0, int32_t& ia, int32_t(&hi)[4], float(&hw)[4]) {
        ia = -1;
        if (e0 + c < end) {
            const int32_t i = hist_idx[e0 + c];
            if (i >= 0 && static_cast<int64_t>(i) < M) ia = i;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t e = e0 + 4 * g + u;
            hi[u] = -1;
            hw[u] = 1.f;
            if (e < end) {
                const int32_t i = hist_idx[e];
                if (i >= 0 && static_cast<int64_t>(i) < M) hi[u] = i;
                if (hist_w) hw[u] = hist_w[e];
            }
        }
    };
    // float4 g, g + 4, g + 8, g + 12 of block jb (64 columns) of item ia's row / of this lane's slot
    // of set s: component x, y, z, w of float4 j is the k-step 4 j + 0 .. 3 of the block for both
    auto load_a = [&](int32_t ia, int jb, float4(&a)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cc = jb * 16 + g + 4 * j;
            a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ia >= 0 && cc < c4) a[j] = Cn4[static_cast<int64_t>(ia) * c4 + cc];
        }
    };
    auto load_b = [&](int s, int jb, float4(&b)[4]) {
        const int t = s * 16 + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cc = jb * 16 + g + 4 * j;
            b[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < k && cc < c4) b[j] = rows[t * c4 + cc];
        }
    };
    const int nblk = (c4 + 15) >> 4;
    // block 0 of the slots' rows stays in registers (all of a row up to D = 64) while they are few
    constexpr bool kKeepB = KS <= 2;
    float4 b0[kKeepB ? KS : 1][4];
    if (kKeepB) {
#pragma unroll
        for (int s = 0; s < KS; ++s) load_b(s, 0, b0[kKeepB ? s : 0]);
    }

    const int64_t stride = static_cast<int64_t>(W) * kRound;
    int64_t e0 = beg + wv * kRound;
    int32_t ia1, ia2, hi1[4], hi2[4];  // the next round's entries, and those of the round after it
    float hw1[4], hw2[4];
    float4 a1[4];                      // the next round's rows (block 0)
    entries(e0, ia1, hi1, hw1);
    load_a(ia1, 0, a1);
    entries(e0 + stride, ia2, hi2, hw2);
    for (; e0 < end; e0 += stride) {  // wave-uniform
        int32_t ia = ia1, hi[4];
        float hw[4];
        float4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            hi[u] = hi1[u];
            hw[u] = hw1[u];
            a[u] = a1[u];
            hi1[u] = hi2[u];
            hw1[u] = hw2[u];
        }
        ia1 = ia2;
        load_a(ia1, 0, a1);  // in flight while this round computes
        entries(e0 + 2 * stride, ia2, hi2, hw2);
        f32x4 acc[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int jb = 0; jb < nblk; ++jb) {
            if (jb > 0) load_a(ia, jb, a);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                float4 b[4];
                if (kKeepB && jb == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = b0[kKeepB ? s : 0][j];
                } else {
                    load_b(s, jb, b);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 bj = b[j];
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, bj.x, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, bj.y, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, bj.z, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, bj.w, acc[s], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int32_t j = recj[s];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (hi[u] >= 0 && j >= 0 && hi[u] != j) {
                    float cv = acc[s][u];
                    if (hist_w) cv = hw[u] * cv;
                    sum[s] += cv;
                    explain_insert(L[s], explain_word(cv, hi[u]));
                }
            }
        }
    }

    // merge the four lanes' lists of each slot (an entry was seen by one of them only: no duplicates)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            unsigned long long O[kExplainList];
#pragma unroll
            for (int p = 0; p < kExplainList; ++p) O[p] = __shfl_xor(L[s][p], off, 64);
#pragma unroll
            for (int p = 0; p < kExplainList; ++p) explain_insert(L[s], O[p]);
            sum[s] += __shfl_xor(sum[s], off, 64);
        }
    }
    if (W > 1) {  // then the waves' lists, through LDS: wave 0 collects, in wave order
        unsigned long long* mlist = reinterpret_cast<unsigned long long*>(smem);
        float* msum = reinterpret_cast<float*>(smem + static_cast<size_t>(W - 1) * k * kExplainList * 8);
        __syncthreads();  // every wave is done with the rows
        if (wv > 0 && g == 0) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int t = s * 16 + c;
                if (t < k) {
                    const int at = (wv - 1) * k + t;
#pragma unroll
                    for (int p = 0; p < kExplainList; ++p) mlist[at * kExplainList + p] = L[s][p];
                    msum[at] = sum[s];
                }
            }
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int t = s * 16 + c;
                if (t < k) {
                    for (int w = 1; w < W; ++w) {
                        const int at = (w - 1) * k + t;
#pragma unroll
                        for (int p = 0; p < kExplainList; ++p) explain_insert(L[s], mlist[at * kExplainList + p]);
                        sum[s] += msum[at];
                    }
                }
            }
        }
    }
    if (wv != 0) return;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = s * 16 + c;
        if (t < k) {
            const int64_t base = (q * k + t) * r;
            int32_t n = 0;
#pragma unroll
            for (int p = 0; p < kExplainList; ++p) {
                const unsigned long long w = L[s][p];
                if (p < r) {
                    n += w != 0ull;
                    if ((p & 3) == g) {  // the slot's four lanes share the stores
                        const uint32_t low = static_cast<uint32_t>(w);
                        const float val = (low & 1u) ? ordered_value(static_cast<uint32_t>(w >> 32)) : NAN;
                        out_idx[base + p] = w ? static_cast<int32_t>(0x7FFFFFFFu - (low >> 1)) : -1;
                        out_val[base + p] = w ? val : -INFINITY;
                    }
                }
            }
            if (g == 0) {
                out_n[q * k + t] = n;
                if (out_sum) out_sum[q * k + t] = sum[s];
            }
        }
    }
}

template <int KS>
__global__ __launch_bounds__(64) void k_explain_topr(
    const int32_t* __restrict__ rec_idx, int64_t ld, int32_t k, const int64_t* __restrict__ hist_ptr,
    const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w, const int64_t* __restrict__ hist_row,
    int64_t hist_rows, const float* __restrict__ Cn, int64_t M, int32_t D, int32_t r, int32_t* __restrict__ out_idx,
    float* __restrict__ out_val, int32_t* __restrict__ out_n, float* __restrict__ out_sum) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t q = blockIdx.x;
    int64_t beg, end;
    ragged_row(q, hist_ptr, hist_row, hist_rows, beg, end);
    if (end - beg > kExplainLong) return;  // k_explain_topr_long's
    explain_query<KS, 1>(smem, q, beg, end, rec_idx, ld, k, hist_idx, hist_w, Cn, M, D, r, out_idx, out_val, out_n,
                         out_sum);
}

template <int KS>
__global__ __launch_bounds__(64 * kExplainWaves) void k_explain_topr_long(
    const int32_t* __restrict__ rec_idx, int64_t ld, int32_t k, int64_t Q, const int64_t* __restrict__ hist_ptr,
    const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w, const int64_t* __restrict__ hist_row,
    int64_t hist_rows, const float* __restrict__ Cn, int64_t M, int32_t D, int32_t r, int32_t* __restrict__ out_idx,
    float* __restrict__ out_val, int32_t* __restrict__ out_n, float* __restrict__ out_sum) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int i = 0; i < kExplainWaves; ++i) {  // workgroup-uniform throughout
        const int64_t q = static_cast<int64_t>(blockIdx.x) * kExplainWaves + i;
        if (q >= Q) break;
        int64_t beg, end;
        ragged_row(q, hist_ptr, hist_row, hist_rows, beg, end);
        if (end - beg > kExplainLong)
            explain_query<KS, kExplainWaves>(smem, q, beg, end, rec_idx, ld, k, hist_idx, hist_w, Cn, M, D, r, out_idx,
                                             out_val, out_n, out_sum);
    }
}

}  // namespace lgcn

using namespace lgcn;

namespace {

template <int KS>
int launch_explain(const int32_t* rec_idx, int64_t ld, int32_t k, int64_t Q, const int64_t* hist_ptr,
                   const int32_t* hist_idx, const float* hist_w, const int64_t* hist_row, int64_t hist_rows,
                   const float* Cn, int64_t M, int32_t D, int32_t r, int32_t* out_idx, float* out_val, int32_t* out_n,
                   float* out_sum, hipStream_t s) {
    const size_t lds = static_cast<size_t>(k) * D * 4;
    k_explain_topr<KS><<<dim3(static_cast<unsigned>(Q)), 64, lds, s>>>(rec_idx, ld, k, hist_ptr, hist_idx, hist_w,
                                                                      hist_row, hist_rows, Cn, M, D, r, out_idx,
                                                                      out_val, out_n, out_sum);
    int rc = check_launch("k_explain_topr");
    if (rc != LGCN_OK) return rc;
    const size_t merge = static_cast<size_t>(kExplainWaves - 1) * k * kExplainMergeBytes;
    const unsigned groups = static_cast<unsigned>((Q + kExplainWaves - 1) / kExplainWaves);
    k_explain_topr_long<KS><<<dim3(groups), 64 * kExplainWaves, lds > merge ? lds : merge, s>>>(
        rec_idx, ld, k, Q, hist_ptr, hist_idx, hist_w, hist_row, hist_rows, Cn, M, D, r, out_idx, out_val, out_n,
        out_sum);
    return check_launch("k_explain_topr_long");
}

}  // namespace

extern "C" {

int lgcn_explain_topr(const int32_t* rec_idx, int64_t ld, int32_t k, int64_t Q, const int64_t* hist_ptr,
                      const int32_t* hist_idx, const float* hist_w, const int64_t* hist_row, int64_t hist_rows,
                      const float* Cn, int64_t M, int32_t D, int32_t r, int32_t* out_idx, float* out_val,
                      int32_t* out_n, float* out_sum, lgcn_stream_t stream) {
    const char* me = "lgcn_explain_topr";
    if (!rec_idx) return fail(LGCN_E_ARG, "%s: rec_idx is null", me);
    if (!hist_ptr) return fail(LGCN_E_ARG, "%s: hist_ptr is null", me);
    if (!hist_idx) return fail(LGCN_E_ARG, "%s: hist_idx is null", me);
    if (!Cn) return fail(LGCN_E_ARG, "%s: Cn is null", me);
    if (!out_idx) return fail(LGCN_E_ARG, "%s: out_idx is null", me);
    if (!out_val) return fail(LGCN_E_ARG, "%s: out_val is null", me);
    if (!out_n) return fail(LGCN_E_ARG, "%s: out_n is null", me);
    if (k < 1 || k > ld) return fail(LGCN_E_ARG, "%s: k=%d outside [1, ld=%lld]", me, k, (long long)ld);
    if (r < 1) return fail(LGCN_E_ARG, "%s: r=%d", me, r);
    if (Q < 0) return fail(LGCN_E_ARG, "%s: Q=%lld", me, (long long)Q);
    if (M < 0) return fail(LGCN_E_ARG, "%s: M=%lld", me, (long long)M);
    if (hist_rows < 0) return fail(LGCN_E_ARG, "%s: hist_rows=%lld", me, (long long)hist_rows);
    if (D < 1 || D > 256) return fail(LGCN_E_ARG, "%s: D=%d outside [1, 256]", me, D);
    if (D % 4 != 0) return fail(LGCN_E_ARG, "%s: D=%d is not a multiple of 4 (use lgcn_recall_width)", me, D);
    if (reinterpret_cast<uintptr_t>(Cn) % 16 != 0) return fail(LGCN_E_ARG, "%s: Cn is not 16-byte aligned", me);
    if (k > LGCN_EXPLAIN_MAX_K)
        return fail(LGCN_E_UNSUPPORTED, "%s: k=%d exceeds LGCN_EXPLAIN_MAX_K=%d", me, k, LGCN_EXPLAIN_MAX_K);
    if (r > LGCN_EXPLAIN_MAX_R)
        return fail(LGCN_E_UNSUPPORTED, "%s: r=%d exceeds LGCN_EXPLAIN_MAX_R=%d", me, r, LGCN_EXPLAIN_MAX_R);
    if (Q > INT32_MAX) return fail(LGCN_E_ARG, "%s: Q=%lld is too many queries for one launch", me, (long long)Q);
    if (Q == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
    const int sets = (k + 15) / 16;
#define LGCN_EXPLAIN_ARGS \
    rec_idx, ld, k, Q, hist_ptr, hist_idx, hist_w, hist_row, hist_rows, Cn, M, D, r, out_idx, out_val, out_n, out_sum, s
    if (sets <= 1) return launch_explain<1>(LGCN_EXPLAIN_ARGS);
    if (sets <= 2) return launch_explain<2>(LGCN_EXPLAIN_ARGS);
    if (sets <= 3) return launch_explain<3>(LGCN_EXPLAIN_ARGS);
    static_assert(LGCN_EXPLAIN_MAX_K == 64 && LGCN_EXPLAIN_MAX_R == 8, "the dispatch covers four sets of 16 slots");
    return launch_explain<4>(LGCN_EXPLAIN_ARGS);
#undef LGCN_EXPLAIN_ARGS
}

}  // extern "C"
