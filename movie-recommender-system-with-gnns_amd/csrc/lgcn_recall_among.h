// The kernels of per-query candidate sets (lgcn_score_lists, lgcn_score_lists_boost), their launch and
// the entry points' one argument check. lgcn_recall_among.hip, which describes the kernels,
// instantiates them without a boost and lgcn_recall_boost.hip with one: two translation units, for the
// reason lgcn_recall_lists.h gives for its own two.
// kBoost: the key of entry j is boosted_key(the score behind row_keys' key, boost[j]) — row_keys' key
// maps back to its score bit for bit (a NaN to a NaN, which stays one). The round's boosts are loaded
// with the round's rows, one round ahead.
#pragma once

#include "lgcn_common.h"
#include "lgcn_ragged.h"
#include "lgcn_scoretile.h"

using namespace lgcn;

namespace {

constexpr int kAmongChunk = 512;  // entries of one wave's chunk of a long row
constexpr int kAmongLong = 512;   // row entries above which the waves of a workgroup share a row

template <int D>
constexpr int among_waves() { return D >= 256 ? 4 : 8; }

struct AmongArgs {
    const float* Qn;
    int64_t Q;
    const float* Cn;
    int64_t M;
    const int64_t* among_ptr;
    const int32_t* among_idx;
    const int64_t* among_row;
    int64_t among_rows;
    uint32_t* list_key;
    int32_t* list_idx;
    int32_t* list_n;
    int32_t cap;
};

// A kernel's one argument: AmongArgs, with the boost vector behind it in a boosted instantiation only,
// so the unboosted kernels keep the argument block they had (an empty record of its own would move
// the hidden arguments behind it by eight bytes).
template <bool kBoost>
struct AmongKernelArgs : AmongArgs {};
template <>
struct AmongKernelArgs<true> : AmongArgs {
    const float* boost;  // [M] f32, by candidate index
};

// Query q's row ent[0 .. len) by the W waves of the calling workgroup (64 * W threads, all of them
// call). s_n: the workgroup's slot counter (W > 1; zero on entry, the row's count on return).
template <int D, int W, bool kBoost>
__device__ __forceinline__ void among_query(int32_t* s_n, const AmongKernelArgs<kBoost>& A, int64_t q,
                                            const int32_t* __restrict__ ent, int64_t len) {
    using Tile = ScoreTile<D>;
    constexpr int V = D / 8;  // float4 of a half-row
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const unsigned long long below = (1ull << lane) - 1ull;
    float4 qa[V];
    Tile::load_half(A.Qn, q, h, qa);
    // the candidate of entry e + i (-1: past the row, or outside [0, M): never read, never listed)
    auto entry = [&](int64_t e) -> int32_t {
        int32_t j = -1;
        if (e + i < len) {
            const int32_t v = ent[e + i];
            if (v >= 0 && static_cast<int64_t>(v) < A.M) j = v;
        }
        return j;
    };
    // the wave's round after the one at e: the next 32 entries of its chunk, then its next chunk
    auto next = [&](int64_t e) -> int64_t {
        e += 32;
        if (W > 1 && (e & (kAmongChunk - 1)) == 0) e += static_cast<int64_t>(W - 1) * kAmongChunk;
        return e;
    };
    // candidate j's boost (0 for "none": that lane keeps nothing)
    [[maybe_unused]] auto boost_of = [&](int32_t j) -> float {
        if constexpr (kBoost) return j >= 0 ? A.boost[j] : 0.f;
        return 0.f;
    };
    uint32_t* keys = A.list_key + q * A.cap;
    int32_t* idxs = A.list_idx + q * A.cap;
    int64_t e = static_cast<int64_t>(wv) * kAmongChunk;
    int64_t e1 = next(e);
    int32_t j1 = entry(e), j2 = entry(e1);  // the next round's candidates, and those of the round after it
    float4 b1[V];                            // the next round's rows
    Tile::load_half(A.Cn, j1, h, b1);
    [[maybe_unused]] float bo1 = boost_of(j1);  // ... and boosts
    int32_t total = 0;                       // W == 1: the wave's running count
    for (; e < len; e = e1, e1 = next(e1)) {  // wave-uniform
        const int32_t j = j1;
        float4 b[V];
#pragma unroll
        for (int v = 0; v < V; ++v) b[v] = b1[v];
        [[maybe_unused]] const float bo = bo1;
        j1 = j2;
        Tile::load_half(A.Cn, j1, h, b1);  // in flight while this round computes
        if constexpr (kBoost) bo1 = boost_of(j1);
        j2 = entry(next(e1));
        uint32_t key = Tile::row_keys(qa, b);
        if constexpr (kBoost) key = boosted_key(key_score(key), bo);
        const bool keep = h == 0 && j >= 0;
        const unsigned long long m = __ballot(keep);
        const int n = __popcll(m);
        int32_t base = total;
        if (W == 1) {
            total += n;
        } else {
            int32_t claimed = 0;
            if (lane == 0 && n > 0) claimed = atomicAdd(s_n, n);
            base = __shfl(claimed, 0, 64);
        }
        if (keep) {
            const int32_t p = base + __popcll(m & below);
            if (p < A.cap) {
                keys[p] = key;
                idxs[p] = j;
            }
        }
    }
    if (W == 1) {
        if (lane == 0) A.list_n[q] = total;
    } else {
        __syncthreads();  // every wave's claims are in
        if (threadIdx.x == 0) A.list_n[q] = *s_n;
    }
}

template <int D, bool kBoost = false>
__global__ __launch_bounds__(64) void k_score_lists(const AmongKernelArgs<kBoost> A) {
    const int64_t q = blockIdx.x;
    int64_t beg, end;
    ragged_row(q, A.among_ptr, A.among_row, A.among_rows, beg, end);
    if (end - beg > kAmongLong) return;  // k_score_lists_long's
    among_query<D, 1, kBoost>(nullptr, A, q, A.among_idx + beg, end - beg);
}

template <int D, bool kBoost = false>
__global__ __launch_bounds__(64 * among_waves<D>()) void k_score_lists_long(const AmongKernelArgs<kBoost> A) {
    constexpr int W = among_waves<D>();
    __shared__ int32_t s_n;
    for (int u = 0; u < W; ++u) {  // workgroup-uniform throughout
        const int64_t q = static_cast<int64_t>(blockIdx.x) + static_cast<int64_t>(u) * gridDim.x;
        if (q >= A.Q) break;
        int64_t beg, end;
        ragged_row(q, A.among_ptr, A.among_row, A.among_rows, beg, end);
        if (end - beg <= kAmongLong) continue;
        if (threadIdx.x == 0) s_n = 0;  // thread 0 read the previous query's count before this
        __syncthreads();
        among_query<D, W, kBoost>(&s_n, A, q, A.among_idx + beg, end - beg);
    }
}

template <int D, bool kBoost>
int launch_among(const AmongKernelArgs<kBoost>& A, hipStream_t s) {
    constexpr int W = among_waves<D>();
    k_score_lists<D, kBoost><<<dim3(static_cast<unsigned>(A.Q)), 64, 0, s>>>(A);
    const int rc = check_launch(kBoost ? "k_score_lists<boost>" : "k_score_lists");
    if (rc != LGCN_OK) return rc;
    k_score_lists_long<D, kBoost><<<dim3(static_cast<unsigned>((A.Q + W - 1) / W)), 64 * W, 0, s>>>(A);
    return check_launch(kBoost ? "k_score_lists_long<boost>" : "k_score_lists_long");
}

// the two entry points: one argument check, the kernel instantiations by kBoost
template <bool kBoost>
int score_lists(const char* me, const float* Qn, int64_t Qvalid, const float* Cn, int64_t M, int32_t D,
                const int64_t* among_ptr, const int32_t* among_idx, const int64_t* among_row, int64_t among_rows,
                uint32_t* list_key, int32_t* list_idx, int32_t* list_n, int32_t cap, const float* boost,
                lgcn_stream_t stream) {
    if (kBoost && !boost) return fail(LGCN_E_ARG, "%s: boost is null", me);
    if (!Qn) return fail(LGCN_E_ARG, "%s: Qn is null", me);
    if (!Cn) return fail(LGCN_E_ARG, "%s: Cn is null", me);
    if (!among_ptr) return fail(LGCN_E_ARG, "%s: among_ptr is null", me);
    if (!among_idx) return fail(LGCN_E_ARG, "%s: among_idx is null", me);
    if (!list_key) return fail(LGCN_E_ARG, "%s: list_key is null", me);
    if (!list_idx) return fail(LGCN_E_ARG, "%s: list_idx is null", me);
    if (!list_n) return fail(LGCN_E_ARG, "%s: list_n is null", me);
    if (cap < 1) return fail(LGCN_E_ARG, "%s: cap=%d", me, cap);
    if (D != 8 && D != 16 && D != 32 && D != 64 && D != 128 && D != 256)
        return fail(LGCN_E_ARG, "%s: D=%d (use lgcn_recall_width)", me, D);
    if (Qvalid < 0 || Qvalid > INT32_MAX) return fail(LGCN_E_ARG, "%s: Qvalid=%lld", me, (long long)Qvalid);
    if (M < 0 || M > INT32_MAX) return fail(LGCN_E_ARG, "%s: M=%lld", me, (long long)M);
    if (among_rows < 0) return fail(LGCN_E_ARG, "%s: among_rows=%lld", me, (long long)among_rows);
    if (reinterpret_cast<uintptr_t>(Qn) % 16 != 0) return fail(LGCN_E_ARG, "%s: Qn is not 16-byte aligned", me);
    if (reinterpret_cast<uintptr_t>(Cn) % 16 != 0) return fail(LGCN_E_ARG, "%s: Cn is not 16-byte aligned", me);
    if (Qvalid == 0) return LGCN_OK;
    AmongKernelArgs<kBoost> A;
    static_cast<AmongArgs&>(A) = {Qn, Qvalid, Cn, M, among_ptr, among_idx, among_row, among_rows, list_key, list_idx,
                                  list_n, cap};
    if constexpr (kBoost) A.boost = boost;
    hipStream_t s = as_stream(stream);
    switch (D) {
        case 8: return launch_among<8, kBoost>(A, s);
        case 16: return launch_among<16, kBoost>(A, s);
        case 32: return launch_among<32, kBoost>(A, s);
        case 64: return launch_among<64, kBoost>(A, s);
        case 128: return launch_among<128, kBoost>(A, s);
        default: return launch_among<256, kBoost>(A, s);
    }
}

}  // namespace
