// BPR negatives on gfx950 (lgcn_sample_negatives): per triplet one item the user has no train edge
// to, drawn exactly uniformly over the unseen items without rejection, or the hardest (highest
// cosine) of n such draws. The draw is a counter hash of (seed, step, the triplet's global index,
// the candidate's number), spelled out in include/lgcn.h, so the same triplet gets the same
// negative whatever the batch it arrives in, the launch geometry or the run.
//
//   neg_candidate    candidate j of a triplet: r = umul64hi(hash, m) over the m = I - c items that
//                    are not in the user's ascending row s[0 .. c), mapped to the r-th unseen item
//                    by one binary search: s[p] - p is non-decreasing, t = #{p : s[p] - p <= r}
//                    entries of the row lie below the answer, the item is r + t.
//   k_neg_uniform    n = 1: one thread per triplet, integers only.
//   k_neg_hardest    n > 1: a 16-lane group per triplet, four triplets per wave, 16 per workgroup.
//                    Lanes 0 .. n-1 of a group draw the candidates (lane l also draws l + 16 when
//                    n > 16) and broadcast them. A row of d columns is read as float4 per lane,
//                    64 columns per pass; a pass issues the user's chunk and the chunks of all NB
//                    candidate rows of a batch (NB = pow2 >= n, at most 16; n > 16 takes two
//                    batches) before it uses any: the gathers wait for one memory round trip, not
//                    for NB in a row. Dot and candidate norm come from the same pass, reduced by an
//                    exchange butterfly over the 16 lanes (a fixed tree, the same bits on every
//                    lane), and the pick is one 64-bit max of (score key, n - 1 - j): the highest
//                    score, the lowest j among equals.
//
// The summation order is a function of d alone. No value of users reads out of bounds: the row of a
// user outside the CSR is empty, a user outside [0, U) reads no table row, and every candidate is
// in [0, I). The two stats counters get one atomic add per workgroup (none when it counts
// nothing); there are no other atomics, no workspace, and plain vector stores only.
#include "lgcn_common.h"
#include "lgcn_ragged.h"

#include <cmath>

#pragma clang fp contract(off)

namespace lgcn {

constexpr uint64_t kNegGolden = 0x9E3779B97F4A7C15ull;
constexpr int kNegGroup = 16;                 // lanes of a triplet
constexpr int kNegPerBlock = 256 / kNegGroup; // triplets of a k_neg_hardest workgroup

__host__ __device__ __forceinline__ uint64_t neg_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// what a triplet's candidates are drawn from: its hash and its user's row of the seen CSR
struct NegDraw {
    uint64_t h1;
    const int32_t* row;
    int64_t c, m;
};

__device__ __forceinline__ NegDraw neg_draw(uint64_t h0, int64_t b_global, int64_t b,
                                            const int64_t* __restrict__ users,
                                            const int64_t* __restrict__ seen_ptr,
                                            const int32_t* __restrict__ seen_idx, int64_t seen_rows, int64_t I) {
    NegDraw D;
    D.h1 = neg_mix(h0 ^ static_cast<uint64_t>(b_global));
    int64_t beg = 0, end = 0;
    if (seen_ptr) ragged_row(b, seen_ptr, users, seen_rows, beg, end);
    D.row = seen_idx + beg;
    D.c = end - beg;
    D.m = I - D.c;
    return D;
}

// candidate j: the r-th item outside the row, or any item when the row leaves none (m <= 0)
__device__ __forceinline__ int32_t neg_candidate(const NegDraw& D, int j, int64_t I) {
    const uint64_t h2 = neg_mix(D.h1 + kNegGolden * static_cast<uint64_t>(j + 1));
    if (D.m <= 0) return static_cast<int32_t>(__umul64hi(h2, static_cast<uint64_t>(I)));
    const int64_t r = static_cast<int64_t>(__umul64hi(h2, static_cast<uint64_t>(D.m)));
    int64_t lo = 0, hi = D.c;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (static_cast<int64_t>(D.row[mid]) - mid <= r) lo = mid + 1;
        else hi = mid;
    }
    return static_cast<int32_t>(r + lo);  // below I <= INT32_MAX: r < m and lo <= c
}

// stats[i] += the workgroup's count of threads with flag[i] set: one atomic per counter, none for 0.
// Every thread of the workgroup calls it.
__device__ __forceinline__ void neg_count(bool f0, bool f1, int64_t* __restrict__ stats) {
    __shared__ int32_t part[4][2];
    const int wv = threadIdx.x >> 6;
    const int n0 = __popcll(__ballot(f0)), n1 = __popcll(__ballot(f1));
    if ((threadIdx.x & 63) == 0) {
        part[wv][0] = n0;
        part[wv][1] = n1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int32_t s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + threadIdx.x, static_cast<unsigned long long>(s));
    }
}

__global__ __launch_bounds__(256) void k_neg_uniform(const int64_t* __restrict__ users, int64_t B, int64_t first,
                                                     const int64_t* __restrict__ seen_ptr,
                                                     const int32_t* __restrict__ seen_idx, int64_t seen_rows,
                                                     int64_t I, uint64_t h0, int64_t* __restrict__ out,
                                                     float* __restrict__ out_score, int64_t* __restrict__ stats) {
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    bool all_seen = false;
    if (b < B) {
        const NegDraw D = neg_draw(h0, first + b, b, users, seen_ptr, seen_idx, seen_rows, I);
        all_seen = D.m <= 0;
        out[b] = neg_candidate(D, 0, I);
        if (out_score) out_score[b] = 0.f;
    }
    neg_count(all_seen, false, stats);
}

struct NegTables {
    const float* user_rows;
    const float* item_rows;
    int64_t U, ldu, ldi;
    int32_t d;
};

template <int NB>
__global__ __launch_bounds__(256) void k_neg_hardest(const int64_t* __restrict__ users, int64_t B, int64_t first,
                                                     const int64_t* __restrict__ seen_ptr,
                                                     const int32_t* __restrict__ seen_idx, int64_t seen_rows,
                                                     int64_t I, uint64_t h0, int n, NegTables T,
                                                     int64_t* __restrict__ out, float* __restrict__ out_score,
                                                     int64_t* __restrict__ stats) {
    const int lane = threadIdx.x & 63, l = lane & (kNegGroup - 1), base = lane & ~(kNegGroup - 1);
    const int64_t slot = static_cast<int64_t>(blockIdx.x) * kNegPerBlock + (threadIdx.x >> 4);
    const bool live = slot < B;
    const int64_t b = live ? slot : B - 1;  // a group past the end repeats the last triplet and stores nothing
    const NegDraw D = neg_draw(h0, first + b, b, users, seen_ptr, seen_idx, seen_rows, I);
    const int64_t u = users[b];
    const bool has_user = u >= 0 && u < T.U;
    // this lane's draws: candidate l, and l + 16 when there are that many
    const int32_t mine0 = l < n ? neg_candidate(D, l, I) : 0;
    const int32_t mine1 = l + kNegGroup < n ? neg_candidate(D, l + kNegGroup, I) : 0;
    const int32_t cand0 = __shfl(mine0, base, 64);

    uint64_t best = 0;  // (ordered_key_nan_last(score) << 32) | (n - 1 - j): never 0 for a candidate
    float best_score = 0.f;
    if (has_user) {  // uniform over the group; the shuffles below stay inside it
        const float* urow = T.user_rows + u * T.ldu;
        for (int j0 = 0; j0 < n; j0 += NB) {  // workgroup-uniform
            int32_t cand[NB];
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                const int32_t c = __shfl(j0 == 0 ? mine0 : mine1, base | (jj & (kNegGroup - 1)), 64);
                cand[jj] = j0 + jj < n ? c : cand0;  // a slot past n reads candidate 0's row and is not ranked
            }
            float dot[NB], nn[NB], uu = 0.f;
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) dot[jj] = nn[jj] = 0.f;
            for (int k0 = 0; k0 < T.d; k0 += 4 * kNegGroup) {  // workgroup-uniform
                const bool on = k0 + 4 * l < T.d;
                const int c0 = on ? k0 + 4 * l : 0;  // a lane past the row reads its first columns and drops them
                const float4 uv = *reinterpret_cast<const float4*>(urow + c0);
                float4 v[NB];
#pragma unroll
                for (int jj = 0; jj < NB; ++jj)
                    v[jj] = *reinterpret_cast<const float4*>(T.item_rows + static_cast<int64_t>(cand[jj]) * T.ldi + c0);
                if (on) {
                    uu += uv.x * uv.x + uv.y * uv.y + uv.z * uv.z + uv.w * uv.w;
#pragma unroll
                    for (int jj = 0; jj < NB; ++jj) {
                        dot[jj] += uv.x * v[jj].x + uv.y * v[jj].y + uv.z * v[jj].z + uv.w * v[jj].w;
                        nn[jj] += v[jj].x * v[jj].x + v[jj].y * v[jj].y + v[jj].z * v[jj].z + v[jj].w * v[jj].w;
                    }
                }
            }
            for (int off = kNegGroup >> 1; off > 0; off >>= 1) {
                uu += __shfl_xor(uu, off, 64);
#pragma unroll
                for (int jj = 0; jj < NB; ++jj) {
                    dot[jj] += __shfl_xor(dot[jj], off, 64);
                    nn[jj] += __shfl_xor(nn[jj], off, 64);
                }
            }
            const float un = sqrtf(uu);
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                if (j0 + jj < n) {
                    // 0 / 0 for a zero row: NaN, ranked as -inf
                    const float score = dot[jj] / (un * sqrtf(nn[jj]));
                    const uint64_t key = (static_cast<uint64_t>(ordered_key_nan_last(score)) << 32) |
                                         static_cast<uint32_t>(n - 1 - (j0 + jj));
                    if (key > best) {
                        best = key;
                        best_score = score;
                    }
                }
            }
        }
    }
    int32_t pick = cand0;
    float score = NAN;  // no user row, no cosine
    if (has_user) {
        const int j = n - 1 - static_cast<int>(best & 0xFFFFFFFFu);  // the same on every lane of the group
        pick = __shfl(j < kNegGroup ? mine0 : mine1, base | (j & (kNegGroup - 1)), 64);
        score = best_score;
    }
    if (live && l == 0) {
        out[slot] = pick;
        if (out_score) out_score[slot] = score;
    }
    neg_count(live && l == 0 && D.m <= 0, live && l == 0 && !has_user, stats);
}

}  // namespace lgcn

using namespace lgcn;

namespace {

template <int NB>
int launch_hardest(const int64_t* users, int64_t B, int64_t first, const int64_t* seen_ptr, const int32_t* seen_idx,
                   int64_t seen_rows, int64_t I, uint64_t h0, int n, const NegTables& T, int64_t* out,
                   float* out_score, int64_t* stats, hipStream_t s) {
    const unsigned groups = static_cast<unsigned>((B + kNegPerBlock - 1) / kNegPerBlock);
    k_neg_hardest<NB><<<dim3(groups), 256, 0, s>>>(users, B, first, seen_ptr, seen_idx, seen_rows, I, h0, n, T, out,
                                                  out_score, stats);
    return check_launch("k_neg_hardest");
}

}  // namespace

extern "C" {

int lgcn_sample_negatives(const int64_t* users, int64_t B, int64_t first, const int64_t* seen_ptr,
                          const int32_t* seen_idx, int64_t seen_rows, int64_t I, uint64_t seed, int64_t step,
                          int32_t n, const float* user_rows, int64_t ldu, int64_t U, const float* item_rows,
                          int64_t ldi, int32_t d, int64_t* out, float* out_score, int64_t* stats,
                          lgcn_stream_t stream) {
    const char* me = "lgcn_sample_negatives";
    if (B < 0) return fail(LGCN_E_ARG, "%s: B=%lld", me, (long long)B);
    if (B > INT32_MAX) return fail(LGCN_E_ARG, "%s: B=%lld is too many triplets for one launch", me, (long long)B);
    if (first < 0) return fail(LGCN_E_ARG, "%s: first=%lld", me, (long long)first);
    if (I < 1 || I > INT32_MAX) return fail(LGCN_E_ARG, "%s: I=%lld", me, (long long)I);
    if (seen_rows < 0) return fail(LGCN_E_ARG, "%s: seen_rows=%lld", me, (long long)seen_rows);
    if (n < 1) return fail(LGCN_E_ARG, "%s: n=%d", me, n);
    if (n > LGCN_NEGATIVES_MAX_N)
        return fail(LGCN_E_UNSUPPORTED, "%s: n=%d exceeds LGCN_NEGATIVES_MAX_N=%d", me, n, LGCN_NEGATIVES_MAX_N);
    if (!users) return fail(LGCN_E_ARG, "%s: users is null", me);
    if (!out) return fail(LGCN_E_ARG, "%s: out is null", me);
    if (!stats) return fail(LGCN_E_ARG, "%s: stats is null", me);
    if ((seen_ptr == nullptr) != (seen_idx == nullptr))
        return fail(LGCN_E_ARG, "%s: seen_ptr and seen_idx are both null (nothing excluded) or neither", me);
    NegTables T;
    T.user_rows = user_rows;
    T.item_rows = item_rows;
    T.U = U;
    T.ldu = ldu;
    T.ldi = ldi;
    T.d = d;
    if (n > 1) {
        if (!user_rows) return fail(LGCN_E_ARG, "%s: user_rows is null (n=%d)", me, n);
        if (!item_rows) return fail(LGCN_E_ARG, "%s: item_rows is null (n=%d)", me, n);
        if (U < 0) return fail(LGCN_E_ARG, "%s: U=%lld", me, (long long)U);
        if (d < 4 || d % 4 != 0) return fail(LGCN_E_ARG, "%s: d=%d is no positive multiple of 4", me, d);
        if (d > LGCN_NEGATIVES_MAX_D)
            return fail(LGCN_E_UNSUPPORTED, "%s: d=%d exceeds LGCN_NEGATIVES_MAX_D=%d", me, d, LGCN_NEGATIVES_MAX_D);
        if (ldu < d || ldu % 4 != 0 || ldu > INT32_MAX)
            return fail(LGCN_E_ARG, "%s: ldu=%lld is no stride of 16-byte aligned rows of d=%d", me, (long long)ldu, d);
        if (ldi < d || ldi % 4 != 0 || ldi > INT32_MAX)
            return fail(LGCN_E_ARG, "%s: ldi=%lld is no stride of 16-byte aligned rows of d=%d", me, (long long)ldi, d);
        if (reinterpret_cast<uintptr_t>(user_rows) % 16 != 0 || reinterpret_cast<uintptr_t>(item_rows) % 16 != 0)
            return fail(LGCN_E_ARG, "%s: the tables are not 16-byte aligned", me);
    }
    if (B == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
    const uint64_t h0 = neg_mix(seed + kNegGolden * (static_cast<uint64_t>(step) + 1));
    if (n == 1) {
        k_neg_uniform<<<dim3(static_cast<unsigned>((B + 255) / 256)), 256, 0, s>>>(
            users, B, first, seen_ptr, seen_idx, seen_rows, I, h0, out, out_score, stats);
        return check_launch("k_neg_uniform");
    }
#define LGCN_NEG_LAUNCH(NB)                                                                                         \
    return launch_hardest<NB>(users, B, first, seen_ptr, seen_idx, seen_rows, I, h0, n, T, out, out_score, stats, s)
    if (n <= 2) LGCN_NEG_LAUNCH(2);
    if (n <= 4) LGCN_NEG_LAUNCH(4);
    if (n <= 8) LGCN_NEG_LAUNCH(8);
    LGCN_NEG_LAUNCH(16);
#undef LGCN_NEG_LAUNCH
}

}  // extern "C"
