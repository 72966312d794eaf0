// Greedy Maximal Marginal Relevance re-ranking of per-query candidate pools on gfx950
// (lgcn_rerank_mmr): a pool of N (index, relevance) pairs per query plus the unit rows of the
// candidates in, the k picks of the greedy rule in pick order out, with each pick's summed
// similarity to the picks before it (what intra-list diversity is made of).
//
//   k_rerank_mmr   one wave per query, one query per 64-thread workgroup. The wave gathers the
//                  pool's N unit rows into LDS once (float4 loads, 16 bytes per lane, the rows of
//                  out-of-range pool entries never read), then runs the k dependent steps on LDS
//                  and registers: pool position p lives in lane p % 64, slot p / 64, which keeps
//                  its index, relevance, largest similarity m and similarity sum a in registers.
//                  A step forms each live position's value, takes the wave's argmax by a butterfly
//                  on one 64-bit word (ordered value image above, inverted position below: the
//                  larger word is the larger value, then the lower position), lets the winner's
//                  lane store the pick, and updates m and a of the others with one dot product
//                  against the winner's row: a row per lane, float4 reads of its own row and of
//                  the winner's (one address for the whole wave: a broadcast), the winner's read
//                  shared by the lane's slots.
//
// Why this shape. The work of a query is k dependent steps of N short dot products: too little to
// spread over waves that would have to meet at a barrier every step, and independent of every
// other query. So a query gets one wave and no synchronisation, and the CU is filled by queries:
// a 64-thread workgroup asks for N * (D + 4) * 4 + N * 4 bytes of LDS, so the 160 KiB of a CU hold
// five pools of 100 rows at D = 64 and one pool at the limit of 128 KiB of rows.
// LDS rows are D + 4 floats apart: row strides of D floats (a power of two) would put a row-per-
// lane read on one bank for all lanes; D / 4 + 1 sixteen-byte slots is odd, so the 16 lanes of a
// ds_read_b128 lane group fall on 16 different slots of the 64-bank row.
// No global atomics, no waiting on other workgroups, nothing allocated, stream-ordered. A pool
// above 64 KiB of LDS needs the kernel's dynamic-LDS attribute raised; the entry point does that
// (a host-side call, no synchronisation) before such a launch.
#include "lgcn_common.h"
#include "lgcn_ragged.h"

#include <cmath>

#pragma clang fp contract(off)

namespace lgcn {

constexpr int kMmrMaxSlots = LGCN_MMR_MAX_POOL / 64;
constexpr int kMmrRowPad = 4;  // floats between LDS rows beyond D (one 16-byte access width)

template <int SLOTS>
__global__ __launch_bounds__(64) void k_rerank_mmr(
    const int32_t* __restrict__ pool_idx, const float* __restrict__ pool_score, int64_t ld, int32_t N,
    const float* __restrict__ Cn, int64_t M, int32_t D, int32_t k, float delta, int32_t* __restrict__ out_idx,
    float* __restrict__ out_score, float* __restrict__ out_pair, int32_t* __restrict__ out_n) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int c4 = D >> 2;             // float4 per row
    const int rs4 = c4 + kMmrRowPad / 4;  // LDS row stride in float4
    float4* rows = reinterpret_cast<float4*>(smem);
    int32_t* sidx = reinterpret_cast<int32_t*>(smem + static_cast<size_t>(N) * rs4 * 16);

    // this lane's positions: index, relevance, and whether the entry is eligible (its row is staged)
    int32_t idx[SLOTS];
    float rel[SLOTS], mx[SLOTS], acc[SLOTS];
    uint32_t live = 0;  // bit j: slot j is eligible and not taken yet
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int p = j * 64 + lane;
        idx[j] = -1;
        rel[j] = 0.f;
        mx[j] = 0.f;
        acc[j] = 0.f;
        if (p < N) {
            idx[j] = pool_idx[q * ld + p];
            rel[j] = pool_score[q * ld + p];
            const bool ok = idx[j] >= 0 && static_cast<int64_t>(idx[j]) < M;
            if (ok) live |= 1u << j;
            sidx[p] = ok ? idx[j] : -1;
        }
    }
    __syncthreads();
    // gather the eligible rows: float4 e of the pool image is column e % c4 of position e / c4
    // (the wave takes 64 consecutive float4 per instruction), four loads in flight per lane
    {
        int p = lane / c4, c = lane % c4;
        const int dp = 64 / c4, dc = 64 % c4;
        auto fetch = [&](float4& v, int& at) {
            at = -1;
            v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < N) {
                const int32_t i = sidx[p];
                if (i >= 0) {
                    v = reinterpret_cast<const float4*>(Cn + static_cast<int64_t>(i) * D)[c];
                    at = p * rs4 + c;
                }
            }
            p += dp;
            c += dc;
            if (c >= c4) {
                c -= c4;
                ++p;
            }
        };
        while (p < N) {
            float4 v0, v1, v2, v3;
            int a0, a1, a2, a3;
            fetch(v0, a0);
            fetch(v1, a1);
            fetch(v2, a2);
            fetch(v3, a3);
            if (a0 >= 0) rows[a0] = v0;
            if (a1 >= 0) rows[a1] = v1;
            if (a2 >= 0) rows[a2] = v2;
            if (a3 >= 0) rows[a3] = v3;
        }
    }
    __syncthreads();

    const float keep = 1.f - delta;
    int32_t t = 0;
    for (; t < k; ++t) {
        // the lane's best live position (slots ascend in position: strict > keeps the lowest)
        unsigned long long best = 0ull;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            if (live >> j & 1u) {
                const float a = keep * rel[j];
                const float b = delta * mx[j];
                const float v = a - b;
                const unsigned long long w = static_cast<unsigned long long>(ordered_key_nan_last(v)) << 32 |
                                             (0xFFFFFFFFu - static_cast<uint32_t>(j * 64 + lane));
                best = w > best ? w : best;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o > best ? o : best;
        }
        if (best == 0ull) break;  // wave-uniform: no eligible position is left
        const int pw = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(best));
        const int wl = pw & 63, wj = pw >> 6;
        if (lane == wl) {
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                if (j == wj) {
                    out_idx[q * k + t] = idx[j];
                    out_score[q * k + t] = rel[j];
                    out_pair[q * k + t] = acc[j];
                    live &= ~(1u << j);
                }
            }
        }
        if (t + 1 == k) {  // the last pick: nobody reads m and a again
            ++t;
            break;
        }
        // similarity of every position to the pick (rows of ineligible or absent positions are
        // read clamped and dropped: their m and a are never used)
        float4 s4[SLOTS];
        int rowoff[SLOTS];
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            s4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int p = j * 64 + lane;
            rowoff[j] = ((live >> j & 1u) ? p : pw) * rs4;
        }
        const float4* wrow = rows + pw * rs4;
        for (int c = 0; c < c4; ++c) {
            const float4 w = wrow[c];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const float4 x = rows[rowoff[j] + c];
                s4[j].x += x.x * w.x;
                s4[j].y += x.y * w.y;
                s4[j].z += x.z * w.z;
                s4[j].w += x.w * w.w;
            }
        }
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            if (live >> j & 1u) {
                const float s = (s4[j].x + s4[j].y) + (s4[j].z + s4[j].w);
                mx[j] = t == 0 ? s : fmaxf(mx[j], s);
                acc[j] += s;
            }
        }
    }
    // slots nobody could fill
    for (int32_t u = t + lane; u < k; u += 64) {
        out_idx[q * k + u] = -1;
        out_score[q * k + u] = -INFINITY;
        out_pair[q * k + u] = 0.f;
    }
    if (lane == 0) out_n[q] = t;
}

}  // namespace lgcn

using namespace lgcn;

namespace {

template <int SLOTS>
int launch_mmr(const int32_t* pool_idx, const float* pool_score, int64_t ld, int32_t N, int64_t Q, const float* Cn,
               int64_t M, int32_t D, int32_t k, float diversity, int32_t* out_idx, float* out_score, float* out_pair,
               int32_t* out_n, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024) {  // above the default dynamic-LDS ceiling: raise it (host-side, no synchronisation)
        int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rerank_mmr<SLOTS>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)),
                           "lgcn_rerank_mmr: hipFuncSetAttribute");
        if (rc != LGCN_OK) return rc;
    }
    k_rerank_mmr<SLOTS><<<dim3(static_cast<unsigned>(Q)), 64, lds, s>>>(pool_idx, pool_score, ld, N, Cn, M, D, k,
                                                                       diversity, out_idx, out_score, out_pair, out_n);
    return check_launch("k_rerank_mmr");
}

}  // namespace

extern "C" {

int lgcn_rerank_mmr(const int32_t* pool_idx, const float* pool_score, int64_t ld, int32_t N, int64_t Q,
                    const float* Cn, int64_t M, int32_t D, int32_t k, float diversity, int32_t* out_idx,
                    float* out_score, float* out_pair, int32_t* out_n, lgcn_stream_t stream) {
    const char* me = "lgcn_rerank_mmr";
    if (!pool_idx) return fail(LGCN_E_ARG, "%s: pool_idx is null", me);
    if (!pool_score) return fail(LGCN_E_ARG, "%s: pool_score is null", me);
    if (!Cn) return fail(LGCN_E_ARG, "%s: Cn is null", me);
    if (!out_idx) return fail(LGCN_E_ARG, "%s: out_idx is null", me);
    if (!out_score) return fail(LGCN_E_ARG, "%s: out_score is null", me);
    if (!out_pair) return fail(LGCN_E_ARG, "%s: out_pair is null", me);
    if (!out_n) return fail(LGCN_E_ARG, "%s: out_n is null", me);
    if (k < 1 || k > N) return fail(LGCN_E_ARG, "%s: k=%d outside [1, N=%d]", me, k, N);
    if (ld < N) return fail(LGCN_E_ARG, "%s: ld=%lld < N=%d", me, (long long)ld, N);
    if (Q < 0) return fail(LGCN_E_ARG, "%s: Q=%lld", me, (long long)Q);
    if (M < 0) return fail(LGCN_E_ARG, "%s: M=%lld", me, (long long)M);
    if (D < 1) return fail(LGCN_E_ARG, "%s: D=%d", me, D);
    if (D % 4 != 0) return fail(LGCN_E_ARG, "%s: D=%d is not a multiple of 4 (use lgcn_recall_width)", me, D);
    if (reinterpret_cast<uintptr_t>(Cn) % 16 != 0) return fail(LGCN_E_ARG, "%s: Cn is not 16-byte aligned", me);
    if (!(diversity >= 0.f && diversity <= 1.f))
        return fail(LGCN_E_ARG, "%s: diversity=%g outside [0, 1]", me, static_cast<double>(diversity));
    if (N > LGCN_MMR_MAX_POOL)
        return fail(LGCN_E_UNSUPPORTED, "%s: N=%d exceeds LGCN_MMR_MAX_POOL=%d", me, N, LGCN_MMR_MAX_POOL);
    if (static_cast<int64_t>(N) * D * 4 > LGCN_MMR_MAX_LDS_BYTES)
        return fail(LGCN_E_UNSUPPORTED, "%s: N * D * 4 = %lld bytes of pool rows exceed LGCN_MMR_MAX_LDS_BYTES=%d", me,
                    (long long)N * D * 4, LGCN_MMR_MAX_LDS_BYTES);
    if (Q > INT32_MAX) return fail(LGCN_E_ARG, "%s: Q=%lld is too many queries for one launch", me, (long long)Q);
    if (Q == 0) return LGCN_OK;
    const size_t lds = static_cast<size_t>(N) * (D + kMmrRowPad) * 4 + static_cast<size_t>(N) * 4;
    hipStream_t s = as_stream(stream);
    const int slots = (N + 63) / 64;
#define LGCN_MMR_ARGS pool_idx, pool_score, ld, N, Q, Cn, M, D, k, diversity, out_idx, out_score, out_pair, out_n, lds, s
    if (slots <= 1) return launch_mmr<1>(LGCN_MMR_ARGS);
    if (slots <= 2) return launch_mmr<2>(LGCN_MMR_ARGS);
    if (slots <= 4) return launch_mmr<4>(LGCN_MMR_ARGS);
    static_assert(kMmrMaxSlots == 8, "the slot dispatch below covers pools of up to 512 entries");
    return launch_mmr<8>(LGCN_MMR_ARGS);
#undef LGCN_MMR_ARGS
}

}  // extern "C"
