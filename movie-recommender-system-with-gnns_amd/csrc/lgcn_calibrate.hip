// Calibrated re-ranking on gfx950 (Steck, RecSys 2018): lists that keep the genre mix of the user's
// own history. Genres are the 32 bits of a candidate's attribute word; an item's own distribution is
// uniform over its set bits, b(g|i) = [bit g of attr[i]] / popcount(attr[i]).
//
//   lgcn_attr_profile        per query a history row of a CSR in, the weighted mean of its items'
//                            distributions out (the target p [32]) with the weight it was formed from.
//   lgcn_rerank_calibrated   per query a pool of N (index, relevance) pairs and a target in, the k
//                            greedy picks of (1 - lambda) * relevance - lambda * KL(p || q~(list)) out.
//
// The profile. A lane owns one genre and one half of the entries: lane l sums genre l % 32 over the
// entries of parity l / 32 within each 64-entry block, in float64, so nothing is added atomically and
// the order of a sum follows from the entry's position in its row alone. A step loads kProfileDepth
// entries per lane (index and weight, then every attr gather of the step before the first is used),
// reduces each to (word, w / popcount in float64) and passes them round the wave: 32 rounds per
// 64-entry block, each lane taking the entry of its parity and adding its value when the word has the
// lane's bit (adding +0.0 otherwise: exact). The two halves meet in one exchange, the weights in a
// butterfly, and p = sum / W is rounded to f32 once.
//   k_attr_profile        one wave per history of at most kProfileLong entries, four per workgroup.
//   k_attr_profile_long   a 512-thread workgroup per eight consecutive queries, for those among them
//                         with a longer history: wave w sums the chunks w, w + 8, ... of
//                         kProfileChunk entries, wave 0 adds the eight sums in wave order through LDS.
//
// The re-rank. One wave per query, one query per 64-thread workgroup; pool position p lives in lane
// p % 64, slot p / 64, which keeps its index, relevance and attribute word in registers (16 slots at
// the limit of 1024). The state is mass_g (float64, lane g % 32 holds genre g in both half-waves: the
// sum of b(g|i) over the picks stays exact to 2^-53 over 1024 picks) and m, the picks with a word.
// A step:
//   1. every lane forms, for its genre, q~_g of the state with one more counted pick and nothing
//      added to the genre ((1 - alpha) * mass_g / (m + 1) + alpha * p_g), its log L_g and the term
//      p_g * (ln p_g - L_g); a half-wave butterfly sums the terms to `base` (the same bits in both
//      halves), and p_g, mass_g and L_g go to a 512-byte LDS table.
//   2. a live position with word w corrects only its own genres:
//        KL(picks + c) = base + sum_{g in w, p_g > 0} p_g * (L_g - ln q~'_g),
//        q~'_g = (1 - alpha) * ((mass_g + 1 / popcount(w)) / (m + 1)) + alpha * p_g,
//      one table read and one log per set bit (1 to 3 on MovieLens, against 32 logs for the naive
//      form); a position without a word leaves the list's distribution as it is and keeps the KL of
//      the pick before it, bit for bit (before the first pick: base, whose divisor is then 1). The
//      value is a function of (relevance bits, word, state) and of nothing else: two positions equal
//      in both tie at every step.
//   3. the argmax is one butterfly on a 64-bit word (ordered value image above, inverted position
//      below), the winner's lane stores the pick with its KL, its word travels to all lanes, and the
//      lanes whose genre it names add 1 / popcount to their mass.
// logf is the library's (within an ulp), never the fast intrinsic: tests/calibrate_checker.py holds
// every value and KL to 64 * 2^-24 of their scale. No global atomics, no waiting on other workgroups,
// nothing allocated, stream-ordered.
#include "lgcn_common.h"
#include "lgcn_ragged.h"

#include <cmath>

#pragma clang fp contract(off)

namespace lgcn {

static_assert(LGCN_CALIB_GENRES == 32, "a genre is a bit of the 32-bit attribute word and a lane of a half-wave");

constexpr int kProfileWaves = 8;                   // waves that share a long history
constexpr int kProfileLong = LGCN_PROFILE_LONG;    // history entries above which they do
constexpr int kProfileChunk = LGCN_PROFILE_CHUNK;  // entries of a chunk of a long history
constexpr int kProfileDepth = 4;                   // entries a lane has in flight
constexpr int kProfileShort = 4;                   // histories (waves) per workgroup of k_attr_profile

static_assert(kProfileChunk % (64 * kProfileDepth) == 0, "a chunk is whole steps: lane and parity follow the row position");

// Adds this lane's share of the entries [beg, end) to acc (genre lane % 32 over the entries of parity
// lane / 32 within each 64-entry block, ascending) and the weights of the entries the lane itself
// loaded to wsum. An entry counts when 0 <= i < M, attr[i] != 0 and its weight is > 0 (a NaN is not).
__device__ __forceinline__ void profile_sum(const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w,
                                            const uint32_t* __restrict__ attr, int64_t M, int64_t beg, int64_t end,
                                            int lane, double& acc, double& wsum) {
    const int g = lane & 31, h = lane >> 5;
    for (int64_t e0 = beg; e0 < end; e0 += 64 * kProfileDepth) {  // wave-uniform
        int32_t it[kProfileDepth];
        float w[kProfileDepth];
        bool ok[kProfileDepth];
        uint32_t word[kProfileDepth];
#pragma unroll
        for (int u = 0; u < kProfileDepth; ++u) {  // a clamped position: the loads need no branch
            const int64_t e = e0 + u * 64 + lane;
            const int64_t ec = e < end ? e : end - 1;
            it[u] = hist_idx[ec];
            w[u] = hist_w ? hist_w[ec] : 1.f;
            ok[u] = e < end;
        }
#pragma unroll
        for (int u = 0; u < kProfileDepth; ++u) {  // every gather of the step before the first is used
            ok[u] = ok[u] && it[u] >= 0 && static_cast<int64_t>(it[u]) < M && w[u] > 0.f;
            word[u] = ok[u] ? attr[it[u]] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kProfileDepth; ++u) {
            if (e0 + u * 64 >= end) break;  // wave-uniform
            double c = 0.0;
            if (word[u] != 0u) {
                const double wd = static_cast<double>(w[u]);
                c = wd / static_cast<double>(__popc(word[u]));
                wsum += wd;
            }
            for (int j = 0; j < 32; ++j) {
                const int src = 2 * j + h;
                const uint32_t wj = __shfl(word[u], src, 64);
                const double cj = __shfl(c, src, 64);
                acc += (wj >> g & 1u) ? cj : 0.0;
            }
        }
    }
}

// the two halves' sums of a genre and the lanes' weights, combined: the same bits on every lane
__device__ __forceinline__ void profile_combine(double& acc, double& wsum) {
    acc += __shfl_xor(acc, 32, 64);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) wsum += __shfl_xor(wsum, off, 64);
}

__device__ __forceinline__ void profile_store(int64_t q, int lane, double acc, double W, float* __restrict__ out_p,
                                              float* __restrict__ out_w) {
    if (lane < 32) out_p[q * 32 + lane] = W > 0.0 ? static_cast<float>(acc / W) : 0.f;
    if (lane == 0) out_w[q] = W > 0.0 ? static_cast<float>(W) : 0.f;
}

__global__ __launch_bounds__(64 * kProfileShort) void k_attr_profile(
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w,
    const int64_t* __restrict__ hist_row, int64_t hist_rows, int64_t Q, const uint32_t* __restrict__ attr, int64_t M,
    float* __restrict__ out_p, float* __restrict__ out_w) {
    const int lane = threadIdx.x & 63;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kProfileShort + (threadIdx.x >> 6);
    if (q >= Q) return;  // wave-uniform, and no barrier follows
    int64_t beg, end;
    ragged_row(q, hist_ptr, hist_row, hist_rows, beg, end);
    if (end - beg > kProfileLong) return;  // k_attr_profile_long's
    double acc = 0.0, wsum = 0.0;
    profile_sum(hist_idx, hist_w, attr, M, beg, end, lane, acc, wsum);
    profile_combine(acc, wsum);
    profile_store(q, lane, acc, wsum, out_p, out_w);
}

__global__ __launch_bounds__(64 * kProfileWaves) void k_attr_profile_long(
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w,
    const int64_t* __restrict__ hist_row, int64_t hist_rows, int64_t Q, const uint32_t* __restrict__ attr, int64_t M,
    float* __restrict__ out_p, float* __restrict__ out_w) {
    __shared__ double part[kProfileWaves - 1][32];
    __shared__ double pw[kProfileWaves - 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = 0; i < kProfileWaves; ++i) {  // workgroup-uniform throughout
        const int64_t q = static_cast<int64_t>(blockIdx.x) * kProfileWaves + i;
        if (q >= Q) break;
        int64_t beg, end;
        ragged_row(q, hist_ptr, hist_row, hist_rows, beg, end);
        if (end - beg <= kProfileLong) continue;
        double acc = 0.0, wsum = 0.0;
        for (int64_t b = beg + static_cast<int64_t>(wv) * kProfileChunk; b < end;
             b += static_cast<int64_t>(kProfileWaves) * kProfileChunk) {
            const int64_t e = b + kProfileChunk < end ? b + kProfileChunk : end;
            profile_sum(hist_idx, hist_w, attr, M, b, e, lane, acc, wsum);
        }
        profile_combine(acc, wsum);
        __syncthreads();  // the workgroup's previous long history is done with the LDS
        if (wv > 0) {
            if (lane < 32) part[wv - 1][lane] = acc;
            if (lane == 0) pw[wv - 1] = wsum;
        }
        __syncthreads();
        if (wv == 0) {
            for (int w = 0; w < kProfileWaves - 1; ++w) {
                acc += part[w][lane & 31];
                wsum += pw[w];
            }
            profile_store(q, lane, acc, wsum, out_p, out_w);
        }
    }
}

constexpr int kCalibMaxSlots = LGCN_CALIB_MAX_POOL / 64;

template <int SLOTS>
__global__ __launch_bounds__(64) void k_rerank_calibrated(
    const int32_t* __restrict__ pool_idx, const float* __restrict__ pool_score, int64_t ld, int32_t N,
    const uint32_t* __restrict__ attr, int64_t M, const float* __restrict__ target, int32_t k, float lambda,
    float alpha, int32_t* __restrict__ out_idx, float* __restrict__ out_score, float* __restrict__ out_kl,
    int32_t* __restrict__ out_n) {
    __shared__ float4 tab[32];  // per genre: p_g (0 when it is not > 0), mass_g, L_g = ln q~_g of the base state
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int g = lane & 31;

    // this lane's positions: index, relevance, word (0 for an ineligible entry, whose attr is never read)
    int32_t idx[SLOTS];
    float rel[SLOTS];
    uint32_t word[SLOTS];
    uint32_t live = 0;  // bit j: slot j is eligible and not taken yet
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const int p = j * 64 + lane;
        idx[j] = -1;
        rel[j] = 0.f;
        word[j] = 0u;
        if (p < N) {
            idx[j] = pool_idx[q * ld + p];
            rel[j] = pool_score[q * ld + p];
            if (idx[j] >= 0 && static_cast<int64_t>(idx[j]) < M) {
                live |= 1u << j;
                word[j] = attr[idx[j]];
            }
        }
    }
    const float pg = target[q * 32 + g];
    const bool pos = pg > 0.f;  // a NaN is not
    const float lnp = pos ? logf(pg) : 0.f;
    const float ap = alpha * pg;
    const float oma = 1.f - alpha, oml = 1.f - lambda;
    double mass = 0.0;  // of genre g, the same in both half-waves
    int32_t m = 0;      // picks with a non-zero word
    float klprev = 0.f;  // the KL of the list as it is: the last pick's

    int32_t t = 0;
    for (; t < k; ++t) {
        const float den1 = static_cast<float>(m + 1);
        const float mf = static_cast<float>(mass);
        const float qb = mf / den1;
        const float qt = oma * qb + ap;
        const float L = pos ? logf(qt) : 0.f;
        float T = pos ? pg * (lnp - L) : 0.f;
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) T += __shfl_xor(T, off, 64);
        const float base = T;
        if (t == 0) klprev = base;  // no pick yet: m + 1 == max(1, m)
        __syncthreads();  // the previous step's readers are done with the table
        if (lane < 32) tab[g] = make_float4(pos ? pg : 0.f, mf, L, 0.f);
        __syncthreads();

        // the lane's best live position (slots ascend in position: strict > keeps the lowest)
        unsigned long long best = 0ull;
        float bestkl = 0.f;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            if (live >> j & 1u) {
                float kl = klprev;
                uint32_t w = word[j];
                if (w != 0u) {
                    const float inv = 1.f / static_cast<float>(__popc(w));
                    float corr = 0.f;
                    while (w != 0u) {
                        const int b = __ffs(w) - 1;
                        w &= w - 1u;
                        const float4 e = tab[b];
                        if (e.x > 0.f) {
                            const float s = e.y + inv;
                            const float qn = s / den1;
                            const float x = oma * qn;
                            const float y = alpha * e.x;
                            const float d = e.z - logf(x + y);
                            corr += e.x * d;
                        }
                    }
                    kl = base + corr;
                }
                const float a = oml * rel[j];
                const float c = lambda * kl;
                const float v = a - c;
                const unsigned long long key = static_cast<unsigned long long>(ordered_key_nan_last(v)) << 32 |
                                               (0xFFFFFFFFu - static_cast<uint32_t>(j * 64 + lane));
                if (key > best) {
                    best = key;
                    bestkl = kl;
                }
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
        uint32_t ww = 0u;
        if (lane == wl) {
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                if (j == wj) {
                    out_idx[q * k + t] = idx[j];
                    out_score[q * k + t] = rel[j];
                    out_kl[q * k + t] = bestkl;
                    live &= ~(1u << j);
                    ww = word[j];
                }
            }
        }
        ww = __shfl(ww, wl, 64);
        klprev = __shfl(bestkl, wl, 64);
        if (ww != 0u) {  // wave-uniform
            ++m;
            if (ww >> g & 1u) mass += 1.0 / static_cast<double>(__popc(ww));
        }
    }
    // slots nobody could fill
    for (int32_t u = t + lane; u < k; u += 64) {
        out_idx[q * k + u] = -1;
        out_score[q * k + u] = -INFINITY;
        out_kl[q * k + u] = 0.f;
    }
    if (lane == 0) out_n[q] = t;
}

}  // namespace lgcn

using namespace lgcn;

namespace {

template <int SLOTS>
int launch_calibrated(const int32_t* pool_idx, const float* pool_score, int64_t ld, int32_t N, int64_t Q,
                      const uint32_t* attr, int64_t M, const float* target, int32_t k, float lambda, float alpha,
                      int32_t* out_idx, float* out_score, float* out_kl, int32_t* out_n, hipStream_t s) {
    k_rerank_calibrated<SLOTS><<<dim3(static_cast<unsigned>(Q)), 64, 0, s>>>(
        pool_idx, pool_score, ld, N, attr, M, target, k, lambda, alpha, out_idx, out_score, out_kl, out_n);
    return check_launch("k_rerank_calibrated");
}

}  // namespace

extern "C" {

int lgcn_attr_profile(const int64_t* hist_ptr, const int32_t* hist_idx, const float* hist_w, const int64_t* hist_row,
                      int64_t hist_rows, int64_t Q, const uint32_t* attr, int64_t M, float* out_p, float* out_w,
                      lgcn_stream_t stream) {
    const char* me = "lgcn_attr_profile";
    if (!hist_ptr) return fail(LGCN_E_ARG, "%s: hist_ptr is null", me);
    if (!hist_idx) return fail(LGCN_E_ARG, "%s: hist_idx is null", me);
    if (!attr) return fail(LGCN_E_ARG, "%s: attr is null", me);
    if (!out_p) return fail(LGCN_E_ARG, "%s: out_p is null", me);
    if (!out_w) return fail(LGCN_E_ARG, "%s: out_w is null", me);
    if (Q < 0) return fail(LGCN_E_ARG, "%s: Q=%lld", me, (long long)Q);
    if (M < 0) return fail(LGCN_E_ARG, "%s: M=%lld", me, (long long)M);
    if (hist_rows < 0) return fail(LGCN_E_ARG, "%s: hist_rows=%lld", me, (long long)hist_rows);
    if (Q > INT32_MAX) return fail(LGCN_E_ARG, "%s: Q=%lld is too many queries for one launch", me, (long long)Q);
    if (Q == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
    const unsigned short_groups = static_cast<unsigned>((Q + kProfileShort - 1) / kProfileShort);
    k_attr_profile<<<dim3(short_groups), 64 * kProfileShort, 0, s>>>(hist_ptr, hist_idx, hist_w, hist_row, hist_rows, Q,
                                                                    attr, M, out_p, out_w);
    int rc = check_launch("k_attr_profile");
    if (rc != LGCN_OK) return rc;
    const unsigned long_groups = static_cast<unsigned>((Q + kProfileWaves - 1) / kProfileWaves);
    k_attr_profile_long<<<dim3(long_groups), 64 * kProfileWaves, 0, s>>>(hist_ptr, hist_idx, hist_w, hist_row,
                                                                        hist_rows, Q, attr, M, out_p, out_w);
    return check_launch("k_attr_profile_long");
}

int lgcn_rerank_calibrated(const int32_t* pool_idx, const float* pool_score, int64_t ld, int32_t N, int64_t Q,
                           const uint32_t* attr, int64_t M, const float* target, int32_t k, float lambda, float alpha,
                           int32_t* out_idx, float* out_score, float* out_kl, int32_t* out_n, lgcn_stream_t stream) {
    const char* me = "lgcn_rerank_calibrated";
    if (!pool_idx) return fail(LGCN_E_ARG, "%s: pool_idx is null", me);
    if (!pool_score) return fail(LGCN_E_ARG, "%s: pool_score is null", me);
    if (!attr) return fail(LGCN_E_ARG, "%s: attr is null", me);
    if (!target) return fail(LGCN_E_ARG, "%s: target is null", me);
    if (!out_idx) return fail(LGCN_E_ARG, "%s: out_idx is null", me);
    if (!out_score) return fail(LGCN_E_ARG, "%s: out_score is null", me);
    if (!out_kl) return fail(LGCN_E_ARG, "%s: out_kl is null", me);
    if (!out_n) return fail(LGCN_E_ARG, "%s: out_n is null", me);
    if (N > LGCN_CALIB_MAX_POOL)
        return fail(LGCN_E_UNSUPPORTED, "%s: N=%d exceeds LGCN_CALIB_MAX_POOL=%d", me, N, LGCN_CALIB_MAX_POOL);
    if (k < 1 || k > N) return fail(LGCN_E_ARG, "%s: k=%d outside [1, N=%d]", me, k, N);
    if (ld < N) return fail(LGCN_E_ARG, "%s: ld=%lld < N=%d", me, (long long)ld, N);
    if (Q < 0) return fail(LGCN_E_ARG, "%s: Q=%lld", me, (long long)Q);
    if (M < 0) return fail(LGCN_E_ARG, "%s: M=%lld", me, (long long)M);
    if (!(lambda >= 0.f && lambda <= 1.f))
        return fail(LGCN_E_ARG, "%s: lambda=%g outside [0, 1]", me, static_cast<double>(lambda));
    if (!(alpha > 0.f && alpha < 1.f))
        return fail(LGCN_E_ARG, "%s: alpha=%g outside (0, 1)", me, static_cast<double>(alpha));
    if (Q > INT32_MAX) return fail(LGCN_E_ARG, "%s: Q=%lld is too many queries for one launch", me, (long long)Q);
    if (Q == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
    const int slots = (N + 63) / 64;
#define LGCN_CALIB_ARGS \
    pool_idx, pool_score, ld, N, Q, attr, M, target, k, lambda, alpha, out_idx, out_score, out_kl, out_n, s
    if (slots <= 1) return launch_calibrated<1>(LGCN_CALIB_ARGS);
    if (slots <= 2) return launch_calibrated<2>(LGCN_CALIB_ARGS);
    if (slots <= 4) return launch_calibrated<4>(LGCN_CALIB_ARGS);
    if (slots <= 8) return launch_calibrated<8>(LGCN_CALIB_ARGS);
    static_assert(kCalibMaxSlots == 16, "the slot dispatch below covers pools of up to 1024 entries");
    return launch_calibrated<16>(LGCN_CALIB_ARGS);
#undef LGCN_CALIB_ARGS
}

}  // extern "C"
