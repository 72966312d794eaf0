// Group recommendation (lgcn_score_filter_groups of include/lgcn.h): one list for several members.
//
// The score tile of lgcn_scoretile.h holds 32 query rows per wave; here those rows are the members of
// 32 / S groups of S rows each (S = 2, 4, 8, 16, 32; rows past a group's size are padding), and the
// epilogue reduces a candidate's member scores to ONE key per group before anything is tested or
// stored: the minimum (least misery), the maximum (most pleasure) or the mean of the members' scores,
// with an optional floor no member's score may lie under. What leaves the kernel are group lists, so
// the ranked selection, the exclusion rows and the host's block loop serve groups as they serve
// queries, and the list traffic is 1/S of the members' own.
//
// Where a candidate's 32 scores sit (ScoreTile::row): lane (i, h) of candidate i holds in accumulator
// r the score of row (r & 3) + 8 (r >> 2) + 4 h. Rows come in blocks of four, block b = row >> 2 in
// half h = b & 1 at accumulators 4 (b >> 1) .. + 3:
//   S = 2, 4    a group lies inside one block, so inside one lane: no exchange at all;
//   S = 8..32   a group is S / 4 consecutive blocks that alternate between the two halves. Minimum and
//               maximum reduce each half's rows first and meet in one exchange per group; the mean is a
//               chain in member order, handed to the other half after every four rows (S / 4 - 1
//               exchanges per group) and ends in half 1, whose lanes own the group's key.
// The translation unit is its own so that the filter modules' code and register budget stay as they
// are (lgcn_recall_lists.h says why). The MFMA loop is instantiated once per D; S and the aggregate
// are wave-uniform switches around the templated reduction.

#include "lgcn_scoretile.h"

using namespace lgcn;

namespace {

constexpr int kStage = 512;    // staged accepted keys per wave, as in k_score_filter
constexpr int kMaxSlots = 8;   // group keys a lane can own (S = 2: eight groups per lane)

// Which groups of the wave a lane owns, by slot.
template <int S>
struct GroupMap {
    static constexpr int kSlots = S == 2 ? 8 : S == 4 ? 4 : 32 / S;
    // group within the wave of a lane's slot
    static __device__ __forceinline__ int group(int slot, int h) {
        if constexpr (S == 2) return 4 * (slot >> 1) + 2 * h + (slot & 1);
        if constexpr (S == 4) return 2 * slot + h;
        return slot;
    }
    // whether the lanes of half h hold the finished key
    static __device__ __forceinline__ bool owner(int h) { return S <= 4 || h == 1; }
};

// One member's score into the running reduction. valid: the row is a member (and this lane's to take).
// MEAN: sum = s for member 0, sum + s after it. Otherwise `best` is the maximum of the members' keys
// with `flip` applied (0 for the maximum; 0xFFFFFFFF for the minimum, which is the maximum of the
// complements), a NaN being 0xFFFFFFFF under either. low: some member lies under the floor.
template <bool MEAN>
__device__ __forceinline__ void member(float s, bool first, bool valid, uint32_t flip, float flo, float& sum,
                                       uint32_t& best, bool& low) {
    low |= valid & (s < flo);
    if constexpr (MEAN) {
        const float next = first ? s : sum + s;
        sum = valid ? next : sum;
    } else {
        const uint32_t x = s != s ? 0xFFFFFFFFu : (ordered_key(s) ^ flip);
        const uint32_t v = valid ? x : 0u;
        best = best > v ? best : v;
    }
}

template <bool MEAN>
__device__ __forceinline__ uint32_t finish(float sum, uint32_t best, uint32_t n, uint32_t flip) {
    if constexpr (MEAN) return score_key(sum / static_cast<float>(n));
    return best == 0xFFFFFFFFu ? best : (best ^ flip);
}

// The keys of the groups a lane owns (key[slot], low[slot]) from the tile's accumulators; gng[slot] is
// the group's size (low byte). Called by whole waves.
template <int S, bool MEAN>
__device__ __forceinline__ void group_keys(const f32x16& acc, int lane, uint32_t flip, const uint32_t (&gng)[kMaxSlots],
                                           const float* sflo, uint32_t (&key)[kMaxSlots], bool (&low)[kMaxSlots]) {
    const int h = lane >> 5;
    if constexpr (S <= 4) {
        constexpr int PB = 4 / S;  // groups per block of four rows
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int u = 0; u < PB; ++u) {
                const int slot = t * PB + u;
                const uint32_t n = gng[slot] & 255u;
                const float flo = sflo ? sflo[gng[slot] >> 8] : -__builtin_inff();
                float sum = 0.f;
                uint32_t best = 0u;
                bool lo = false;
#pragma unroll
                for (int m = 0; m < S; ++m)
                    member<MEAN>(acc[4 * t + u * S + m], m == 0, static_cast<uint32_t>(m) < n, flip, flo, sum,
                                 best, lo);
                key[slot] = finish<MEAN>(sum, best, n, flip);
                low[slot] = lo;
            }
        }
    } else {
        constexpr int NB = S / 4;  // blocks of four rows per group, alternating between the halves
#pragma unroll
        for (int gw = 0; gw < 32 / S; ++gw) {
            const uint32_t n = gng[gw] & 255u;
            const float flo = sflo ? sflo[gw] : -__builtin_inff();
            float sum = 0.f;
            uint32_t best = 0u;
            bool lo = false;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const int t = (gw * NB + c) >> 1;
                const bool active = h == (c & 1);
                if constexpr (MEAN) {
                    if (c > 0) {  // the chain crosses to the half that holds the next four members
                        const float other = __shfl_xor(sum, 32, 64);
                        sum = active ? other : sum;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    member<MEAN>(acc[4 * t + u], c == 0 && u == 0, active & (static_cast<uint32_t>(4 * c + u) < n),
                                 flip, flo, sum, best, lo);
            }
            if constexpr (!MEAN) {
                const uint32_t other = __shfl_xor(best, 32, 64);
                best = best > other ? best : other;
            }
            const unsigned long long bm = __ballot(lo);
            key[gw] = finish<MEAN>(sum, best, n, flip);
            low[gw] = (((bm >> lane) | (bm >> (lane ^ 32))) & 1ull) != 0ull;
        }
    }
}

// a lane's slots: the group's size and its index within the wave (gng = n | gw << 8) and its threshold
// key. Padding groups and empty groups get size 0 and take nothing. (The floors stay in LDS, read per
// block only when there is a floor: eight more registers held through the MFMA loop cost the filter's
// occupancy at D = 64.)
template <int S>
__device__ __forceinline__ void group_slots(int h, int64_t g0, int64_t Gvalid, const int32_t* __restrict__ gsize,
                                            const uint32_t* __restrict__ thr, uint32_t (&gng)[kMaxSlots],
                                            uint32_t (&gthr)[kMaxSlots]) {
#pragma unroll
    for (int slot = 0; slot < GroupMap<S>::kSlots; ++slot) {
        const int gw = GroupMap<S>::group(slot, h);
        const int64_t g = g0 + gw;
        int32_t n = g < Gvalid ? gsize[g] : 0;
        n = n < 0 ? 0 : (n > S ? S : n);
        gng[slot] = static_cast<uint32_t>(n) | (static_cast<uint32_t>(gw) << 8);
        gthr[slot] = (g < Gvalid && thr) ? thr[g] : 0u;
    }
}

// k_score_filter's loop (lgcn_recall_lists.h: the double-buffered candidate blocks, place, the
// wave-private staging, one returning atomic per list and flush) with the group reduction between the
// MFMA chain and the test. lgS = log2(S).
template <int D>
__global__ __launch_bounds__(kBlock, ScoreTile<D>::kWaves) void k_score_filter_groups(
    const float* __restrict__ Qn, int64_t Gvalid, int32_t lgS, const int32_t* __restrict__ gsize, int32_t agg,
    const float* __restrict__ floor, int32_t nqg, int32_t nchunk, const float* __restrict__ Cn, int64_t M,
    int64_t stride, const uint32_t* __restrict__ thr, uint32_t* __restrict__ list_key, int32_t* __restrict__ list_idx,
    int32_t* __restrict__ list_n, int32_t cap) {
    using Tile = ScoreTile<D>;
    __shared__ float cs[2][Tile::kLdsFloats];
    __shared__ uint32_t st_key[4][kStage];
    __shared__ int32_t st_idx[4][kStage];
    __shared__ uint8_t st_row[4][kStage];  // group within the wave's (at most 16)
    __shared__ uint16_t st_rank[4][kStage];
    __shared__ int32_t st_cnt[4][32];
    __shared__ int32_t st_base[4][32];
    __shared__ float s_flo[4][16];  // the floors of each wave's groups
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int i = lane & 31;
    const int h = lane >> 5;
    int chunk;
    int64_t q0;  // first member row of this wave
    Tile::place(nqg, chunk, q0);
    Tile tile;
    tile.load_queries(Qn, q0);
    const int64_t g0 = q0 >> lgS;  // first group of this wave
    const uint32_t flip = agg == LGCN_GROUP_MIN ? 0xFFFFFFFFu : 0u;
    const bool mean = agg == LGCN_GROUP_MEAN;
    uint32_t gng[kMaxSlots], gthr[kMaxSlots];
#pragma unroll
    for (int s = 0; s < kMaxSlots; ++s) {
        gng[s] = 0u;
        gthr[s] = 0u;
    }
    // wave-private, written before the block loop's first barrier; null: no floor, nothing is read
    const float* sflo = floor ? s_flo[wv] : nullptr;
    if (floor && lane < 16) s_flo[wv][lane] = (g0 + lane < Gvalid && lane < (32 >> lgS)) ? floor[g0 + lane] : -__builtin_inff();
    int nslots = 0;
    bool own = true;
    switch (lgS) {
#define LGCN_GROUP_SLOTS(S) \
    group_slots<S>(h, g0, Gvalid, gsize, thr, gng, gthr); \
    nslots = GroupMap<S>::kSlots; \
    own = GroupMap<S>::owner(h); \
    break
        case 1: LGCN_GROUP_SLOTS(2);
        case 2: LGCN_GROUP_SLOTS(4);
        case 3: LGCN_GROUP_SLOTS(8);
        case 4: LGCN_GROUP_SLOTS(16);
        default: LGCN_GROUP_SLOTS(32);
#undef LGCN_GROUP_SLOTS
    }
    int scnt = 0;  // wave-uniform staged count
    const unsigned long long below = (1ull << lane) - 1ull;
    auto flush = [&]() {
        if (lane < 32) st_cnt[wv][lane] = 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int e = lane; e < scnt; e += 64)
            st_rank[wv][e] = static_cast<uint16_t>(atomicAdd(&st_cnt[wv][st_row[wv][e]], 1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane < 32) {
            const int c = st_cnt[wv][lane];  // 0 for every lane past the wave's groups
            st_base[wv][lane] = c > 0 ? atomicAdd(list_n + g0 + lane, c) : 0;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        for (int e = lane; e < scnt; e += 64) {
            const int row = st_row[wv][e];
            const int32_t pos = st_base[wv][row] + st_rank[wv][e];
            if (pos < cap) {
                const int64_t g = g0 + row;
                list_key[g * cap + pos] = st_key[wv][e];
                list_idx[g * cap + pos] = st_idx[wv][e];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        scnt = 0;
    };
    const int64_t nblk = (M + 31) / 32;
    int64_t cb = chunk;
    if (cb < nblk) {
        tile.fetch(Cn, M, stride, cb);
        tile.land(cs, 0);
    }
    __syncthreads();
    int buf = 0;
    for (; cb < nblk; cb += nchunk) {
        const int64_t nxt = cb + nchunk;
        if (nxt < nblk) tile.fetch(Cn, M, stride, nxt);  // in flight during this block's MFMAs
        const f32x16 acc = tile.scores(cs, buf);
        const int64_t j = cb * 32 + i;
        const int32_t jj = static_cast<int32_t>(j * stride);
        const bool jok = (j < M) & own;
        uint32_t key[kMaxSlots];
        bool low[kMaxSlots];
#pragma unroll
        for (int s = 0; s < kMaxSlots; ++s) {
            key[s] = 0u;
            low[s] = false;
            // the sizes are loop-invariant, and left to itself the compiler hoists every "member m is
            // valid" compare out of the loop as a lane mask: dozens of SGPR pairs, spilled. Opaque per
            // block, the compare (one VALU op) stays where its select is.
            asm volatile("" : "+v"(gng[s]));
        }
        switch (lgS * 2 + (mean ? 1 : 0)) {
#define LGCN_GROUP_KEYS(S) \
    case 2 * (S == 2 ? 1 : S == 4 ? 2 : S == 8 ? 3 : S == 16 ? 4 : 5): \
        group_keys<S, false>(acc, lane, flip, gng, sflo, key, low); \
        break; \
    case 2 * (S == 2 ? 1 : S == 4 ? 2 : S == 8 ? 3 : S == 16 ? 4 : 5) + 1: \
        group_keys<S, true>(acc, lane, flip, gng, sflo, key, low); \
        break
            LGCN_GROUP_KEYS(2);
            LGCN_GROUP_KEYS(4);
            LGCN_GROUP_KEYS(8);
            LGCN_GROUP_KEYS(16);
            LGCN_GROUP_KEYS(32);
#undef LGCN_GROUP_KEYS
            default: break;
        }
        // one test and one append per group the lane owns
#pragma unroll
        for (int s = 0; s < kMaxSlots; ++s) {
            if (s >= nslots) break;  // wave-uniform
            const uint32_t n = gng[s] & 255u;
            const int gw = static_cast<int>(gng[s] >> 8);
            const bool take = jok & (n > 0u) & !low[s] & (key[s] >= gthr[s]);
            if (thr == nullptr) {  // dense mode: every group key at its candidate's slot
                if (take) {
                    const int64_t g = g0 + gw;
                    list_key[g * cap + j] = key[s];
                    list_idx[g * cap + j] = jj;
                }
                continue;
            }
            const unsigned long long m = __ballot(take);
            if (m == 0ull) continue;
            const int cnt = __popcll(m);
            if (scnt + cnt > kStage) flush();
            if (take) {
                const int sl = scnt + __popcll(m & below);
                st_key[wv][sl] = key[s];
                st_idx[wv][sl] = jj;
                st_row[wv][sl] = static_cast<uint8_t>(gw);
            }
            scnt += cnt;
        }
        if (nxt < nblk) tile.land(cs, buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    if (thr != nullptr) flush();
}

template <int D>
int launch_groups(const float* Qn, int64_t rows, int64_t Gvalid, int32_t lgS, const int32_t* gsize, int32_t agg,
                  const float* floor, const float* Cn, int64_t M, int64_t stride, const uint32_t* thr, uint32_t* lk,
                  int32_t* li, int32_t* ln, int32_t cap, hipStream_t s) {
    const int64_t nqg = rows / kTileQueries;
    int32_t nchunk;
    unsigned grid;
    if (!score_grid(nqg, M, nchunk, grid)) return fail(LGCN_E_ARG, "lgcn_score_filter_groups: too many groups");
    k_score_filter_groups<D><<<dim3(grid), kBlock, 0, s>>>(Qn, Gvalid, lgS, gsize, agg, floor,
                                                           static_cast<int32_t>(nqg), nchunk, Cn, M, stride, thr, lk, li,
                                                           ln, cap);
    return check_launch("k_score_filter_groups");
}

}  // namespace

extern "C" {

int lgcn_score_filter_groups(const float* Qn, int64_t Gpad, int64_t Gvalid, int32_t S, const int32_t* gsize,
                             int32_t agg, const float* floor, const float* Cn, int64_t M, int64_t stride, int32_t D,
                             const uint32_t* thr, uint32_t* list_key, int32_t* list_idx, int32_t* list_n, int32_t cap,
                             lgcn_stream_t stream) {
    const char* me = "lgcn_score_filter_groups";
    int32_t lgS = 0;
    while (lgS < 6 && (1 << lgS) != S) ++lgS;
    if (lgS < 1 || lgS > 5)
        return fail(LGCN_E_ARG, "%s: S=%d (2, 4, 8, 16 or %d members per group)", me, S, LGCN_GROUP_MAX_MEMBERS);
    if (agg != LGCN_GROUP_MIN && agg != LGCN_GROUP_MAX && agg != LGCN_GROUP_MEAN)
        return fail(LGCN_E_ARG, "%s: agg=%d", me, agg);
    if (Gpad <= 0 || Gpad > (int64_t(1) << 40) || (Gpad * S) % kTileQueries != 0)
        return fail(LGCN_E_ARG, "%s: Gpad=%lld groups of S=%d are not a multiple of %d rows", me, (long long)Gpad, S,
                    kTileQueries);
    if (!gsize) return fail(LGCN_E_ARG, "%s: gsize is null", me);
    if (!list_key) return fail(LGCN_E_ARG, "%s: list_key is null", me);
    if (!list_idx) return fail(LGCN_E_ARG, "%s: list_idx is null", me);
    if (thr && !list_n) return fail(LGCN_E_ARG, "%s: list_n is null while thr is set", me);
    if (floor && !thr)
        return fail(LGCN_E_ARG, "%s: thr is null while floor is set (list mode only: a dense row cannot say absent)", me);
    if (!Qn || Gvalid < 0 || Gvalid > Gpad || M < 0 || stride <= 0 || cap <= 0 || (M > 0 && !Cn) ||
        (M - 1) * stride >= (int64_t(1) << 31))
        return fail(LGCN_E_ARG, "%s: bad args", me);
    if (!thr && M > cap) return fail(LGCN_E_ARG, "%s: dense mode needs M <= cap", me);
    if (M == 0 || Gvalid == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
#define LGCN_GROUPS(W) \
    case W: \
        return launch_groups<W>(Qn, Gpad * S, Gvalid, lgS, gsize, agg, floor, Cn, M, stride, thr, list_key, list_idx, \
                                list_n, cap, s)
    switch (D) {
        LGCN_GROUPS(8);
        LGCN_GROUPS(16);
        LGCN_GROUPS(32);
        LGCN_GROUPS(64);
        LGCN_GROUPS(128);
        LGCN_GROUPS(256);
        default: return fail(LGCN_E_UNSUPPORTED, "%s: D=%d (use lgcn_recall_width)", me, D);
    }
#undef LGCN_GROUPS
}

}  // extern "C"
