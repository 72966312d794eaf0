// The list kernels of top-k serving and Recall@k, with their launches: k_score_filter (the score tile
// of lgcn_scoretile.h plus the filtering epilogue) and k_select_ranked (the ranked selection with an
// exclusion row), each with the attribute filter of include/lgcn.h as a bool template parameter, and
// k_score_filter with the per-candidate boost as another.
// lgcn_recall.hip instantiates the unfiltered kernels, lgcn_recall_attr.hip the filtered ones and
// lgcn_recall_boost.hip the boosted filters: separate
// translation units, so that adding a filtered instantiation leaves the unfiltered kernels' module,
// and with it their code and register budget, exactly as it was (within one module the compiler's
// output for one instantiation moves with the presence of the other).
#pragma once

#include "lgcn_common.h"
#include "lgcn_ragged.h"
#include "lgcn_scoretile.h"

using namespace lgcn;

namespace {

// Attribute filters (lgcn_score_filter_attr, lgcn_select_topk_ranked_attr): a candidate carries a
// 32-bit attribute word, a query three masks (any, all, none), and attr_passes below is tested where
// the score is tested, so a list only ever holds candidates that pass.

constexpr int kStage = 512;  // staged accepted scores per wave

// A filtered kernel's two extra arguments, and nothing at all in the unfiltered instantiation (an empty
// record takes no kernel argument, so that one keeps the argument block it had).
template <bool kAttr>
struct AttrArgs {};
template <>
struct AttrArgs<true> {
    const uint32_t* attr;   // [M] attribute words, by candidate index
    const uint32_t* where;  // [Qvalid, 3] (any, all, none)
};

// the attribute predicate of include/lgcn.h: no bit of `none`, every bit of `all`, and a bit of `any`
// unless `any` is 0
__device__ __forceinline__ bool attr_passes(uint32_t a, uint32_t any, uint32_t all, uint32_t none) {
    return ((a & none) == 0u) & ((a & all) == all) & ((any == 0u) | ((a & any) != 0u));
}

// The score tile of lgcn_scoretile.h (which explains the tiling, the grid and the occupancy) with
// the filtering epilogue: the thresholds of a lane's 16 query rows in registers, accepted scores
// staged per wave in LDS.
// kAttr (list mode only, thr set): a score is kept only if its candidate's attribute word passes the
// query's masks. The lane's word attr[j * stride] of a block is loaded with the block's rows, one
// block ahead; the masks of the wave's 32 queries sit in LDS (96 words per wave, staged once) and are
// read per query row, only for the rows whose threshold some lane met: the lanes of a half read one
// address, a broadcast.
// kBoost (lgcn_score_filter_boost; dense and list mode, with kAttr or without): the score of the lane's
// candidate j is acc[r] + boost[j * stride], one f32 addition, wherever a score is used — the threshold
// test and the key — so the thresholds, the lists and the selection all see boosted keys. The lane's
// boost of a block is loaded with the block's rows, one block ahead, as the attribute word is (0 past
// M, where nothing is taken): two registers. Padding queries take nothing under any boost (the row
// test beside the threshold test). The boosted instantiations live in lgcn_recall_boost.hip,
// for the reason the head of this file gives for lgcn_recall_attr.hip.
template <int D, bool kAttr = false, bool kBoost = false>
__global__ __launch_bounds__(kBlock, ScoreTile<D>::kWaves) void k_score_filter(
    const float* __restrict__ Qn, int64_t Qvalid, int32_t nqg, int32_t nchunk, const float* __restrict__ Cn, int64_t M,
    int64_t stride, const uint32_t* __restrict__ thr, uint32_t* __restrict__ list_key, int32_t* __restrict__ list_idx,
    int32_t* __restrict__ list_n, int32_t cap, AttrArgs<kAttr> fa, BoostArgs<kBoost> fb) {
    using Tile = ScoreTile<D>;
    __shared__ float cs[2][Tile::kLdsFloats];
    __shared__ uint32_t wh[kAttr ? 4 : 1][96];  // (any, all, none) of each wave's 32 queries
    // wave-private staging of accepted scores: appended without atomics (ballot prefix), flushed
    // to the per-query lists with ONE returning global atomic per query per flush
    __shared__ uint32_t st_key[4][kStage];
    __shared__ int32_t st_idx[4][kStage];
    __shared__ uint8_t st_row[4][kStage];  // query row within the wave's 32
    __shared__ uint16_t st_rank[4][kStage];
    __shared__ int32_t st_cnt[4][32];
    __shared__ int32_t st_base[4][32];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int i = lane & 31;
    const int h = lane >> 5;
    int chunk;
    int64_t q0;  // first query of this wave
    Tile::place(nqg, chunk, q0);
    Tile tile;
    tile.load_queries(Qn, q0);
    // this lane's 16 output rows. The test runs on floats, inclusively:
    // !(score < t) keeps every score whose key is >= the threshold key (and NaN, which ranks
    // first, and -0 beside +0 — extra entries are harmless, the selection works on exact keys).
    // Padding queries get +inf (their zero rows score 0).
    float th[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t q = q0 + Tile::row(r, h);
        th[r] = (q < Qvalid) ? (thr ? key_score(thr[q]) : -__builtin_inff()) : __builtin_inff();
    }
    if constexpr (kAttr) {  // padding queries take nothing (th = +inf): their masks are not read
        for (int t = lane; t < 96; t += 64) wh[wv][t] = (q0 + t / 3 < Qvalid) ? fa.where[q0 * 3 + t] : 0u;
    }
    // this lane's candidate of block cb: its attribute word (0 past M, where nothing is taken)
    [[maybe_unused]] auto attr_of = [&](int64_t b) -> uint32_t {
        const int64_t j = b * 32 + i;
        if constexpr (kAttr) return j < M ? fa.attr[j * stride] : 0u;
        return 0u;
    };
    [[maybe_unused]] uint32_t at = 0u, at_nxt = 0u;
    // ... and its boost
    [[maybe_unused]] auto boost_of = [&](int64_t b) -> float {
        const int64_t j = b * 32 + i;
        if constexpr (kBoost) return j < M ? fb.boost[j * stride] : 0.f;
        return 0.f;
    };
    [[maybe_unused]] float bo = 0.f, bo_nxt = 0.f;
    // kBoost: the wave's real query rows are [0, nv). th = +inf keeps a padding row's plain score out, but
    // not a +inf or NaN sum (!(sc < +inf) holds for both), so a boosted kernel tests the row as well.
    [[maybe_unused]] const int64_t left = Qvalid - q0;
    [[maybe_unused]] const int nv = left >= 32 ? 32 : left <= 0 ? 0 : static_cast<int>(left);
    int scnt = 0;  // wave-uniform staged count
    const unsigned long long below = (1ull << lane) - 1ull;
    // flush (wave-uniform): ranks within each query row from LDS atomics (list order does not
    // matter: selection ranks keys), one global atomic per row, then the stores
    auto flush = [&]() {
        if (lane < 32) st_cnt[wv][lane] = 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int e = lane; e < scnt; e += 64)
            st_rank[wv][e] = static_cast<uint16_t>(atomicAdd(&st_cnt[wv][st_row[wv][e]], 1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane < 32) {
            const int c = st_cnt[wv][lane];
            st_base[wv][lane] = c > 0 ? atomicAdd(list_n + q0 + lane, c) : 0;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        for (int e = lane; e < scnt; e += 64) {
            const int row = st_row[wv][e];
            const int32_t pos = st_base[wv][row] + st_rank[wv][e];
            if (pos < cap) {
                const int64_t q = q0 + row;
                list_key[q * cap + pos] = st_key[wv][e];
                list_idx[q * cap + pos] = st_idx[wv][e];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        scnt = 0;
    };
    const int64_t nblk = (M + 31) / 32;
    int64_t cb = chunk;
    if (cb < nblk) {
        tile.fetch(Cn, M, stride, cb);
        if constexpr (kAttr) at = attr_of(cb);
        if constexpr (kBoost) bo = boost_of(cb);
        tile.land(cs, 0);
    }
    __syncthreads();
    int buf = 0;
    for (; cb < nblk; cb += nchunk) {
        const int64_t nxt = cb + nchunk;
        if (nxt < nblk) {  // in flight during this block's MFMAs
            tile.fetch(Cn, M, stride, nxt);
            if constexpr (kAttr) at_nxt = attr_of(nxt);
            if constexpr (kBoost) bo_nxt = boost_of(nxt);
        }
        const f32x16 acc = tile.scores(cs, buf);
        // epilogue: column = candidate j (this lane's), rows = queries; branch-free test, and
        // a wave-uniform branch only for the (rare) slots where some lane passes
        const int64_t j = cb * 32 + i;
        const int32_t jj = static_cast<int32_t>(j * stride);
        const bool jok = j < M;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = Tile::row(r, h);
            float sc = acc[r];
            if constexpr (kBoost) sc = __fadd_rn(sc, bo);
            bool take = jok & !(sc < th[r]);
            if constexpr (kBoost) take &= row < nv;
            if constexpr (kAttr) {
                if (__ballot(take) == 0ull) continue;
                const uint32_t* w = &wh[wv][row * 3];
                take &= attr_passes(at, w[0], w[1], w[2]);
            }
            if (!kAttr && thr == nullptr) {  // dense mode: every subset score at its subset slot
                const uint32_t key = score_key(sc);
                if (take) {
                    const int64_t q = q0 + row;
                    list_key[q * cap + j] = key;
                    list_idx[q * cap + j] = jj;
                }
                continue;
            }
            const unsigned long long m = __ballot(take);
            if (m == 0ull) continue;
            const int n = __popcll(m);
            if (scnt + n > kStage) flush();
            if (take) {
                const int sl = scnt + __popcll(m & below);
                st_key[wv][sl] = score_key(sc);
                st_idx[wv][sl] = jj;
                st_row[wv][sl] = static_cast<uint8_t>(row);
            }
            scnt += n;
        }
        if (nxt < nblk) tile.land(cs, buf ^ 1);
        __syncthreads();
        buf ^= 1;
        if constexpr (kAttr) at = at_nxt;
        if constexpr (kBoost) bo = bo_nxt;
    }
    if (kAttr || thr != nullptr) flush();
}

// workgroup of the select kernels (k_select_topk in lgcn_recall.hip, k_select_ranked here)
constexpr int kSelBlock = 1024;

// ---------------------------------------------------------------------------------------------
// Ranked selection with a per-query exclusion row (lgcn_select_topk_ranked): which candidates, in
// which order. One workgroup per query over the same (key, index) lists as k_select_topk.
//   1. eligibility: an entry whose candidate index is found in the query's sorted exclusion row
//      (binary search) is dropped; one bit per entry in LDS, written per wave from a ballot, so the
//      search runs once per entry and later passes read the bit;
//   2. the k-th best eligible entry under (key descending, index ascending): a radix select over
//      the 64-bit composite (key << 32) | (0xFFFFFFFF - index), 8-bit digits from the top. The
//      composites of a list are distinct (an index appears once), so the order is total and equal
//      scores never depend on the order the filter's atomics appended them in. score_key never
//      gives key 0 (only the bit pattern 0xFFFFFFFF maps there, and it is a NaN, keyed
//      0xFFFFFFFF), so composite 0 marks a dropped entry. When every entry tied with the k-th key
//      is taken the index digits decide nothing and are skipped;
//   3. threshold mode: the k-th key; emit mode: the winners (composite >= the k-th) are gathered
//      in LDS, ranked there (all-pairs count; at most 1024 distinct composites) and stored in
//      rank order.
// No global atomics, no waiting on other workgroups; list loads are coalesced (thread t reads
// entries t, t + 1024, ...).
// kAttr (lgcn_select_topk_ranked_attr): step 1 also requires attr_passes of the entry's candidate
// against the query's masks (uniform over the workgroup); everything after it reads the bit.
// kRepeats (dense_n == LGCN_RANKED_REPEATS beside list_n): a list may name a candidate more than once,
// as lgcn_score_lists' may, so composites may be EQUAL, which step 3 above cannot take: copies of the
// k-th composite T that straddle slot k make the gather `c >= T` take more than k entries, and the
// guard `slot < k` may then drop a better entry instead of a copy; and equal winners compute the same
// rank, so one slot is written twice and one never. This instantiation gathers only the entries
// ABOVE T (at most k, by the definition of T) and counts the entries equal to T — they are all T —
// which fill the slots that are left; equal winners above T take consecutive ranks in gather order.
// A template parameter and not a change of step 3, so that the lists without repeats (every caller
// before lgcn_score_lists) are ranked by the instruction stream they were ranked by.
constexpr int kRankMaxK = LGCN_RANKED_MAX_K;
constexpr int kRankMaxCap = LGCN_RANKED_MAX_CAP;

template <bool kAttr, bool kRepeats = false>
__global__ __launch_bounds__(kSelBlock) void k_select_ranked(
    const uint32_t* __restrict__ list_key, const int32_t* __restrict__ list_idx, const int32_t* __restrict__ list_n,
    int32_t dense_n, int32_t cap, int32_t k, int64_t Qvalid, const int64_t* __restrict__ excl_ptr,
    const int32_t* __restrict__ excl_idx, const int64_t* __restrict__ excl_row, int64_t excl_rows,
    uint32_t* __restrict__ thr_out, int32_t* __restrict__ out_idx, float* __restrict__ out_score,
    int32_t* __restrict__ out_n, AttrArgs<kAttr> fa) {
    __shared__ unsigned long long elig[kRankMaxCap / 64];
    __shared__ unsigned long long win[kRankMaxK];
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long s_prefix, s_mask;
    __shared__ uint32_t s_k, s_bin, s_cnt;
    __shared__ uint32_t s_eq;  // kRepeats: entries equal to the k-th composite
    __shared__ int32_t red[kSelBlock / 64];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const float ninf = -__builtin_inff();
    if (q >= Qvalid) {  // padding queries: nothing ranked
        if (thr_out && tid == 0) thr_out[q] = 0xFFFFFFFFu;
        if (out_idx) {
            for (int t = tid; t < k; t += kSelBlock) {
                out_idx[q * k + t] = -1;
                out_score[q * k + t] = ninf;
            }
            if (tid == 0) out_n[q] = 0;
        }
        return;
    }
    int32_t n = list_n ? list_n[q] : dense_n;
    if (n > cap) n = cap;
    if (n < 0) n = 0;
    const uint32_t* keys = list_key + q * cap;
    const int32_t* idx = list_idx + q * cap;
    // this query's exclusion row (a row outside [0, excl_rows) excludes nothing)
    int64_t exb = 0, exe = 0;
    if (excl_ptr) ragged_row(q, excl_ptr, excl_row, excl_rows, exb, exe);
    const int32_t* ex = excl_idx + exb;
    const int64_t exn = exe - exb;
    uint32_t w_any = 0u, w_all = 0u, w_none = 0u;
    if constexpr (kAttr) {
        w_any = fa.where[q * 3];
        w_all = fa.where[q * 3 + 1];
        w_none = fa.where[q * 3 + 2];
    }
    // 1. eligibility bits, 64 entries per wave step
    int32_t mine = 0;
    for (int32_t base = wv * 64; base < n; base += kSelBlock) {
        const int32_t e = base + lane;
        bool ok = e < n;
        if constexpr (kAttr) {
            if (ok) ok = attr_passes(fa.attr[idx[e]], w_any, w_all, w_none);
        }
        if (ok && exn > 0) ok = !sorted_contains(ex, exn, idx[e]);
        const unsigned long long m = __ballot(ok);
        if (lane == 0) {
            elig[base >> 6] = m;
            mine += __popcll(m);
        }
    }
    if (lane == 0) red[wv] = mine;
    if (tid == 0) {
        s_prefix = 0ull;
        s_mask = 0ull;
        s_k = static_cast<uint32_t>(k);
        s_bin = 0u;
        s_cnt = 0u;
        if constexpr (kRepeats) s_eq = 0u;
    }
    __syncthreads();
    int32_t n_elig = 0;
#pragma unroll
    for (int w = 0; w < kSelBlock / 64; ++w) n_elig += red[w];
    auto composite = [&](int32_t e) -> unsigned long long {
        if (!((elig[e >> 6] >> (e & 63)) & 1ull)) return 0ull;
        return (static_cast<unsigned long long>(keys[e]) << 32) |
               static_cast<unsigned long long>(0xFFFFFFFFu - static_cast<uint32_t>(idx[e]));
    };
    // 2. the k-th best composite T (1 = "every eligible entry" when fewer than k are eligible)
    unsigned long long T = 1ull;
    if (n_elig >= k) {
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int t = tid; t < 256; t += kSelBlock) hist[t] = 0u;
            __syncthreads();
            const unsigned long long prefix = s_prefix, mask = s_mask;
            for (int32_t e = tid; e < n; e += kSelBlock) {
                const unsigned long long c = composite(e);
                if (c != 0ull && (c & mask) == prefix) atomicAdd(&hist[(c >> shift) & 255ull], 1u);
            }
            __syncthreads();
            if (wv == 0) {
                // the first bin from the top at which the running count reaches s_k, by wave 0:
                // lane l sums bins 255 - 4l .. 252 - 4l, a prefix over the lanes finds the lane
                // the count is reached in, and that lane walks its four bins
                const int b0 = 255 - 4 * lane;
                const uint32_t h[4] = {hist[b0], hist[b0 - 1], hist[b0 - 2], hist[b0 - 3]};
                const uint32_t sum = h[0] + h[1] + h[2] + h[3];
                uint32_t inc = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t up = __shfl_up(inc, off, 64);
                    if (lane >= off) inc += up;
                }
                const uint32_t kk = s_k;
                uint32_t cum = inc - sum;
                if (cum < kk && kk <= inc) {
                    int j = 0;
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        if (j == t && cum + h[t] < kk) {
                            cum += h[t];
                            j = t + 1;
                        }
                    }
                    s_k = kk - cum;
                    s_bin = j == 0 ? h[0] : j == 1 ? h[1] : j == 2 ? h[2] : h[3];
                    s_prefix = prefix | (static_cast<unsigned long long>(b0 - j) << shift);
                    s_mask = mask | (255ull << shift);
                }
            }
            __syncthreads();
            // the key is fixed and all s_bin entries that carry it are taken: the index digits
            // would only find the last of them
            if (shift == 32 && s_k == s_bin) break;
        }
        T = s_prefix;
    }
    if (thr_out && tid == 0) thr_out[q] = n_elig >= k ? static_cast<uint32_t>(T >> 32) : 0u;
    if (!out_idx) return;
    if constexpr (kRepeats) {  // 3. with equal composites: see the head of the kernel
        for (int32_t e = tid; e < n; e += kSelBlock) {
            const unsigned long long c = composite(e);
            if (c > T) {
                const uint32_t slot = atomicAdd(&s_cnt, 1u);
                if (slot < static_cast<uint32_t>(k)) win[slot] = c;
            } else if (c != 0ull && c == T) {
                atomicAdd(&s_eq, 1u);
            }
        }
        __syncthreads();
        const int32_t G = s_cnt < static_cast<uint32_t>(k) ? static_cast<int32_t>(s_cnt) : k;  // above T
        const int32_t W = s_eq < static_cast<uint32_t>(k - G) ? G + static_cast<int32_t>(s_eq) : k;
        for (int t = tid; t < k; t += kSelBlock) {
            if (t < W) {
                const unsigned long long c = t < G ? win[t] : T;
                int32_t rank = t;  // the copies of T stand below everything gathered, in their slots
                if (t < G) {
                    rank = 0;
                    for (int32_t j = 0; j < G; ++j) rank += (win[j] > c) | ((win[j] == c) & (j < t));
                }
                out_idx[q * k + rank] = static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(c));
                out_score[q * k + rank] = key_score(static_cast<uint32_t>(c >> 32));
            } else {
                out_idx[q * k + t] = -1;
                out_score[q * k + t] = ninf;
            }
        }
        if (tid == 0) out_n[q] = W;
        return;
    }
    // 3. gather the winners, rank them, store in rank order
    for (int32_t e = tid; e < n; e += kSelBlock) {
        const unsigned long long c = composite(e);
        if (c != 0ull && c >= T) {
            const uint32_t slot = atomicAdd(&s_cnt, 1u);
            if (slot < static_cast<uint32_t>(k)) win[slot] = c;
        }
    }
    __syncthreads();
    const int32_t W = s_cnt < static_cast<uint32_t>(k) ? static_cast<int32_t>(s_cnt) : k;
    for (int t = tid; t < k; t += kSelBlock) {
        if (t < W) {
            const unsigned long long c = win[t];
            int32_t rank = 0;
            for (int32_t j = 0; j < W; ++j) rank += win[j] > c ? 1 : 0;
            out_idx[q * k + rank] = static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(c));
            out_score[q * k + rank] = key_score(static_cast<uint32_t>(c >> 32));
        } else {
            out_idx[q * k + t] = -1;
            out_score[q * k + t] = ninf;
        }
    }
    if (tid == 0) out_n[q] = W;
}

template <int D, bool kAttr = false, bool kBoost = false>
int launch_filter(const float* Qn, int64_t Qpad, int64_t Qvalid, const float* Cn, int64_t M, int64_t stride,
                  const uint32_t* thr, uint32_t* lk, int32_t* li, int32_t* ln, int32_t cap, hipStream_t s,
                  const uint32_t* attr = nullptr, const uint32_t* where = nullptr, const float* boost = nullptr) {
    const char* me = kBoost ? "lgcn_score_filter_boost" : kAttr ? "lgcn_score_filter_attr" : "lgcn_score_filter";
    if (Qpad % kTileQueries != 0)
        return fail(LGCN_E_ARG, "%s: padded query count %lld not a multiple of %d", me, (long long)Qpad, kTileQueries);
    const int64_t nqg = Qpad / kTileQueries;
    int32_t nchunk;
    unsigned grid;
    if (!score_grid(nqg, M, nchunk, grid)) return fail(LGCN_E_ARG, "%s: too many queries", me);
    AttrArgs<kAttr> fa;
    if constexpr (kAttr) fa = {attr, where};
    BoostArgs<kBoost> fb;
    if constexpr (kBoost) fb = {boost};
    k_score_filter<D, kAttr, kBoost><<<dim3(grid), kBlock, 0, s>>>(Qn, Qvalid, static_cast<int32_t>(nqg), nchunk, Cn, M,
                                                                   stride, thr, lk, li, ln, cap, fa, fb);
    return check_launch(kBoost ? (kAttr ? "k_score_filter<attr, boost>" : "k_score_filter<boost>")
                               : kAttr ? "k_score_filter<attr>" : "k_score_filter");
}


// the two ranked entry points: one argument check, the kernel instantiation by kAttr
template <bool kAttr>
int select_ranked(const char* me, const uint32_t* list_key, const int32_t* list_idx, const int32_t* list_n,
                  int32_t dense_n, int32_t cap, int32_t k, int64_t Qpad, int64_t Qvalid, const int64_t* excl_ptr,
                  const int32_t* excl_idx, const int64_t* excl_row, int64_t excl_rows, uint32_t* thr_out,
                  int32_t* out_idx, float* out_score, int32_t* out_n, const uint32_t* attr, const uint32_t* where,
                  lgcn_stream_t stream) {
    if (kAttr && !attr) return fail(LGCN_E_ARG, "%s: attr is null", me);
    if (kAttr && !where) return fail(LGCN_E_ARG, "%s: where is null", me);
    if (!list_key) return fail(LGCN_E_ARG, "%s: list_key is null", me);
    if (!list_idx) return fail(LGCN_E_ARG, "%s: list_idx is null", me);
    if (k < 1 || k > kRankMaxK) return fail(LGCN_E_ARG, "%s: k=%d outside [1, %d]", me, k, kRankMaxK);
    if (cap < k) return fail(LGCN_E_ARG, "%s: cap=%d < k=%d", me, cap, k);
    if (cap > kRankMaxCap) return fail(LGCN_E_UNSUPPORTED, "%s: cap=%d > %d", me, cap, kRankMaxCap);
    if (!list_n && (dense_n < 0 || dense_n > cap))
        return fail(LGCN_E_ARG, "%s: dense_n=%d outside [0, cap=%d] (list_n is null)", me, dense_n, cap);
    if (Qpad <= 0 || Qvalid < 0 || Qvalid > Qpad || Qpad > INT32_MAX)
        return fail(LGCN_E_ARG, "%s: Qvalid=%lld / Qpad=%lld", me, (long long)Qvalid, (long long)Qpad);
    if (excl_ptr && !excl_idx) return fail(LGCN_E_ARG, "%s: excl_idx is null while excl_ptr is set", me);
    if (excl_ptr && excl_rows < 0) return fail(LGCN_E_ARG, "%s: excl_rows=%lld", me, (long long)excl_rows);
    const bool emit = out_idx || out_score || out_n;
    if (!thr_out && !emit) return fail(LGCN_E_ARG, "%s: no output (thr_out and out_idx are null)", me);
    if (emit && !out_idx) return fail(LGCN_E_ARG, "%s: out_idx is null", me);
    if (emit && !out_score) return fail(LGCN_E_ARG, "%s: out_score is null", me);
    if (emit && !out_n) return fail(LGCN_E_ARG, "%s: out_n is null", me);
    AttrArgs<kAttr> fa;
    if constexpr (kAttr) fa = {attr, where};
    if (list_n && dense_n == LGCN_RANKED_REPEATS) {  // lists that may name a candidate more than once
        k_select_ranked<kAttr, true><<<dim3(static_cast<unsigned>(Qpad)), kSelBlock, 0, as_stream(stream)>>>(
            list_key, list_idx, list_n, dense_n, cap, k, Qvalid, excl_ptr, excl_idx, excl_row, excl_rows, thr_out,
            out_idx, out_score, out_n, fa);
        return check_launch(kAttr ? "k_select_ranked<attr, repeats>" : "k_select_ranked<repeats>");
    }
    k_select_ranked<kAttr><<<dim3(static_cast<unsigned>(Qpad)), kSelBlock, 0, as_stream(stream)>>>(
        list_key, list_idx, list_n, dense_n, cap, k, Qvalid, excl_ptr, excl_idx, excl_row, excl_rows, thr_out, out_idx,
        out_score, out_n, fa);
    return check_launch(kAttr ? "k_select_ranked<attr>" : "k_select_ranked");
}


}  // namespace
