// Exact full-ranking positions on gfx950 (lgcn_rank_positions): for every (query, held-out item)
// pair the number of eligible candidates that stand above the item under the ranking rule of
// lgcn_select_topk_ranked — lgcn_score_filter's key descending, candidate index ascending, NaN
// first, the query's seen row dropped — without a [Q, M] score matrix and without candidate lists.
// What AUC, mean percentile rank, an uncapped MRR and "where does item X rank for this user" are
// made of. Three stages on the caller's stream:
//
//   k_target_keys   one wave per query: the keys of its truth row's items, 32 per round, and the
//                   zeroed counts. A round is ONE 32x32 tile of the filter's instruction,
//                   v_mfma_f32_32x32x2_f32, in the filter's column order, every A row the query and
//                   B column c the round's c-th item: row 0 of the tile is the 32 scores
//                   (ScoreTile::row_keys, defined in lgcn_scoretile.h beside the filter's chain). The
//                   keys are therefore the filter's bit for bit — same instruction, same operands,
//                   same order — and not a restatement of its rounding as an fmaf chain. The tile's
//                   other 31 rows are redundant work, 32 x a few thousand pairs: nothing beside stage b.
//   k_count_above   the hot path: k_score_filter's tile loop (lgcn_scoretile.h: 32 queries per wave in
//                   registers, 32-candidate blocks double-buffered through LDS, the XCD-aware grid)
//                   with another epilogue. Each of a lane's 16 scores becomes a key and is compared with
//                   TC targets of its query row; the thresholds are read from LDS (the 32 lanes of
//                   a half-wave share a row: a broadcast), the 16 x TC counters stay in registers.
//                   At the end of the wave's candidate chunk the counters are summed over the 32
//                   lanes of each row and added to the global int32 count of the (query, target)
//                   with one integer atomic each — integer sums, so any order gives the same bits.
//                   Targets are taken TC per pass over the candidates (a truth row may be of any
//                   length); a wave none of whose 32 queries has a target in the pass skips the
//                   arithmetic and keeps the workgroup's barriers. A key EQUAL to a threshold — the
//                   target itself, a duplicated row, NaN beside NaN — sets a flag; a tile with the
//                   flag set anywhere in the wave runs a second, wave-uniform sweep that applies the
//                   index rule. Nothing proportional to M is stored, and the work does not depend
//                   on the scores (ties apart).
//   k_finish[_long] per query: the keys of its seen row's candidates (the same one-tile rounds), kept
//                   in LDS 512 per wave, then every target counts the seen candidates that beat it
//                   and takes them off its dense count; a target outside [0, M) or found in the seen
//                   row gets -1. One wave per query; seen rows above 512 entries are shared by the
//                   eight waves of a workgroup (which looks at eight queries a grid apart), as
//                   lgcn_explain.hip and lgcn_foldin.hip do for long histories. A target is owned by one thread throughout: no atomics here.
//
// TC (targets per pass) per width, from -Rpass-analysis=kernel-resource-usage: see DESIGN.md §17.
#include "lgcn_common.h"
#include "lgcn_ragged.h"
#include "lgcn_scoretile.h"

using namespace lgcn;

namespace {

constexpr uint32_t kNoKey = 0u;             // below every score's key (score_key never gives 0)
constexpr int32_t kNoIndex = 0x7FFFFFFF;    // an index no target is above

// i beats j: key above, or the same key and the lower index
__device__ __forceinline__ int beats(uint32_t ki, int32_t i, uint32_t kj, int32_t j) {
    return (ki > kj) | ((ki == kj) & (i < j));
}

// A fence in the instruction order of k_count_above's epilogue: the row's counters are complete
// before it and no LDS read crosses it, so a row's thresholds are live for two rows, not sixteen.
template <int TC>
__device__ __forceinline__ void pin_row(int32_t (&c)[TC]) {
#pragma unroll
    for (int t = 0; t < TC; t += 4)
        asm volatile("" : "+v"(c[t]), "+v"(c[t + 1]), "+v"(c[t + 2]), "+v"(c[t + 3])::"memory");
}

// a. one wave per query (four queries per workgroup)
template <int D>
__global__ __launch_bounds__(kBlock) void k_target_keys(const float* __restrict__ Qn, int64_t Q,
                                                        const float* __restrict__ Cn, int64_t M,
                                                        const int64_t* __restrict__ truth_ptr,
                                                        const int32_t* __restrict__ truth_idx,
                                                        const int64_t* __restrict__ truth_row, int64_t truth_rows,
                                                        const int64_t* __restrict__ out_ptr, int64_t nnz,
                                                        int32_t* __restrict__ pos_out, uint32_t* __restrict__ key_out,
                                                        int32_t* __restrict__ tgt) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    if (q >= Q) return;  // wave-uniform
    int64_t tb, te;
    ragged_row(q, truth_ptr, truth_row, truth_rows, tb, te);
    const int64_t base = out_ptr[q];
    const int64_t n = out_ptr[q + 1] - base;
    for (int64_t t0 = 0; t0 < n; t0 += 32) {  // wave-uniform
        const int64_t t = t0 + i;
        int32_t j = -1;
        if (t < n && tb + t < te) {
            const int32_t v = truth_idx[tb + t];
            if (v >= 0 && static_cast<int64_t>(v) < M) j = v;
        }
        const uint32_t key = ScoreTile<D>::row_keys(Qn + q * D, Cn, j, h);
        if (h == 0 && t < n && base + t >= 0 && base + t < nnz) {
            key_out[base + t] = j >= 0 ? key : kNoKey;
            tgt[base + t] = j;
            pos_out[base + t] = 0;
        }
    }
}

// b. the score tile of lgcn_scoretile.h (k_score_filter's, which explains the tiling and the grid)
// with the counting epilogue: see the head of the file.
template <int D, int TC>
__global__ __launch_bounds__(kBlock, ScoreTile<D>::kWaves) void k_count_above(
    const float* __restrict__ Qn, int64_t Q, int32_t nqg, int32_t nchunk, const float* __restrict__ Cn, int64_t M,
    const int64_t* __restrict__ out_ptr, int64_t nnz, const uint32_t* __restrict__ key_out,
    const int32_t* __restrict__ tgt, int32_t* __restrict__ pos_out) {
    static_assert(TC % 4 == 0, "thresholds are read four at a time");
    using Tile = ScoreTile<D>;
    __shared__ float cs[2][Tile::kLdsFloats];
    __shared__ __attribute__((aligned(16))) uint32_t s_thr[4][32 * TC];  // [wave][row][target of the pass]
    __shared__ __attribute__((aligned(16))) int32_t s_tgt[4][32 * TC];
    __shared__ int64_t s_base[4][32];
    __shared__ int32_t s_len[4][32];
    __shared__ int32_t s_max;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int i = lane & 31;
    const int h = lane >> 5;
    int chunk;
    int64_t q0;  // first query of this wave
    Tile::place(nqg, chunk, q0);
    // the truth rows of the workgroup's 128 queries: where their counts are, how many, the longest
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    int32_t mylen = 0;
    if (lane < 32) {
        const int64_t q = q0 + lane;
        int64_t b = 0, n = 0;
        if (q < Q) {
            b = out_ptr[q];
            n = out_ptr[q + 1] - b;
            if (n < 0 || b < 0 || b + n > nnz) n = 0;
            if (n > 0x7FFFFFFF) n = 0x7FFFFFFF;
        }
        s_base[wv][lane] = b;
        s_len[wv][lane] = mylen = static_cast<int32_t>(n);
    }
    int32_t wmax = mylen;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(wmax, off, 64);
        wmax = o > wmax ? o : wmax;
    }
    if (lane == 0 && wmax > 0) atomicMax(&s_max, wmax);
    __syncthreads();
    const int32_t gmax = s_max;  // workgroup-uniform
    if (gmax == 0) return;
    Tile tile;
    tile.load_queries(Qn, q0);
    const int64_t nblk = (M + 31) / 32;
    for (int32_t g0 = 0; g0 < gmax; g0 += TC) {  // a pass: targets g0 .. g0 + TC - 1 of every row
        const bool active = g0 < wmax;  // wave-uniform
        // this wave's thresholds of the pass; a row without a target at a slot gets a key no score
        // reaches from below (nothing counts) and index -1 (no candidate index is below it)
        for (int e = lane; e < 32 * TC; e += 64) {
            const int row = e / TC, t = g0 + e % TC;
            uint32_t k = 0xFFFFFFFFu;
            int32_t j = -1;
            if (t < s_len[wv][row]) {
                const int64_t at = s_base[wv][row] + t;
                k = key_out[at];
                j = tgt[at];
            }
            s_thr[wv][e] = k;
            s_tgt[wv][e] = j;
        }
        int32_t cnt[16][TC];
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int t = 0; t < TC; ++t) cnt[r][t] = 0;
        int64_t cb = chunk;
        if (cb < nblk) {
            tile.fetch(Cn, M, 1, cb);
            tile.land(cs, 0);
        }
        __syncthreads();  // also: the thresholds are in place, the previous pass is done with cs
        int buf = 0;
        for (; cb < nblk; cb += nchunk) {
            const int64_t nxt = cb + nchunk;
            if (nxt < nblk) tile.fetch(Cn, M, 1, nxt);  // in flight during this block's MFMAs
            if (active) {
                const f32x16 acc = tile.scores(cs, buf);
                // epilogue: column = candidate j (this lane's), rows = queries Tile::row(r, h)
                const int64_t j = cb * 32 + i;
                const int32_t jj = static_cast<int32_t>(j);
                const uint32_t jmask = j < M ? 0xFFFFFFFFu : kNoKey;  // a candidate past M has no key
                uint32_t tie = 0u;
                // straight-line code, a row's thresholds read one row ahead of its comparisons and
                // no earlier (left alone the compiler reads all 16 * TC up front, which spills)
                const uint4* tp = reinterpret_cast<const uint4*>(&s_thr[wv][4 * h * TC]);
                uint4 th[TC / 4];
#pragma unroll
                for (int t4 = 0; t4 < TC / 4; ++t4) th[t4] = tp[t4];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t key = score_key(acc[r]) & jmask;
                    uint4 nx[TC / 4];
                    if (r < 15) {
                        const int row0 = Tile::row(r + 1, 0);  // tp is at row 4h
#pragma unroll
                        for (int t4 = 0; t4 < TC / 4; ++t4) nx[t4] = tp[row0 * (TC / 4) + t4];
                    }
#pragma unroll
                    for (int t4 = 0; t4 < TC / 4; ++t4) {
                        cnt[r][4 * t4] += key > th[t4].x;
                        cnt[r][4 * t4 + 1] += key > th[t4].y;
                        cnt[r][4 * t4 + 2] += key > th[t4].z;
                        cnt[r][4 * t4 + 3] += key > th[t4].w;
                        tie |= (key == th[t4].x) | (key == th[t4].y) | (key == th[t4].z) | (key == th[t4].w);
                    }
                    pin_row(cnt[r]);
                    if (r < 15) {
#pragma unroll
                        for (int t4 = 0; t4 < TC / 4; ++t4) th[t4] = nx[t4];
                    }
                }
                if (__ballot(tie != 0u) != 0ull) {  // rare, wave-uniform: equal keys go by index
                    // the sweep reads its thresholds again: without this the first sweep's loaded
                    // values would be kept alive for it
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = Tile::row(r, h);
                        const uint32_t key = score_key(acc[r]) & jmask;
#pragma unroll
                        for (int t = 0; t < TC; ++t)
                            cnt[r][t] += (key == s_thr[wv][row * TC + t]) & (jj < s_tgt[wv][row * TC + t]);
                        pin_row(cnt[r]);  // row by row here too
                    }
                }
            }
            if (nxt < nblk) tile.land(cs, buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
        if (active) {
            // sum each counter over the 32 lanes of its row, one atomic per (query, target)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = Tile::row(r, h);
                const int32_t len = s_len[wv][row];
                const int64_t base = s_base[wv][row];
#pragma unroll
                for (int t = 0; t < TC; ++t) {
                    int32_t c = cnt[r][t];
#pragma unroll
                    for (int off = 16; off > 0; off >>= 1) c += __shfl_xor(c, off, 32);
                    if (i == 0 && g0 + t < len && c != 0) atomicAdd(pos_out + base + g0 + t, c);
                }
            }
        }
        // the next pass rewrites the thresholds: every lane of the wave is done reading them (the
        // barrier at the end of the last tile, or none of them was read)
    }
}

// c. the seen correction and the final value of one query's targets, by the W waves of the calling
// workgroup (64 * W threads, all of them call). ent holds kFinishChunk * W (key, index) pairs.
constexpr int kFinishChunk = 512;  // seen entries of one wave's share of a round
constexpr int kFinishWaves = 8;    // waves that share a long seen row
constexpr int kFinishLong = 512;   // seen entries above which they do

template <int D, int W>
__device__ __forceinline__ void finish_query(uint2* ent, int64_t q, const float* __restrict__ Qn,
                                             const float* __restrict__ Cn, int64_t M,
                                             const int32_t* __restrict__ seen, int64_t slen, int64_t base,
                                             int64_t tlen, const uint32_t* __restrict__ key_out,
                                             const int32_t* __restrict__ tgt, int32_t* __restrict__ pos_out,
                                             int32_t* __restrict__ eligible_out) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 31, h = lane >> 5;
    if (tid == 0) {  // the row is ascending and distinct: its entries inside [0, M) are one run
        int64_t lo = 0, hi = slen;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (seen[mid] < 0) lo = mid + 1;
            else hi = mid;
        }
        const int64_t first = lo;
        hi = slen;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (static_cast<int64_t>(seen[mid]) < M) lo = mid + 1;
            else hi = mid;
        }
        eligible_out[q] = static_cast<int32_t>(M - (lo - first));
    }
    if (tlen <= 0) return;  // workgroup-uniform
    for (int64_t c0 = 0; c0 < slen; c0 += kFinishChunk * W) {
        if (c0 > 0) __syncthreads();  // the previous round's readers are done
        for (int rd = 0; rd < kFinishChunk / 32; ++rd) {
            const int64_t e0 = c0 + wv * kFinishChunk + rd * 32;
            if (e0 >= slen) break;  // wave-uniform
            int32_t cand = -1;
            if (e0 + i < slen) {
                const int32_t v = seen[e0 + i];
                if (v >= 0 && static_cast<int64_t>(v) < M) cand = v;
            }
            const uint32_t key = ScoreTile<D>::row_keys(Qn + q * D, Cn, cand, h);
            if (h == 0)
                ent[wv * kFinishChunk + rd * 32 + i] =
                    cand >= 0 ? make_uint2(key, static_cast<uint32_t>(cand)) : make_uint2(kNoKey, kNoIndex);
        }
        __syncthreads();
        const int64_t left = slen - c0;
        const int n = left < kFinishChunk * W ? static_cast<int>(left) : kFinishChunk * W;
        for (int64_t t = tid; t < tlen; t += 64 * W) {
            const uint32_t kt = key_out[base + t];
            const int32_t jt = tgt[base + t];
            int32_t c = 0;
            for (int p = 0; p < n; ++p) {
                const uint2 e = ent[p];
                c += beats(e.x, static_cast<int32_t>(e.y), kt, jt);
            }
            if (c) pos_out[base + t] -= c;  // thread tid owns target t in every round
        }
    }
    for (int64_t t = tid; t < tlen; t += 64 * W) {
        const int32_t jt = tgt[base + t];
        if (jt < 0 || sorted_contains(seen, slen, jt)) pos_out[base + t] = -1;
    }
}

struct FinishArgs {
    const float* Qn;
    int64_t Q;
    const float* Cn;
    int64_t M;
    const int64_t* seen_ptr;
    const int32_t* seen_idx;
    const int64_t* seen_row;
    int64_t seen_rows;
    const int64_t* out_ptr;
    int64_t nnz;
    const uint32_t* key_out;
    const int32_t* tgt;
    int32_t* pos_out;
    int32_t* eligible_out;
};

// query q's seen row and its targets' slots (none when out_ptr is out of step with nnz)
__device__ __forceinline__ void finish_rows(const FinishArgs& A, int64_t q, int64_t& sb, int64_t& slen, int64_t& base,
                                            int64_t& tlen) {
    int64_t se = 0;
    sb = 0;
    if (A.seen_ptr) ragged_row(q, A.seen_ptr, A.seen_row, A.seen_rows, sb, se);
    slen = se - sb;
    base = A.out_ptr[q];
    tlen = A.out_ptr[q + 1] - base;
    if (tlen < 0 || base < 0 || base + tlen > A.nnz) tlen = 0;
}

template <int D>
__global__ __launch_bounds__(64) void k_finish(const FinishArgs A) {
    __shared__ uint2 ent[kFinishChunk];
    const int64_t q = blockIdx.x;
    int64_t sb, slen, base, tlen;
    finish_rows(A, q, sb, slen, base, tlen);
    if (slen > kFinishLong) return;  // k_finish_long's
    finish_query<D, 1>(ent, q, A.Qn, A.Cn, A.M, A.seen_idx + sb, slen, base, tlen, A.key_out, A.tgt, A.pos_out,
                       A.eligible_out);
}

template <int D>
__global__ __launch_bounds__(64 * kFinishWaves) void k_finish_long(const FinishArgs A) {
    __shared__ uint2 ent[kFinishChunk * kFinishWaves];
    // a workgroup's eight queries lie a grid apart: callers hand the queries over sorted by truth
    // length, which puts the long seen rows side by side too, and consecutive queries would leave
    // them all to a few workgroups (55 ms against 13 ms at the probe's 20 % split)
    for (int u = 0; u < kFinishWaves; ++u) {  // workgroup-uniform throughout
        const int64_t q = static_cast<int64_t>(blockIdx.x) + static_cast<int64_t>(u) * gridDim.x;
        if (q >= A.Q) break;
        int64_t sb, slen, base, tlen;
        finish_rows(A, q, sb, slen, base, tlen);
        if (slen <= kFinishLong) continue;
        __syncthreads();  // the workgroup's previous query is done with the LDS
        finish_query<D, kFinishWaves>(ent, q, A.Qn, A.Cn, A.M, A.seen_idx + sb, slen, base, tlen, A.key_out, A.tgt,
                                      A.pos_out, A.eligible_out);
    }
}

// targets per pass of k_count_above (DESIGN.md §17 has the compiler's register counts behind these)
template <int D>
constexpr int count_targets() { return D >= 128 && D < 256 ? 4 : 8; }

template <int D>
int launch_positions(const float* Qn, int64_t Qpad, int64_t Q, const float* Cn, int64_t M, const int64_t* truth_ptr,
                     const int32_t* truth_idx, const int64_t* truth_row, int64_t truth_rows, const FinishArgs& F,
                     uint32_t* key_out, int32_t* tgt, int32_t stages, hipStream_t s) {
    int rc = LGCN_OK;
    if (stages & LGCN_RANKPOS_KEYS) {
        k_target_keys<D><<<grid_for(Q * 64, kBlock, int64_t(1) << 31), kBlock, 0, s>>>(
            Qn, Q, Cn, M, truth_ptr, truth_idx, truth_row, truth_rows, F.out_ptr, F.nnz, F.pos_out, key_out, tgt);
        rc = check_launch("k_target_keys");
        if (rc != LGCN_OK) return rc;
    }
    if (M > 0 && (stages & LGCN_RANKPOS_COUNT)) {
        // query groups that hold a real query (<= Qpad / kTileQueries)
        const int64_t nqg = (Q + kTileQueries - 1) / kTileQueries;
        int32_t nchunk;
        unsigned grid;
        if (!score_grid(nqg, M, nchunk, grid))
            return fail(LGCN_E_ARG, "lgcn_rank_positions: too many queries for one launch");
        k_count_above<D, count_targets<D>()><<<dim3(grid), kBlock, 0, s>>>(
            Qn, Q, static_cast<int32_t>(nqg), nchunk, Cn, M, F.out_ptr, F.nnz, key_out, tgt, F.pos_out);
        rc = check_launch("k_count_above");
        if (rc != LGCN_OK) return rc;
    }
    if (!(stages & LGCN_RANKPOS_FINISH)) return rc;
    k_finish<D><<<dim3(static_cast<unsigned>(Q)), 64, 0, s>>>(F);
    rc = check_launch("k_finish");
    if (rc != LGCN_OK || !F.seen_ptr) return rc;
    k_finish_long<D><<<dim3(static_cast<unsigned>((Q + kFinishWaves - 1) / kFinishWaves)), 64 * kFinishWaves, 0, s>>>(F);
    return check_launch("k_finish_long");
}

}  // namespace

extern "C" {

int lgcn_rank_positions_workspace_size(int64_t Q, int64_t nnz, size_t* bytes) {
    if (!bytes || Q < 0 || nnz < 0) return fail(LGCN_E_ARG, "lgcn_rank_positions_workspace_size: bad args");
    *bytes = align_up(static_cast<size_t>(nnz) * sizeof(int32_t), 256) + 256;  // the targets' checked indices
    return LGCN_OK;
}

int lgcn_rank_positions(const float* Qn, int64_t Qpad, int64_t Q, const float* Cn, int64_t M, int32_t D,
                        const int64_t* truth_ptr, const int32_t* truth_idx, const int64_t* truth_row,
                        int64_t truth_rows, const int64_t* seen_ptr, const int32_t* seen_idx,
                        const int64_t* seen_row, int64_t seen_rows, const int64_t* out_ptr, int64_t nnz,
                        int32_t* pos_out, uint32_t* key_out, int32_t* eligible_out, void* workspace,
                        size_t workspace_bytes, int32_t stages, lgcn_stream_t stream) {
    const char* me = "lgcn_rank_positions";
    if (!Qn) return fail(LGCN_E_ARG, "%s: Qn is null", me);
    if (!Cn) return fail(LGCN_E_ARG, "%s: Cn is null", me);
    if (!truth_ptr) return fail(LGCN_E_ARG, "%s: truth_ptr is null", me);
    if (!truth_idx) return fail(LGCN_E_ARG, "%s: truth_idx is null", me);
    if (seen_ptr && !seen_idx) return fail(LGCN_E_ARG, "%s: seen_idx is null while seen_ptr is set", me);
    if (!out_ptr) return fail(LGCN_E_ARG, "%s: out_ptr is null", me);
    if (!pos_out) return fail(LGCN_E_ARG, "%s: pos_out is null", me);
    if (!key_out) return fail(LGCN_E_ARG, "%s: key_out is null", me);
    if (!eligible_out) return fail(LGCN_E_ARG, "%s: eligible_out is null", me);
    if (Q < 0 || Qpad < Q || Qpad > INT32_MAX)
        return fail(LGCN_E_ARG, "%s: Q=%lld / Qpad=%lld", me, (long long)Q, (long long)Qpad);
    if (Qpad % 128 != 0) return fail(LGCN_E_ARG, "%s: padded query count %lld not a multiple of 128", me, (long long)Qpad);
    if (M < 0 || M > INT32_MAX) return fail(LGCN_E_ARG, "%s: M=%lld", me, (long long)M);
    if (nnz < 0) return fail(LGCN_E_ARG, "%s: nnz=%lld", me, (long long)nnz);
    if (stages < 1 || stages > LGCN_RANKPOS_ALL) return fail(LGCN_E_ARG, "%s: stages=%d outside [1, %d]", me, stages, LGCN_RANKPOS_ALL);
    if (truth_rows < 0) return fail(LGCN_E_ARG, "%s: truth_rows=%lld", me, (long long)truth_rows);
    if (seen_ptr && seen_rows < 0) return fail(LGCN_E_ARG, "%s: seen_rows=%lld", me, (long long)seen_rows);
    if (reinterpret_cast<uintptr_t>(Qn) % 16 != 0) return fail(LGCN_E_ARG, "%s: Qn is not 16-byte aligned", me);
    if (reinterpret_cast<uintptr_t>(Cn) % 16 != 0) return fail(LGCN_E_ARG, "%s: Cn is not 16-byte aligned", me);
    if (D != 8 && D != 16 && D != 32 && D != 64 && D != 128 && D != 256)
        return fail(LGCN_E_UNSUPPORTED, "%s: D=%d (use lgcn_recall_width)", me, D);
    if (Q == 0 || nnz == 0) return LGCN_OK;
    size_t need = 0;
    lgcn_rank_positions_workspace_size(Q, nnz, &need);
    Carver cv{static_cast<char*>(workspace), workspace_bytes};
    int32_t* tgt = cv.take<int32_t>(static_cast<size_t>(nnz));
    if (!cv.ok)
        return fail(LGCN_E_WORKSPACE, "%s: workspace of %zu bytes, need %zu (or it is null)", me, workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0)
        return fail(LGCN_E_ARG, "%s: workspace is not 256-byte aligned", me);
    hipStream_t s = as_stream(stream);
    const FinishArgs F{Qn, Q, Cn, M, seen_ptr, seen_idx, seen_row, seen_rows, out_ptr, nnz, key_out, tgt, pos_out,
                       eligible_out};
#define LGCN_RANKPOS_ARGS Qn, Qpad, Q, Cn, M, truth_ptr, truth_idx, truth_row, truth_rows, F, key_out, tgt, stages, s
    switch (D) {
        case 8: return launch_positions<8>(LGCN_RANKPOS_ARGS);
        case 16: return launch_positions<16>(LGCN_RANKPOS_ARGS);
        case 32: return launch_positions<32>(LGCN_RANKPOS_ARGS);
        case 64: return launch_positions<64>(LGCN_RANKPOS_ARGS);
        case 128: return launch_positions<128>(LGCN_RANKPOS_ARGS);
        default: return launch_positions<256>(LGCN_RANKPOS_ARGS);
    }
#undef LGCN_RANKPOS_ARGS
}

}  // extern "C"
