// The 32-query x 32-candidate f32 score tile that lgcn_recall.hip's k_score_filter and
// lgcn_rankpos.hip's k_count_above stream the candidates through, and the key a score becomes. One
// definition each, so the position count's keys are the filter's bit for bit and a change of the
// tiling is made once.
//
// Workgroup = 4 waves over the same candidate blocks; wave w owns the 32 queries
// [(qg*4 + w)*32, +32), held in registers for the whole launch. Lane l = (i = l&31, h = l>>5)
// holds, for MFMA step s, A = Q[i][h*D/2 + s] and B = C[j][h*D/2 + s], so each step's 2-wide k
// slice is columns s and D/2+s and the D/2 steps cover the row (v_mfma_f32_32x32x2_f32, exact f32).
// Candidate blocks (32 rows) are staged through LDS, double-buffered: the global loads of block
// n+1 are in flight (in registers) while block n's MFMAs run, and land in the other buffer.
// At <= 170 VGPRs two waves share each SIMD, so one wave's epilogue hides under the other's MFMAs.
// D = 256 asks for one: its two candidate buffers + the kernel's own LDS (≈ 89 KB per workgroup in
// the filter) leave room for one workgroup (one wave per SIMD) per CU whatever the register count.
//
// A kernel owns the two LDS buffers (__shared__ float cs[2][ScoreTile<D>::kLdsFloats]) and its
// barriers, and per candidate block of its chunk runs
//     fetch(next block) -> scores(cs, this buffer) -> its epilogue -> land(cs, the other) -> barrier.
#pragma once

#include "lgcn_common.h"
#include "lgcn_ragged.h"

namespace lgcn {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ordered_key with every NaN first (the highest key)
__device__ __forceinline__ uint32_t score_key(float s) { return s != s ? 0xFFFFFFFFu : ordered_key(s); }

// inverse of score_key (the NaN key maps back to a NaN)
__device__ __forceinline__ float key_score(uint32_t k) { return ordered_value(k); }

// Per-candidate score boosts (lgcn_score_filter_boost, lgcn_score_lists_boost): a boosted kernel's one
// extra argument, and nothing at all in the unboosted instantiation (an empty record takes no kernel
// argument, so that one keeps the argument block it had).
template <bool kBoost>
struct BoostArgs {};
template <>
struct BoostArgs<true> {
    const float* boost;  // [M] f32, by candidate index
};

// the key of a boosted pair: ONE IEEE f32 addition (the library is built with -ffp-contract=off),
// then the key of the sum. b = -0.0 gives score_key(s) for every s, NaN and -0 included.
__device__ __forceinline__ uint32_t boosted_key(float s, float b) { return score_key(__fadd_rn(s, b)); }

constexpr int kTileQueries = 4 * 32;  // queries per workgroup

template <int D>
struct ScoreTile {
    static constexpr int H = D / 2;
    static constexpr int ROWF = D + 4;      // padded LDS row: conflict-free ds_read_b128 down a column
    static constexpr int NF4 = 32 * D / 4;  // float4s per candidate block
    static constexpr int PER = (NF4 + kBlock - 1) / kBlock;
    static constexpr int kLdsFloats = 32 * ROWF;      // one candidate buffer
    static constexpr int kWaves = D >= 256 ? 1 : 2;   // per SIMD (__launch_bounds__)

    float a[H];      // this lane's half of query q0 + i
    float4 pre[PER];  // the block in flight

    // Grid: 1-D, XCD-aware (score_grid below sizes it). Workgroup wid runs on XCD wid % 8; the query
    // groups of one candidate chunk get consecutive slots of the SAME XCD, so they run together and
    // share its L2 copy of the chunk's rows (the queries, not the candidates, are what differs
    // between them). chunk: the first candidate block of the workgroup, which then takes every
    // nchunk-th; q0: the first query of the calling wave.
    static __device__ __forceinline__ void place(int32_t nqg, int& chunk, int64_t& q0) {
        const int wid = blockIdx.x;
        const int slot = wid >> 3;
        const int qg = slot % nqg;
        chunk = (slot / nqg) * 8 + (wid & 7);
        q0 = (int64_t(qg) * 4 + (threadIdx.x >> 6)) * 32;
    }

    // the query row a lane of half h holds in accumulator r
    static __device__ __forceinline__ int row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

    __device__ __forceinline__ void load_queries(const float* __restrict__ Qn, int64_t q0) {
        const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
        const float4* src = reinterpret_cast<const float4*>(Qn + (q0 + i) * D + h * H);
#pragma unroll
        for (int v = 0; v < H / 4; ++v) {
            const float4 t = src[v];
            a[4 * v] = t.x;
            a[4 * v + 1] = t.y;
            a[4 * v + 2] = t.z;
            a[4 * v + 3] = t.w;
        }
    }

    // candidate block cb (rows cb*32 .. +31 of the M, `stride` rows of Cn apart; zeros past M) into
    // registers, and from there into buffer b of the kernel's two (the buffer goes by index, not by
    // pointer: k_count_above<64> spills one more register on a pointer that is swapped per block)
    __device__ __forceinline__ void fetch(const float* __restrict__ Cn, int64_t M, int64_t stride, int64_t cb) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int t = threadIdx.x + p * kBlock;
            const int r = t / (D / 4), c4 = t % (D / 4);
            const int64_t j = cb * 32 + r;
            pre[p] = (t < NF4 && j < M) ? reinterpret_cast<const float4*>(Cn + j * stride * D)[c4]
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ __forceinline__ void land(float (*cs)[kLdsFloats], int b) const {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int t = threadIdx.x + p * kBlock;
            if (t < NF4) *reinterpret_cast<float4*>(&cs[b][(t / (D / 4)) * ROWF + (t % (D / 4)) * 4]) = pre[p];
        }
    }

    // The wave's 32 queries against the 32 candidates of buffer b. A lane's accumulator r is the
    // score of query row(r, h) and candidate i (its column).
    __device__ __forceinline__ f32x16 scores(const float (*cs)[kLdsFloats], int b) const {
        const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* brow = &cs[b][i * ROWF + h * H];
        // B in groups of G float4 per LDS wait (G*4 MFMAs behind each wait)
        constexpr int G = (H / 4) >= 4 ? 4 : (H / 4);
#pragma unroll
        for (int v0 = 0; v0 < H / 4; v0 += G) {
            float4 bv[G];
#pragma unroll
            for (int g = 0; g < G; ++g) bv[g] = *reinterpret_cast<const float4*>(brow + 4 * (v0 + g));
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int v = v0 + g;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * v], bv[g].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * v + 1], bv[g].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * v + 2], bv[g].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * v + 3], bv[g].w, acc, 0, 0, 0);
            }
        }
        return acc;
    }

    // The keys of ONE query against 32 candidates, one per lane pair: lane (i, h) passes candidate
    // i's index (-1: none, a zero row) and gets candidate i's key. One tile of the chain above with
    // every A row the query, operands from global memory: step s covers columns s and D/2 + s in the
    // same order, so the key is the one scores() gives that pair. Called by whole waves.
    static __device__ __forceinline__ uint32_t row_keys(const float* __restrict__ qrow, const float* __restrict__ Cn,
                                                        int32_t cand, int h) {
        const float4* a4 = reinterpret_cast<const float4*>(qrow + h * H);
        const float4* b4 = reinterpret_cast<const float4*>(Cn + static_cast<int64_t>(cand < 0 ? 0 : cand) * D + h * H);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int v = 0; v < H / 4; ++v) {
            const float4 qa = a4[v];
            const float4 b = cand >= 0 ? b4[v] : make_float4(0.f, 0.f, 0.f, 0.f);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.w, b.w, acc, 0, 0, 0);
        }
        return score_key(acc[0]);  // row 4h of the tile, column i: every row is the query
    }

    // Lane (i, h)'s half of row `row` of a table of D-wide rows, as row_keys reads it from memory:
    // float4 v holds columns h*D/2 + 4v .. 4v + 3. row < 0: none, zeros (nothing is read).
    static __device__ __forceinline__ void load_half(const float* __restrict__ rows, int64_t row, int h,
                                                     float4 (&v)[H / 4]) {
        const float4* src = reinterpret_cast<const float4*>(rows + (row < 0 ? 0 : row) * D + h * H);
#pragma unroll
        for (int x = 0; x < H / 4; ++x) v[x] = row >= 0 ? src[x] : make_float4(0.f, 0.f, 0.f, 0.f);
    }

    // row_keys on operands already in registers (load_half's): qa the query's half, b the half of
    // candidate i's row. The same tile, the same steps in the same order, so the same key; a caller
    // keeps qa for a whole row of candidates and has the next b in flight while this chain runs
    // (lgcn_recall_among.hip).
    static __device__ __forceinline__ uint32_t row_keys(const float4 (&qa)[H / 4], const float4 (&b)[H / 4]) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int v = 0; v < H / 4; ++v) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[v].x, b[v].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[v].y, b[v].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[v].z, b[v].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[v].w, b[v].w, acc, 0, 0, 0);
        }
        return score_key(acc[0]);
    }
};

// The launch of a tile kernel over nqg >= 1 query groups and M > 0 candidates: candidate chunks are a
// multiple of 8 (the XCD mapping), ~2048 workgroups in all. False when the grid does not fit a launch.
inline bool score_grid(int64_t nqg, int64_t M, int32_t& nchunk, unsigned& grid) {
    const int64_t nblk = (M + 31) / 32;
    int64_t nc = (2048 / nqg + 7) / 8 * 8;
    const int64_t need = (nblk + 7) / 8 * 8;
    if (nc > need) nc = need;
    if (nc < 8) nc = 8;
    if (nqg * nc > INT32_MAX) return false;  // nqg too, then: nc >= 8
    nchunk = static_cast<int32_t>(nc);
    grid = static_cast<unsigned>(nqg * nc);
    return true;
}

}  // namespace lgcn
