// Fold-in on gfx950 (lgcn_foldin_rows): the row of a node the model never saw, as one more
// propagation over its own edges would give it. Per query a history row of a CSR in, the weighted sum
// of the table rows it names out:
//     out[q] = s_q * sum_e (hist_w[e] * isd[i_e]) * table[i_e],   s_q = 1 / sqrt(eligible entries)
// A ragged gather-sum: every byte it moves is a table row read once, so the shape follows the loads.
//
//   foldin_sum       the sum over the entries [beg, end) of one history, by one wave. A row of d
//                    columns is P = pow2 >= ceil(d / 4) lanes of four columns each (16 lanes of
//                    float4 at d = 64), so the wave holds G = 64 / P lane groups and one
//                    wave-instruction fetches G rows. Group g takes the entries beg + g, + G, + 2 G ...
//                    in ascending order into one accumulator per column; a step issues the rows of
//                    kFoldinDepth entries per group (8 G rows in flight per wave: 32 at d = 64) before
//                    it adds the first, and the item indices and weights of the NEXT step travel with
//                    them, so a step waits for one memory round trip, not for two in a row.
//                    An entry outside [0, M) is skipped: neither isd nor the table is read for it.
//   foldin_groups    the G groups' sums and counts combined by an exchange butterfly (P, 2 P, ... 32):
//                    a fixed tree, the same bits on every lane since a + b == b + a.
//   k_foldin_rows        one wave per history, four histories per 256-thread workgroup: every
//                        history of at most kFoldinLong entries.
//   k_foldin_rows_long   a 512-thread workgroup per eight consecutive queries: those among them with
//                        a longer history, one after the other. The history is cut into chunks of
//                        kFoldinChunk entries, wave w of the eight sums the chunks w, w + 8, ... (one
//                        running sum, chunk after chunk), and wave 0 adds the eight sums in wave
//                        order through LDS. A workgroup without a long history ends after reading
//                        eight row lengths; nothing is read back to find the long rows.
//
// The summation order is a function of (history length, d) alone: which lane group and which wave
// takes an entry follows from its position in the row, never from the query's place in the batch,
// the table's alignment or what else runs. Rows whose table cannot be read as float4 (d, ldt or the
// base address not a multiple of four floats) take scalar loads of the same columns on the same
// lanes, so the bits do not depend on the view either. No atomics, no waiting on other workgroups,
// nothing allocated, stream-ordered; the two launches write disjoint queries.
//
// Why eight waves and no workspace: ML-25M-shaped histories have mean 77 and longest 31,703. One
// wave for that row would run some 4,000 dependent steps while the rest of the chip is long done;
// eight waves with 32 rows each in flight cut it to about 125 round trips at d = 64. Spreading one
// history over several workgroups would need a workspace for their partial sums and a third launch;
// DESIGN.md §15 has the measured share of the longest history.
#include "lgcn_common.h"
#include "lgcn_ragged.h"

#include <cmath>

#pragma clang fp contract(off)

namespace lgcn {

constexpr int kFoldinWaves = 8;                  // waves that share a long history
constexpr int kFoldinLong = LGCN_FOLDIN_LONG;    // history entries above which they do
constexpr int kFoldinChunk = LGCN_FOLDIN_CHUNK;  // entries of a chunk of a long history
constexpr int kFoldinDepth = 8;                  // rows a lane has in flight
constexpr int kFoldinShort = 4;                  // histories (waves) per workgroup of k_foldin_rows

static_assert(kFoldinChunk % 64 == 0, "a chunk starts on lane group 0 whatever the row width");
static_assert(LGCN_FOLDIN_MAX_D == 256, "a row is at most 64 lanes of four columns");

struct FoldinTable {
    const float* table;
    const float* isd;
    int64_t M, ldt;
    int32_t d;
};

// Adds this lane's share of the entries [beg, end) to acc (columns 4 p .. 4 p + 3 of the entries
// beg + g, beg + g + G, ...) and their eligible count to cnt. p = lane % P, g = lane / P, G = 64 / P.
// VEC: the rows can be read as float4. Every load of a step is issued before anything uses one (a
// use between two loads makes the second wait for the first): the next step's indices and weights are
// fetched unconditionally from a clamped position and judged a step later, when they have arrived.
template <bool VEC>
__device__ __forceinline__ void foldin_sum(const FoldinTable& T, const int32_t* __restrict__ hist_idx,
                                           const float* __restrict__ hist_w, int64_t beg, int64_t end, int p, int g,
                                           int G, float (&acc)[4], int32_t& cnt) {
    if (beg >= end) return;  // wave-uniform
    const int c0 = 4 * p;
    const bool lane_on = c0 < T.d;
    const bool has_f = hist_w != nullptr || T.isd != nullptr;
    const uint32_t ldt32 = static_cast<uint32_t>(T.ldt);
    int32_t ni[kFoldinDepth];  // the next step's items and weights as loaded (of entry end - 1 past the end)
    float nw[kFoldinDepth];
    auto entries = [&](int64_t e0) {
#pragma unroll
        for (int u = 0; u < kFoldinDepth; ++u) {
            int64_t e = e0 + static_cast<int64_t>(u) * G + g;
            e = e < end ? e : end - 1;
            ni[u] = hist_idx[e];
            nw[u] = hist_w ? hist_w[e] : 1.f;
        }
    };
    const int64_t step = static_cast<int64_t>(kFoldinDepth) * G;
    entries(beg);
    for (int64_t e0 = beg; e0 < end; e0 += step) {  // wave-uniform
        int32_t it[kFoldinDepth];  // this step's items (-1: none, or outside [0, M) and never read)
        float fw[kFoldinDepth], fs[kFoldinDepth];
        float4 v[kFoldinDepth];
        uint64_t off[kFoldinDepth];  // every row offset first, then nothing but loads
#pragma unroll
        for (int u = 0; u < kFoldinDepth; ++u) {
            const bool in = e0 + static_cast<int64_t>(u) * G + g < end;
            it[u] = in && ni[u] >= 0 && static_cast<int64_t>(ni[u]) < T.M ? ni[u] : -1;
            fw[u] = nw[u];
            // one 32 x 32 -> 64 bit product: the entry point holds ldt below 2^31
            off[u] = static_cast<uint64_t>(static_cast<uint32_t>(ni[u])) * ldt32 + c0;
        }
        // Pin the step's items and offsets here. The loads below sit in branches, and the wait counter
        // is in order: a wait for an index placed between two of them would wait for the rows as well.
#pragma unroll
        for (int u = 0; u < kFoldinDepth; ++u) asm volatile("" : "+v"(it[u]), "+v"(off[u]));
#pragma unroll
        for (int u = 0; u < kFoldinDepth; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            fs[u] = 1.f;
            if (it[u] >= 0) {
                if (T.isd) fs[u] = T.isd[it[u]];
                if (lane_on) {
                    const float* row = T.table + off[u];
                    if (VEC) {
                        v[u] = *reinterpret_cast<const float4*>(row);
                    } else {
                        v[u].x = row[0];
                        if (c0 + 1 < T.d) v[u].y = row[1];
                        if (c0 + 2 < T.d) v[u].z = row[2];
                        if (c0 + 3 < T.d) v[u].w = row[3];
                    }
                }
            }
        }
        entries(e0 + step);  // in flight while this step adds (unconditional: the wait counter stays exact)
#pragma unroll
        for (int u = 0; u < kFoldinDepth; ++u) {
            if (it[u] >= 0) {
                float4 t = v[u];
                if (has_f) {
                    const float f = hist_w ? (T.isd ? fw[u] * fs[u] : fw[u]) : fs[u];
                    t.x = f * t.x;
                    t.y = f * t.y;
                    t.z = f * t.z;
                    t.w = f * t.w;
                }
                acc[0] += t.x;
                acc[1] += t.y;
                acc[2] += t.z;
                acc[3] += t.w;
                ++cnt;
            }
        }
    }
}

// the G lane groups' sums and counts, combined: afterwards every lane p of every group holds them
__device__ __forceinline__ void foldin_groups(int P, float (&acc)[4], int32_t& cnt) {
    for (int off = P; off < 64; off <<= 1) {  // wave-uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
        cnt += __shfl_xor(cnt, off, 64);
    }
}

// out[q, 4 p .. 4 p + 3] = s * acc, by the lanes of group 0 (exact zeros for an empty history)
__device__ __forceinline__ void foldin_store(int64_t q, int p, int g, const float (&acc)[4], int32_t n, int32_t d,
                                             float* __restrict__ out, int64_t ldo, bool vec_out,
                                             int32_t* __restrict__ out_n) {
    if (g != 0) return;
    const int c0 = 4 * p;
    if (p == 0 && out_n) out_n[q] = n;
    if (c0 >= d) return;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) {
        const float s = static_cast<float>(1.0 / sqrt(static_cast<double>(n)));
        r = make_float4(s * acc[0], s * acc[1], s * acc[2], s * acc[3]);
    }
    float* o = out + q * ldo + c0;
    if (vec_out) {
        *reinterpret_cast<float4*>(o) = r;
    } else {
        o[0] = r.x;
        if (c0 + 1 < d) o[1] = r.y;
        if (c0 + 2 < d) o[2] = r.z;
        if (c0 + 3 < d) o[3] = r.w;
    }
}

template <bool VEC>
__global__ __launch_bounds__(64 * kFoldinShort) void k_foldin_rows(
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w,
    const int64_t* __restrict__ hist_row, int64_t hist_rows, int64_t Q, FoldinTable T, int P, int shift,
    float* __restrict__ out, int64_t ldo, bool vec_out, int32_t* __restrict__ out_n) {
    const int lane = threadIdx.x & 63;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kFoldinShort + (threadIdx.x >> 6);
    if (q >= Q) return;  // wave-uniform, and no barrier follows
    int64_t beg, end;
    ragged_row(q, hist_ptr, hist_row, hist_rows, beg, end);
    if (end - beg > kFoldinLong) return;  // k_foldin_rows_long's
    const int p = lane & (P - 1), g = lane >> shift;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t cnt = 0;
    foldin_sum<VEC>(T, hist_idx, hist_w, beg, end, p, g, 64 >> shift, acc, cnt);
    foldin_groups(P, acc, cnt);
    foldin_store(q, p, g, acc, cnt, T.d, out, ldo, vec_out, out_n);
}

template <bool VEC>
__global__ __launch_bounds__(64 * kFoldinWaves) void k_foldin_rows_long(
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, const float* __restrict__ hist_w,
    const int64_t* __restrict__ hist_row, int64_t hist_rows, int64_t Q, FoldinTable T, int P, int shift,
    float* __restrict__ out, int64_t ldo, bool vec_out, int32_t* __restrict__ out_n) {
    __shared__ float part[kFoldinWaves - 1][LGCN_FOLDIN_MAX_D];
    __shared__ int32_t pcnt[kFoldinWaves - 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = lane & (P - 1), g = lane >> shift;
    for (int i = 0; i < kFoldinWaves; ++i) {  // workgroup-uniform throughout
        const int64_t q = static_cast<int64_t>(blockIdx.x) * kFoldinWaves + i;
        if (q >= Q) break;
        int64_t beg, end;
        ragged_row(q, hist_ptr, hist_row, hist_rows, beg, end);
        if (end - beg <= kFoldinLong) continue;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int32_t cnt = 0;
        for (int64_t b = beg + static_cast<int64_t>(wv) * kFoldinChunk; b < end;
             b += static_cast<int64_t>(kFoldinWaves) * kFoldinChunk) {
            const int64_t e = b + kFoldinChunk < end ? b + kFoldinChunk : end;
            foldin_sum<VEC>(T, hist_idx, hist_w, b, e, p, g, 64 >> shift, acc, cnt);
        }
        foldin_groups(P, acc, cnt);
        __syncthreads();  // the workgroup's previous long history is done with the LDS
        if (wv > 0 && g == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) part[wv - 1][4 * p + j] = acc[j];  // 4 p + 3 < 4 * 64
            if (p == 0) pcnt[wv - 1] = cnt;
        }
        __syncthreads();
        if (wv == 0) {
            for (int w = 0; w < kFoldinWaves - 1; ++w) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += part[w][4 * p + j];
                cnt += pcnt[w];
            }
            foldin_store(q, p, g, acc, cnt, T.d, out, ldo, vec_out, out_n);
        }
    }
}

}  // namespace lgcn

using namespace lgcn;

namespace {

template <bool VEC>
int launch_foldin(const int64_t* hist_ptr, const int32_t* hist_idx, const float* hist_w, const int64_t* hist_row,
                  int64_t hist_rows, int64_t Q, const FoldinTable& T, int P, int shift, float* out, int64_t ldo,
                  bool vec_out, int32_t* out_n, hipStream_t s) {
    const unsigned short_groups = static_cast<unsigned>((Q + kFoldinShort - 1) / kFoldinShort);
    k_foldin_rows<VEC><<<dim3(short_groups), 64 * kFoldinShort, 0, s>>>(hist_ptr, hist_idx, hist_w, hist_row, hist_rows,
                                                                       Q, T, P, shift, out, ldo, vec_out, out_n);
    int rc = check_launch("k_foldin_rows");
    if (rc != LGCN_OK) return rc;
    const unsigned long_groups = static_cast<unsigned>((Q + kFoldinWaves - 1) / kFoldinWaves);
    k_foldin_rows_long<VEC><<<dim3(long_groups), 64 * kFoldinWaves, 0, s>>>(
        hist_ptr, hist_idx, hist_w, hist_row, hist_rows, Q, T, P, shift, out, ldo, vec_out, out_n);
    return check_launch("k_foldin_rows_long");
}

}  // namespace

extern "C" {

int lgcn_foldin_rows(const int64_t* hist_ptr, const int32_t* hist_idx, const float* hist_w, const int64_t* hist_row,
                     int64_t hist_rows, int64_t Q, const float* table, int64_t M, int32_t d, int64_t ldt,
                     const float* isd, float* out, int64_t ldo, int32_t* out_n, lgcn_stream_t stream) {
    const char* me = "lgcn_foldin_rows";
    if (!hist_ptr) return fail(LGCN_E_ARG, "%s: hist_ptr is null", me);
    if (!hist_idx) return fail(LGCN_E_ARG, "%s: hist_idx is null", me);
    if (!table) return fail(LGCN_E_ARG, "%s: table is null", me);
    if (!out) return fail(LGCN_E_ARG, "%s: out is null", me);
    if (Q < 0) return fail(LGCN_E_ARG, "%s: Q=%lld", me, (long long)Q);
    if (M < 0) return fail(LGCN_E_ARG, "%s: M=%lld", me, (long long)M);
    if (hist_rows < 0) return fail(LGCN_E_ARG, "%s: hist_rows=%lld", me, (long long)hist_rows);
    if (d < 1) return fail(LGCN_E_ARG, "%s: d=%d", me, d);
    if (d > LGCN_FOLDIN_MAX_D)
        return fail(LGCN_E_UNSUPPORTED, "%s: d=%d exceeds LGCN_FOLDIN_MAX_D=%d", me, d, LGCN_FOLDIN_MAX_D);
    if (ldt < d) return fail(LGCN_E_ARG, "%s: ldt=%lld below d=%d", me, (long long)ldt, d);
    if (ldo < d) return fail(LGCN_E_ARG, "%s: ldo=%lld below d=%d", me, (long long)ldo, d);
    if (ldt > INT32_MAX) return fail(LGCN_E_ARG, "%s: ldt=%lld is no row stride", me, (long long)ldt);
    if (Q > INT32_MAX) return fail(LGCN_E_ARG, "%s: Q=%lld is too many queries for one launch", me, (long long)Q);
    if (Q == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
    int P = 1, shift = 0;  // lanes of a row: the power of two at or above ceil(d / 4)
    while (4 * P < d) {
        P <<= 1;
        ++shift;
    }
    FoldinTable T;
    T.table = table;
    T.isd = isd;
    T.M = M;
    T.ldt = ldt;
    T.d = d;
    const bool vec = d % 4 == 0 && ldt % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0;
    const bool vec_out = d % 4 == 0 && ldo % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (vec)
        return launch_foldin<true>(hist_ptr, hist_idx, hist_w, hist_row, hist_rows, Q, T, P, shift, out, ldo, vec_out,
                                   out_n, s);
    return launch_foldin<false>(hist_ptr, hist_idx, hist_w, hist_row, hist_rows, Q, T, P, shift, out, ldo, vec_out,
                                out_n, s);
}

}  // extern "C"
