// Full-ranking evaluation counts on gfx950 (lgcn_rank_metrics): ranked candidate lists plus a
// held-out (truth) CSR in, per-query hit counts, DCG sums, first hit rank and truth length out.
//
//   k_rank_metrics   one wave per query, four queries per 256-thread workgroup. The wave walks the
//                    query's k ranks 64 at a time: each lane loads its candidate index (coalesced)
//                    and binary-searches the query's sorted truth row (sorted_contains, as
//                    k_select_ranked does on its exclusion row); a ballot gives the step's 64-bit hit mask. Per
//                    cutoff the hit count is a popcount of the mask under "ranks below the
//                    cutoff" and the lane adds its discount 1 / log2(rank + 2) to a float64
//                    partial. One butterfly reduction at the end, lane 0 stores.
//
// Every cutoff is served by the one pass; the cutoffs arrive by value in a kernel argument, so the
// entry point allocates nothing and copies nothing. No LDS, no atomics, no waiting on other
// workgroups. The DCG is formed and summed in float64 and rounded to float32 once, on store: the
// stored value is within one float32 ulp of the exact sum whatever the reduction order.
#include "lgcn_common.h"
#include "lgcn_ragged.h"

namespace lgcn {

constexpr int kMetricCutoffs = LGCN_METRICS_MAX_CUTOFFS;
constexpr int kMetricWaves = kBlock / 64;  // queries per workgroup

struct MetricCutoffs {
    int32_t n;
    int32_t c[kMetricCutoffs];
};

__global__ __launch_bounds__(kBlock) void k_rank_metrics(
    const int32_t* __restrict__ ranked_idx, int64_t ld, int32_t k, int64_t Q, const int64_t* __restrict__ truth_ptr,
    const int32_t* __restrict__ truth_idx, const int64_t* __restrict__ truth_row, int64_t truth_rows,
    MetricCutoffs cut, int32_t* __restrict__ hits_out, float* __restrict__ dcg_out, int32_t* __restrict__ first_out,
    int32_t* __restrict__ ntruth_out) {
    const int lane = threadIdx.x & 63;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kMetricWaves + (threadIdx.x >> 6);
    if (q >= Q) return;  // whole waves leave; nothing below synchronises across waves
    // this query's truth row (a row outside [0, truth_rows) is an empty set)
    int64_t tb, te;
    ragged_row(q, truth_ptr, truth_row, truth_rows, tb, te);
    const int32_t* tr = truth_idx + tb;
    const int64_t tn = te - tb;
    const int32_t* ranked = ranked_idx + q * ld;
    int32_t hits[kMetricCutoffs];
    double dcg[kMetricCutoffs];
#pragma unroll
    for (int c = 0; c < kMetricCutoffs; ++c) {
        hits[c] = 0;
        dcg[c] = 0.0;
    }
    int32_t first = INT32_MAX;
    if (tn > 0) {
        for (int32_t base = 0; base < k; base += 64) {
            const int32_t r = base + lane;
            bool hit = false;
            if (r < k) {
                const int32_t cand = ranked[r];
                if (cand >= 0) hit = sorted_contains(tr, tn, cand);  // the -1 tail of a short list is never a hit
            }
            const unsigned long long mask = __ballot(hit);
            if (mask == 0ull) continue;  // wave-uniform
            const double disc = hit ? 1.0 / log2(static_cast<double>(r + 2)) : 0.0;
            if (hit && r < first) first = r;
#pragma unroll
            for (int c = 0; c < kMetricCutoffs; ++c) {
                if (c < cut.n) {  // wave-uniform
                    const int32_t rem = cut.c[c] - base;  // ranks of this step below the cutoff
                    const unsigned long long below = rem >= 64 ? ~0ull : rem <= 0 ? 0ull : (1ull << rem) - 1ull;
                    hits[c] += __popcll(mask & below);
                    if (r < cut.c[c]) dcg[c] += disc;
                }
            }
        }
    }
    // one butterfly over the 64 lanes: every lane ends with the sums (hits are wave-uniform already)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int32_t o = __shfl_xor(first, off, 64);
        first = o < first ? o : first;
#pragma unroll
        for (int c = 0; c < kMetricCutoffs; ++c)
            if (c < cut.n) dcg[c] += __shfl_xor(dcg[c], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kMetricCutoffs; ++c) {
            if (c < cut.n) {
                hits_out[q * cut.n + c] = hits[c];
                dcg_out[q * cut.n + c] = static_cast<float>(dcg[c]);  // the one rounding
            }
        }
        first_out[q] = first == INT32_MAX ? -1 : first;
        ntruth_out[q] = static_cast<int32_t>(tn > INT32_MAX ? INT32_MAX : tn);
    }
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int lgcn_rank_metrics(const int32_t* ranked_idx, int64_t ld, int32_t k, int64_t Q, const int64_t* truth_ptr,
                      const int32_t* truth_idx, const int64_t* truth_row, int64_t truth_rows, const int32_t* cutoffs,
                      int32_t n_cutoffs, int32_t* hits_out, float* dcg_out, int32_t* first_out, int32_t* ntruth_out,
                      lgcn_stream_t stream) {
    const char* me = "lgcn_rank_metrics";
    if (!ranked_idx) return fail(LGCN_E_ARG, "%s: ranked_idx is null", me);
    if (!truth_ptr) return fail(LGCN_E_ARG, "%s: truth_ptr is null", me);
    if (!truth_idx) return fail(LGCN_E_ARG, "%s: truth_idx is null", me);
    if (!cutoffs) return fail(LGCN_E_ARG, "%s: cutoffs is null", me);
    if (!hits_out) return fail(LGCN_E_ARG, "%s: hits_out is null", me);
    if (!dcg_out) return fail(LGCN_E_ARG, "%s: dcg_out is null", me);
    if (!first_out) return fail(LGCN_E_ARG, "%s: first_out is null", me);
    if (!ntruth_out) return fail(LGCN_E_ARG, "%s: ntruth_out is null", me);
    if (k < 1 || k > LGCN_RANKED_MAX_K) return fail(LGCN_E_ARG, "%s: k=%d outside [1, %d]", me, k, LGCN_RANKED_MAX_K);
    if (ld < k) return fail(LGCN_E_ARG, "%s: ld=%lld < k=%d", me, (long long)ld, k);
    if (Q < 0) return fail(LGCN_E_ARG, "%s: Q=%lld", me, (long long)Q);
    if (truth_rows < 0) return fail(LGCN_E_ARG, "%s: truth_rows=%lld", me, (long long)truth_rows);
    if (n_cutoffs < 1 || n_cutoffs > kMetricCutoffs)
        return fail(LGCN_E_ARG, "%s: n_cutoffs=%d outside [1, %d]", me, n_cutoffs, kMetricCutoffs);
    MetricCutoffs cut;
    cut.n = n_cutoffs;
    for (int c = 0; c < kMetricCutoffs; ++c) {
        cut.c[c] = c < n_cutoffs ? cutoffs[c] : 0;
        if (c >= n_cutoffs) continue;
        if (cut.c[c] < 1 || cut.c[c] > k)
            return fail(LGCN_E_ARG, "%s: cutoffs[%d]=%d outside [1, k=%d]", me, c, cut.c[c], k);
        if (c > 0 && cut.c[c] <= cut.c[c - 1])
            return fail(LGCN_E_ARG, "%s: cutoffs[%d]=%d not above cutoffs[%d]=%d (strictly ascending)", me, c, cut.c[c],
                        c - 1, cut.c[c - 1]);
    }
    const int64_t grid = (Q + kMetricWaves - 1) / kMetricWaves;
    if (grid > INT32_MAX) return fail(LGCN_E_ARG, "%s: Q=%lld is too many queries for one launch", me, (long long)Q);
    if (Q == 0) return LGCN_OK;
    k_rank_metrics<<<dim3(static_cast<unsigned>(grid)), kBlock, 0, as_stream(stream)>>>(
        ranked_idx, ld, k, Q, truth_ptr, truth_idx, truth_row, truth_rows, cut, hits_out, dcg_out, first_out,
        ntruth_out);
    return check_launch("k_rank_metrics");
}

}  // extern "C"
