// Recall@k of the reference's evaluate() (reference utils/train_test.py:165-212) on gfx950.
//
// The reference scores sample_size sampled "user" rows against every positive and negative row
// of the edge set (cosine = mm of L2-normalised rows), takes torch.topk(k) per user and counts
// the hits that are positives (index < P). Per user, that count is all we need, so nothing of
// the [Q, M] score matrix is kept:
//
//   k_normalize_rows  x[r] / ||x[r]|| (optionally gathered through an index list), written into a
//                     zero-padded [rows, D] image (D = the compiled width >= d);
//   k_score_filter    f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32) scores of 32-query blocks
//                     against 32-candidate blocks (the tile of lgcn_scoretile.h); an epilogue keeps
//                     (key, index) of every score at or above the query's threshold key in a
//                     per-query list;
//   k_select_topk     one workgroup per query: radix select (4 x 8-bit passes) of the k-th
//                     largest key in its list, then either that key (a new threshold) or the
//                     hit count (positives above it, plus positives among the ties);
//   k_select_ranked   the same lists ranked for recommendation (reference utils/recommend.py):
//                     entries found in a per-query exclusion row dropped, the rest ordered by
//                     (key descending, index ascending); the k-th key or the k winners themselves.
//
// k_score_filter and k_select_ranked live in lgcn_recall_lists.h; this unit instantiates them
// unfiltered, lgcn_recall_attr.hip with the attribute filter.
//
// Thresholds come from a strided candidate subset first: the k-th largest score of ANY subset is
// <= the k-th largest of all M, so the filtered list always holds the true top k, and it holds
// about k * M / |subset| entries. If a list overflows its capacity, its kept entries are real
// candidates too, so their k-th largest is again a valid (tighter) threshold and the caller
// re-runs the filter (lgcn_amd.recall does this; it never happens at the reference's sizes).
//
// Ties at the k-th score take the lowest candidate indices first, which are the positives
// (torch.topk leaves tie order unspecified). NaN scores (zero rows, normalised as 0/0 like the
// reference) rank first, as torch.topk ranks NaN above every number.

#include "lgcn_recall_lists.h"

namespace {

// one 32-lane half-wave per row
__global__ __launch_bounds__(kBlock) void k_normalize_rows(const float* __restrict__ x, const int64_t* __restrict__ idx,
                                                           int64_t rows, int64_t ld, int32_t d,
                                                           float* __restrict__ out, int32_t D, int64_t out_rows) {
    const int64_t r = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / 32;
    const int l = threadIdx.x & 31;
    if (r >= out_rows) return;
    float* o = out + r * D;
    if (r >= rows) {  // padding rows: zeros
        for (int c = l; c < D; c += 32) o[c] = 0.f;
        return;
    }
    const float* src = x + (idx ? idx[r] : r) * ld;
    float ss = 0.f;
    for (int c = l; c < d; c += 32) {
        const float v = src[c];
        ss += v * v;
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 32);
    const float n = sqrtf(ss);
    for (int c = l; c < D; c += 32) o[c] = (c < d) ? src[c] / n : 0.f;
}

// k-th largest key per query list (radix select), then the threshold or the hit count.
__global__ __launch_bounds__(kSelBlock) void k_select_topk(const uint32_t* __restrict__ list_key,
                                                           const int32_t* __restrict__ list_idx,
                                                           const int32_t* __restrict__ list_n, int32_t dense_n,
                                                           int32_t cap, int32_t k, int64_t P, int64_t Qvalid,
                                                           uint32_t* __restrict__ thr_out, int32_t* __restrict__ hits_out) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_mask, s_k;
    __shared__ int32_t red[kSelBlock / 64][2];
    const int64_t q = blockIdx.x;
    if (q >= Qvalid) {
        if (threadIdx.x == 0) {
            if (thr_out) thr_out[q] = 0xFFFFFFFFu;
            if (hits_out) hits_out[q] = 0;
        }
        return;
    }
    int32_t n = list_n ? list_n[q] : dense_n;
    if (n > cap) n = cap;
    const uint32_t* keys = list_key + q * cap;
    const int32_t* idx = list_idx + q * cap;
    if (n < k) {  // cannot rank k: threshold "everything", hits invalid
        if (threadIdx.x == 0) {
            if (thr_out) thr_out[q] = 0u;
            if (hits_out) hits_out[q] = -1;
        }
        return;
    }
    if (threadIdx.x == 0) {
        s_prefix = 0u;
        s_mask = 0u;
        s_k = static_cast<uint32_t>(k);
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int t = threadIdx.x; t < 256; t += kSelBlock) hist[t] = 0u;
        __syncthreads();
        const uint32_t prefix = s_prefix, mask = s_mask;
        for (int e = threadIdx.x; e < n; e += kSelBlock) {
            const uint32_t key = keys[e];
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t cum = 0, kk = s_k;
            int bsel = 0;
            for (int bin = 255; bin >= 0; --bin) {
                if (cum + hist[bin] >= kk) {
                    bsel = bin;
                    break;
                }
                cum += hist[bin];
            }
            s_k = kk - cum;
            s_prefix = prefix | (static_cast<uint32_t>(bsel) << shift);
            s_mask = mask | (255u << shift);
        }
        __syncthreads();
    }
    const uint32_t T = s_prefix;
    const int32_t need = static_cast<int32_t>(s_k);  // taken from the keys equal to T
    if (thr_out && threadIdx.x == 0) thr_out[q] = T;
    if (!hits_out) return;
    int32_t above = 0, ties = 0;
    for (int e = threadIdx.x; e < n; e += kSelBlock) {
        const uint32_t key = keys[e];
        const bool pos = idx[e] < P;
        above += (key > T && pos) ? 1 : 0;
        ties += (key == T && pos) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        above += __shfl_xor(above, off, 64);
        ties += __shfl_xor(ties, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = above;
        red[threadIdx.x >> 6][1] = ties;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t A = 0, Ti = 0;
        for (int w = 0; w < kSelBlock / 64; ++w) {
            A += red[w][0];
            Ti += red[w][1];
        }
        hits_out[q] = A + (Ti < need ? Ti : need);
    }
}

// ---------------------------------------------------------------------------------------------
// CPU torch.topk's tie rule (lgcn_select_topk_stl). On CPU, the reference's torch.topk(scores, k)
// (utils/train_test.py:197) runs ATen's topk_impl_loop (TopKImpl.h): the row as (value, index)
// pairs, then std::partial_sort(k) when k * 64 <= M, else std::nth_element(k - 1), both with the
// comparator (isnan(x) && !isnan(y)) || x > y — libstdc++ (GCC 11) instantiated inside libtorch.
// Which of several EQUAL scores make the top k is therefore whatever those two algorithms leave
// in the first k slots; with duplicated candidate rows (an item that is a positive of one edge and
// a sampled negative of another scores identically) that decides hits. The kernels below run the
// same libstdc++ algorithms, step for step, on the same (key, index) sequence (checked against
// torch.topk on tie-heavy rows in tests/test_recall_stl.py's host model of these steps).
// Keys compare as the floats do: -0 is mapped onto +0's key (equal as floats), NaN is highest.
namespace stl {

struct El {
    uint32_t k;
    int32_t i;
};

__device__ __forceinline__ uint32_t canon(uint32_t k) { return k == 0x7FFFFFFFu ? 0x80000000u : k; }
__device__ __forceinline__ bool comp(const El& x, const El& y) { return x.k > y.k; }

// (key, index) arrays in LDS or global memory (flat addresses)
struct Arr {
    uint32_t* k;
    int32_t* i;
    __device__ __forceinline__ El get(int64_t p) const { return El{k[p], i[p]}; }
    __device__ __forceinline__ void set(int64_t p, const El& e) const {
        k[p] = e.k;
        i[p] = e.i;
    }
    __device__ __forceinline__ void swap(int64_t a, int64_t b) const {
        const El x = get(a), y = get(b);
        set(a, y);
        set(b, x);
    }
};

// std::__adjust_heap + std::__push_heap
__device__ void adjust_heap(const Arr& a, int64_t first, int64_t hole, int64_t len, El value) {
    const int64_t top = hole;
    int64_t second = hole;
    while (second < (len - 1) / 2) {
        second = 2 * (second + 1);
        if (comp(a.get(first + second), a.get(first + second - 1))) --second;
        a.set(first + hole, a.get(first + second));
        hole = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
        second = 2 * (second + 1);
        a.set(first + hole, a.get(first + second - 1));
        hole = second - 1;
    }
    int64_t parent = (hole - 1) / 2;
    while (hole > top && comp(a.get(first + parent), value)) {
        a.set(first + hole, a.get(first + parent));
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a.set(first + hole, value);
}

// std::__make_heap
__device__ void make_heap(const Arr& a, int64_t first, int64_t last) {
    const int64_t len = last - first;
    if (len < 2) return;
    for (int64_t parent = (len - 2) / 2;; --parent) {
        adjust_heap(a, first, parent, len, a.get(first + parent));
        if (parent == 0) return;
    }
}

// std::__heap_select: the heap of [first, middle) keeps the best; an element replaces the heap's
// top (its worst) only if strictly better (std::__pop_heap into the element's slot)
__device__ void heap_select(const Arr& a, int64_t first, int64_t middle, int64_t last) {
    make_heap(a, first, middle);
    for (int64_t i = middle; i < last; ++i) {
        if (comp(a.get(i), a.get(first))) {
            const El v = a.get(i);
            a.set(i, a.get(first));
            adjust_heap(a, first, 0, middle - first, v);
        }
    }
}

// std::__move_median_to_first
__device__ void move_median_to_first(const Arr& a, int64_t r, int64_t x, int64_t y, int64_t z) {
    const El A = a.get(x), B = a.get(y), C = a.get(z);
    if (comp(A, B)) {
        if (comp(B, C)) a.swap(r, y);
        else if (comp(A, C)) a.swap(r, z);
        else a.swap(r, x);
    } else if (comp(A, C)) {
        a.swap(r, x);
    } else if (comp(B, C)) {
        a.swap(r, z);
    } else {
        a.swap(r, y);
    }
}

// std::__unguarded_partition around the pivot at `pivot`
__device__ int64_t unguarded_partition(const Arr& a, int64_t first, int64_t last, int64_t pivot) {
    const El pv = a.get(pivot);  // the pivot slot is outside [first, last): never swapped here
    while (true) {
        while (comp(a.get(first), pv)) ++first;
        --last;
        while (comp(pv, a.get(last))) --last;
        if (!(first < last)) return first;
        a.swap(first, last);
        ++first;
    }
}

// std::__insertion_sort (with __unguarded_linear_insert)
__device__ void insertion_sort(const Arr& a, int64_t first, int64_t last) {
    if (first == last) return;
    for (int64_t i = first + 1; i != last; ++i) {
        const El v = a.get(i);
        if (comp(v, a.get(first))) {
            for (int64_t j = i; j > first; --j) a.set(j, a.get(j - 1));  // std::move_backward
            a.set(first, v);
        } else {
            int64_t j = i, nx = i - 1;
            while (comp(v, a.get(nx))) {
                a.set(j, a.get(nx));
                j = nx;
                --nx;
            }
            a.set(j, v);
        }
    }
}

__device__ __forceinline__ int64_t lg(int64_t n) { return 63 - __clzll(static_cast<unsigned long long>(n)); }

// std::nth_element -> std::__introselect(first, nth, last, 2 * __lg(last - first))
__device__ void nth_element(const Arr& a, int64_t first, int64_t nth, int64_t last) {
    if (first == last || nth == last) return;
    int64_t depth = 2 * lg(last - first);
    while (last - first > 3) {
        if (depth == 0) {
            heap_select(a, first, nth + 1, last);
            a.swap(first, nth);  // the nth element to its final place
            return;
        }
        --depth;
        const int64_t mid = first + (last - first) / 2;
        move_median_to_first(a, first, first + 1, mid, last - 1);
        const int64_t cut = unguarded_partition(a, first + 1, last, first);
        if (cut <= nth) first = cut;
        else last = cut;
    }
    insertion_sort(a, first, last);
}

}  // namespace stl

constexpr int kStlHeapMax = 4096;  // k of the partial_sort path (k * 64 <= M): 32 KB of LDS

// partial_sort path: one wave per query streams its dense key row in index order; an element is
// compared with the heap's top in parallel (64 per step), and the few that beat it are inserted in
// index order by lane 0 (std::__heap_select's loop, with the heap in LDS).
__global__ __launch_bounds__(64) void k_select_stl_heap(const uint32_t* __restrict__ list_key, int64_t cap, int64_t M,
                                                        int32_t k, int64_t P, int64_t Qvalid,
                                                        int32_t* __restrict__ hits_out) {
    __shared__ uint32_t hk[kStlHeapMax];
    __shared__ int32_t hi[kStlHeapMax];
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    if (q >= Qvalid) {
        if (lane == 0) hits_out[q] = 0;
        return;
    }
    const uint32_t* row = list_key + q * cap;
    for (int t = lane; t < k; t += 64) {
        hk[t] = stl::canon(row[t]);
        hi[t] = t;
    }
    __syncthreads();
    const stl::Arr heap{hk, hi};
    if (lane == 0) stl::make_heap(heap, 0, k);
    __syncthreads();
    constexpr int U = 8;  // 64-key steps loaded together
    for (int64_t base = k; base < M; base += 64 * U) {
        uint32_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = base + u * 64 + lane;
            v[u] = j < M ? stl::canon(row[j]) : 0u;  // key 0 is below every score's key
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            unsigned long long m = __ballot(v[u] > hk[0]);
            while (m) {
                const int l = __ffsll(static_cast<long long>(m)) - 1;
                m &= m - 1ull;
                const uint32_t vl = __shfl(v[u], l, 64);
                if (lane == 0 && vl > hk[0])
                    stl::adjust_heap(heap, 0, 0, k, stl::El{vl, static_cast<int32_t>(base + u * 64 + l)});
            }
            __syncthreads();  // lane 0's heap writes before the next top read
        }
    }
    int32_t h = 0;
    for (int t = lane; t < k; t += 64) h += hi[t] < P ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off, 64);
    if (lane == 0) hits_out[q] = h;
}

// nth_element path (k * 64 > M, so M < 64 k): lane 0 runs std::nth_element in place on the
// query's dense (key, index) row in global memory; the top k are then its first k slots.
__global__ __launch_bounds__(64) void k_select_stl_nth(uint32_t* __restrict__ list_key, int32_t* __restrict__ list_idx,
                                                       int64_t cap, int64_t M, int32_t k, int64_t P, int64_t Qvalid,
                                                       int32_t* __restrict__ hits_out) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    if (q >= Qvalid) {
        if (lane == 0) hits_out[q] = 0;
        return;
    }
    uint32_t* kr = list_key + q * cap;
    int32_t* ir = list_idx + q * cap;
    for (int64_t t = lane; t < M; t += 64) {
        kr[t] = stl::canon(kr[t]);
        ir[t] = static_cast<int32_t>(t);
    }
    __syncthreads();
    if (lane == 0) stl::nth_element(stl::Arr{kr, ir}, 0, k - 1, M);
    __syncthreads();
    int32_t h = 0;
    for (int t = lane; t < k; t += 64) h += ir[t] < P ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off, 64);
    if (lane == 0) hits_out[q] = h;
}

}  // namespace

extern "C" {

int lgcn_recall_width(int32_t d, int32_t* D_out, int32_t* qpad_multiple) {
    if (d <= 0 || d > 256 || !D_out) return fail(LGCN_E_UNSUPPORTED, "lgcn_recall_width: d=%d (max 256)", d);
    int D = 8;
    while (D < d) D <<= 1;
    *D_out = D;
    if (qpad_multiple) *qpad_multiple = 128;
    return LGCN_OK;
}

int lgcn_normalize_rows(const float* x, const int64_t* idx, int64_t rows, int64_t ld, int32_t d, float* out,
                        int32_t D, int64_t out_rows, lgcn_stream_t stream) {
    if (rows < 0 || out_rows < rows || d <= 0 || D < d || ld < d || (out_rows > 0 && !out) || (rows > 0 && !x))
        return fail(LGCN_E_ARG, "lgcn_normalize_rows: bad args");
    if (out_rows == 0) return LGCN_OK;
    const int64_t threads = out_rows * 32;
    k_normalize_rows<<<grid_for(threads, kBlock, int64_t(1) << 31), kBlock, 0, as_stream(stream)>>>(x, idx, rows, ld, d,
                                                                                                   out, D, out_rows);
    return check_launch("k_normalize_rows");
}

int lgcn_score_filter(const float* Qn, int64_t Qpad, int64_t Qvalid, const float* Cn, int64_t M, int64_t stride,
                      int32_t D, const uint32_t* thr, uint32_t* list_key, int32_t* list_idx, int32_t* list_n,
                      int32_t cap, lgcn_stream_t stream) {
    if (!Qn || Qpad <= 0 || Qvalid > Qpad || M < 0 || stride <= 0 || !list_key || !list_idx || cap <= 0 ||
        (thr && !list_n) || (M > 0 && !Cn) || (M - 1) * stride >= (int64_t(1) << 31))
        return fail(LGCN_E_ARG, "lgcn_score_filter: bad args");
    if (!thr && M > cap) return fail(LGCN_E_ARG, "lgcn_score_filter: dense mode needs M <= cap");
    if (M == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
    switch (D) {
        case 8: return launch_filter<8>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, s);
        case 16: return launch_filter<16>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, s);
        case 32: return launch_filter<32>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, s);
        case 64: return launch_filter<64>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, s);
        case 128: return launch_filter<128>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, s);
        case 256: return launch_filter<256>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, s);
        default: return fail(LGCN_E_UNSUPPORTED, "lgcn_score_filter: D=%d (use lgcn_recall_width)", D);
    }
}

int lgcn_select_topk(const uint32_t* list_key, const int32_t* list_idx, const int32_t* list_n, int32_t dense_n,
                     int32_t cap, int32_t k, int64_t P, int64_t Qpad, int64_t Qvalid, uint32_t* thr_out,
                     int32_t* hits_out, lgcn_stream_t stream) {
    if (!list_key || !list_idx || cap <= 0 || k <= 0 || Qpad <= 0 || Qvalid > Qpad || (!thr_out && !hits_out) ||
        (!list_n && dense_n < 0))
        return fail(LGCN_E_ARG, "lgcn_select_topk: bad args");
    k_select_topk<<<dim3(static_cast<unsigned>(Qpad)), kSelBlock, 0, as_stream(stream)>>>(
        list_key, list_idx, list_n, dense_n, cap, k, P, Qvalid, thr_out, hits_out);
    return check_launch("k_select_topk");
}

int lgcn_select_topk_ranked(const uint32_t* list_key, const int32_t* list_idx, const int32_t* list_n, int32_t dense_n,
                            int32_t cap, int32_t k, int64_t Qpad, int64_t Qvalid, const int64_t* excl_ptr,
                            const int32_t* excl_idx, const int64_t* excl_row, int64_t excl_rows, uint32_t* thr_out,
                            int32_t* out_idx, float* out_score, int32_t* out_n, lgcn_stream_t stream) {
    return select_ranked<false>("lgcn_select_topk_ranked", list_key, list_idx, list_n, dense_n, cap, k, Qpad, Qvalid,
                                excl_ptr, excl_idx, excl_row, excl_rows, thr_out, out_idx, out_score, out_n, nullptr,
                                nullptr, stream);
}

int lgcn_select_topk_stl(uint32_t* list_key, int32_t* list_idx, int64_t cap, int64_t M, int32_t k, int64_t P,
                         int64_t Qpad, int64_t Qvalid, int32_t* hits_out, lgcn_stream_t stream) {
    if (!list_key || !list_idx || !hits_out || k <= 0 || M < k || cap < M || Qpad <= 0 || Qvalid > Qpad ||
        Qpad > INT32_MAX || M > INT32_MAX)
        return fail(LGCN_E_ARG, "lgcn_select_topk_stl: bad args");
    const bool heap = static_cast<int64_t>(k) * 64 <= M;  // ATen topk_impl_loop's use_partial_sort
    if (heap) {
        if (k > kStlHeapMax)
            return fail(LGCN_E_UNSUPPORTED, "lgcn_select_topk_stl: k=%d > %d on the partial_sort path", k, kStlHeapMax);
        k_select_stl_heap<<<dim3(static_cast<unsigned>(Qpad)), 64, 0, as_stream(stream)>>>(list_key, cap, M, k, P,
                                                                                           Qvalid, hits_out);
        return check_launch("k_select_stl_heap");
    }
    k_select_stl_nth<<<dim3(static_cast<unsigned>(Qpad)), 64, 0, as_stream(stream)>>>(list_key, list_idx, cap, M, k, P,
                                                                                      Qvalid, hits_out);
    return check_launch("k_select_stl_nth");
}

}  // extern "C"
