// What the serving kernels share (lgcn_recall.hip's ranked select, lgcn_metrics.hip, lgcn_rerank.hip,
// lgcn_explain.hip, lgcn_foldin.hip): a query's row of a ragged CSR, membership in a sorted row, and
// the order-preserving integer image of a float. One definition each, so the kernels agree on what
// an empty row is and on how scores order.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace lgcn {

// [beg, end) of query q's row in the index array of the CSR ptr [rows + 1]: row q_row[q], or row q
// when q_row is null. Empty (beg == end) for a row outside [0, rows) and for a malformed pair
// ptr[row + 1] < ptr[row].
__device__ __forceinline__ void ragged_row(int64_t q, const int64_t* __restrict__ ptr,
                                           const int64_t* __restrict__ q_row, int64_t rows, int64_t& beg,
                                           int64_t& end) {
    beg = end = 0;
    const int64_t row = q_row ? q_row[q] : q;
    if (row >= 0 && row < rows) {
        beg = ptr[row];
        end = ptr[row + 1];
        if (end < beg) end = beg;
    }
}

// whether the ascending row[0 .. n) holds value (lower-bound binary search)
__device__ __forceinline__ bool sorted_contains(const int32_t* __restrict__ row, int64_t n, int32_t value) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row[mid] < value) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && row[lo] == value;
}

// Order-preserving image of a float's bits: a < b <=> ordered_key(a) < ordered_key(b) for numbers
// (-0 just below +0). NaNs land beyond the infinities on the side of their sign, so a caller that
// ranks them says where they go before it calls. Never 0 for a number.
__device__ __forceinline__ uint32_t ordered_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// inverse of ordered_key
__device__ __forceinline__ float ordered_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// ordered_key for values that compare as floats do and rank a NaN last: NaN counts as -inf, -0 as +0,
// so a > b <=> image(a) > image(b)
__device__ __forceinline__ uint32_t ordered_key_nan_last(float v) {
    if (!(v == v)) v = -INFINITY;
    if (v == 0.f) v = 0.f;
    return ordered_key(v);
}

}  // namespace lgcn
