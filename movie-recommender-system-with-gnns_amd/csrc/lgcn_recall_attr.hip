// The attribute-filtered entry points of include/lgcn.h: the kAttr instantiations of the list
// kernels of lgcn_recall_lists.h (which says why they are a translation unit of their own).

#include "lgcn_recall_lists.h"

extern "C" {

int lgcn_score_filter_attr(const float* Qn, int64_t Qpad, int64_t Qvalid, const float* Cn, int64_t M, int64_t stride,
                           int32_t D, const uint32_t* thr, uint32_t* list_key, int32_t* list_idx, int32_t* list_n,
                           int32_t cap, const uint32_t* attr, const uint32_t* where, lgcn_stream_t stream) {
    const char* me = "lgcn_score_filter_attr";
    if (!thr) return fail(LGCN_E_ARG, "%s: thr is null (list mode only: dense rows are lgcn_score_filter's)", me);
    if (!attr) return fail(LGCN_E_ARG, "%s: attr is null", me);
    if (!where) return fail(LGCN_E_ARG, "%s: where is null", me);
    if (!Qn || Qpad <= 0 || Qvalid > Qpad || M < 0 || stride <= 0 || !list_key || !list_idx || cap <= 0 || !list_n ||
        (M > 0 && !Cn) || (M - 1) * stride >= (int64_t(1) << 31))
        return fail(LGCN_E_ARG, "%s: bad args", me);
    if (M == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
#define LGCN_FILTER_ATTR(W) \
    case W: \
        return launch_filter<W, true>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, s, attr, where)
    switch (D) {
        LGCN_FILTER_ATTR(8);
        LGCN_FILTER_ATTR(16);
        LGCN_FILTER_ATTR(32);
        LGCN_FILTER_ATTR(64);
        LGCN_FILTER_ATTR(128);
        LGCN_FILTER_ATTR(256);
        default: return fail(LGCN_E_UNSUPPORTED, "%s: D=%d (use lgcn_recall_width)", me, D);
    }
#undef LGCN_FILTER_ATTR
}

int lgcn_select_topk_ranked_attr(const uint32_t* list_key, const int32_t* list_idx, const int32_t* list_n,
                                 int32_t dense_n, int32_t cap, int32_t k, int64_t Qpad, int64_t Qvalid,
                                 const int64_t* excl_ptr, const int32_t* excl_idx, const int64_t* excl_row,
                                 int64_t excl_rows, uint32_t* thr_out, int32_t* out_idx, float* out_score,
                                 int32_t* out_n, const uint32_t* attr, const uint32_t* where, lgcn_stream_t stream) {
    return select_ranked<true>("lgcn_select_topk_ranked_attr", list_key, list_idx, list_n, dense_n, cap, k, Qpad,
                               Qvalid, excl_ptr, excl_idx, excl_row, excl_rows, thr_out, out_idx, out_score, out_n, attr,
                               where, stream);
}

}  // extern "C"
