// The boosted entry points of include/lgcn.h: a per-candidate f32 boost added to the score where the
// key is formed, so everything downstream of a key — the thresholds from the strided subset, the
// overflow tightening, the ranked selection, the exclusion search — works on boosted keys and needs no
// change. This unit holds the kBoost instantiations of k_score_filter (lgcn_recall_lists.h, with the
// attribute filter and without) and of the candidate-set kernels (lgcn_recall_among.h): a translation
// unit of its own, so that the unboosted kernels' modules stay what they were (lgcn_recall_lists.h
// says why).

#include "lgcn_recall_among.h"
#include "lgcn_recall_lists.h"

extern "C" {

int lgcn_score_filter_boost(const float* Qn, int64_t Qpad, int64_t Qvalid, const float* Cn, int64_t M, int64_t stride,
                            int32_t D, const uint32_t* thr, uint32_t* list_key, int32_t* list_idx, int32_t* list_n,
                            int32_t cap, const uint32_t* attr, const uint32_t* where, const float* boost,
                            lgcn_stream_t stream) {
    const char* me = "lgcn_score_filter_boost";
    if (!boost) return fail(LGCN_E_ARG, "%s: boost is null", me);
    if (attr && !where) return fail(LGCN_E_ARG, "%s: where is null while attr is set", me);
    if (where && !attr) return fail(LGCN_E_ARG, "%s: attr is null while where is set", me);
    if (!thr && attr)
        return fail(LGCN_E_ARG, "%s: attr is set while thr is null (dense rows take no attribute filter)", me);
    if (!Qn || Qpad <= 0 || Qvalid > Qpad || M < 0 || stride <= 0 || !list_key || !list_idx || cap <= 0 ||
        (thr && !list_n) || (M > 0 && !Cn) || (M - 1) * stride >= (int64_t(1) << 31))
        return fail(LGCN_E_ARG, "%s: bad args", me);
    if (!thr && M > cap) return fail(LGCN_E_ARG, "%s: dense mode needs M <= cap", me);
    if (M == 0) return LGCN_OK;
    hipStream_t s = as_stream(stream);
#define LGCN_FILTER_BOOST(W) \
    case W: \
        return attr ? launch_filter<W, true, true>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, cap, \
                                                   s, attr, where, boost) \
                    : launch_filter<W, false, true>(Qn, Qpad, Qvalid, Cn, M, stride, thr, list_key, list_idx, list_n, \
                                                    cap, s, nullptr, nullptr, boost)
    switch (D) {
        LGCN_FILTER_BOOST(8);
        LGCN_FILTER_BOOST(16);
        LGCN_FILTER_BOOST(32);
        LGCN_FILTER_BOOST(64);
        LGCN_FILTER_BOOST(128);
        LGCN_FILTER_BOOST(256);
        default: return fail(LGCN_E_UNSUPPORTED, "%s: D=%d (use lgcn_recall_width)", me, D);
    }
#undef LGCN_FILTER_BOOST
}

int lgcn_score_lists_boost(const float* Qn, int64_t Qvalid, const float* Cn, int64_t M, int32_t D,
                           const int64_t* among_ptr, const int32_t* among_idx, const int64_t* among_row,
                           int64_t among_rows, uint32_t* list_key, int32_t* list_idx, int32_t* list_n, int32_t cap,
                           const float* boost, lgcn_stream_t stream) {
    return score_lists<true>("lgcn_score_lists_boost", Qn, Qvalid, Cn, M, D, among_ptr, among_idx, among_row,
                             among_rows, list_key, list_idx, list_n, cap, boost, stream);
}

}  // extern "C"
