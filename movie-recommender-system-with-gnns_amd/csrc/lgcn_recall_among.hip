// Per-query candidate sets on gfx950 (lgcn_score_lists): query q ranks the entries of ITS row of a
// ragged CSR and nothing else — a watchlist, a retrieval stage's output, one held-out item among 99
// sampled negatives. This is the kernel between the CSR and the ranked selection: it scores each
// row into the (key, index) lists lgcn_select_topk_ranked[_attr] reads, with no [Q, M] work, no
// padded [Q, Lmax, D] gather and no workspace; the cost is the sum of the row lengths.
//
//   among_query      the work of one query, by W waves of one workgroup. The query's half-row stays
//                    in registers for the whole row (lane (i, h) holds columns h*D/2 .. of it). The
//                    row is taken in rounds of 32 entries: lane (i, h) reads entry i's candidate
//                    index and its half of that candidate's row, and the round's 32 keys are ONE
//                    32x32 tile of the filter's instruction (v_mfma_f32_32x32x2_f32, every A row the
//                    query, B column c the round's c-th candidate): ScoreTile::row_keys in
//                    lgcn_scoretile.h, beside the filter's own chain, so the keys are the filter's bit
//                    for bit. The loads run ahead of the arithmetic, as in lgcn_explain.hip: a round
//                    issues the candidate indices of the round after next and the rows of the next
//                    one (whose indices arrived a round ago) before its own MFMA chain starts.
//                    An entry outside [0, M) scores nothing and takes no slot: the kept entries of
//                    a round are compacted by a ballot prefix onto the wave's running count (W = 1)
//                    or onto slots the wave claims with one integer LDS atomic per round (W > 1; the
//                    order of a list is free, the selection ranks (key, index)). Entries past cap
//                    are counted and not stored.
//   k_score_lists       one wave per query, one query per 64-thread workgroup: every row of at
//                       most kAmongLong entries. Writes list_n[q] itself: no atomics at all.
//   k_score_lists_long  rows above kAmongLong entries, by the W waves of a workgroup in chunks of
//                       kAmongChunk entries (wave w takes chunks w, w + W, ...). A workgroup looks
//                       at W queries a grid apart (callers hand the queries over longest row first,
//                       which would otherwise leave all long rows to a few workgroups) and ends
//                       after reading their row lengths when none is long.
//
// The kernels themselves live in lgcn_recall_among.h, which lgcn_recall_boost.hip instantiates with a
// per-candidate boost (lgcn_score_lists_boost); this unit instantiates them without.
// The two launches write disjoint queries. W is 8, and 4 at D = 256, whose three half-rows in
// registers (query, this round, next round: 384) need the whole register file of a SIMD per wave.
#include "lgcn_recall_among.h"

extern "C" {

int lgcn_score_lists(const float* Qn, int64_t Qvalid, const float* Cn, int64_t M, int32_t D,
                     const int64_t* among_ptr, const int32_t* among_idx, const int64_t* among_row,
                     int64_t among_rows, uint32_t* list_key, int32_t* list_idx, int32_t* list_n, int32_t cap,
                     lgcn_stream_t stream) {
    return score_lists<false>("lgcn_score_lists", Qn, Qvalid, Cn, M, D, among_ptr, among_idx, among_row, among_rows,
                              list_key, list_idx, list_n, cap, nullptr, stream);
}

}  // extern "C"
