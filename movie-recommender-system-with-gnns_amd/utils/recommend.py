"""Recommendations from a trained model — the reference's utils/recommend.py API on the HIP path.

``recommend_from_user(model, user_id, data_handler, excluded_train_items=None)`` and
``recommend_from_movie(model, movie_id, data_handler, excluded_train_users=None)`` keep the
reference's signatures, inputs (the raw rows of ``model.get_embeddings``, cosine-scored) and return
shapes: {'recommendations': [{'title', 'score'} x 10]}, {'top_users': [{'user_id', 'score'} x 10]}
or {'error': 'Invalid user ID' / 'Invalid movie ID'}; fewer than ten entries when fewer candidates
are left. Where the reference sorts a dense score row and walks it in Python, one
lgcn_amd.recommend.topk_rows call with a one-row exclusion CSR ranks on the device; equal scores
come in ascending index order. ``recommend_for_users`` serves a batch of users in one call, with
``diversity=`` a list re-ranked for diversity (greedy MMR over a relevance pool, on the device) and
with ``explain=r`` every movie carrying the r movies of the user's history that point at it most
strongly ('because', lgcn_amd.explain on the device). ``recommend_for_histories`` serves people who
were not in the training graph from the movies they name (fold-in, lgcn_amd.foldin on the device;
``python utils/recommend.py --movies 1,296,318``). ``rank_for_user`` answers the counterpart of a
list: where do these movies rank for this user, among all the user could be served (exact positions,
lgcn_amd.metrics.rank_positions on the device; ``python utils/recommend.py USER_ID --rank 1,296,318``).
``genres=`` / ``genres_all=`` / ``without_genres=`` (recommend_for_users, recommend_for_histories) serve
"ten comedies", "anything but horror": the ``genres`` column of movies.csv as one attribute word per
movie (``genre_table``), tested on the device where the score is tested
(``python utils/recommend.py USER_ID --genres Comedy,Romance --without Horror``, likewise with ``--movies``).
``among=`` (recommend_for_users, recommend_for_histories) ranks a given set of movies and nothing else —
a watchlist, tonight's schedule, another model's shortlist — at the cost of the sets' sizes
(lgcn_amd.recommend.topk_rows' among; ``python utils/recommend.py USER_ID --among 1,296,318``, likewise
with ``--movies``).
``calibration=`` (recommend_for_users, recommend_for_histories) serves a list that keeps the genre mix of
the user's own history — 70 % drama and 30 % comedy watched, about that served — by a greedy re-rank of
a relevance pool against the KL divergence between the two genre distributions, on the device
(lgcn_amd.recommend.topk_rows_calibrated; ``python utils/recommend.py USER_ID --calibrate 0.5``, likewise
with ``--movies``).
``boost=`` / ``less_popular=`` (recommend_for_users_boosted, recommend_for_histories_boosted: the two
batch calls with two more arguments) move scores instead of
choosing candidates: a value per movie added to its score before anything is ranked — a lift for this
month's releases, a title buried without being removed, a second model's item bias — and a penalty on
popular movies, ``less_popular`` times the movie's share of the log of the highest training interaction
count (lgcn_amd.recommend.topk_rows' boost and popularity_boost, on the device;
``python utils/recommend.py USER_ID --less-popular 0.2``, likewise with ``--movies``).
``recommend_for_groups`` / ``recommend_for_group`` serve several users ONE list — "what do the four of us
watch tonight?" — by least misery (the minimum of the members' scores), most pleasure (the maximum) or
the average, optionally without anything a member scores under a floor; the members' scores are reduced
on the device (lgcn_amd.recommend.topk_groups; ``python utils/recommend.py --group 1,5,9 --strategy average
--floor 0.2``).
Not carried over: the plotting (``visualizations``) and the import-time seeding (nothing here draws
random numbers). Unknown ids are answered without touching the GPU; everything else needs the model
on a ROCm device (lgcn_amd._ffi.LgcnError otherwise, there is no CPU fallback).
How good the served lists are (full-ranking Recall / Precision / HitRate / NDCG / MRR, the same raw
rows, training items left out):
    utils.ranking_eval.evaluate_ranking(model, train_data.edge_index, test_data.edge_index, 'cuda', ks=(10, 20))
"""
from typing import Any, Dict, List, Mapping, Optional, Sequence, Union

import torch

if __name__ == '__main__':  # run as a script: the package root (this file's parent's parent) is not on the path yet
    import os
    import sys

    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

from lgcn_amd import explain as _explain
from lgcn_amd import foldin as _foldin
from lgcn_amd import metrics as _metrics
from lgcn_amd import recommend as _rec

TOP_N = 10  # the reference's list length


def _one_row_csr(excluded, num_candidates: int, device):
    """The exclusion CSR of one query from a list or tensor of candidate indices."""
    if excluded is None:
        return None
    e = torch.as_tensor(excluded, dtype=torch.int64, device=device).view(-1)
    e = torch.unique(e[(e >= 0) & (e < num_candidates)], sorted=True)
    ptr = torch.tensor([0, e.numel()], dtype=torch.int64, device=device)
    return ptr, e.to(torch.int32)


def _id_map(handler, name: str, forward: Dict[int, int]) -> Dict[int, int]:
    """index -> id (the handler's own inverse map when it keeps one)."""
    inv = getattr(handler, name, None)
    return inv if inv is not None else {i: k for k, i in forward.items()}


def _title_of(movies) -> Dict[int, str]:
    first = movies.drop_duplicates("movieId")
    return dict(zip(first["movieId"].tolist(), first["title"].tolist()))


NO_GENRES = '(no genres listed)'  # movies.csv's placeholder: no bit


def genre_table(handler: Any):
    """(vocabulary, attrs) of the handler's movies: the sorted distinct labels of
    ``handler.movies['genres']`` split on '|' — '(no genres listed)', empty and missing values give no
    label — and the int32 [num_items] attribute words in item-index order (CPU), bit b set for
    vocabulary[b] (lgcn_amd.recommend.attr_bits). A movie of ``movie_id_map`` without a row in
    ``movies`` gets 0."""
    movies = handler.movies.drop_duplicates("movieId")
    if "genres" not in movies.columns:
        raise ValueError("genre_table: the handler's movies have no 'genres' column")
    labels_of = {}
    for movie_id, g in zip(movies["movieId"].tolist(), movies["genres"].tolist()):
        parts = g.split('|') if isinstance(g, str) else []
        labels_of[movie_id] = [x.strip() for x in parts if x.strip() and x.strip() != NO_GENRES]
    vocabulary = sorted({x for labels in labels_of.values() for x in labels})
    num_users = len(handler.user_id_map)
    rows: list = [[] for _ in handler.movie_id_map]
    for movie_id, index in handler.movie_id_map.items():
        rows[index - num_users] = labels_of.get(movie_id, [])
    return vocabulary, _rec.attr_bits(rows, vocabulary)


def _genre_filter(who: str, handler: Any, genres, genres_all, without_genres):
    """topk_rows' attrs / where keywords of one genre filter for the whole call (attrs still on the
    CPU); {} when all three are None. An unknown name is a ValueError that lists the vocabulary."""
    if genres is None and genres_all is None and without_genres is None:
        return {}
    vocabulary, attrs = genre_table(handler)
    masks = []
    for names in (genres, genres_all, without_genres):
        if isinstance(names, str):
            names = [names]
        mask = 0
        for name in names or ():
            if name not in vocabulary:
                raise ValueError(f"{who}: unknown genre {name!r}; the handler's movies have {vocabulary}")
            mask |= 1 << vocabulary.index(name)
        masks.append(mask)
    return {"attrs": attrs, "where": tuple(masks)}


def _among_csr(who: str, among, inputs: int, served, handler: Any, device):
    """topk_rows' among= of the served queries, {} when among is None. among: a sequence of movie ids
    shared by every query; a mapping key -> ids; or a sequence of id sequences aligned with the
    caller's ``inputs`` entries. served: one (position among the inputs, mapping key) per query, in
    query order. Unknown ids are dropped, an id named twice counts once (candidate_csr)."""
    if among is None:
        return {}
    num_users, movie_id_map = len(handler.user_id_map), handler.movie_id_map
    known = lambda ids: [movie_id_map[m] - num_users for m in ids if m in movie_id_map]
    if isinstance(among, Mapping):
        rows = [known(among.get(key, ())) for _, key in served]
    else:
        among = list(among)
        if among and all(hasattr(x, '__iter__') and not isinstance(x, (str, bytes)) for x in among):
            if len(among) != inputs:
                raise ValueError(f"{who}: among holds {len(among)} sets for {inputs} entries")
            rows = [known(among[slot]) for slot, _ in served]
        else:  # one set for everybody: one CSR row, named by every query
            ptr, idx = _rec.candidate_csr([known(among)], device=device)
            return {"among": (ptr, idx, torch.zeros(len(served), dtype=torch.int64))}
    return {"among": _rec.candidate_csr(rows, device=device)}


def _boost_vector(who: str, handler: Any, boost, less_popular, counts, device) -> dict:
    """topk_rows' boost= of one call, {} when both arguments are None: float32 [num_items] on ``device``.
    boost: a float tensor over the items (item-index order), or a mapping MovieLens movie id -> value
    with the movies it does not name at -0.0, the exact identity (unknown ids are dropped).
    less_popular: a float b, adding lgcn_amd.recommend.popularity_boost(counts(), b); counts: a function
    that returns the training interaction count per item (called only when it is needed)."""
    if boost is None and less_popular is None:
        return {}
    num_users, num_items = len(handler.user_id_map), len(handler.movie_id_map)
    vec = None
    if isinstance(boost, Mapping):
        host = torch.full((num_items,), -0.0, dtype=torch.float32)
        for movie_id, value in boost.items():
            if movie_id in handler.movie_id_map:
                host[handler.movie_id_map[movie_id] - num_users] = float(value)
        vec = host.to(device)
    elif boost is not None:
        if not isinstance(boost, torch.Tensor) or not boost.is_floating_point() or boost.dim() != 1:
            raise ValueError(f"{who}: boost is a float tensor over the items or a mapping movie id -> value")
        if boost.numel() != num_items:
            raise ValueError(f"{who}: boost has {boost.numel()} values for {num_items} movies")
        vec = boost.detach().to(device=device, dtype=torch.float32)
    if less_popular is not None:
        penalty = _rec.popularity_boost(counts().to(device), float(less_popular))
        vec = penalty if vec is None else vec + penalty
    return {"boost": vec.contiguous()}


def _cli_option(argv: List[str], flag: str) -> Optional[List[str]]:
    """``--flag A,B`` taken out of the argument list ``argv``: the names, or None when it is absent."""
    if flag not in argv[1:-1]:
        return None
    at = argv.index(flag)
    names = [x.strip() for x in argv[at + 1].split(',') if x.strip()]
    del argv[at:at + 2]
    return names


def _cli_ids(names: Optional[List[str]]) -> Optional[List[int]]:
    return None if names is None else [int(x) for x in names]


def _ranked(idx: torch.Tensor, score: torch.Tensor):
    """Host lists of one topk_rows result, the unfilled (-1) slots dropped."""
    idx, score = idx.cpu(), score.cpu()
    return [[(int(i), float(s)) for i, s in zip(ri.tolist(), rs.tolist()) if i >= 0] for ri, rs in zip(idx, score)]


def _check_options(who: str, diversity, pool, explain, calibration=None) -> Optional[int]:
    """The batch calls' ``pool`` / ``explain`` / ``calibration`` refusals under the caller's prefix; explain as
    an int, or None."""
    if diversity is not None and calibration is not None:
        raise ValueError(f"{who}: diversity and calibration are two re-ranks; one per call")
    if calibration is not None:
        _rec._calibration(calibration)
    if diversity is None and calibration is None and pool is not None:
        raise ValueError(f"{who}: pool is the re-rank's pool and needs diversity")
    if explain is None:
        return None
    explain = int(explain)
    if explain < 1 or explain > _explain.MAX_R:
        raise ValueError(f"{who}: explain={explain} outside [1, {_explain.MAX_R}]")
    return explain


def _serve(handler: Any, out: list, slots: Sequence[int], queries: torch.Tensor, item_emb: torch.Tensor, k: int, excl,
           diversity, pool, flt: dict, explain=None, calibration=None, profile=None) -> list:
    """The batch calls' common end: rank item_emb's rows for the queries (one row per slot of ``slots``;
    topk_rows, topk_rows_diverse with ``diversity``, or topk_rows_calibrated with ``calibration`` towards
    the genre mix of ``profile`` = (history CSR with a row per query, its weights or None)), explain the
    lists (``explain``: None, or a function of the ranked indices that returns lgcn_amd.explain's Explained) and write each query's
    [{'movie_id', 'title', 'score'[, 'because']}] into ``out`` at its slot. Returns out."""
    picked = torch.arange(len(slots))
    with torch.no_grad():
        if calibration is not None:
            attrs = flt["attrs"] if "attrs" in flt else genre_table(handler)[1].to(queries.device)
            target = _rec.attr_profile(profile[0], attrs, weights=profile[1])[0]
            idx, score = _rec.topk_rows_calibrated(queries, picked, item_emb, k, calibration, attrs=attrs, target=target,
                                                   pool=pool, excl=excl,
                                                   **{key: v for key, v in flt.items() if key != "attrs"})[:2]
        elif diversity is None:
            idx, score = _rec.topk_rows(queries, picked, item_emb, k, excl=excl, **flt)
        else:
            idx, score = _rec.topk_rows_diverse(queries, picked, item_emb, k, diversity, pool=pool, excl=excl, **flt)[:2]
        why = None if explain is None else explain(idx)
    num_users = len(handler.user_id_map)
    id_movie = _id_map(handler, "id_movie_map", handler.movie_id_map)
    title_of = _title_of(handler.movies)

    def movie(i: int) -> Dict[str, Any]:
        return {'movie_id': id_movie[i + num_users], 'title': title_of[id_movie[i + num_users]]}

    idx, score = idx.tolist(), score.tolist()
    widx, wval = (None, None) if why is None else (why.idx.tolist(), why.value.tolist())

    def because(q: int, j: int) -> Dict[str, Any]:
        if why is None:
            return {}
        return {'because': [dict(movie(b), similarity=v) for b, v in zip(widx[q][j], wval[q][j]) if b >= 0]}

    for q, slot in enumerate(slots):  # the unfilled (-1) slots of a short list are dropped
        out[slot] = [dict(movie(i), score=s, **because(q, j)) for j, (i, s) in enumerate(zip(idx[q], score[q])) if i >= 0]
    return out


def recommend_from_user(model: torch.nn.Module, user_id: int, data_handler: Any,
                        excluded_train_items: Optional[Union[List[int], torch.Tensor]] = None
                        ) -> Dict[str, Union[str, List[Dict[str, Union[str, float]]]]]:
    """The ten best movies for a user, without ``excluded_train_items`` (0-based item indices)."""
    user_id_map, movie_id_map = data_handler.user_id_map, data_handler.movie_id_map
    user_index = user_id_map.get(user_id)
    if user_index is None:
        return {'error': 'Invalid user ID'}
    num_users, num_items = len(user_id_map), len(movie_id_map)
    dev = model.user_embedding.weight.device
    with torch.no_grad():
        user_emb, item_emb = model.get_embeddings(user_indices=torch.tensor([user_index], device=dev),
                                                  item_indices=torch.arange(num_items, device=dev))
        idx, score = _rec.topk_rows(user_emb, torch.arange(1), item_emb, min(TOP_N, max(num_items, 1)),
                                    excl=_one_row_csr(excluded_train_items, num_items, dev))
    id_movie = _id_map(data_handler, "id_movie_map", movie_id_map)
    movies = data_handler.movies
    recommendations = []
    for i, s in _ranked(idx, score)[0]:
        movie_id = id_movie[i + num_users]
        recommendations.append({'title': movies.loc[movies['movieId'] == movie_id, 'title'].iloc[0], 'score': s})
    return {'recommendations': recommendations}


def recommend_from_movie(model: torch.nn.Module, movie_id: int, data_handler: Any,
                         excluded_train_users: Optional[Union[List[int], torch.Tensor]] = None
                         ) -> Dict[str, Union[str, List[Dict[str, Union[int, float]]]]]:
    """The ten best users for a movie, without ``excluded_train_users`` (user indices)."""
    user_id_map, movie_id_map = data_handler.user_id_map, data_handler.movie_id_map
    movie_index = movie_id_map.get(movie_id)
    if movie_index is None:
        return {'error': 'Invalid movie ID'}
    num_users = len(user_id_map)
    movie_index -= num_users
    dev = model.user_embedding.weight.device
    with torch.no_grad():
        user_emb, item_emb = model.get_embeddings(user_indices=torch.arange(num_users, device=dev),
                                                  item_indices=torch.tensor([movie_index], device=dev))
        idx, score = _rec.topk_rows(item_emb, torch.arange(1), user_emb, min(TOP_N, max(num_users, 1)),
                                    excl=_one_row_csr(excluded_train_users, num_users, dev))
    id_user = _id_map(data_handler, "id_user_map", user_id_map)
    return {'top_users': [{'user_id': id_user[i], 'score': s} for i, s in _ranked(idx, score)[0]]}


def recommend_for_users(model: torch.nn.Module, user_ids: Sequence[int], data_handler: Any, k: int = 10,
                        exclude_seen: bool = True, train_edge_index: Optional[torch.Tensor] = None,
                        diversity: Optional[float] = None, pool: Optional[int] = None,
                        explain: Optional[int] = None, genres: Optional[Sequence[str]] = None,
                        genres_all: Optional[Sequence[str]] = None, without_genres: Optional[Sequence[str]] = None,
                        among=None, calibration: Optional[float] = None
                        ) -> List[Union[Dict[str, str], List[Dict[str, Any]]]]:
    """One entry per id of ``user_ids``: the user's k best movies as [{'movie_id', 'title', 'score'}],
    or {'error': 'Invalid user ID'} for an unknown id. With ``exclude_seen`` the movies a user has an
    edge to in ``train_edge_index`` (default: every edge the handler holds, ``data_handler.edge_index``)
    are left out. All known users are ranked by one lgcn_amd.recommend.topk_rows call.
    ``diversity`` (a float in [0, 1]; None: relevance only, as above) serves
    lgcn_amd.recommend.topk_rows_diverse's lists instead: each user's ``pool`` most relevant movies
    (its default when None) re-ranked by greedy Maximal Marginal Relevance down to k, in pick order;
    'score' stays the cosine relevance, so it no longer descends along a list.
    ``explain`` (an int r in [1, lgcn_amd.explain.MAX_R]; None: today's dictionaries, no new key) adds
    'because': [{'movie_id', 'title', 'similarity'}] to every movie: the at most r movies the user has
    an edge to — in the same edge set ``exclude_seen`` uses, whether or not it is set — whose rows have
    the largest cosine to the recommended movie's row, best first (lgcn_amd.explain.explain_items on
    the rows the list was ranked with); fewer than r for a shorter history. It explains the re-ranked
    list when ``diversity`` is set.
    ``genres`` / ``genres_all`` / ``without_genres`` (sequences of genre names; None for all three:
    today's calls) keep only movies with at least one genre of ``genres``, every genre of
    ``genres_all`` and none of ``without_genres`` — one filter for the whole call, genre_table's
    attribute words tested on the device (topk_rows' attrs / where). A list is shorter than k when
    fewer movies are left; an unknown name is a ValueError that lists the vocabulary. They combine
    with ``diversity`` (the pool holds passing movies only) and ``explain``.
    ``among`` (None: today's calls) ranks given movies only: a sequence of MovieLens ids shared by every
    user, a mapping user_id -> ids, or a sequence of id sequences aligned with ``user_ids``. Unknown
    ids are dropped and an id named twice counts once; a user whose set is empty (or who is missing
    from the mapping) gets []. The list is the user's full ranking restricted to the set
    (lgcn_amd.recommend.topk_rows' among, at the cost of the sets' sizes) and combines with
    ``exclude_seen``, ``diversity`` (the pool holds movies of the set only), ``explain`` and the genre
    arguments.
    ``calibration`` (a float in [0, 1]; None: today's calls and dictionaries) serves
    lgcn_amd.recommend.topk_rows_calibrated's lists: each user's ``pool`` most relevant movies re-ranked
    down to k so that the list's genre mix follows that of the movies the user has an edge to (in the
    edge set ``exclude_seen`` uses, whether or not it is set; genre_table's words, a movie's genres
    sharing its weight equally), in pick order; 0.0 is the relevance list, 1.0 follows the genre mix
    alone. 'score' stays the cosine relevance. It works beside the genre arguments, ``among`` and
    ``explain``, and not with ``diversity`` (ValueError: one re-rank per call).
    recommend_for_users_boosted is this call with two more arguments, a per-movie score boost and a
    popularity penalty; this one is that one without them."""
    return recommend_for_users_boosted(model, user_ids, data_handler, k=k, exclude_seen=exclude_seen,
                                       train_edge_index=train_edge_index, diversity=diversity, pool=pool, explain=explain,
                                       genres=genres, genres_all=genres_all, without_genres=without_genres, among=among,
                                       calibration=calibration)


def recommend_for_users_boosted(model: torch.nn.Module, user_ids: Sequence[int], data_handler: Any, boost=None,
                                less_popular: Optional[float] = None, k: int = 10, exclude_seen: bool = True,
                                train_edge_index: Optional[torch.Tensor] = None, diversity: Optional[float] = None,
                                pool: Optional[int] = None, explain: Optional[int] = None,
                                genres: Optional[Sequence[str]] = None, genres_all: Optional[Sequence[str]] = None,
                                without_genres: Optional[Sequence[str]] = None, among=None,
                                calibration: Optional[float] = None
                                ) -> List[Union[Dict[str, str], List[Dict[str, Any]]]]:
    """recommend_for_users with the scores moved before anything is ranked; every other argument and the
    returned entries are recommend_for_users'.
    ``boost`` (None: recommend_for_users' calls and dictionaries) adds a value to a movie's score for every user before
    anything is ranked: a float tensor over the items in item-index order, or a mapping
    {MovieLens movie id: value} whose unnamed movies get -0.0, which changes nothing. 'score' is the
    boosted score. -inf buries a movie (it is served only when nothing else is left), a positive value
    lifts one; the scale is the cosine's. ``less_popular`` (a float b; None: nothing) adds
    lgcn_amd.recommend.popularity_boost of the movies' interaction counts in the edge set
    ``exclude_seen`` uses (whether or not it is set): 0 for a movie nobody has an edge to, -b for the one
    most have, the logarithm of the count in between. Both may be given (they add) and both work beside
    the genre arguments, ``among``, ``diversity``, ``calibration`` (the re-ranks then weigh the boosted
    score) and ``explain``."""
    explain = _check_options("recommend_for_users", diversity, pool, explain, calibration)
    flt = _genre_filter("recommend_for_users", data_handler, genres, genres_all, without_genres)
    user_id_map, movie_id_map = data_handler.user_id_map, data_handler.movie_id_map
    num_users, num_items = len(user_id_map), len(movie_id_map)
    out: list = [{'error': 'Invalid user ID'} for _ in user_ids]
    known = [(slot, user_id_map[u]) for slot, u in enumerate(user_ids) if u in user_id_map]
    if not known:
        return out
    dev = model.user_embedding.weight.device
    if flt:
        flt["attrs"] = flt["attrs"].to(dev)
    users = torch.tensor([u for _, u in known], dtype=torch.int64, device=dev)
    flt.update(_among_csr("recommend_for_users", among, len(user_ids), [(slot, user_ids[slot]) for slot, _ in known],
                          data_handler, dev))
    excl = history = None
    if exclude_seen or explain is not None or calibration is not None or less_popular is not None:
        ei = data_handler.edge_index if train_edge_index is None else train_edge_index
        history = _rec.seen_csr(ei.to(dev), num_users, num_items, by="user")
        if exclude_seen:
            excl = (history[0], history[1], users)
    flt.update(_boost_vector("recommend_for_users", data_handler, boost, less_popular,
                             lambda: torch.bincount(history[1].to(torch.int64), minlength=num_items), dev))
    with torch.no_grad():
        user_emb, item_emb = model.get_embeddings(user_indices=users, item_indices=torch.arange(num_items, device=dev))
    why = None if explain is None else (lambda idx: _explain.explain_items(item_emb, users, idx, history, r=explain))
    profile = None if calibration is None else ((history[0], history[1], users), None)
    return _serve(data_handler, out, [slot for slot, _ in known], user_emb, item_emb, k, excl, diversity, pool, flt, why,
                  calibration, profile)



def recommend_for_histories(model: torch.nn.Module, histories: Sequence[Sequence[int]], data_handler: Any, k: int = 10,
                            exclude_history: bool = True, train_edge_index: Optional[torch.Tensor] = None,
                            embeddings: str = "raw", weights: Optional[Sequence[Sequence[float]]] = None,
                            diversity: Optional[float] = None, pool: Optional[int] = None,
                            explain: Optional[int] = None, genres: Optional[Sequence[str]] = None,
                            genres_all: Optional[Sequence[str]] = None,
                            without_genres: Optional[Sequence[str]] = None, among=None,
                            calibration: Optional[float] = None
                            ) -> List[Union[Dict[str, str], List[Dict[str, Any]]]]:
    """Lists for people the model never saw — someone who has just rated a few films, an anonymous
    session: one entry per history of ``histories`` (each a sequence of MovieLens movie ids), the k
    best movies as recommend_for_users' dictionaries [{'movie_id', 'title', 'score'}], or
    {'error': 'No known movie IDs'} where no id of the history is a movie of the handler. Unknown ids
    are dropped and an id named twice counts once (a graph holds one edge per pair).
    Each history is folded in on the device (lgcn_amd.foldin): the row one more propagation over the
    history's edges would give the new user, every trained row left as it is — the sum of the
    history's item rows, each over sqrt(n * (deg + 1)), n the history's known movies and deg the
    movie's users in ``train_edge_index`` (default ``data_handler.edge_index``). ``weights``: one
    sequence per history, one float per id (a rating, say), None for 1.
    embeddings="raw" folds against and ranks the raw item rows, as every list of this module;
    "propagated" folds against lgcn_amd.foldin.layer_tables' S_item and ranks
    model(train_edge_index)'s item rows, which gives the new user the row the K-layer model would.
    ``exclude_history`` leaves the history's movies out of the list. ``diversity`` / ``pool`` /
    ``explain`` and ``genres`` / ``genres_all`` / ``without_genres`` are recommend_for_users'; the
    'because' movies come from the supplied history (lgcn_amd.explain.explain_rows). All histories are served by one fold-in and one ranking call;
    if no history has a known id the answer comes without touching the model or the GPU.
    ``among`` is recommend_for_users': one sequence of ids for every history, a sequence of id sequences
    aligned with ``histories``, or a mapping from a history's position to its ids.
    ``calibration`` is recommend_for_users', the target being the genre mix of the supplied history
    (under its ``weights``).
    recommend_for_histories_boosted is this call with a per-movie score boost and a popularity penalty."""
    return recommend_for_histories_boosted(model, histories, data_handler, k=k, exclude_history=exclude_history,
                                           train_edge_index=train_edge_index, embeddings=embeddings, weights=weights,
                                           diversity=diversity, pool=pool, explain=explain, genres=genres,
                                           genres_all=genres_all, without_genres=without_genres, among=among,
                                           calibration=calibration)


def recommend_for_histories_boosted(model: torch.nn.Module, histories: Sequence[Sequence[int]], data_handler: Any,
                                    boost=None, less_popular: Optional[float] = None, k: int = 10,
                                    exclude_history: bool = True, train_edge_index: Optional[torch.Tensor] = None,
                                    embeddings: str = "raw", weights: Optional[Sequence[Sequence[float]]] = None,
                                    diversity: Optional[float] = None, pool: Optional[int] = None,
                                    explain: Optional[int] = None, genres: Optional[Sequence[str]] = None,
                                    genres_all: Optional[Sequence[str]] = None,
                                    without_genres: Optional[Sequence[str]] = None, among=None,
                                    calibration: Optional[float] = None
                                    ) -> List[Union[Dict[str, str], List[Dict[str, Any]]]]:
    """recommend_for_histories with the scores moved before anything is ranked: ``boost`` and
    ``less_popular`` are recommend_for_users_boosted's, the interaction counts being the movies' users in
    ``train_edge_index`` (the degrees the fold-in divides by); every other argument and the returned entries
    are recommend_for_histories'."""
    if embeddings not in ("raw", "propagated"):
        raise ValueError(f"recommend_for_histories: embeddings must be 'raw' or 'propagated', got {embeddings!r}")
    explain = _check_options("recommend_for_histories", diversity, pool, explain, calibration)
    if weights is not None and len(weights) != len(histories):
        raise ValueError(f"recommend_for_histories: {len(weights)} weight lists for {len(histories)} histories")
    flt = _genre_filter("recommend_for_histories", data_handler, genres, genres_all, without_genres)
    user_id_map, movie_id_map = data_handler.user_id_map, data_handler.movie_id_map
    num_users, num_items = len(user_id_map), len(movie_id_map)
    out: list = [{'error': 'No known movie IDs'} for _ in histories]
    slots, rows, row_w = [], [], []
    for slot, hist in enumerate(histories):
        w = [1.0] * len(hist) if weights is None else list(weights[slot])
        if len(w) != len(hist):
            raise ValueError(f"recommend_for_histories: history {slot} has {len(hist)} ids and {len(w)} weights")
        known: Dict[int, float] = {}
        for m, x in zip(hist, w):
            if m in movie_id_map:
                known.setdefault(movie_id_map[m] - num_users, float(x))
        if known:
            slots.append(slot)
            rows.append(sorted(known))  # ascending and distinct: the row also serves as exclusion and explain CSR
            row_w.append([known[i] for i in rows[-1]])
    if not slots:
        return out
    dev = model.user_embedding.weight.device
    if flt:
        flt["attrs"] = flt["attrs"].to(dev)
    flt.update(_among_csr("recommend_for_histories", among, len(histories), [(slot, slot) for slot in slots],
                          data_handler, dev))
    ptr = torch.tensor([0] + [len(r) for r in rows], dtype=torch.int64).cumsum(0).to(dev)
    hidx = torch.tensor([i for r in rows for i in r], dtype=torch.int32, device=dev)
    hw = None if weights is None else torch.tensor([x for r in row_w for x in r], dtype=torch.float32, device=dev)
    history = (ptr, hidx)
    ei = (data_handler.edge_index if train_edge_index is None else train_edge_index).to(dev)
    by_item = _rec.seen_csr(ei, num_users, num_items, by="item")
    degree = by_item[0][1:] - by_item[0][:-1]
    flt.update(_boost_vector("recommend_for_histories", data_handler, boost, less_popular, lambda: degree, dev))
    with torch.no_grad():
        if embeddings == "raw":
            item_emb = model.get_embeddings(item_indices=torch.arange(num_items, device=dev))[1]
            table = item_emb
        else:
            item_emb = model(ei)[1]
            table = _foldin.layer_tables(model.user_embedding.weight, model.item_embedding.weight, model.plan_for(ei),
                                         model.num_layers)[1]
        queries = _foldin.fold_in(history, table, count=degree, weights=hw).rows
    why = None if explain is None else (lambda idx: _explain.explain_rows(idx, history, item_emb, r=explain))
    return _serve(data_handler, out, slots, queries, item_emb, k, history if exclude_history else None, diversity, pool,
                  flt, why, calibration, None if calibration is None else (history, hw))



def recommend_for_groups(model: torch.nn.Module, groups_of_user_ids: Sequence[Sequence[int]], data_handler: Any,
                         k: int = 10, strategy: str = "least_misery", floor=None, seen_by: Optional[str] = "any",
                         genres: Optional[Sequence[str]] = None, genres_all: Optional[Sequence[str]] = None,
                         without_genres: Optional[Sequence[str]] = None,
                         train_edge_index: Optional[torch.Tensor] = None
                         ) -> List[Union[Dict[str, str], List[Dict[str, Any]]]]:
    """One entry per group of ``groups_of_user_ids`` (each a sequence of user ids, at most 32): the k
    best movies for the group as a whole, as recommend_for_users' dictionaries [{'movie_id', 'title',
    'score'}], or {'error': 'Invalid user ID'} where the group names an unknown id; a group of nobody
    gets []. All groups are ranked by one lgcn_amd.recommend.topk_groups call.
    ``strategy``: 'least_misery' ranks a movie by the lowest of the members' cosine scores,
    'most_pleasure' by the highest, 'average' by their mean (summed in the order the members are named;
    a user named twice counts twice); 'score' is that value. ``floor`` (None, a float, or one value per
    group): a movie that some member scores below it is left out — 'average' with a floor is "average
    without misery". ``seen_by``: 'any' leaves out what any member has an edge to in
    ``train_edge_index`` (default ``data_handler.edge_index``), 'all' only what every member has, None
    nothing. ``genres`` / ``genres_all`` / ``without_genres`` are recommend_for_users'. A list is shorter
    than k when fewer movies are left."""
    if seen_by not in ("any", "all", None):
        raise ValueError(f"recommend_for_groups: seen_by must be 'any', 'all' or None, got {seen_by!r}")
    flt = _genre_filter("recommend_for_groups", data_handler, genres, genres_all, without_genres)
    user_id_map, movie_id_map = data_handler.user_id_map, data_handler.movie_id_map
    num_users, num_items = len(user_id_map), len(movie_id_map)
    groups = [list(g) for g in groups_of_user_ids]
    out: list = [{'error': 'Invalid user ID'} for _ in groups]
    slots = [slot for slot, g in enumerate(groups) if all(u in user_id_map for u in g)]
    if not slots:
        return out
    members = [[user_id_map[u] for u in groups[slot]] for slot in slots]  # user indices, in the order named
    if floor is not None and not isinstance(floor, (int, float)):
        floor = torch.as_tensor(floor, dtype=torch.float32).reshape(-1)
        if floor.numel() != len(groups):
            raise ValueError(f"recommend_for_groups: {floor.numel()} floors for {len(groups)} groups")
        floor = floor[torch.tensor(slots)]
    dev = model.user_embedding.weight.device
    if flt:
        flt["attrs"] = flt["attrs"].to(dev)
    distinct = sorted({u for g in members for u in g})
    row_of = {u: r for r, u in enumerate(distinct)}
    excl = None
    if seen_by is not None:
        ei = data_handler.edge_index if train_edge_index is None else train_edge_index
        excl = _rec.group_seen_csr(_rec.seen_csr(ei.to(dev), num_users, num_items, by="user"), members, by=seen_by)
    with torch.no_grad():
        user_emb, item_emb = model.get_embeddings(user_indices=torch.tensor(distinct, dtype=torch.int64, device=dev),
                                                  item_indices=torch.arange(num_items, device=dev))
        idx, score = _rec.topk_groups(user_emb, [[row_of[u] for u in g] for g in members], item_emb, k,
                                      strategy=strategy, floor=floor, excl=excl, **flt)
    id_movie = _id_map(data_handler, "id_movie_map", movie_id_map)
    title_of = _title_of(data_handler.movies)
    for slot, ranked in zip(slots, _ranked(idx, score)):
        out[slot] = [{'movie_id': id_movie[i + num_users], 'title': title_of[id_movie[i + num_users]], 'score': s}
                     for i, s in ranked]
    return out


def recommend_for_group(model: torch.nn.Module, user_ids: Sequence[int], data_handler: Any, k: int = 10,
                        **kw) -> Union[Dict[str, str], List[Dict[str, Any]]]:
    """recommend_for_groups for one group: its list, or {'error': 'Invalid user ID'}."""
    return recommend_for_groups(model, [user_ids], data_handler, k=k, **kw)[0]


def rank_for_user(model: torch.nn.Module, user_id: int, movie_ids: Sequence[int], data_handler: Any,
                  exclude_seen: bool = True, train_edge_index: Optional[torch.Tensor] = None
                  ) -> Union[Dict[str, str], List[Dict[str, Any]]]:
    """Where each movie of ``movie_ids`` ranks for the user: one {'movie_id', 'title', 'rank', 'score',
    'of'} per id, in the order given. 'rank' is 1-based among the 'of' movies the user could be
    served — rank r is slot r of recommend_for_users' list with the same ``exclude_seen`` /
    ``train_edge_index`` — and None, like 'score' and 'title' where unknown, for a movie the user has
    seen (with ``exclude_seen``) or an id the handler does not know. An unknown user gives
    {'error': 'Invalid user ID'}, answered without touching the GPU. One
    lgcn_amd.metrics.rank_positions call whatever the number of movies."""
    user_id_map, movie_id_map = data_handler.user_id_map, data_handler.movie_id_map
    user_index = user_id_map.get(user_id)
    if user_index is None:
        return {'error': 'Invalid user ID'}
    num_users, num_items = len(user_id_map), len(movie_id_map)
    title_of = _title_of(data_handler.movies)
    out = [{'movie_id': m, 'title': title_of.get(m), 'rank': None, 'score': None, 'of': None} for m in movie_ids]
    known = sorted({movie_id_map[m] - num_users for m in movie_ids if m in movie_id_map})
    dev = model.user_embedding.weight.device
    seen = None
    if exclude_seen:
        ei = data_handler.edge_index if train_edge_index is None else train_edge_index
        history = _rec.seen_csr(ei.to(dev), num_users, num_items, by="user")
        seen = (history[0], history[1], torch.tensor([user_index]))
    truth = (torch.tensor([0, len(known)], dtype=torch.int64, device=dev),
             torch.tensor(known, dtype=torch.int32, device=dev))
    with torch.no_grad():
        user_emb, item_emb = model.get_embeddings(user_indices=torch.tensor([user_index], device=dev),
                                                  item_indices=torch.arange(num_items, device=dev))
        got = _metrics.rank_positions(user_emb, torch.arange(1), item_emb, truth, seen=seen)
    pos, score, of = got.pos.tolist(), got.score.tolist(), int(got.eligible[0])
    at = {i: t for t, i in enumerate(known)}
    for entry in out:
        entry['of'] = of
        if entry['movie_id'] in movie_id_map:
            t = at[movie_id_map[entry['movie_id']] - num_users]
            if pos[t] >= 0:
                entry['rank'], entry['score'] = pos[t] + 1, score[t]
    return out


if __name__ == '__main__':
    from data.dataset_handler import MovieLensDataHandler
    from models.light_gcn import LightGCN

    def option(flag):  # --flag A,B taken out of the argument list: the names, or None
        return _cli_option(sys.argv, flag)

    # a genre filter: --genres Comedy,Romance (any of) --genres-all Comedy,Romance (each of) --without Horror;
    # a given set of movies to rank, and nothing else: --among 1,296,318
    genre_kw = dict(genres=option('--genres'), genres_all=option('--genres-all'), without_genres=option('--without'),
                    among=_cli_ids(option('--among')))
    calibrate = option('--calibrate')  # a list that keeps the history's genre mix: --calibrate 0.5
    genre_kw['calibration'] = None if calibrate is None else float(calibrate[0])
    less_popular = option('--less-popular')  # a penalty on popular movies: --less-popular 0.2
    less_popular = None if less_popular is None else float(less_popular[0])
    genre_kw['less_popular'] = less_popular  # counts as a filter below: the batch call serves the list
    filtered = any(v is not None for v in genre_kw.values())
    group = _cli_ids(option('--group'))
    strategy = (option('--strategy') or ['least_misery'])[0]
    group_floor = option('--floor')
    group_floor = None if group_floor is None else float(group_floor[0])
    handler = MovieLensDataHandler('data/movielens-25m/ratings.csv', 'data/movielens-25m/movies.csv')
    model = LightGCN(*handler.get_num_users_items()).to('cuda')
    if os.path.exists('best_model.pth'):
        model.load_state_dict(torch.load('best_model.pth', map_location='cuda'))
    model.eval()
    if len(sys.argv) > 2 and sys.argv[1] == '--movies':  # someone the model never saw: --movies 1,296,318
        watched = [int(m) for m in sys.argv[2].split(',') if m.strip()]
        served = recommend_for_histories_boosted(model, [watched], handler, k=TOP_N, explain=3, **genre_kw)[0]
        if isinstance(served, dict):
            sys.exit(served['error'])
        print(f"Top 10 Recommendations for someone who watched {', '.join(map(str, watched))}:")
        for rank, rec in enumerate(served, 1):
            print(f"{rank}. {rec['title']} (Score: {rec['score']:.4f})")
            if rec['because']:
                print("   because you watched: " + ", ".join(f"{b['title']} ({b['similarity']:.2f})"
                                                              for b in rec['because']))
        sys.exit(0)
    if group is not None:  # one list for several users: --group 1,5,9 [--strategy average] [--floor 0.2]
        if genre_kw.pop('among') is not None:
            sys.exit("--among is not supported with --group")
        if genre_kw.pop('calibration') is not None:
            sys.exit("--calibrate is not supported with --group")
        if genre_kw.pop('less_popular') is not None:
            sys.exit("--less-popular is not supported with --group")
        train_data, _, _ = handler.get_datasets()
        served = recommend_for_group(model, group, handler, k=TOP_N, strategy=strategy, floor=group_floor,
                                     train_edge_index=train_data.edge_index, **genre_kw)
        if isinstance(served, dict):
            sys.exit(served['error'])
        print(f"Top 10 Recommendations for users {', '.join(map(str, group))} together ({strategy}"
              + ("" if group_floor is None else f", nothing under {group_floor}") + "):")
        for rank, rec in enumerate(served, 1):
            print(f"{rank}. {rec['title']} (Score: {rec['score']:.4f})")
        sys.exit(0)
    uid = int(sys.argv[1]) if len(sys.argv) > 1 else next(iter(handler.user_id_map))
    if uid not in handler.user_id_map:
        sys.exit(recommend_from_user(model, uid, handler)['error'])
    train_data, _, _ = handler.get_datasets()
    ei = train_data.edge_index
    if len(sys.argv) > 3 and sys.argv[2] == '--rank':  # where do these movies rank: USER_ID --rank 1,296,318
        asked = [int(m) for m in sys.argv[3].split(',') if m.strip()]
        for r in rank_for_user(model, uid, asked, handler, train_edge_index=ei):
            where = 'unknown movie' if r['title'] is None else \
                'already seen' if r['rank'] is None else f"rank {r['rank']} of {r['of']} (Score: {r['score']:.4f})"
            print(f"{r['movie_id']}: {r['title'] or '?'}: {where}")
        sys.exit(0)
    seen_items = ei[1, ei[0] == handler.user_id_map[uid]] - handler.num_users
    why = recommend_for_users_boosted(model, [uid], handler, k=TOP_N, train_edge_index=ei, explain=3, **genre_kw)[0]
    # the reference's own call serves the unfiltered list; a genre filter is recommend_for_users' alone
    result = {'recommendations': why} if filtered else recommend_from_user(model, uid, handler, seen_items)
    because = {rec['title']: rec['because'] for rec in why}
    print(f"Top 10 Recommendations for user {uid}:")
    for rank, rec in enumerate(result['recommendations'], 1):
        print(f"{rank}. {rec['title']} (Score: {rec['score']:.4f})")
        if because.get(rec['title']):
            print("   because you watched: " + ", ".join(f"{b['title']} ({b['similarity']:.2f})"
                                                          for b in because[rec['title']]))
