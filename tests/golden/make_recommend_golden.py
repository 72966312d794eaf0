"""Generate tests/golden/recommend.npz from the reference's OWN utils/recommend.py (run in the
build container, where the reference is mounted at /root/reference; the GPU box never runs this).

The reference module is imported unmodified; its one import that is absent here, ``visualizations``
(matplotlib plotting, not used by the two functions recorded), is served by an in-memory stub.
recommend_from_user / recommend_from_movie are called on a small stand-in handler (the two id
maps and a titles DataFrame) and a seeded weight pair behind the reference's get_embeddings
semantics, with and without exclusions (a list and a tensor, as the reference's __main__ passes).
The file holds arrays and names only: the weights, the id and title lists, and per call the query
id, the excluded indices, the returned titles / user ids and scores.

Usage:  python tests/golden/make_recommend_golden.py
"""
from __future__ import annotations

import hashlib
import pathlib
import sys
import types

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REF = pathlib.Path("/root/reference")
# pinned when the fixture was made: a changed file is refused before it runs
REF_SHA256 = {"utils/recommend.py": "a8fb490d8cb8b45dbfd771900a399b3756329cc357c11d8695c2facbe3498f52"}


def reference_recommend():
    if not REF.exists():
        raise SystemExit("/root/reference is not mounted: this fixture can only be made in the build container")
    for rel, want in REF_SHA256.items():
        got = hashlib.sha256((REF / rel).read_bytes()).hexdigest()
        if got != want:
            raise SystemExit(f"/root/reference/{rel} changed (sha256 {got}); refusing to execute it")
    stub = types.ModuleType("visualizations")
    stub.plot_recommendations = stub.analyze_user_recommendations = None  # the names the module imports
    sys.modules["visualizations"] = stub
    sys.dont_write_bytecode = True
    import importlib.util

    spec = importlib.util.spec_from_file_location("ref_recommend", REF / "utils" / "recommend.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Tables:
    """The two embedding tables behind get_embeddings as reference models/light_gcn.py:42-64 serves it."""

    def __init__(self, users, items):
        self.users, self.items = users, items

    def get_embeddings(self, user_indices=None, item_indices=None):
        return self.users[user_indices], self.items[item_indices]


class Handler:
    pass


def main():
    import pandas as pd
    import torch

    ref = reference_recommend()
    rng = np.random.default_rng(41)
    U, I, d = 40, 60, 16
    uw = rng.standard_normal((U, d)).astype(np.float32) * 0.01
    iw = rng.standard_normal((I, d)).astype(np.float32) * 0.01
    user_ids = rng.permutation(np.arange(1, 10 * U))[:U].astype(np.int64)
    movie_ids = rng.permutation(np.arange(1, 10 * I))[:I].astype(np.int64)
    titles = np.array([f"Movie {m}" for m in movie_ids])
    h = Handler()
    h.user_id_map = {int(u): i for i, u in enumerate(user_ids)}
    h.movie_id_map = {int(m): i + U for i, m in enumerate(movie_ids)}
    order = rng.permutation(I)  # movies.csv is not in index order
    h.movies = pd.DataFrame({"movieId": movie_ids[order], "title": titles[order]})
    model = Tables(torch.from_numpy(uw), torch.from_numpy(iw))
    out = dict(user_weight=uw, item_weight=iw, user_ids=user_ids, movie_ids=movie_ids, titles=titles)
    n = 0
    for u in user_ids[[0, 7, 19, 39]]:
        for excl in (None, sorted(rng.choice(I, 25, replace=False).tolist()),
                     torch.from_numpy(rng.choice(I, 52, replace=False))):
            r = ref.recommend_from_user(model, int(u), h, excl)["recommendations"]
            out[f"u{n}_id"] = np.int64(u)
            out[f"u{n}_has_excl"] = np.bool_(excl is not None)
            out[f"u{n}_excl"] = np.asarray([] if excl is None else excl, dtype=np.int64)
            out[f"u{n}_titles"] = np.array([x["title"] for x in r])
            out[f"u{n}_scores"] = np.array([x["score"] for x in r], dtype=np.float32)
            n += 1
    out["n_user_calls"] = np.int64(n)
    n = 0
    for m in movie_ids[[0, 11, 33, 59]]:
        for excl in (None, sorted(rng.choice(U, 15, replace=False).tolist()),
                     torch.from_numpy(rng.choice(U, 33, replace=False))):
            r = ref.recommend_from_movie(model, int(m), h, excl)["top_users"]
            out[f"m{n}_id"] = np.int64(m)
            out[f"m{n}_has_excl"] = np.bool_(excl is not None)
            out[f"m{n}_excl"] = np.asarray([] if excl is None else excl, dtype=np.int64)
            out[f"m{n}_users"] = np.array([x["user_id"] for x in r], dtype=np.int64)
            out[f"m{n}_scores"] = np.array([x["score"] for x in r], dtype=np.float32)
            n += 1
    out["n_movie_calls"] = np.int64(n)
    assert ref.recommend_from_user(model, -1, h) == {"error": "Invalid user ID"}
    assert ref.recommend_from_movie(model, -1, h) == {"error": "Invalid movie ID"}
    np.savez_compressed(HERE / "recommend.npz", **out)
    print("recommend.npz:", (HERE / "recommend.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
