"""Top-k recommendation without a GPU: lgcn_select_topk_ranked checks its arguments before any HIP
call, seen_csr builds the exclusion CSR with plain torch ops, utils.recommend answers unknown ids
on the host, and the ranked path refuses CPU tensors (no silent fallback)."""
import ctypes

import numpy as np
import pytest
import torch


def _ranked_args(**over):
    """A well-formed lgcn_select_topk_ranked argument list over host buffers (never launched:
    every call below must fail validation first), with some arguments replaced."""
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    a = dict(list_key=p, list_idx=p, list_n=p, dense_n=0, cap=64, k=10, Qpad=128, Qvalid=1, excl_ptr=None,
             excl_idx=None, excl_row=None, excl_rows=0, thr_out=None, out_idx=p, out_score=p, out_n=p, stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(list_key=None), b"list_key"),
    (dict(list_idx=None), b"list_idx"),
    (dict(k=0), b"k=0"),
    (dict(k=1025), b"k=1025"),
    (dict(cap=9), b"cap=9"),
    (dict(excl_ptr=1, excl_idx=None), b"excl_idx"),
    (dict(out_idx=None), b"out_idx"),
    (dict(out_score=None), b"out_score"),
    (dict(out_n=None), b"out_n"),
    (dict(out_idx=None, out_score=None, out_n=None), b"no output"),
    (dict(list_n=None, dense_n=65), b"dense_n"),
    (dict(Qvalid=129), b"Qvalid"),
])
def test_select_topk_ranked_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    buf, args = _ranked_args(**over)
    assert lib.lgcn_select_topk_ranked(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_select_topk_ranked" in msg and word in msg, msg


def test_select_topk_ranked_limits_are_the_headers():
    from lgcn_amd import _ffi, recommend

    lib = _ffi.load()
    assert recommend.MAX_K == _ffi.RANKED_MAX_K == 1024
    buf, args = _ranked_args(cap=_ffi.RANKED_MAX_CAP + 1)
    assert lib.lgcn_select_topk_ranked(*args) == _ffi.E_UNSUPPORTED
    assert _ffi.ABI_VERSION == 11 and "lgcn_select_topk_ranked" in _ffi.EXPORTED


def _seen_numpy(edges, U, I, by):
    rows = [set() for _ in range(U if by == "user" else I)]
    for a, b in edges.T.tolist():
        if a >= U:
            a, b = b, a
        u, i = a, b - U
        if by == "user":
            rows[u].add(i)
        else:
            rows[i].add(u)
    ptr = np.cumsum([0] + [len(r) for r in rows])
    idx = np.array([c for r in rows for c in sorted(r)], dtype=np.int32)
    return ptr.astype(np.int64), idx


@pytest.mark.parametrize("by", ["user", "item"])
@pytest.mark.parametrize("directed", [False, True])
def test_seen_csr_matches_numpy(by, directed):
    from lgcn_amd.recommend import seen_csr

    rng = np.random.default_rng(3)
    U, I, E = 17, 11, 90
    u = rng.integers(0, U - 1, E)  # user U-1 has no edges
    i = rng.integers(0, I, E) + U  # E > the distinct pairs drawn: duplicates
    assert len(set(zip(u.tolist(), i.tolist()))) < E
    edges = np.stack([u, i]) if directed else np.concatenate([np.stack([u, i]), np.stack([i, u])[:, ::2]], axis=1)
    ptr, idx = seen_csr(torch.from_numpy(edges), U, I, by=by)
    want_ptr, want_idx = _seen_numpy(edges, U, I, by)
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int32
    np.testing.assert_array_equal(ptr.numpy(), want_ptr)
    np.testing.assert_array_equal(idx.numpy(), want_idx)
    if by == "user":
        assert ptr[U] == ptr[U - 1]  # the user without edges: an empty row


def test_seen_csr_empty_and_bad_mode():
    from lgcn_amd.recommend import seen_csr

    ptr, idx = seen_csr(torch.zeros((2, 0), dtype=torch.int64), 4, 3)
    assert ptr.tolist() == [0] * 5 and idx.numel() == 0
    with pytest.raises(ValueError):
        seen_csr(torch.zeros((2, 0), dtype=torch.int64), 4, 3, by="movie")


class _Handler:
    def __init__(self):
        import pandas as pd

        self.user_id_map = {10: 0, 20: 1, 30: 2}
        self.id_user_map = {v: k for k, v in self.user_id_map.items()}
        self.movie_id_map = {7: 3, 8: 4, 9: 5, 5: 6}
        self.id_movie_map = {v: k for k, v in self.movie_id_map.items()}
        self.movies = pd.DataFrame({"movieId": [5, 7, 8, 9], "title": ["E", "G", "H", "I"]})
        self.edge_index = torch.tensor([[0, 1, 3, 4], [3, 4, 0, 1]])


def test_unknown_ids_give_the_reference_error_dicts():
    from models.light_gcn import LightGCN
    from utils import recommend as R

    h = _Handler()
    model = LightGCN(3, 4, num_layers=1, dim_h=8)
    assert R.recommend_from_user(model, 11, h) == {'error': 'Invalid user ID'}
    assert R.recommend_from_movie(model, 6, h, [0]) == {'error': 'Invalid movie ID'}
    assert R.recommend_for_users(model, [11, 12], h) == [{'error': 'Invalid user ID'}] * 2


def test_k_limits_raise_value_error():
    from lgcn_amd.recommend import topk_rows

    x = torch.zeros(4, 8)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k="):
            topk_rows(x, torch.arange(2), x, k)


def test_ranked_path_fails_loudly_without_gpu():
    from lgcn_amd import _ffi
    from lgcn_amd.recommend import topk_items, topk_rows
    from models.light_gcn import LightGCN
    from utils import recommend as R

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = torch.randn(4, 8)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        topk_rows(x, torch.arange(2), x, 2)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        topk_items(x, x, [0, 1], 2)
    h = _Handler()
    model = LightGCN(3, 4, num_layers=1, dim_h=8)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        R.recommend_from_user(model, 10, h, [0])
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        R.recommend_from_movie(model, 7, h)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        R.recommend_for_users(model, [10, 99], h)


def test_script_entry_point_resolves_its_imports(tmp_path):
    """`python utils/recommend.py`, the documented command: the package's modules resolve when the
    file is run as a script, and the run stops at the data files that are not there."""
    import subprocess
    import sys

    from conftest import PKG

    r = subprocess.run([sys.executable, str(PKG / "utils" / "recommend.py")], cwd=tmp_path, capture_output=True,
                       text=True)
    assert r.returncode != 0 and "ModuleNotFoundError" not in r.stderr and "ImportError" not in r.stderr, r.stderr
    assert "FileNotFoundError" in r.stderr and "MovieLens-25M is not present" in r.stderr, r.stderr
