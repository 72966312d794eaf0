"""Golden fixtures kept as several small .npz parts (tests/golden/<stem>/part_NNN.npz), so that no
committed file is large. A part holds whole arrays under their own names; an array too large for
one part is cut along its first axis into pieces "<name>@@<i>", put back together on load."""
from __future__ import annotations

import pathlib

import numpy as np

PART_BYTES = 900_000  # uncompressed array bytes per part (a part's file is no larger than that + headers)
_PIECE = "@@"


class Parts(dict):
    """name -> array, with the .files list of the np.load object it stands in for."""

    @property
    def files(self):
        return list(self)


def save_parts(directory, arrays: dict, part_bytes: int = PART_BYTES) -> int:
    """Write `arrays` as directory/part_NNN.npz (compressed), filling each part in the given order
    up to part_bytes; returns the number of parts."""
    directory = pathlib.Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    pieces = []
    for name, a in arrays.items():
        a = np.asarray(a)
        if _PIECE in name:
            raise ValueError(f"array name {name!r} contains {_PIECE!r}")
        if a.nbytes <= part_bytes or a.ndim == 0:
            pieces.append((name, a))
            continue
        rows = max(1, int(part_bytes // max(1, a.nbytes // a.shape[0])))
        for i, r in enumerate(range(0, a.shape[0], rows)):
            pieces.append((f"{name}{_PIECE}{i}", a[r:r + rows]))
    parts, cur, size = [], {}, 0
    for name, a in pieces:
        if cur and size + a.nbytes > part_bytes:
            parts.append(cur)
            cur, size = {}, 0
        cur[name] = a
        size += a.nbytes
    if cur:
        parts.append(cur)
    for i, p in enumerate(parts):
        np.savez_compressed(directory / f"part_{i:03d}.npz", **p)
    return len(parts)


def load_parts(directory) -> Parts:
    """Every array of directory/part_*.npz under its name (pieces concatenated in order)."""
    directory = pathlib.Path(directory)
    files = sorted(directory.glob("part_*.npz"))
    if not files:
        raise FileNotFoundError(f"no golden parts under {directory}")
    whole, cut = Parts(), {}
    for f in files:
        with np.load(f) as z:
            for k in z.files:
                if _PIECE in k:
                    name, i = k.split(_PIECE)
                    cut.setdefault(name, {})[int(i)] = z[k]
                else:
                    whole[k] = z[k]
    for name, ps in cut.items():
        assert sorted(ps) == list(range(len(ps))), f"{name}: pieces {sorted(ps)}"
        whole[name] = np.concatenate([ps[i] for i in range(len(ps))], axis=0)
    return whole
