"""The golden fixtures under tests/golden/ as the tests read them and tests/golden/make_golden.py writes them.

A fixture whose compressed .npz would exceed 1 MiB (the limit for a committed file) is stored as <name>.partNN.npz: consecutive runs of
its arrays, in order; an array too large for one part is cut into flat pieces `<key>@@NNN` with its shape in `<key>@@shape`.  `load`
returns the same arrays, with the same keys in the same order, however a fixture is stored."""
from __future__ import annotations

import glob
import io
import os

import numpy as np

LIMIT = 1 << 20                 # bytes per committed file
PART = 900 << 10                # what a part is filled to (the zip headers come on top)
SEP = "@@"


class Golden:
    """The arrays of a fixture stored in parts, with the part of np.load's NpzFile interface the tests use."""

    def __init__(self, arrays):
        self._arrays = arrays
        self.files = list(arrays)

    def __getitem__(self, key):
        return self._arrays[key]

    def __contains__(self, key):
        return key in self._arrays

    def __iter__(self):
        return iter(self.files)

    def keys(self):
        return list(self.files)


def _parts(path):
    return sorted(glob.glob(path[:-len(".npz")] + ".part[0-9][0-9].npz"))


def load(path):
    """np.load(path) for a fixture stored whole; the reassembled arrays for one stored in parts."""
    if os.path.exists(path):
        return np.load(path)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    arrays, pieces = {}, {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                if SEP in k:
                    base, tag = k.rsplit(SEP, 1)
                    arrays.setdefault(base, None)
                    pieces.setdefault(base, {})[tag] = z[k]
                else:
                    arrays[k] = z[k]
    for base, d in pieces.items():
        shape = tuple(int(s) for s in d.pop("shape"))
        arrays[base] = np.concatenate([d[t] for t in sorted(d)]).reshape(shape)
    return Golden(arrays)


def _compressed_size(a):
    buf = io.BytesIO()
    np.savez_compressed(buf, a=a)
    return buf.tell()


def save(path, **arrays):
    """np.savez_compressed(path, **arrays), split into parts when the file would exceed LIMIT.  Returns the files written."""
    for old in _parts(path) + ([path] if os.path.exists(path) else []):
        os.remove(old)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    if buf.tell() <= LIMIT:
        with open(path, "wb") as f:
            f.write(buf.getvalue())
        return [path]
    items = []
    for k, a in arrays.items():
        a = np.asarray(a)
        size = _compressed_size(a)
        if size <= PART:
            items.append((k, a, size))
            continue
        n = -(-size // (PART // 2))
        for i, piece in enumerate(np.array_split(a.reshape(-1), n)):
            items.append((f"{k}{SEP}{i:03d}", piece, _compressed_size(piece)))
        items.append((f"{k}{SEP}shape", np.array(a.shape, np.int64), 0))
    groups, cur, filled = [], {}, 0
    for k, a, size in items:
        if cur and filled + size > PART:
            groups.append(cur)
            cur, filled = {}, 0
        cur[k] = a
        filled += size
    groups.append(cur)
    assert len(groups) <= 100, f"{path}: {len(groups)} parts"
    written = []
    for i, g in enumerate(groups):
        p = f"{path[:-len('.npz')]}.part{i:02d}.npz"
        np.savez_compressed(p, **g)
        assert os.path.getsize(p) <= LIMIT, f"{p}: {os.path.getsize(p)} bytes"
        written.append(p)
    return written
