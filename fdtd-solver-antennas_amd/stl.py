"""A small STL reader (and a writer for tests and tools): triangles [ntri][3][3] float64 (triangle, corner, x y z), numpy only.

Binary: an 80-byte header, a little-endian uint32 triangle count, then 50-byte records (normal, three corners as float32, a uint16
attribute); recognised by size == 84 + 50 * count, whatever the header says (a binary file may start with "solid").  ASCII:
`facet` / `vertex` lines.  The stored normals are ignored (primitives.py: the inside rule does not use them).  No PLY.
"""
from __future__ import annotations

import os
import numpy as np

_RECORD = np.dtype([("normal", "<f4", 3), ("corners", "<f4", (3, 3)), ("attr", "<u2")])
assert _RECORD.itemsize == 50


def read_stl(filename) -> np.ndarray:
    """The triangles of an STL file.  ValueError for a missing, truncated or facet-less file and for non-finite coordinates."""
    name = os.fspath(filename)
    try:
        with open(name, "rb") as fh:
            raw = fh.read()
    except OSError as e:
        raise ValueError(f"STL file '{name}': cannot be read ({e.strerror or e})") from None
    tri = None
    if len(raw) >= 84:
        count = int(np.frombuffer(raw, "<u4", 1, 80)[0])
        if len(raw) == 84 + 50 * count:
            tri = np.frombuffer(raw, _RECORD, count, 84)["corners"].astype(np.float64)
    if tri is None:
        tri = _read_ascii(raw, name)
    if tri.shape[0] == 0:
        raise ValueError(f"STL file '{name}': no facet")
    if not np.all(np.isfinite(tri)):
        raise ValueError(f"STL file '{name}': non-finite coordinates")
    return tri


def _read_ascii(raw: bytes, name: str) -> np.ndarray:
    try:
        text = raw.decode("ascii")
    except UnicodeDecodeError:
        raise ValueError(f"STL file '{name}': truncated or not an STL file (neither 84 + 50 n bytes nor ASCII text)") from None
    tokens = text.split()
    if not tokens or tokens[0].lower() != "solid":
        raise ValueError(f"STL file '{name}': truncated or not an STL file (neither 84 + 50 n bytes nor a 'solid')")
    corners, open_facet, pending = [], False, 0
    q = 0
    while q < len(tokens):
        t = tokens[q].lower()
        if t == "facet":
            if open_facet:
                raise ValueError(f"STL file '{name}': truncated: a facet inside a facet")
            open_facet, pending = True, 0
        elif t == "vertex":
            if not open_facet or q + 3 > len(tokens) - 1:
                raise ValueError(f"STL file '{name}': truncated: a vertex line is incomplete")
            try:
                corners.append([float(tokens[q + 1]), float(tokens[q + 2]), float(tokens[q + 3])])
            except ValueError:
                raise ValueError(f"STL file '{name}': a vertex line holds no three numbers") from None
            pending += 1
            q += 3
        elif t == "endfacet":
            if not open_facet or pending != 3:
                raise ValueError(f"STL file '{name}': truncated: a facet with {pending} vertices")
            open_facet = False
        q += 1
    if open_facet or "endsolid" not in (t.lower() for t in tokens):
        raise ValueError(f"STL file '{name}': truncated: the last facet or the solid is not closed")
    return np.array(corners, np.float64).reshape(-1, 3, 3)


def write_stl(filename, triangles, binary: bool = True, name: str = "mesh") -> None:
    """Write triangles [ntri][3][3], rounded to float32 (what the binary format holds; the ASCII text spells the same values exactly,
    so both writings of a mesh read back identical)."""
    tri = np.asarray(triangles, np.float64).reshape(-1, 3, 3).astype(np.float32).astype(np.float64)
    if binary:
        rec = np.zeros(tri.shape[0], _RECORD)
        rec["corners"] = tri
        with open(filename, "wb") as fh:
            fh.write(name.encode("ascii")[:80].ljust(80, b" "))
            fh.write(np.array([tri.shape[0]], "<u4").tobytes())
            fh.write(rec.tobytes())
        return
    with open(filename, "w") as fh:
        fh.write(f"solid {name}\n")
        for t in tri:
            fh.write(" facet normal 0 0 0\n  outer loop\n")
            for c in t:
                fh.write(f"   vertex {float(c[0])!r} {float(c[1])!r} {float(c[2])!r}\n")
            fh.write("  endloop\n endfacet\n")
        fh.write(f"endsolid {name}\n")
