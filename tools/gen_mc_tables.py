#!/usr/bin/env python3
"""Derives the marching-cubes case table of pixel-nerf_amd/csrc/pnr_mesh.hip (the rows of pnr_mc_tables.inc) from one rule,
so that the 256 x 16 numbers need not be trusted: `python tools/gen_mc_tables.py` prints the rows, `--check FILE` compares
them with FILE (pixel-nerf_amd/csrc/pnr_mc_tables.inc).  tests/test_mesh_host.py checks the properties below on the tables the built library
hands out (pnr_marching_cubes_tables), independently of this script.

Conventions (include/pixelnerf_hip.h, pnr_marching_cubes_tables):
  corner c of a cell = (dx, dy, dz) with c = dx + 2 dy + 4 dz; bit c of the case index is set iff the corner is inside;
  edge e = 4 axis + r joins the corner whose other two coordinates (in axis order) are (r & 1, r >> 1) with its neighbour
  along `axis` (x = 0, y = 1, z = 2).

Rule: on every cube face the patch boundary is a function of the face's four inside flags alone.  Two crossed edges are
joined by one segment; four crossed edges (the two inside corners are diagonal) are joined so that each INSIDE corner is cut
off on its own.  The segments of all six faces close into loops, each loop is filled with a triangle fan from its smallest edge
id, and loops are ordered by their smallest edge id.  Winding: (v1 - v0) x (v2 - v0) points from inside to outside."""
import sys

import numpy as np


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_corners(e):
    axis, r = e >> 2, e & 3
    o = [0, 0, 0]
    others = [a for a in range(3) if a != axis]
    o[others[0]], o[others[1]] = r & 1, r >> 1
    lo = o[0] + 2 * o[1] + 4 * o[2]
    return lo, lo + (1 << axis)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def face_corners(axis, side):
    """the four corners of a face in face-local order (u, v) = (0,0), (1,0), (0,1), (1,1); u, v: the other axes, ascending"""
    u, v = [a for a in range(3) if a != axis]
    out = []
    for fv in (0, 1):
        for fu in (0, 1):
            o = [0, 0, 0]
            o[axis], o[u], o[v] = side, fu, fv
            out.append(o[0] + 2 * o[1] + 4 * o[2])
    return out


def face_segments(case, axis, side):
    """undirected segments (pairs of edge ids) of the patch boundary on one face"""
    c = face_corners(axis, side)
    inside = [(case >> k) & 1 for k in c]
    ring = [0, 1, 3, 2]  # face-local corners in cyclic order
    crossed = []         # (edge id, position in the ring of the edge's first corner)
    for i in range(4):
        a, b = ring[i], ring[(i + 1) % 4]
        if inside[a] != inside[b]:
            crossed.append((EDGE_OF[frozenset((c[a], c[b]))], i))
    if not crossed:
        return []
    if len(crossed) == 2:
        return [(crossed[0][0], crossed[1][0])]
    segs = []            # ambiguous: cut off each inside corner
    for i in range(4):
        if inside[ring[i]]:
            prev_edge = EDGE_OF[frozenset((c[ring[i - 1]], c[ring[i]]))]
            next_edge = EDGE_OF[frozenset((c[ring[i]], c[ring[(i + 1) % 4]]))]
            segs.append((prev_edge, next_edge))
    return segs


def case_triangles(case):
    nbr = {}
    for axis in range(3):
        for side in (0, 1):
            for a, b in face_segments(case, axis, side):
                nbr.setdefault(a, []).append(b)
                nbr.setdefault(b, []).append(a)
    assert all(len(v) == 2 for v in nbr.values())
    mid = {e: (corner_xyz(edge_corners(e)[0]) + corner_xyz(edge_corners(e)[1])) / 2.0 for e in nbr}
    tris, seen = [], set()
    for start in sorted(nbr):
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        while True:
            seen.add(cur)
            nxt = nbr[cur][0] if nbr[cur][0] != prev else nbr[cur][1]  # (two edges share one face at most: no 2-loops)
            if nxt == start:
                break
            loop.append(nxt)
            prev, cur = cur, nxt
        # orientation: the loop's area vector (Newell) against the inside -> outside directions of its edges
        n = np.zeros(3)
        for i in range(len(loop)):
            n += np.cross(mid[loop[i]], mid[loop[(i + 1) % len(loop)]])
        d = np.zeros(3)
        for e in loop:
            a, b = edge_corners(e)
            s = 1.0 if (case >> a) & 1 else -1.0  # a inside: a -> b points outwards
            d += s * (corner_xyz(b) - corner_xyz(a))
        assert abs(n @ d) > 1e-9
        if n @ d < 0:
            loop = [loop[0]] + loop[:0:-1]
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def tables():
    edge_mask = np.zeros(256, np.int32)
    tri = np.full((256, 16), -1, np.int32)
    for case in range(256):
        for e in range(12):
            a, b = edge_corners(e)
            if ((case >> a) & 1) != ((case >> b) & 1):
                edge_mask[case] |= 1 << e
        t = case_triangles(case)
        assert len(t) <= 5, (case, len(t))
        tri[case, :3 * len(t)] = np.array(t, np.int32).reshape(-1)
    return edge_mask, tri


def rows(tri):
    """the rows of pixel-nerf_amd/csrc/pnr_mc_tables.inc"""
    return "\n".join("{" + ", ".join(f"{int(v):2d}" for v in r) + "}," for r in tri) + "\n"


if __name__ == "__main__":
    text = rows(tables()[1])
    if len(sys.argv) == 3 and sys.argv[1] == "--check":
        have = "".join(ln for ln in open(sys.argv[2]) if not ln.startswith("//"))
        print("tables match" if have == text else "tables DIFFER")
        sys.exit(0 if have == text else 1)
    sys.stdout.write(text)
