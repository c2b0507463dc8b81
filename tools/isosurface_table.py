#!/usr/bin/env python3
"""Derive ISO_TRI, the case table of raynet_amd/csrc/raynet_isosurface.inl,
and print it as the C++ initialiser that file holds; --check compares with the file.

For each of the six Kuhn tetrahedra of a cell and each of the 16 inside / outside patterns of its
four corners the table lists at most two triangles, every entry one of the tetrahedron's six
edges.  The order of the entries is the definition's; the last two are swapped where the
right-hand normal would point from outside to inside.  That is decided here in integers: with
the crossings at the edges' midpoints (doubled: lattice points), the sign of
det(v1 - v0, v2 - v0, outside corner - inside corner) for any inside / outside pair of corners --
the surface separates the two, so the sign does not depend on the pair.

A word: bits 0-1 the number of triangles, then 3 bits per entry, triangle 0 from bit 2, triangle
1 from bit 11; an entry is the index of (l, m) in EDGES, l < m local corners.
"""
import itertools
import os
import re
import sys

EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def tets():
    out = []
    for perm in itertools.permutations(range(3)):
        m, t = 0, [0]
        for axis in perm:
            m |= 1 << axis
            t.append(m)
        out.append(t)
    return out


def xyz(mask):
    return [mask & 1, (mask >> 1) & 1, (mask >> 2) & 1]


def det(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) +
            a[2] * (b[0] * c[1] - b[1] * c[0]))


def triangles(tet, case):
    ins = [l for l in range(4) if (case >> l) & 1]
    out = [l for l in range(4) if not (case >> l) & 1]
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in out]]
    elif len(ins) == 3:
        tris = [[(i, out[0]) for i in ins]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    else:
        return []
    result = []
    for tri in tris:
        v = [[p + q for p, q in zip(xyz(tet[l]), xyz(tet[m]))] for l, m in tri]
        e1 = [p - q for p, q in zip(v[1], v[0])]
        e2 = [p - q for p, q in zip(v[2], v[0])]
        signs = set()
        for i in ins:
            for o in out:
                signs.add(det(e1, e2, [p - q for p, q in zip(xyz(tet[o]), xyz(tet[i]))]) > 0)
                assert det(e1, e2, [p - q for p, q in zip(xyz(tet[o]), xyz(tet[i]))]) != 0
        assert len(signs) == 1
        if not signs.pop():
            tri = [tri[0], tri[2], tri[1]]
        result.append([EDGES.index((min(l, m), max(l, m))) for l, m in tri])
    return result


def words():
    out = []
    for tet in tets():
        for case in range(16):
            tris = triangles(tet, case)
            w = len(tris)
            for r, tri in enumerate(tris):
                for e, edge in enumerate(tri):
                    w |= edge << (2 + 9 * r + 3 * e)
            out.append(w)
    return out


def initialiser():
    w = words()
    lines = []
    for t in range(6):
        row = ", ".join("0x%05x" % x for x in w[16 * t:16 * t + 16])
        lines.append("    " + row[:len(row) // 2 + 1].rstrip() + "\n     " + row[len(row) // 2 + 1:] + ",")
    return "\n".join(lines)


def main(argv):
    if "--check" in argv:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "raynet_amd", "csrc", "raynet_isosurface.inl")
        m = re.search(r"ISO_TRI\[96\] = \{(.*?)\};", open(path).read(), re.S)
        have = [int(x, 16) for x in re.findall(r"0x[0-9a-f]+", m.group(1))]
        if have != words():
            print("ISO_TRI in %s differs from the derivation" % path)
            return 1
        print("ISO_TRI: 96 words as derived")
        return 0
    print(initialiser())
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
