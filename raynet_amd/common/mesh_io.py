"""Readers of the ground-truth meshes and point clouds of the two dataset layouts.

A Restrepo scene ships its ground truth as `gt_mesh.obj` or `gt_mesh.ply`
(raynet/common/parse_input_data.py:60-153), a DTU scan as the binary point cloud
`Points/stl/stl%03d_total.ply` (parse_input_data.py:163-258).  One PLY reader serves both: it
parses the header (elements, properties, format) instead of assuming the reference's fixed
13 header lines, and reads `ascii`, `binary_little_endian` and `binary_big_endian` bodies.
Host-side parsing only.  These files come from outside: malformed input is an error with a
message that names the file.
"""
import os

import numpy as np


class MeshFormatError(ValueError):
    pass


_PLY_TYPES = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1",
    "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
    "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
    "float": "f4", "float32": "f4", "double": "f8", "float64": "f8",
}


class PlyElement(object):
    def __init__(self, name, count):
        self.name, self.count = name, count
        self.properties = []    # (name, dtype) or (name, (count dtype, item dtype)) for lists


def _read_ply_header(f, path):
    if f.readline().strip() != b"ply":
        raise MeshFormatError("%s: not a PLY file" % path)
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise MeshFormatError("%s: no end_header" % path)
        words = line.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            if len(words) < 2 or words[1] not in ("ascii", "binary_little_endian",
                                                   "binary_big_endian"):
                raise MeshFormatError("%s: unknown format line %r" % (path, line))
            fmt = words[1]
        elif words[0] == "element":
            if len(words) != 3:
                raise MeshFormatError("%s: bad element line %r" % (path, line))
            elements.append(PlyElement(words[1], int(words[2])))
        elif words[0] == "property":
            if not elements:
                raise MeshFormatError("%s: property before any element" % path)
            if len(words) == 5 and words[1] == "list":
                if words[2] not in _PLY_TYPES or words[3] not in _PLY_TYPES:
                    raise MeshFormatError("%s: bad property line %r" % (path, line))
                elements[-1].properties.append(
                    (words[4], (_PLY_TYPES[words[2]], _PLY_TYPES[words[3]])))
            elif len(words) == 3 and words[1] in _PLY_TYPES:
                elements[-1].properties.append((words[2], _PLY_TYPES[words[1]]))
            else:
                raise MeshFormatError("%s: bad property line %r" % (path, line))
        else:
            raise MeshFormatError("%s: unknown header line %r" % (path, line))
    if fmt is None:
        raise MeshFormatError("%s: no format line" % path)
    return fmt, elements


def _fixed_rows(el, path):
    return MeshFormatError("%s: the rows of element %s have lists of different lengths (faces: "
                           "only triangles are supported)" % (path, el.name))


def _read_element_ascii(tokens, pos, el, path):
    """One element from the token stream, every row laid out like its first one (a list's
    length read there): ({property: [count] or [count, k] array}, new pos)."""
    if el.count == 0:
        return {n: np.zeros((0,), t if not isinstance(t, tuple) else t[1])
                for n, t in el.properties}, pos
    try:
        cols, w = [], 0
        for n, t in el.properties:        # the first row's layout: (column, list length)
            c = int(tokens[pos + w]) if isinstance(t, tuple) else None
            cols.append((w, c))
            w += 1 + (c or 0) if c is not None else 1
        block = np.array(tokens[pos:pos + el.count * w], dtype=np.float64).reshape(el.count, w)
    except (IndexError, ValueError):
        raise MeshFormatError("%s: element %s is truncated or malformed" % (path, el.name))
    out = {}
    for (n, t), (j, c) in zip(el.properties, cols):
        if c is None:
            out[n] = block[:, j].astype(t)
        else:
            if (block[:, j] != c).any():
                raise _fixed_rows(el, path)
            out[n] = block[:, j + 1:j + 1 + c].astype(t[1])
    return out, pos + el.count * w


def _read_element_binary(buf, pos, el, order, path):
    """As _read_element_ascii, for a binary body: one structured read."""
    fields, off = [], pos
    try:
        for n, t in el.properties:
            if isinstance(t, tuple):
                c = int(np.frombuffer(buf, order + t[0], 1, off)[0]) if el.count else 0
                fields += [(n + "#count", order + t[0]), (n, order + t[1], (c,))]
            else:
                fields.append((n, order + t))
            off = pos + np.dtype(fields).itemsize
        dt = np.dtype(fields)
        rec = np.frombuffer(buf, dtype=dt, count=el.count, offset=pos)
    except ValueError:
        raise MeshFormatError("%s: element %s is truncated" % (path, el.name))
    out = {}
    for n, t in el.properties:
        if isinstance(t, tuple):
            if (rec[n + "#count"] != dt[n].shape[0]).any():
                raise _fixed_rows(el, path)
            out[n] = rec[n].astype(t[1])
        else:
            out[n] = rec[n].astype(t)
    return out, pos + el.count * dt.itemsize


def read_ply(path):
    """{element name: {property name: array}}: a scalar property as a [count] array, a list
    property as a [count, k] array (every row of an element must have lists of the same
    lengths)."""
    with open(path, "rb") as f:
        fmt, elements = _read_ply_header(f, path)
        body = f.read()
    if fmt == "ascii":
        body = body.split()
    order = "<" if fmt == "binary_little_endian" else ">"
    out, pos = {}, 0
    for el in elements:
        if fmt == "ascii":
            out[el.name], pos = _read_element_ascii(body, pos, el, path)
        else:
            out[el.name], pos = _read_element_binary(body, pos, el, order, path)
    return out


def _check_faces(faces, n_vertices, path):
    if len(faces) and (faces.min() < 0 or faces.max() >= n_vertices):
        raise MeshFormatError("%s: a face refers to a vertex outside 0..%d" % (path, n_vertices - 1))
    return faces


def parse_gt_data_from_ply(path):
    """(points [V,3] f32, normals [V,k] f32 (the vertex properties after x, y, z; k may be 0),
    faces [T,3] int64) -- what parse_input_data.py:60-90 returns for its fixed layout."""
    data = read_ply(path)
    if "vertex" not in data or not all(c in data["vertex"] for c in "xyz"):
        raise MeshFormatError("%s: no vertex element with x, y, z" % path)
    v = data["vertex"]
    points = np.stack([v[c] for c in "xyz"], axis=1).astype(np.float32)
    rest = [n for n in v if n not in ("x", "y", "z") and v[n].ndim == 1]
    normals = (np.stack([v[n] for n in rest], axis=1).astype(np.float32) if rest
               else np.zeros((len(points), 0), np.float32))
    faces = np.zeros((0, 3), np.int64)
    if "face" in data:
        lists = [p for p in data["face"].values() if p.ndim == 2]
        if len(lists) != 1:
            raise MeshFormatError("%s: the face element needs exactly one list property" % path)
        if len(lists[0]) and lists[0].shape[1] != 3:      # (`element face 0`: lists of no length)
            raise MeshFormatError("%s: faces have %d vertices; only triangles are supported"
                                  % (path, lists[0].shape[1]))
        if len(lists[0]):
            faces = lists[0].astype(np.int64)
    return points, normals, _check_faces(faces, len(points), path)


def parse_gt_data_from_obj(path):
    """(points [V,3] f32, normals [N,3] f32, faces [T,3] int64) from `v`, `vn` and `f` lines
    (parse_input_data.py:93-137); a face index is the integer before the first '/'."""
    vertices, normals, faces = [], [], []
    with open(path, "r") as f:
        for ln, line in enumerate(f, 1):
            words = line.split()
            if not words:
                continue
            try:
                if words[0] == "v":
                    vertices.append([float(x) for x in words[1:4]])
                    if len(vertices[-1]) != 3:
                        raise ValueError
                elif words[0] == "vn":
                    normals.append([float(x) for x in words[1:4]])
                    if len(normals[-1]) != 3:
                        raise ValueError
                elif words[0] == "f":
                    idx = [int(w.split("/")[0]) for w in words[1:]]
                    if len(idx) != 3:
                        raise MeshFormatError(
                            "%s:%d: face with %d vertices; only triangles are supported"
                            % (path, ln, len(idx)))
                    # 1-based; negative indices count back from the last vertex read
                    faces.append([i - 1 if i > 0 else len(vertices) + i for i in idx])
            except MeshFormatError:
                raise
            except ValueError:
                raise MeshFormatError("%s:%d: malformed line %r" % (path, ln, line))
    points = np.array(vertices, dtype=np.float32).reshape(-1, 3)
    return (points, np.array(normals, dtype=np.float32).reshape(-1, 3),
            _check_faces(np.array(faces, dtype=np.int64).reshape(-1, 3), len(points), path))


def gt_mesh_file(directory):
    """The ground-truth mesh of a Restrepo scene: gt_mesh.obj before gt_mesh.ply
    (parse_input_data.py:140-153); None if neither exists."""
    for name in ("gt_mesh.obj", "gt_mesh.ply"):
        p = os.path.join(directory, name)
        if os.path.isfile(p):
            return p
    return None


def parse_gt_data(directory):
    """(points [V,3] f32, normals, faces [T,3] int64) of a scene directory's ground truth."""
    path = gt_mesh_file(directory)
    if path is None:
        raise FileNotFoundError("no gt_mesh.obj or gt_mesh.ply in %s" % directory)
    if path.endswith(".obj"):
        return parse_gt_data_from_obj(path)
    return parse_gt_data_from_ply(path)


def get_triangles(points, faces):
    """[T, 9] float32 rows p0 | p1 | p2 (training_utils.py:179-191)."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.ascontiguousarray(points[faces].reshape(-1, 9))


def parse_stl_file_to_pointcloud(path):
    """Points [V,3] f32 of a DTU STL point cloud (parse_input_data.py:243-258): the x, y, z
    properties of the vertex element of a PLY file of any of the three formats."""
    data = read_ply(path)
    if "vertex" not in data or not all(c in data["vertex"] for c in "xyz"):
        raise MeshFormatError("%s: no vertex element with x, y, z" % path)
    return np.stack([data["vertex"][c] for c in "xyz"], axis=1).astype(np.float32)
