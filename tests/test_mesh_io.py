"""Readers of ground-truth meshes and point clouds (raynet_amd/common/mesh_io.py), the
DTU STL point cloud through DTUScene, and the no-GPU refusal of MeshRaycaster.  CPU only."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], np.float32)
FACES = np.array([[0, 1, 2], [0, 2, 3], [1, 3, 2]])


def test_obj_face_forms(tmp_path):
    from raynet_amd.common.mesh_io import get_triangles, parse_gt_data
    with open(tmp_path / "gt_mesh.obj", "w") as f:
        f.write("# comment\no thing\n")
        for p in TRI:
            f.write("v  %r %r %r\n" % tuple(float(x) for x in p))
        f.write("vn 0 0 1\nvn 0 1 0\nvt 0.5 0.5\n")
        f.write("f 1 2 3\n")              # i
        f.write("f 1//1 3//2 4//1\n")     # i//n
        f.write("f 2/1/1 4/1/2 3/1/1\n")  # i/t/n
    points, normals, faces = parse_gt_data(str(tmp_path))
    assert points.dtype == np.float32 and np.array_equal(points, TRI)
    assert normals.shape == (2, 3)
    assert np.array_equal(faces, FACES)
    tri = get_triangles(points, faces)
    assert tri.shape == (3, 9) and tri.dtype == np.float32
    assert np.array_equal(tri[1], np.concatenate([TRI[0], TRI[2], TRI[3]]))


def _ply_header(fmt, n_v, n_f, extra_v=(), face_count="uchar", face_idx="int", comments=0):
    h = ["ply", "format %s 1.0" % fmt] + ["comment line %d" % i for i in range(comments)]
    h += ["obj_info made by a test", "element vertex %d" % n_v, "property float x",
          "property float y", "property float z"]
    h += ["property %s %s" % (t, n) for n, t in extra_v]
    h += ["element face %d" % n_f, "property list %s %s vertex_indices" % (face_count, face_idx),
          "property uchar red", "end_header"] if n_f is not None else ["end_header"]
    return ("\n".join(h) + "\n").encode()


def test_ascii_ply_with_a_long_header(tmp_path):
    from raynet_amd.common.mesh_io import parse_gt_data
    p = tmp_path / "gt_mesh.ply"
    with open(p, "wb") as f:
        f.write(_ply_header("ascii", 4, 3, extra_v=[("nx", "float"), ("ny", "float"),
                                                   ("nz", "float")], comments=25))
        for q in TRI:
            f.write(("%r %r %r 0 0 1\n" % tuple(float(x) for x in q)).encode())
        for fc in FACES:
            f.write(("3  %d %d %d 7\n" % tuple(fc)).encode())
    points, normals, faces = parse_gt_data(str(tmp_path))
    assert np.array_equal(points, TRI) and normals.shape == (4, 3)
    assert np.array_equal(faces, FACES)


@pytest.mark.parametrize("order,fmt", [("<", "binary_little_endian"), (">", "binary_big_endian")])
def test_binary_ply_with_extra_properties(tmp_path, order, fmt):
    from raynet_amd.common.mesh_io import parse_gt_data, parse_stl_file_to_pointcloud
    p = tmp_path / "gt_mesh.ply"
    vdt = np.dtype([("x", order + "f4"), ("y", order + "f4"), ("z", order + "f4"),
                    ("q", order + "f8"), ("c", "u1")])
    v = np.zeros(4, vdt)
    v["x"], v["y"], v["z"] = TRI[:, 0], TRI[:, 1], TRI[:, 2]
    v["q"], v["c"] = 2.5, 9
    fdt = np.dtype([("n", "u1"), ("i", order + "i4", (3,)), ("red", "u1")])
    fc = np.zeros(3, fdt)
    fc["n"], fc["i"], fc["red"] = 3, FACES, 4
    with open(p, "wb") as f:
        f.write(_ply_header(fmt, 4, 3, extra_v=[("q", "double"), ("c", "uchar")]))
        f.write(v.tobytes())
        f.write(fc.tobytes())
    points, normals, faces = parse_gt_data(str(tmp_path))
    assert np.array_equal(points, TRI) and np.array_equal(faces, FACES)
    assert normals.shape == (4, 2) and (normals[:, 0] == 2.5).all()
    assert np.array_equal(parse_stl_file_to_pointcloud(str(p)), TRI)


def test_non_triangles_and_bad_input_are_rejected(tmp_path):
    from raynet_amd.common.mesh_io import MeshFormatError, parse_gt_data_from_obj, \
        parse_gt_data_from_ply
    obj = tmp_path / "quad.obj"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    with pytest.raises(MeshFormatError, match="only triangles"):
        parse_gt_data_from_obj(str(obj))
    ply = tmp_path / "quad.ply"
    with open(ply, "wb") as f:
        f.write(_ply_header("ascii", 4, 2))
        f.write(b"0 0 0\n1 0 0\n1 1 0\n0 1 0\n3 0 1 2 0\n4 0 1 2 3 0\n")
    with pytest.raises(MeshFormatError, match="only triangles"):
        parse_gt_data_from_ply(str(ply))
    bad = tmp_path / "bad.ply"
    bad.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nend_header\n1\n")
    with pytest.raises(MeshFormatError):
        parse_gt_data_from_ply(str(bad))
    oob = tmp_path / "oob.obj"
    oob.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1 2 9\n")
    with pytest.raises(MeshFormatError, match="outside"):
        parse_gt_data_from_obj(str(oob))


def test_obj_before_ply(tmp_path):
    from raynet_amd.common.mesh_io import gt_mesh_file, parse_gt_data
    with open(tmp_path / "gt_mesh.ply", "wb") as f:
        f.write(_ply_header("ascii", 3, 1))
        f.write(b"0 0 0\n1 0 0\n0 1 0\n3 0 1 2 0\n")
    assert gt_mesh_file(str(tmp_path)).endswith("gt_mesh.ply")
    (tmp_path / "gt_mesh.obj").write_text("v 0 0 5\nv 1 0 5\nv 0 1 5\nf 1 2 3\n")
    assert gt_mesh_file(str(tmp_path)).endswith("gt_mesh.obj")
    assert parse_gt_data(str(tmp_path))[0][0, 2] == 5


def test_fixture_parses_equal_to_the_reference():
    from raynet_amd.common.mesh_io import get_triangles, parse_gt_data_from_ply
    g = np.load(os.path.join(GOLDEN, "ref_raycast.npz"))
    points, normals, faces = parse_gt_data_from_ply(os.path.join(GOLDEN, "raycast_city.ply"))
    assert np.array_equal(points, g["ref_points"]) and points.dtype == np.float32
    assert np.array_equal(faces, g["ref_faces"]) and normals.shape == (len(points), 0)
    assert np.array_equal(get_triangles(points, faces), g["ref_triangles"])
    tri = g["ref_triangles"].reshape(-1, 3, 3)
    assert (tri.min((0, 1)) >= [-5, -5, -0.7]).all() and (tri.max((0, 1)) <= [5, 5, 1.5]).all()


def test_dtu_scene_pointcloud(tmp_path):
    from raynet_amd.common.scene import DTUScene
    base = tmp_path / "dtu"
    os.makedirs(base / "Rectified" / "scan006")
    os.makedirs(base / "SampleSet/MVS_Data/Calibration/cal18")
    os.makedirs(base / "Points" / "stl")
    rng = np.random.default_rng(0)
    pts = rng.normal(0, 100, (1000, 3)).astype(np.float32)
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                    ("blue", "u1"), ("alpha", "u1")])
    v = np.zeros(len(pts), vdt)
    v["x"], v["y"], v["z"] = pts.T
    with open(base / "Points" / "stl" / "stl006_total.ply", "wb") as f:
        f.write(_ply_header("binary_little_endian", len(pts), None,
                            extra_v=[("red", "uchar"), ("green", "uchar"), ("blue", "uchar"),
                                     ("alpha", "uchar")]))
        f.write(v.tobytes())
    s = DTUScene(str(base), 6)
    pc = s.get_pointcloud()
    assert pc.points.shape == (3, 1000) and np.array_equal(pc.points.T, pts)


def test_mesh_raycaster_without_a_gpu_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from raynet_amd import _lib
    from raynet_amd.mesh import MeshRaycaster
    with pytest.raises(_lib.RaynetHipError):
        MeshRaycaster(np.zeros((1, 9), np.float32))


def test_restrepo_scene_without_mesh_or_maps_still_raises(tmp_path):
    import shutil
    from PIL import Image as PILImage
    from raynet_amd.common.scene import RestrepoScene
    dst = str(tmp_path / "s")
    shutil.copytree(os.path.join(GOLDEN, "restrepo_mock_scene_1"), dst)
    os.makedirs(os.path.join(dst, "imgs"))
    for c in sorted(os.listdir(os.path.join(dst, "cams_krt")))[:2]:
        PILImage.fromarray(np.zeros((9, 16, 3), np.uint8)).save(
            os.path.join(dst, "imgs", c.replace("_cam.txt", ".png")))
    s = RestrepoScene(dst)
    with pytest.raises(NotImplementedError):
        s.get_depth_map(0)
    with pytest.raises(NotImplementedError):
        s.get_depth_for_pixel(0, 1, 1)
