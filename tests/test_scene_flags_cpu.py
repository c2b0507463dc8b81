"""The scene flags of the seven scripts that open a scene (raynet_amd/scripts/scene_flags.py, no
GPU, no torch): every script's scene flags against the literal table read off the parsers before
the flags had a module; the --start_end usage error; the frames the flags choose; the per-frame
maps they load; the scene they open; and mesh_flags.voxel_diagonal against the expression it
replaces."""
import importlib
import os
import types

import numpy as np
import pytest

INTS, FRAME_IDXS = "ints", "frame_idxs_type"        # the types that are the module's own functions

# dest -> (default, type, choices, help), the same in every script that has the flag ...
DATASET = {
    "dataset_type": ("restrepo", None, ["restrepo", "dtu"], None),
    "select_neighbors_based_on": ("filesystem", None, ["filesystem", "distance"], None),
    "illumination_condition": ("max", None, None, None),
}
START_END = {
    "start_end": ("0,5", INTS, None, None),
    "skip_every": (0, int, None, None),
}
FRAME_IDXS_FLAG = {
    "frame_idxs": (":", FRAME_IDXS, None,
                   "Choose the frames that correspond to the ordered prediction files"),
}


def _scene_idx(default):
    return {"scene_idx": (default, int, None, "DTU: the scan number")}


# ... and per script: the two that name their output after the scan default to scan 0 and choose
# frames with --frame_idxs, the five others default to scan 1 and choose with --start_end
PARENT = {
    "forward_pass": dict(DATASET, **START_END, **_scene_idx(1)),
    "render_volume": dict(DATASET, **START_END, **_scene_idx(1)),
    "render_mesh": dict(DATASET, **START_END, **_scene_idx(1)),
    "fuse_depth_maps": dict(DATASET, **START_END, **_scene_idx(1)),
    "filter_depth_maps": dict(DATASET, **START_END, **_scene_idx(1)),
    "compute_metrics": dict(DATASET, **FRAME_IDXS_FLAG, **_scene_idx(0)),
    "convert_to_pointcloud": dict(DATASET, **FRAME_IDXS_FLAG, **_scene_idx(0)),
}
ALL_SCENE_FLAGS = set(DATASET) | set(START_END) | set(FRAME_IDXS_FLAG) | {"scene_idx"}
# the positional arguments each script wants before its flags
POSITIONALS = {
    "forward_pass": ["scene", "out"],
    "render_volume": ["scene", "occupancy.npz", "out"],
    "render_mesh": ["scene", "mesh.ply", "out"],
    "fuse_depth_maps": ["scene", "predictions", "out.ply"],
    "filter_depth_maps": ["scene", "predictions", "out"],
}


def _script(name):
    return importlib.import_module("raynet_amd.scripts." + name)


@pytest.mark.parametrize("name", sorted(PARENT))
def test_every_script_keeps_its_scene_flags(name):
    from raynet_amd.scripts import scene_flags
    own = {INTS: scene_flags.ints, FRAME_IDXS: scene_flags.frame_idxs_type}
    got = {a.dest: (a.default, a.type, a.choices, a.help)
           for a in _script(name).build_parser()._actions if a.dest in ALL_SCENE_FLAGS}
    want = {dest: (default, own.get(type_, type_), choices, help_)
            for dest, (default, type_, choices, help_) in PARENT[name].items()}
    assert got == want
    assert scene_flags.ints("3,04,-5") == (3, 4, -5)


@pytest.mark.parametrize("value", ["3", "0,1,2"])
@pytest.mark.parametrize("name", sorted(POSITIONALS))
def test_a_start_end_that_is_no_pair_is_a_usage_error(name, value, tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        _script(name).main(POSITIONALS[name] + ["--start_end", value])
    err = capsys.readouterr().err
    assert e.value.code == 2 and err.startswith("usage: ")
    assert err.endswith(": error: --start_end takes two numbers, START,END\n")
    assert os.listdir(str(tmp_path)) == []


class _Parser(object):
    def error(self, message):
        raise SystemExit(message)


def _frames(script, argv, required=True):
    from raynet_amd.scripts import scene_flags
    parser = _script(script).build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    return scene_flags.frames(_Parser(), args, types.SimpleNamespace(n_images=7), required)


def test_frames_of_start_end_are_clamped_to_the_scene():
    base = POSITIONALS["fuse_depth_maps"]
    assert _frames("fuse_depth_maps", base) == [0, 1, 2, 3, 4]                  # the default 0,5
    assert _frames("fuse_depth_maps", base + ["--start_end", "0,5", "--skip_every", "0"]) == \
        [0, 1, 2, 3, 4]
    assert _frames("fuse_depth_maps", base + ["--start_end", "2,100", "--skip_every", "2"]) == [2, 5]
    with pytest.raises(SystemExit) as e:
        _frames("fuse_depth_maps", base + ["--start_end", "5,5"])
    assert str(e.value) == "--start_end selects no frame of the scene"
    assert _frames("fuse_depth_maps", base + ["--start_end", "5,5"], required=False) == []


def test_frames_of_frame_idxs_index_the_scene():
    base = ["scene", "predictions", "out"]
    got = _frames("convert_to_pointcloud", base + ["--frame_idxs", "1,4"])
    assert got == [1, 4] and all(type(i) is int for i in got)
    assert _frames("convert_to_pointcloud", base + ["--frame_idxs", ":"]) == list(range(7))
    assert _frames("convert_to_pointcloud", base) == list(range(7))             # the default ":"
    assert _frames("compute_metrics", base[:2] + ["ppmde", "--frame_idxs", "1:6:2"]) == [1, 3, 5]


def test_load_maps_finds_the_format_reports_the_missing_and_keeps_the_dtype(tmp_path):
    from raynet_amd.scripts import scene_flags
    d = str(tmp_path)
    maps = {i: (np.arange(6).reshape(2, 3) + i).astype(np.float64) for i in (3, 4, 12)}
    for i, m in maps.items():
        np.save(os.path.join(d, "depth_%03d.npy" % i), m)
    got = scene_flags.load_maps(_Parser(), d, "depth", [3, 4, 12])              # the padded names
    assert all(g.dtype == np.float64 and np.array_equal(g, maps[i])
               for g, i in zip(got, (3, 4, 12)))
    for i in (3, 4):                                        # the first frame decides: unpadded now
        np.save(os.path.join(d, "depth_%d.npy" % i), maps[i].astype(np.float16))
    got = scene_flags.load_maps(_Parser(), d, "depth", [3, 4])
    assert all(g.dtype == np.float16 and np.array_equal(g, maps[i]) for g, i in zip(got, (3, 4)))
    np.save(os.path.join(d, "confidence_1.npy"), np.ones((2, 3), np.uint8))
    assert scene_flags.load_maps(_Parser(), d, "confidence", [1])[0].dtype == np.uint8
    with pytest.raises(SystemExit) as e:
        scene_flags.load_maps(_Parser(), d, "depth", [3, 5, 4])
    assert str(e.value) == "1 of 3 depth maps are missing (first: %s)" % os.path.join(d, "depth_5.npy")
    with pytest.raises(SystemExit) as e:                    # the key is the one asked for
        scene_flags.load_maps(_Parser(), d, "confidence", [7, 8])
    assert str(e.value) == ("2 of 2 confidence maps are missing (first: %s)"
                            % os.path.join(d, "confidence_007.npy"))


def test_open_scene_passes_what_each_layout_takes(monkeypatch):
    import raynet_amd.common.scene as scene_module
    from raynet_amd.scripts import scene_flags
    calls = []
    monkeypatch.setattr(scene_module, "get_scene",
                        lambda *a, **k: calls.append((a, k)) or "the scene")
    args = types.SimpleNamespace(dataset_type="dtu", dataset_directory="root", scene_idx=9,
                                 illumination_condition="3_r5000",
                                 select_neighbors_based_on="distance")
    assert scene_flags.open_scene(args) == "the scene"
    args.dataset_type = "restrepo"
    assert scene_flags.open_scene(args) == "the scene"
    assert calls == [
        (("dtu", "root", 9), dict(illumination="3_r5000", select_neighbors_based_on="distance")),
        (("restrepo", "root"), dict(select_neighbors_based_on="distance"))]


def test_voxel_diagonal_is_the_expression_it_replaces():
    from raynet_amd.scripts import mesh_flags
    volume = types.SimpleNamespace(bbox=np.array([-1.0, 0.5, 2.0, 3.3, 2.6, 2.9], np.float32),
                                   grid_shape=(7, 5, 3))
    sides = mesh_flags.voxel_sides(volume)
    assert len(set(sides.tolist())) == 3
    want = float(np.sqrt((mesh_flags.voxel_sides(volume) ** 2).sum()))
    got = mesh_flags.voxel_diagonal(volume)
    assert type(got) is float and got == want and got.hex() == want.hex()
