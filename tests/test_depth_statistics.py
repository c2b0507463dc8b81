"""Depth statistics, the parts that need no GPU: the C ABI's declaration and its ctypes mirror,
the scripts' flags, and the schedule that cannot provide them."""
import ctypes
import re

import numpy as np
import pytest

from raynet_amd import _lib

# rn_scene_plan as it was before the statistics fields: their offsets must never move
PLAN_FIELDS_BEFORE = [
    "n_images", "n", "rows_per_image", "ray_idxs", "order", "features_views", "cameras", "vox",
    "rvc", "Sr", "msgs", "ray_segments", "acc", "acc_fixed", "depth", "prior", "row_layout",
    "depth_image", "depth_image_stride", "sweep_xcd_chunk"]
PLAN_FIELDS_NEW = ["stats", "stats_image", "stats_image_stride"]


def _header():
    return open(_lib.HEADER).read()


def _plan_fields_of_header():
    """[(name, ctypes type)] of rn_scene_plan in the header's order."""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} rn_scene_plan;", text).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"^(.*?)(\w+)(\[(\d+)\])?$", decl)
        ctype, name, count = m.group(1).strip(), m.group(2), m.group(4)
        if "*" in ctype:
            t = ctypes.c_void_p
        else:
            t = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[ctype]
        fields.append((name, t * int(count) if count else t))
    return fields


def test_entry_is_declared_and_mirrored():
    text = " ".join(_header().split())
    m = re.search(r"int rn_scene_depth_stats\(([^)]*)\);", text)
    assert m, "include/raynet_hip.h does not declare rn_scene_depth_stats"
    params = [p.strip() for p in m.group(1).split(",")]
    # rn_scene_depth's arguments plus `float *stats, int64_t stats_stride` before the stream
    plain = [p.strip() for p in re.search(r"int rn_scene_depth\(([^)]*)\);", text).group(1).split(",")]
    assert params == plain[:-1] + ["float *stats", "int64_t stats_stride"] + plain[-1:]
    sig = _lib.SIGNATURES["rn_scene_depth_stats"]
    assert sig == _lib.SIGNATURES["rn_scene_depth"][:-1] + [ctypes.c_void_p, ctypes.c_int64,
                                                             ctypes.c_void_p]
    assert len(sig) == len(params)


def test_plan_mirror_matches_the_header():
    fields = _plan_fields_of_header()
    names = [n for n, _ in fields]
    assert names == PLAN_FIELDS_BEFORE + PLAN_FIELDS_NEW        # appended at the end
    from_header = type("PlanFromHeader", (ctypes.Structure,), {"_fields_": fields})
    before = type("PlanBefore", (ctypes.Structure,),
                  {"_fields_": fields[:len(PLAN_FIELDS_BEFORE)]})
    mirror = _lib.ScenePlan
    assert [n for n, _ in mirror._fields_] == names
    assert ctypes.sizeof(mirror) == ctypes.sizeof(from_header)
    for name in names:
        assert getattr(mirror, name).offset == getattr(from_header, name).offset, name
        assert getattr(mirror, name).size == getattr(from_header, name).size, name
    for name in PLAN_FIELDS_BEFORE:                              # ... and no old offset moved
        assert getattr(mirror, name).offset == getattr(before, name).offset, name
    # a zero-initialised mirror asks for no statistics
    pl = mirror()
    assert pl.stats is None and pl.stats_image is None and pl.stats_image_stride == 0


def test_forward_pass_script_flag():
    from raynet_amd.scripts import forward_pass as script
    p = script.build_parser()
    assert p.parse_args(["in", "out"]).depth_statistics is False
    assert p.parse_args(["in", "out", "--depth_statistics"]).depth_statistics is True
    with pytest.raises(SystemExit):       # the literal schedule has no distribution to keep
        script.main(["in", "out", "--depth_statistics", "--schedule", "reference"])
    with pytest.raises(SystemExit):
        script.main(["in", "out", "--depth_statistics", "--forward_pass_factory", "multi_view_cnn"])


def test_convert_to_pointcloud_flag(tmp_path):
    from raynet_amd.scripts import convert_to_pointcloud as script
    p = script.build_parser()
    assert p.parse_args(["d", "p", "o"]).min_confidence is None
    assert p.parse_args(["d", "p", "o", "--min_confidence", "0.25"]).min_confidence == 0.25

    class Scene(object):
        n_images = 3
        observation_mask = None

    # the confidence maps are looked for before anything touches a GPU: a clear message
    args = p.parse_args(["d", str(tmp_path), str(tmp_path / "out"), "--min_confidence", "0.5"])
    args.frame_idxs = slice(None)
    for i in range(3):
        np.save(str(tmp_path / ("depth_%03d.npy" % i)), np.zeros((4, 4), np.float32))
    np.save(str(tmp_path / "confidence_000.npy"), np.zeros((4, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        script.run(Scene(), args)
    assert "confidence_001.npy" in str(e.value) and "--depth_statistics" in str(e.value)


def test_reference_schedule_refuses_statistics():
    from raynet_amd.forward_pass import DepthStatistics, get_forward_pass_factory
    fp = get_forward_pass_factory("raynet")(None, None, "sample_in_bbox", (4, 4), 0,
                                            schedule="reference")
    with pytest.raises(ValueError, match="resident"):
        fp.forward_pass(None, (0, 1, 1), with_statistics=True)
    s = DepthStatistics(1, 2, 3)
    assert (s.confidence, s.expected_depth, s.depth_std) == (1, 2, 3) == tuple(s)
    assert DepthStatistics.FIELDS == ("confidence", "expected_depth", "depth_std")
