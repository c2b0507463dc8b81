"""The per-view step that the colours, the bake and the fusion share, the host side (no GPU):
raynet_amd/csrc/raynet_views_args.h as a stand-alone program under the address and
undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter -- and where
the header may be named."""
import os
import re

from conftest import REPO
from host_program import run_host_program

CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def test_the_step_against_a_straight_line_implementation_under_sanitizers(tmp_path):
    run_host_program("views", tmp_path)


def test_the_header_is_plain_guards_its_loads_and_is_stated_once():
    from raynet_amd import _lib
    header = open(os.path.join(CSRC, "raynet_views_args.h")).read()
    code = re.sub(r"//.*", "", header)
    assert "#pragma once" in header and "namespace rn_view" in header
    assert "hip" not in code.lower() and "__device__" not in code and "sqrt" not in code
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", header, re.M)
    assert os.path.join(CSRC, "raynet_views_args.h") in _lib.sources()
    # every image and depth load goes through image_index / map_index with pixel_in-guarded
    # coordinates
    loads = re.findall(r"a\.(images|depths)\[(\w+)\(", code)
    assert sorted(loads) == [("depths", "map_index")] + [("images", "image_index")] * 4
    assert len(re.findall(r"a\.(images|depths)\[", code)) == 5
    assert code.count("pixel_in(yr, a.H) ? yr : 0") == 1 and code.count("pixel_in(xr, a.W) ? xr : 0") == 1
    assert "x0 = pixel_in(x0, a.W) ? x0 : 0;" in code and "y0 = pixel_in(y0, a.H) ? y0 : 0;" in code
    assert "std::min(x0 + 1, a.W - 1)" in code and "std::min(y0 + 1, a.H - 1)" in code
    # the projection of a P | centre row and the lerp are stated here, and once more where
    # k_project_colors keeps the step written out for its speed's sake -- nowhere else (the
    # K | R | t cameras of the depth-map clouds are another definition)
    stated = {"projection": [], "lerp": []}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".inl", ".hip")):
            text = re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())
            stated["projection"] += [name] * text.count("X = h0 / h2")
            stated["lerp"] += [name] * len(re.findall(r"top \+ fy \* \(bot - top\)", text))
    assert stated["projection"] == stated["lerp"] == ["raynet_appearance.inl", "raynet_views_args.h"]
    # the stages take the names from here
    for name, uses in (("raynet_appearance_args.h", "using rn_view::CAMERA_DOUBLES, rn_view::image_index, rn_view::pixel_in;"),
                       ("raynet_fusion_args.h", "using rn_view::CAMERA_DOUBLES, rn_view::map_index, rn_view::pixel_in;")):
        assert uses in open(os.path.join(CSRC, name)).read(), name
    # the older stages do not know the new one
    assert "texture" not in header.lower()
