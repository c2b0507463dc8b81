"""The argument checks and the output addressing of rn_occupancy_grid / rn_volume_render
(raynet_amd/csrc/raynet_volume_args.h) as a stand-alone host program under the address and the
undefined-behaviour sanitizers: tests/volume_args_main.cpp, compiled with g++ and run here --
no GPU, no HIP, nothing loaded into this interpreter."""
import os

from host_program import REPO, run_host_program


def test_launcher_argument_checks_under_sanitizers(tmp_path):
    run_host_program("volume", tmp_path)


def test_the_launchers_use_these_checks():
    """raynet_volume.inl decides on the header's verdicts and addresses `out` with its function."""
    src = open(os.path.join(REPO, "raynet_amd", "csrc", "raynet_volume.inl")).read()
    assert "rn_volume::render_args(" in src and "rn_volume::grid_args(" in src
    assert src.count("rn_volume::out_index(") == 5
