"""The argument checks and the output addressing of rn_occupancy_grid / rn_volume_render
(raynet_amd/csrc/raynet_volume_args.h) as a stand-alone host program under the address and the
undefined-behaviour sanitizers: tests/volume_args_main.cpp, compiled with g++ and run here --
no GPU, no HIP, nothing loaded into this interpreter."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launcher_argument_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "volume_args")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall",
                           "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "raynet_amd", "csrc"),
                           os.path.join(REPO, "tests", "volume_args_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("volume_args: ok"), r.stdout


def test_the_launchers_use_these_checks():
    """raynet_volume.inl decides on the header's verdicts and addresses `out` with its function."""
    src = open(os.path.join(REPO, "raynet_amd", "csrc", "raynet_volume.inl")).read()
    assert "rn_volume::render_args(" in src and "rn_volume::grid_args(" in src
    assert src.count("rn_volume::out_index(") == 5
