"""The halves of tools/quadric_bench.py that need no GPU, as tests/test_mesh_bench_tools.py holds
the other mesh tools: --merge_trace on a synthetic rocprofv3 kernel trace whose durations follow
that file's rule, over a copy of the committed record, and --merge_box."""
import json
import os
import shutil
import subprocess
import sys

from conftest import REPO
from test_mesh_bench_tools import TIMED, TOOLS, duration, merged, run_tool, stats, without_trace

KERNELS = ("k_quadric_clear", "k_quadric_members", "k_quadric_faces", "k_quadric_solve")


def test_the_merge_halves_import_neither_torch_nor_the_package():
    code = ("import sys; sys.path.insert(0, %r); import quadric_bench; "
            "assert quadric_bench.OWN == %r; "
            "assert 'torch' not in sys.modules and 'raynet_amd' not in sys.modules" % (TOOLS, KERNELS))
    r = subprocess.run([sys.executable, "-c", code], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr


def test_the_record_holds_both_placements_and_both_entries():
    record = json.loads(open(os.path.join(REPO, "profiles", "quadric_bench.json")).read())
    assert list(record["meshes"]) == ["mrf_128", "fused_256"]
    assert record["cells_in_voxel_sides"] == [2.0, 4.0] and record["regularization"] == 2.0 ** -10
    for entry in record["meshes"].values():
        for one in entry["cells"].values():
            assert one["place_quadric"]["ms_median"] > 0 and one["simplify"]["ms_median"] > 0
            assert one["workspace_bytes"] == 88 * one["nv_out"]
            assert 0 <= one["moved"] <= one["nv_out"] and 0 <= one["fell_back"] <= one["nv_out"]
            distance = one["distance_to_unsimplified_surface_in_cell_sides"]
            assert set(distance) == {"mean_placement", "quadric_placement"}
            for d in distance.values():
                assert 0 <= d["mean"] <= d["rms"] <= d["max"]


def test_quadric_bench_merges_the_last_dispatches_of_a_trace(tmp_path):
    settings = [(name, cell) for name in ("mrf_128", "fused_256") for cell in ("2", "4")]
    before, after = merged("quadric_bench", tmp_path, KERNELS, [{k: 1 for k in KERNELS}] * 4)
    for s, (name, cell) in enumerate(settings):
        one = after["meshes"][name]["cells"][cell]
        assert without_trace(one) == without_trace(before["meshes"][name]["cells"][cell])
        own = one["kernel_trace"]
        medians = {}
        for j, k in enumerate(KERNELS):
            want = stats([duration(j, s, t) for t in TIMED])
            assert {x: own[k][x] for x in ("ms_min", "ms_median")} == want, (name, cell, k)
            medians[k] = want["ms_median"]
            assert own[k]["GB_per_s"] == round(
                one["bytes_must_move"][k] / (medians[k] * 1e-3) / 1e9, 1)
        assert own["sum_of_kernels_ms"] == round(sum(medians.values()), 4)
    # one dispatch too few of one kernel: nothing is merged
    from test_mesh_bench_tools import write_trace
    trace, out = str(tmp_path / "short.csv"), str(tmp_path / "quadric_bench.json")
    write_trace(trace, KERNELS, [{k: 1 for k in KERNELS}] * 4, 35, earlier=0, extra=-1)
    kept = open(out).read()
    r = run_tool("quadric_bench", "--merge_trace", trace, "--out", out)
    assert r.returncode != 0 and open(out).read() == kept
    assert "k_quadric_clear: 139 dispatches in the trace, expected 140" in r.stderr


def test_merge_box_takes_the_last_line_that_opens_a_brace(tmp_path):
    out, box_file = str(tmp_path / "quadric_bench.json"), str(tmp_path / "bench.txt")
    shutil.copy(os.path.join(REPO, "profiles", "quadric_bench.json"), out)
    before = json.loads(open(out).read())
    box = {"metric": "images_per_s", "value": 12.5, "gpus": 1}
    with open(box_file, "w") as f:
        f.write("warming up\n" + json.dumps({"value": -1.0}) + "\n  " + json.dumps(box) + "\n\ndone\n")
    r = run_tool("quadric_bench", "--merge_box", box_file, "--out", out)
    assert r.returncode == 0, r.stderr
    after = json.loads(r.stdout)
    assert after["box"] == box
    assert {k: v for k, v in after.items() if k != "box"} == \
        {k: v for k, v in before.items() if k != "box"}
