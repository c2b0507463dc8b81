"""The halves of tools/{components,smooth,simplify,holes}_bench.py that need no GPU: --merge_trace on
a synthetic rocprofv3 kernel trace whose durations follow a rule stated here, over a copy of the
committed record, and --merge_box.  Every figure asserted is computed from the rule."""
import csv
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

TOOLS = os.path.join(REPO, "tools")
GAP = 500               # ns between two dispatches
JUNK = 9000000          # ns an earlier dispatch of the same kernel takes: 9 ms, to be ignored


def duration(kernel, setting, turn, launch=0):
    """The rule, in ns: kernel j of the tool's list, in setting s (a mesh, or a mesh and a
    parameter, in the tool's order), in turn t, launch l of that turn."""
    return 1000 * (100 * (kernel + 1) + 7 * setting + turn) + 13 * launch


def stats(ns, launches=1):
    """min and median, in ms to four decimals, of the dispatches' times -- of every `launches`
    of them added up, where a turn has several."""
    ms = [x * 1e-6 for x in ns]
    ms = [sum(ms[i:i + launches]) for i in range(0, len(ms), launches)]
    return {"ms_min": round(float(min(ms)), 4), "ms_median": round(float(np.median(ms)), 4)}


def write_trace(path, kernels, plan, turns, earlier=3, extra=0):
    """The run as a kernel trace: `earlier` dispatches of every kernel first (what built the
    meshes), then per setting of the plan [{kernel: launches per turn}] the turns, every kernel in
    order; `extra` dispatches more (or, negative, fewer) of the first kernel.  Rows are written
    last dispatch first: the tools sort by start."""
    rows, clock = [], 1000000

    def dispatch(name, ns):
        nonlocal clock
        rows.append({"Kind": "KERNEL_DISPATCH", "Kernel_Name": "void %s(Args) [clone .kd]" % name,
                     "Start_Timestamp": clock, "End_Timestamp": clock + ns})
        clock += ns + GAP

    for name in kernels:
        for _ in range(earlier):
            dispatch(name, JUNK)
        dispatch("k_some_other_kernel", JUNK)
    for _ in range(max(extra, 0)):
        dispatch(kernels[0], JUNK)
    skip = -min(extra, 0)
    for s, per_turn in enumerate(plan):
        for t in range(turns):
            for j, name in enumerate(kernels):
                for l in range(per_turn[name]):
                    if j == 0 and skip:
                        skip -= 1
                        continue
                    dispatch(name, duration(j, s, t, l))
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, ["Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        w.writeheader()
        w.writerows(rows[::-1])


def run_tool(tool, *flags):
    return subprocess.run([sys.executable, os.path.join(TOOLS, tool + ".py")] + list(flags),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def merged(tool, tmp_path, kernels, plan, **kw):
    """-> (the committed record, the record after --merge_trace of the synthetic trace)."""
    out, trace = str(tmp_path / (tool + ".json")), str(tmp_path / "kernel_trace.csv")
    shutil.copy(os.path.join(REPO, "profiles", tool + ".json"), out)
    before = json.loads(open(out).read())
    assert (before["warmup"], before["repeats"]) == (5, 30)
    write_trace(trace, kernels, plan, 35, **kw)
    r = run_tool(tool, "--merge_trace", trace, "--out", out)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(out).read() and r.stdout.count("\n") == 1
    return before, json.loads(r.stdout)


def without_trace(entry):
    return {k: v for k, v in entry.items() if k != "kernel_trace"}


TIMED = range(5, 35)


def test_the_merge_halves_import_neither_torch_nor_the_package():
    code = ("import sys; sys.path.insert(0, %r); "
            "import components_bench, smooth_bench, simplify_bench, holes_bench, mesh_bench; "
            "assert 'torch' not in sys.modules and 'raynet_amd' not in sys.modules" % TOOLS)
    r = subprocess.run([sys.executable, "-c", code], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr


def test_smooth_bench_merges_the_last_dispatches_of_a_trace(tmp_path):
    kernels = ("k_smooth_ring", "k_smooth_step", "k_vertex_area_normals")
    per_turn = {"k_smooth_ring": 1, "k_smooth_step": 20, "k_vertex_area_normals": 1}
    before, after = merged("smooth_bench", tmp_path, kernels, [per_turn] * 2)
    assert list(after["meshes"]) == ["mrf_128", "fused_256"]
    for s, name in enumerate(after["meshes"]):
        entry, own = after["meshes"][name], after["meshes"][name]["kernel_trace"]
        assert without_trace(entry) == without_trace(before["meshes"][name])
        want = {k: stats([duration(j, s, t, l) for t in TIMED for l in range(per_turn[k])])
                for j, k in enumerate(kernels)}
        for k in kernels:
            assert {x: own[k][x] for x in ("ms_min", "ms_median")} == want[k], (name, k)
        step, ring = want["k_smooth_step"]["ms_median"], want["k_smooth_ring"]["ms_median"]
        assert own["k_smooth_step"]["GB_per_s"] == round(
            entry["bytes_must_move_per_step"] / (step * 1e-3) / 1e9, 1)
        assert own["k_smooth_ring"]["GB_per_s"] == round(
            entry["bytes_must_move_ring"] / (ring * 1e-3) / 1e9, 1)
        assert own["step_to_normals"] == round(step / want["k_vertex_area_normals"]["ms_median"], 3)
        assert own["ring_to_step"] == round(ring / step, 3)
    assert {k: v for k, v in after.items() if k != "meshes"} == \
        {k: v for k, v in before.items() if k != "meshes"}


def test_simplify_bench_merges_the_sums_of_every_turn(tmp_path):
    sys.path.insert(0, TOOLS)
    try:
        from simplify_bench import OWN, scan_launches
    finally:
        sys.path.remove(TOOLS)
    assert scan_launches(256) == (0, 1) and scan_launches(257) == (1, 2)
    assert scan_launches(65536) == (1, 2) and scan_launches(65537) == (2, 3)
    record = json.loads(open(os.path.join(REPO, "profiles", "simplify_bench.json")).read())
    kernels = OWN + ("k_scan_reduce", "k_scan_tile")
    plan, settings = [], []
    for name in ("mrf_128", "fused_256"):
        entry = record["meshes"][name]
        reduce_n, tile_n = (sum(x) for x in zip(scan_launches(entry["nf"]), scan_launches(entry["nv"])))
        assert (reduce_n, tile_n) == (4, 6)                 # three levels for both, at these sizes
        for cell in ("2", "4"):
            per_turn = {k: 1 for k in OWN}
            per_turn.update(k_scan_reduce=reduce_n, k_scan_tile=tile_n)
            plan.append(per_turn)
            settings.append((name, cell))
    before, after = merged("simplify_bench", tmp_path, kernels, plan)
    for s, (name, cell) in enumerate(settings):
        one = after["meshes"][name]["cells"][cell]
        own = one["kernel_trace"]
        assert without_trace(one) == without_trace(before["meshes"][name]["cells"][cell])
        medians = {}
        for j, k in enumerate(kernels):
            p = plan[s][k]
            want = stats([duration(j, s, t, l) for t in TIMED for l in range(p)], launches=p)
            assert {x: own[k][x] for x in ("ms_min", "ms_median")} == want, (name, cell, k)
            assert own[k]["launches"] == p
            medians[k] = own[k]["ms_median"]
        scans = medians["k_scan_reduce"] + medians["k_scan_tile"]
        assert own["scans"]["ms_median"] == round(scans, 4)
        assert own["sum_of_kernels_ms"] == round(sum(medians[k] for k in OWN) + scans, 4)
        for k in OWN:
            assert own[k]["GB_per_s"] == round(
                one["bytes_must_move"][k] / (medians[k] * 1e-3) / 1e9, 1)


def test_holes_bench_merges_the_last_dispatches_of_a_trace(tmp_path):
    kernels = ("k_holes_init", "k_holes_edges", "k_holes_flatten", "k_holes_tally", "k_holes_flags",
               "k_holes_emit")
    settings = [(name, m) for name in ("mrf_128", "fused_256") for m in ("16", "64", "1024")]
    before, after = merged("holes_bench", tmp_path, kernels, [{k: 1 for k in kernels}] * 6)
    for s, (name, m) in enumerate(settings):
        one = after["meshes"][name]["max_edges"][m]
        assert without_trace(one) == without_trace(before["meshes"][name]["max_edges"][m])
        want = {k: stats([duration(j, s, t) for t in TIMED]) for j, k in enumerate(kernels)}
        total = round(sum(want[k]["ms_median"] for k in kernels), 4)
        assert one["kernel_trace"] == dict(want, sum_of_own_kernels_ms=total), (name, m)
    # one dispatch too few of one kernel: nothing is merged
    trace, out = str(tmp_path / "short.csv"), str(tmp_path / "holes_bench.json")
    write_trace(trace, kernels, [{k: 1 for k in kernels}] * 6, 35, earlier=0, extra=-1)
    kept = open(out).read()
    r = run_tool("holes_bench", "--merge_trace", trace, "--out", out)
    assert r.returncode != 0 and open(out).read() == kept
    assert "k_holes_init: 209 dispatches in the trace, expected 210" in r.stderr


def test_components_bench_wants_exactly_its_dispatches(tmp_path):
    kernels = ("k_cc_init", "k_cc_hook", "k_cc_flatten", "k_cc_count")
    plan = [{k: 1 for k in kernels}] * 3
    before, after = merged("components_bench", tmp_path, kernels, plan, earlier=0)
    assert list(after["meshes"]) == ["mrf_128", "fused_256", "strip_2m"]
    for s, name in enumerate(after["meshes"]):
        entry = after["meshes"][name]
        assert without_trace(entry) == without_trace(before["meshes"][name])
        want = {k: stats([duration(j, s, t) for t in TIMED]) for j, k in enumerate(kernels)}
        want["first_start_to_last_end"] = stats(
            [sum(duration(j, s, t) for j in range(4)) + 3 * GAP for t in TIMED])
        assert entry["kernel_trace"] == want, name
    out = str(tmp_path / "components_bench.json")
    kept = open(out).read()
    for extra, found in ((1, 106), (-1, 104)):
        trace = str(tmp_path / ("trace_%d.csv" % found))
        write_trace(trace, kernels, plan, 35, earlier=0, extra=extra)
        r = run_tool("components_bench", "--merge_trace", trace, "--out", out)
        assert r.returncode != 0 and open(out).read() == kept
        assert "k_cc_init: %d dispatches in the trace, expected 105" % found in r.stderr


@pytest.mark.parametrize("tool", ["components_bench", "smooth_bench", "simplify_bench", "holes_bench"])
def test_merge_box_takes_the_last_line_that_opens_a_brace(tmp_path, tool):
    out, box_file = str(tmp_path / (tool + ".json")), str(tmp_path / "bench.txt")
    shutil.copy(os.path.join(REPO, "profiles", tool + ".json"), out)
    before = json.loads(open(out).read())
    box = {"metric": "images_per_s", "value": 12.5, "gpus": 1, "nested": {"steps": 3}}
    with open(box_file, "w") as f:
        f.write("warming up\n" + json.dumps({"value": -1.0}) + "\nstep 3 of 3\n  "
                + json.dumps(box) + "\n\ndone: 3 steps\n")
    r = run_tool(tool, "--merge_box", box_file, "--out", out)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(out).read() and r.stdout.count("\n") == 1
    after = json.loads(r.stdout)
    assert after["box"] == box
    assert {k: v for k, v in after.items() if k != "box"} == \
        {k: v for k, v in before.items() if k != "box"}
