#!/usr/bin/env python3
"""What rendering a mesh costs: rn_mesh_render, all outputs with three
colour channels, of the 5 views at 480 x 640 of the synthetic scene, against five launches of
rn_mesh_depthmap over the same BVH -- the same traversal without the attributes --, the two taking
turns, on two meshes.

  mrf_128       the MRF's surface of the synthetic scene after a pass at bench.py's shape (128^3)
  fused_256     the mesh fused from that pass's depth maps at 256 x 256 x 128 (fusion_bench's)

One process on one GPU.  Per call a hipEvent pair on the stream (rn_timer_*), after `--warmup`
calls, min and median over `--repeats`.  Recorded per mesh: the bytes the render writes beyond the
five depth maps and what they cost at the copy rate of DESIGN.md section 5, and whether depth[v] of
the render has the bits of the v-th depth map.  Prints one JSON line and writes it to
profiles/render_bench.json.

The lane mapping is one constant of csrc/raynet_render.inl (RENDER_TILED: a wavefront per 8 x 8
tile; false: 64 pixels of a row).  The other mapping is a library of its own, built from a copy of
the sources with that constant turned over, and timed in a process of its own on the meshes this
one saved (two processes cannot take turns: each has the GPU to itself while it runs):

    python tools/render_bench.py --build_rows OUT.so          # no GPU
    python tools/render_bench.py [--repeats 30] [--warmup 5] [--rows_lib OUT.so]
    python tools/render_bench.py --merge_box FILE             # bench.py's JSON line of the same visit

With --rows_lib the record also says whether both libraries wrote the same bytes.
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_bench as mb  # noqa: E402  (puts the repository on the path)

import numpy as np  # noqa: E402

MESHES = mb.MESHES
CHANNELS = 3
COPY_TBS = 6.29          # the copy rate DESIGN.md section 5 records
TILED = "constexpr bool RENDER_TILED = true;"
ROWS = "constexpr bool RENDER_TILED = false;"


def build_rows(out):
    """The library with the other lane mapping: a copy of the sources, one constant turned over,
    the library's own flags; its rn_version() says so."""
    from raynet_amd import _lib
    with tempfile.TemporaryDirectory() as tmp:
        csrc = os.path.join(tmp, "raynet_amd", "csrc")
        shutil.copytree(_lib.CSRC, csrc, ignore=shutil.ignore_patterns("*.so"))
        shutil.copytree(os.path.dirname(_lib.HEADER), os.path.join(tmp, "include"))
        path = os.path.join(csrc, "raynet_render.inl")
        text = open(path).read()
        if text.count(TILED) != 1:
            raise SystemExit("raynet_render.inl: expected one `%s`" % TILED)
        with open(path, "w") as f:
            f.write(text.replace(TILED, ROWS))
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, '-DRN_BUILD_EXTRA="render_rows"'] + _lib.HIPCC_FLAGS +
                              ["raynet_hip.hip", "-o", os.path.abspath(out)], cwd=csrc)
    print(out)


def camera_rows():
    """The (V, 15) camera rows of the synthetic scene bench_meshes() renders."""
    from raynet_amd.render import camera_rows as rows_of
    from raynet_amd.synthetic import make_synthetic_scene
    scene, _ = make_synthetic_scene(H=mb.H, W=mb.W, n_views=mb.V, focal=1.5 * mb.H, seed=1234)
    return rows_of([scene.get_image(i).camera for i in range(mb.V)])


def attributes(nv, seed):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(nv, 3))
    return (rng.random((nv, CHANNELS)).astype(np.float32),
            (n / np.linalg.norm(n, axis=1)[:, None]).astype(np.float32))


class Job(object):
    """One mesh on the device with its BVH, its attributes and the outputs of both entries."""

    def __init__(self, vertices, faces, rows, colors, normals):
        import torch
        from raynet_amd.mesh import MeshRaycaster

        def dev(a):
            return a.cuda() if isinstance(a, torch.Tensor) else torch.from_numpy(a).cuda()
        self.vertices, self.faces, self.rows = dev(vertices), dev(faces), dev(rows)
        self.colors, self.normals = dev(colors), dev(normals)
        self.caster = MeshRaycaster(self.vertices[self.faces.long()].reshape(-1, 9))
        self.ctx = self.caster._ctx
        self.maps = torch.empty((mb.V, mb.H, mb.W), dtype=torch.float32, device="cuda")
        self.P = [self.rows[v, :12].contiguous() for v in range(mb.V)]
        self.c = [self.rows[v, 12:].contiguous() for v in range(mb.V)]
        self.out = None

    def render(self):
        self.out = self.ctx.mesh_render(self.caster.nodes, self.caster.leaves, self.vertices,
                                        self.faces, self.rows, mb.H, mb.W, self.colors, self.normals)

    def depth_maps(self):
        for v in range(mb.V):
            self.ctx.mesh_depthmap(mb.H, mb.W, self.P[v], self.c[v], self.caster.nodes,
                                   self.caster.leaves, self.maps[v])

    def digest(self):
        import torch
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in self.out:
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()


def rows_child(args):
    """The process of the other library (RAYNET_HIP_LIB names it): the render alone, on the meshes
    the parent saved."""
    from raynet_amd import _lib
    res = {"version": _lib.load().rn_version().decode(), "meshes": {}}
    for name in MESHES:
        z = np.load(os.path.join(args.rows_child, name + ".npz"))
        job = Job(z["vertices"], z["faces"], z["rows"], z["colors"], z["normals"])
        ms = mb.take_turns(job.ctx, {"render": job.render}, args.warmup, args.repeats)
        res["meshes"][name] = dict(render=mb.stats(ms["render"]), sha256=job.digest())
    with open(os.path.join(args.rows_child, "rows.json"), "w") as f:
        json.dump(res, f)


def measure(args):
    import torch
    from raynet_amd import _lib
    _lib.build()
    found = mb.bench_meshes()
    rows = camera_rows()
    res = {"tool": "render_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "views": mb.V, "H": mb.H, "W": mb.W, "channels": CHANNELS,
           "lane_mapping": "8 x 8 tiles", "copy_rate_TBs": COPY_TBS, "meshes": {}}
    pixels = mb.V * mb.H * mb.W
    extra_bytes = pixels * (4 + 8 + 4 * CHANNELS + 12)          # face, bary, colour, normal
    with tempfile.TemporaryDirectory() as tmp:
        digests = {}
        for k, name in enumerate(MESHES):
            vertices, faces, _ = found[name]
            colors, normals = attributes(len(vertices), k)
            job = Job(vertices, faces, rows, colors, normals)
            ms = mb.take_turns(job.ctx, {"render": job.render, "depth_x5": job.depth_maps},
                               args.warmup, args.repeats)
            one = {"nv": len(vertices), "nf": len(faces), "bvh_depth": job.caster.depth,
                   "render": mb.stats(ms["render"]), "depth_x5": mb.stats(ms["depth_x5"])}
            one["render"]["ratio_to_depth_x5"] = round(
                one["render"]["ms_median"] / one["depth_x5"]["ms_median"], 3)
            one["extra_bytes"] = extra_bytes
            one["extra_bytes_ms_at_copy_rate"] = round(extra_bytes / (COPY_TBS * 1e12) * 1e3, 4)
            one["covered"] = round(float((job.out[0] >= 0).float().mean()), 4)
            one["depth_has_the_depth_maps_bits"] = bool(
                torch.equal(job.out[1].view(torch.int32), job.maps.view(torch.int32)))
            digests[name] = job.digest()
            res["meshes"][name] = one
            if args.rows_lib:
                np.savez(os.path.join(tmp, name + ".npz"), vertices=vertices.cpu().numpy(),
                         faces=faces.cpu().numpy(), rows=rows, colors=colors, normals=normals)
            del job
        if args.rows_lib:
            env = dict(os.environ, RAYNET_HIP_LIB=os.path.abspath(args.rows_lib))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--rows_child", tmp,
                                   "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                                  env=env)
            child = json.load(open(os.path.join(tmp, "rows.json")))
            res["rows_version"] = child["version"]
            for name in MESHES:
                one, other = res["meshes"][name], child["meshes"][name]
                one["render_rows"] = other["render"]
                one["render_rows"]["ratio_to_tiles"] = round(
                    other["render"]["ms_median"] / one["render"]["ms_median"], 3)
                one["both_mappings_wrote_the_same_bytes"] = other["sha256"] == digests[name]
    mb.write_record(res, args.out)


def merge_trace(args):
    raise SystemExit("render_bench: one kernel per call, the event pair brackets it; no trace to merge")


if __name__ == "__main__":
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument("--build_rows", default=None)
    own.add_argument("--rows_lib", default=None)
    own.add_argument("--rows_child", default=None)
    mine, rest = own.parse_known_args()
    if mine.build_rows:
        build_rows(mine.build_rows)
    elif mine.rows_child:
        timing = argparse.ArgumentParser()
        timing.add_argument("--repeats", type=int, default=30)
        timing.add_argument("--warmup", type=int, default=5)
        child = timing.parse_args(rest)
        child.rows_child = mine.rows_child
        rows_child(child)
    else:
        sys.argv = sys.argv[:1] + rest

        def with_rows(args):
            args.rows_lib = mine.rows_lib
            measure(args)
        mb.main("render_bench", with_rows, merge_trace)
