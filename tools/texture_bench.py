#!/usr/bin/env python3
"""What a texture atlas costs: rn_texture_bake of the 5 views at 480 x 640
of the synthetic scene, three channels, with the mesh's own depth maps as the occluder, on two
meshes of bench.py's pass,

  mrf_128_simplified   the MRF's surface at 128^3 after vertex clustering at two voxel sides, T = 16
  mrf_128              that surface as it is, T = 4

against rn_project_colors over as many points as the atlas has owned texels (the vertices, taken
round and round, with their normals): the same per-view step without the atlas arithmetic, in ns
per texel-view; and rn_texture_sample of the 5 rendered views against the rn_mesh_render that
made its planes.  The entries take turns.

One process on one GPU.  Per call a hipEvent pair on the stream (rn_timer_*), after `--warmup`
calls, min and median over `--repeats`.  Prints one JSON line and writes it to
profiles/texture_bench.json.  No time is asserted anywhere.

The lane mapping of the bake is one constant of csrc/raynet_texture.inl (TEXTURE_TILED: a wavefront
per 8 x 8 tile of texels; false: 64 texels of a row).  The other mapping is a library of its own,
built from a copy of the sources with that constant turned over, and timed in a process of its own
on the inputs this one saved (two processes cannot take turns: each has the GPU to itself while it
runs):

    python tools/texture_bench.py --build_rows OUT.so          # no GPU
    python tools/texture_bench.py [--repeats 30] [--warmup 5] [--rows_lib OUT.so]
    python tools/texture_bench.py --merge_box FILE             # bench.py's JSON line of the same visit

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

JOBS = (("mrf_128_simplified", 16), ("mrf_128", 4))
CHANNELS = 3
TILED = "constexpr bool TEXTURE_TILED = true;"
ROWS = "constexpr bool TEXTURE_TILED = false;"


def build_rows(out):
    """The library with the other lane mapping: a copy of the sources, one constant turned over,
    the library's own flags; its rn_version() says so."""
    from raynet_amd import _lib
    with tempfile.TemporaryDirectory() as tmp:
        csrc = os.path.join(tmp, "raynet_amd", "csrc")
        shutil.copytree(_lib.CSRC, csrc, ignore=shutil.ignore_patterns("*.so"))
        shutil.copytree(os.path.dirname(_lib.HEADER), os.path.join(tmp, "include"))
        path = os.path.join(csrc, "raynet_texture.inl")
        text = open(path).read()
        if text.count(TILED) != 1:
            raise SystemExit("raynet_texture.inl: expected one `%s`" % TILED)
        with open(path, "w") as f:
            f.write(text.replace(TILED, ROWS))
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, '-DRN_BUILD_EXTRA="texture_rows"'] + _lib.HIPCC_FLAGS +
                              ["raynet_hip.hip", "-o", os.path.abspath(out)], cwd=csrc)
    print(out)


def scene_views():
    """-> (cameras, images [V, H, W, 3] f32) of the synthetic scene bench_meshes() reconstructs.  The
    scene carries feature maps, not photographs: the images are smooth waves over the pixels, which
    cost what any image costs to fetch."""
    from raynet_amd.synthetic import make_synthetic_scene
    scene, _ = make_synthetic_scene(H=mb.H, W=mb.W, n_views=mb.V, focal=1.5 * mb.H, seed=1234)
    v, y, x, c = np.meshgrid(np.arange(mb.V), np.arange(mb.H), np.arange(mb.W), np.arange(CHANNELS),
                             indexing="ij")
    images = 0.5 + 0.5 * np.sin(0.05 * (c + 1) * x + 0.03 * y + v)
    return [scene.get_image(i).camera for i in range(mb.V)], images.astype(np.float32)


class Job(object):
    """One mesh on the device with its BVH, the views, the atlas and the outputs of the entries."""

    def __init__(self, vertices, faces, T, rows32, rows64, images, tol):
        import torch
        from raynet_amd import texture
        from raynet_amd.mesh import MeshRaycaster

        def dev(a):
            return a.cuda() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.vertices, self.faces = dev(vertices).float().contiguous(), dev(faces).int().contiguous()
        self.rows32, self.rows64, self.images = dev(rows32), dev(rows64), dev(images)
        self.tol = float(tol)
        self.caster = MeshRaycaster(self.vertices[self.faces.long()].reshape(-1, 9))
        self.ctx = self.caster._ctx
        self.layout = L = texture.atlas_layout(len(self.faces), T)
        self.owned = int(texture.owned_texels(L).sum())
        self.texture = torch.empty((L.Ht, L.Wt, CHANNELS), dtype=torch.float32, device="cuda")
        self.weight = torch.empty((L.Ht, L.Wt), dtype=torch.float32, device="cuda")
        self.views = torch.empty((L.Ht, L.Wt), dtype=torch.int32, device="cuda")
        self.planes = None
        self.render()
        self.depths = self.planes[1]
        # as many points as owned texels: the vertices round and round, with their area normals
        # (the bake tests every texel against its face's normal)
        from raynet_amd.appearance import corner_table
        at = torch.arange(self.owned, device="cuda") % len(self.vertices)
        self.points = self.vertices[at].contiguous()
        normals = self.ctx.vertex_area_normals(self.vertices, self.faces,
                                               *corner_table(self.faces, len(self.vertices)))
        self.normals = normals[at].contiguous()
        self.p_colors = torch.empty((self.owned, CHANNELS), dtype=torch.float32, device="cuda")
        self.p_weight = torch.empty((self.owned,), dtype=torch.float32, device="cuda")
        self.p_views = torch.empty((self.owned,), dtype=torch.int32, device="cuda")
        self.sampled = torch.empty(tuple(self.planes[0].shape) + (CHANNELS,), dtype=torch.float32,
                                   device="cuda")

    def render(self):
        self.planes = self.ctx.mesh_render(self.caster.nodes, self.caster.leaves, self.vertices,
                                           self.faces, self.rows32, mb.H, mb.W)

    def bake(self):
        L = self.layout
        self.ctx.texture_bake(self.vertices, self.faces, None, L.T, L.cells_per_row, self.rows64,
                              self.images, self.depths, self.tol, 0.0, 0.0, 0, self.texture,
                              self.weight, self.views)

    def project(self):
        self.ctx.project_colors(self.points, self.normals, self.rows64, self.images, self.depths,
                                self.tol, 0.0, 0.0, 0, self.p_colors, self.p_weight, self.p_views)

    def sample(self):
        L = self.layout
        self.ctx.texture_sample(self.planes[0], self.planes[2], L.n_faces, L.T, L.cells_per_row,
                                self.texture, True, self.sampled)

    def digest(self):
        import torch
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (self.texture, self.weight, self.views):
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()


def rows_child(args):
    """The process of the other library (RAYNET_HIP_LIB names it): the bake alone, on the inputs
    the parent saved."""
    from raynet_amd import _lib
    res = {"version": _lib.load().rn_version().decode(), "meshes": {}}
    for name, T in JOBS:
        z = np.load(os.path.join(args.rows_child, name + ".npz"))
        job = Job(z["vertices"], z["faces"], T, z["rows32"], z["rows64"], z["images"], float(z["tol"]))
        ms = mb.take_turns(job.ctx, {"bake": job.bake}, args.warmup, args.repeats)
        res["meshes"][name] = dict(bake=mb.stats(ms["bake"]), sha256=job.digest())
        del job
    with open(os.path.join(args.rows_child, "rows.json"), "w") as f:
        json.dump(res, f)


def measure(args):
    import torch
    from raynet_amd import _lib
    from raynet_amd.appearance import pack_cameras
    from raynet_amd.render import camera_rows
    from raynet_amd.volume import SurfaceMesh
    _lib.build()
    vertices, faces, voxel = mb.bench_meshes()["mrf_128"]
    cameras, images = scene_views()
    rows32, rows64 = camera_rows(cameras), pack_cameras(cameras)
    tol = float(np.sqrt((np.asarray(voxel, np.float64) ** 2).sum()))
    small = SurfaceMesh(vertices.cpu().numpy(), faces.cpu().numpy()).simplified(2.0 * np.asarray(voxel))
    meshes = {"mrf_128_simplified": (small.vertices, small.faces),
              "mrf_128": (vertices.cpu().numpy(), faces.cpu().numpy())}
    res = {"tool": "texture_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "views": mb.V, "H": mb.H, "W": mb.W, "channels": CHANNELS,
           "lane_mapping": "8 x 8 tiles", "occlusion_tolerance": round(tol, 6), "meshes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        digests = {}
        for name, T in JOBS:
            v, f = meshes[name]
            job = Job(v, f, T, rows32, rows64, images, tol)
            launches = {"bake": job.bake, "project_colors": job.project, "render": job.render,
                        "sample": job.sample}
            if args.trace:
                launches = {"bake": job.bake, "sample": job.sample}
            ms = mb.take_turns(job.ctx, launches, args.warmup, args.repeats)
            if args.trace:
                del job
                continue
            L = job.layout
            texels = L.Wt * L.Ht
            one = {"nv": len(v), "nf": len(f), "T": T, "atlas": [L.Wt, L.Ht], "texels": texels,
                   "owned_texels": job.owned}
            for k in launches:
                one[k] = mb.stats(ms[k])
            one["bake"]["ns_per_owned_texel_view"] = round(
                one["bake"]["ms_median"] * 1e6 / (job.owned * mb.V), 6)
            one["project_colors"]["ns_per_point_view"] = round(
                one["project_colors"]["ms_median"] * 1e6 / (job.owned * mb.V), 6)
            one["bake"]["ratio_to_project_colors"] = round(
                one["bake"]["ms_median"] / one["project_colors"]["ms_median"], 3)
            one["sample"]["ratio_to_render"] = round(
                one["sample"]["ms_median"] / one["render"]["ms_median"], 3)
            seen = job.views != 0
            one["seen_of_owned"] = round(float(seen.sum()) / job.owned, 4)
            one["covered"] = round(float((job.planes[0] >= 0).float().mean()), 4)
            digests[name] = job.digest()
            res["meshes"][name] = one
            if args.rows_lib:
                np.savez(os.path.join(tmp, name + ".npz"), vertices=v, faces=f, rows32=rows32,
                         rows64=rows64, images=images, tol=tol)
            del job
            torch.cuda.empty_cache()
        if args.trace:
            return
        if args.rows_lib:
            env = dict(os.environ, RAYNET_HIP_LIB=os.path.abspath(args.rows_lib))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--rows_child", tmp,
                                   "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                                  env=env)
            child = json.load(open(os.path.join(tmp, "rows.json")))
            res["rows_version"] = child["version"]
            for name, _ in JOBS:
                one, other = res["meshes"][name], child["meshes"][name]
                one["bake_rows"] = other["bake"]
                one["bake_rows"]["ratio_to_tiles"] = round(
                    other["bake"]["ms_median"] / one["bake"]["ms_median"], 3)
                one["both_mappings_wrote_the_same_bytes"] = other["sha256"] == digests[name]
    mb.write_record(res, args.out)


def merge_trace(args):
    """The kernels' own times of a rocprofv3 kernel trace of --trace, under "kernel_trace"."""
    res = json.loads(open(args.out).read())
    names = ("k_texture_bake", "k_texture_sample")
    rows = mb.keep_last(mb.trace_rows(args.merge_trace, names),
                        {k: len(JOBS) * (args.warmup + args.repeats) for k in names})
    per = args.warmup + args.repeats
    res["kernel_trace"] = {}
    for j, (name, _) in enumerate(JOBS):
        res["kernel_trace"][name] = {
            k: mb.stats([(e - s) / 1e6 for s, e in rows[k][j * per + args.warmup:(j + 1) * per]])
            for k in names}
    mb.write_record(res, args.out)


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
        mb.main("texture_bench", with_rows, merge_trace)
