#!/usr/bin/env python3
"""Golden vectors for `sample_in_range` and `sample_in_disparity` from the REFERENCE's own NumPy
sampling schemes (raynet/common/sampling_schemes.py:178-297).

Runs only where the reference is at hand.  What is run, and how, is what
gen_sampling_from_reference.py (next to this file) does: `load_reference()` of that generator
converts raynet/common/camera.py and raynet/utils/{geometry,checks}.py with lib2to3 into a scratch
directory outside this repository and cuts class / method definitions out of the reference files
with `ast` AT RUN TIME.  On top of that this generator cuts `SamplingInRangeScheme`,
`SamplingInDisparityScheme` and `Image.project`; their bodies name `ray_ray_intersection` and
`project` of utils/geometry.py.  No reference text is written anywhere.

What is called: `sample_points_across_ray(scene, 0, y, x)` of both schemes, per ray (the
disparity scheme has no vectorised entry), and `SamplingInRangeScheme._sample_points_across_rays`
on the same rays as `sample_points_across_rays_batched` does (:228-237).

Cameras: the five first cameras of tests/golden/restrepo_mock_scene_1 with that scene's box and
depth_range (3, 7) -- the reference's own test values, tests/test_sampling_schemes.py -- and the
five synthetic ring cameras with box [-1, 1]^3 and range (2, 4).  D in {5, 16, 32, 64}.  At most
250 seeded rays per camera, the four corners and the centre pixel among them.  The far view of
the disparity scheme is the last of the view's neighbour list as `Scene` gives it
(view_indices_with_neighbors(i, 4)).

Output: tests/golden/ref_sampling_schemes_np.npz -- inputs (P, P_pinv, centre, the far view's,
bbox, range, image size, ray indices) and the reference's points, nothing else.
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import gen_sampling_from_reference as base  # noqa: E402


RAYS = 150        # per camera (at most 250; the file stays below 1 MiB)


class _Holder(base._Holder):
    def project(self, point):
        return self._ns["project_image"](self, point)


class _Scene(object):
    def __init__(self, images, bbox):
        self._images, self.bbox = images, bbox

    def get_image(self, i):
        return self._images[0]

    def get_image_with_neighbors(self, i):
        return self._images


class _GP(object):
    def __init__(self, name, D, depth_range):
        self.sampling_type, self.depth_planes, self.depth_range = name, D, depth_range


def main():
    from raynet_amd.common.scene import Scene, parse_scene_info, read_krt
    from raynet_amd.synthetic import ring_cameras
    camera_mod, geometry, ns, scratch = base.load_reference()
    rng = np.random.default_rng(20181018)
    flat = {}
    try:
        import ast
        ns["ray_ray_intersection"] = geometry.ray_ray_intersection
        # `cut` is local to load_reference: the same three lines on the two classes wanted here
        src = open(os.path.join(base.REF, "raynet", "common", "sampling_schemes.py")).read()
        lines = src.split("\n")
        depth0 = [i for i, l in enumerate(lines) if l and not l[0].isspace() and not l.startswith("#")]
        for cls in ("SamplingInRangeScheme", "SamplingInDisparityScheme"):
            start = next(i for i in depth0 if lines[i].startswith("class %s(" % cls))
            end = next((i for i in depth0 if i > start), len(lines))
            exec(compile(ast.parse("\n".join(lines[start:end])),
                         "<raynet/common/sampling_schemes.py>", "exec"), ns)
        src = open(os.path.join(base.REF, "raynet", "common", "image.py")).read()
        lines = src.split("\n")
        depth0 = [i for i, l in enumerate(lines) if l and not l[0].isspace() and not l.startswith("#")]
        start = next(i for i in depth0 if lines[i].startswith("class Image("))
        end = next((i for i in depth0 if i > start), len(lines))
        tree = ast.parse("\n".join(lines[start:end]))
        fn = next(n for n in tree.body[0].body if isinstance(n, ast.FunctionDef) and n.name == "project")
        fn.name = "project_image"          # `project` is utils/geometry.py's in this namespace
        exec(compile(ast.Module(body=[fn], type_ignores=[]), "<raynet/common/image.py>", "exec"), ns)

        groups = []
        rdir = os.path.join(HERE, "restrepo_mock_scene_1")
        bbox = np.asarray(parse_scene_info(os.path.join(rdir, "scene_info.xml")), np.float32).reshape(1, 6)
        files = sorted(os.listdir(os.path.join(rdir, "cams_krt")))[:5]
        groups.append(("restrepo", [read_krt(os.path.join(rdir, "cams_krt", f)) for f in files],
                       bbox, (3.0, 7.0), 72, 128))
        ring_bbox = np.array([[-1, -1, -1, 1, 1, 1]], np.float32)
        groups.append(("ring", [(c.K, c.R, c.t) for c in ring_cameras(5, 480, 640, focal=1.5 * 480)],
                       ring_bbox, (2.0, 4.0), 480, 640))
        Ds = (5, 16, 32, 64)
        for gname, krts, bb, rng_d, H, W in groups:
            cams = [camera_mod.Camera(np.asarray(K, np.float64), np.asarray(R, np.float64),
                                      np.asarray(t, np.float64).reshape(3, 1)) for K, R, t in krts]
            # the neighbour rule of the loaders (common/scene.py, "filesystem")
            order = Scene(images=[None] * len(cams), bbox=bb)
            for k, cam in enumerate(cams):
                name = "%s%d" % (gname, k)
                D = Ds[(k + (gname == "ring")) % len(Ds)]
                views = order.view_indices_with_neighbors(k, 4)
                holders = [_Holder(cams[v], H, W, ns) for v in views]
                scene = _Scene(holders, bb)
                n = min(RAYS, H * W)
                ridx = np.sort(rng.choice(H * W, n, replace=False)).astype(np.int32)
                ridx[:5] = [0, H - 1, (W - 1) * H, W * H - 1, (W // 2) * H + H // 2]
                ridx = np.unique(ridx)
                rs = ns["SamplingInRangeScheme"](_GP("sample_in_range", D, rng_d))
                ds = ns["SamplingInDisparityScheme"](_GP("sample_in_disparity", D, rng_d))
                p_range = np.zeros((len(ridx), D, 3), np.float32)
                p_disp = np.full((len(ridx), D, 3), np.nan, np.float32)
                hit = np.zeros(len(ridx), np.int32)
                for j, r in enumerate(ridx):
                    y, x = int(r % H), int(r // H)
                    p = np.asarray(rs.sample_points_across_ray(scene, 0, y, x))
                    assert p.shape == (D, 4) and np.all(p[:, 3] == 1.0)
                    p_range[j] = p[:, :3]
                    p = ds.sample_points_across_ray(scene, 0, y, x)
                    if p is not None:
                        assert p.shape == (D, 4) and np.all(p[:, 3] == 1.0)
                        p_disp[j] = p[:, :3]
                        hit[j] = 1
                # the vectorised range entry on the same rays (:228-237)
                center, rays = holders[0].rays()
                directions = rays - center
                directions /= np.sqrt(np.sum(directions ** 2, axis=0))
                vec = rs._sample_points_across_rays(center, directions[:, ridx])      # (4, n, D)
                assert np.abs(vec[:3].transpose(1, 2, 0) - p_range).max() < 1e-4
                far = cams[views[-1]]
                flat[name + "/P"] = np.asarray(cam.P, np.float64)
                flat[name + "/P_pinv"] = np.asarray(cam.P_pinv, np.float64)
                flat[name + "/center"] = np.asarray(cam.center, np.float32).ravel()
                flat[name + "/far_P"] = np.asarray(far.P, np.float64)
                flat[name + "/far_P_pinv"] = np.asarray(far.P_pinv, np.float64)
                flat[name + "/far_center"] = np.asarray(far.center, np.float32).ravel()
                flat[name + "/far_view"] = np.array([views[-1]], np.int32)
                flat[name + "/bbox"] = bb.ravel()
                flat[name + "/range"] = np.asarray(rng_d, np.float32)
                flat[name + "/HWD"] = np.array([H, W, D], np.int32)
                flat[name + "/ray_idxs"] = ridx
                flat[name + "/points_range"] = p_range
                flat[name + "/points_disparity"] = p_disp
                flat[name + "/disparity_hit"] = hit
        out = os.path.join(HERE, "ref_sampling_schemes_np.npz")
        np.savez_compressed(out, **flat)
        print("wrote", out, os.path.getsize(out), "bytes;", len(flat) // 14, "cameras")
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
