"""tests/mesh_harness.py itself (no GPU): the scene directory comes back from the scene loader as it
was written, the three variants of the two-sphere maps are one scene, the guard assertions see a
write one element behind the used rows and one byte into the workspace's tail, and the bit
comparison tells -0.0 from 0.0 and, if asked, takes one NaN for another."""
import numpy as np
import pytest

import mesh_harness as h

F = np.float32


def _printed(a):
    """What a reader of the text gets: the float32 of each number's %.9g."""
    return np.array([float("%.9g" % x) for x in np.asarray(a, np.float64).ravel()], F)


def test_a_written_scene_comes_back_from_the_loader(tmp_path):
    from raynet_amd.common.scene import get_scene
    bbox, cams, H, W, _, _, _, gt_maps = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED)
    bbox = bbox + np.array([0.1, 0, 0, 0, 1 / 3, 0], F)         # not only whole numbers
    path = str(tmp_path / "scene")
    h.write_restrepo_scene(path, bbox, cams, H, W, gt_maps)
    scene = get_scene("restrepo", path)
    assert scene.n_images == 3
    assert np.array_equal(np.asarray(scene.bbox).ravel(), _printed(bbox))
    for i, (cam, depth) in enumerate(zip(cams, gt_maps)):
        image = scene.get_image(i)
        assert image.image.shape == (H, W, 3)
        for name in ("K", "R", "t"):
            got = np.asarray(getattr(image.camera, name))
            assert got.dtype == F and np.array_equal(got.ravel(), _printed(getattr(cam, name))), name
        back = scene.get_depth_map(i)
        assert back.dtype == F and np.array_equal(h.bits(back), h.bits(depth))


def test_the_three_variants_of_the_two_sphere_maps_are_one_scene():
    plain = h.two_sphere_maps()
    noisy = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED)
    blanked = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED, blank=h.PATCH)
    for other in (noisy, blanked):
        assert np.array_equal(other[0], plain[0]) and other[2:7] == plain[2:7]
        for a, b in zip(other[1], plain[1]):
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("K", "R", "t"))
    assert plain[2:5] == (20, 30, (18, 22, 14)) and len(plain[7]) == 3
    outside = np.ones((20, 30), bool)
    outside[h.PATCH] = False
    for p, n, b in zip(plain[7], noisy[7], blanked[7]):
        assert p.dtype == n.dtype == b.dtype == F and p.shape == n.shape == b.shape == (20, 30)
        assert (p >= 0).all() and 0 < (p > 0).sum() < p.size
        assert np.array_equal(p == 0, n == 0)
        assert not np.array_equal(p, n) and np.abs(n - p).max() < 6 * h.NOISE_SIGMA
        assert (n[h.PATCH] > 0).all() and (b[h.PATCH] == 0).all()
        assert np.array_equal(h.bits(b[outside]), h.bits(n[outside]))
    # the same seed gives the same maps, another one other noise on the same pixels
    again = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED)[7]
    other = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED + 1)[7]
    for n, a, o in zip(noisy[7], again, other):
        assert np.array_equal(h.bits(n), h.bits(a)) and not np.array_equal(n, o)
        assert np.array_equal(n == 0, o == 0)


@pytest.mark.parametrize("fill,dtype", [(-7.5, "float32"), (-77, "int32"), (-7, "int32"),
                                        (-77, "int64"), (-7.0, "float32")])
def test_the_guard_rows_see_one_element_written_behind_the_used_part(fill, dtype):
    import torch
    out = h.padded((4, 3), fill, getattr(torch, dtype), device="cpu")
    assert tuple(out.shape) == (4 + h.PAD, 3) and (out == fill).all()
    out[:4] = 1                                         # the used rows may hold anything
    h.assert_untouched(out, 4, fill, "untouched")
    h.assert_untouched(out.numpy(), 4, fill, "untouched, as an array")
    out[4, 0] = 1                                       # one element behind them
    with pytest.raises(AssertionError, match="written behind row 4"):
        h.assert_untouched(out, 4, fill, "planted")
    flat = h.padded(0, fill, getattr(torch, dtype), pad=2, device="cpu")
    h.assert_untouched(flat, 0, fill)
    flat[-1] = 0
    with pytest.raises(AssertionError):
        h.assert_untouched(flat, 0, fill)


def test_the_pad_is_compared_by_bits():
    import torch
    out = h.padded(3, 0.0, torch.float32, device="cpu")
    h.assert_untouched(out, 3, 0.0)
    out[3] = -0.0                                       # equal by value
    with pytest.raises(AssertionError):
        h.assert_untouched(out, 3, 0.0)


def test_the_workspace_tail_sees_one_byte():
    work = h.workspace(24, device="cpu")
    assert work.numel() == 24 + h.TAIL and (work == 0xA5).all()
    work[:24] = 0
    h.assert_untouched(work, 24, h.TAIL_BYTE)
    work[24] = 0xA4                                     # one byte into the tail
    with pytest.raises(AssertionError, match="written behind row 24"):
        h.assert_untouched(work, 24, h.TAIL_BYTE)


def test_an_input_keeps_its_bits_or_the_assertion_fails():
    import torch
    uploaded = np.array([[0.0, -0.0, 1.5], [np.nan, np.inf, -2.0]], F)
    tensor = torch.from_numpy(uploaded.copy())
    h.assert_input_kept(tensor, uploaded)
    tensor[0, 0] = -0.0                                 # equal by value, other bits
    with pytest.raises(AssertionError, match="an input was written"):
        h.assert_input_kept(tensor, uploaded)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int64)
    tensor = torch.from_numpy(faces.astype(np.int32))
    h.assert_input_kept(tensor, faces)
    tensor[1, 2] = 4
    with pytest.raises(AssertionError):
        h.assert_input_kept(tensor, faces)


def test_the_bit_comparison_tells_minus_zero_from_zero_and_names_the_rows():
    want = np.arange(30, dtype=F).reshape(10, 3)
    want[2, 1] = 0.0
    got = want.copy()
    h.assert_same_bits(got, want, "equal")
    h.assert_same_bits(got[:0], want[:0], "empty")
    got[2, 1] = -0.0
    got[7, 0] += 1
    assert np.array_equal(got[2], want[2])              # by value the row is the same
    with pytest.raises(AssertionError) as e:
        h.assert_same_bits(got, want, "two rows")
    what, count, rows, first_got, first_want = e.value.args[0]
    assert (what, count, rows.tolist()) == ("two rows", 2, [2, 7])
    assert np.array_equal(first_got, got[[2, 7]]) and np.array_equal(first_want, want[[2, 7]])
    with pytest.raises(AssertionError):
        h.assert_same_bits(got[:5], want, "another shape")


def test_the_nan_option_takes_any_nan_for_a_nan_and_nothing_else():
    quiet = np.array([0x7fc00000, 0xffc00001, 0x7f800001], np.uint32).view(F)   # three payloads
    assert np.isnan(quiet).all()
    want = np.array([[1.0, quiet[0], 2.0], [quiet[0], 3.0, -0.0]], F)
    got = np.array([[1.0, quiet[1], 2.0], [quiet[2], 3.0, -0.0]], F)
    h.assert_same_bits(got, want, "payloads", nan_payloads=True)
    with pytest.raises(AssertionError):
        h.assert_same_bits(got, want, "payloads count without the option")
    for row, col, value in ((0, 1, 5.0), (0, 0, quiet[0]), (1, 2, 0.0)):
        bad = got.copy()
        bad[row, col] = value                           # a number for a NaN, a NaN for a number, 0.0
        with pytest.raises(AssertionError):
            h.assert_same_bits(bad, want, "not the truth", nan_payloads=True)
