"""Target distributions of the pre-training stage over a ray's D sample points
(raynet/utils/training_utils.py:71-141), batched over rays in torch.

target [n, 4] (or [n, 3]): the ground-truth point of every ray; points [n, D, 4]: its sample
points.  Returns [n, D] float32.  The factories have the reference's names and arguments; the
training scripts put one on `GenerationParameters.target_distribution_factory`.
"""
import torch


def _squared_distances(target, points):
    return ((target[:, None, :3] - points[:, :, :3]) ** 2).sum(-1)


def dirac_distribution(target, points):
    """All mass on the sample point closest to the target (the first of equals, as argmin)."""
    d = _squared_distances(target, points)
    out = torch.zeros_like(d)
    out[torch.arange(d.shape[0], device=d.device), d.argmin(1)] = 1.0
    return out


def get_std(stddev_factor, points, std_is_distance):
    """[n]: stddev_factor * |near - far| / D, or with the SQUARED distance when
    std_is_distance is off (training_utils.py:95-105)."""
    sq = ((points[:, 0, :3] - points[:, -1, :3]) ** 2).sum(-1)
    span = torch.sqrt(sq) if std_is_distance else sq
    return stddev_factor * span / points.shape[1]


def gaussian_distribution(stddev_factor, std_is_distance):
    def inner(target, points):
        std = get_std(stddev_factor, points, std_is_distance)
        d = _squared_distances(target, points)
        g = torch.exp(-d / (2 * std ** 2)[:, None])
        total = g.sum(1, keepdim=True)
        if bool((total == 0).any()):
            raise ValueError("gaussian_distribution: a ray's distribution is all zero (std %g)"
                             % float(std[(total == 0).squeeze(1)][0]))
        return g / total
    return inner


def get_target_distribution_factory(name, stddev_factor=1.0, std_is_distance=False):
    """--target_distribution_factory: "dirac" or "guassian" (the reference's spelling; "gaussian"
    is taken too)."""
    if name == "dirac":
        return dirac_distribution
    if name in ("guassian", "gaussian"):
        return gaussian_distribution(stddev_factor, std_is_distance)
    raise ValueError("unknown target distribution %r" % (name,))
