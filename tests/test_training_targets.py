"""raynet_amd/train_network/targets.py against the reference's own dirac_distribution /
gaussian_distribution (tests/golden/ref_training_targets.npz, written by
gen_training_targets_from_reference.py).  CPU."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_training_targets.npz"))


def test_dirac_is_the_references_exactly(golden):
    import torch
    from raynet_amd.train_network.targets import dirac_distribution
    got = dirac_distribution(torch.from_numpy(golden["targets"]), torch.from_numpy(golden["points"]))
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), golden["dirac"])
    assert np.all(golden["dirac"].sum(1) == 1) and len(set(golden["dirac"].argmax(1))) > 8


@pytest.mark.parametrize("std_is_distance", [False, True])
def test_gaussian_is_the_references_to_1e6(golden, std_is_distance):
    import torch
    from raynet_amd.train_network.targets import gaussian_distribution, get_target_distribution_factory
    t, p = torch.from_numpy(golden["targets"]), torch.from_numpy(golden["points"])
    for f in golden["stddev_factors"]:
        want = golden["gaussian_%s_%g" % ("distance" if std_is_distance else "squared", f)]
        got = gaussian_distribution(float(f), std_is_distance)(t, p).numpy()
        assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
        assert np.abs(got.sum(1) - 1).max() < 1e-5
        same = get_target_distribution_factory("guassian", float(f), std_is_distance)(t, p).numpy()
        assert np.array_equal(same, got)
    # the two meanings of the standard deviation are different distributions
    a = golden["gaussian_distance_1"]
    b = golden["gaussian_squared_1"]
    assert np.abs(a - b).max() > 1e-3
