"""The adaptive box scatter's tile-shape policy (raynet_amd/csrc/raynet_box_policy.h) on its own:
host-only integer logic, compiled with g++ behind tests/box_policy_shim.cpp and driven through
ctypes -- no GPU, no HIP.

The expectations are what launch_bp did with the context's eight box_* fields before they became
one type: per launch, look at the host mirror of the cumulative counters {chunks, overflowed
chunks} (observe), launch at the level that gives, then count the probe down and say whether the
counters are copied out behind the launch (launched)."""
import ctypes
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = 12      # launches after a start / reset / step whose counters are copied out
U = ctypes.c_uint


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("box_policy") / "box_policy_shim.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-shared", "-fPIC", "-I", os.path.join(REPO, "raynet_amd", "csrc"),
                           os.path.join(REPO, "tests", "box_policy_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.bp_new.restype = ctypes.c_void_p
    lib.bp_new.argtypes = [ctypes.c_int, ctypes.c_int]
    for name, args in (("bp_free", []), ("bp_reset", []), ("bp_settled", []),
                       ("bp_start", [ctypes.c_int, ctypes.c_int]), ("bp_observe", [U, U]),
                       ("bp_launched", [ctypes.c_int]),
                       ("bp_state", [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(U), ctypes.POINTER(U)])):
        getattr(lib, name).argtypes = [ctypes.c_void_p] + args
    lib.bp_free.restype = lib.bp_reset.restype = lib.bp_start.restype = lib.bp_state.restype = None
    return lib


class Policy:
    def __init__(self, lib, level=0, pin=False):
        self.lib, self.h = lib, lib.bp_new(level, int(pin))

    def __del__(self):
        self.lib.bp_free(self.h)

    def start(self, level, pin=False):
        self.lib.bp_start(self.h, level, int(pin))

    def reset(self):
        self.lib.bp_reset(self.h)

    def observe(self, chunks, overflowed):
        return self.lib.bp_observe(self.h, chunks, overflowed)

    def launched(self, level):
        return bool(self.lib.bp_launched(self.h, level))

    def settled(self):
        return bool(self.lib.bp_settled(self.h))

    def state(self):
        level, c, o = ctypes.c_int(), U(), U()
        self.lib.bp_state(self.h, ctypes.byref(level), ctypes.byref(c), ctypes.byref(o))
        return level.value, c.value, o.value


@pytest.mark.parametrize("chunks,overflowed,level", [
    (100, 2, 0),        # 2 x 50 = 100: not above 2 %
    (100, 3, 1),
    (50, 1, 0),
    (50, 2, 1),
    (1000, 0, 0),
])
def test_level_0_steps_above_two_percent(lib, chunks, overflowed, level):
    b = Policy(lib)
    assert b.observe(chunks, overflowed) == level
    assert b.state() == (level, chunks, overflowed)


@pytest.mark.parametrize("chunks,overflowed,level", [
    (100, 25, 1),       # 25 x 4 = 100: not above 25 %
    (100, 26, 2),
    (100, 3, 1),        # what steps level 0 leaves level 1 alone
    (4, 1, 1),
    (4, 2, 2),
])
def test_level_1_steps_above_a_quarter(lib, chunks, overflowed, level):
    b = Policy(lib, level=1)
    assert b.observe(chunks, overflowed) == level


def test_one_step_per_observation_and_never_past_the_slab_scatter(lib):
    b = Policy(lib)
    assert b.observe(100, 100) == 1         # everything overflowed: still one step
    assert b.observe(200, 200) == 2
    assert b.observe(300, 300) == 2
    assert b.state() == (2, 100, 100)
    b = Policy(lib, level=2)
    assert b.observe(100, 100) == 2


def test_pinned_policy_observes_but_stays(lib):
    b = Policy(lib, level=0, pin=True)
    for k in range(PROBE):
        assert b.observe(100 * (k + 1), 100 * (k + 1)) == 0
        assert b.launched(0)
    assert b.state() == (0, 100, 100)
    assert b.settled()                      # no step, so nothing re-armed the probe
    b = Policy(lib, level=1, pin=True)
    assert b.observe(100, 100) == 1


def test_probe_counts_launches_and_settled_is_its_zero(lib):
    b = Policy(lib)
    for k in range(PROBE):
        assert not b.settled()
        assert b.launched(0)                # counters are copied out behind this launch
    assert b.settled()
    assert not b.launched(0)                # ... and behind none after that
    assert b.settled()
    b.reset()
    assert not b.settled()
    # a launch that went to the slab scatter (no box counters to copy) still counts
    for k in range(PROBE):
        assert not b.settled()
        assert not b.launched(2)
    assert b.settled()


def test_a_step_re_arms_the_probe(lib):
    b = Policy(lib)
    for k in range(PROBE - 1):
        assert b.launched(b.observe(0, 0))
    assert not b.settled()                  # one launch left
    assert b.observe(100, 3) == 1           # the counters of those launches arrive: step
    for k in range(PROBE):
        assert not b.settled()
        assert b.launched(1)
    assert b.settled()
    # an observation that does not step leaves the countdown alone
    b = Policy(lib)
    for k in range(PROBE - 1):
        assert b.launched(0)
    assert b.observe(100, 2) == 0
    assert b.launched(0)
    assert b.settled()


def test_identical_counters_are_nothing_arrived(lib):
    b = Policy(lib)
    assert b.observe(0, 0) == 0             # the mirror as rn_create leaves it
    assert b.state() == (0, 0, 0)
    assert b.observe(100, 1) == 0
    # the chunk count is what says that more launches have arrived
    assert b.observe(100, 90) == 0
    assert b.state() == (0, 100, 1)
    assert b.observe(100, 1) == 0
    assert b.state() == (0, 100, 1)


def test_state_is_the_last_observed_difference(lib):
    b = Policy(lib)
    b.observe(100, 1)
    assert b.state() == (0, 100, 1)
    b.observe(250, 2)
    assert b.state() == (0, 150, 1)
    b.observe(1250, 102)                    # 100 of 1000: steps
    assert b.state() == (1, 1000, 100)
    b.reset()
    assert b.state() == (0, 0, 0)


def test_after_a_reset_with_launches_in_flight_the_first_counters_are_a_baseline(lib):
    b = Policy(lib)
    assert b.launched(b.observe(0, 0))      # a scatter has run; its counters are under way
    assert b.observe(100, 0) == 0
    b.reset()
    assert b.observe(100, 0) == 0           # nothing new yet: still waiting for the baseline
    assert b.observe(300, 200) == 0         # the old scene's launches, all overflowed: no step
    assert b.state() == (0, 0, 0)
    assert b.observe(400, 202) == 0         # from here on differences count: 2 of 100
    assert b.state() == (0, 100, 2)
    assert b.observe(500, 205) == 1         # 3 of 100
    # rn_set_options restarts the same way
    b.start(0)
    assert b.state() == (0, 0, 0)
    assert b.observe(600, 305) == 0
    assert b.state() == (0, 0, 0)
    assert b.observe(700, 405) == 1


def test_a_reset_before_any_launch_expects_no_baseline(lib):
    b = Policy(lib)
    b.reset()
    assert b.observe(100, 3) == 1


def test_reset_returns_to_the_starting_level(lib):
    b = Policy(lib, level=1)
    assert b.observe(100, 100) == 2
    b.reset()
    assert b.state() == (1, 0, 0)
    b.start(0)
    assert b.state() == (0, 0, 0)
    assert b.observe(200, 200) == 1         # (no launch yet: an observation, not a baseline)
