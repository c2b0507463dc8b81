// raynet_box_policy.h -- which tile shape the LDS-box accumulator scatter runs at.  Host-only
// integer logic, nothing of HIP in here: tests/test_box_policy.py compiles it with g++.
//
// Patch-ordered rows start with the LDS-box scatter on 128-ray x 32-step tiles.  The kernel
// counts the chunks whose bounding box did not fit its LDS budget; the count of the previous
// launches is copied out asynchronously (it may lag a launch) and when too many overflowed the
// launcher steps down: more LDS, then narrower chunks, then -- pixel spacing above the voxel
// size, nothing to sum per voxel anyway -- the slab scatter.
// levels: 0 = 128 x 32 tiles with a 4096-voxel box (32 KB), 1 = 256 x 16 tiles with 6144 voxels
// (48 KB; measured best of 4096..8192 on the 256^3 grid of config 4), 2 = slab scatter.
// 0 -> 1 above 2 % overflowed chunks, 1 -> 2 only above 25 % (the box kernel's quarter-chunk
// fallback still beats the slab scatter below that).
#pragma once

struct BoxPolicy {
    static constexpr int LAST = 2;
    // scatter launches after a start / reset whose overflow counters are read back: the tile
    // shape settles within the first launches, and two 8-byte operations behind every scatter
    // are two more dependent items on a stream whose kernels take 70 us each on an eight-rank shard
    static constexpr int PROBE_LAUNCHES = 12;

    int level = 0, level0 = 0;      // in use / the one a start or reset returns to
    bool pin = false;               // stay at the starting level (A/B runs)
    // the device counters {chunks, overflowed chunks} are cumulative over launches: what the
    // launcher had seen of them at its previous look, and the difference = the launches in between
    unsigned seen[2] = {0, 0}, obs[2] = {0, 0};
    int probe = PROBE_LAUNCHES;     // how many more launches copy the counters out
    bool used = false;              // some scatter has run since the context was created
    bool rebase = false;            // the next counters that arrive are a baseline, not an observation

    // rn_create / rn_set_options
    void start(int level_, bool pin_) {
        level0 = level_;
        pin = pin_;
        reset();
    }
    // rn_scatter_reset: launches since the last look at the counters belong to the old scene
    void reset() {
        level = level0;
        obs[0] = obs[1] = 0;
        probe = PROBE_LAUNCHES;
        rebase = used;
    }
    // the counters as the host sees them now -> the level of this launch
    int observe(unsigned c0, unsigned c1) {
        if (c0 != seen[0] && rebase) {
            // last looked at before the reset: what has arrived mixes launches of the previous
            // scene / tile shape in
            seen[0] = c0;
            seen[1] = c1;
            rebase = false;
        } else if (c0 != seen[0]) {   // counters of more launches have arrived
            obs[0] = c0 - seen[0];
            obs[1] = c1 - seen[1];
            seen[0] = c0;
            seen[1] = c1;
            const unsigned per = level < LAST - 1 ? 50u : 4u;
            if (!pin && level < LAST && obs[1] * per > obs[0]) {
                level++;
                probe = PROBE_LAUNCHES;      // look at the new shape as well
            }
        }
        return level;
    }
    // a scatter went out at `launch_level`: does the caller copy the counters out behind it?
    bool launched(int launch_level) {
        used = true;
        if (probe == 0) return false;
        probe--;
        return launch_level < LAST;
    }
    // no launch copies counters out any more: the level stays until the next start / reset
    // (what a captured step relies on)
    bool settled() const { return probe == 0; }
    void state(int *level_, unsigned *chunks, unsigned *overflowed) const {
        *level_ = level;
        *chunks = obs[0];
        *overflowed = obs[1];
    }
};
