// raynet_scan_args.h -- the size arithmetic of the library's grid-level exclusive scan of 64-bit
// words (raynet_scan.inl), host-only and free of HIP: the users of the scan lay their workspaces
// out with it (raynet_isosurface_args.h, raynet_simplify_args.h), and tests/isosurface_args_main.cpp
// checks it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstdint>

namespace rn_scan {

constexpr int SCAN_TILE = 256;          // entries one workgroup of the scan takes: one per thread

// Level 0 is the data; level k + 1 holds one sum per SCAN_TILE entries of level k, down to a
// level of at most SCAN_TILE entries that one workgroup scans on its own.
constexpr int64_t scan_tiles(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
// 64-bit words of scratch below the data: every level above level 0
constexpr int64_t scan_scratch_words(int64_t n) {
    int64_t words = 0;
    while (n > SCAN_TILE) {
        n = scan_tiles(n);
        words += n;
    }
    return words;
}
constexpr int scan_levels(int64_t n) {
    int levels = 1;
    while (n > SCAN_TILE) {
        n = scan_tiles(n);
        levels++;
    }
    return levels;
}

}  // namespace rn_scan
