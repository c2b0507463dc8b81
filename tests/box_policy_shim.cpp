// C face of raynet_amd/csrc/raynet_box_policy.h for tests/test_box_policy.py (g++, no HIP).
#include "raynet_box_policy.h"

extern "C" {
BoxPolicy *bp_new(int level, int pin) {
    BoxPolicy *b = new BoxPolicy();
    b->start(level, pin != 0);
    return b;
}
void bp_free(BoxPolicy *b) { delete b; }
void bp_start(BoxPolicy *b, int level, int pin) { b->start(level, pin != 0); }
void bp_reset(BoxPolicy *b) { b->reset(); }
int bp_observe(BoxPolicy *b, unsigned chunks, unsigned overflowed) { return b->observe(chunks, overflowed); }
int bp_launched(BoxPolicy *b, int level) { return b->launched(level) ? 1 : 0; }
int bp_settled(const BoxPolicy *b) { return b->settled() ? 1 : 0; }
void bp_state(const BoxPolicy *b, int *level, unsigned *chunks, unsigned *overflowed) {
    b->state(level, chunks, overflowed);
}
}
