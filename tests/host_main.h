// What the stand-alone host programs of the suite (tests/*_args_main.cpp) share: the counter of
// failed expectations, EXPECT, buffers of exactly the size of their content (so that one element
// past the end is an error under the address sanitizer), and the program's last line, which
// tests/host_program.py looks for.
#pragma once

#include <algorithm>
#include <cstdio>
#include <memory>
#include <vector>

inline int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: expected %s\n", __LINE__, #cond);      \
            failures++;                                                  \
        }                                                                \
    } while (0)

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &from) {
    std::unique_ptr<T[]> p(new T[from.size()]);         // exactly sized: one past is an error
    std::copy(from.begin(), from.end(), p.get());
    return p;
}

// main's return value: "<name>_args: ok" and 0, or the number of failed expectations and 1
inline int finish(const char *name) {
    if (failures) {
        std::printf("%s_args: %d expectation(s) failed\n", name, failures);
        return 1;
    }
    std::printf("%s_args: ok\n", name);
    return 0;
}
