// How many bits a radix sort key needs (plain C++: the build and the CPU-tested append plans share it).
#pragma once
#include <stdint.h>

namespace rwr {

inline int bit_length(uint64_t v)
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// ... of keys in [0, top]: at least one bit, the sort takes no zero-bit key
inline int key_bits(uint64_t top)
{
    const int b = bit_length(top);
    return b > 0 ? b : 1;
}

}  // namespace rwr
