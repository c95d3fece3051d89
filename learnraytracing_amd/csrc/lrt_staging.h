// The layout of a *_host call's device mirrors: plain C++, no HIP, so that it compiles and is
// tested on its own (tests/test_staging_layout.py). A call lists its buffers, then the plan places
// every buffer that is present in one allocation, each at an offset rounded up to 16 B (a 4 B id
// plane may sit between RGBA frames in any order). HostMirrors (lrt_internal.h) does the device
// work on top of it.
#pragma once
#include <cstddef>

namespace lrt {

struct StagingPlan {
    static constexpr int kCapacity = 16;
    static constexpr size_t kAlign = 16;
    // A buffer of the call. host_in: copied to the mirror before the device work; host_out: copied
    // back after it; either may be null. Both null: the buffer is absent, it takes no bytes and has
    // no mirror. Both the same pointer: a buffer updated in place, or an output of which a part
    // survives the call, with one mirror.
    struct Item {
        const void* host_in;
        void* host_out;
        size_t bytes;
        size_t offset;   // of the mirror in the allocation (present items)
    };
    Item item[kCapacity];
    int count = 0;
    size_t bytes = 0;   // the allocation

    // Returns the item's index, or -1 past kCapacity (nothing is added then).
    int add(const void* host_in, void* host_out, size_t size) {
        if (count == kCapacity) return -1;
        const bool here = host_in || host_out;
        item[count] = {host_in, host_out, here ? size : 0, here ? bytes : 0};
        if (here) bytes += (size + kAlign - 1) / kAlign * kAlign;
        return count++;
    }
    bool present(int i) const { return item[i].host_in || item[i].host_out; }
    size_t offset(int i) const { return item[i].offset; }
    size_t total() const { return bytes; }
};

}  // namespace lrt
