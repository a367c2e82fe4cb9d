// wf_layout.h -- workspace layouts as byte offsets (host only, no HIP).  A layout function walks one Bump over the parts of a workspace in their
// order; the size query returns where it ended and the entry point carves the caller's buffer at the offsets it handed out.
#pragma once
#include <cstdint>

namespace wf {

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

struct Bump {
    int64_t at = 0;   // bytes handed out so far: the offset of the next part, the total at the end
    int64_t take(int64_t bytes) {
        const int64_t offset = at;
        at += align256(bytes);
        return offset;
    }
};

}  // namespace wf
