// device_cub.hpp -- hipcub's two-phase calls, each written once: a callable run(void* temp, size_t& bytes) that
// is the hipcub function bound to its arguments serves the size query (temp == nullptr) and the run.  The
// query comes before the scratch block exists, so the callable captures its pointer variables by reference
// (a size query touches no memory).  CubTemp is the temporary storage several calls may share: size() keeps
// the largest need plus 16 bytes of padding, lay_out() makes it a piece of the layout, run() runs a call in it.
#pragma once

#include <algorithm>

#include "mqr_common.hpp"
#include "scratch_layout.hpp"

namespace mqr {

struct CubTemp {
    void* p = nullptr;
    size_t bytes = 0;
    template <class Run>
    hipError_t size(Run&& call) {
        size_t b = 0;
        const hipError_t e = call(nullptr, b);
        bytes = std::max(bytes, b + 16);
        return e;
    }
    // size() of every call sharing the temporary, which then becomes a piece of L; the first error
    template <class... Run>
    hipError_t lay_out(ScratchLayout& L, Run&&... call) {
        hipError_t e = hipSuccess;
        ((e = e == hipSuccess ? size(call) : e), ...);
        L.add_bytes(p, bytes);
        return e;
    }
    template <class Run>
    hipError_t run(Run&& call) const {
        size_t b = bytes - 16;  // what the size queries asked for
        return call(p, b);
    }
};

}  // namespace mqr
