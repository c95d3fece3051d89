// counts_trace_kernel instances for max_depth 9..64 (lrt_render_counts.h): levels beyond the 8 in LDS
// go to the overflow stack.
#include "lrt_render_counts.h"

namespace lrt {

int launch_counts_d64(const KernelArgs& a, const CountsArgs& ca, bool lds, hipStream_t s) {
    return launch_counts_trace<64>(a, ca, lds, s);
}

}  // namespace lrt
