// counts_trace_kernel instances for max_depth <= 8 (lrt_render_counts.h): the 8 recursion levels live in LDS.
#include "lrt_render_counts.h"

namespace lrt {

int launch_counts_d8(const KernelArgs& a, const CountsArgs& ca, bool lds, hipStream_t s) {
    return launch_counts_trace<8>(a, ca, lds, s);
}

}  // namespace lrt
