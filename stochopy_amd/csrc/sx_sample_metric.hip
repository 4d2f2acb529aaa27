// Samplers: the resident chain kernels with per-axis scales learnt in the warm-up (sx_sample_metric; the rule is stated in
// include/stochopy_hip.h and written once in sx_sample.hpp metric_update).  The third form of the kernel templates of
// sx_sample_kernels.hpp, in a translation unit of its own so that it compiles next to the other two, not behind them.
#include "sx_sample_kernels.hpp"

using namespace sx;

extern "C" int sx_sample_metric_bytes(void) { return (int)sizeof(sx_sample_metric); }

extern "C" int sx_sample_run_metric(const sx_sample_args *a, const sx_sample_adapt *ad, const sx_sample_metric *mt, int64_t it0,
                                    int64_t steps, void *stream) {
    return run_chains<true, true>("sx_sample_run_metric", a, ad, mt, it0, steps, stream);
}
