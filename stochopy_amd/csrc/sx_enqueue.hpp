// One typed path for every kernel that can go either onto a stream now or into a hipGraph for replay: a generation is
// written once, against an Enqueue, and the sink decides whether that is a launch or a node.
#pragma once
#include <cstdint>

#include "../../include/stochopy_hip.h"
#include "sx_host.hpp"

namespace sx {

template <class T>
struct as_declared {  // (a non-deduced context: the values below convert to the kernel's parameter types, as in a direct call)
    using type = T;
};

// Where a kernel goes: a stream (launched now), or a graph under construction (a node appended behind the last one).
// (Hidden, as GraphBuild below: the instantiations stay out of the library's exported symbols.)
class __attribute__((visibility("hidden"))) Enqueue {
  public:
    explicit Enqueue(hipStream_t s) : stream_(s) {}
    explicit Enqueue(hipGraph_t g) : graph_(g) {}
    // null while a graph is built: what a generation uploads on the way (the wide rows' plans) then stays outside the graph
    hipStream_t stream() const { return stream_; }

    template <class... KA>
    int kernel(void (*fn)(KA...), dim3 grid, dim3 block, size_t lds, typename as_declared<KA>::type... v) {
        void *argv[] = {(void *)&v..., nullptr};
        if (graph_ == nullptr) {
            SX_HIP(hipLaunchKernel((const void *)fn, grid, block, argv, lds, stream_));
            return 0;
        }
        hipKernelNodeParams kp = {};
        kp.func = (void *)fn;
        kp.gridDim = grid;
        kp.blockDim = block;
        kp.sharedMemBytes = (unsigned)lds;
        kp.kernelParams = argv;
        kp.extra = nullptr;
        hipGraphNode_t node;
        SX_HIP(hipGraphAddKernelNode(&node, graph_, last_ ? &last_ : nullptr, last_ ? 1 : 0, &kp));
        last_ = node;
        return 0;
    }

  private:
    hipStream_t stream_ = nullptr;
    hipGraph_t graph_ = nullptr;
    hipGraphNode_t last_ = nullptr;
};

// A graph under construction.  begin(), enqueue into sink(), finish(out); whatever returns before finish() has succeeded
// leaves the graph, its executable and its scratch to the destructor.
class __attribute__((visibility("hidden"))) GraphBuild {
  public:
    GraphBuild() = default;
    GraphBuild(const GraphBuild &) = delete;
    GraphBuild &operator=(const GraphBuild &) = delete;
    ~GraphBuild() { (void)sx_graph_destroy(gr_); }

    int begin() {
        gr_ = new sx_graph();
        SX_HIP(hipGraphCreate(&gr_->graph, 0));
        sink_ = Enqueue(gr_->graph);
        return 0;
    }
    Enqueue &sink() { return sink_; }
    // zeroed device memory that the graph's nodes own (freed with the graph)
    int alloc_scratch(size_t bytes) {
        SX_HIP(hipMalloc(&gr_->scratch, bytes));
        SX_HIP(hipMemset(gr_->scratch, 0, bytes));
        return 0;
    }
    void *scratch() const { return gr_->scratch; }
    int finish(sx_graph **out) {
        SX_HIP(hipGraphInstantiate(&gr_->exec, gr_->graph, nullptr, nullptr, 0));
        *out = gr_;
        gr_ = nullptr;
        return 0;
    }

  private:
    sx_graph *gr_ = nullptr;
    Enqueue sink_{(hipStream_t) nullptr};
};

// best / termination of one generation (sx_core.hip): one kernel, three for rows of more than kMaxDim elements
int enqueue_finalize(Enqueue &q, const double *part_f, const int64_t *part_i, int64_t npart, const double *rows0,
                     const double *rows1, int64_t ld, int n, double *gbest, sx_state *state, int maxiter, double xtol,
                     double ftol);

}  // namespace sx
