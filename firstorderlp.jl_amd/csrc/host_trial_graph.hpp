// host_trial_graph.hpp -- part of the single translation unit pdhg_hip.hip (included there, at the place its text used to stand).
// the trial step as a HIP graph: the helpers that add a kernel node / give one new parameters, and the pinned result words
// (host side).  Which nodes a fused product has is not decided here: host_product.hpp states its steps, the sinks in
// host_trial_graph_build.hpp call these helpers.

// ---- the trial step as a HIP graph ---------------------------------------------------

// a kernel node's description; `params` points at the arguments, which outlive the call that consumes it
inline hipKernelNodeParams kernel_node_params(const void *func, dim3 grid, dim3 block, size_t lds, void **params) {
  hipKernelNodeParams p{};
  p.func = const_cast<void *>(func);
  p.gridDim = grid; p.blockDim = block; p.sharedMemBytes = (unsigned)lds;
  p.kernelParams = params; p.extra = nullptr;
  return p;
}
template <typename... Args>
hipError_t graph_add_kernel(hipGraph_t g, hipGraphNode_t *node, const std::vector<hipGraphNode_t> &deps,
                            const void *func, dim3 grid, dim3 block, Args... args) {
  void *params[] = {(void *)&args...};
  const hipKernelNodeParams p = kernel_node_params(func, grid, block, 0, params);
  return hipGraphAddKernelNode(node, g, deps.empty() ? nullptr : deps.data(), deps.size(), &p);
}
template <typename... Args>
hipError_t graph_set_kernel(hipGraphExec_t exec, hipGraphNode_t node, const void *func, dim3 grid, dim3 block,
                            Args... args) {
  void *params[] = {(void *)&args...};
  const hipKernelNodeParams p = kernel_node_params(func, grid, block, 0, params);
  return hipGraphExecKernelNodeSetParams(exec, node, &p);
}

// pinned, host-coherent result words of the one-launch paths (grid_sync.hpp): [0..5) sums, [5] the barriers' error word
int ensure_result_word(pdhg_handle *h) {
  if (h->seq_dev) return 0;
  HIP_TRY(hipMalloc((void **)&h->seq_dev, sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(h->seq_dev, 0, sizeof(unsigned long long), nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));   // the null stream does not order against h->stream
  HIP_TRY(hipHostMalloc((void **)&h->res_host, (RES_HOST_CAP + 2) * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped));
  for (int q = 0; q < RES_HOST_CAP + 2; ++q) h->res_host[q] = 0.0;
  return 0;
}

// wait for launch number seq_expected's results in pinned memory; the barriers' error word goes to h->res_error
int wait_result_word(pdhg_handle *h, double out[5]) {
  double w[RES_HOST_K];
  const int rc = wait_words(h->stream, h->res_host, RES_HOST_CAP, RES_HOST_K, h->seq_expected, w, 40000000L,
                            "one-launch trial finished without publishing its results");
  if (rc == 998)      // resynchronise: the next launch can succeed
    h->seq_expected = reinterpret_cast<const volatile unsigned long long *>(h->res_host)[RES_HOST_CAP + 1];
  if (rc) return rc;
  for (int q = 0; q < 5; ++q) out[q] = w[q];
  h->res_error = w[5];
  out[4] *= 0.5;
  return 0;
}

