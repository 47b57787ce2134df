// host_trial_graph_build.hpp -- part of the single translation unit pdhg_hip.hip (included there, at the place its text used to stand).
// The trial step as a HIP graph, second part: eligibility, the two sinks that turn a fused product's steps (host_product.hpp:
// which kernels, in which form, with which arguments) into graph nodes and into parameter updates, building and launch (host
// side; the node helpers are in host_trial_graph.hpp).

bool graph_eligible(pdhg_handle *h) {
  if (h->graph_mode < 0) {
    const char *ev = getenv("PDHG_GRAPH");
    // stream layouts only.  The sweep can run as graph nodes too (PDHG_GRAPH_TILED=1) but gains nothing: with the
    // take_step loop in C the separate launches already overlap the kernels -- random 1M x 1M 5 709 it/s as a graph
    // against 5 637, 4M x 4M 1 667 / 1 672, config S 611 / 613 (profiles/r03_trial_kernel.txt).
    const bool tiled_ok = dev_env("PDHG_GRAPH_TILED") != nullptr;
    bool on = !h->grp && !h->has_q && h->n > 0 && h->A.segs.empty() && h->At.segs.empty() && (tiled_ok || (!h->A.tiled && !h->At.tiled));
    if (ev) on = on && ev[0] != '0';
    h->graph_mode = on ? 1 : 0;
  }
  return h->graph_mode == 1 && !h->has_q && !h->profile;
}

void graph_destroy(pdhg_handle::TrialGraph &G) {
  if (G.exec) (void)hipGraphExecDestroy(G.exec);
  if (G.graph) (void)hipGraphDestroy(G.graph);
  G = pdhg_handle::TrialGraph();
}

// the argument packs of the three nodes whose scalars change from trial to trial
struct GraphArgs {
  pdhg_handle *h;
  int n;
  dim3 primal_grid;
  EpiArgs dual_epi;
  GraphArgs(pdhg_handle *h_, double sigma) : h(h_), n((int)h_->n), primal_grid(ew_grid((h_->n + 1) / 2)) {
    dual_epi = dual_epilogue(h, sigma);
  }
};

// (code placement, third list: see spmv_placement_a in pdhg_hip.hip)
[[maybe_unused]] const void *const spmv_placement_c[] = {
    (const void *)spmv_stream_pipe_kernel<1, true, 0>, (const void *)spmv_stream_kernel<1, true, 0>, (const void *)spmv_stream_pipe_kernel<1, false, 0>,
    (const void *)spmv_stream_kernel<1, false, 0>, (const void *)spmv_long_final_kernel<1>};

// A fused product's steps (host_product.hpp) as graph nodes: the chain's passes depend on one another, the long-row pair
// is a parallel branch off `deps`.
struct GraphAddSink {
  static constexpr bool issues = true;
  hipGraph_t graph;
  const std::vector<hipGraphNode_t> &deps;
  hipGraphNode_t chain = nullptr, epi = nullptr, part = nullptr, fin = nullptr;      // the chain's last node so far; the roles' nodes
  template <class... P>
  int operator()(StepRole role, const KernelRef<P...> &k, dim3 grid, dim3 block, size_t lds, const step_arg_t<P> &...args) {
    const bool lng = role == STEP_LONG_PARTIAL || role == STEP_LONG_FINAL;
    const hipGraphNode_t after = role == STEP_LONG_FINAL ? part : (lng ? nullptr : chain);
    hipGraphNode_t &nd = role == STEP_LONG_FINAL ? fin : (lng ? part : chain);
    void *params[] = {const_cast<void *>((const void *)&args)...};
    const hipKernelNodeParams p = kernel_node_params((const void *)k.fn, grid, block, lds, params);
    HIP_TRY(hipGraphAddKernelNode(&nd, graph, after ? &after : (deps.empty() ? nullptr : deps.data()), after ? 1 : deps.size(), &p));
    if (role == STEP_EPILOGUE) epi = nd;
    return 0;
  }
};

// nodes of one fused SpMV.  `done` receives the nodes the next stage must wait for;
// main_node / long_node (optional) receive the nodes that carry the epilogue's scalars.
template <int MODE, int TAG>
int graph_add_spmv(pdhg_handle *h, hipGraph_t graph, const CsrDev &D, const double *xin, const EpiArgs &e,
                   const std::vector<hipGraphNode_t> &deps, std::vector<hipGraphNode_t> &done,
                   hipGraphNode_t *main_node, hipGraphNode_t *long_node) {
  GraphAddSink sink{graph, deps};
  if (int rc = product_steps<MODE, TAG>(h, D, xin, e, sink)) return rc;
  if (sink.chain) done.push_back(sink.chain);
  if (sink.fin) done.push_back(sink.fin);
  if (main_node && sink.epi) *main_node = sink.epi;
  if (long_node && sink.fin) *long_node = sink.fin;
  return 0;
}

// the same walk again with a new epilogue: only the nodes that carry it get new parameters
struct GraphSetSink {
  static constexpr bool issues = true;
  hipGraphExec_t exec;
  hipGraphNode_t epi, fin;
  template <class... P>
  int operator()(StepRole role, const KernelRef<P...> &k, dim3 grid, dim3 block, size_t lds, const step_arg_t<P> &...args) {
    const hipGraphNode_t nd = role == STEP_EPILOGUE ? epi : (role == STEP_LONG_FINAL ? fin : nullptr);
    if (!nd) return 0;
    void *params[] = {const_cast<void *>((const void *)&args)...};
    const hipKernelNodeParams p = kernel_node_params((const void *)k.fn, grid, block, lds, params);
    HIP_TRY(hipGraphExecKernelNodeSetParams(exec, nd, &p));
    return 0;
  }
};

// the dual product's nodes again, with a new sigma
int graph_set_dual(pdhg_handle *h, pdhg_handle::TrialGraph &G, const EpiArgs &dual_epi) {
  GraphSetSink sink{G.exec, G.n_dual, G.n_dual_long};
  return product_steps<MODE_DUAL, 0>(h, h->A, h->xbar, dual_epi, sink);
}

int graph_build(pdhg_handle *h, pdhg_handle::TrialGraph &G, double tau, double theta, double sigma) {
  graph_destroy(G);
  int rcw = ensure_result_word(h);
  if (rcw) return rcw;
  HIP_TRY(hipGraphCreate(&G.graph, 0));
  GraphArgs a(h, sigma);
  const double *nullq = nullptr;
  // K1+K2
  HIP_TRY(graph_add_kernel(G.graph, &G.n_primal, {}, (const void *)primal_kernel<false, true>, a.primal_grid, dim3(TPB),
                           a.n, (const double *)h->x, (const double *)h->c, (const double *)h->aty, nullq,
                           bound_view(h, 0), bound_view(h, 1), tau, theta, h->x_next, h->xbar,
                           h->pend_w, h->pend_x ? h->sum_x : (double *)nullptr, 0.0, (double *)nullptr, 0));
  // K3+K4 on CSR(A), K5+K6 on CSR(A'): the stream kernel (or its column-slab passes, a
  // chain) and the long-row pair are independent branches
  std::vector<hipGraphNode_t> dual_done, aty_done;
  {
    int rc = graph_add_spmv<MODE_DUAL, 0>(h, G.graph, h->A, h->xbar, a.dual_epi, {G.n_primal}, dual_done, &G.n_dual, &G.n_dual_long);
    if (rc) return rc;
  }
  if (dual_done.empty()) dual_done.push_back(G.n_primal);
  const CsrDev &A = h->A;
  const CsrDev &T = h->At;
  {
    int rc = graph_add_spmv<MODE_ATY, 1>(h, G.graph, T, h->y_next, aty_epilogue(h), dual_done, aty_done, nullptr, nullptr);
    if (rc) return rc;
  }
  if (aty_done.empty()) aty_done = dual_done;
  // K6b -> pinned host memory + sequence number
  const FinalSpec sp = trial_final_spec(h, T.slots(), A.slots(), 0, A.slots(), nullptr);
  hipGraphNode_t fin = nullptr;
  HIP_TRY(graph_add_kernel(G.graph, &fin, aty_done, (const void *)final_reduce_host_kernel, dim3(1), dim3(FINAL_TPB), sp,
                           h->seq_dev, h->res_host));
  HIP_TRY(hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0));
  G.x = h->x; G.y = h->y; G.aty = h->aty;
  G.tau = tau; G.theta = theta; G.sigma = sigma;
  G.bounds_version = h->bounds_version;
  G.add_x = h->pend_x; G.add_wx = h->pend_w;
  G.add_y = h->pend_y; G.add_wy = h->pend_w;
  return 0;
}

int graph_trial(pdhg_handle *h, const TrialArgs &ta, double out[5]) {
  const double tau = ta.step_size / ta.primal_weight, sigma = ta.primal_weight * ta.step_size, theta = ta.theta;
  if (int rcb = bounds_fresh(h)) return rcb;       // (the primal node carries the views)
  pdhg_handle::TrialGraph *G = nullptr;
  for (int k = 0; k < 2; ++k)
    if (h->tgraph[k].exec && h->tgraph[k].x == h->x && h->tgraph[k].y == h->y && h->tgraph[k].aty == h->aty)
      G = &h->tgraph[k];
  if (!G) {
    G = !h->tgraph[0].exec ? &h->tgraph[0] : (!h->tgraph[1].exec ? &h->tgraph[1] : &h->tgraph[0]);
    int rc = graph_build(h, *G, tau, theta, sigma);
    if (rc) return rc;
  } else {
    const auto c0 = std::chrono::steady_clock::now();
    GraphArgs a(h, sigma);
    if (G->tau != tau || G->theta != theta || G->add_x != h->pend_x || (h->pend_x && G->add_wx != h->pend_w) ||
        G->bounds_version != h->bounds_version) {      // (bounds_rebuild: the node's views point at freed arrays)
      const double *nullq = nullptr;
      HIP_TRY(graph_set_kernel(G->exec, G->n_primal, (const void *)primal_kernel<false, true>, a.primal_grid, dim3(TPB),
                               a.n, (const double *)h->x, (const double *)h->c, (const double *)h->aty, nullq,
                               bound_view(h, 0), bound_view(h, 1), tau, theta, h->x_next, h->xbar,
                               h->pend_w, h->pend_x ? h->sum_x : (double *)nullptr, 0.0, (double *)nullptr, 0));
      G->tau = tau; G->theta = theta; G->bounds_version = h->bounds_version;
      G->add_x = h->pend_x; G->add_wx = h->pend_w;
    }
    if (G->sigma != sigma || G->add_y != h->pend_y || (h->pend_y && G->add_wy != h->pend_w)) {
      int rc = graph_set_dual(h, *G, a.dual_epi);
      if (rc) return rc;
      G->sigma = sigma;
      G->add_y = h->pend_y; G->add_wy = h->pend_w;
    }
    h->t_set += std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
  }
  h->seq_expected += 1;
  const auto c1 = std::chrono::steady_clock::now();
  HIP_TRY(hipGraphLaunch(G->exec, h->stream));
#ifdef PDHG_PROBE_GRAPH_TWICE      // latency probe only (the deferred sums are applied twice): the boundary between two queued graphs, tools/archive/r6_w.sh
  HIP_TRY(hipGraphLaunch(G->exec, h->stream));
  h->seq_expected += 1;
#endif
  const auto c2 = std::chrono::steady_clock::now();
  h->t_launch += std::chrono::duration<double>(c2 - c1).count();
  h->n_graph_trials += 1;
  h->pend_x = h->pend_y = false;     // the launch carries the deferred average update
  int rcw = wait_result_word(h, out);
  h->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - c2).count();
  return rcw;
}

// A batch handle, or a member of a batch, whose batch was given new matrix values and has not been rescaled since
// (pdhg_batch_update_matrix_values): the members hold the vectors of the old scaling, the matrix the new raw values.
// Every entry point but pdhg_rescale on the batch handle, pdhg_destroy and the info calls refuses such a handle.
// rescales: the caller is pdhg_rescale, which a batch that awaits it accepts.
int batch_awaits_rescale(const pdhg_handle *h, const std::string &who, bool rescales = false) {
  const pdhg_handle *b = h->owner ? h->owner : h;
  if (b->members_await_rescale == 2)
    return fail(-1, who + "an update of the batch's matrix values failed on the device midway: its matrix and its members' vectors "
                          "disagree; destroy the batch (pdhg_destroy)");
  if (!b->members_await_rescale || rescales) return 0;
  return fail(-1, who + "the batch was given new matrix values: rescale the batch first (pdhg_rescale on the batch handle)");
}

// queues_work: the entry point may put work on the shards' own streams (everything but a trial step and a lazy accept)
// rescales: the entry point is pdhg_rescale, which a batch that awaits it (batch_awaits_rescale) accepts
int check_handle(pdhg_handle *h, bool queues_work = true, bool batch_ok = false, bool rescales = false) {
  if (!h) return fail(-1, "null handle");
  if (h->fleet) return fail(-1, "a fleet handle runs no iterations of its own: call this on a member (pdhg_fleet_add)");
  if (h->bat && !batch_ok) return fail(-1, "a batch handle holds the shared matrix only: call this on a member (pdhg_batch_member)");
  if (int rcw = batch_awaits_rescale(h, "", rescales)) return rcw;
  if (queues_work && h->grp && !h->grp->coop_dev.empty()) {
    DistGroup &g = *h->grp;
    if (g.join_pending) {          // the members' streams wait for the last persistent group launch (group_kernel.hpp)
      for (GroupDevLaunch &D : g.coop_dev) {
        HIP_TRY(hipSetDevice(D.device));
        for (int i : D.members)
          if (g.sh[(size_t)i]->stream != D.stream) HIP_TRY(hipStreamWaitEvent(g.sh[(size_t)i]->stream, D.ev_done, 0));
      }
      g.join_pending = false;
    }
    g.members_dirty = true;
  }
  HIP_TRY(hipSetDevice(h->device));
  return 0;
}

int sync_all(const Shards &L) {
  FOR_SHARDS(L, s) HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}

// Settle a deferred K7 (lazy accept): sum_x += w * x and / or sum_y += w * y on the
// iterate that is current now.  Called by every entry point other than the trial itself.
int flush_pending(const Shards &L) {
  FOR_SHARDS(L, h) {
    drop_staging(h);          // the pending term goes into the sums themselves: alternates made from them are stale
    if (!h->pend_x && !h->pend_y) continue;
    ProfScope ps(h, PDHG_K_ACCEPT);
    const int64_t o = h->clo;
    const int nn = h->pend_x ? (int)h->cn : 0, mm = h->pend_y ? (int)h->m : 0;
    hipLaunchKernelGGL(accept_kernel, dim3(ew_grid(std::max<int64_t>(std::max(nn, mm), 1))), dim3(TPB), 0, h->stream, nn, mm,
                       h->pend_w, h->x + o, h->sum_x + o, h->y, h->sum_y);
    HIP_TRY(hipGetLastError());
    h->pend_x = h->pend_y = false;
  }
  return 0;
}

void bump_version(const Shards &L) {   // x, y, the running sums or A change: cached A*x / A'*y are stale
  for (int i = 0; i < L.count; ++i) L.p[i]->state_version += 1;
}
