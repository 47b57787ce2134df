// host_product.hpp -- part of the single translation unit pdhg_hip.hip (included there, in front of launch_spmv).
// The kernel steps of one fused sparse product, stated ONCE: product_steps<MODE, TAG> walks a layout and hands every kernel
// step -- function, profiler name, launch shape, typed arguments, role -- to a sink, exactly once and in issue order.  The
// sinks: LaunchSink (launch_spmv, launch_spmv_plain_part, launch_tiled: below and in pdhg_hip.hip), GraphAddSink and
// GraphSetSink (the trial graph's nodes and the re-parameterised dual nodes: host_trial_graph_build.hpp) and NameSink
// (pdhg_kernel_name, pdhg_layout_describe).  A new kernel variant, template instance or argument is added HERE.

enum ProductKind { PRODUCT_SWEEP, PRODUCT_SJ, PRODUCT_PIPE, PRODUCT_BLOCKS };
// the form one pass over row blocks was built in (a whole stream-class layout or one column slab of it) ...
template <class L>
ProductKind pass_kind(const L &S) {
  return S.sj.on() ? PRODUCT_SJ : (S.pipe_grid > 0 ? PRODUCT_PIPE : PRODUCT_BLOCKS);
}
// ... and a layout's, looking through its column slabs (all slabs share one form: build_sj_copies)
inline ProductKind product_kind(const CsrDev &D) {
  return D.tiled ? PRODUCT_SWEEP : (D.slabs.empty() ? pass_kind(D) : pass_kind(D.slabs.front()));
}

// STEP_PASS: a column-slab pass that hands its row sums on; STEP_EPILOGUE: the pass that carries the caller's epilogue
// (the last of the chain, or the only one); the long-row pair runs beside the chain
enum StepRole { STEP_PASS, STEP_EPILOGUE, STEP_LONG_PARTIAL, STEP_LONG_FINAL };

// One kernel instance: its function and its name as rocprofv3 prints it, both made from the same tokens (PDHG_KERNEL).
struct TArg {
  int v = 0;
  bool is_bool = false;
  TArg() = default;
  TArg(int x) : v(x) {}
  TArg(bool x) : v(x), is_bool(true) {}
};
template <class... P>
struct KernelRef {
  void (*fn)(P...);
  const char *family;
  TArg targ[4];
  int ntarg;
  std::string name() const {
    std::string s = std::string(family) + "<";
    for (int i = 0; i < ntarg; ++i) s += (i ? ", " : "") + (targ[i].is_bool ? std::string(targ[i].v ? "true" : "false") : std::to_string(targ[i].v));
    return s + ">";
  }
};
template <class... P, class... T>
KernelRef<P...> kernel_ref(void (*fn)(P...), const char *family, T... t) {
  return KernelRef<P...>{fn, family, {TArg(t)...}, (int)sizeof...(T)};
}
#define PDHG_KERNEL(K, ...) kernel_ref(K<__VA_ARGS__>, #K, __VA_ARGS__)
// a sink's argument types come from the kernel's signature alone (const step_arg_t<P> &...): what the walk passes binds
// to them directly or is converted, and the sink points the launch's parameter array at them -- no copy of its own
template <class T> struct step_arg { using type = T; };
template <class T> using step_arg_t = typename step_arg<T>::type;

// The sweep over the workgroups [g0, g1): the five chunk variants, the dynamic-LDS opt-in (sinks that issue), the XCD dealing.
template <int MODE, class Sink>
int sweep_step(const pdhg_handle *h, const CsrDev &D, const double *xin, const EpiArgs &e, int g0, int g1, Sink &sink) {
  const size_t lds = tiled_lds_bytes(D);
  const int w0 = g0 * TW_WPB;
  const int per_xcd = tiled_per_xcd(h, D, g1 - g0);
  const auto k = D.tw_mode == 1   ? PDHG_KERNEL(spmv_tiled_kernel, MODE, 1)
                 : D.tw_mode == 2 ? PDHG_KERNEL(spmv_tiled_kernel, MODE, 2)
                 : D.tw_mode == 3 ? PDHG_KERNEL(spmv_tiled_kernel, MODE, 3)
                 : D.tw_mode == 4 ? PDHG_KERNEL(spmv_tiled_kernel, MODE, 4)
                                  : PDHG_KERNEL(spmv_tiled_kernel, MODE, 0);      // (the builder sets tw_mode to 0 ... 4 only)
  if (Sink::issues)
    if (int rc = ensure_lds_limit(h, MODE, k.targ[1].v, lds, (const void *)k.fn)) return rc;
  return sink(STEP_EPILOGUE, k, dim3(per_xcd > 0 ? per_xcd * NUM_XCD : g1 - g0), dim3(TW_WPB * WAVE), lds, D.wave_rows + w0, D.wave_ent,
              D.wave_step_off + w0, D.step_tile, D.wg_step_off + g0, D.nwaves - w0, D.tile_shift, D.tw_rows, D.pk, D.tv, xin, e, g1 - g0, per_xcd);
}

// One pass over the row blocks of S (a layout or a column slab; `view`: its CSR arrays) in the form it was built in.  A slab's
// stream-kernel pass carries flag 2 (rx | 2); the pass with the epilogue owns the block-partial slots of S.grid.
template <int MODE, bool INIT, int TAG, class L, class Sink>
int pass_step(const pdhg_handle *h, const L &S, const CsrView &view, bool slab, StepRole role, const double *xin, const EpiArgs &e, Sink &sink) {
  const int rm = h->remap ? 1 : 0, rx = h->relaxed ? 1 : 0, slots = role == STEP_EPILOGUE ? S.grid : 0;
  switch (pass_kind(S)) {
    case PRODUCT_SJ:
      return sink(role, S.sj.G > 1 ? PDHG_KERNEL(spmv_sj_kernel, MODE, INIT, TAG, SJ_WIDE_G) : PDHG_KERNEL(spmv_sj_kernel, MODE, INIT, TAG, 1),
                  dim3(S.sj.grid), dim3(TPB), 0, sj_view(S.sj, rx), xin, rm, slots, e);
    case PRODUCT_PIPE:
      return sink(role, PDHG_KERNEL(spmv_stream_pipe_kernel, MODE, INIT, TAG), dim3(S.pipe_grid), dim3(TPB), 0, view, xin, S.ext, S.nblk,
                  S.per_xcd, rm, rx, slots, e);
    default:
      return sink(role, PDHG_KERNEL(spmv_stream_kernel, MODE, INIT, TAG), dim3(S.grid), dim3(TPB), 0, view, xin, S.blks, S.ext, S.nblk,
                  S.per_xcd, rm, slab ? rx | 2 : rx, e);
  }
}

// The long-row pair of D (nothing when D has no long rows): chunk sums, then one wave per row with the epilogue.
template <int MODE, int TAG, class Sink>
int long_steps(const CsrDev &D, const double *xin, const EpiArgs &e, Sink &sink) {
  if (D.nlong <= 0) return 0;
  int rc;
  if ((rc = sink(STEP_LONG_PARTIAL, PDHG_KERNEL(spmv_long_partial_kernel, TAG), dim3(D.nchunks), dim3(TPB), 0, D.view(), xin, D.chunk_row,
                 D.chunk_off, D.chunk_partial)))
    return rc;
  return sink(STEP_LONG_FINAL, PDHG_KERNEL(spmv_long_final_kernel, MODE), dim3(D.long_grid), dim3(TPB), 0, D.long_row, D.long_chunk_ptr, D.nlong,
              D.chunk_partial, e, D.grid);
}

// Every kernel step of the product of layout D (no row segments: launch_spmv loops over those) with epilogue `e`; e.init !=
// nullptr: the row sums start from e.init[row] (a carried product).  Stops at the first sink that returns non-zero.
// (launch_spmv_plain_part, which runs a sweep in rounds of workgroups, calls long_steps and sweep_step itself.)
template <int MODE, int TAG, class Sink>
int product_steps(const pdhg_handle *h, const CsrDev &D, const double *xin, const EpiArgs &e, Sink &sink) {
  int rc = 0;
  if (D.tiled) {
    if (D.grid > 0) rc = sweep_step<MODE>(h, D, xin, e, 0, D.grid, sink);
  } else if (!D.slabs.empty()) {
    // column-slab passes, ascending: partial row sums travel through slab_partial
    const size_t P = D.slabs.size();
    EpiArgs pe{}, le = e;
    pe.out = D.slab_partial;
    pe.init = le.init = D.slab_partial;
    for (size_t p = 0; p < P && !rc; ++p) {
      const SlabDev &S = D.slabs[p];
      const CsrView view = S.view(D.rows);
      if (p + 1 == P) rc = pass_step<MODE, true, TAG>(h, S, view, true, STEP_EPILOGUE, xin, le, sink);
      else if (p == 0) rc = pass_step<MODE_PLAIN, false, TAG>(h, S, view, true, STEP_PASS, xin, pe, sink);
      else rc = pass_step<MODE_PLAIN, true, TAG>(h, S, view, true, STEP_PASS, xin, pe, sink);
    }
  } else if (pass_kind(D) != PRODUCT_BLOCKS || D.grid > 0) {
    if (e.init) rc = pass_step<MODE, true, TAG>(h, D, D.view(), false, STEP_EPILOGUE, xin, e, sink);
    else rc = pass_step<MODE, false, TAG>(h, D, D.view(), false, STEP_EPILOGUE, xin, e, sink);
  }
  return rc ? rc : long_steps<MODE, TAG>(D, xin, e, sink);
}

// ---- the sinks that need no graph: direct launches and names

// launches on one stream; the caller checks hipGetLastError once behind the walk
struct LaunchSink {
  static constexpr bool issues = true;
  hipStream_t stream;
  template <class... P>
  int operator()(StepRole, const KernelRef<P...> &k, dim3 grid, dim3 block, size_t lds, const step_arg_t<P> &...args) {
    void *params[] = {const_cast<void *>((const void *)&args)...};
    (void)hipLaunchKernel((const void *)k.fn, grid, block, params, lds, stream);
    return 0;
  }
};

// the step names joined by " + " (the middle slab passes share one name: once)
struct NameSink {
  static constexpr bool issues = false;
  std::string out, last;
  template <class... P, class... A>
  int operator()(StepRole role, const KernelRef<P...> &k, dim3, dim3, size_t, const A &...) {
    const std::string name = k.name();
    if (role != STEP_PASS || name != last) out += (out.empty() ? "" : " + ") + name;
    last = name;
    return 0;
  }
};

// The kernels behind one fused product, as rocprofv3 prints them (template arguments <MODE,
// INIT, TAG> / <MODE, CH> / <TAG>; MODE 0 plain, 1 dual epilogue, 2 A'y epilogue; TAG 0 = A,
// 1 = A'), joined by " + ": a profile of the separate launches adds up to the product by
// summing these names (tools/rocprof_summary.py does).  They are the names of the steps launch_spmv issues; (mode, tag)
// is one of the five products the library runs (another pair would add kernel instances).
template <int MODE, int TAG>
std::string product_names(const pdhg_handle *h, const CsrDev &D) {
  NameSink names;
  (void)product_steps<MODE, TAG>(h, D, nullptr, EpiArgs{}, names);
  return names.out.empty() ? "(no kernel: empty matrix)" : names.out;
}
std::string product_kernels(const pdhg_handle *h, const CsrDev &D, int mode, int tag) {
  if (!D.segs.empty())
    return product_kernels(h, D.segs.front(), mode, tag) + " (x " + std::to_string(D.segs.size()) + " row segments)";
  if (mode == MODE_DUAL && tag == 0) return product_names<MODE_DUAL, 0>(h, D);
  if (mode == MODE_ATY && tag == 1) return product_names<MODE_ATY, 1>(h, D);
  if (mode == MODE_PLAIN && tag == 0) return product_names<MODE_PLAIN, 0>(h, D);
  if (mode == MODE_PLAIN && tag == 1) return product_names<MODE_PLAIN, 1>(h, D);
  if (mode == MODE_PLAIN && tag == 2) return product_names<MODE_PLAIN, 2>(h, D);
  return "?";
}
