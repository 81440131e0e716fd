// What the C-ABI of libndq.so (csrc/ndq_api.hip) and of libndq64.so (csrc/ndq_api64.hip, NDQ_F64) have in common, written
// once against ndq::real: NDQ_API(x) names the entry point ndq_x / ndq64_x of include/ndq.h.
//   * descriptor dispatch: the kernel table lookup and the seven *_mlp_* entry points
//   * the *_epoch_tail and *_adam_step entry points around ndq_tail.h's epoch_tail_kernel<T> / adam_kernel<T>
//   * NDQ_PIN16: the statement that keeps sixteen rows of a column-sum thread in flight at once
//   * fused_steps_ok / fused_steps_run: a training epoch of 1..4 networks as closure launch + ONE sums / tail launch
// Include it after ndq_launch.h and ndq_tail.h, and after the including file has defined what is its own:
//   NDQ_API_KERNELS       the initialiser list of its built-in kernel table (make_kernels<Cfg<...>>(), ...)
//   ndq::hidden_ok(desc)  the hidden widths its kernels serve
#pragma once
#include <vector>

#if NDQ_F64
#define NDQ_API(name) ndq64_##name
#else
#define NDQ_API(name) ndq_##name
#endif

namespace ndq {

// ---------------------------------------------------------------------------------------------- descriptor dispatch
static const kernels_record kTable[] = {NDQ_API_KERNELS};
static std::vector<const kernels_record*> g_registered;     // extension modules (*_mlp_register)

static const kernels_record* find(const ndq_mlp_desc* d) {
  if (!d || !hidden_ok(*d)) return nullptr;
  for (const kernels_record& e : kTable)
    if (same_desc(e.desc, *d)) return &e;
  for (const kernels_record* e : g_registered)
    if (same_desc(e->desc, *d)) return e;
  return nullptr;
}

// ---------------------------------------------------------------------------------------------- column sums
// The column sums of both libraries (ndq_api.hip ColumnRows, ndq_api64.hip reduce_partials64_kernel / reduce_tail64_kernel)
// issue sixteen rows of a thread as straight-line CLAMPED loads and only then select and add.  A load whose value is only
// used under "row < nparts" gets sunk into that branch by the compiler -- one load + s_waitcnt per row, a memory round trip
// each (seen in the ISA) -- so the loads are unconditional and this ONE empty asm statement, which needs all sixteen raw
// values live at once, stands between them and the selection.  A macro, not a function over a row-chunk struct: with the
// struct (issue() / pin() members) every kernel that used it came out with other register numbers and another instruction
// order -- same work, but not the device code the bit-for-bit tests and the timings of profiles/ were taken on.
// What happens to the values afterwards is NOT shared either: the fp32 sums replace the rows at or past nparts by +0.0f and
// add all sixteen, the fp64 sums (column_chunk64) skip those rows, so that a column of -0.0 stays -0.0 like in the loop it
// replaces.  Different arithmetic, each pinned bit for bit by tests: two functions.
#define NDQ_PIN16(x)                                                                                                          \
  asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(x[8]), \
                    "+v"(x[9]), "+v"(x[10]), "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15]))

// ---------------------------------------------------------------------------------------------- fused step
// What *_fused_multi_step_run / ndq64_fused_step_run / ndq64_reduce_tail check before any HIP call.  Step: ndq_fused_step or
// ndq64_fused_step.  Network 0 carries what the system shares: loss partials, history, best loss, row count.
template <class Step>
static bool fused_steps_ok(const Step* steps, int n_nets, int adam_step, int hist_index, int parity) {
  if (!steps || n_nets < 1 || n_nets > 4 || adam_step <= 0 || hist_index < 0 || (parity != 0 && parity != 1)) return false;
  const Step& s0 = steps[0];
  if (!s0.loss_partials || !s0.loss_hist || !s0.best_loss || !s0.loss_slot || s0.blocks <= 0) return false;
  for (int k = 0; k < n_nets; ++k) {
    const Step& s = steps[k];
    if (!s.params || !s.partials || !s.grad || !s.adam_m || !s.adam_v || s.n_params <= 0) return false;
#if !NDQ_F64
    if (!s.loss_slot) return false;        // (fp32: every network's tail is handed its own slot; fp64: network 0's serves all)
#endif
  }
  return true;
}

// Validate, launch the closure kernel of all networks (`launch`: the generated module's multi-network launcher), then the
// library's sums + tail launch `sums_tail` over the partial rows it left.
template <class Step, class Launch>
static int fused_steps_run(const Step* steps, int n_nets, Launch launch, const real* coords, int adam_step, int hist_index,
                           int parity, void* stream, int (*sums_tail)(const Step*, int, int, int, int, void*)) {
  if (!launch || !coords || !fused_steps_ok(steps, n_nets, adam_step, hist_index, parity)) return NDQ_EINVAL;
  const Step& s0 = steps[0];
  const real* params[4];
  real* partials[4];
  for (int k = 0; k < n_nets; ++k) {
    params[k] = steps[k].params;
    partials[k] = steps[k].partials;
  }
  int rc = launch(coords, s0.ldc, s0.n, params, partials, s0.loss_partials, nullptr, nullptr, s0.ldj, s0.seed, 1, stream);
  if (rc) return rc;
  return sums_tail(steps, n_nets, adam_step, hist_index, parity, stream);
}

}  // namespace ndq

extern "C" {

int NDQ_API(mlp_supported)(const ndq_mlp_desc* desc) { return ndq::find(desc) ? 1 : 0; }

int NDQ_API(mlp_register)(const ndq::kernels_record* k) {
  if (!k || !k->fwd || !k->bwd || !ndq::hidden_ok(k->desc) || k->n_streams < 1 || k->n_params < 1 || k->bwd_waves < 1 ||
      k->lds_bytes > 160 * 1024)
    return NDQ_EINVAL;
  if (!ndq::find(&k->desc)) ndq::g_registered.push_back(k);
  return 0;
}

int NDQ_API(mlp_num_streams)(const ndq_mlp_desc* desc) {
  const ndq::kernels_record* e = ndq::find(desc);
  return e ? e->n_streams : NDQ_EUNSUPPORTED;
}

int NDQ_API(mlp_num_params)(const ndq_mlp_desc* desc) {
  const ndq::kernels_record* e = ndq::find(desc);
  return e ? e->n_params : NDQ_EUNSUPPORTED;
}

int NDQ_API(mlp_bwd_blocks)(const ndq_mlp_desc* desc, int n) {
  const ndq::kernels_record* e = ndq::find(desc);
  if (!e) return NDQ_EUNSUPPORTED;
  if (n <= 0) return NDQ_EINVAL;
  return ndq::bwd_blocks(e->bwd_waves, n);
}

int NDQ_API(mlp_jet_fwd)(const ndq_mlp_desc* desc, const ndq::real* coords, int ldc, int n, const ndq::real* params,
                         ndq::real* jets, int ldj, void* stream) {
  const ndq::kernels_record* e = ndq::find(desc);
  if (!e) return NDQ_EUNSUPPORTED;
  if (!coords || !params || !jets || n <= 0 || ldc < n || ldj < n) return NDQ_EINVAL;
  return e->fwd(coords, ldc, n, params, jets, ldj, stream);
}

int NDQ_API(mlp_jet_bwd)(const ndq_mlp_desc* desc, const ndq::real* coords, int ldc, int n, const ndq::real* params,
                         const ndq::real* gbar, int ldj, ndq::real* partials, void* stream) {
  const ndq::kernels_record* e = ndq::find(desc);
  if (!e) return NDQ_EUNSUPPORTED;
  if (!coords || !params || !gbar || !partials || n <= 0 || ldc < n || ldj < n) return NDQ_EINVAL;
  return e->bwd(coords, ldc, n, params, gbar, ldj, partials, ndq::bwd_blocks(e->bwd_waves, n), stream);
}

// Adam and the device-side end of an epoch whose sums are done: ONE source in float and in double, so an fp64 epoch through
// ndq64_epoch_tail and one through ndq64_adam_step agree bit for bit, like their fp32 twins
int NDQ_API(adam_step)(ndq::real* params, const ndq::real* grad, ndq::real* exp_avg, ndq::real* exp_avg_sq, int len,
                       ndq::real lr, ndq::real beta1, ndq::real beta2, ndq::real eps, ndq::real weight_decay, int step,
                       void* stream) {
  if (!params || !grad || !exp_avg || !exp_avg_sq || len <= 0 || step <= 0) return NDQ_EINVAL;
  hipLaunchKernelGGL(ndq::adam_kernel<ndq::real>, dim3((len + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), params,
                     grad, exp_avg, exp_avg_sq, len, ndq::adam_consts(lr, beta1, beta2, eps, weight_decay, step));
  return (int)hipGetLastError();
}

int NDQ_API(epoch_tail)(ndq::real* params, const ndq::real* grad, ndq::real* exp_avg, ndq::real* exp_avg_sq, int len,
                        ndq::real lr, ndq::real beta1, ndq::real beta2, ndq::real eps, ndq::real weight_decay, int step,
                        const ndq::real* loss_slots, int n_batches, ndq::real* loss_hist, int hist_index,
                        ndq::real* best_loss, int parity, ndq::real* best_flat, int write_scalars, void* stream) {
  const bool adam = exp_avg != nullptr;
  if (!params || len <= 0 || !loss_slots || n_batches <= 0 || !loss_hist || !best_loss || hist_index < 0 ||
      (parity != 0 && parity != 1) || (adam && (!grad || !exp_avg_sq || step <= 0)))
    return NDQ_EINVAL;
  ndq::TailArgsT<ndq::real> a{};
  a.p = params; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.len = len;
  a.adam = ndq::adam_consts(lr, beta1, beta2, eps, weight_decay, adam ? step : 0);
  a.loss_slots = loss_slots; a.nb = n_batches; a.loss_hist = loss_hist; a.hist_index = hist_index;
  a.best_loss = best_loss; a.parity = parity; a.best_flat = best_flat; a.write_scalars = write_scalars;
  hipLaunchKernelGGL(ndq::epoch_tail_kernel<ndq::real>, dim3((len + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

}  // extern "C"
