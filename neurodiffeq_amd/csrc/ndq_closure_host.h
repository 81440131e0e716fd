// Host side of a generated single-launch closure module: the launchers and the extern "C" ndq_fused_* entry points
// (include/ndq.h: ndq_fused_launch_fn, ndq_fused_launch_tv_fn, ndq_fused_launch_loop_fn, plus the query functions
// codegen.FusedKernel reads).  Nothing in here is generated and nothing depends on the precision: everything is written
// against ndq::real, so the fp32 and the NDQ_F64 build of a module share this text.
//
// Included by: the modules neurodiffeq_amd/codegen.py emits (PointwiseProgram.fused_source), as their LAST line, after
// ndq_mlp.h / ndq_wide.h, the per-point function, `using CFG`, `struct PW` and -- the contract -- one traits struct
// named `Closure` in the module's anonymous namespace that says what differs between the closure kernels (one
// network on 16-point tiles, 2..4 networks, grouped, wide):
//
//   using Cfg, Pw               the ndq::Cfg / ndq::WideCfg instantiation and the generated per-point stage
//   using Args                  ndq::FusedArgs (one network) or ndq::FusedMultiArgs (K networks)
//   K                           networks (parameter sets) per launch
//   THREADS                     threads per workgroup
//   POINTS, SLOTS               a workgroup takes SLOTS units of POINTS points per round: fused_blocks(n) is
//                               ceil(ceil(n / POINTS) / SLOTS), at least 1, at most NDQ_MAX_BLOCKS
//   train, eval, tv             kernel entry points (constexpr pointers): training closure, forward-only closure,
//                               training + validation closure;  LDS_TRAIN, LDS_EVAL their dynamic LDS bytes
//   loop, LDS_LOOP              the loop-mode kernel and its LDS bytes, or `nullptr` and 0 where there is none
//   NO_PULL                     optional; true: the kernels have no pull prologue whatever the Cfg (evaluation-site modules)
#pragma once
#include <cstdlib>
#include <type_traits>

namespace {

template <class T> int fused_blocks(int n) {
  const int units = (n + T::POINTS - 1) / T::POINTS;
  int b = (units + T::SLOTS - 1) / T::SLOTS;
  return b > NDQ_MAX_BLOCKS ? NDQ_MAX_BLOCKS : (b < 1 ? 1 : b);
}

// trainable scalars of the equations (PW::NT of them): values read by every launch, block sums of their adjoints written by
// training launches -- bound by the engine before it launches (ndq_fused_bind_theta)
const ndq::real* g_theta = nullptr;
ndq::real* g_theta_partials = nullptr;

// params / partials: host arrays of K device pointers (one per network)
template <int K> void fill(ndq::FusedArgs& a, const ndq::real* const* params, ndq::real* const* partials) {
  a.params = params[0]; a.partials = partials ? partials[0] : nullptr;
}
template <int K> void fill(ndq::FusedMultiArgs& a, const ndq::real* const* params, ndq::real* const* partials) {
  for (int k = 0; k < K; ++k) { a.params[k] = params[k]; a.partials[k] = partials ? partials[k] : nullptr; }
}

// does the module's train + validation kernel carry the pull prologue (csrc/ndq_tail.h)?
template <class T, class = void> struct no_pull : std::false_type {};
template <class T> struct no_pull<T, std::void_t<decltype(T::NO_PULL)>> : std::bool_constant<T::NO_PULL> {};
template <class T> constexpr bool pull_ok() { return ndq::pull_supported<typename T::Cfg>() && !no_pull<T>::value; }

template <class T>
int launch(const ndq::real* coords, int ldc, int n, const ndq::real* const* params, ndq::real* const* partials,
           ndq::real* loss_partials, ndq::real* funcs, ndq::real* resid, int ldj, ndq::real seed, int train, void* stream) {
  if (!coords || !params || !loss_partials || n <= 0 || ldc < n || (train && !partials)) return -2;
  if (T::Pw::NT > 0 && !g_theta) return -2;
  typename T::Args a{};
  a.coords = coords; a.loss_partials = loss_partials;
  fill<T::K>(a, params, partials);
  a.funcs = funcs; a.resid = resid; a.n = n; a.ldc = ldc; a.ldj = ldj; a.seed = seed;
  a.theta = g_theta; a.theta_partials = train ? g_theta_partials : nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(T::train),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_TRAIN);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(T::eval),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_EVAL);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  if (train)
    hipLaunchKernelGGL(T::train, dim3(fused_blocks<T>(n)), dim3(T::THREADS), T::LDS_TRAIN, s, a);
  else
    hipLaunchKernelGGL(T::eval, dim3(fused_blocks<T>(n)), dim3(T::THREADS), T::LDS_EVAL, s, a);
  return (int)hipGetLastError();
}

// The train + validation closure kernel (csrc/ndq_mlp.h: fused_*_closure_tv_kernel): workgroups [0, blocks(n)) run the
// training closure on the training batch, the next blocks(vn) the forward-only closure on the validation batch;
// n = 0 / vn = 0 drops a half.
template <class T>
int launch_tv(const ndq::real* coords, int ldc, int n, const ndq::real* const* params, ndq::real* const* partials,
              ndq::real* loss_partials, ndq::real seed, const ndq::real* vcoords, int vldc, int vn,
              ndq::real* vloss_partials, const void* pull, void* stream) {
  if (!params || n < 0 || vn < 0 || (n == 0 && vn == 0)) return -2;
  if (n > 0 && (!coords || !partials || !loss_partials || ldc < n)) return -2;
  if (vn > 0 && (!vcoords || !vloss_partials || vldc < vn)) return -2;
  typename T::Args t{}, v{};
  t.coords = coords; t.loss_partials = loss_partials; t.n = n; t.ldc = ldc; t.ldj = ldc; t.seed = seed;
  t.theta = g_theta; t.theta_partials = g_theta_partials;
  fill<T::K>(t, params, partials);
  v.coords = vcoords; v.loss_partials = vloss_partials; v.n = vn; v.ldc = vldc; v.ldj = vldc; v.seed = 0.f;
  v.theta = g_theta;
  fill<T::K>(v, params, nullptr);
  // a training epoch on its own is the plain training kernel (the same device code as the training half of the combined
  // kernel -- engine.verify_fused compares the two bit for bit -- without the second body's registers: C2 -1 us, C3 -13 us)
  static const bool always_tv = getenv("NDQ_TV_ALWAYS") != nullptr;        // measurement knob
  if (vn == 0 && !pull && !always_tv)
    return launch<T>(coords, ldc, n, params, partials, loss_partials, nullptr, nullptr, ldc, seed, 1, stream);
  const int tb = n > 0 ? fused_blocks<T>(n) : 0, vb = vn > 0 ? fused_blocks<T>(vn) : 0;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(T::tv),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_TRAIN);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  ndq::PullArgs pa{};        // pull prologue (csrc/ndq_tail.h): the launch finishes the previous epoch itself
  if (pull) {
    if (!pull_ok<T>()) return -2;
    pa = *static_cast<const ndq::PullArgs*>(pull);
  }
  hipLaunchKernelGGL(T::tv, dim3(tb + vb), dim3(T::THREADS), tb > 0 ? T::LDS_TRAIN : T::LDS_EVAL,
                     static_cast<hipStream_t>(stream), t, v, tb, pa);
  return (int)hipGetLastError();
}

// loop mode (csrc/ndq_tail.h: LoopArgs): ONE workgroup runs a run of fit()'s launches back to back, state in LDS
template <class T> constexpr bool has_loop() { return !std::is_same_v<std::remove_cv_t<decltype(T::loop)>, std::nullptr_t>; }

template <class T>
int launch_loop(const ndq::real* coords, int ldc, int n, ndq::real seed, const ndq::real* vcoords, int vldc, int vn,
                const void* loop, void* stream) {
  if constexpr (!has_loop<T>()) {
    return -2;
  } else {
    if (!loop || !pull_ok<T>() || n < 0 || vn < 0 ||
        (n > 0 && (!coords || ldc < n || fused_blocks<T>(n) != 1)) ||
        (vn > 0 && (!vcoords || vldc < vn || fused_blocks<T>(vn) != 1)))
      return -2;
    typename T::Args t{}, v{};
    t.coords = coords; t.n = n; t.ldc = ldc; t.ldj = ldc; t.seed = seed; t.theta = g_theta;
    v.coords = vcoords; v.n = vn; v.ldc = vldc; v.ldj = vldc; v.seed = 0.f; v.theta = g_theta;
    static bool attr = false;
    if (!attr) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(T::loop),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_LOOP);
      if (e != hipSuccess) return (int)e;
      attr = true;
    }
    hipLaunchKernelGGL(T::loop, dim3(1), dim3(T::THREADS), T::LDS_LOOP, static_cast<hipStream_t>(stream), t, v,
                       *static_cast<const ndq::LoopArgs*>(loop));
    return (int)hipGetLastError();
  }
}
template <class T> int loop_ok() {
  return has_loop<T>() && pull_ok<T>() && T::LDS_LOOP <= 160 * 1024 ? 1 : 0;
}

}  // namespace

extern "C" int ndq_fused_blocks(int n) { return fused_blocks<Closure>(n); }
extern "C" int ndq_fused_num_params() { return Closure::Cfg::P; }
extern "C" int ndq_fused_num_theta() { return Closure::Pw::NT; }
extern "C" void ndq_fused_bind_theta(const ndq::real* theta, ndq::real* theta_partials) {
  g_theta = theta; g_theta_partials = theta_partials;
}
extern "C" int ndq_fused_num_nets() { return Closure::K; }
extern "C" int ndq_fused_threads() { return Closure::THREADS; }
extern "C" unsigned long ndq_fused_lds_bytes() { return (unsigned long)Closure::LDS_TRAIN; }

#ifdef NDQ_PHASE_TS
extern "C" int ndq_fused_phase_ts(unsigned long long* out) {    // experiments: scripts/phase_ts.py, scripts/phase_ts_group.py
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ndq::ndq_phase_ts), sizeof(unsigned long long) * 256 * 8);
}
extern "C" int ndq_fused_pull_ts(unsigned long long* out) {    // experiments: scripts/archive/pull_ts.py
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ndq::ndq_pull_ts), sizeof(unsigned long long) * 8);
}
extern "C" int ndq_fused_tile_ts(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ndq::ndq_tile_ts), sizeof(unsigned long long) * 48);
}
#endif

// one network: the ndq_fused_launch_fn of include/ndq.h
extern "C" int ndq_fused_launch(const ndq::real* coords, int ldc, int n, const ndq::real* params, ndq::real* partials,
                                ndq::real* loss_partials, ndq::real* funcs, ndq::real* resid, int ldj, ndq::real seed,
                                int train, void* stream) {
  if (Closure::K != 1) return -2;
  const ndq::real* pp[1] = {params};
  ndq::real* qq[1] = {partials};
  return launch<Closure>(coords, ldc, n, pp, partials ? qq : nullptr, loss_partials, funcs, resid, ldj, seed, train, stream);
}

// any number of networks: params / partials are host arrays of device pointers
extern "C" int ndq_fused_launch_multi(const ndq::real* coords, int ldc, int n, const ndq::real* const* params,
                                      ndq::real* const* partials, ndq::real* loss_partials, ndq::real* funcs,
                                      ndq::real* resid, int ldj, ndq::real seed, int train, void* stream) {
  return launch<Closure>(coords, ldc, n, params, partials, loss_partials, funcs, resid, ldj, seed, train, stream);
}

// the ndq_fused_launch_tv_fn of include/ndq.h
extern "C" int ndq_fused_launch_tv(const ndq::real* coords, int ldc, int n, const ndq::real* const* params,
                                   ndq::real* const* partials, ndq::real* loss_partials, ndq::real seed,
                                   const ndq::real* vcoords, int vldc, int vn, ndq::real* vloss_partials, const void* pull,
                                   void* stream) {
  return launch_tv<Closure>(coords, ldc, n, params, partials, loss_partials, seed, vcoords, vldc, vn, vloss_partials, pull, stream);
}
extern "C" int ndq_fused_pull_ok() { return pull_ok<Closure>() ? 1 : 0; }
// the ndq_fused_launch_loop_fn of include/ndq.h
extern "C" int ndq_fused_launch_loop(const ndq::real* coords, int ldc, int n, ndq::real seed, const ndq::real* vcoords,
                                     int vldc, int vn, const void* loop, void* stream) {
  return launch_loop<Closure>(coords, ldc, n, seed, vcoords, vldc, vn, loop, stream);
}
extern "C" int ndq_fused_loop_ok() { return loop_ok<Closure>(); }
