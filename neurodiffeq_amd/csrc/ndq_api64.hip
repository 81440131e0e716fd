// libndq64.so: the stream kernels of ndq_mlp.h compiled for fp64 (NDQ_F64) behind the ndq64_* entry points of include/ndq.h;
// serves fp64 networks (the reference's default precision) through the torch custom ops of autograd_ops.py.  Its own here:
// the built-in kernel table, the fixed-order second-stage sum in double and the fp64 sums + tail launch.  Descriptor dispatch,
// epoch tail, Adam and the fused-step runner are csrc/ndq_api_common.h, shared with libndq.so.
#define NDQ_F64 1
#include "ndq_launch.h"
#include "ndq_tail.h"

namespace ndq {

// X(D, FIRST, MASK2, NB, L, ACT, NOUT): value-only and full second-order stream sets of the default network shapes;
// everything else is compiled on first use as an extension module (codegen.ensure_mlp_kernels(desc, f64=True))
#define NDQ64_CFG_TABLE(X)        \
  X(1, 0, 0, 2, 2, ACT_TANH, 1)   \
  X(1, 1, 1, 2, 2, ACT_TANH, 1)   \
  X(2, 0, 0, 2, 2, ACT_TANH, 1)   \
  X(2, 1, 7, 2, 2, ACT_TANH, 1)   \
  X(1, 0, 0, 2, 2, ACT_SIN, 1)    \
  X(1, 1, 1, 2, 2, ACT_SIN, 1)

#define NDQ64_ENTRY(D, F, M, NB, L, A, O) make_kernels<Cfg<D, F, M, NB, L, A, O, 0>>(),
#define NDQ_API_KERNELS NDQ64_CFG_TABLE(NDQ64_ENTRY)

// (hidden > 64: ONE hidden layer of up to 512 units -- csrc/ndq_wide.h compiled in double, registered extension modules only)
static bool hidden_ok(const ndq_mlp_desc& d) { return d.hidden >= 1 && d.hidden <= (d.layers == 1 ? 512 : 64); }

}  // namespace ndq

#include "ndq_api_common.h"

namespace ndq {

// out[i] = (acc ? out[i] : 0) + scale * sum_r partials[r*len + i], rows in fixed order.  A workgroup owns 64 columns; its
// 16 row groups each add up every 16th row in four independent chains, the 16 group sums are added in index order (the
// layout of ndq_api.hip's column_sum_1024).  An fp64 adjoint launch leaves up to 1 024 partial rows: with one thread per
// column walking all of them this sum took 15 us of a 130 us epoch, and the loss sum (len = 1) was a single thread.
__global__ __launch_bounds__(1024) void reduce_partials64_kernel(const double* __restrict__ part, int nparts, int len,
                                                                 double* __restrict__ out, int accumulate, double scale) {
  __shared__ double sm[16 * 64];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + c;
  // Sixteen rows of a thread at a time as straight-line clamped loads, pinned by one empty asm statement, then added in
  // EXACTLY the order of the loops they replace:
  //     for (r = rg; r + 48 < nparts; r += 64) { s0 += row r; s1 += row r + 16; s2 += row r + 32; s3 += row r + 48; }
  //     for (; r < nparts; r += 16) s0 += row r;
  // which compile to "four loads, s_waitcnt vmcnt(0), four adds, branch" -- one memory round trip per 64 rows, sixteen of them
  // behind an fp64 adjoint launch's 1 024 partial rows (round 5; csrc/ndq_api.hip ColumnRows has the fp32 story).
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  const bool live = i < len;
  const int cc = live ? i : len - 1;
  for (int base = 0; base < nparts; base += 256) {
    double x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = base + rg + 16 * j;
      x[j] = part[(size_t)(r < nparts ? r : nparts - 1) * len + cc];
    }
    NDQ_PIN16(x);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r0 = base + rg + 64 * it;
      if (r0 + 48 < nparts) {
        s0 += x[4 * it]; s1 += x[4 * it + 1]; s2 += x[4 * it + 2]; s3 += x[4 * it + 3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r0 + 16 * k < nparts) s0 += x[4 * it + k];
      }
    }
  }
  sm[rg * 64 + c] = live ? (s0 + s1) + (s2 + s3) : 0.;
  __syncthreads();
  if (rg == 0 && i < len) {
    double s = 0.;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += sm[k * 64 + c];
    s *= scale;
    out[i] = accumulate ? out[i] + s : s;
  }
}

// ---- second-stage sums AND the epoch tail of an fp64 epoch in ONE launch (ndq64_reduce_tail): reduce_tail_multi_kernel of
// csrc/ndq_api.hip in double, blockIdx.y = network.  What it leaves is, bit for bit, what the launches it replaces leave:
// reduce_partials64_kernel over every network's gradient rows and over the loss partials as a one-column matrix (x seed),
// then epoch_tail_kernel<double> per network -- so a training run does not depend on which route served an epoch
// (csrc/ndq_tail.h).  The loss therefore follows the COLUMN order here, not the wave-shuffle tree of the fp32 kernel.

// One 256-row chunk of a thread's rows (base + rg + 16 j, j = 0 .. 15) added to its four chains in EXACTLY
// reduce_partials64_kernel's order (rows past nparts are skipped, not added as zeros: -0.0 stays -0.0).
__device__ __forceinline__ void column_chunk64(const double (&x)[16], int base, int rg, int nparts, double& s0, double& s1,
                                               double& s2, double& s3) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r0 = base + rg + 64 * it;
    if (r0 + 48 < nparts) {
      s0 += x[4 * it]; s1 += x[4 * it + 1]; s2 += x[4 * it + 2]; s3 += x[4 * it + 3];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (r0 + 16 * k < nparts) s0 += x[4 * it + k];
    }
  }
}

struct ReduceTail64Net {
  const double* part;         // [nparts][t.len] gradient partial rows
  double* grad;               // [t.len] their sum
  double* loss_slot;          // [1] the epoch loss (network 0 writes it)
  TailArgsT<double> t;        // p / m / v / len / adam / best_flat / write_scalars
};
struct ReduceTail64Args {
  const double* lpart;        // [nparts] loss partials
  int nparts;
  double lscale;              // seed
  double* loss_hist; int hist_index;
  double* best_loss; int parity;
  ReduceTail64Net net[4];
};
static_assert(sizeof(ReduceTail64Args) <= 4096, "by-value kernel arguments are limited to 4 KiB");

// 64 columns x 16 row groups.  Latency-bound like its fp32 twin: every global load -- this thread's sixteen gradient rows
// and sixteen loss partials, parameter, moments, best loss -- is issued before the first add (the empty asm statements pin
// the raw values: a load that is only selected under "row < nparts" gets sunk into that branch), and there is ONE barrier.
__global__ __launch_bounds__(1024) void reduce_tail64_kernel(ReduceTail64Args a) {
  const ReduceTail64Net& mine = a.net[blockIdx.y];
  const int len = mine.t.len, nparts = a.nparts;
  if ((int)blockIdx.x * 64 >= len) return;                  // a network with fewer parameters than the widest one
  __shared__ double sm[16 * 64];
  __shared__ double sml[16];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + c;
  const bool live = i < len, upd = live && rg == 0;
  const int cc = live ? i : len - 1;
  double x[16], y[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int r = rg + 16 * j, rr = r < nparts ? r : nparts - 1;
    x[j] = mine.part[(size_t)rr * len + cc];
    y[j] = a.lpart[rr];
  }
  double pi = 0., m0 = 0., v0 = 0.;
  if (upd) { pi = mine.t.p[i]; m0 = mine.t.m[i]; v0 = mine.t.v[i]; }
  double best = a.best_loss[a.parity];                      // (uniform address: a scalar load, pinned below like the rest)
  NDQ_PIN16(x);
  NDQ_PIN16(y);
  asm volatile("" : "+s"(best));
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0., l0 = 0., l1 = 0., l2 = 0., l3 = 0.;
  column_chunk64(x, 0, rg, nparts, s0, s1, s2, s3);
  column_chunk64(y, 0, rg, nparts, l0, l1, l2, l3);
  for (int base = 256; base < nparts; base += 256) {        // (more than 256 partial rows: the further chunks, same scheme)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = base + rg + 16 * j, rr = r < nparts ? r : nparts - 1;
      x[j] = mine.part[(size_t)rr * len + cc];
      y[j] = a.lpart[rr];
    }
    NDQ_PIN16(x);
    NDQ_PIN16(y);
    column_chunk64(x, base, rg, nparts, s0, s1, s2, s3);
    column_chunk64(y, base, rg, nparts, l0, l1, l2, l3);
  }
  sm[rg * 64 + c] = live ? (s0 + s1) + (s2 + s3) : 0.;
  if (c == 0) sml[rg] = (l0 + l1) + (l2 + l3);
  __syncthreads();
  double slot = 0.;
#pragma unroll
  for (int k = 0; k < 16; ++k) slot += sml[k];
  slot *= a.lscale;                                         // what ndq64_reduce_partials(len = 1, scale = seed) stores
  double loss = 0.;                                         // ... and epoch_tail_kernel's mean over that ONE slot
  loss += slot;
  loss /= 1.;
  const bool better = (mine.t.best_flat != nullptr) && (loss < best);     // false for NaN, like the reference's comparison
  if (upd) {
    double g = 0.;
#pragma unroll
    for (int k = 0; k < 16; ++k) g += sm[k * 64 + c];
    mine.grad[i] = g;
    if (better) mine.t.best_flat[i] = pi;
    double pn, mi, vi;
    adam_value(mine.t.adam, pi, g, m0, v0, pn, mi, vi);
    mine.t.m[i] = mi;
    mine.t.v[i] = vi;
    mine.t.p[i] = pn;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && mine.t.write_scalars) {
    *mine.loss_slot = slot;
    a.loss_hist[a.hist_index] = loss;
    a.best_loss[a.parity ^ 1] = better ? loss : best;
  }
}

}  // namespace ndq

using namespace ndq;

// the sums + tail launch of validated steps
static int reduce_tail64_launch(const ndq64_fused_step* steps, int n_nets, int adam_step, int hist_index, int parity, void* stream) {
  const ndq64_fused_step& s0 = steps[0];
  ReduceTail64Args a{};
  a.lpart = s0.loss_partials; a.nparts = s0.blocks; a.lscale = s0.seed;
  a.loss_hist = s0.loss_hist; a.hist_index = hist_index; a.best_loss = s0.best_loss; a.parity = parity;
  int max_params = 0;
  for (int k = 0; k < n_nets; ++k) {
    const ndq64_fused_step& s = steps[k];
    ReduceTail64Net& n = a.net[k];
    n.part = s.partials; n.grad = s.grad; n.loss_slot = s0.loss_slot;
    n.t.p = s.params; n.t.g = s.grad; n.t.m = s.adam_m; n.t.v = s.adam_v; n.t.len = s.n_params;
    n.t.adam = adam_consts(s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, adam_step);
    n.t.best_flat = s.best_flat; n.t.write_scalars = k == 0 ? 1 : 0;
    if (s.n_params > max_params) max_params = s.n_params;
  }
  for (int k = n_nets; k < 4; ++k) a.net[k] = a.net[0];
  hipLaunchKernelGGL(reduce_tail64_kernel, dim3((max_params + 63) / 64, n_nets), dim3(1024), 0,
                     static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

extern "C" {

int ndq64_reduce_partials(const double* partials, int nparts, int len, double* out, int accumulate, double scale,
                          void* stream) {
  if (!partials || !out || nparts <= 0 || len <= 0) return NDQ_EINVAL;
  hipLaunchKernelGGL(reduce_partials64_kernel, dim3((len + 63) / 64), dim3(1024), 0, static_cast<hipStream_t>(stream),
                     partials, nparts, len, out, accumulate, scale);
  return (int)hipGetLastError();
}

int ndq64_fused_step_bytes(void) { return (int)sizeof(ndq64_fused_step); }

int ndq64_reduce_tail(const ndq64_fused_step* steps, int n_nets, int adam_step, int hist_index, int parity, void* stream) {
  if (!fused_steps_ok(steps, n_nets, adam_step, hist_index, parity)) return NDQ_EINVAL;
  return reduce_tail64_launch(steps, n_nets, adam_step, hist_index, parity, stream);
}

int ndq64_fused_step_run(const ndq64_fused_step* steps, int n_nets, ndq64_fused_launch_multi_fn launch, const double* coords,
                         int adam_step, int hist_index, int parity, void* stream) {
  return fused_steps_run(steps, n_nets, launch, coords, adam_step, hist_index, parity, stream, &reduce_tail64_launch);
}

}  // extern "C"
