// C-ABI of libndq.so (declared in include/ndq.h).  Its own here: the built-in fp32 kernel table, the second-stage sums, the
// sums + tail launches on every route (single GPU, data parallel, multi-network, fit()), the samplers and the one-shot
// all-reduce.  Descriptor dispatch, epoch tail, Adam and the runner behind ndq_fused_multi_step_run are
// csrc/ndq_api_common.h, shared with libndq64.so.
#include <cstdlib>
#include "ndq_launch.h"
#include "ndq_sample.h"
#include "ndq_oneshot.h"
#include "ndq_tail.h"

extern "C" int ndq_oneshot_allreduce(const void* send, void* recv, size_t count, int dtype, int op, void* comm, void* stream);

namespace ndq {

// ---------------------------------------------------------------------------------------------- kernel table
// X(D, FIRST, MASK2, NB, L, ACT, NOUT, LAP).  Stream sets are closed under "second order needs first order".
// BASELINE configs: C1 (1,1,0,2,2,SIN) | C2 (2,1,0b101,2,2,TANH) | C3 (2,1,0b001,4,3,TANH) | C5 u,v (2,1,0b101,4,3,TANH),
// p (2,1,0,4,3,TANH); value-only variants serve solution evaluation (solvers.py:682-720).
// sigmoid / swish: 1-D and 2-D stream sets at the default width.  d = 3: SolverSpherical's default FCNN(3,1,(32,32)) (solvers_spherical.py) -- diagonal (0b101001), Laplacian-merged and full Hessian.
#ifndef NDQ_CFG_TABLE
#define NDQ_CFG_TABLE(X)      \
  X(1, 0, 0, 2, 2, ACT_SIN, 1, 0)   \
  X(1, 1, 0, 2, 2, ACT_SIN, 1, 0)   \
  X(1, 1, 1, 2, 2, ACT_SIN, 1, 0)   \
  X(1, 0, 0, 2, 2, ACT_TANH, 1, 0)  \
  X(1, 1, 0, 2, 2, ACT_TANH, 1, 0)  \
  X(1, 1, 1, 2, 2, ACT_TANH, 1, 0)  \
  X(2, 0, 0, 2, 2, ACT_TANH, 1, 0)  \
  X(2, 1, 0, 2, 2, ACT_TANH, 1, 0)  \
  X(2, 1, 1, 2, 2, ACT_TANH, 1, 0)  \
  X(2, 1, 5, 2, 2, ACT_TANH, 1, 0)  \
  X(2, 1, 7, 2, 2, ACT_TANH, 1, 0)  \
  X(2, 0, 0, 4, 3, ACT_TANH, 1, 0)  \
  X(2, 1, 0, 4, 3, ACT_TANH, 1, 0)  \
  X(2, 1, 1, 4, 3, ACT_TANH, 1, 0)  \
  X(2, 1, 5, 4, 3, ACT_TANH, 1, 0)  \
  X(1, 0, 0, 2, 2, ACT_TANH, 25, 0) \
  X(1, 1, 1, 2, 2, ACT_TANH, 25, 0) \
  X(2, 1, 5, 2, 2, ACT_TANH, 3, 0)  \
  X(2, 1, 5, 2, 2, ACT_TANH, 1, 1)  \
  X(2, 1, 5, 4, 3, ACT_TANH, 1, 1)  \
  X(3, 0, 0, 2, 2, ACT_TANH, 1, 0)  \
  X(3, 1, 0, 2, 2, ACT_TANH, 1, 0)  \
  X(3, 1, 1, 2, 2, ACT_TANH, 1, 0)  \
  X(3, 1, 41, 2, 2, ACT_TANH, 1, 0) \
  X(3, 1, 41, 2, 2, ACT_TANH, 1, 1) \
  X(3, 1, 63, 2, 2, ACT_TANH, 1, 0)  \
  X(1, 0, 0, 2, 2, ACT_SIGMOID, 1, 0) \
  X(1, 1, 0, 2, 2, ACT_SIGMOID, 1, 0) \
  X(1, 1, 1, 2, 2, ACT_SIGMOID, 1, 0) \
  X(2, 0, 0, 2, 2, ACT_SIGMOID, 1, 0) \
  X(2, 1, 0, 2, 2, ACT_SIGMOID, 1, 0) \
  X(2, 1, 1, 2, 2, ACT_SIGMOID, 1, 0) \
  X(2, 1, 5, 2, 2, ACT_SIGMOID, 1, 0) \
  X(2, 1, 7, 2, 2, ACT_SIGMOID, 1, 0) \
  X(2, 1, 5, 2, 2, ACT_SIGMOID, 1, 1) \
  X(1, 0, 0, 2, 2, ACT_SWISH, 1, 0) \
  X(1, 1, 0, 2, 2, ACT_SWISH, 1, 0) \
  X(1, 1, 1, 2, 2, ACT_SWISH, 1, 0) \
  X(2, 0, 0, 2, 2, ACT_SWISH, 1, 0) \
  X(2, 1, 0, 2, 2, ACT_SWISH, 1, 0) \
  X(2, 1, 1, 2, 2, ACT_SWISH, 1, 0) \
  X(2, 1, 5, 2, 2, ACT_SWISH, 1, 0) \
  X(2, 1, 7, 2, 2, ACT_SWISH, 1, 0) \
  X(2, 1, 5, 2, 2, ACT_SWISH, 1, 1)
#endif

#define NDQ_ENTRY(D, F, M, NB, L, A, O, LP) make_kernels<Cfg<D, F, M, NB, L, A, O, LP>>(),
#define NDQ_API_KERNELS NDQ_CFG_TABLE(NDQ_ENTRY)

static bool hidden_ok(const ndq_mlp_desc& d) { return d.hidden >= 1 && d.hidden <= NDQ_MAX_HIDDEN; }

}  // namespace ndq

#include "ndq_api_common.h"

namespace ndq {

// ---------------------------------------------------------------------------------------------- reduction
// out[i] = (acc ? out[i] : 0) + scale * sum_r partials[r*len + i];  one thread per 4 columns, rows in fixed order,
// 4 independent row chains per thread for memory-level parallelism (combined in a fixed order).
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ part, int nparts, int len,
                                                              float* __restrict__ out, int accumulate, float scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  // fp64 accumulators: a loss over 1 M points arrives as 4 096 block sums of one sign -- a sequential fp32 sum of those
  // measured 5e-6 off at C5; the adds are nothing next to the loads
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  int r = 0;
#pragma unroll 4                      // (16 loads in flight per thread instead of 4: the chains stay in order)
  for (; r + 3 < nparts; r += 4) {
    s0 += (double)part[(size_t)r * len + i];
    s1 += (double)part[(size_t)(r + 1) * len + i];
    s2 += (double)part[(size_t)(r + 2) * len + i];
    s3 += (double)part[(size_t)(r + 3) * len + i];
  }
  for (; r < nparts; ++r) s0 += (double)part[(size_t)r * len + i];
  const float s = (float)(((s0 + s1) + (s2 + s3)) * (double)scale);
  out[i] = accumulate ? out[i] + s : s;
}

// both second-stage sums of one batch in one launch: blocks [0, gridDim.x-1) reduce 64 gradient columns each with 4
// row groups per column (fixed order: row groups sequentially, then the 4 group sums in order); the last block sums
// the loss partials (wave shuffle tree + the 4 waves in order).
struct Reduce2Args {
  const float* part; int nparts, len; float* out; int accumulate;
  const float* lpart; int nlparts; float* lout; float lscale;
};

// ---- the per-thread part of a column sum with EVERY load in flight before the first add (round 5).
// The loops "for (r = rg; r + 48 < nparts; r += 64) { s0 += ..; s1 += ..; s2 += ..; s3 += ..; }" below compile to four
// loads, s_waitcnt vmcnt(0), four adds, branch: with the closure kernel's 256 partial rows that is FOUR dependent round
// trips to memory written by the previous launch (i.e. HBM / another XCD's L2, ~0.7 us each) inside a kernel whose whole
// duration is 5 us -- and the loss-partial loop in front of it and the parameter / moment loads behind it add three more.
// ColumnRows issues the first 16 rows of a thread (rows rg, rg + 16, ..., rg + 240: all of them for nparts <= 256, the
// closure kernels' maximum) as straight-line clamped loads; finish() adds them in EXACTLY the order of the loops it
// replaces (rows beyond nparts contribute +0.0f), then walks any further rows the old way.
struct ColumnRows {
  float v[16];
  // UNCONDITIONAL clamped loads: a load whose value is only selected under "row < nparts" gets sunk into that branch by the
  // compiler (one load + s_waitcnt per row -- seen in the ISA), so the raw values are pinned by one empty asm statement in
  // finish(), where all sixteen must be live at once; the selection happens after it.
  __device__ __forceinline__ void issue(const float* __restrict__ part, int nparts, int len, int col, int rg) {
    const int cc = col < len ? col : len - 1;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = rg + 16 * j;
      v[j] = part[(size_t)(r < nparts ? r : nparts - 1) * len + cc];
    }
  }
  // (s0 + s1) + (s2 + s3) of: for (r = rg; r + 48 < nparts; r += 64) {s0 += row r; s1 += row r+16; s2 += row r+32; s3 += row r+48;}
  //                           for (; r < nparts; r += 16) s0 += row r;
  __device__ __forceinline__ float finish(const float* __restrict__ part, int nparts, int len, int col, int rg) const {
    float x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = v[j];
    NDQ_PIN16(x);
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = (rg + 16 * j < nparts && col < len) ? x[j] : 0.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      if (rg + 64 * it + 48 < nparts) { s0 += x[4 * it]; s1 += x[4 * it + 1]; s2 += x[4 * it + 2]; s3 += x[4 * it + 3]; }
      else { s0 += x[4 * it]; s0 += x[4 * it + 1]; s0 += x[4 * it + 2]; s0 += x[4 * it + 3]; }
    }
    if (nparts > 256 && col < len) {                     // (larger partial sets: the remaining rows, same scheme)
      int r = rg + 256;
      for (; r + 48 < nparts; r += 64) {
        s0 += part[(size_t)r * len + col];
        s1 += part[(size_t)(r + 16) * len + col];
        s2 += part[(size_t)(r + 32) * len + col];
        s3 += part[(size_t)(r + 48) * len + col];
      }
      for (; r < nparts; r += 16) s0 += part[(size_t)r * len + col];
    }
    return (s0 + s1) + (s2 + s3);
  }
};

// column sums of partials[nparts][len] for the 64 columns of this workgroup: 16 row groups x 64 columns, every thread
// keeps 4 independent chains (rows rg, rg+16, ...), then the 16 group sums are added in fixed order.  Returns the
// column total in the threads of row group 0 (valid where col < len).
__device__ __forceinline__ float column_sum_1024(const float* __restrict__ part, int nparts, int len, int col, int rg,
                                                 float* sm /* [16*64] */) {
  ColumnRows rows;
  rows.issue(part, nparts, len, col, rg);
  sm[rg * 64 + (threadIdx.x & 63)] = rows.finish(part, nparts, len, col, rg);
  __syncthreads();
  float s = 0.f;
  if (rg == 0) {
#pragma unroll
    for (int g = 0; g < 16; ++g) s += sm[g * 64 + (threadIdx.x & 63)];
  }
  return s;
}

// sum of n floats by one 1024-thread workgroup, fixed order; result valid in thread 0
__device__ __forceinline__ float block_sum_1024(const float* __restrict__ v, int n, float* sm16) {
  float x = 0.f;
  for (int r = threadIdx.x; r < n; r += 1024) x += v[r];
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
  if ((threadIdx.x & 63) == 0) sm16[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int w = 0; w < 16; ++w) s += sm16[w];
  return s;
}

__global__ __launch_bounds__(1024) void reduce_grad_loss_kernel(Reduce2Args a) {
  __shared__ float sm[16 * 64];
  if (blockIdx.x + 1 < gridDim.x) {
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + c;
    const float s = column_sum_1024(a.part, a.nparts, a.len, i, rg, sm);
    if (rg == 0 && i < a.len) a.out[i] = a.accumulate ? a.out[i] + s : s;
  } else {
    const float s = block_sum_1024(a.lpart, a.nlparts, sm);
    if (threadIdx.x == 0) *a.lout = s * a.lscale;
  }
}

// ---------------------------------------------------------------------------------------------- epoch tail
// (the tail of an epoch whose sums are done already, ndq_epoch_tail: ndq_tail.h's kernel behind ndq_api_common.h's entry point)
using TailArgs = ndq::TailArgsT<float>;

// second-stage sums AND the epoch tail in one launch (single batch per epoch, no all-reduce in between): every
// workgroup first adds up the loss partials itself (nlparts <= a few hundred floats), then reduces its 64 gradient
// columns and applies best-snapshot + Adam to them.
// loss of a validation batch evaluated by the same closure launch (ndq_fused_fit_run): block partials -> one scalar
struct ValidArgs {
  const float* part; int nparts; float scale; float* hist; int index;
  int best_on_valid;          // 1: the best-network snapshot follows the validation loss instead of the training loss
};
struct ReduceTailArgs {
  Reduce2Args r;
  TailArgs t;
  int tail_blocks;            // workgroups [tail_blocks, gridDim.x) draw the next batch (smp), if any
  ndq::SampleArgs smp;
  ValidArgs v;                // v.part == nullptr: no validation loss in this launch
};
// TC: gradient columns per workgroup (TC x 16 threads).  64 (1024 threads) is the layout of rounds 2 - 5; narrower workgroups
// spread the 1.2 MB of partial rows over more CUs / XCDs and launch faster (NDQ_TAIL_COLS; profiles/r06p_tail_cols_ab.txt).  The
// per-column order (16 row groups of 16 rows) and the loss order (64-lane tree per wave, waves in index order) do not depend on
// TC as long as the loss partials fit one per thread -- the launchers fall back to 64 columns otherwise.
#ifndef NDQ_TAIL_COLS
#define NDQ_TAIL_COLS 64
#endif
template <int TC>
__device__ __forceinline__ void reduce_tail_body(const ReduceTailArgs& a) {
  // Latency-bound (19 workgroups at C2): every global load -- loss partials, this thread's rows of the gradient
  // partials, the parameter / moment values it will update -- is issued before the first reduction step, and there is
  // ONE barrier.  Summation orders are fixed (per-thread chains, then LDS slots added in index order).
  constexpr int TT = TC * 16, WAVES = TT / 64;
  __shared__ float sm[16 * TC];
  __shared__ float smw[16];
  __shared__ float smv[16];
  const int tid = threadIdx.x, c = tid % TC, rg = tid / TC, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * TC + c;
  const bool col = i < a.r.len;
  const bool has_valid = a.v.part != nullptr;           // uniform over the launch
  const bool has_train = a.r.nparts > 0;                // false: stand-alone validation epoch (no sums, no Adam)
  // ---- issue: gradient-partial rows, first loss / validation partial, parameter + moments, best loss -- straight-line
  // (see ColumnRows: the loops these replace serialised seven memory round trips)
  ColumnRows rows;
  if (has_train) rows.issue(a.r.part, a.r.nparts, a.r.len, i, rg);
  const float lp0 = tid < a.r.nlparts ? a.r.lpart[tid] : 0.f;
  const float vp0 = has_valid && tid < a.v.nparts ? a.v.part[tid] : 0.f;
  const bool upd = (rg == 0) && col;
  const float* p_in = a.t.p_in ? a.t.p_in : a.t.p;
  const float* m_in = a.t.m_in ? a.t.m_in : a.t.m;
  const float* v_in = a.t.v_in ? a.t.v_in : a.t.v;
  float pi = 0.f, m0 = 0.f, v0 = 0.f;
  if (upd) {
    pi = p_in[i];
    if (has_train || a.t.p_in) { m0 = m_in[i]; v0 = v_in[i]; }
  }
  const float best = a.t.best_loss[a.t.parity];
  // ---- use
  float lp = lp0, vp = vp0;
  for (int r = tid + TT; r < a.r.nlparts; r += TT) lp += a.r.lpart[r];       // (TC < 64: never taken, see the launchers)
  if (has_valid)
    for (int r = tid + TT; r < a.v.nparts; r += TT) vp += a.v.part[r];
  const float colsum = has_train ? rows.finish(a.r.part, a.r.nparts, a.r.len, i, rg) : 0.f;
  for (int off = 32; off > 0; off >>= 1) lp += __shfl_down(lp, off);
  if (has_valid)
    for (int off = 32; off > 0; off >>= 1) vp += __shfl_down(vp, off);
  if (lane == 0) { smw[wave] = lp; smv[wave] = vp; }
  sm[rg * TC + c] = colsum;
  __syncthreads();
  float loss = 0.f, vloss = 0.f;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) loss += smw[w];      // (the 16 - WAVES waves a 1024-thread workgroup would add hold exact zeros)
  loss *= a.r.lscale;
  if (has_valid) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) vloss += smv[w];
    vloss *= a.v.scale;
  }
  // what the snapshot follows: the validation loss of the parameters this epoch starts from (fit() with validation
  // epochs), else the training loss (solvers.py:414-415: n_batches_valid = 0)
  const bool on_valid = has_valid && a.v.best_on_valid != 0;
  const float cmp = on_valid ? vloss : loss;
  const bool better = (a.t.best_flat != nullptr) && (on_valid || has_train) && (cmp < best);
  if (upd) {
    if (better) a.t.best_flat[i] = pi;
    if (has_train) {
      float g = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) g += sm[k * TC + c];
      a.r.out[i] = g;
      float pn, mi, vi;
      ndq::adam_value(a.t.adam, pi, g, m0, v0, pn, mi, vi);
      a.t.m[i] = mi;
      a.t.v[i] = vi;
      a.t.p[i] = pn;
    } else if (a.t.p_in) {             // a validation-only tail that also brings the parameters / moments home
      a.t.p[i] = pi; a.t.m[i] = m0; a.t.v[i] = v0;
    }
  }
  if (blockIdx.x == 0 && tid == 0 && a.t.write_scalars) {
    if (has_train) {
      *a.r.lout = loss;
      a.t.loss_hist[a.t.hist_index] = loss;
    }
    if (has_valid) a.v.hist[a.v.index] = vloss;
    a.t.best_loss[a.t.parity ^ 1] = better ? cmp : best;
  }
}
__global__ __launch_bounds__(1024) void reduce_tail_kernel(ReduceTailArgs a) {
  if ((int)blockIdx.x >= a.tail_blocks) {                  // prefetch of the next batch (ndq_fused_step.next_sampler)
    ndq::sample_point_store(a.smp, ((int)blockIdx.x - a.tail_blocks) * 1024 + (int)threadIdx.x);
    return;
  }
  reduce_tail_body<64>(a);
}

// Data parallel with the one-shot exchange (ndq_oneshot.h): the SAME launch also carries the all-reduce.  Every
// workgroup reduces its 64 gradient columns (and the loss) locally, pushes that slice [64 gradients | loss] into every
// rank's inbox, waits for the slices of all ranks, adds them in rank order and applies best-snapshot + Adam to its
// columns -- a data-parallel training epoch is two launches, like a single-GPU one.  Inbox slice of workgroup b:
// floats [65 b, 65 b + 65) of the parity's per-rank vector; flag (parity, source rank, b).
__global__ __launch_bounds__(1024) void reduce_tail_dp_kernel(ReduceTailArgs a, ndq::OneshotDev c, unsigned step) {
  __shared__ float sm[16 * 64];
  __shared__ float smw[16];
  __shared__ float sloss;
  __shared__ int timed_out;
  if (threadIdx.x == 0) timed_out = 0;
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6, blk = blockIdx.x;
  const int i = blk * 64 + col;
  const bool incol = i < a.r.len;
  ColumnRows rows;                                        // (every load in flight before the first add: see ColumnRows)
  rows.issue(a.r.part, a.r.nparts, a.r.len, i, rg);
  const float lp0 = tid < a.r.nlparts ? a.r.lpart[tid] : 0.f;
  const bool upd = (rg == 0) && incol;
  float pi = 0.f, m0 = 0.f, v0 = 0.f;
  if (upd) { pi = a.t.p[i]; m0 = a.t.m[i]; v0 = a.t.v[i]; }
  const float best = a.t.best_loss[a.t.parity];
  float lp = lp0;
  for (int r = tid + 1024; r < a.r.nlparts; r += 1024) lp += a.r.lpart[r];
  const float colsum = rows.finish(a.r.part, a.r.nparts, a.r.len, i, rg);
  for (int off = 32; off > 0; off >>= 1) lp += __shfl_down(lp, off);
  if (col == 0) smw[rg] = lp;
  sm[rg * 64 + col] = colsum;
  __syncthreads();
  // ---- push this workgroup's slice [64 local column sums | local loss] to every rank
  const int parity = step & 1u;
  const size_t slot = ((size_t)parity * c.world + c.rank) * c.max_len + (size_t)blk * 65;
  if (rg == 0) {
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) g += sm[k * 64 + col];
    for (int q = 0; q < c.world; ++q)
      __hip_atomic_store(c.inbox[q] + slot + col, incol ? g : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (col == 0) {
      float loss = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) loss += smw[w];
      loss *= a.r.lscale;
      for (int q = 0; q < c.world; ++q)
        __hip_atomic_store(c.inbox[q] + slot + 64, loss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __threadfence_system();
  __syncthreads();
  if (tid < c.world) {
    unsigned* f = c.flags[tid] + ((size_t)parity * c.world + c.rank) * c.max_blocks + blk;
    __hip_atomic_store(f, step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned* mine = c.flags[c.rank] + ((size_t)parity * c.world + tid) * c.max_blocks + blk;
    if (!ndq::oneshot_wait(mine, step, c.spin_limit, c.status)) timed_out = 1;
  }
  __syncthreads();
  // a peer's slice never arrived (counted in the status word, which the solver turns into an error at its next history
  // flush): no parameter is updated with a stale inbox, and the epoch's loss is NaN
  const bool bad = timed_out != 0;
  // ---- fixed-order sum over the ranks, then the tail on the global values
  const float* inbox = c.inbox[c.rank] + (size_t)parity * c.world * c.max_len + (size_t)blk * 65;
  if (tid == 0) {
    float loss = 0.f;
    for (int q = 0; q < c.world; ++q)
      loss += __hip_atomic_load(inbox + (size_t)q * c.max_len + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    sloss = bad ? __builtin_nanf("") : loss;
  }
  __syncthreads();
  const float loss = sloss;
  const bool better = (a.t.best_flat != nullptr) && (loss < best);
  if (upd && !bad) {
    float g = 0.f;
    for (int q = 0; q < c.world; ++q)
      g += __hip_atomic_load(inbox + (size_t)q * c.max_len + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    a.r.out[i] = g;
    if (better) a.t.best_flat[i] = pi;
    float pn, mi, vi;
    ndq::adam_value(a.t.adam, pi, g, m0, v0, pn, mi, vi);
    a.t.m[i] = mi;
    a.t.v[i] = vi;
    a.t.p[i] = pn;
  }
  if (blk == 0 && tid == 0 && a.t.write_scalars) {
    *a.r.lout = loss;
    a.t.loss_hist[a.t.hist_index] = loss;
    a.t.best_loss[a.t.parity ^ 1] = better ? loss : best;
  }
}

// the same for the 2..4 networks behind one multi-network closure launch, in ONE launch: blockIdx.y = network
struct ReduceTailMultiArgs {
  ReduceTailArgs net[4];
};
template <int TC>
__global__ __launch_bounds__(TC * 16) void reduce_tail_multi_kernel(ReduceTailMultiArgs a) {
  const ReduceTailArgs& mine = a.net[blockIdx.y];
  if ((int)blockIdx.x * TC >= mine.r.len) return;          // networks of one shape: never taken, kept for safety
  reduce_tail_body<TC>(mine);
}
// the sums / tail launch of all networks of a system: narrow workgroups where every loss partial has a thread of its own
static int launch_tail_multi(ReduceTailMultiArgs& a, int max_params, int n_nets, int max_lparts, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int k = n_nets; k < 4; ++k) a.net[k] = a.net[0];
  if (NDQ_TAIL_COLS < 64 && max_lparts <= NDQ_TAIL_COLS * 16)
    hipLaunchKernelGGL(reduce_tail_multi_kernel<NDQ_TAIL_COLS>, dim3((max_params + NDQ_TAIL_COLS - 1) / NDQ_TAIL_COLS, n_nets),
                       dim3(NDQ_TAIL_COLS * 16), 0, st, a);
  else
    hipLaunchKernelGGL(reduce_tail_multi_kernel<64>, dim3((max_params + 63) / 64, n_nets), dim3(1024), 0, st, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- trainable scalars
// The scalars of an inverse problem (include/ndq.h: ndq_theta_step) as one more row of the multi-network sums + tail launch:
// workgroup (0, n_nets) reduces theta_partials [nparts][nt] and steps the scalars; the other workgroups of that row leave at
// once.  Per-scalar Adam constants travel as kernel arguments (host: adam_consts from every scalar's own step count).
constexpr int kThetaMax = NDQ_THETA_MAX;
constexpr int kThetaStage = 2048;       // floats of partial rows one workgroup stages in LDS (more: the sum reads global memory)
struct ThetaArgs {
  int nt, nparts; unsigned frozen;
  const float* part; float* theta; float* gtheta; float* m; float* v;
  float lr[kThetaMax], b1[kThetaMax], b2[kThetaMax], eps[kThetaMax], wd[kThetaMax], bc1[kThetaMax], bc2s[kThetaMax];
};
// TT threads.  Latency-bound like the rest of the launch (everything read here was written by the closure launch): the partial
// rows are ONE contiguous block of nparts * nt floats, which all threads fetch side by side -- kThetaStage / TT straight-line
// clamped loads each -- next to the value and the moments of the scalar a thread owns; only then the first add.  Thread j < nt
// then adds column j out of LDS in the order of reduce_partials_kernel (fp64 accumulators, chains over rows r, r + 1, r + 2,
// r + 3 (+ 4 k), (s0 + s1) + (s2 + s3), scale 1): the same additions, the same bits.  No atomics; nothing depends on the grid.
template <int TT>
__device__ __forceinline__ void theta_row(const ThetaArgs& a) {
  constexpr int PER = kThetaStage / TT;
  static_assert(PER >= 1 && PER * TT == kThetaStage, "the workgroup fills the staging block exactly");
  __shared__ float st[kThetaStage];
  const int tid = threadIdx.x, nt = a.nt, nparts = a.nparts, total = nt * nparts;
  const bool staged = total <= kThetaStage;              // uniform
  float x[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int e = tid + q * TT;
    x[q] = a.part[e < total ? e : total - 1];
  }
  const bool mine = tid < nt;
  const int j = mine ? tid : 0;
  const float p0 = a.theta[j], m0 = a.m[j], v0 = a.v[j];
#pragma unroll
  for (int q = 0; q < PER; ++q) st[tid + q * TT] = x[q];
  __syncthreads();
  if (!mine) return;
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  int r = 0;
  if (staged) {
    for (; r + 3 < nparts; r += 4) {
      s0 += (double)st[r * nt + j];
      s1 += (double)st[(r + 1) * nt + j];
      s2 += (double)st[(r + 2) * nt + j];
      s3 += (double)st[(r + 3) * nt + j];
    }
    for (; r < nparts; ++r) s0 += (double)st[r * nt + j];
  } else {
#pragma unroll 4
    for (; r + 3 < nparts; r += 4) {
      s0 += (double)a.part[(size_t)r * nt + j];
      s1 += (double)a.part[(size_t)(r + 1) * nt + j];
      s2 += (double)a.part[(size_t)(r + 2) * nt + j];
      s3 += (double)a.part[(size_t)(r + 3) * nt + j];
    }
    for (; r < nparts; ++r) s0 += (double)a.part[(size_t)r * nt + j];
  }
  const float g = (float)(((s0 + s1) + (s2 + s3)) * (double)1.0f);
  a.gtheta[j] = g;
  if ((a.frozen >> j) & 1u) return;
  ndq::AdamConsts c{};
#pragma unroll
  for (int k = 0; k < kThetaMax; ++k)                    // static indices into the kernel arguments, selected per lane
    if (k == j) c = ndq::AdamConsts{a.lr[k], a.b1[k], a.b2[k], a.eps[k], a.wd[k], a.bc1[k], a.bc2s[k]};
  float pn, mi, vi;
  ndq::adam_value(c, p0, g, m0, v0, pn, mi, vi);
  a.m[j] = mi;
  a.v[j] = vi;
  a.theta[j] = pn;
}
struct ReduceTailThetaArgs {
  ReduceTailMultiArgs nets;
  ThetaArgs th;
  int n_nets;
};
static_assert(sizeof(ReduceTailThetaArgs) <= 4096, "kernel arguments of the sums + tail launch with scalars");
template <int TC>
__global__ __launch_bounds__(TC * 16) void reduce_tail_theta_kernel(ReduceTailThetaArgs a) {
  if ((int)blockIdx.y == a.n_nets) {
    if (blockIdx.x == 0) theta_row<TC * 16>(a.th);
    return;
  }
  const ReduceTailArgs& mine = a.nets.net[blockIdx.y];
  if ((int)blockIdx.x * TC >= mine.r.len) return;
  reduce_tail_body<TC>(mine);
}
// launch_tail_multi with the scalars' row behind the networks' (the same workgroup shape for the same sizes)
static int launch_tail_theta(ReduceTailThetaArgs& a, int max_params, int n_nets, int max_lparts, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int k = n_nets; k < 4; ++k) a.nets.net[k] = a.nets.net[0];
  a.n_nets = n_nets;
  if (NDQ_TAIL_COLS < 64 && max_lparts <= NDQ_TAIL_COLS * 16)
    hipLaunchKernelGGL(reduce_tail_theta_kernel<NDQ_TAIL_COLS>, dim3((max_params + NDQ_TAIL_COLS - 1) / NDQ_TAIL_COLS, n_nets + 1),
                       dim3(NDQ_TAIL_COLS * 16), 0, st, a);
  else
    hipLaunchKernelGGL(reduce_tail_theta_kernel<64>, dim3((max_params + 63) / 64, n_nets + 1), dim3(1024), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace ndq

using namespace ndq;

extern "C" {

int ndq_reduce_partials(const float* partials, int nparts, int len, float* out, int accumulate, float scale,
                        void* stream) {
  if (!partials || !out || nparts <= 0 || len <= 0) return NDQ_EINVAL;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((len + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     partials, nparts, len, out, accumulate, scale);
  return (int)hipGetLastError();
}

int ndq_reduce_grad_loss(const float* partials, int nparts, int len, float* out, int accumulate,
                         const float* loss_partials, int n_loss_parts, float* loss_out, float loss_scale, void* stream) {
  if (!partials || !out || !loss_partials || !loss_out || nparts <= 0 || len <= 0 || n_loss_parts <= 0) return NDQ_EINVAL;
  Reduce2Args a{partials, nparts, len, out, accumulate, loss_partials, n_loss_parts, loss_out, loss_scale};
  hipLaunchKernelGGL(reduce_grad_loss_kernel, dim3((len + 63) / 64 + 1), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

}  // extern "C"

// The arguments of ONE sums + tail launch for network `s` -- every route (single GPU, data parallel, multi-network,
// fit() in its three modes) builds them here.  `s0`: the network whose seed / loss_hist / best_loss count (net[0] of a
// system).  part / lpart: the gradient and loss partial rows, nparts of each; nparts = 0: no training part (no sums, no
// Adam: a validation tail).  adam_step <= 0: no optimiser step.  best_flat: where to snapshot the pre-update parameters
// when the tracked loss improved (nullptr: this launch only hands the best value on).  v: the validation loss this launch
// records, if any.  p_in / m_in / v_in: the state the epoch started from when that is not s.params / adam_m / adam_v.
static ReduceTailArgs reduce_tail_args(const ndq_fused_step& s, const ndq_fused_step& s0, const float* part, const float* lpart,
                                       int nparts, int adam_step, int hist_index, int parity, int write_scalars,
                                       float* best_flat, const ValidArgs& v = ValidArgs{}, const float* p_in = nullptr,
                                       const float* m_in = nullptr, const float* v_in = nullptr) {
  ReduceTailArgs a{};
  a.r = Reduce2Args{part, nparts, s.n_params, s.grad, 0, lpart, nparts, s.loss_slot, s0.seed};
  a.t.p = s.params; a.t.g = s.grad; a.t.m = s.adam_m; a.t.v = s.adam_v; a.t.len = s.n_params;
  a.t.adam = adam_consts(s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, adam_step);
  a.t.p_in = p_in; a.t.m_in = m_in; a.t.v_in = v_in;
  a.t.loss_slots = s.loss_slot; a.t.nb = 1; a.t.loss_hist = s0.loss_hist; a.t.hist_index = hist_index;
  a.t.best_loss = s0.best_loss; a.t.parity = parity; a.t.best_flat = best_flat; a.t.write_scalars = write_scalars;
  a.tail_blocks = 0x7fffffff;
  a.v = v;
  return a;
}

// the sums + tail launch of validated steps: all networks behind one multi-network closure launch (fused_steps_run)
static int reduce_tail_multi(const ndq_fused_step* steps, int n_nets, int adam_step, int hist_index, int parity, void* stream) {
  const ndq_fused_step& s0 = steps[0];
  ReduceTailMultiArgs a{};
  int max_params = 0;
  for (int k = 0; k < n_nets; ++k) {
    a.net[k] = reduce_tail_args(steps[k], s0, steps[k].partials, s0.loss_partials, s0.blocks, adam_step, hist_index, parity,
                                k == 0 ? 1 : 0, steps[k].best_flat);
    if (steps[k].n_params > max_params) max_params = steps[k].n_params;
  }
  return launch_tail_multi(a, max_params, n_nets, s0.blocks, stream);
}

extern "C" {

int ndq_fused_step_run(const ndq_fused_step* s, const float* coords, int adam_step, int hist_index, int parity,
                       void* stream) {
  if (!s || !s->launch || !coords) return NDQ_EINVAL;
  int rc = s->launch(coords, s->ldc, s->n, s->params, s->partials, s->loss_partials, nullptr, nullptr, s->ldj, s->seed,
                     1, stream);
  if (rc) return rc;
  if (!s->adam_m)
    return ndq_reduce_grad_loss(s->partials, s->blocks, s->n_params, s->grad, 0, s->loss_partials, s->blocks,
                                s->loss_slot, s->seed, stream);
  if (adam_step <= 0 || hist_index < 0 || (parity != 0 && parity != 1) || !s->loss_hist || !s->best_loss) return NDQ_EINVAL;
  const bool oneshot = s->allreduce == reinterpret_cast<ndq_allreduce_fn>(&ndq_oneshot_allreduce) && s->comm &&
                       ((s->n_params + 63) / 64) * 65 <= static_cast<ndq::Oneshot*>(s->comm)->dev.max_len &&
                       (s->n_params + 63) / 64 <= static_cast<ndq::Oneshot*>(s->comm)->dev.max_blocks;
  if (s->allreduce && !oneshot) {
    // data parallel: local second-stage sums -> ONE all-reduce of [grad | loss] -> tail on the reduced vector
    if (s->loss_slot != s->grad + s->n_params) return NDQ_EINVAL;
    rc = ndq_reduce_grad_loss(s->partials, s->blocks, s->n_params, s->grad, 0, s->loss_partials, s->blocks, s->loss_slot,
                              s->seed, stream);
    if (rc) return rc;
    rc = s->allreduce(s->grad, s->grad, (size_t)s->n_params + 1, /*ncclFloat32*/ 7, /*ncclSum*/ 0, s->comm, stream);
    if (rc) return 1000 + rc;   // ncclResult_t, offset so that it cannot be taken for a hipError_t
    return ndq_epoch_tail(s->params, s->grad, s->adam_m, s->adam_v, s->n_params, s->lr, s->beta1, s->beta2, s->eps,
                          s->weight_decay, adam_step, s->loss_slot, 1, s->loss_hist, hist_index, s->best_loss, parity,
                          s->best_flat, 1, stream);
  }
  ReduceTailArgs a = reduce_tail_args(*s, *s, s->partials, s->loss_partials, s->blocks, adam_step, hist_index, parity, 1,
                                      s->best_flat);
  int blocks = (s->n_params + 63) / 64;
  if (oneshot) {
    // data parallel over the one-shot exchange: local sums + exchange + tail in ONE launch (reduce_tail_dp_kernel)
    ndq::Oneshot* c = static_cast<ndq::Oneshot*>(s->comm);
    const unsigned step = ++c->step;
    hipLaunchKernelGGL(reduce_tail_dp_kernel, dim3(blocks), dim3(1024), 0, static_cast<hipStream_t>(stream), a, c->dev, step);
    return (int)hipGetLastError();
  }
  a.tail_blocks = blocks;
  if (s->next_sampler) {
    rc = ndq::fill_sample_args(a.smp, s->next_sampler, s->next_seed, s->next_draw, s->next_stream, s->next_coords,
                               s->next_ldc);
    if (rc) return rc;
    blocks += (a.smp.total + 1023) / 1024;
  }
  hipLaunchKernelGGL(reduce_tail_kernel, dim3(blocks), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

int ndq_fused_multi_step_run(const ndq_fused_step* steps, int n_nets, ndq_fused_launch_multi_fn launch,
                             const float* coords, int adam_step, int hist_index, int parity, void* stream) {
  return fused_steps_run(steps, n_nets, launch, coords, adam_step, hist_index, parity, stream, &reduce_tail_multi);
}

}  // extern "C"

// ---- the same epoch with the scalars of an inverse problem in the sums + tail launch (ndq_theta_step)
static bool theta_step_ok(const ndq_theta_step* th) {
  if (!th || th->n_theta < 1 || th->n_theta > NDQ_THETA_MAX || !th->theta || !th->partials || !th->gtheta || !th->adam_m ||
      !th->adam_v)
    return false;
  for (int j = 0; j < th->n_theta; ++j)
    if (!((th->frozen >> j) & 1u) && th->step[j] <= 0) return false;
  return true;
}
static ndq::AdamConsts theta_consts(const ndq_theta_step& th, int j) {
  return adam_consts(th.lr[j], th.beta1[j], th.beta2[j], th.eps[j], th.weight_decay[j], th.step[j]);
}
// validated steps + scalars -> ONE launch (reduce_tail_theta_kernel: blockIdx.y = network, last row = the scalars)
static int reduce_tail_theta(const ndq_fused_step* steps, int n_nets, const ndq_theta_step& th, int adam_step, int hist_index,
                             int parity, void* stream) {
  const ndq_fused_step& s0 = steps[0];
  ReduceTailThetaArgs a{};
  int max_params = 0;
  for (int k = 0; k < n_nets; ++k) {
    a.nets.net[k] = reduce_tail_args(steps[k], s0, steps[k].partials, s0.loss_partials, s0.blocks, adam_step, hist_index, parity,
                                     k == 0 ? 1 : 0, steps[k].best_flat);
    if (steps[k].n_params > max_params) max_params = steps[k].n_params;
  }
  ThetaArgs& t = a.th;
  t.nt = th.n_theta; t.nparts = s0.blocks; t.frozen = th.frozen;
  t.part = th.partials; t.theta = th.theta; t.gtheta = th.gtheta; t.m = th.adam_m; t.v = th.adam_v;
  for (int j = 0; j < th.n_theta; ++j) {
    const ndq::AdamConsts c = theta_consts(th, j);
    t.lr[j] = c.lr; t.b1[j] = c.b1; t.b2[j] = c.b2; t.eps[j] = c.eps; t.wd[j] = c.wd; t.bc1[j] = c.bc1; t.bc2s[j] = c.bc2s;
  }
  return launch_tail_theta(a, max_params, n_nets, s0.blocks, stream);
}

extern "C" {

int ndq_theta_step_bytes(void) { return (int)sizeof(ndq_theta_step); }

int ndq_theta_step_consts(const ndq_theta_step* th, int j, float* out7) {
  if (!th || !out7 || j < 0 || j >= th->n_theta || th->n_theta > NDQ_THETA_MAX) return NDQ_EINVAL;
  const ndq::AdamConsts c = theta_consts(*th, j);
  out7[0] = c.lr; out7[1] = c.b1; out7[2] = c.b2; out7[3] = c.eps; out7[4] = c.wd; out7[5] = c.bc1; out7[6] = c.bc2s;
  return 0;
}

int ndq_fused_theta_step_run(const ndq_fused_step* s, const ndq_theta_step* th, const float* coords, int adam_step,
                             int hist_index, int parity, void* stream) {
  if (!s || !s->launch || !coords || !theta_step_ok(th) || !fused_steps_ok(s, 1, adam_step, hist_index, parity)) return NDQ_EINVAL;
  int rc = s->launch(coords, s->ldc, s->n, s->params, s->partials, s->loss_partials, nullptr, nullptr, s->ldj, s->seed, 1,
                     stream);
  if (rc) return rc;
  return reduce_tail_theta(s, 1, *th, adam_step, hist_index, parity, stream);
}

int ndq_fused_theta_multi_step_run(const ndq_fused_step* steps, int n_nets, ndq_fused_launch_multi_fn launch,
                                   const ndq_theta_step* th, const float* coords, int adam_step, int hist_index, int parity,
                                   void* stream) {
  if (!launch || !coords || !theta_step_ok(th) || !fused_steps_ok(steps, n_nets, adam_step, hist_index, parity)) return NDQ_EINVAL;
  const ndq_fused_step& s0 = steps[0];
  const float* params[4];
  float* partials[4];
  for (int k = 0; k < n_nets; ++k) {
    params[k] = steps[k].params;
    partials[k] = steps[k].partials;
  }
  int rc = launch(coords, s0.ldc, s0.n, params, partials, s0.loss_partials, nullptr, nullptr, s0.ldj, s0.seed, 1, stream);
  if (rc) return rc;
  return reduce_tail_theta(steps, n_nets, *th, adam_step, hist_index, parity, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- fit()
// ndq_fused_fit_run: see include/ndq.h.  One validated call, shared by its three routes.  Buffer set 0 is the primary
// state (net[k].params / adam_m / adam_v / partials, loss partials), set 1 the alt_* members pull and loop mode need.
struct FitCall {
  const ndq_fused_fit* f;
  int n_epochs; const float* const* train_coords;
  int adam_step, hist_index, valid_index;        // of the call's first epoch
  void* stream;
  bool valid;
  int max_params, max_lparts;
  float* P[2][4]; float* M[2][4]; float* V[2][4]; float* PART[2][4]; float* LP[2]; float* VP[2];
};

// What the snapshot of a launch follows: the training loss (track_best = 1) or the validation loss (2).  A launch that does
// not carry that loss only hands the best value on to the other slot of the ping-pong.
static bool fit_tracks(const ndq_fused_fit* f, bool with_train, bool with_valid) {
  return (f->track_best == 1 && with_train) || (f->track_best == 2 && with_valid);
}

// Sums + tail launch of all networks, reading buffer set `set`: the training epoch with Adam step `adam_step` (with_train)
// and / or the validation loss -> valid_hist[vindex] (with_valid); set != 0 also brings parameters and moments home.
static int fit_tail(const FitCall& c, int set, bool with_train, bool with_valid, int adam_step, int hist_index, int vindex,
                    int parity) {
  const ndq_fused_fit* f = c.f;
  const ndq_fused_step& s0 = f->net[0];
  ValidArgs v{};
  if (with_valid) v = ValidArgs{c.VP[set], f->valid_blocks, f->valid_scale, f->valid_hist, vindex, f->track_best == 2 ? 1 : 0};
  const bool track = fit_tracks(f, with_train, with_valid);
  ReduceTailMultiArgs a{};
  for (int k = 0; k < f->n_nets; ++k) {
    const ndq_fused_step& s = f->net[k];
    a.net[k] = reduce_tail_args(s, s0, c.PART[set][k], c.LP[set], with_train ? s0.blocks : 0, with_train ? adam_step : 0,
                                hist_index, parity, k == 0 ? 1 : 0, track ? s.best_flat : nullptr, v,
                                set ? c.P[set][k] : nullptr, set ? c.M[set][k] : nullptr, set ? c.V[set][k] : nullptr);
  }
  return launch_tail_multi(a, c.max_params, f->n_nets, c.max_lparts, c.stream);
}

// Per epoch ONE closure launch (training workgroups + validation workgroups) and ONE sums / tail launch (blockIdx.y =
// network); a trailing validation-only pair closes the call.  Tail e < n_epochs: training epoch e + the validation loss
// of epoch e - 1.
static int fit_two_launch(const FitCall& c, int parity) {
  const ndq_fused_fit* f = c.f;
  const ndq_fused_step& s0 = f->net[0];
  for (int e = 0; e < c.n_epochs; ++e, parity ^= 1) {
    if (!c.train_coords[e]) return NDQ_EINVAL;
    const bool with_valid = c.valid && e > 0;
    int rc = f->launch(c.train_coords[e], s0.ldc, s0.n, c.P[0], c.PART[0], c.LP[0], s0.seed,
                       with_valid ? f->valid_coords : nullptr, f->valid_ldc, with_valid ? f->valid_n : 0, c.VP[0], nullptr,
                       c.stream);
    if (rc) return rc;
    rc = fit_tail(c, 0, true, with_valid, c.adam_step + e, c.hist_index + e, c.valid_index + e - 1, parity);
    if (rc) return rc;
  }
  if (!c.valid) return 0;
  int rc = f->launch(nullptr, 0, 0, c.P[0], nullptr, nullptr, 0.f, f->valid_coords, f->valid_ldc, f->valid_n, c.VP[0], nullptr,
                     c.stream);
  if (rc) return rc;
  return fit_tail(c, 0, false, true, 0, c.hist_index + c.n_epochs, c.valid_index + (c.n_epochs > 0 ? c.n_epochs - 1 : 0), parity);
}

// ---- pull and loop mode: launch e = 0 .. last of the sequence runs the training closure of epoch e (e < n_epochs), the
// validation closure on the parameters it starts from (valid && e >= 1), and FIRST, in its prologue (e >= 1), finishes
// training epoch e - 1 from buffer set (e - 1) & 1 into set e & 1.  What launch e finishes -- the ONE definition for the
// host of pull mode, the bias corrections of loop mode (whose device code, ndq_tail.h loop_pull_args, counts the same way)
// and the tail that closes the call, which is launch last + 1 without closures:
struct Finishes { int adam_step, hist_index, valid_index; bool with_valid; };
static Finishes launch_finishes(const FitCall& c, int e) {
  const int j = e - 1;                            // the training epoch; its launch also evaluated the validation of epoch j - 1
  return {c.adam_step + j, c.hist_index + j, c.valid_index + j - 1, c.valid && j >= 1};
}
static int fit_last_launch(const FitCall& c) { return c.valid ? c.n_epochs : c.n_epochs - 1; }

// the call's last launch: an ordinary tail, reading set `fin`, that leaves everything in the primary buffers -- with a
// validation batch the validation of the last epoch (no Adam), else the last training epoch's update
static int fit_closing_tail(const FitCall& c, int fin, int parity) {
  const Finishes w = launch_finishes(c, fit_last_launch(c) + 1);
  return fit_tail(c, fin, !c.valid, c.valid, w.adam_step, w.hist_index, w.valid_index, parity);
}

// PULL MODE: one launch per epoch
static int fit_pull(const FitCall& c, int parity) {
  const ndq_fused_fit* f = c.f;
  const ndq_fused_step& s0 = f->net[0];
  const int last = fit_last_launch(c);
  for (int e = 0; e <= last; ++e) {
    ndq::PullArgs pa{};
    if (e >= 1) {
      const Finishes w = launch_finishes(c, e);
      const int in = (e - 1) & 1, out = e & 1;
      pa.enabled = 1; pa.n_nets = f->n_nets; pa.nparts = s0.blocks;
      pa.lpart = c.LP[in]; pa.nlparts = s0.blocks; pa.lscale = s0.seed;
      pa.loss_hist = s0.loss_hist; pa.hist_index = w.hist_index; pa.loss_slot = s0.loss_slot;
      pa.vpart = w.with_valid ? c.VP[in] : nullptr; pa.nvparts = f->valid_blocks; pa.vscale = f->valid_scale;
      pa.valid_hist = f->valid_hist; pa.valid_index = w.valid_index; pa.best_on_valid = f->track_best == 2 ? 1 : 0;
      pa.best_loss = s0.best_loss; pa.parity = parity;
      const bool track = fit_tracks(f, true, w.with_valid);
      for (int k = 0; k < f->n_nets; ++k) {
        const ndq_fused_step& s = f->net[k];
        ndq::PullNet& n = pa.net[k];
        n.part = c.PART[in][k];
        n.p_in = c.P[in][k]; n.m_in = c.M[in][k]; n.v_in = c.V[in][k];
        n.p_out = c.P[out][k]; n.m_out = c.M[out][k]; n.v_out = c.V[out][k];
        n.grad = s.grad; n.best_flat = track ? s.best_flat : nullptr; n.len = s.n_params;
        n.adam = adam_consts(s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, w.adam_step);
      }
      parity ^= 1;                                 // every prologue is a tail
    }
    const bool train_part = e < c.n_epochs, valid_part = c.valid && e >= 1;
    if (train_part && !c.train_coords[e]) return NDQ_EINVAL;
    int rc = f->launch(train_part ? c.train_coords[e] : nullptr, s0.ldc, train_part ? s0.n : 0, c.P[e & 1],
                       train_part ? c.PART[e & 1] : nullptr, c.LP[e & 1], s0.seed, valid_part ? f->valid_coords : nullptr,
                       f->valid_ldc, valid_part ? f->valid_n : 0, c.VP[e & 1], &pa, c.stream);
    if (rc) return rc;
  }
  return fit_closing_tail(c, last & 1, parity);
}

// LOOP MODE: training and validation grid are ONE workgroup each -> runs of up to kLoopMaxLaunches launches of fit_pull's
// sequence become one launch of one workgroup that keeps the state in LDS (csrc/ndq_tail.h: LoopArgs); segment i reads
// buffer set i & 1 and leaves the other one.  `stride`: floats between the training batches of consecutive epochs.
static int fit_loop(const FitCall& c, long long stride, int parity) {
  const ndq_fused_fit* f = c.f;
  const ndq_fused_step& s0 = f->net[0];
  const int last = fit_last_launch(c);
  int in = 0;
  for (int e0 = 0; e0 <= last; e0 += ndq::kLoopMaxLaunches, in ^= 1) {
    const int e1 = e0 + ndq::kLoopMaxLaunches <= last + 1 ? e0 + ndq::kLoopMaxLaunches : last + 1;
    const int out = in ^ 1;
    ndq::LoopArgs L{};
    L.e0 = e0; L.e1 = e1; L.n_epochs = c.n_epochs; L.has_valid = c.valid ? 1 : 0; L.track_best = f->track_best;
    L.hist_index = c.hist_index; L.valid_index = c.valid_index; L.parity = parity; L.coord_stride = stride;
    L.lp_in = c.LP[in]; L.vp_in = c.VP[in]; L.lp_out = c.LP[out]; L.vp_out = c.VP[out];
    L.lscale = s0.seed; L.vscale = f->valid_scale;
    L.loss_hist = s0.loss_hist; L.loss_slot = s0.loss_slot; L.valid_hist = f->valid_hist; L.best_loss = s0.best_loss;
    for (int k = 0; k < f->n_nets; ++k) {
      const ndq_fused_step& s = f->net[k];
      ndq::LoopNet& n = L.net[k];
      n.p_in = c.P[in][k]; n.m_in = c.M[in][k]; n.v_in = c.V[in][k]; n.part_in = c.PART[in][k];
      n.p_out = c.P[out][k]; n.m_out = c.M[out][k]; n.v_out = c.V[out][k]; n.part_out = c.PART[out][k];
      n.grad = s.grad; n.best_flat = s.best_flat;
      n.lr = s.lr; n.b1 = s.beta1; n.b2 = s.beta2; n.eps = s.eps; n.wd = s.weight_decay;
      for (int e = e0 > 1 ? e0 : 1; e < e1; ++e) {
        const ndq::AdamConsts a = adam_consts(s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, launch_finishes(c, e).adam_step);
        n.bc1[e - e0] = a.bc1; n.bc2s[e - e0] = a.bc2s;
      }
    }
    int rc = f->launch_loop(c.train_coords[0], s0.ldc, s0.n, s0.seed, c.valid ? f->valid_coords : nullptr, f->valid_ldc,
                            c.valid ? f->valid_n : 0, &L, c.stream);
    if (rc) return rc;
  }
  // L.parity is the parity of the call's first launch in every segment (the kernel flips it per prologue): `last` prologues
  return fit_closing_tail(c, in, parity ^ (last & 1));
}

extern "C" {

int ndq_fused_fit_run(const ndq_fused_fit* f, int n_epochs, const float* const* train_coords, int adam_step,
                      int hist_index, int valid_index, int parity, void* stream) {
  if (!f || !f->launch || f->n_nets < 1 || f->n_nets > 4 || n_epochs < 0 || (n_epochs > 0 && (!train_coords || adam_step <= 0)) ||
      hist_index < 0 || valid_index < 0 || (parity != 0 && parity != 1) || f->track_best < 0 || f->track_best > 2)
    return NDQ_EINVAL;
  const ndq_fused_step& s0 = f->net[0];
  const bool valid = f->valid_coords != nullptr;
  if (!valid && n_epochs == 0) return NDQ_EINVAL;
  if (!s0.best_loss || (n_epochs > 0 && (!s0.loss_hist || !s0.loss_partials || s0.n <= 0 || s0.blocks <= 0))) return NDQ_EINVAL;
  if (valid && (!f->valid_loss_partials || !f->valid_hist || f->valid_n <= 0 || f->valid_blocks <= 0)) return NDQ_EINVAL;
  if (f->track_best == 2 && !valid) return NDQ_EINVAL;
  FitCall c{f, n_epochs, train_coords, adam_step, hist_index, valid_index, stream, valid};
  c.max_lparts = s0.blocks > f->valid_blocks ? s0.blocks : f->valid_blocks;
  c.LP[0] = s0.loss_partials; c.LP[1] = f->alt_loss_partials;
  c.VP[0] = f->valid_loss_partials; c.VP[1] = f->alt_valid_loss_partials;
  bool pull = f->pull_ok != 0 && n_epochs >= 2 && s0.blocks * f->n_nets <= ndq::kPullMaxWork && f->alt_loss_partials &&
              (!valid || f->alt_valid_loss_partials);
  for (int k = 0; k < f->n_nets; ++k) {
    const ndq_fused_step& s = f->net[k];
    if (!s.params || s.n_params <= 0 || (f->track_best && !s.best_flat)) return NDQ_EINVAL;
    if (n_epochs > 0 && (!s.partials || !s.grad || !s.adam_m || !s.adam_v || !s.loss_slot)) return NDQ_EINVAL;
    if (s.n_params > c.max_params) c.max_params = s.n_params;
    c.P[0][k] = s.params; c.M[0][k] = s.adam_m; c.V[0][k] = s.adam_v; c.PART[0][k] = s.partials;
    c.P[1][k] = f->alt_params[k]; c.M[1][k] = f->alt_m[k]; c.V[1][k] = f->alt_v[k]; c.PART[1][k] = f->alt_partials[k];
    pull = pull && c.P[1][k] && c.M[1][k] && c.V[1][k] && c.PART[1][k];
  }
  if (!pull) return fit_two_launch(c, parity);
  bool loop = f->loop_ok != 0 && f->launch_loop && s0.blocks == 1 && (!valid || f->valid_blocks == 1) &&
              f->n_nets <= ndq::kLoopMaxNets;
  long long stride = 0;
  if (loop) {                  // ... and the batches of the epochs are equally spaced in memory
    if (!train_coords[0] || !train_coords[1]) return NDQ_EINVAL;
    stride = train_coords[1] - train_coords[0];
    for (int e = 2; e < n_epochs && loop; ++e) {
      if (!train_coords[e]) return NDQ_EINVAL;
      loop = train_coords[e] - train_coords[0] == stride * e;
    }
  }
  return loop ? fit_loop(c, stride, parity) : fit_pull(c, parity);
}

int ndq_sample(const ndq_sampler_desc* desc, unsigned long long seed, unsigned long long draw, unsigned stream_id,
               float* coords, int ldc, void* stream) {
  return ndq::launch_sample(desc, seed, draw, stream_id, coords, ldc, (hipStream_t)stream);
}

int ndq_sample_table(const ndq_table_sampler_desc* desc, unsigned long long seed, unsigned long long draw,
                     unsigned stream_id, float* coords, int ldc, void* stream) {
  return ndq::launch_sample_table(desc, seed, draw, stream_id, coords, ldc, (hipStream_t)stream);
}

int ndq_sample_plan(const ndq_plan_sampler_desc* desc, unsigned long long seed, unsigned long long draw,
                    unsigned stream_id, float* coords, int ldc, void* stream) {
  return ndq::launch_sample_plan(desc, seed, draw, stream_id, coords, ldc, (hipStream_t)stream);
}

int ndq_sample_plan_indexed(const ndq_plan_sampler_desc* desc, const ndq_plan_index_desc* index, unsigned long long seed,
                            unsigned long long draw, unsigned stream_id, float* coords, int ldc, void* stream) {
  return ndq::launch_sample_plan_indexed(desc, index, seed, draw, stream_id, coords, ldc, (hipStream_t)stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- one-shot all-reduce
extern "C" {

int ndq_oneshot_create(int rank, int world, int max_len, void** out, unsigned char* handle64) {
  if (!out || !handle64 || world < 1 || world > ndq::kOneshotMaxRanks || rank < 0 || rank >= world || max_len < 1)
    return NDQ_EINVAL;
  ndq::Oneshot* c = new (std::nothrow) ndq::Oneshot();
  if (!c) return NDQ_EINVAL;
  std::memset(c, 0, sizeof(*c));
  int max_blocks = 0;
  const size_t bytes = ndq::oneshot_layout(world, max_len, &c->inbox_bytes, &c->flag_bytes, &max_blocks);
  // fine-grained (uncached) device memory: remote stores of the peers become visible to this device's loads without a
  // kernel boundary
  hipError_t e = hipExtMallocWithFlags(&c->base, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) e = hipExtMallocWithFlags(&c->base, bytes, hipDeviceMallocFinegrained);
  if (e != hipSuccess) { delete c; return (int)e; }
  e = hipMemset(c->base, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  hipIpcMemHandle_t h;
  if (e == hipSuccess) e = hipIpcGetMemHandle(&h, c->base);
  if (e != hipSuccess) { (void)hipFree(c->base); delete c; return (int)e; }
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "HIP IPC handles are 64 bytes");
  std::memcpy(handle64, &h, 64);
  c->dev.rank = rank; c->dev.world = world; c->dev.max_len = max_len; c->dev.max_blocks = max_blocks;
  c->dev.spin_limit = ndq::kOneshotSpinLimit;
  if (const char* e = std::getenv("NDQ_ONESHOT_SPIN_LIMIT")) c->dev.spin_limit = std::strtoull(e, nullptr, 10);
  c->dev.status = reinterpret_cast<unsigned*>(static_cast<char*>(c->base) + c->inbox_bytes + c->flag_bytes);
  c->step = 0;
  *out = c;
  return 0;
}

// handles: world x 64 bytes, rank-major (every rank's ndq_oneshot_create handle, its own included)
int ndq_oneshot_connect(void* ctx, const unsigned char* handles) {
  ndq::Oneshot* c = static_cast<ndq::Oneshot*>(ctx);
  if (!c || !handles) return NDQ_EINVAL;
  for (int q = 0; q < c->dev.world; ++q) {
    void* p = c->base;
    if (q != c->dev.rank) {
      hipIpcMemHandle_t h;
      std::memcpy(&h, handles + 64 * q, 64);
      hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) return (int)e;
      c->peer_base[q] = p;
    }
    c->dev.inbox[q] = static_cast<float*>(p);
    c->dev.flags[q] = reinterpret_cast<unsigned*>(static_cast<char*>(p) + c->inbox_bytes);
  }
  return 0;
}

// ncclAllReduce's signature (sum of fp32 only): what ndq_fused_step.allreduce points at, with .comm = the context
int ndq_oneshot_allreduce(const void* send, void* recv, size_t count, int dtype, int op, void* comm, void* stream) {
  ndq::Oneshot* c = static_cast<ndq::Oneshot*>(comm);
  if (!c || !send || !recv || dtype != 7 || op != 0 || count == 0 || (long)count > c->dev.max_len) return NDQ_EINVAL;
  const unsigned step = ++c->step;
  const int blocks = ((int)count + ndq::kOneshotChunk - 1) / ndq::kOneshotChunk;
  hipLaunchKernelGGL(ndq::oneshot_allreduce_kernel, dim3(blocks), dim3(1024), 0, static_cast<hipStream_t>(stream), c->dev,
                     static_cast<const float*>(send), static_cast<float*>(recv), (int)count, step);
  return (int)hipGetLastError();
}

// number of flag waits that ran into their spin limit since creation (synchronises the device); 0 = healthy
int ndq_oneshot_status(void* ctx) {
  ndq::Oneshot* c = static_cast<ndq::Oneshot*>(ctx);
  if (!c) return NDQ_EINVAL;
  unsigned v = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(&v, c->dev.status, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (int)v;
}

int ndq_oneshot_destroy(void* ctx) {
  ndq::Oneshot* c = static_cast<ndq::Oneshot*>(ctx);
  if (!c) return NDQ_EINVAL;
  (void)hipDeviceSynchronize();
  for (int q = 0; q < c->dev.world; ++q)
    if (q != c->dev.rank && c->peer_base[q]) (void)hipIpcCloseMemHandle(c->peer_base[q]);
  (void)hipFree(c->base);
  delete c;
  return 0;
}

}  // extern "C"
