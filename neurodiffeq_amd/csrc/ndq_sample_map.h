// Per-point stages above a plan (TransformGenerator / FilterGenerator: generators.plan_spec `stages`), drawn on the device.  Tail
// of a generated module (codegen.SamplerMapProgram): the module defines NDQ_MAP_DIN / NDQ_MAP_DOUT / NDQ_MAP_FILTER and
//   __device__ __forceinline__ void ndq_map_point(float (&v)[6], bool& keep);
// -- the user's traced callables as straight-line fp32 code: v holds the NDQ_MAP_DIN rows of a plan point on entry and the
// NDQ_MAP_DOUT rows handed out on return; keep: the AND of the filters' masks -- and then includes this file: the kernels, each a
// template on the index mode like sample_plan_kernel, and the one exported launcher.
//
// A point is a pure function of (seed, draw, stream id, i) -- Philox is counter-based --, so the filter route RECOMPUTES its points
// instead of keeping them: count (kept points per workgroup) -> scan (exclusive offsets, total) -> compact (recompute, store the
// kept points at offset + rank).  Three stream-ordered launches; no atomics, no spin-wait, nothing waits on another workgroup.
// Order-preserving: the output is the kept points in the order of the unfiltered draw (what x[mask] gives the reference).
#pragma once
#include "ndq_sample.h"

namespace ndq {

// rows of output point i after the stages; false: past the end, or filtered out.  Every thread of the workgroup comes back (no
// early return: the callers go on to a barrier).
template <int MODE, class Args>
__device__ __forceinline__ bool map_point(const Args& args, unsigned i, float (&v)[NDQ_TABLE_MAX_AXES]) {
  const bool inside = plan_point<MODE>(args, i, v);
  bool keep = true;
  if (inside) ndq_map_point(v, keep);
  return inside && keep;
}

// Transform only: one thread per point, NDQ_MAP_DOUT coalesced row stores -- the plan kernel's traffic, nothing else.
template <int MODE, class Args>
__global__ void __launch_bounds__(256) sample_plan_map_kernel(Args args) {
  const PlanArgs& a = plan_args(args);
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  float v[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (!map_point<MODE>(args, i, v)) return;                  // (no filter: false only past the end)
#pragma unroll
  for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c)
    if (c < NDQ_MAP_DOUT) a.coords[(size_t)c * a.ldc + i] = v[c];
}

// kept lanes of the four waves of a workgroup, in LDS; read in fixed order
__device__ __forceinline__ unsigned long long wave_kept(bool keep, unsigned (&wc)[4]) {
  const unsigned long long b = __ballot(keep);
  if ((threadIdx.x & 63u) == 0u) wc[threadIdx.x >> 6] = (unsigned)__popcll(b);
  __syncthreads();
  return b;
}

template <int MODE, class Args>
__global__ void __launch_bounds__(256) count_kernel(Args args, unsigned* counts) {
  __shared__ unsigned wc[4];
  float v[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  wave_kept(map_point<MODE>(args, blockIdx.x * 256u + threadIdx.x, v), wc);
  if (threadIdx.x == 0u) counts[blockIdx.x] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
}

// ONE workgroup: counts[0 .. n) -> exclusive offsets in place, total -> kept[0].  Chunks of 256 with a running carry; every loop
// bound is workgroup-uniform.
__global__ void __launch_bounds__(256) scan_kernel(unsigned* counts, int n, unsigned* kept) {
  __shared__ unsigned s[256];
  const unsigned t = threadIdx.x;
  unsigned carry = 0u;
  for (int base = 0; base < n; base += 256) {
    const int j = base + (int)t;
    const unsigned c = j < n ? counts[j] : 0u;
    s[t] = c;
    __syncthreads();
    for (unsigned off = 1u; off < 256u; off <<= 1) {        // inclusive Hillis-Steele scan of the chunk
      const unsigned below = t >= off ? s[t - off] : 0u;
      __syncthreads();
      s[t] += below;
      __syncthreads();
    }
    if (j < n) counts[j] = carry + s[t] - c;
    carry += s[255];
    __syncthreads();                                        // (s is rewritten by the next chunk)
  }
  if (t == 0u) kept[0] = carry;
}

template <int MODE, class Args>
__global__ void __launch_bounds__(256) compact_kernel(Args args, const unsigned* offsets) {
  __shared__ unsigned wc[4];
  const PlanArgs& a = plan_args(args);
  float v[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const bool keep = map_point<MODE>(args, blockIdx.x * 256u + threadIdx.x, v);
  const unsigned long long b = wave_kept(keep, wc);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned rank = (unsigned)__popcll(b & ((1ull << lane) - 1ull));       // kept lanes below this one
#pragma unroll
  for (unsigned q = 0u; q < 3u; ++q)
    if (q < wave) rank += wc[q];
  const unsigned pos = offsets[blockIdx.x] + rank;          // < kept <= output points <= ldc (the same points as count_kernel)
  if (!keep || pos >= (unsigned)a.ldc) return;
#pragma unroll
  for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c)
    if (c < NDQ_MAP_DOUT) a.coords[(size_t)c * a.ldc + pos] = v[c];
}

template <int MODE, class Args>
int launch_map(const Args& a, unsigned out, unsigned* work, hipStream_t stream) {
  const dim3 grid((out + 255u) / 256u), block(256);
#if NDQ_MAP_FILTER
  hipLaunchKernelGGL((count_kernel<MODE, Args>), grid, block, 0, stream, a, work + 1);
  hipLaunchKernelGGL(scan_kernel, dim3(1), block, 0, stream, work + 1, (int)grid.x, work);
  hipLaunchKernelGGL((compact_kernel<MODE, Args>), grid, block, 0, stream, a, (const unsigned*)(work + 1));
#else
  hipLaunchKernelGGL((sample_plan_map_kernel<MODE, Args>), grid, block, 0, stream, a);
#endif
  return (int)hipGetLastError();
}

}  // namespace ndq

extern "C" int ndq_map_rows_in(void) { return NDQ_MAP_DIN; }
extern "C" int ndq_map_rows_out(void) { return NDQ_MAP_DOUT; }
extern "C" int ndq_map_filters(void) { return NDQ_MAP_FILTER; }

// One draw of a plan with stages into coords[rows][ldc].  index: NULL, or the Resample / Batch root (ndq_sample_plan_indexed).
// Filter modules: work[0] receives the kept count, work[1 .. 1 + workgroups) are the per-workgroup counts / offsets (work_len
// entries in all); the kept points are rows [0, kept) of the first NDQ_MAP_DOUT rows.  NDQ_EINVAL (nothing launched): whatever
// ndq_sample_plan / ndq_sample_plan_indexed refuse, a plan of another row count than the stages were traced for, fewer rows than
// NDQ_MAP_DOUT, a missing or short work buffer.
extern "C" int ndq_map_launch(const ndq_plan_sampler_desc* p, const ndq_plan_index_desc* index, unsigned long long seed,
                              unsigned long long draw, unsigned stream_id, float* coords, int ldc, int rows, unsigned* work,
                              int work_len, void* stream) {
  using namespace ndq;
  if (!p || p->d != NDQ_MAP_DIN || rows < NDQ_MAP_DOUT) return NDQ_EINVAL;
  PlanIndexArgs a;
  int rc;
  if (index) {
    rc = fill_plan_index_args(a, p, index, seed, draw, stream_id, coords, ldc);
  } else {
    rc = fill_plan_args(a.p, p, seed, draw, stream_id, coords, ldc);
    a.out = a.p.total;
  }
  if (rc) return rc;
  const unsigned out = (unsigned)a.out;
  if (NDQ_MAP_FILTER && (!work || work_len < 1 || (unsigned)(work_len - 1) < (out + 255u) / 256u)) return NDQ_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!index) return launch_map<NDQ_INDEX_PLAIN>(a.p, out, work, s);
  if (index->mode == NDQ_INDEX_PERMUTE) return launch_map<NDQ_INDEX_PERMUTE>(a, out, work, s);
  if (index->mode == NDQ_INDEX_REPLACE) return launch_map<NDQ_INDEX_REPLACE>(a, out, work, s);
  return launch_map<NDQ_INDEX_NONE>(a, out, work, s);
}
