// Device-side collocation-point sampler (include/ndq.h: ndq_sample).  One Philox4x32-10 block per point, keyed by
// (seed, draw counter, stream id): counter-based, so a batch is reproducible from three integers, shards on different
// ranks never overlap and no generator state lives in HBM.  HBM-bound by construction: writes d floats per point.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ndq.h"

namespace ndq {

struct U4 { unsigned x, y, z, w; };

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the generator torch uses on
// GPUs; restated in oracle/philox_ref.py and pinned there to the Random123 known-answer vectors.
__host__ __device__ inline U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
    U4 n;
    n.x = (unsigned)(p1 >> 32) ^ c.y ^ k0;
    n.y = (unsigned)p1;
    n.z = (unsigned)(p0 >> 32) ^ c.w ^ k1;
    n.w = (unsigned)p0;
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

__device__ inline float u01(unsigned x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }          // [0, 1)
__device__ inline float u01_open(unsigned x) { return (float)((x >> 8) + 1u) * 5.9604644775390625e-8f; }  // (0, 1]

// torch.linspace(lo, hi, n)[i]: stepped from the nearer end with one fused multiply-add (ATen RangeFactories)
__device__ inline float linspace_at(float lo, float hi, int n, int i) {
  if (n <= 1) return lo;
  const float step = (hi - lo) / (float)(n - 1);
  return (i < n / 2) ? fmaf(step, (float)i, lo) : fmaf(-step, (float)(n - 1 - i), hi);
}

struct SampleArgs {
  ndq_sampler_desc s;
  unsigned k0, k1, c1, c2, c3;
  float* coords;
  int ldc, total;
};

// point i of the batch described by a (one thread per point; also called from the epoch tail kernel's extra
// workgroups, which draw the NEXT batch while the optimiser step is applied: csrc/ndq_api.hip)
__device__ __forceinline__ void sample_point_store(const SampleArgs& a, int i) {
  if (i >= a.total) return;
  const U4 r = philox4x32_10(U4{(unsigned)i, a.c1, a.c2, a.c3}, a.k0, a.k1);
  const unsigned w[4] = {r.x, r.y, r.z, r.w};
  const ndq_sampler_desc& s = a.s;
  if (s.kind == NDQ_SAMPLE_UNIFORM) {                       // generators.py:150-152 (Generator1D 'uniform')
    for (int c = 0; c < s.d; ++c) a.coords[(size_t)c * a.ldc + i] = s.lo[c] + (s.hi[c] - s.lo[c]) * u01(w[c]);
  } else if (s.kind == NDQ_SAMPLE_GRID) {                   // generators.py:253-266: ij-meshgrid + N(0, std^2) jitter
    // Box-Muller: (w0, w1) -> two normals, (w2, w3) -> two more
    const float r0 = sqrtf(-2.0f * __logf(u01_open(w[0]))), t0 = 6.283185307179586f * u01(w[1]);
    const float r1 = sqrtf(-2.0f * __logf(u01_open(w[2]))), t1 = 6.283185307179586f * u01(w[3]);
    const float z[3] = {r0 * __cosf(t0), r0 * __sinf(t0), r1 * __cosf(t1)};
    int rem = i;
    int idx[3] = {0, 0, 0};
    for (int c = s.d - 1; c >= 0; --c) { idx[c] = rem % s.n[c]; rem /= s.n[c]; }
    for (int c = 0; c < s.d; ++c) {
      float v = linspace_at(s.lo[c], s.hi[c], s.n[c], idx[c]);
      if (s.noise_std[c] != 0.0f) v = fmaf(s.noise_std[c], z[c], v);
      a.coords[(size_t)c * a.ldc + i] = v;
    }
  } else {                                                  // generators.py:622-646 (GeneratorSpherical)
    const float p = u01_open(w[0]), q = u01_open(w[1]), t = u01_open(w[2]);
    const float inv = 1.0f / (p + q + t);
    float x = sqrtf(p * inv) + 1e-6f, y = sqrtf(q * inv) + 1e-6f, z = fminf(sqrtf(t * inv) + 1e-6f, 1.0f);
    if (w[0] & 1u) x = -x;                                  // the low 8 bits of each word are not used by u01
    if (w[1] & 1u) y = -y;
    if (w[2] & 1u) z = -z;
    const float u = u01(w[3]);
    const float lo = s.lo[0], hi = s.hi[0];
    const float rad = s.radial ? lo + (hi - lo) * u : sqrtf((hi * hi - lo * lo) * u + lo * lo);
    a.coords[i] = rad;
    a.coords[(size_t)a.ldc + i] = acosf(z);
    a.coords[(size_t)2 * a.ldc + i] = 3.14159265358979f - atan2f(y, x);
  }
}

__global__ void __launch_bounds__(256) sample_kernel(SampleArgs a) { sample_point_store(a, blockIdx.x * 256 + threadIdx.x); }

// validated launch arguments of one draw; returns 0 or NDQ_EINVAL
inline int fill_sample_args(SampleArgs& a, const ndq_sampler_desc* s, unsigned long long seed, unsigned long long draw,
                            unsigned stream_id, float* coords, int ldc) {
  if (!s || !coords || s->d < 1 || s->d > 3) return NDQ_EINVAL;
  long long total = 0;
  if (s->kind == NDQ_SAMPLE_GRID) {
    total = 1;
    for (int c = 0; c < s->d; ++c) {
      if (s->n[c] < 1) return NDQ_EINVAL;
      total *= s->n[c];
    }
  } else if (s->kind == NDQ_SAMPLE_UNIFORM || s->kind == NDQ_SAMPLE_SPHERICAL) {
    total = s->n[0];
    if (s->kind == NDQ_SAMPLE_SPHERICAL && s->d != 3) return NDQ_EINVAL;
  } else {
    return NDQ_EINVAL;
  }
  if (total < 1 || total > 0x7fffffffLL || ldc < total) return NDQ_EINVAL;
  a.s = *s;
  a.k0 = (unsigned)seed; a.k1 = (unsigned)(seed >> 32);
  a.c1 = (unsigned)draw; a.c2 = (unsigned)(draw >> 32); a.c3 = stream_id;
  a.coords = coords; a.ldc = ldc; a.total = (int)total;
  return 0;
}

inline int launch_sample(const ndq_sampler_desc* s, unsigned long long seed, unsigned long long draw, unsigned stream_id,
                         float* coords, int ldc, hipStream_t stream) {
  SampleArgs a;
  const int rc = fill_sample_args(a, s, seed, draw, stream_id, coords, ldc);
  if (rc) return rc;
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------ table sampler
// include/ndq.h: ndq_sample_table.  The node positions / jitter widths of every axis come from small device tables the
// host built from the wrapped generator's own tensors (GeneratorND: generators.py:419-569, any method per axis, `cut`,
// `abs_value`; Generator1D 'log-spaced[-noisy]', 'chebyshev*'), so up to six axes and any spacing cost the same kernel.
struct TableArgs {
  ndq_table_sampler_desc s;
  unsigned k0, k1, c1, c2, c3;
  float* coords;
  int ldc, total, noisy;      // noisy == 0: no axis has a width table or a random law -- no Philox block is computed
};

// two Box-Muller pairs of one Philox block, three of the four normals: the words of NDQ_SAMPLE_GRID, in its order
__device__ __forceinline__ void normals3(const U4& r, float& z0, float& z1, float& z2) {
  const float r0 = sqrtf(-2.0f * __logf(u01_open(r.x))), t0 = 6.283185307179586f * u01(r.y);
  const float r1 = sqrtf(-2.0f * __logf(u01_open(r.z))), t1 = 6.283185307179586f * u01(r.w);
  z0 = r0 * __cosf(t0); z1 = r0 * __sinf(t0); z2 = r1 * __cosf(t1);
}

// One thread per point; every loop over the axes is unrolled to NDQ_TABLE_MAX_AXES with `c < d` guards so that n / idx /
// z stay in registers (no runtime-indexed private array, no scratch).  Stores: consecutive lanes -> consecutive floats
// of each SoA row.  Table reads: axis c repeats an entry over prod(n[c+1..]) consecutive points -- L1/L2 hits; in 1-D the
// table is streamed once, coalesced.
__global__ void __launch_bounds__(256) sample_table_kernel(TableArgs a) {
  const unsigned iu = blockIdx.x * 256u + threadIdx.x;      // (unsigned: the last workgroup of a 2^31 - 1 point draw)
  if (iu >= (unsigned)a.total) return;
  const int i = (int)iu;
  const ndq_table_sampler_desc& s = a.s;
  // (fill_table_args admits CHEB2_NOISY on axis 0 of a one-axis descriptor only, so law[0] decides for the whole draw)
  if (s.law[0] == NDQ_AXIS_CHEB2_NOISY) {                   // generators.py:32-34 (_chebyshev_second_noisy); d == 1
    const U4 r = philox4x32_10(U4{(unsigned)i, a.c1, a.c2, a.c3}, a.k0, a.k1);
    const float t = ((float)i + (2.0f * u01(r.x) - 1.0f)) / (float)(s.n[0] - 1) * 3.14159265358979f;
    const float lo = s.lo[0], hi = s.hi[0];
    a.coords[i] = ((lo + hi) + (hi - lo) * cosf(t)) / 2.0f;
    return;
  }
  float z[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (a.noisy) {
    normals3(philox4x32_10(U4{(unsigned)i, a.c1, a.c2, a.c3}, a.k0, a.k1), z[0], z[1], z[2]);
    // axes 3..5: a second block whose counter word 0 has the top bit set (total <= 2^31 - 1: no point owns that word)
    if (s.d > 3) normals3(philox4x32_10(U4{(unsigned)i | 0x80000000u, a.c1, a.c2, a.c3}, a.k0, a.k1), z[3], z[4], z[5]);
  }
  unsigned rem = (unsigned)i;
  int idx[NDQ_TABLE_MAX_AXES] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = NDQ_TABLE_MAX_AXES - 1; c >= 0; --c)
    if (c < s.d) { const unsigned n = (unsigned)s.n[c]; idx[c] = (int)(rem % n); rem /= n; }
#pragma unroll
  for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c)
    if (c < s.d) {
      float v = s.mean[c][idx[c]];
      if (s.std[c]) {
        const float w = s.std[c][idx[c]];
        if (w != 0.0f) v = fmaf(w, z[c], v);
      }
      if (s.abs_value) v = fabsf(v);
      a.coords[(size_t)c * a.ldc + i] = v;
    }
}

// validated launch arguments of one table draw; returns 0 or NDQ_EINVAL (nothing is launched on NDQ_EINVAL)
inline int fill_table_args(TableArgs& a, const ndq_table_sampler_desc* s, unsigned long long seed, unsigned long long draw,
                           unsigned stream_id, float* coords, int ldc) {
  if (!s || !coords || s->d < 1 || s->d > NDQ_TABLE_MAX_AXES) return NDQ_EINVAL;
  long long total = 1;
  int noisy = 0;
  for (int c = 0; c < s->d; ++c) {
    if (s->n[c] < 1) return NDQ_EINVAL;
    total *= s->n[c];
    if (total > 0x7fffffffLL) return NDQ_EINVAL;
    if (s->law[c] == NDQ_AXIS_NORMAL) {
      if (!s->mean[c]) return NDQ_EINVAL;
      noisy |= s->std[c] != nullptr;
    } else if (s->law[c] == NDQ_AXIS_CHEB2_NOISY) {
      if (s->d != 1 || s->n[c] < 2) return NDQ_EINVAL;
      noisy = 1;
    } else {
      return NDQ_EINVAL;
    }
  }
  if (ldc < total) return NDQ_EINVAL;
  a.s = *s;
  a.k0 = (unsigned)seed; a.k1 = (unsigned)(seed >> 32);
  a.c1 = (unsigned)draw; a.c2 = (unsigned)(draw >> 32); a.c3 = stream_id;
  a.coords = coords; a.ldc = ldc; a.total = (int)total; a.noisy = noisy;
  return 0;
}

inline int launch_sample_table(const ndq_table_sampler_desc* s, unsigned long long seed, unsigned long long draw,
                               unsigned stream_id, float* coords, int ldc, hipStream_t stream) {
  TableArgs a;
  const int rc = fill_table_args(a, s, seed, draw, stream_id, coords, ldc);
  if (rc) return rc;
  hipLaunchKernelGGL(sample_table_kernel, dim3(((unsigned)a.total + 255u) / 256u), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ndq
