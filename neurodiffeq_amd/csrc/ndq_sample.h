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

// Box-Muller on one Philox block: (w0, w1) -> two normals, (w2, w3) -> a third; the words of NDQ_SAMPLE_GRID, in its order
__device__ __forceinline__ void normals3(const U4& r, float& z0, float& z1, float& z2) {
  const float r0 = sqrtf(-2.0f * __logf(u01_open(r.x))), t0 = 6.283185307179586f * u01(r.y);
  const float r1 = sqrtf(-2.0f * __logf(u01_open(r.z))), t1 = 6.283185307179586f * u01(r.w);
  z0 = r0 * __cosf(t0); z1 = r0 * __sinf(t0); z2 = r1 * __cosf(t1);
}

// Philox key and counter words 1..3 of one draw of one generator: key = seed, counter = (point, draw_lo, draw_hi, stream id)
struct DrawKey { unsigned k0, k1, c1, c2, c3; };
__device__ __forceinline__ U4 block_a(const DrawKey& k, int j) { return philox4x32_10(U4{(unsigned)j, k.c1, k.c2, k.c3}, k.k0, k.k1); }
// a second block whose counter word 0 has the top bit set (at most 2^31 - 1 points: no point owns that word)
__device__ __forceinline__ U4 block_b(const DrawKey& k, int j) {
  return philox4x32_10(U4{(unsigned)j | 0x80000000u, k.c1, k.c2, k.c3}, k.k0, k.k1);
}

// ---- THE definition of every ndq_sampler_desc law: point j of the draw `k` of `s` -> v[0 .. s.d - 1].  Called by sample_kernel,
// by the epoch tail kernel's prefetch workgroups and by sample_plan_kernel.  Every loop over the coordinates is unrolled with
// `c < d` guards (no runtime-indexed private array, no scratch).  noisy == 0 (an exact grid): no Philox block is computed.
__device__ __forceinline__ void simple_point(const ndq_sampler_desc& s, int noisy, const DrawKey& k, int j, float (&v)[3]) {
  U4 r = U4{0u, 0u, 0u, 0u};
  if (noisy) r = block_a(k, j);
  if (s.kind == NDQ_SAMPLE_UNIFORM) {                       // generators.py:150-152 (Generator1D 'uniform')
    const unsigned w[3] = {r.x, r.y, r.z};
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < s.d) v[c] = s.lo[c] + (s.hi[c] - s.lo[c]) * u01(w[c]);
  } else if (s.kind == NDQ_SAMPLE_GRID) {                   // generators.py:253-266: ij-meshgrid + N(0, std^2) jitter
    float z[3] = {0.0f, 0.0f, 0.0f};
    if (noisy) normals3(r, z[0], z[1], z[2]);
    int rem = j;
    int idx[3] = {0, 0, 0};
#pragma unroll
    for (int c = 2; c >= 0; --c)
      if (c < s.d) { idx[c] = rem % s.n[c]; rem /= s.n[c]; }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < s.d) {
        float x = linspace_at(s.lo[c], s.hi[c], s.n[c], idx[c]);
        if (s.noise_std[c] != 0.0f) x = fmaf(s.noise_std[c], z[c], x);
        v[c] = x;
      }
  } else {                                                  // generators.py:622-646 (GeneratorSpherical)
    const float p = u01_open(r.x), q = u01_open(r.y), t = u01_open(r.z);
    const float inv = 1.0f / (p + q + t);
    float x = sqrtf(p * inv) + 1e-6f, y = sqrtf(q * inv) + 1e-6f, z = fminf(sqrtf(t * inv) + 1e-6f, 1.0f);
    if (r.x & 1u) x = -x;                                   // the low 8 bits of each word are not used by u01
    if (r.y & 1u) y = -y;
    if (r.z & 1u) z = -z;
    const float u = u01(r.w);
    const float lo = s.lo[0], hi = s.hi[0];
    v[0] = s.radial ? lo + (hi - lo) * u : sqrtf((hi * hi - lo * lo) * u + lo * lo);
    v[1] = acosf(z);
    v[2] = 3.14159265358979f - atan2f(y, x);
  }
}

// point i of the batch described by a (one thread per point; also called from the epoch tail kernel's extra
// workgroups, which draw the NEXT batch while the optimiser step is applied: csrc/ndq_api.hip)
__device__ __forceinline__ void sample_point_store(const SampleArgs& a, int i) {
  if (i >= a.total) return;
  float v[3] = {0.0f, 0.0f, 0.0f};
  simple_point(a.s, 1, DrawKey{a.k0, a.k1, a.c1, a.c2, a.c3}, i, v);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (c < a.s.d) a.coords[(size_t)c * a.ldc + i] = v[c];
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

// ---- THE definition of every ndq_table_sampler_desc law: point j of the draw `k` of `s` -> v[0 .. s.d - 1] (sample_table_kernel,
// sample_plan_kernel).  Every loop over the axes is unrolled to NDQ_TABLE_MAX_AXES with `c < d` guards so that n / idx / z
// stay in registers (no runtime-indexed private array, no scratch).  noisy == 0: no axis has a width table or a random
// law -- no Philox block is computed; block B only for d > 3.  Table reads: axis c repeats an entry over
// prod(n[c+1..]) consecutive points -- L1/L2 hits; in 1-D the table is streamed once, coalesced.
__device__ __forceinline__ void table_point(const ndq_table_sampler_desc& s, int noisy, const DrawKey& k, int j,
                                            float (&v)[NDQ_TABLE_MAX_AXES]) {
  // (fill_table_args admits CHEB2_NOISY on axis 0 of a one-axis descriptor only, so law[0] decides for the whole draw)
  if (s.law[0] == NDQ_AXIS_CHEB2_NOISY) {                   // generators.py:32-34 (_chebyshev_second_noisy); d == 1
    const U4 r = block_a(k, j);
    const float t = ((float)j + (2.0f * u01(r.x) - 1.0f)) / (float)(s.n[0] - 1) * 3.14159265358979f;
    const float lo = s.lo[0], hi = s.hi[0];
    v[0] = ((lo + hi) + (hi - lo) * cosf(t)) / 2.0f;
    return;
  }
  float z[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (noisy) {
    normals3(block_a(k, j), z[0], z[1], z[2]);
    if (s.d > 3) normals3(block_b(k, j), z[3], z[4], z[5]);
  }
  unsigned rem = (unsigned)j;
  int idx[NDQ_TABLE_MAX_AXES] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = NDQ_TABLE_MAX_AXES - 1; c >= 0; --c)
    if (c < s.d) { const unsigned n = (unsigned)s.n[c]; idx[c] = (int)(rem % n); rem /= n; }
#pragma unroll
  for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c)
    if (c < s.d) {
      float x = s.mean[c][idx[c]];
      if (s.std[c]) {
        const float w = s.std[c][idx[c]];
        if (w != 0.0f) x = fmaf(w, z[c], x);
      }
      if (s.abs_value) x = fabsf(x);
      v[c] = x;
    }
}

// One thread per point.  Stores: consecutive lanes -> consecutive floats of each SoA row.
__global__ void __launch_bounds__(256) sample_table_kernel(TableArgs a) {
  const unsigned iu = blockIdx.x * 256u + threadIdx.x;      // (unsigned: the last workgroup of a 2^31 - 1 point draw)
  if (iu >= (unsigned)a.total) return;
  const int i = (int)iu;
  float v[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  table_point(a.s, a.noisy, DrawKey{a.k0, a.k1, a.c1, a.c2, a.c3}, i, v);
#pragma unroll
  for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c)
    if (c < a.s.d) a.coords[(size_t)c * a.ldc + i] = v[c];
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

// ------------------------------------------------------------------------------------------------------- plan sampler
// include/ndq.h: ndq_sample_plan.  Composed generators (g1 + g2, g1 * g2, g1 ^ g2 over leaf generators) in ONE launch.
// The host flattens the plan into one record per LEAF: which output points its segment owns, how an output point maps to
// the leaf-local index, which rows it writes and under which key it draws.
struct PlanLeaf {
  int kind, row0, rows, noisy;     // noisy == 0: an exact leaf (exact nodes, DATA) -- no Philox block
  unsigned off, size;              // its segment's output points: [off, off + size)
  unsigned div, n;                 // MESH factor: local index = (i - off) / div % n (div = product of the later factors' sizes);
                                   // div == 0 (LEAF / ENSEMBLE): local index = i - off
  unsigned k0, k1;                 // seed + l * 0x9E3779B97F4A7C15
  union {
    ndq_sampler_desc simple;
    ndq_table_sampler_desc table;
    const float* data[NDQ_TABLE_MAX_AXES];
  } u;
};
struct PlanArgs {                  // by value: 8 x 240 + 40 bytes of the 4 KB kernarg segment
  PlanLeaf leaf[NDQ_PLAN_MAX_LEAVES];
  int n_leaves;
  unsigned c1, c2, c3;
  float* coords;
  int ldc, total;
  int d;                           // rows of the plan (every point has all of them)
};
static_assert(sizeof(PlanArgs) <= 2048, "PlanArgs is passed by value");

// One thread per output point.  The loop runs over the LEAVES, not over the thread's own segment: the trip count and the
// index into a.leaf are wave-uniform, so every descriptor field is a scalar load from the kernarg segment and a wave none
// of whose lanes lies in a leaf's segment skips it in one branch; lanes diverge only in the waves that straddle a
// segment boundary.  Each leaf's values come from the value functions above (one definition of every law); its rows are
// stored at coords[(row0 + c) * ldc + i]: consecutive lanes -> consecutive floats of every row.
// The kernel is a template on the index mode (NDQ_INDEX_*; NDQ_INDEX_PLAIN: ndq_sample_plan, whose instantiation is the kernel
// as it was before there was an index) and on its launch arguments; the indexed modes are described further down, at
// PlanIndexArgs.
#define NDQ_INDEX_PLAIN (-1)
struct PlanIndexArgs;
template <int MODE> struct PlanIndexPoint;                  // window + index map of one output point (indexed modes)
__device__ __forceinline__ const PlanArgs& plan_args(const PlanArgs& a) { return a; }
__device__ __forceinline__ const PlanArgs& plan_args(const PlanIndexArgs& a);

// ---- THE per-point body of the plan sampler: the rows of output point i, in registers (sample_plan_kernel; the generated
// map / filter kernels of csrc/ndq_sample_map.h recompute a point with it instead of storing it).  false: i is past the last
// output point (v is then not meaningful).  No thread returns before the barrier of PlanIndexPoint<PERMUTE>::map, so a caller may
// go on to a workgroup barrier of its own.  v[row0 + c] is written through selects on wave-uniform conditions (row0 / rows are
// scalar loads from the kernarg segment): no runtime-indexed private array, no scratch.
template <int MODE, class Args>
__device__ __forceinline__ bool plan_point(const Args& args, unsigned i, float (&v)[NDQ_TABLE_MAX_AXES]) {
  const PlanArgs& a = plan_args(args);
  unsigned pt = 0u, k1 = 0u, k2 = 0u;                       // indexed: plan point and draw counter words of output point i
  if constexpr (MODE == NDQ_INDEX_PLAIN) {
    if (i >= (unsigned)a.total) return false;
  } else {
    if (!PlanIndexPoint<MODE>::map(args, i, pt, k1, k2)) return false;
  }
  for (int l = 0; l < a.n_leaves; ++l) {
    const PlanLeaf& L = a.leaf[l];
    const unsigned rel = (MODE == NDQ_INDEX_PLAIN ? i : pt) - L.off;
    if (rel >= L.size) continue;
    const int j = (int)(L.div ? rel / L.div % L.n : rel);
    const DrawKey k{L.k0, L.k1, MODE == NDQ_INDEX_PLAIN ? a.c1 : k1, MODE == NDQ_INDEX_PLAIN ? a.c2 : k2, a.c3};
    float w[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (L.kind == NDQ_LEAF_SIMPLE) {
      float s[3] = {0.0f, 0.0f, 0.0f};
      simple_point(L.u.simple, L.noisy, k, j, s);
      w[0] = s[0]; w[1] = s[1]; w[2] = s[2];
    } else if (L.kind == NDQ_LEAF_TABLE) {
      table_point(L.u.table, L.noisy, k, j, w);
    } else {
#pragma unroll
      for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c)
        if (c < L.rows) w[c] = L.u.data[c][j];
    }
#pragma unroll
    for (int r = 0; r < NDQ_TABLE_MAX_AXES; ++r)
#pragma unroll
      for (int c = 0; c <= r; ++c)
        if (c < L.rows && L.row0 + c == r) v[r] = w[c];
  }
  return true;
}

template <int MODE, class Args>
__global__ void __launch_bounds__(256) sample_plan_kernel(Args args) {
  const PlanArgs& a = plan_args(args);
  const unsigned i = blockIdx.x * 256u + threadIdx.x;       // (unsigned: the last workgroup of a 2^31 - 1 point draw)
  float v[NDQ_TABLE_MAX_AXES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (!plan_point<MODE>(args, i, v)) return;
  // (fill_plan_args: the leaves of every segment cover the rows 0 .. d - 1, each once -- every point has all d rows)
#pragma unroll
  for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c)
    if (c < a.d) a.coords[(size_t)c * a.ldc + i] = v[c];
}

// validated launch arguments of one plan draw; returns 0 or NDQ_EINVAL (nothing is launched on NDQ_EINVAL)
inline int fill_plan_args(PlanArgs& a, const ndq_plan_sampler_desc* p, unsigned long long seed, unsigned long long draw,
                          unsigned stream_id, float* coords, int ldc) {
  if (!p || !coords || p->d < 1 || p->d > NDQ_TABLE_MAX_AXES) return NDQ_EINVAL;
  if (p->n_leaves < 1 || p->n_leaves > NDQ_PLAN_MAX_LEAVES || p->n_segments < 1 || p->n_segments > p->n_leaves) return NDQ_EINVAL;
  a = PlanArgs{};                                           // (unused leaf records: zeros, not stack bytes)
  long long total = 0;
  int next_leaf = 0;
  for (int s = 0; s < p->n_segments; ++s) {
    const ndq_plan_segment& g = p->seg[s];
    if (g.mode != NDQ_SEG_LEAF && g.mode != NDQ_SEG_ENSEMBLE && g.mode != NDQ_SEG_MESH) return NDQ_EINVAL;
    if (g.first != next_leaf || g.count < 1 || g.count > p->n_leaves - next_leaf) return NDQ_EINVAL;
    if (g.mode == NDQ_SEG_LEAF && g.count != 1) return NDQ_EINVAL;
    if (g.size < 1 || g.offset != total) return NDQ_EINVAL;
    unsigned covered = 0;
    long long product = 1;
    for (int l = g.first; l < g.first + g.count; ++l) {
      const ndq_plan_leaf& f = p->leaf[l];
      PlanLeaf& o = a.leaf[l];
      long long n = 0;
      // (each leaf's own validation: its size is the `total` of its launch arguments; the block is not written here)
      if (f.kind == NDQ_LEAF_SIMPLE) {
        SampleArgs t;
        if (fill_sample_args(t, &f.u.simple, seed, draw, stream_id, coords, 0x7fffffff) || f.rows != f.u.simple.d) return NDQ_EINVAL;
        n = t.total;
        o.noisy = f.u.simple.kind != NDQ_SAMPLE_GRID;
        for (int c = 0; c < f.rows; ++c) o.noisy |= f.u.simple.noise_std[c] != 0.0f;
        o.u.simple = f.u.simple;
      } else if (f.kind == NDQ_LEAF_TABLE) {
        TableArgs t;
        if (fill_table_args(t, &f.u.table, seed, draw, stream_id, coords, 0x7fffffff) || f.rows != f.u.table.d) return NDQ_EINVAL;
        n = t.total;
        o.noisy = t.noisy;
        o.u.table = f.u.table;
      } else if (f.kind == NDQ_LEAF_DATA) {
        if (f.rows < 1 || f.rows > NDQ_TABLE_MAX_AXES || f.n < 1) return NDQ_EINVAL;
        for (int c = 0; c < NDQ_TABLE_MAX_AXES; ++c) {
          if (c < f.rows && !f.u.data[c]) return NDQ_EINVAL;
          o.u.data[c] = c < f.rows ? f.u.data[c] : nullptr;
        }
        n = f.n;
        o.noisy = 0;
      } else {
        return NDQ_EINVAL;
      }
      if (f.row0 < 0 || f.row0 + f.rows > p->d) return NDQ_EINVAL;
      const unsigned mask = ((1u << f.rows) - 1u) << f.row0;
      if (covered & mask) return NDQ_EINVAL;
      covered |= mask;
      if (g.mode == NDQ_SEG_MESH) {
        if (f.rows != 1) return NDQ_EINVAL;
        product *= n;
        if (product > 0x7fffffffLL) return NDQ_EINVAL;
      } else if (n != g.size) {
        return NDQ_EINVAL;
      }
      const unsigned long long key = seed + (unsigned long long)l * 0x9E3779B97F4A7C15ull;
      o.kind = f.kind; o.row0 = f.row0; o.rows = f.rows;
      o.off = (unsigned)g.offset; o.size = (unsigned)g.size;
      o.div = 0u; o.n = (unsigned)n;
      o.k0 = (unsigned)key; o.k1 = (unsigned)(key >> 32);
    }
    if (covered != (1u << p->d) - 1u) return NDQ_EINVAL;
    if (g.mode == NDQ_SEG_MESH) {
      if (product != g.size) return NDQ_EINVAL;
      unsigned div = 1u;                                    // last factor fastest
      for (int l = g.first + g.count - 1; l >= g.first; --l) { a.leaf[l].div = div; div *= a.leaf[l].n; }
    }
    next_leaf += g.count;
    total += g.size;
    if (total > 0x7fffffffLL) return NDQ_EINVAL;
  }
  if (next_leaf != p->n_leaves || ldc < total) return NDQ_EINVAL;
  a.n_leaves = p->n_leaves;
  a.c1 = (unsigned)draw; a.c2 = (unsigned)(draw >> 32); a.c3 = stream_id;
  a.coords = coords; a.ldc = ldc; a.total = (int)total; a.d = p->d;
  return 0;
}

inline int launch_sample_plan(const ndq_plan_sampler_desc* p, unsigned long long seed, unsigned long long draw,
                              unsigned stream_id, float* coords, int ldc, hipStream_t stream) {
  PlanArgs a;
  const int rc = fill_plan_args(a, p, seed, draw, stream_id, coords, ldc);
  if (rc) return rc;
  hipLaunchKernelGGL((sample_plan_kernel<NDQ_INDEX_PLAIN, PlanArgs>), dim3(((unsigned)a.total + 255u) / 256u), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

// ----------------------------------------------------------------------------------------------- indexed plan sampler
// include/ndq.h: ndq_sample_plan_indexed.  ResampleGenerator / BatchGenerator directly above a plan: output point i is element
// r of inner draw k (the window), r is mapped to the plan point j (the index map), and the plan's own per-point body runs
// at j with k as the draw number.  Philox is counter-based, so nothing is drawn twice and nothing is gathered.
struct PlanIndexArgs {             // by value: PlanArgs + 40 bytes
  PlanArgs p;                      // p.total = n, the points of the plan; p.c1 / p.c2 are not used (k replaces the draw number)
  unsigned long long k0;           // inner draw of output point 0
  unsigned r0, m, n, rounds;       // its element there; points of one inner draw; plan points; PERMUTE: 2 bitlen(n - 1) + 8
  unsigned s0, s1;                 // the index key: seed + 8 * 0x9E3779B97F4A7C15
  int out;                         // output points
};
static_assert(sizeof(PlanIndexArgs) <= 2112, "PlanIndexArgs is passed by value");
#define NDQ_INDEX_MAX_ROUNDS 70    // n <= 2^31 - 1: 2 * 31 + 8

__host__ __device__ inline unsigned fmix32(unsigned h) {   // the murmur3 finaliser
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// (K_q, S_q) of round q of the swap-or-not shuffle of inner draw k: a function of (k, q) only
__device__ __forceinline__ uint2 index_round_key(const PlanIndexArgs& a, unsigned q, unsigned c1, unsigned c2) {
  const U4 b = philox4x32_10(U4{q | 0x80000000u, c1, c2, a.p.c3}, a.s0, a.s1);
  return make_uint2(__umulhi(b.x, a.n), b.y);
}

// one round: x and p = (K - x) mod n are partners (the round is an involution), the pair's coin decides for both
__device__ __forceinline__ unsigned swap_or_not(unsigned x, uint2 ks, unsigned n) {
  const unsigned p = ks.x >= x ? ks.x - x : ks.x + n - x;
  return (fmix32(max(x, p) ^ ks.y) & 0x80000000u) ? p : x;
}

__device__ __forceinline__ const PlanArgs& plan_args(const PlanIndexArgs& a) { return a.p; }

// Output point i of sample_plan_kernel<MODE, PlanIndexArgs>: window -> index map -> (plan point pt, counter words c1 / c2 of
// its inner draw); false: i is past the last output point.  PERMUTE: the trip count `rounds` is wave-uniform and fixed by n (no
// data-dependent loop).  The round keys depend on (k, q) only, so a workgroup all of whose points lie in ONE inner draw lets
// thread q compute round q once into LDS (rounds x 8 bytes; every lane then reads the same address: a broadcast); a workgroup
// that straddles an inner-draw boundary computes them per thread (same numbers).  Which of the two is decided from blockIdx
// and launch arguments alone: workgroup-uniform, so the barrier is reached by all threads or by none, before any returns.
template <int MODE>
struct PlanIndexPoint {
  static __device__ __forceinline__ bool map(const PlanIndexArgs& a, unsigned i, unsigned& pt, unsigned& c1, unsigned& c2) {
    const unsigned u = a.r0 + i;                            // (r0 < m <= 2^31 - 1, i < 2^31 + 255: no wrap)
    const unsigned ki = u / a.m, r = u - ki * a.m;
    const unsigned long long k = a.k0 + ki;
    c1 = (unsigned)k; c2 = (unsigned)(k >> 32);
    pt = r;
    if constexpr (MODE == NDQ_INDEX_REPLACE) {
      pt = __umulhi(philox4x32_10(U4{r, c1, c2, a.p.c3}, a.s0, a.s1).x, a.n);
    } else if constexpr (MODE == NDQ_INDEX_PERMUTE) {
      __shared__ uint2 keys[NDQ_INDEX_MAX_ROUNDS + 2];
      const unsigned u_first = a.r0 + blockIdx.x * 256u;
      const unsigned u_last = min(u_first + 255u, a.r0 + (unsigned)a.out - 1u);
      const bool one_draw = u_first / a.m == u_last / a.m;
      if (one_draw) {
        const unsigned long long kw = a.k0 + u_first / a.m;
        if (threadIdx.x < a.rounds) keys[threadIdx.x] = index_round_key(a, threadIdx.x, (unsigned)kw, (unsigned)(kw >> 32));
        __syncthreads();
      }
      if (i >= (unsigned)a.out) return false;
      unsigned x = r;
      if (one_draw) {
        for (unsigned q = 0; q < a.rounds; ++q) x = swap_or_not(x, keys[q], a.n);
      } else {
        for (unsigned q = 0; q < a.rounds; ++q) x = swap_or_not(x, index_round_key(a, q, c1, c2), a.n);
      }
      pt = x;
    }
    return i < (unsigned)a.out;
  }
};

// validated launch arguments of one indexed plan draw; returns 0 or NDQ_EINVAL (nothing is launched on NDQ_EINVAL)
inline int fill_plan_index_args(PlanIndexArgs& a, const ndq_plan_sampler_desc* p, const ndq_plan_index_desc* ix, unsigned long long seed,
                                unsigned long long draw, unsigned stream_id, float* coords, int ldc) {
  // (the plan itself: as for ndq_sample_plan; its `ldc >= n` does not apply -- the block holds the OUTPUT points)
  const int rc = fill_plan_args(a.p, p, seed, draw, stream_id, coords, 0x7fffffff);
  if (rc) return rc;
  if (!ix) return NDQ_EINVAL;
  const int n = a.p.total;
  if (ix->mode != NDQ_INDEX_NONE && ix->mode != NDQ_INDEX_PERMUTE && ix->mode != NDQ_INDEX_REPLACE) return NDQ_EINVAL;
  if (ix->m < 1 || ix->batch < 0) return NDQ_EINVAL;
  if (ix->mode == NDQ_INDEX_PERMUTE && ix->m > n) return NDQ_EINVAL;
  if (ix->mode == NDQ_INDEX_NONE && ix->m != n) return NDQ_EINVAL;
  const int out = ix->batch ? ix->batch : ix->m;
  if (ldc < out) return NDQ_EINVAL;
  a.p.ldc = ldc;
  a.m = (unsigned)ix->m; a.n = (unsigned)n; a.out = out;
  if (ix->batch) {
    const unsigned long long g0 = draw * (unsigned long long)ix->batch;
    a.k0 = g0 / a.m; a.r0 = (unsigned)(g0 % a.m);
  } else {
    a.k0 = draw; a.r0 = 0u;
  }
  unsigned bits = 0u;
  for (unsigned v = a.n - 1u; v; v >>= 1) ++bits;
  a.rounds = 2u * bits + 8u;
  const unsigned long long key = seed + 8ull * 0x9E3779B97F4A7C15ull;
  a.s0 = (unsigned)key; a.s1 = (unsigned)(key >> 32);
  return 0;
}

inline int launch_sample_plan_indexed(const ndq_plan_sampler_desc* p, const ndq_plan_index_desc* ix, unsigned long long seed,
                                      unsigned long long draw, unsigned stream_id, float* coords, int ldc, hipStream_t stream) {
  PlanIndexArgs a;
  const int rc = fill_plan_index_args(a, p, ix, seed, draw, stream_id, coords, ldc);
  if (rc) return rc;
  const dim3 grid(((unsigned)a.out + 255u) / 256u), block(256);
  if (ix->mode == NDQ_INDEX_PERMUTE) hipLaunchKernelGGL((sample_plan_kernel<NDQ_INDEX_PERMUTE, PlanIndexArgs>), grid, block, 0, stream, a);
  else if (ix->mode == NDQ_INDEX_REPLACE) hipLaunchKernelGGL((sample_plan_kernel<NDQ_INDEX_REPLACE, PlanIndexArgs>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((sample_plan_kernel<NDQ_INDEX_NONE, PlanIndexArgs>), grid, block, 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ndq
