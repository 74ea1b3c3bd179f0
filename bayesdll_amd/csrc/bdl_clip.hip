// bdl_clip.hip — per-chain clip_grad_norm_ of stacked chains
// (include/bdl_clip.h: the arithmetic, the segment form, the alignment rule).
//
// Both sweeps run on a (blocks_per_chain, K) grid: blockIdx.y is the chain, so
// a workgroup never leaves its chain, its partial sum belongs to one chain and
// no lane looks a chain up.  A workgroup walks the segment table (wave-uniform
// loads of 24-B entries) and, in every segment, takes its share of the chain's
// slice: the 16-B aligned body in block iterations of kBlock x 4 float4 groups
// (four non-temporal 16-B loads in flight per lane), grid-strided over the
// chain's workgroups, the first of which is rotated by the segment index so
// that a table of many small tensors does not pile up on workgroup 0; the (up
// to 3) unaligned elements before and after the body go to three lanes each of
// that first workgroup.  The norm is reduced like the clip norm of
// bdl_api.hip: per-lane fp64 fma accumulators, a 64-lane butterfly
// (bdl_chain_common.hpp's wave_sum), the 4 waves through LDS, one partial per
// workgroup written with an ordinary store, then
// one workgroup per chain that combines the chain's partials in a fixed order.
// No atomics, no host synchronisation, no allocation.
#include "bdl_chain_common.hpp"
#include "bdl_clip.h"

namespace bdl {
namespace {

constexpr int kClipUnroll = 4;                                 // float4 groups in flight per lane
constexpr int64_t kClipIter = (int64_t)kBlock * kClipUnroll;   // groups per block iteration
constexpr int kClipWgPerCu = 4;                                // default grid: this many per CU

// Chain k's slice of a segment: `head` elements up to the first 16-B
// boundary, `nbody` float4 groups from `body` on, `tail` elements after them.
struct Slice {
  float* p;
  float* body;
  int64_t nbody;
  int head, tail;
};

__device__ __forceinline__ Slice slice_of(const bdl_clip_segment& s, int k) {
  Slice c;
  c.p = s.base + (int64_t)k * s.chain_stride;
  const int64_t mis = (int64_t)((reinterpret_cast<uintptr_t>(c.p) >> 2) & 3u);
  const int64_t h0 = (4 - mis) & 3;
  const int64_t h = h0 < s.numel ? h0 : s.numel;
  c.head = (int)h;
  c.body = c.p + h;
  c.nbody = (s.numel - h) >> 2;
  c.tail = (int)(s.numel - h - 4 * c.nbody);
  return c;
}

// The block's sum in thread 0 (4 waves through LDS, in wave order).
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double s_wave[kBlock / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) t += s_wave[w];
  }
  return t;
}

__device__ __forceinline__ double sq4(f4v v, double acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = fma((double)v[j], (double)v[j], acc);
  return acc;
}

// partials[k * gridDim.x + b]: workgroup b's share of chain k's sum of squares.
__global__ __launch_bounds__(kBlock) void bdl_chain_sqnorm_kernel(
    const bdl_clip_segment* __restrict__ segs, int nseg, double* __restrict__ partials) {
  const int k = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * kClipIter;
  double acc = 0.0;
  for (int i = 0; i < nseg; ++i) {
    const Slice c = slice_of(segs[i], k);
    const uint32_t b = rotated_block(i);
    int64_t gb = (int64_t)b * kClipIter;
    for (; gb + kClipIter <= c.nbody; gb += stride) {
      f4v v[kClipUnroll];
#pragma unroll
      for (int u = 0; u < kClipUnroll; ++u)
        v[u] = vload(c.body + 4 * (gb + (int64_t)u * kBlock + threadIdx.x));
#pragma unroll
      for (int u = 0; u < kClipUnroll; ++u) acc = sq4(v[u], acc);
    }
    if (gb < c.nbody) {  // at most one partial iteration per workgroup and segment
#pragma unroll
      for (int u = 0; u < kClipUnroll; ++u) {
        const int64_t gi = gb + (int64_t)u * kBlock + threadIdx.x;
        if (gi < c.nbody) acc = sq4(vload(c.body + 4 * gi), acc);
      }
    }
    if (b == 0) {
      const int t = threadIdx.x;
      if (t < c.head) {
        const float x = sload(c.p + t);
        acc = fma((double)x, (double)x, acc);
      } else if (t >= 4 && t - 4 < c.tail) {
        const float x = sload(c.body + 4 * c.nbody + (t - 4));
        acc = fma((double)x, (double)x, acc);
      }
    }
  }
  const double t = block_sum(acc);
  if (threadIdx.x == 0) partials[(int64_t)k * gridDim.x + blockIdx.x] = t;
}

// One workgroup per chain: the chain's partials in a fixed order (thread t
// takes t, t + 256, ...; the butterfly; the waves in order), then
// bdl_clip_finalize_kernel's norm and coefficient.
__global__ __launch_bounds__(kBlock) void bdl_chain_clip_finalize_kernel(
    const double* __restrict__ partials, int nparts, float max_norm, float* __restrict__ out) {
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kBlock) acc += partials[(int64_t)k * nparts + i];
  const double t = block_sum(acc);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(t);
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6) (Tensor.__rtruediv__
    // = reciprocal() * other), clamped at 1.0
    float coef = (1.0f / (norm + 1e-6f)) * max_norm;
    coef = fminf(coef, 1.0f);
    out[2 * k] = norm;
    out[2 * k + 1] = coef;
  }
}

__device__ __forceinline__ f4v scale4(f4v v, float coef) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = v[j] * coef;
  return v;
}

// g <- g * coef_k in place, the norm sweep's traversal; a chain that is not
// clipped is left after one scalar read.
__global__ __launch_bounds__(kBlock) void bdl_chain_scale_kernel(
    const bdl_clip_segment* __restrict__ segs, int nseg, const float* __restrict__ out) {
  const int k = blockIdx.y;
  const float coef = out[2 * k + 1];
  if (!(coef < 1.0f)) return;
  const int64_t stride = (int64_t)gridDim.x * kClipIter;
  for (int i = 0; i < nseg; ++i) {
    const Slice c = slice_of(segs[i], k);
    const uint32_t b = rotated_block(i);
    int64_t gb = (int64_t)b * kClipIter;
    for (; gb + kClipIter <= c.nbody; gb += stride) {
      f4v v[kClipUnroll];
#pragma unroll
      for (int u = 0; u < kClipUnroll; ++u)
        v[u] = vload(c.body + 4 * (gb + (int64_t)u * kBlock + threadIdx.x));
#pragma unroll
      for (int u = 0; u < kClipUnroll; ++u)
        vstore(c.body + 4 * (gb + (int64_t)u * kBlock + threadIdx.x), scale4(v[u], coef));
    }
    if (gb < c.nbody) {
#pragma unroll
      for (int u = 0; u < kClipUnroll; ++u) {
        const int64_t gi = gb + (int64_t)u * kBlock + threadIdx.x;
        if (gi < c.nbody) vstore(c.body + 4 * gi, scale4(vload(c.body + 4 * gi), coef));
      }
    }
    if (b == 0) {
      const int t = threadIdx.x;
      if (t < c.head) {
        sstore(c.p + t, sload(c.p + t) * coef);
      } else if (t >= 4 && t - 4 < c.tail) {
        float* q = c.body + 4 * c.nbody + (t - 4);
        sstore(q, sload(q) * coef);
      }
    }
  }
}

int64_t coef_bytes(int32_t chains) { return ((int64_t)chains * 8 + 15) & ~(int64_t)15; }

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_chain_clip_workspace_bytes(int32_t chains) {
  if (chains < 1 || chains > BDL_CLIP_MAX_CHAINS) return 0;
  return coef_bytes(chains) +
         (int64_t)chains * BDL_CLIP_MAX_BLOCKS_PER_CHAIN * (int64_t)sizeof(double);
}

int bdl_chain_clip(const bdl_chain_clip_args* d, void* stream) {
  if (const int rc = no_redirect("bdl_chain_clip")) return rc;
  if (!d) return fail(BDL_ERR_NULL, "bdl_chain_clip: null args");
  if (!d->segments) return fail(BDL_ERR_NULL, "bdl_chain_clip: null segments");
  if (!d->workspace) return fail(BDL_ERR_NULL, "bdl_chain_clip: null workspace");
  if (misaligned(d->workspace, 15))
    return fail(BDL_ERR_ALIGN, "bdl_chain_clip: workspace not 16-B aligned");
  if (misaligned(d->segments, 7))
    return fail(BDL_ERR_ALIGN, "bdl_chain_clip: segments not 8-B aligned");
  if (d->chains < 1 || d->chains > BDL_CLIP_MAX_CHAINS)
    return fail(BDL_ERR_ARG, "bdl_chain_clip: chains in [1, " +
                std::to_string(BDL_CLIP_MAX_CHAINS) + "]");
  if (d->nsegments < 1 || d->nsegments > BDL_CLIP_MAX_SEGMENTS)
    return fail(BDL_ERR_ARG, "bdl_chain_clip: nsegments in [1, " +
                std::to_string(BDL_CLIP_MAX_SEGMENTS) + "]");
  if (!(d->max_norm > 0.0f)) return fail(BDL_ERR_ARG, "bdl_chain_clip: max_norm must be > 0");
  if (d->blocks_per_chain < 0 || d->blocks_per_chain > BDL_CLIP_MAX_BLOCKS_PER_CHAIN)
    return fail(BDL_ERR_ARG, "bdl_chain_clip: blocks_per_chain in [0, " +
                std::to_string(BDL_CLIP_MAX_BLOCKS_PER_CHAIN) + "]");

  int bpc = d->blocks_per_chain;
  if (bpc == 0)  // the table's sizes are on the device: fill the CUs, whatever it holds
    bpc = (int)blocks_per_chain(kClipWgPerCu, d->chains, BDL_CLIP_MAX_BLOCKS_PER_CHAIN);
  float* out = reinterpret_cast<float*>(d->workspace);
  double* partials =
      reinterpret_cast<double*>(reinterpret_cast<char*>(d->workspace) + coef_bytes(d->chains));
  const dim3 grid((unsigned)bpc, (unsigned)d->chains);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bdl_chain_sqnorm_kernel, grid, dim3(kBlock), 0, st, d->segments, d->nsegments,
                     partials);
  hipLaunchKernelGGL(bdl_chain_clip_finalize_kernel, dim3((unsigned)d->chains), dim3(kBlock), 0, st,
                     partials, bpc, d->max_norm, out);
  hipLaunchKernelGGL(bdl_chain_scale_kernel, grid, dim3(kBlock), 0, st, d->segments, d->nsegments,
                     out);
  return launched("bdl_chain_clip");
}

}  // extern "C"
