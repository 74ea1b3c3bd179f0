// bdl_fn.hip — the function-space fold of stacked chains: the K chains' probe
// logits to class probabilities, folded into the batch-means accumulators of
// bdl_ess.h (include/bdl_fn.h: the arithmetic contract, the geometry).
//
// Two kernel templates over the chains * probe rows, grid-strided.
// bdl_fn_wave_kernel (classes <= 256): a wave owns a row, lane l its 16-B class
// group l, everything stays in registers and the two row reductions are wave
// butterflies.  bdl_fn_block_kernel: the workgroup owns a row, thread t its
// class groups t, t + 256, ...; a group's e is parked in LDS between the two
// workgroup reductions (max, then the fp64 sum) and read back by the thread
// that wrote it, so the only barriers are the reductions' own.  The fold's
// flags are template parameters, as in bdl_ess.hip: a vector a fold does not
// need appears in no instruction.  VEC (classes % 4 == 0): every row of the
// logits, of probs and of the accumulators is 16-B aligned and whole groups
// move as non-temporal 16-B accesses; otherwise element by element.
#include "bdl_chain_elem.hpp"
#include "bdl_fn.h"

namespace bdl {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kFnBpc = 4;  // default workgroups per CU

struct NArgs {
  const float* __restrict__ logits;
  float* __restrict__ bsum;
  float* __restrict__ smean;
  float* __restrict__ sM2;
  float* __restrict__ bM2;
  float* __restrict__ probs;
  int64_t rows;   // chains * probe
  int64_t probe;
  int64_t slot;   // elements per chain slot, 4 * chain_groups
  int32_t classes;
  float fs, fb, c;
};

// Class group at c0 of a row; a class >= C reads as a masked one (-inf).
template <bool VEC>
__device__ __forceinline__ f4v load_group(const float* __restrict__ row, int c0, int C) {
  const float ninf = -__builtin_inff();
  f4v v = {ninf, ninf, ninf, ninf};
  if constexpr (VEC) {
    v = vload(row + c0);
  } else {
    if (c0 + 0 < C) v.x = sload(row + c0 + 0);
    if (c0 + 1 < C) v.y = sload(row + c0 + 1);
    if (c0 + 2 < C) v.z = sload(row + c0 + 2);
    if (c0 + 3 < C) v.w = sload(row + c0 + 3);
  }
  return v;
}

// Four elements at p (VEC: one 16-B access; else those below `left`).
template <bool VEC>
__device__ __forceinline__ f4v acc_load(const float* __restrict__ p, int left) {
  if constexpr (VEC) {
    return vload(p);
  } else {
    f4v v = {0.f, 0.f, 0.f, 0.f};
    if (0 < left) v.x = sload(p + 0);
    if (1 < left) v.y = sload(p + 1);
    if (2 < left) v.z = sload(p + 2);
    if (3 < left) v.w = sload(p + 3);
    return v;
  }
}

template <bool VEC>
__device__ __forceinline__ void acc_store(float* __restrict__ p, int left, f4v v) {
  if constexpr (VEC) {
    vstore(p, v);
  } else {
    if (0 < left) sstore(p + 0, v.x);
    if (1 < left) sstore(p + 1, v.y);
    if (2 < left) sstore(p + 2, v.z);
    if (3 < left) sstore(p + 3, v.w);
  }
}

// The probabilities of class group c0 of row r (accumulator offset o of the
// row's first class) out and into the accumulators.
template <int FLAGS, bool VEC>
__device__ __forceinline__ void fold_probs(const NArgs& a, int64_t r, int64_t o, int c0, f4v p) {
  constexpr bool kFirstSample = FLAGS & BDL_ESS_FIRST_SAMPLE;
  constexpr bool kFirstInBatch = FLAGS & BDL_ESS_FIRST_IN_BATCH;
  constexpr bool kClose = FLAGS & BDL_ESS_CLOSE;
  constexpr bool kFirstBatch = FLAGS & BDL_ESS_FIRST_BATCH;
  const int left = a.classes - c0;  // classes of this group (>= 4: all)
  const int64_t e = o + c0;
  if (a.probs) acc_store<VEC>(a.probs + r * a.classes + c0, left, p);
  const f4v z = {0.f, 0.f, 0.f, 0.f};
  f4v sm = z, M = z, bs = z, B = z;
  if constexpr (!kFirstSample) {
    sm = acc_load<VEC>(a.smean + e, left);
    M = acc_load<VEC>(a.sM2 + e, left);
  }
  if constexpr (!kFirstInBatch) bs = acc_load<VEC>(a.bsum + e, left);
  if constexpr (kClose && !kFirstBatch) B = acc_load<VEC>(a.bM2 + e, left);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s1 = sm[j], m2 = M[j], b1 = bs[j], b2 = B[j];
    ess_fold_elem<FLAGS>(p[j], s1, m2, b1, b2, a.fs, a.fb, a.c);
    sm[j] = s1;
    M[j] = m2;
    bs[j] = b1;
    B[j] = b2;
  }
  acc_store<VEC>(a.smean + e, left, sm);
  acc_store<VEC>(a.sM2 + e, left, M);
  if constexpr (kClose)
    acc_store<VEC>(a.bM2 + e, left, B);
  else
    acc_store<VEC>(a.bsum + e, left, bs);
}

// A group's contribution to the row's maximum; a NaN or a +inf sets the flag.
__device__ __forceinline__ void group_max(const f4v x, float& m, int& nonf) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v = x[j];
    if (v != v || v == __builtin_inff())
      nonf = 1;
    else if (v > m)
      m = v;
  }
}

// e = expf(x - m) of a group; its four e added to z in element order.
__device__ __forceinline__ f4v group_exp(const f4v x, float m, double& z) {
  f4v e;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float d = x[j] - m;
    const float ex = expf(d);
    e[j] = ex;
    z += (double)ex;
  }
  return e;
}

__device__ __forceinline__ f4v group_probs(const f4v e, double rz, bool bad) {
  const float fnan = __builtin_nanf("");
  f4v p;
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = bad ? fnan : (float)((double)e[j] * rz);
  return p;
}

__device__ __forceinline__ void wave_max(float& m, int& nonf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off, 64);
    nonf |= __shfl_xor(nonf, off, 64);
    if (om > m) m = om;
  }
}

// Accumulator offset of row r's first class.
__device__ __forceinline__ int64_t row_offset(const NArgs& a, int64_t r) {
  const int64_t k = r / a.probe, b = r - k * a.probe;
  return k * a.slot + b * a.classes;
}

// One wave per row: rows 4 * blockIdx.x + wave, then grid-strided.
template <int FLAGS, bool VEC>
__global__ __launch_bounds__(kBlock) void bdl_fn_wave_kernel(const NArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int C = a.classes, c0 = 4 * lane;
  const bool mine = c0 < C;  // lanes past the last class group idle
  const float ninf = -__builtin_inff();
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < a.rows; r += stride) {
    f4v x = {ninf, ninf, ninf, ninf};
    if (mine) x = load_group<VEC>(a.logits + r * C, c0, C);
    float m = ninf;
    int nonf = 0;
    group_max(x, m, nonf);
    wave_max(m, nonf);
    const bool bad = nonf || m == ninf;  // uniform over the wave
    double z = 0.0;
    const f4v e = group_exp(x, m, z);
    z = wave_sum(z);
    const double rz = 1.0 / z;
    if (mine) fold_probs<FLAGS, VEC>(a, r, row_offset(a, r), c0, group_probs(e, rz, bad));
  }
}

// One workgroup per row: rows blockIdx.x, then grid-strided.  s_e[q] belongs to
// the thread q % 256 alone.  The two reduction buffers alternate along the
// row's barriers: one is rewritten only after the other's barrier, which every
// thread passes after its reads of the first.
template <int FLAGS, bool VEC>
__global__ __launch_bounds__(kBlock) void bdl_fn_block_kernel(const NArgs a) {
  __shared__ f4v s_e[BDL_FN_MAX_CLASSES / 4];
  __shared__ float s_m[kWaves];
  __shared__ int s_f[kWaves];
  __shared__ double s_z[kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int C = a.classes, Q = (C + 3) >> 2;  // class groups of a row
  const float ninf = -__builtin_inff();
  for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
    const float* __restrict__ row = a.logits + r * C;
    float m = ninf;
    int nonf = 0;
    for (int q = t; q < Q; q += kBlock) {
      const f4v x = load_group<VEC>(row, 4 * q, C);
      s_e[q] = x;
      group_max(x, m, nonf);
    }
    wave_max(m, nonf);
    if (lane == 0) {
      s_m[w] = m;
      s_f[w] = nonf;
    }
    __syncthreads();
    m = s_m[0];
    nonf = s_f[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      if (s_m[k] > m) m = s_m[k];
      nonf |= s_f[k];
    }
    const bool bad = nonf || m == ninf;  // uniform over the workgroup
    double z = 0.0;
    for (int q = t; q < Q; q += kBlock) s_e[q] = group_exp(s_e[q], m, z);
    z = wave_sum(z);
    if (lane == 0) s_z[w] = z;
    __syncthreads();
    z = s_z[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) z += s_z[k];
    const double rz = 1.0 / z;
    const int64_t o = row_offset(a, r);
    for (int q = t; q < Q; q += kBlock)
      fold_probs<FLAGS, VEC>(a, r, o, 4 * q, group_probs(s_e[q], rz, bad));
  }
}

static_assert(BDL_FN_WAVE_CLASSES == 4 * 64, "a wave's lanes own one class group each");
static_assert(BDL_FN_MAX_CLASSES % 4 == 0, "whole class groups in LDS");

typedef void (*FnKernel)(const NArgs);

template <int FLAGS>
FnKernel pick_geometry(bool vec, bool wave) {
  if (wave) return vec ? bdl_fn_wave_kernel<FLAGS, true> : bdl_fn_wave_kernel<FLAGS, false>;
  return vec ? bdl_fn_block_kernel<FLAGS, true> : bdl_fn_block_kernel<FLAGS, false>;
}

// the flag sets a (sample, batch) pair can imply (bdl_ess.hip's)
FnKernel pick_fn(int flags, bool vec, bool wave) {
  switch (flags) {
    case 0: return pick_geometry<0>(vec, wave);
    case BDL_ESS_FIRST_IN_BATCH: return pick_geometry<BDL_ESS_FIRST_IN_BATCH>(vec, wave);
    case BDL_ESS_CLOSE: return pick_geometry<BDL_ESS_CLOSE>(vec, wave);
    case BDL_ESS_CLOSE | BDL_ESS_FIRST_BATCH:
      return pick_geometry<BDL_ESS_CLOSE | BDL_ESS_FIRST_BATCH>(vec, wave);
    case BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE:
      return pick_geometry<BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE>(vec, wave);
    case BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH:
      return pick_geometry<BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH>(vec, wave);
    case BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE | BDL_ESS_FIRST_BATCH:
      return pick_geometry<BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE |
                           BDL_ESS_FIRST_BATCH>(vec, wave);
    default: return nullptr;
  }
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int bdl_fn_fold(const bdl_fn_fold_args* d, void* stream) {
  const std::string me = "bdl_fn_fold: ";
  if (const int rc = no_redirect("bdl_fn_fold")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->logits) return fail(BDL_ERR_NULL, me + "null logits");
  if (!d->smean || !d->sM2 || !d->bM2)
    return fail(BDL_ERR_NULL, me + "smean, sM2 and bM2 are required");
  if (d->chains < 1 || d->chains > BDL_ESS_MAX_CHAINS)
    return fail(BDL_ERR_ARG, me + "chains must be in [1, 65535]");
  if (d->probe < 1) return fail(BDL_ERR_ARG, me + "probe must be >= 1");
  if (d->classes < 1 || d->classes > BDL_FN_MAX_CLASSES)
    return fail(BDL_ERR_ARG, me + "classes in [1, " + std::to_string(BDL_FN_MAX_CLASSES) + "]");
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_FN_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_FN_MAX_GRID) + "]");
  // every byte offset of logits fits int64
  if (d->probe > INT64_MAX / 4 / d->classes / d->chains)
    return fail(BDL_ERR_ARG, me + "chains * probe * classes overflows the element index");
  const int64_t n = d->probe * d->classes;
  if (const char* why = stacked_slot_error(d->chains, n, d->chain_groups))
    return fail(BDL_ERR_ARG, me + why);
  if (d->batch < 1 || d->batch >= BDL_ESS_MAX_COUNT)
    return fail(BDL_ERR_ARG, me + "batch must be in [1, 2^24)");
  if (d->sample < 1 || d->sample >= BDL_ESS_MAX_COUNT)
    return fail(BDL_ERR_ARG, me + "sample must be in [1, 2^24)");
  if (d->batch > 1 && !d->bsum) return fail(BDL_ERR_NULL, me + "bsum is required with batch > 1");
  const int64_t s = d->sample, b = d->batch, p = (s - 1) % b + 1;
  const int want = (s == 1 ? BDL_ESS_FIRST_SAMPLE : 0) | (p == 1 ? BDL_ESS_FIRST_IN_BATCH : 0) |
                   (p == b ? BDL_ESS_CLOSE : 0) | (s == b ? BDL_ESS_FIRST_BATCH : 0);
  if (d->flags != want)
    return fail(BDL_ERR_ARG, me + "flags " + std::to_string(d->flags) + " are not what sample " +
                std::to_string(s) + " of batch " + std::to_string(b) + " implies (" +
                std::to_string(want) + ")");
  if (d->fs != (float)s || d->fb != (float)b)
    return fail(BDL_ERR_ARG, me + "fs / fb are not fl32(sample) / fl32(batch)");
  if ((want & BDL_ESS_CLOSE) && !(want & BDL_ESS_FIRST_BATCH)) {
    const int64_t i = s / b;
    if (d->c != (float)((double)i / (double)(i - 1)))
      return fail(BDL_ERR_ARG, me + "c is not fl32(i/(i-1)) of the batch being closed");
  }
  float* const bsum = b > 1 ? d->bsum : nullptr;  // never touched at batch == 1
  struct Span {
    const char* name;
    const void* p;
    uint64_t bytes;
  };
  const uint64_t lb = 4 * (uint64_t)d->chains * (uint64_t)n;
  const uint64_t ab = 4 * (4 * d->chain_groups * (uint64_t)(d->chains - 1) + (uint64_t)n);
  const Span spans[] = {{"logits", d->logits, lb}, {"probs", d->probs, lb}, {"bsum", bsum, ab},
                        {"smean", d->smean, ab},   {"sM2", d->sM2, ab},     {"bM2", d->bM2, ab}};
  constexpr int kSpans = (int)(sizeof(spans) / sizeof(spans[0]));
  for (const Span& v : spans)
    if (misaligned(v.p, 15)) return fail(BDL_ERR_ALIGN, me + v.name + " not 16-B aligned");
  for (int i = 1; i < kSpans; ++i)
    for (int j = 0; j < i; ++j)
      if (overlap(spans[i].p, spans[j].p, spans[i].bytes, spans[j].bytes))
        return fail(BDL_ERR_ARG, me + spans[i].name + " overlaps " + spans[j].name);
  const bool wave = d->classes <= BDL_FN_WAVE_CLASSES;
  FnKernel k = pick_fn(want, d->classes % 4 == 0, wave);
  if (!k) return fail(BDL_ERR_ARG, me + "no kernel for these flags");

  NArgs a;
  a.logits = d->logits;
  a.bsum = bsum;
  a.smean = d->smean;
  a.sM2 = d->sM2;
  a.bM2 = d->bM2;
  a.probs = d->probs;
  a.rows = (int64_t)d->chains * d->probe;
  a.probe = d->probe;
  a.slot = (int64_t)(4 * d->chain_groups);
  a.classes = d->classes;
  a.fs = d->fs;
  a.fb = d->fb;
  a.c = d->c;
  const int64_t rpb = wave ? kWaves : 1;  // rows per workgroup trip
  const int64_t cap = d->grid_blocks > 0
                          ? d->grid_blocks
                          : std::min<int64_t>((int64_t)cu_count() * kFnBpc, BDL_FN_MAX_GRID);
  const int grid = (int)capped_grid((a.rows + rpb - 1) / rpb, cap);
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
  return launched("bdl_fn_fold");
}

}  // extern "C"
