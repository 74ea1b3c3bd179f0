// bdl_rank.hip — exact rank statistics of score rows against 0 / 1 marks
// (include/bdl_rank.h: the definitions, the geometry, the order of ap_sum).
//
// Scores are compared through a signed integer key of their bits, monotone in
// the value (-0.0 folded onto +0.0), so that no floating-point mode touches a
// comparison; INT32_MIN is below every key (-inf is 0x807fffff) and stands for
// "no example": an excluded j, or one past the row.  The count kernel stages a
// tile of j as TWO key arrays — the positives' (kNone elsewhere) and the
// negatives' — so its inner loop needs no mark: per (i, j) three integer
// compares, each added to its counter.  All lanes read the same 16 B of LDS.
#include "bdl_chain_common.hpp"
#include "bdl_rank.h"

namespace bdl {
namespace {

constexpr int kU = BDL_RANK_U;
constexpr int kITile = BDL_RANK_ITILE;
constexpr int kJTile = BDL_RANK_JTILE;
constexpr int kWaves = kBlock / 64;
constexpr int32_t kNone = INT32_MIN;

typedef int32_t i4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) i4v gi4v;
typedef __attribute__((address_space(1))) int32_t gint;
typedef __attribute__((address_space(1))) uint32_t guint;

static_assert(kJTile == 4 * kBlock, "a thread stages one 16-B group of a tile");
static_assert(kITile == kU * kBlock, "a thread holds kU examples");

struct RArgs {
  const float* __restrict__ scores;
  const int32_t* __restrict__ marks;
  uint32_t* __restrict__ ge_pos;
  uint32_t* __restrict__ ge_neg;
  uint32_t* __restrict__ gt_neg;
  uint32_t* __restrict__ ws;  // [3][rows * n]: ge_pos, ge_neg, gt_neg
  int64_t n;
  int64_t plane;  // rows * n
  int32_t scores_per_group, mark_rows;
};

// The key of a score (any order-preserving map would do: only comparisons
// between keys of one row are made), or kNone for a NaN.
__device__ __forceinline__ int32_t key_of(float x) {
  int32_t b = __float_as_int(x);
  if ((b & 0x7fffffff) > 0x7f800000) return kNone;  // NaN
  if ((b & 0x7fffffff) == 0) b = 0;                 // -0.0 is +0.0
  return b ^ ((b >> 31) & 0x7fffffff);
}

__device__ __forceinline__ int64_t mark_row(const RArgs& a, int row) {
  return a.mark_rows == 1 ? 0 : row / a.scores_per_group;
}

__global__ __launch_bounds__(kBlock) void bdl_rank_count_kernel(const RArgs a) {
  __shared__ i4v s_pos[kBlock];
  __shared__ i4v s_neg[kBlock];
  const int t = threadIdx.x;
  const int row = blockIdx.y;
  const int64_t n = a.n;
  const int64_t sbase = (int64_t)row * n, mbase = mark_row(a, row) * n;
  const float* __restrict__ x = a.scores + sbase;
  const int32_t* __restrict__ m = a.marks + mbase;
  // both rows start on a 16-B boundary (the bases are 16-B aligned)
  const bool aligned = ((sbase | mbase) & 3) == 0;

  int32_t ki[kU];
  uint32_t gp[kU], gn[kU], gt[kU];
  int any = 0;
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t i = (int64_t)blockIdx.x * kITile + u * kBlock + t;
    ki[u] = kNone;
    if (i < n) {
      const int32_t mk = *(const gint*)(m + i);
      if (mk == 0 || mk == 1) ki[u] = key_of(sload(x + i));
    }
    any |= ki[u] != kNone;
    gp[u] = gn[u] = gt[u] = 0;
  }

  if (__syncthreads_or(any)) {  // workgroup-uniform
    for (int64_t j0 = 0; j0 < n; j0 += kJTile) {
      const int64_t e = j0 + 4 * t;
      f4v xs = {0.f, 0.f, 0.f, 0.f};
      i4v ms = {-1, -1, -1, -1};  // past the row: excluded
      if (aligned && e + 4 <= n) {
        xs = vload(x + e);
        ms = __builtin_nontemporal_load((const gi4v*)(m + e));
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (e + c < n) {
            xs[c] = sload(x + e + c);
            ms[c] = *(const gint*)(m + e + c);
          }
      }
      i4v kp, kn;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int32_t k = key_of(xs[c]);
        kp[c] = ms[c] == 1 ? k : kNone;
        kn[c] = ms[c] == 0 ? k : kNone;
      }
      __syncthreads();  // the previous tile's reads
      s_pos[t] = kp;
      s_neg[t] = kn;
      __syncthreads();
      const int64_t left = n - j0;
      const int groups = left >= kJTile ? kBlock : (int)((left + 3) >> 2);
      for (int q = 0; q < groups; ++q) {
        const i4v p = s_pos[q], g = s_neg[q];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int u = 0; u < kU; ++u) {
            gp[u] += p[c] >= ki[u] ? 1u : 0u;
            gn[u] += g[c] >= ki[u] ? 1u : 0u;
            gt[u] += g[c] > ki[u] ? 1u : 0u;
          }
      }
    }
  }

#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t i = (int64_t)blockIdx.x * kITile + u * kBlock + t;
    if (i >= n) continue;
    if (ki[u] == kNone) gp[u] = gn[u] = gt[u] = 0;  // kNone >= kNone counted the excluded j
    const int64_t o = sbase + i;
    *(guint*)(a.ws + o) = gp[u];
    *(guint*)(a.ws + a.plane + o) = gn[u];
    *(guint*)(a.ws + 2 * a.plane + o) = gt[u];
    if (a.ge_pos) *(guint*)(a.ge_pos + o) = gp[u];
    if (a.ge_neg) *(guint*)(a.ge_neg + o) = gn[u];
    if (a.gt_neg) *(guint*)(a.gt_neg + o) = gt[u];
  }
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// One workgroup per row.  A valid example has ge_pos + ge_neg >= 1 (itself),
// an excluded one 0 + 0: the counts and the mark say everything.
__global__ __launch_bounds__(kBlock) void bdl_rank_finalize_kernel(
    const RArgs a, bdl_rank_totals* __restrict__ totals, int64_t need_arg, int64_t tpr_num,
    int64_t tpr_den) {
  __shared__ int64_t s_i[4][kWaves];
  __shared__ double s_d[kWaves];
  __shared__ int64_t s_need;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int row = blockIdx.x;
  const int64_t n = a.n;
  const int64_t sbase = (int64_t)row * n;
  const int32_t* __restrict__ m = a.marks + mark_row(a, row) * n;
  const uint32_t* __restrict__ gp = a.ws + sbase;
  const uint32_t* __restrict__ gn = a.ws + a.plane + sbase;
  const uint32_t* __restrict__ gt = a.ws + 2 * a.plane + sbase;

  int64_t np = 0, nn = 0, nx = 0, below = 0;  // below: sum over positives of ge_neg + gt_neg
  double ap = 0.0;
  for (int64_t i = t; i < n; i += kBlock) {
    const uint32_t p = gp[i], g = gn[i];
    if (p + g == 0) {
      ++nx;
    } else if (m[i] == 1) {
      ++np;
      below += (int64_t)g + (int64_t)gt[i];
      ap += (double)p / (double)((int64_t)p + (int64_t)g);
    } else {
      ++nn;
    }
  }
  np = wave_sum_i64(np);
  nn = wave_sum_i64(nn);
  nx = wave_sum_i64(nx);
  below = wave_sum_i64(below);
  ap = wave_sum(ap);
  if (lane == 0) {
    s_i[0][w] = np;
    s_i[1][w] = nn;
    s_i[2][w] = nx;
    s_i[3][w] = below;
    s_d[w] = ap;
  }
  __syncthreads();
  if (t == 0) {
    np = s_i[0][0];
    nn = s_i[1][0];
    nx = s_i[2][0];
    below = s_i[3][0];
    ap = s_d[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      np += s_i[0][k];
      nn += s_i[1][k];
      nx += s_i[2][k];
      below += s_i[3][k];
      ap += s_d[k];
    }
    totals[row].n_pos = np;
    totals[row].n_neg = nn;
    totals[row].n_excluded = nx;
    totals[row].u2 = 2 * nn * np - below;
    totals[row].ap_sum = ap;
    // P = 0: no threshold keeps a true positive, nothing qualifies
    s_need = need_arg > 0 ? need_arg : np == 0 ? INT64_MAX : (np * tpr_num + tpr_den - 1) / tpr_den;
  }
  __syncthreads();
  const int64_t need = s_need;
  int64_t fp = INT64_MAX;
  for (int64_t i = t; i < n; i += kBlock) {
    const uint32_t p = gp[i], g = gn[i];
    if (p + g != 0 && (int64_t)p >= need && (int64_t)g < fp) fp = (int64_t)g;
  }
  fp = wave_min_i64(fp);
  if (lane == 0) s_i[0][w] = fp;  // thread 0 read s_i before the barrier above
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 1; k < kWaves; ++k) fp = s_i[0][k] < fp ? s_i[0][k] : fp;
    totals[row].fp_at_tpr = fp == INT64_MAX ? -1 : fp;
  }
}

static_assert(sizeof(bdl_rank_totals) == 48, "no padding");
static_assert(sizeof(bdl_rank_args) == 96, "no padding");

int64_t workspace_bytes(int64_t rows, int64_t n) { return (rows * n * 12 + 15) & ~(int64_t)15; }

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_rank_workspace_bytes(int32_t rows, int64_t n) {
  if (rows < 1 || rows > BDL_RANK_MAX_ROWS) return 0;
  if (n < 1 || n > INT32_MAX) return 0;
  return workspace_bytes(rows, n);
}

int bdl_rank(const bdl_rank_args* d, void* stream) {
  const std::string me = "bdl_rank: ";
  if (const int rc = no_redirect("bdl_rank")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->scores) return fail(BDL_ERR_NULL, me + "null scores");
  if (!d->marks) return fail(BDL_ERR_NULL, me + "null marks");
  if (!d->totals) return fail(BDL_ERR_NULL, me + "null totals");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->rows < 1 || d->rows > BDL_RANK_MAX_ROWS)
    return fail(BDL_ERR_ARG, me + "rows in [1, " + std::to_string(BDL_RANK_MAX_ROWS) + "]");
  if (d->n < 1 || d->n > INT32_MAX) return fail(BDL_ERR_ARG, me + "n in [1, 2^31 - 1]");
  if (d->scores_per_group < 1) return fail(BDL_ERR_ARG, me + "scores_per_group must be >= 1");
  if (d->rows % d->scores_per_group)
    return fail(BDL_ERR_ARG, me + "scores_per_group must divide rows");
  if (d->mark_rows != 1 && d->mark_rows != d->rows / d->scores_per_group)
    return fail(BDL_ERR_ARG, me + "mark_rows is rows / scores_per_group or 1");
  if (d->need < 0) return fail(BDL_ERR_ARG, me + "need must be >= 0");
  if (d->tpr_num < 1 || d->tpr_num > d->tpr_den)
    return fail(BDL_ERR_ARG, me + "1 <= tpr_num <= tpr_den");
  if (d->pad0 != 0) return fail(BDL_ERR_ARG, me + "pad0 must be 0");
  if (misaligned(d->scores, 15)) return fail(BDL_ERR_ALIGN, me + "scores not 16-B aligned");
  if (misaligned(d->marks, 15)) return fail(BDL_ERR_ALIGN, me + "marks not 16-B aligned");
  if (misaligned(d->workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  if (misaligned(d->totals, 7)) return fail(BDL_ERR_ALIGN, me + "totals not 8-B aligned");

  const uint64_t rn = (uint64_t)d->rows * (uint64_t)d->n;
  struct Span {
    const char* name;
    const void* p;
    uint64_t bytes;
  };
  const Span spans[] = {
      {"scores", d->scores, rn * 4},
      {"marks", d->marks, (uint64_t)d->mark_rows * (uint64_t)d->n * 4},
      {"ge_pos", d->ge_pos, rn * 4},
      {"ge_neg", d->ge_neg, rn * 4},
      {"gt_neg", d->gt_neg, rn * 4},
      {"totals", d->totals, (uint64_t)d->rows * sizeof(bdl_rank_totals)},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->rows, d->n)},
  };
  constexpr int kSpans = (int)(sizeof(spans) / sizeof(spans[0]));
  for (int i = 2; i < 5; ++i)
    if (misaligned(spans[i].p, 3))
      return fail(BDL_ERR_ALIGN, me + spans[i].name + " not 4-B aligned");
  for (int i = 2; i < kSpans; ++i)  // every written span against the inputs and the other ones
    for (int j = 0; j < i; ++j)
      if (overlap(spans[i].p, spans[j].p, spans[i].bytes, spans[j].bytes))
        return fail(BDL_ERR_ARG, me + spans[i].name + " overlaps " + spans[j].name);

  RArgs a;
  a.scores = d->scores;
  a.marks = d->marks;
  a.ge_pos = d->ge_pos;
  a.ge_neg = d->ge_neg;
  a.gt_neg = d->gt_neg;
  a.ws = reinterpret_cast<uint32_t*>(d->workspace);
  a.n = d->n;
  a.plane = (int64_t)rn;
  a.scores_per_group = d->scores_per_group;
  a.mark_rows = d->mark_rows;

  hipStream_t st = (hipStream_t)stream;
  const unsigned itiles = (unsigned)((d->n + kITile - 1) / kITile);
  hipLaunchKernelGGL(bdl_rank_count_kernel, dim3(itiles, (unsigned)d->rows), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(bdl_rank_finalize_kernel, dim3((unsigned)d->rows), dim3(kBlock), 0, st, a,
                     d->totals, d->need, (int64_t)d->tpr_num, (int64_t)d->tpr_den);
  return launched("bdl_rank");
}

}  // extern "C"
