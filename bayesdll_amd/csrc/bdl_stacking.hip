// bdl_stacking.hip — Bayesian stacking weights of an ensemble's voters
// (include/bdl_stacking.h: the definitions, the arithmetic contract, the
// geometry, the error bound).
//
// bdl_stack_gather: an example per thread picks logp[k, b, label_b] of every
// voter into column off + b of ell [P, cap]; the three exclusion counts go
// through per-workgroup partials and a combine launch.
// bdl_stack_fit: per iteration a sweep over fixed tiles of 1024 columns (a
// thread owns four columns 256 apart and passes over the P voters three times —
// the maximum, s, the ratios — re-reading its cache-resident values, so nothing
// is indexed dynamically in registers) and a one-workgroup update that adds the
// tile partials in tile order and takes the multiplicative step.
#include "bdl_chain_common.hpp"
#include "bdl_stacking.h"

namespace bdl {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kMaxP = BDL_STACK_MAX_VOTERS;
constexpr int kTile = BDL_STACK_TILE;
constexpr int kPer = kTile / kBlock;  // columns of a tile per thread
constexpr int kExtra = 3;             // words of a partial after R[P]: F, n, the s <= 0 count

static_assert(kTile % kBlock == 0 && kPer == 4, "a thread owns four columns of a tile");
static_assert(kMaxP + kExtra <= kBlock, "one thread per word of a partial");
static_assert(sizeof(bdl_stack_state) == 8 * kMaxP + 48, "the state's layout");

struct GArgs {
  const float* __restrict__ logp;
  const int64_t* __restrict__ labels;
  float* __restrict__ ell;
  int32_t* __restrict__ valid;
  int64_t batch, off, cap;
  int32_t voters, classes;
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// partial[3 * blockIdx.x + c]: this workgroup's count of cause c
__global__ __launch_bounds__(kBlock) void bdl_stack_gather_kernel(const GArgs a,
                                                                  int64_t* __restrict__ partial) {
  __shared__ int s_cnt[kWaves][3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int P = a.voters;
  const int64_t C = a.classes;
  const float inf = __builtin_inff();
  int c_label = 0, c_nonf = 0, c_imp = 0;  // at most 2^24 / 256 examples per thread
  for (int64_t b = (int64_t)blockIdx.x * kBlock + t; b < a.batch; b += (int64_t)gridDim.x * kBlock) {
    const int64_t lab = a.labels[b];
    const bool in = lab >= 0 && lab < C;
    bool nonf = false, imp = true;
    if (in) {
      for (int k = 0; k < P; ++k) {
        const float x = a.logp[((int64_t)k * a.batch + b) * C + lab];
        nonf |= (x != x) || x == inf;
        imp &= x == -inf;
      }
    }
    const bool ok = in && !nonf && !imp;
    if (!in)
      ++c_label;
    else if (nonf)
      ++c_nonf;
    else if (imp)
      ++c_imp;
    const int64_t col = a.off + b;
    for (int k = 0; k < P; ++k)
      a.ell[(int64_t)k * a.cap + col] = ok ? a.logp[((int64_t)k * a.batch + b) * C + lab] : 0.0f;
    a.valid[col] = ok ? 1 : 0;
  }
  c_label = wave_sum_int(c_label);
  c_nonf = wave_sum_int(c_nonf);
  c_imp = wave_sum_int(c_imp);
  if (lane == 0) {
    s_cnt[wave][0] = c_label;
    s_cnt[wave][1] = c_nonf;
    s_cnt[wave][2] = c_imp;
  }
  __syncthreads();
  if (t < 3) {
    int64_t v = 0;
    for (int w = 0; w < kWaves; ++w) v += s_cnt[w][t];
    partial[3 * (int64_t)blockIdx.x + t] = v;
  }
}

__global__ void bdl_stack_gather_combine_kernel(const int64_t* __restrict__ partial, int nblocks,
                                                int64_t* __restrict__ counters, int reset) {
  const int c = threadIdx.x;
  if (c >= 3) return;
  int64_t v = 0;
  for (int i = 0; i < nblocks; ++i) v += partial[3 * (int64_t)i + c];
  counters[c] = reset ? v : counters[c] + v;
}

struct FArgs {
  const float* __restrict__ ell;
  const int32_t* __restrict__ valid;
  bdl_stack_state* state;
  int64_t* partials;  // ntiles x (voters + kExtra) 8-B words
  int64_t n_cols, cap;
  int32_t voters, ntiles;
  int32_t first;  // the fit's first pass: w = 1/P, the state is not read
};

// a launch of a fit that is over leaves everything alone (workgroup-uniform)
__device__ __forceinline__ bool fit_over(const FArgs& a) {
  return !a.first && (a.state->converged != 0 || a.state->degenerate != 0);
}

__global__ __launch_bounds__(kBlock) void bdl_stack_sweep_kernel(const FArgs a) {
  __shared__ double s_w[kMaxP];
  __shared__ double s_stage[kWaves][kMaxP + 1];  // R[P], F
  __shared__ int s_cnt[kWaves][2];               // valid, s <= 0
  if (fit_over(a)) return;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int P = a.voters, W = P + kExtra;
  if (t < P) s_w[t] = a.first ? 1.0 / (double)P : a.state->w[t];
  __syncthreads();
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t c0 = (int64_t)tile * kTile + t;
    bool ok[kPer];
    float m[kPer];
    double s[kPer], inv[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int64_t col = c0 + (int64_t)j * kBlock;
      ok[j] = col < a.n_cols && a.valid[col] != 0;
      m[j] = -__builtin_inff();
      s[j] = 0.0;
      inv[j] = 0.0;
    }
    for (int k = 0; k < P; ++k) {
      const float* __restrict__ row = a.ell + (int64_t)k * a.cap + c0;
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (ok[j]) m[j] = __builtin_fmaxf(m[j], row[j * kBlock]);
    }
    for (int k = 0; k < P; ++k) {
      const float* __restrict__ row = a.ell + (int64_t)k * a.cap + c0;
      const double wk = s_w[k];
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (ok[j]) s[j] += wk * (double)expf(row[j * kBlock] - m[j]);
    }
    double F = 0.0;
    int cnt = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (ok[j]) {
        ++cnt;
        if (s[j] > 0.0) {
          inv[j] = 1.0 / s[j];
          F += log(s[j]) + (double)m[j];
        } else {  // underflow (or a NaN a caller put into a valid column)
          ++bad;
          ok[j] = false;
        }
      }
    for (int k = 0; k < P; ++k) {
      const float* __restrict__ row = a.ell + (int64_t)k * a.cap + c0;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (ok[j]) acc += (double)expf(row[j * kBlock] - m[j]) * inv[j];
      acc = wave_sum(acc);
      if (lane == 0) s_stage[wave][k] = acc;
    }
    F = wave_sum(F);
    cnt = wave_sum_int(cnt);
    bad = wave_sum_int(bad);
    if (lane == 0) {
      s_stage[wave][P] = F;
      s_cnt[wave][0] = cnt;
      s_cnt[wave][1] = bad;
    }
    __syncthreads();
    int64_t* __restrict__ part = a.partials + (int64_t)tile * W;
    if (t <= P) {
      double v = s_stage[0][t];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += s_stage[w][t];
      part[t] = __double_as_longlong(v);
    } else if (t < W) {
      int64_t v = 0;
      for (int w = 0; w < kWaves; ++w) v += s_cnt[w][t - P - 1];
      part[t] = v;
    }
    __syncthreads();  // before the next tile's stage is written
  }
}

__global__ __launch_bounds__(kBlock) void bdl_stack_update_kernel(const FArgs a, double tol,
                                                                  int eval_only) {
  __shared__ double s_sum[kMaxP + 1];
  __shared__ int64_t s_int[2];
  if (fit_over(a)) return;
  const int t = threadIdx.x;
  const int P = a.voters, W = P + kExtra;
  if (t <= P) {
    double v = 0.0;
    for (int i = 0; i < a.ntiles; ++i) v += __longlong_as_double(a.partials[(int64_t)i * W + t]);
    s_sum[t] = v;
  } else if (t < W) {
    int64_t v = 0;
    for (int i = 0; i < a.ntiles; ++i) v += a.partials[(int64_t)i * W + t];
    s_int[t - P - 1] = v;
  }
  __syncthreads();
  if (t != 0) return;
  bdl_stack_state* __restrict__ st = a.state;
  const int64_t n = s_int[0];
  if (a.first) {
    const double nan = __builtin_nan("");
    for (int k = 0; k < kMaxP; ++k) st->w[k] = k < P ? 1.0 / (double)P : 0.0;
    st->objective = st->gap = st->objective_uniform = nan;
    st->iterations = st->converged = st->degenerate = st->pad = 0;
  }
  st->n = n;
  if (n == 0 || s_int[1] != 0) {
    st->degenerate = 1;
    return;
  }
  const double dn = (double)n;
  double gmax = s_sum[0] / dn;
  for (int k = 1; k < P; ++k) {
    const double g = s_sum[k] / dn;
    if (g > gmax) gmax = g;
  }
  const double objective = s_sum[P] / dn, gap = gmax - 1.0;
  st->objective = objective;
  st->gap = gap;
  if (a.first) st->objective_uniform = objective;
  if (gap <= tol) {
    st->converged = 1;
    return;
  }
  if (eval_only) return;
  double sum = 0.0;
  for (int k = 0; k < P; ++k) {
    const double wk = st->w[k] * (s_sum[k] / dn);
    st->w[k] = wk;
    sum += wk;
  }
  for (int k = 0; k < P; ++k) st->w[k] = st->w[k] / sum;
  st->iterations += 1;
}

int64_t tiles_of(int64_t cols) { return (cols + kTile - 1) / kTile; }

int64_t workspace_bytes(int64_t voters, int64_t cols) {
  return std::max<int64_t>(tiles_of(cols) * (voters + kExtra) * 8, BDL_STACK_MAX_GRID * 3 * 8);
}

bool voters_ok(int32_t v) { return v >= 1 && v <= BDL_STACK_MAX_VOTERS; }
bool cols_ok(int64_t c) { return c >= 1 && c <= BDL_STACK_MAX_COLS; }

struct Span {
  const char* name;
  const void* p;
  uint64_t bytes;
};

// every span from `first_written` on against all before it; nullptr: none overlaps
const char* overlap_error(const Span* spans, int count, int first_written, std::string& msg) {
  for (int i = first_written; i < count; ++i)
    for (int j = 0; j < i; ++j)
      if (overlap(spans[i].p, spans[j].p, spans[i].bytes, spans[j].bytes)) {
        msg = std::string(spans[i].name) + " overlaps " + spans[j].name;
        return msg.c_str();
      }
  return nullptr;
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_stack_workspace_bytes(int32_t voters, int64_t cols) {
  if (!voters_ok(voters) || !cols_ok(cols)) return 0;
  return workspace_bytes(voters, cols);
}

int bdl_stack_gather(const bdl_stack_gather_args* d, void* stream) {
  const std::string me = "bdl_stack_gather: ";
  if (const int rc = no_redirect("bdl_stack_gather")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->logp) return fail(BDL_ERR_NULL, me + "null logp");
  if (!d->labels) return fail(BDL_ERR_NULL, me + "null labels");
  if (!d->ell) return fail(BDL_ERR_NULL, me + "null ell");
  if (!d->valid) return fail(BDL_ERR_NULL, me + "null valid");
  if (!d->counters) return fail(BDL_ERR_NULL, me + "null counters");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (!voters_ok(d->voters))
    return fail(BDL_ERR_ARG, me + "voters in [1, " + std::to_string(BDL_STACK_MAX_VOTERS) + "]");
  if (d->batch < 1) return fail(BDL_ERR_ARG, me + "batch must be >= 1");
  if (d->classes < 1 || d->classes > BDL_STACK_MAX_CLASSES)
    return fail(BDL_ERR_ARG, me + "classes in [1, " + std::to_string(BDL_STACK_MAX_CLASSES) + "]");
  if (!cols_ok(d->cap))
    return fail(BDL_ERR_ARG, me + "cap in [1, " + std::to_string(BDL_STACK_MAX_COLS) + "]");
  if (d->off < 0 || d->off > d->cap || d->batch > d->cap - d->off)
    return fail(BDL_ERR_ARG, me + "columns off .. off + batch - 1 must lie in [0, cap)");
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_STACK_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_STACK_MAX_GRID) + "]");
  if (d->flags & ~BDL_STACK_RESET) return fail(BDL_ERR_ARG, me + "unknown flag");
  // batch <= cap <= 2^24, voters <= 64, classes <= 8192: the byte count fits int64
  if (misaligned(d->logp, 3)) return fail(BDL_ERR_ALIGN, me + "logp not 4-B aligned");
  if (misaligned(d->ell, 3)) return fail(BDL_ERR_ALIGN, me + "ell not 4-B aligned");
  if (misaligned(d->valid, 3)) return fail(BDL_ERR_ALIGN, me + "valid not 4-B aligned");
  if (misaligned(d->labels, 7)) return fail(BDL_ERR_ALIGN, me + "labels not 8-B aligned");
  if (misaligned(d->counters, 7)) return fail(BDL_ERR_ALIGN, me + "counters not 8-B aligned");
  if (misaligned(d->workspace, 7)) return fail(BDL_ERR_ALIGN, me + "workspace not 8-B aligned");

  const Span spans[] = {
      {"logp", d->logp, (uint64_t)d->voters * (uint64_t)d->batch * (uint64_t)d->classes * 4},
      {"labels", d->labels, (uint64_t)d->batch * 8},
      {"ell", d->ell, (uint64_t)d->voters * (uint64_t)d->cap * 4},
      {"valid", d->valid, (uint64_t)d->cap * 4},
      {"counters", d->counters, 24},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->voters, d->cap)},
  };
  std::string msg;
  if (overlap_error(spans, 6, 2, msg)) return fail(BDL_ERR_ARG, me + msg);

  GArgs a;
  a.logp = d->logp;
  a.labels = d->labels;
  a.ell = d->ell;
  a.valid = d->valid;
  a.batch = d->batch;
  a.off = d->off;
  a.cap = d->cap;
  a.voters = d->voters;
  a.classes = d->classes;
  int grid = d->grid_blocks;
  if (grid == 0) grid = (int)capped_grid((d->batch + kBlock - 1) / kBlock, BDL_STACK_MAX_GRID);
  int64_t* partial = reinterpret_cast<int64_t*>(d->workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bdl_stack_gather_kernel, dim3(grid), dim3(kBlock), 0, st, a, partial);
  hipLaunchKernelGGL(bdl_stack_gather_combine_kernel, dim3(1), dim3(64), 0, st, partial, grid,
                     d->counters, (int)(d->flags & BDL_STACK_RESET));
  return launched("bdl_stack_gather");
}

int bdl_stack_fit(const bdl_stack_fit_args* d, void* stream) {
  const std::string me = "bdl_stack_fit: ";
  if (const int rc = no_redirect("bdl_stack_fit")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->ell) return fail(BDL_ERR_NULL, me + "null ell");
  if (!d->valid) return fail(BDL_ERR_NULL, me + "null valid");
  if (!d->state) return fail(BDL_ERR_NULL, me + "null state");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (!voters_ok(d->voters))
    return fail(BDL_ERR_ARG, me + "voters in [1, " + std::to_string(BDL_STACK_MAX_VOTERS) + "]");
  if (!cols_ok(d->cap))
    return fail(BDL_ERR_ARG, me + "cap in [1, " + std::to_string(BDL_STACK_MAX_COLS) + "]");
  if (d->n_cols < 1 || d->n_cols > d->cap) return fail(BDL_ERR_ARG, me + "n_cols in [1, cap]");
  if (!(d->tol >= 0.0)) return fail(BDL_ERR_ARG, me + "tol must be >= 0");
  if (d->iterations < 0 || d->iterations > BDL_STACK_MAX_CHUNK)
    return fail(BDL_ERR_ARG,
                me + "iterations in [0, " + std::to_string(BDL_STACK_MAX_CHUNK) + "]");
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_STACK_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_STACK_MAX_GRID) + "]");
  if (d->flags & ~(BDL_STACK_FIRST | BDL_STACK_FINAL)) return fail(BDL_ERR_ARG, me + "unknown flag");
  if (d->iterations == 0 && !(d->flags & BDL_STACK_FINAL))
    return fail(BDL_ERR_ARG, me + "nothing to enqueue (iterations = 0 without BDL_STACK_FINAL)");
  if (misaligned(d->ell, 3)) return fail(BDL_ERR_ALIGN, me + "ell not 4-B aligned");
  if (misaligned(d->valid, 3)) return fail(BDL_ERR_ALIGN, me + "valid not 4-B aligned");
  if (misaligned(d->state, 7)) return fail(BDL_ERR_ALIGN, me + "state not 8-B aligned");
  if (misaligned(d->workspace, 7)) return fail(BDL_ERR_ALIGN, me + "workspace not 8-B aligned");

  const Span spans[] = {
      {"ell", d->ell, (uint64_t)d->voters * (uint64_t)d->cap * 4},
      {"valid", d->valid, (uint64_t)d->cap * 4},
      {"state", d->state, (uint64_t)sizeof(bdl_stack_state)},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->voters, d->n_cols)},
  };
  std::string msg;
  if (overlap_error(spans, 4, 2, msg)) return fail(BDL_ERR_ARG, me + msg);

  FArgs a;
  a.ell = d->ell;
  a.valid = d->valid;
  a.state = d->state;
  a.partials = reinterpret_cast<int64_t*>(d->workspace);
  a.n_cols = d->n_cols;
  a.cap = d->cap;
  a.voters = d->voters;
  a.ntiles = (int32_t)tiles_of(d->n_cols);
  a.first = (d->flags & BDL_STACK_FIRST) ? 1 : 0;
  int grid = d->grid_blocks;
  if (grid == 0)
    grid = (int)capped_grid(std::min<int64_t>(a.ntiles, (int64_t)cu_count() * 2),
                            BDL_STACK_MAX_GRID);
  hipStream_t st = (hipStream_t)stream;
  const int passes = d->iterations + ((d->flags & BDL_STACK_FINAL) ? 1 : 0);
  for (int i = 0; i < passes; ++i) {
    hipLaunchKernelGGL(bdl_stack_sweep_kernel, dim3(grid), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(bdl_stack_update_kernel, dim3(1), dim3(kBlock), 0, st, a, d->tol,
                       (int)(i >= d->iterations));
    a.first = 0;
  }
  return launched("bdl_stack_fit");
}

}  // extern "C"
