// bdl_exchange.hip — replica exchange between stacked SGLD chains
// (include/bdl_exchange.h: the definitions, the arithmetic contract, the
// in-tile and cross-tile order, the bookkeeping).
//
// bdl_exchange_energy: a (chain, tile) item per workgroup iteration, a float4
// group per thread, one fp64 partial per item.
// bdl_exchange_decide: one workgroup adds every chain's partials in the fixed
// order, then a thread per adjacent pair decides and the bookkeeping follows.
// bdl_exchange_swap: the lower slot of every accepted pair exchanges the two
// whole slots of each vector; every other workgroup leaves after one load.
#include "bdl_chain_common.hpp"
#include "bdl_exchange.h"

namespace bdl {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kMaxK = BDL_EXCHANGE_MAX_CHAINS;
constexpr int kTile = BDL_EXCHANGE_TILE;

static_assert(kTile == 4 * kBlock, "a thread owns one float4 group of a tile");
static_assert(kMaxK <= kBlock, "one thread per chain / pair");
static_assert(sizeof(bdl_exchange_state) == 8 * (5 * kMaxK + 1) + 4 * 3 * kMaxK,
              "the state's layout");

struct EArgs {
  const float* __restrict__ theta;
  const float* __restrict__ prior;
  double* __restrict__ partials;
  int64_t n, stride, tiles, items;
};

__global__ __launch_bounds__(kBlock) void bdl_exchange_energy_kernel(const EArgs a) {
  // two stages: an item's stage is rewritten two items later, after a barrier
  // that thread 0 reaches only once it has read it
  __shared__ double s_wave[2][kWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int buf = 0;
  for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x, buf ^= 1) {
    const int64_t k = item / a.tiles, j = item - k * a.tiles;
    const int64_t e = j * kTile + 4 * (int64_t)t;
    double s = 0.0;
    if (e < a.n) {
      f4v d = ld4(a.theta + k * a.stride, e, a.n);
      if (a.prior) d = d - ld4(a.prior + k * a.stride, e, a.n);
      s += (double)d.x * (double)d.x;
      s += (double)d.y * (double)d.y;
      s += (double)d.z * (double)d.z;
      s += (double)d.w * (double)d.w;
    }
    s = wave_sum(s);
    if (lane == 0) s_wave[buf][wave] = s;
    __syncthreads();
    if (t == 0) {
      double v = s_wave[buf][0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += s_wave[buf][w];
      a.partials[item] = v;
    }
  }
}

struct DArgs {
  bdl_exchange_state* __restrict__ state;
  const double* __restrict__ partials;
  const float* __restrict__ loss;
  const double* __restrict__ beta;
  int64_t tiles;
  double n_data, two_sigma2, var;
  uint64_t seed, chain0, attempt;
  int32_t chains, flags;
};

__global__ __launch_bounds__(kBlock) void bdl_exchange_decide_kernel(const DArgs a) {
  __shared__ double s_wave[kWaves];
  __shared__ double s_U[kMaxK];
  __shared__ int s_accept[kMaxK], s_refused[kMaxK];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int K = a.chains;
  bdl_exchange_state* __restrict__ st = a.state;

  // q_k: partials t, t + 256, ... ascending from 0.0, the butterfly, the waves in order
  for (int k = 0; k < K; ++k) {
    const double* __restrict__ part = a.partials + (int64_t)k * a.tiles;
    double s = 0.0;
    for (int64_t i = t; i < a.tiles; i += kBlock) s += part[i];
    s = wave_sum(s);
    if (lane == 0) s_wave[wave] = s;
    __syncthreads();
    if (t == 0) {
      double v = s_wave[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += s_wave[w];
      s_U[k] = v;
    }
    __syncthreads();
  }
  if (t < K) st->q[t] = s_U[t];
  if (a.flags & BDL_EXCHANGE_ENERGY_ONLY) return;

  if (a.flags & BDL_EXCHANGE_FIRST) {
    if (t < kMaxK) {
      st->attempts[t] = st->accepts[t] = st->round_trips[t] = 0;
      st->partner[t] = t < K ? t : 0;
      st->replica[t] = t < K ? t : 0;
      st->direction[t] = K >= 2 && t == 0 ? BDL_EXCHANGE_UP
                         : K >= 2 && t == K - 1 ? BDL_EXCHANGE_DOWN : 0;
      if (t >= K) st->q[t] = st->U[t] = 0.0;
    }
    if (t == 0) st->refused = 0;
  }
  if (t < K) {
    const double U = a.n_data * (double)a.loss[t] + s_U[t] / a.two_sigma2;
    st->U[t] = U;
    st->partner[t] = t;
    s_accept[t] = s_refused[t] = 0;
    s_U[t] = U;  // (entry t held q_t, which only this thread read)
  }
  __syncthreads();

  const int parity = (int)(a.attempt & 1);
  if (t < K - 1 && (t & 1) == parity) {
    const double Ui = s_U[t], Uj = s_U[t + 1];
    const double db = a.beta[t] - a.beta[t + 1];
    const double la = db * (Ui - Uj) - (db * db) * a.var;
    const double big = __builtin_inf();
    const bool finite = __builtin_fabs(Ui) < big && __builtin_fabs(Uj) < big &&
                        __builtin_fabs(la) < big;  // false for a NaN too
    st->attempts[t] += 1;
    if (!finite) {
      s_refused[t] = 1;
    } else {
      const uint64_t s = BDL_EXCHANGE_STEP_BASE + a.attempt;
      const uint4 r = philox4x32_10(
          make_uint4((uint32_t)t, (uint32_t)a.chain0, (uint32_t)s, (uint32_t)(s >> 32)),
          (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
      const double u = ((double)r.x + 0.5) * (1.0 / 4294967296.0);
      if (log(u) < la) {
        s_accept[t] = 1;
        st->accepts[t] += 1;
      }
    }
  }
  __syncthreads();
  // the pairs of one parity are disjoint: thread i owns slots i and i + 1
  if (t < K - 1 && s_accept[t]) {
    st->partner[t] = t + 1;
    st->partner[t + 1] = t;
    const int32_t r = st->replica[t];
    st->replica[t] = st->replica[t + 1];
    st->replica[t + 1] = r;
  }
  __syncthreads();
  if (t == 0) {
    uint64_t ref = 0;
    for (int i = 0; i < K - 1; ++i) ref += (uint64_t)s_refused[i];
    st->refused += ref;
    if (K >= 2) {
      const int32_t r0 = st->replica[0], r1 = st->replica[K - 1];
      if (r0 >= 0 && r0 < K) {  // (a state the caller corrupted indexes nothing)
        if (st->direction[r0] == BDL_EXCHANGE_DOWN) st->round_trips[r0] += 1;
        st->direction[r0] = BDL_EXCHANGE_UP;
      }
      if (r1 >= 0 && r1 < K) st->direction[r1] = BDL_EXCHANGE_DOWN;
    }
  }
}

struct SArgs {
  const bdl_exchange_state* __restrict__ state;
  float* v[BDL_EXCHANGE_MAX_VECTORS];
  int64_t stride, groups;
  int32_t nvec;
};

__global__ __launch_bounds__(kBlock) void bdl_exchange_swap_kernel(const SArgs a) {
  const int k = blockIdx.y;
  const int p = a.state->partner[k];
  if (p <= k || p >= (int)gridDim.y) return;  // stays, or the pair's upper member
  const int64_t step = (int64_t)gridDim.x * kBlock;
#pragma unroll
  for (int i = 0; i < BDL_EXCHANGE_MAX_VECTORS; ++i) {
    if (i >= a.nvec) break;
    float* __restrict__ A = a.v[i] + (int64_t)k * a.stride;
    float* __restrict__ B = a.v[i] + (int64_t)p * a.stride;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < a.groups; g += step) {
      const f4v x = vload(A + 4 * g), y = vload(B + 4 * g);
      vstore(A + 4 * g, y);
      vstore(B + 4 * g, x);
    }
  }
}

bool chains_ok(int32_t c) { return c >= 1 && c <= BDL_EXCHANGE_MAX_CHAINS; }
int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_exchange_workspace_bytes(int32_t chains, int64_t n) {
  if (!chains_ok(chains) || n < 1 || n > INT64_MAX / 8 / chains) return 0;
  return 8 * (int64_t)chains * tiles_of(n);
}

int bdl_exchange_energy(const bdl_exchange_energy_args* d, void* stream) {
  const std::string me = "bdl_exchange_energy: ";
  if (const int rc = no_redirect("bdl_exchange_energy")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->theta) return fail(BDL_ERR_NULL, me + "null theta");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (!chains_ok(d->chains))
    return fail(BDL_ERR_ARG, me + "chains in [1, " + std::to_string(BDL_EXCHANGE_MAX_CHAINS) + "]");
  if (d->n < 1 || d->chain_groups < 1) return fail(BDL_ERR_ARG, me + "n and chain_groups must be >= 1");
  if (const char* why = stacked_slot_error(d->chains, d->n, d->chain_groups))
    return fail(BDL_ERR_ARG, me + why);
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_EXCHANGE_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_EXCHANGE_MAX_GRID) + "]");
  if (misaligned(d->theta, 15)) return fail(BDL_ERR_ALIGN, me + "theta not 16-B aligned");
  if (misaligned(d->prior, 15)) return fail(BDL_ERR_ALIGN, me + "prior not 16-B aligned");
  if (misaligned(d->workspace, 7)) return fail(BDL_ERR_ALIGN, me + "workspace not 8-B aligned");

  EArgs a;
  a.theta = d->theta;
  a.prior = d->prior;
  a.partials = reinterpret_cast<double*>(d->workspace);
  a.n = d->n;
  a.stride = 4 * (int64_t)d->chain_groups;
  a.tiles = tiles_of(d->n);
  a.items = a.tiles * d->chains;
  int64_t grid = d->grid_blocks;
  if (grid == 0)
    grid = capped_grid(a.items, std::min<int64_t>((int64_t)cu_count() * 8, BDL_EXCHANGE_MAX_GRID));
  hipLaunchKernelGGL(bdl_exchange_energy_kernel, dim3((unsigned)grid), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  return launched("bdl_exchange_energy");
}

int bdl_exchange_decide(const bdl_exchange_decide_args* d, void* stream) {
  const std::string me = "bdl_exchange_decide: ";
  if (const int rc = no_redirect("bdl_exchange_decide")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->state) return fail(BDL_ERR_NULL, me + "null state");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->flags & ~(BDL_EXCHANGE_FIRST | BDL_EXCHANGE_ENERGY_ONLY))
    return fail(BDL_ERR_ARG, me + "unknown flag");
  const bool only = (d->flags & BDL_EXCHANGE_ENERGY_ONLY) != 0;
  if (!only && !d->loss) return fail(BDL_ERR_NULL, me + "null loss");
  if (!only && !d->beta) return fail(BDL_ERR_NULL, me + "null beta");
  if (!chains_ok(d->chains))
    return fail(BDL_ERR_ARG, me + "chains in [1, " + std::to_string(BDL_EXCHANGE_MAX_CHAINS) + "]");
  if (d->n < 1 || d->n > INT64_MAX / 8 / d->chains) return fail(BDL_ERR_ARG, me + "n out of range");
  if (!only) {
    if (!(d->sigma2 > 0.0)) return fail(BDL_ERR_ARG, me + "sigma2 must be > 0");
    if (!(d->var >= 0.0)) return fail(BDL_ERR_ARG, me + "var must be >= 0");
    if (d->n_data != d->n_data) return fail(BDL_ERR_ARG, me + "n_data is a NaN");
    if (d->attempt >= (1ull << 62)) return fail(BDL_ERR_ARG, me + "attempt must be < 2^62");
  }
  if (misaligned(d->state, 7)) return fail(BDL_ERR_ALIGN, me + "state not 8-B aligned");
  if (misaligned(d->workspace, 7)) return fail(BDL_ERR_ALIGN, me + "workspace not 8-B aligned");
  if (misaligned(d->beta, 7)) return fail(BDL_ERR_ALIGN, me + "beta not 8-B aligned");
  if (misaligned(d->loss, 3)) return fail(BDL_ERR_ALIGN, me + "loss not 4-B aligned");
  if (overlap(d->state, d->workspace, sizeof(bdl_exchange_state),
              (uint64_t)8 * d->chains * tiles_of(d->n)))
    return fail(BDL_ERR_ARG, me + "state overlaps workspace");

  DArgs a;
  a.state = d->state;
  a.partials = reinterpret_cast<const double*>(d->workspace);
  a.loss = d->loss;
  a.beta = d->beta;
  a.tiles = tiles_of(d->n);
  a.n_data = d->n_data;
  a.two_sigma2 = 2.0 * d->sigma2;
  a.var = d->var;
  a.seed = d->seed;
  a.chain0 = d->chain0;
  a.attempt = d->attempt;
  a.chains = d->chains;
  a.flags = d->flags;
  hipLaunchKernelGGL(bdl_exchange_decide_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, a);
  return launched("bdl_exchange_decide");
}

int bdl_exchange_swap(const bdl_exchange_swap_args* d, void* stream) {
  const std::string me = "bdl_exchange_swap: ";
  if (const int rc = no_redirect("bdl_exchange_swap")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->state) return fail(BDL_ERR_NULL, me + "null state");
  if (!chains_ok(d->chains))
    return fail(BDL_ERR_ARG, me + "chains in [1, " + std::to_string(BDL_EXCHANGE_MAX_CHAINS) + "]");
  if (d->nvectors < 1 || d->nvectors > BDL_EXCHANGE_MAX_VECTORS)
    return fail(BDL_ERR_ARG, me + "nvectors in [1, " + std::to_string(BDL_EXCHANGE_MAX_VECTORS) + "]");
  if (d->chain_groups < 1) return fail(BDL_ERR_ARG, me + "chain_groups must be >= 1");
  if (const char* why = stacked_slot_error(d->chains, 1, d->chain_groups))
    return fail(BDL_ERR_ARG, me + why);
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_EXCHANGE_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_EXCHANGE_MAX_GRID) + "]");
  if (misaligned(d->state, 7)) return fail(BDL_ERR_ALIGN, me + "state not 8-B aligned");
  const uint64_t bytes = 16 * d->chain_groups * (uint64_t)d->chains;
  for (int i = 0; i < d->nvectors; ++i) {
    if (!d->vectors[i]) return fail(BDL_ERR_NULL, me + "null vector");
    if (misaligned(d->vectors[i], 15)) return fail(BDL_ERR_ALIGN, me + "a vector is not 16-B aligned");
    if (overlap(d->vectors[i], d->state, bytes, sizeof(bdl_exchange_state)))
      return fail(BDL_ERR_ARG, me + "a vector overlaps the state");
    for (int j = 0; j < i; ++j)
      if (overlap(d->vectors[i], d->vectors[j], bytes, bytes))
        return fail(BDL_ERR_ARG, me + "two vectors overlap");
  }

  SArgs a;
  a.state = d->state;
  for (int i = 0; i < BDL_EXCHANGE_MAX_VECTORS; ++i) a.v[i] = i < d->nvectors ? d->vectors[i] : nullptr;
  a.stride = 4 * (int64_t)d->chain_groups;
  a.groups = (int64_t)d->chain_groups;
  a.nvec = d->nvectors;
  int64_t bpc = d->grid_blocks;
  if (bpc == 0)
    bpc = std::min<int64_t>(blocks_per_chain(8, d->chains, (a.groups + kBlock - 1) / kBlock),
                            BDL_EXCHANGE_MAX_GRID);
  hipLaunchKernelGGL(bdl_exchange_swap_kernel, dim3((unsigned)bpc, (unsigned)d->chains), dim3(kBlock),
                     0, (hipStream_t)stream, a);
  return launched("bdl_exchange_swap");
}

}  // extern "C"
