// bdl_temper.hip — temperature scaling of the sample-averaged log-probabilities
// on the device (include/bdl_temper.h: the definitions, the special values, the
// arithmetic contract, the geometry).
//
// Two sweep templates over bdl_predict.hip's geometry, bdl_temper_fit_kernel and
// bdl_temper_report_kernel <NT, VEC, WAVE>: an example is handled by 64 threads
// (WAVE: classes <= 256, four examples per workgroup, wave shuffles only) or by
// the whole workgroup; thread ti owns the 16-B class groups ti, ti + TPI, ...
// (NT of them) of the row, and the next example's row is loaded before the
// current one is reduced.  The fit's second launch is the Newton update (one
// workgroup per group), the report's the combine.  The row helpers restate
// bdl_predict.hip's (that unit's code generation is left as it is).
#include "bdl_chain_common.hpp"
#include "bdl_temper.h"

namespace bdl {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr float kBetaMin = 1.0f / BDL_TEMPER_MAX_T, kBetaMax = 1.0f / BDL_TEMPER_MIN_T;

struct RowArgs {
  const float* __restrict__ logp;
  const int64_t* __restrict__ labels;
  const bdl_temper_state* __restrict__ state;
  int64_t batch;
  int32_t groups, classes;
};

// Two slots per reduction buffer: consecutive reductions alternate, so a slot
// is rewritten only after a barrier that every thread passed after its reads.
struct RedScratch {
  float v[2][kWaves];
  int i[2][kWaves];
  int f[2][kWaves];
  double s[2][3][kWaves];
};

// the larger value wins, the lower index among equals
__device__ __forceinline__ void take_max(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// Every thread of the example gets (max, its lowest index, or of the flags).
template <bool WAVE>
__device__ __forceinline__ void red_max(float& v, int& idx, int& flag, RedScratch& s, int& phase) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(idx, off, 64);
    flag |= __shfl_xor(flag, off, 64);
    take_max(v, idx, ov, oi);
  }
  if constexpr (!WAVE) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      s.v[phase][w] = v;
      s.i[phase][w] = idx;
      s.f[phase][w] = flag;
    }
    __syncthreads();
    v = s.v[phase][0];
    idx = s.i[phase][0];
    flag = s.f[phase][0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      take_max(v, idx, s.v[phase][k], s.i[phase][k]);
      flag |= s.f[phase][k];
    }
    phase ^= 1;
  }
}

// Every thread of the example gets the NV fp64 sums (butterfly, then the waves
// in order).
template <bool WAVE, int NV>
__device__ __forceinline__ void red_sum(double (&a)[NV], RedScratch& s, int& phase) {
  static_assert(NV <= 3, "RedScratch holds three sums");
#pragma unroll
  for (int q = 0; q < NV; ++q) a[q] = wave_sum(a[q]);
  if constexpr (!WAVE) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int q = 0; q < NV; ++q) s.s[phase][q][w] = a[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      a[q] = s.s[phase][q][0];
#pragma unroll
      for (int k = 1; k < kWaves; ++k) a[q] += s.s[phase][q][k];
    }
    phase ^= 1;
  }
}

// The class groups q, q + TPI, ... of one row; a class >= C reads as a masked
// one (-inf).  VEC: C % 4 == 0, every group is whole and 16-B aligned.
template <int NT, bool VEC, int TPI>
__device__ __forceinline__ void load_row(f4v (&x)[NT], const float* __restrict__ row, int q, int C) {
  const float ninf = -__builtin_inff();
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int c0 = 4 * (q + TPI * u);
    f4v v = {ninf, ninf, ninf, ninf};
    if constexpr (VEC) {
      if (c0 < C) v = vload(row + c0);
    } else {
      if (c0 + 0 < C) v.x = sload(row + c0 + 0);
      if (c0 + 1 < C) v.y = sload(row + c0 + 1);
      if (c0 + 2 < C) v.z = sload(row + c0 + 2);
      if (c0 + 3 < C) v.w = sload(row + c0 + 3);
    }
    x[u] = v;
  }
}

// (max_c z, its lowest index, a NaN or a +inf anywhere) of the row every thread
// of the example holds a part of.
template <int NT, bool WAVE, int TPI>
__device__ __forceinline__ void row_max(const f4v (&x)[NT], int ti, float& m, int& am, int& nonf,
                                        RedScratch& s, int& phase) {
  m = -__builtin_inff();
  am = INT32_MAX;
  nonf = 0;
#pragma unroll
  for (int u = 0; u < NT; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = x[u][j];
      if (v != v || v == __builtin_inff())
        nonf = 1;
      else if (v > m) {
        m = v;
        am = 4 * (ti + TPI * u) + j;
      }
    }
  red_max<WAVE>(m, am, nonf, s, phase);
}

__device__ __forceinline__ bool finite32(float v) { return v - v == 0.0f; }

// ------------------------------------------------------------------ the fit
struct FitPartial {
  double f, f1, f2;
  int64_t n, n_nonf, n_inf;
};

struct FitAcc {
  double f, f1, f2;
  int64_t n, n_nonf, n_inf;

  static __device__ __forceinline__ FitAcc zero() {
    FitAcc s;
    s.f = s.f1 = s.f2 = 0.0;
    s.n = s.n_nonf = s.n_inf = 0;
    return s;
  }
  __device__ __forceinline__ void add(const FitAcc& o) {
    f += o.f;
    f1 += o.f1;
    f2 += o.f2;
    n += o.n;
    n_nonf += o.n_nonf;
    n_inf += o.n_inf;
  }
};

// every wave's sums in its lane 0: the waves in order, in thread 0
__device__ __forceinline__ FitAcc fit_block_total(const FitAcc& acc) {
  __shared__ FitAcc s_acc[kWaves];
  __syncthreads();  // the previous call's reads
  if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
  __syncthreads();
  FitAcc s = s_acc[0];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s.add(s_acc[k]);
  }
  return s;
}

// partials[g * nw + r]: the share of group g of the workgroup that is r
// workgroups on from the group's first (r < nw = min(grid, ceil(N / IPB))).
template <int NT, bool VEC, bool WAVE>
__global__ __launch_bounds__(kBlock) void bdl_temper_fit_kernel(
    const RowArgs a, FitPartial* __restrict__ partials, int nw) {
  __shared__ RedScratch s_red;
  constexpr int TPI = WAVE ? 64 : kBlock;  // threads per example
  constexpr int IPB = WAVE ? kWaves : 1;   // examples per workgroup iteration
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ti = WAVE ? lane : t;
  const int C = a.classes;
  const float ninf = -__builtin_inff();
  int phase = 0;

  for (int g = 0; g < a.groups; ++g) {
    const uint32_t r = rotated_block(g);
    if ((int64_t)r * IPB >= a.batch) continue;  // workgroup-uniform: no example of this group
    if (a.state[g].done) continue;              // beta is final: the update skips it too
    const float beta = a.state[g].beta;
    FitAcc acc = FitAcc::zero();
    const int64_t bstride = (int64_t)gridDim.x * IPB;
    int64_t b = (int64_t)r * IPB + (WAVE ? wave : 0);
    f4v cur[NT], nxt[NT];
    if (b < a.batch) load_row<NT, VEC, TPI>(cur, a.logp + ((int64_t)g * a.batch + b) * C, ti, C);
    for (; b < a.batch; b += bstride) {
      const float* __restrict__ row = a.logp + ((int64_t)g * a.batch + b) * C;
      if (b + bstride < a.batch) load_row<NT, VEC, TPI>(nxt, row + bstride * C, ti, C);
      const int64_t lab = a.labels ? a.labels[b] : -1;
      const bool labelled = lab >= 0 && lab < C;
      const float zy = labelled ? sload(row + lab) : 0.0f;

      float zmax;
      int am, nonf;
      row_max<NT, WAVE, TPI>(cur, ti, zmax, am, nonf, s_red, phase);
      const float m = beta * zmax;
      double sum[3] = {0.0, 0.0, 0.0};
      const bool bad = nonf || !finite32(m);  // uniform over the example's threads
      if (!bad && labelled) {
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float z = cur[u][j];
            const float tz = beta * z;
            const float d = tz - m;
            const float e = expf(d);
            if (e != 0.0f) {  // a masked class (z = -inf) adds nothing, never 0 * inf
              const double ez = (double)e * (double)z;
              sum[0] += (double)e;
              sum[1] += ez;
              sum[2] += ez * (double)z;
            }
          }
        red_sum<WAVE, 3>(sum, s_red, phase);
      }
#pragma unroll
      for (int u = 0; u < NT; ++u) cur[u] = nxt[u];
      if (ti != 0) continue;
      if (bad) {
        ++acc.n_nonf;
      } else if (labelled) {
        const float ty = beta * zy;
        if (ty == ninf) {
          ++acc.n_inf;
        } else {
          const double E = sum[1] / sum[0];
          double var = sum[2] / sum[0] - E * E;
          var = var > 0.0 ? var : 0.0;
          ++acc.n;
          acc.f += ((double)m + log(sum[0])) - (double)ty;
          acc.f1 += E - (double)zy;
          acc.f2 += var;
        }
      }
    }
    const FitAcc s = fit_block_total(acc);
    if (t == 0) {
      FitPartial* __restrict__ out = partials + (int64_t)g * nw + r;
      out->f = s.f;
      out->f1 = s.f1;
      out->f2 = s.f2;
      out->n = s.n;
      out->n_nonf = s.n_nonf;
      out->n_inf = s.n_inf;
    }
  }
}

// One workgroup per group: thread t adds the partials t, t + 256, ..., then
// the wave butterfly and the waves in order; thread 0 takes the Newton step
// (include/bdl_temper.h, bdl_temper_fit_update, steps 1-5).
__global__ __launch_bounds__(kBlock) void bdl_temper_update_kernel(
    const FitPartial* __restrict__ partials, int nw, bdl_temper_state* __restrict__ state,
    double rtol, int max_iter) {
  bdl_temper_state* __restrict__ st = state + blockIdx.x;
  if (st->done) return;  // workgroup-uniform
  const FitPartial* __restrict__ part = partials + (int64_t)blockIdx.x * nw;
  FitAcc acc = FitAcc::zero();
  for (int i = threadIdx.x; i < nw; i += kBlock) {
    acc.f += part[i].f;
    acc.f1 += part[i].f1;
    acc.f2 += part[i].f2;
    acc.n += part[i].n;
    acc.n_nonf += part[i].n_nonf;
    acc.n_inf += part[i].n_inf;
  }
  acc.f = wave_sum(acc.f);
  acc.f1 = wave_sum(acc.f1);
  acc.f2 = wave_sum(acc.f2);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc.n += __shfl_xor(acc.n, off, 64);
    acc.n_nonf += __shfl_xor(acc.n_nonf, off, 64);
    acc.n_inf += __shfl_xor(acc.n_inf, off, 64);
  }
  const FitAcc s = fit_block_total(acc);
  if (threadIdx.x != 0) return;

  const double dn = (double)s.n;
  const double nll = s.n ? s.f / dn : (double)__builtin_nanf("");
  const double d1 = s.n ? s.f1 / dn : 0.0, d2 = s.n ? s.f2 / dn : 0.0;
  st->n = s.n;
  st->n_nonfinite = s.n_nonf;
  st->n_inf_label = s.n_inf;
  st->nll = nll;
  if (st->sweeps == 0) st->nll_first = nll;
  st->d1 = d1;
  st->d2 = d2;
  st->sweeps += 1;
  const bool degenerate = s.n == 0 || !(d2 > 0.0) || !(d1 - d1 == 0.0);
  st->degenerate = degenerate ? 1 : 0;
  if (degenerate || st->iterations >= max_iter) return;
  const double beta = (double)st->beta;
  double nb = beta - d1 / d2;
  nb = nb < 0.25 * beta ? 0.25 * beta : nb;
  nb = nb > 4.0 * beta ? 4.0 * beta : nb;
  int at_bound = 0;
  if (nb <= (double)kBetaMin) {
    nb = (double)kBetaMin;
    at_bound = 1;
  }
  if (nb >= (double)kBetaMax) {
    nb = (double)kBetaMax;
    at_bound = 1;
  }
  const float nb32 = (float)nb;
  st->at_bound = at_bound;
  if (!at_bound && fabs((double)nb32 - beta) <= rtol * beta) {
    st->converged = 1;
    st->done = 1;
  } else if (at_bound && nb32 == st->beta) {
    st->done = 1;  // on the limit, the step beyond it: nothing moves any more
  } else if (nb32 != st->beta) {
    st->beta = nb32;
    st->iterations += 1;
  }
}

// --------------------------------------------------------------- the report
struct ReportArgs {
  RowArgs r;
  int32_t nb;
  float edges[BDL_TEMPER_MAX_BINS];
};

struct Tot {
  int64_t n, n_lab, n_nonf, n_wrong;
  double nll, ent, conf;

  static __device__ __forceinline__ Tot zero() {
    Tot s;
    s.n = s.n_lab = s.n_nonf = s.n_wrong = 0;
    s.nll = s.ent = s.conf = 0.0;
    return s;
  }
  __device__ __forceinline__ void add(const Tot& o) {
    n += o.n;
    n_lab += o.n_lab;
    n_nonf += o.n_nonf;
    n_wrong += o.n_wrong;
    nll += o.nll;
    ent += o.ent;
    conf += o.conf;
  }
  static __device__ __forceinline__ Tot load(const bdl_temper_totals& p) {
    Tot s;
    s.n = p.n;
    s.n_lab = p.n_labelled;
    s.n_nonf = p.n_nonfinite;
    s.n_wrong = p.n_wrong;
    s.nll = p.nll_sum;
    s.ent = p.entropy_sum;
    s.conf = p.confidence_sum;
    return s;
  }
  __device__ __forceinline__ void store(bdl_temper_totals* __restrict__ p) const {
    p->n = n;
    p->n_labelled = n_lab;
    p->n_nonfinite = n_nonf;
    p->n_wrong = n_wrong;
    p->nll_sum = nll;
    p->entropy_sum = ent;
    p->confidence_sum = conf;
  }
};

struct Bins {
  int64_t cnt, hits;
  double conf;
};

// The workgroup's totals (every wave's scalars in its lane 0, bin j in lane j
// of every wave) summed in wave order and written to — ADD: added to — *out.
__device__ __forceinline__ void block_total(const Tot& tot, const Bins& bn,
                                            bdl_temper_totals* __restrict__ out, bool add) {
  __shared__ Tot s_tot[kWaves];
  __shared__ Bins s_bin[kWaves][64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  __syncthreads();  // the previous call's reads
  if (lane == 0) s_tot[w] = tot;
  s_bin[w][lane] = bn;
  __syncthreads();
  if (t < 64) {
    Bins b = s_bin[0][t];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      b.cnt += s_bin[k][t].cnt;
      b.hits += s_bin[k][t].hits;
      b.conf += s_bin[k][t].conf;
    }
    if (add) {
      b.cnt += out->bin_count[t];
      b.hits += out->bin_hits[t];
      b.conf = out->bin_conf[t] + b.conf;
    }
    out->bin_count[t] = b.cnt;
    out->bin_hits[t] = b.hits;
    out->bin_conf[t] = b.conf;
  }
  if (t == 0) {
    Tot s = s_tot[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s.add(s_tot[k]);
    if (add) {
      Tot o = Tot::load(*out);
      o.add(s);
      s = o;
    }
    s.store(out);
  }
}

template <int NT, bool VEC, bool WAVE>
__global__ __launch_bounds__(kBlock) void bdl_temper_report_kernel(
    const ReportArgs ra, bdl_temper_totals* __restrict__ partials, int nw) {
  __shared__ RedScratch s_red;
  constexpr int TPI = WAVE ? 64 : kBlock;
  constexpr int IPB = WAVE ? kWaves : 1;
  const RowArgs& a = ra.r;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ti = WAVE ? lane : t;
  const int C = a.classes;
  const int Q = (C + 3) >> 2;  // class groups of a row
  int phase = 0;

  for (int g = 0; g < a.groups; ++g) {
    const uint32_t r = rotated_block(g);
    if ((int64_t)r * IPB >= a.batch) continue;  // workgroup-uniform: no example of this group
    const float beta = a.state[g].beta;
    Tot tot = Tot::zero();
    Bins bn = {0, 0, 0.0};
    const int64_t bstride = (int64_t)gridDim.x * IPB;
    int64_t b = (int64_t)r * IPB + (WAVE ? wave : 0);
    f4v cur[NT], nxt[NT];
    if (b < a.batch) load_row<NT, VEC, TPI>(cur, a.logp + ((int64_t)g * a.batch + b) * C, ti, C);
    for (; b < a.batch; b += bstride) {
      const float* __restrict__ row = a.logp + ((int64_t)g * a.batch + b) * C;
      if (b + bstride < a.batch) load_row<NT, VEC, TPI>(nxt, row + bstride * C, ti, C);
      const int64_t lab = a.labels ? a.labels[b] : -1;
      const bool labelled = lab >= 0 && lab < C;
      const float zy = labelled ? sload(row + lab) : 0.0f;

      float zmax;
      int am, nonf;
      row_max<NT, WAVE, TPI>(cur, ti, zmax, am, nonf, s_red, phase);
      const float m = beta * zmax;
      if (nonf || !finite32(m)) {  // uniform over the example's threads
        if (ti == 0) ++tot.n_nonf;
#pragma unroll
        for (int u = 0; u < NT; ++u) cur[u] = nxt[u];
        continue;
      }
      double sum[2] = {0.0, 0.0};
      f4v e[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float tz = beta * cur[u][j];
          const float d = tz - m;
          const float ex = expf(d);
          e[u][j] = ex;
          if (ex != 0.0f) {
            sum[0] += (double)ex;
            sum[1] += (double)ex * (double)d;
          }
        }
      red_sum<WAVE, 2>(sum, s_red, phase);
      const double rz = 1.0 / sum[0];
      if (ti == 0) {
        const double lz = log(sum[0]);
        ++tot.n;
        tot.ent += lz - sum[1] * rz;
        tot.conf += (double)(float)rz;  // q32 of the top class: its e is expf(0) = 1
        if (labelled) {
          const float ty = beta * zy;
          ++tot.n_lab;
          tot.nll += ((double)m + lz) - (double)ty;
          tot.n_wrong += am != (int)lab;
        }
      }
      if (labelled) {  // uniform over the example's threads
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          // lanes of this wave that own a class group in trip u
          int nsrc = Q - ((WAVE ? 0 : wave * 64) + TPI * u);
          nsrc = nsrc < 0 ? 0 : (nsrc > 64 ? 64 : nsrc);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = 4 * (ti + TPI * u) + j;
            const float pj = (float)((double)e[u][j] * rz);
            int k = 0xff;  // no bin: no lane takes it
            if (c < C) {
              k = 0;
              for (int q = 0; q < ra.nb - 1; ++q) k += (pj >= ra.edges[q]) ? 1 : 0;
              k |= (c == lab) ? 0x100 : 0;
            }
            for (int s = 0; s < nsrc; ++s) {
              const int ks = __shfl(k, s, 64);
              const float ps = __shfl(pj, s, 64);
              if ((ks & 0xff) == lane) {
                ++bn.cnt;
                bn.hits += ks >> 8;
                bn.conf += (double)ps;
              }
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < NT; ++u) cur[u] = nxt[u];
    }
    block_total(tot, bn, partials + (int64_t)g * nw + r, false);
  }
}

// One workgroup per group: wave w adds the w-th quarter of the group's
// partials in order (lane j bin j, lane 0 the scalars too), block_total the
// quarters in order and into totals[g].
__global__ __launch_bounds__(kBlock) void bdl_temper_combine_kernel(
    const bdl_temper_totals* __restrict__ partials, int nw, bdl_temper_totals* __restrict__ totals,
    int reset) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bdl_temper_totals* __restrict__ part = partials + (int64_t)blockIdx.x * nw;
  Tot tot = Tot::zero();
  Bins bn = {0, 0, 0.0};
  const int lo = (int)((int64_t)w * nw / kWaves), hi = (int)((int64_t)(w + 1) * nw / kWaves);
  for (int i = lo; i < hi; ++i) {
    bn.cnt += part[i].bin_count[lane];
    bn.hits += part[i].bin_hits[lane];
    bn.conf += part[i].bin_conf[lane];
    if (lane == 0) tot.add(Tot::load(part[i]));
  }
  block_total(tot, bn, totals + blockIdx.x, !reset);
}

// ------------------------------------------------------------------- launch
template <template <int, bool, bool> class L, bool VEC, class... A>
void by_classes(int classes, A&&... a) {
  const int groups4 = (classes + 3) / 4;
  if (classes <= BDL_TEMPER_WAVE_CLASSES)
    L<1, VEC, true>::go(a...);
  else if (groups4 <= kBlock)
    L<1, VEC, false>::go(a...);
  else if (groups4 <= 2 * kBlock)
    L<2, VEC, false>::go(a...);
  else if (groups4 <= 4 * kBlock)
    L<4, VEC, false>::go(a...);
  else
    L<8, VEC, false>::go(a...);
}

template <int NT, bool VEC, bool WAVE>
struct LaunchFit {
  static void go(const RowArgs& a, int grid, int nw, FitPartial* partials, hipStream_t st) {
    hipLaunchKernelGGL((bdl_temper_fit_kernel<NT, VEC, WAVE>), dim3(grid), dim3(kBlock), 0, st, a,
                       partials, nw);
  }
};

template <int NT, bool VEC, bool WAVE>
struct LaunchReport {
  static void go(const ReportArgs& a, int grid, int nw, bdl_temper_totals* partials,
                 hipStream_t st) {
    hipLaunchKernelGGL((bdl_temper_report_kernel<NT, VEC, WAVE>), dim3(grid), dim3(kBlock), 0, st,
                       a, partials, nw);
  }
};

static_assert(BDL_TEMPER_MAX_CLASSES == 8 * 4 * kBlock, "the largest instance covers the limit");
static_assert(BDL_TEMPER_WAVE_CLASSES == 4 * 64, "a wave's lanes own one class group each");
static_assert(sizeof(bdl_temper_totals) == 56 + 24 * BDL_TEMPER_MAX_BINS, "no padding");
static_assert(sizeof(bdl_temper_state) == 88, "no implicit padding");
static_assert(sizeof(FitPartial) <= sizeof(bdl_temper_totals), "one workspace size for both sweeps");

int64_t workspace_bytes(int64_t groups, int64_t grid_blocks) {
  const int64_t g = grid_blocks > 0 ? grid_blocks : BDL_TEMPER_MAX_GRID;
  return groups * g * (int64_t)sizeof(bdl_temper_totals);
}

struct Span {
  const char* name;
  const void* p;
  uint64_t bytes;
};

// What the three entry points share: the ranges, the element index, the
// alignment of the inputs and of the workspace.
int check_rows(const std::string& me, const float* logp, const int64_t* labels, const void* state,
               const void* workspace, int64_t batch, int32_t groups, int32_t classes,
               int32_t grid_blocks) {
  if (!logp) return fail(BDL_ERR_NULL, me + "null logp");
  if (!state) return fail(BDL_ERR_NULL, me + "null state");
  if (!workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (groups < 1 || groups > BDL_TEMPER_MAX_GROUPS)
    return fail(BDL_ERR_ARG, me + "groups in [1, " + std::to_string(BDL_TEMPER_MAX_GROUPS) + "]");
  if (batch < 1) return fail(BDL_ERR_ARG, me + "batch must be >= 1");
  if (classes < 1 || classes > BDL_TEMPER_MAX_CLASSES)
    return fail(BDL_ERR_ARG, me + "classes in [1, " + std::to_string(BDL_TEMPER_MAX_CLASSES) + "]");
  if (grid_blocks < 0 || grid_blocks > BDL_TEMPER_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_TEMPER_MAX_GRID) + "]");
  // every byte offset of logp fits int64
  int64_t lim = INT64_MAX / 4;
  lim /= groups;
  lim /= classes;
  if (batch > lim)
    return fail(BDL_ERR_ARG, me + "groups * batch * classes overflows the element index");
  if (misaligned(logp, 15)) return fail(BDL_ERR_ALIGN, me + "logp not 16-B aligned");
  if (misaligned(workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  if (misaligned(labels, 7)) return fail(BDL_ERR_ALIGN, me + "labels not 8-B aligned");
  if (misaligned(state, 7)) return fail(BDL_ERR_ALIGN, me + "state not 8-B aligned");
  return BDL_OK;
}

// every written span (from first_written on) against the inputs and the other ones
int check_spans(const std::string& me, const Span* spans, int count, int first_written) {
  for (int i = first_written; i < count; ++i)
    for (int j = 0; j < i; ++j)
      if (overlap(spans[i].p, spans[j].p, spans[i].bytes, spans[j].bytes))
        return fail(BDL_ERR_ARG, me + spans[i].name + " overlaps " + spans[j].name);
  return BDL_OK;
}

// The sweep's grid and the partials per group (bdl_predict's default).
void geometry(int64_t batch, int32_t groups, int32_t classes, int32_t grid_blocks, int& grid,
              int& nw) {
  const int64_t ipb = classes <= BDL_TEMPER_WAVE_CLASSES ? kWaves : 1;
  const int64_t per_group = (batch + ipb - 1) / ipb;  // workgroups a group can use
  grid = grid_blocks;
  if (grid == 0) {
    const int64_t want = std::min<int64_t>(per_group, BDL_TEMPER_MAX_GRID) * groups;
    grid = (int)capped_grid(std::min<int64_t>(want, (int64_t)cu_count() * 4), BDL_TEMPER_MAX_GRID);
  }
  nw = (int)std::min<int64_t>(grid, per_group);
}

int check_fit(const char* what, const bdl_temper_fit_args* d) {
  const std::string me = std::string(what) + ": ";
  if (const int rc = no_redirect(what)) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (const int rc = check_rows(me, d->logp, d->labels, d->state, d->workspace, d->batch,
                                d->groups, d->classes, d->grid_blocks))
    return rc;
  if (d->max_iter < 1 || d->max_iter > BDL_TEMPER_MAX_ITER)
    return fail(BDL_ERR_ARG, me + "max_iter in [1, " + std::to_string(BDL_TEMPER_MAX_ITER) + "]");
  if (!(d->rtol >= 0.0) || !(d->rtol < 1.0)) return fail(BDL_ERR_ARG, me + "rtol in [0, 1)");
  const uint64_t gb = (uint64_t)d->groups * (uint64_t)d->batch;
  const Span spans[] = {
      {"logp", d->logp, gb * (uint64_t)d->classes * 4},
      {"labels", d->labels, (uint64_t)d->batch * 8},
      {"state", d->state, (uint64_t)d->groups * sizeof(bdl_temper_state)},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->groups, d->grid_blocks)},
  };
  return check_spans(me, spans, 4, 2);
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_temper_workspace_bytes(int32_t groups, int32_t grid_blocks) {
  if (groups < 1 || groups > BDL_TEMPER_MAX_GROUPS) return 0;
  if (grid_blocks < 0 || grid_blocks > BDL_TEMPER_MAX_GRID) return 0;
  return workspace_bytes(groups, grid_blocks);
}

int bdl_temper_fit_sweep(const bdl_temper_fit_args* d, void* stream) {
  if (const int rc = check_fit("bdl_temper_fit_sweep", d)) return rc;
  RowArgs a;
  a.logp = d->logp;
  a.labels = d->labels;
  a.state = d->state;
  a.batch = d->batch;
  a.groups = d->groups;
  a.classes = d->classes;
  int grid, nw;
  geometry(d->batch, d->groups, d->classes, d->grid_blocks, grid, nw);
  FitPartial* partials = reinterpret_cast<FitPartial*>(d->workspace);
  hipStream_t st = (hipStream_t)stream;
  if (d->classes % 4 == 0)
    by_classes<LaunchFit, true>(d->classes, a, grid, nw, partials, st);
  else
    by_classes<LaunchFit, false>(d->classes, a, grid, nw, partials, st);
  return launched("bdl_temper_fit_sweep");
}

int bdl_temper_fit_update(const bdl_temper_fit_args* d, void* stream) {
  if (const int rc = check_fit("bdl_temper_fit_update", d)) return rc;
  int grid, nw;
  geometry(d->batch, d->groups, d->classes, d->grid_blocks, grid, nw);
  hipLaunchKernelGGL(bdl_temper_update_kernel, dim3(d->groups), dim3(kBlock), 0,
                     (hipStream_t)stream, reinterpret_cast<const FitPartial*>(d->workspace), nw,
                     d->state, d->rtol, (int)d->max_iter);
  return launched("bdl_temper_fit_update");
}

int bdl_temper_report(const bdl_temper_report_args* d, void* stream) {
  const std::string me = "bdl_temper_report: ";
  if (const int rc = no_redirect("bdl_temper_report")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->totals) return fail(BDL_ERR_NULL, me + "null totals");
  if (const int rc = check_rows(me, d->logp, d->labels, d->state, d->workspace, d->batch,
                                d->groups, d->classes, d->grid_blocks))
    return rc;
  if (d->num_bins < 1 || d->num_bins > BDL_TEMPER_MAX_BINS)
    return fail(BDL_ERR_ARG, me + "num_bins in [1, " + std::to_string(BDL_TEMPER_MAX_BINS) + "]");
  if (d->flags & ~BDL_TEMPER_RESET) return fail(BDL_ERR_ARG, me + "unknown flag");
  float prev = 0.0f;
  for (int j = 0; j + 1 < d->num_bins; ++j) {
    const float e = d->edges[j];
    if (!(e > prev) || !(e < 1.0f))
      return fail(BDL_ERR_ARG, me + "edges must be strictly increasing in (0, 1)");
    prev = e;
  }
  if (misaligned(d->totals, 7)) return fail(BDL_ERR_ALIGN, me + "totals not 8-B aligned");
  const uint64_t gb = (uint64_t)d->groups * (uint64_t)d->batch;
  const Span spans[] = {
      {"logp", d->logp, gb * (uint64_t)d->classes * 4},
      {"labels", d->labels, (uint64_t)d->batch * 8},
      {"state", d->state, (uint64_t)d->groups * sizeof(bdl_temper_state)},
      {"totals", d->totals, (uint64_t)d->groups * sizeof(bdl_temper_totals)},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->groups, d->grid_blocks)},
  };
  if (const int rc = check_spans(me, spans, 5, 3)) return rc;

  ReportArgs a;
  a.r.logp = d->logp;
  a.r.labels = d->labels;
  a.r.state = d->state;
  a.r.batch = d->batch;
  a.r.groups = d->groups;
  a.r.classes = d->classes;
  a.nb = d->num_bins;
  for (int j = 0; j < BDL_TEMPER_MAX_BINS; ++j) a.edges[j] = j + 1 < d->num_bins ? d->edges[j] : 2.0f;
  int grid, nw;
  geometry(d->batch, d->groups, d->classes, d->grid_blocks, grid, nw);
  bdl_temper_totals* partials = reinterpret_cast<bdl_temper_totals*>(d->workspace);
  hipStream_t st = (hipStream_t)stream;
  if (d->classes % 4 == 0)
    by_classes<LaunchReport, true>(d->classes, a, grid, nw, partials, st);
  else
    by_classes<LaunchReport, false>(d->classes, a, grid, nw, partials, st);
  hipLaunchKernelGGL(bdl_temper_combine_kernel, dim3(d->groups), dim3(kBlock), 0, st, partials, nw,
                     d->totals, (int)(d->flags & BDL_TEMPER_RESET));
  return launched("bdl_temper_report");
}

}  // extern "C"
