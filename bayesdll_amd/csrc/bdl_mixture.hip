// bdl_mixture.hip — the cycle-end likelihood pass and the weighted predictive
// of stacked cyclical chains (include/bdl_mixture.h: the definitions, the
// arithmetic contracts, the geometry).
//
// Two kernel templates, bdl_member_score_kernel<NT, VEC, WAVE> and
// bdl_mixture_kernel<NT, VEC, WAVE, REF>, on a (grid_blocks, pairs) grid.  A
// row is handled by 64 threads (WAVE: classes <= 256, four rows per workgroup,
// wave shuffles only) or by the whole workgroup (LDS reductions).  Thread ti of
// a row owns the 16-B class groups ti, ti + TPI, ... (NT of them, TPI = 64 or
// 256) — bdl_predict's layout and reduction order, written afresh here, so
// that the arithmetic mixture with all weight on one component is bdl_predict
// on its members bit for bit.  The mixture keeps two fp64 accumulators per
// class (the component's, the mixture's) in the thread's registers over the
// member loop; the next row is loaded before the current one is reduced.  A
// workgroup's counts go through LDS in wave order into its partial; the
// combine adds a pair's partials in a fixed order.
#include "bdl_chain_common.hpp"
#include "bdl_mixture.h"

namespace bdl {
namespace {

constexpr int kWaves = kBlock / 64;

// What a thread / a wave / a workgroup has counted, and a partial in the
// workspace: (n, n_nonfinite, n_wrong, nll_sum) of the score, (n, n_nonfinite,
// -, expected_entropy_sum) of the mixture.
struct Acc {
  int64_t n, n_nonf, n_wrong;
  double sum;

  static __device__ __forceinline__ Acc zero() {
    Acc s;
    s.n = s.n_nonf = s.n_wrong = 0;
    s.sum = 0.0;
    return s;
  }
  __device__ __forceinline__ void add(const Acc& o) {
    n += o.n;
    n_nonf += o.n_nonf;
    n_wrong += o.n_wrong;
    sum += o.sum;
  }
};

// Two slots per reduction buffer: consecutive reductions alternate, so a slot
// is rewritten only after a barrier that every thread passed after its reads.
struct RedScratch {
  float v[2][kWaves];
  int i[2][kWaves];
  int f[2][kWaves];
  double a[2][kWaves];
  double b[2][kWaves];
};

// the larger value wins, the lower index among equals
__device__ __forceinline__ void take_max(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// Every thread of the row gets (max, its lowest index, or of the flags).
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

// Every thread of the row gets the two fp64 sums (butterfly, then the waves in
// order).
template <bool WAVE>
__device__ __forceinline__ void red_sum2(double& a, double& b, RedScratch& s, int& phase) {
  a = wave_sum(a);
  b = wave_sum(b);
  if constexpr (!WAVE) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      s.a[phase][w] = a;
      s.b[phase][w] = b;
    }
    __syncthreads();
    a = s.a[phase][0];
    b = s.b[phase][0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      a += s.a[phase][k];
      b += s.b[phase][k];
    }
    phase ^= 1;
  }
}

// Every thread of the row gets the fp64 maximum.
template <bool WAVE>
__device__ __forceinline__ void red_max64(double& a, RedScratch& s, int& phase) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(a, off, 64);
    a = o > a ? o : a;
  }
  if constexpr (!WAVE) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s.a[phase][w] = a;
    __syncthreads();
    a = s.a[phase][0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) a = s.a[phase][k] > a ? s.a[phase][k] : a;
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

template <int NT, bool VEC, int TPI>
__device__ __forceinline__ void store_row(float* __restrict__ row, const f4v (&x)[NT], int q, int C) {
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int c0 = 4 * (q + TPI * u);
    if constexpr (VEC) {
      if (c0 < C) vstore(row + c0, x[u]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) sstore(row + c0 + j, x[u][j]);
    }
  }
}

// The row's maximum with its lowest index, and whether it is non-finite (a NaN
// or a +inf anywhere, or no finite entry); uniform over the row's threads.
template <int NT, bool WAVE, int TPI>
__device__ __forceinline__ bool row_max(const f4v (&x)[NT], int ti, float& m, int& am,
                                        RedScratch& s, int& phase) {
  const float ninf = -__builtin_inff();
  m = ninf;
  am = INT32_MAX;
  int nonf = 0;
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
  return nonf || m == ninf;
}

// The workgroup's counts (every wave's in its lane 0) summed in wave order
// into *out.
__device__ __forceinline__ void block_total(const Acc& acc, Acc* __restrict__ out) {
  __shared__ Acc s_acc[kWaves];
  const int t = threadIdx.x;
  if ((t & 63) == 0) s_acc[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    Acc s = s_acc[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s.add(s_acc[k]);
    *out = s;
  }
}

struct SArgs {
  const float* __restrict__ logits;
  const int64_t* __restrict__ labels;
  int64_t batch;
  int32_t classes;
};

// partials[pair * gridDim.x + blockIdx.x], pair = blockIdx.y = member*groups + group
template <int NT, bool VEC, bool WAVE>
__global__ __launch_bounds__(kBlock) void bdl_member_score_kernel(const SArgs a,
                                                                  Acc* __restrict__ partials) {
  __shared__ RedScratch s_red;
  constexpr int TPI = WAVE ? 64 : kBlock;  // threads per row
  constexpr int IPB = WAVE ? kWaves : 1;   // rows per workgroup iteration
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ti = WAVE ? lane : t;
  const int C = a.classes;
  const float* __restrict__ base = a.logits + (int64_t)blockIdx.y * a.batch * C;
  const int64_t bstride = (int64_t)gridDim.x * IPB;
  int phase = 0;
  Acc acc = Acc::zero();

  int64_t b = (int64_t)blockIdx.x * IPB + (WAVE ? wave : 0);
  f4v cur[NT], nxt[NT];
  if (b < a.batch) load_row<NT, VEC, TPI>(cur, base + b * C, ti, C);
  for (; b < a.batch; b += bstride) {
    if (b + bstride < a.batch) load_row<NT, VEC, TPI>(nxt, base + (b + bstride) * C, ti, C);
    const int64_t lab = a.labels[b];
    if (lab >= 0 && lab < C) {  // uniform over the row's threads
      float m;
      int am;
      if (row_max<NT, WAVE, TPI>(cur, ti, m, am, s_red, phase)) {
        if (ti == 0) ++acc.n_nonf;
      } else {
        double z = 0.0, xl = 0.0;  // xl: the label's logit, from the thread that owns it
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float d = cur[u][j] - m;
            z += (double)expf(d);
            if (4 * (ti + TPI * u) + j == (int)lab) xl = (double)cur[u][j];
          }
        red_sum2<WAVE>(z, xl, s_red, phase);
        const float lse = m + logf((float)z);
        const float nll = lse - (float)xl;
        if (ti == 0) {
          ++acc.n;
          acc.n_wrong += am != (int)lab;
          acc.sum += (double)nll;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NT; ++u) cur[u] = nxt[u];
  }
  block_total(acc, partials + (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

struct MArgs {
  const float* __restrict__ logits;
  const double* __restrict__ weights;
  float* __restrict__ logp;
  float* __restrict__ expected_entropy;
  int64_t batch;
  int64_t member_stride;  // groups * batch * classes
  int32_t components, draws, groups, classes;
};

// the first component >= c of group g that is not skipped (components: none)
__device__ __forceinline__ int next_component(const MArgs& a, int g, int c) {
  while (c < a.components && a.weights[(int64_t)c * a.groups + g] < BDL_MIXTURE_MIN_WEIGHT) ++c;
  return c;
}

// partials[group * gridDim.x + blockIdx.x], group = blockIdx.y
template <int NT, bool VEC, bool WAVE, bool REF>
__global__ __launch_bounds__(kBlock) void bdl_mixture_kernel(const MArgs a,
                                                             Acc* __restrict__ partials) {
  __shared__ RedScratch s_red;
  constexpr int TPI = WAVE ? 64 : kBlock;  // threads per example
  constexpr int IPB = WAVE ? kWaves : 1;   // examples per workgroup iteration
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ti = WAVE ? lane : t;
  const int C = a.classes, g = blockIdx.y, D = a.draws;
  const float ninf = -__builtin_inff();
  const float fnan = __builtin_nanf("");
  const double dD = (double)D;
  const int64_t bstride = (int64_t)gridDim.x * IPB;
  int phase = 0;
  Acc tot = Acc::zero();

  for (int64_t b = (int64_t)blockIdx.x * IPB + (WAVE ? wave : 0); b < a.batch; b += bstride) {
    const int64_t o = (int64_t)g * a.batch + b;
    const float* __restrict__ row = a.logits + o * C;  // member 0's; member i: + i * member_stride

    double mix[NT][4];
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) mix[u][j] = 0.0;
    double hmix = 0.0;
    bool bad = false;
    f4v cur[NT], nxt[NT];
    int c = next_component(a, g, 0);
    if (c < a.components) load_row<NT, VEC, TPI>(cur, row + (int64_t)c * D * a.member_stride, ti, C);
    while (c < a.components) {
      const int cn = next_component(a, g, c + 1);
      const double w = a.weights[(int64_t)c * a.groups + g];
      double acc[NT][4];
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[u][j] = 0.0;
      double hsum = 0.0;
      for (int s = 0; s < D; ++s) {
        const int64_t i = (int64_t)c * D + s;
        if (s + 1 < D)
          load_row<NT, VEC, TPI>(nxt, row + (i + 1) * a.member_stride, ti, C);
        else if (cn < a.components)
          load_row<NT, VEC, TPI>(nxt, row + (int64_t)cn * D * a.member_stride, ti, C);
        float m;
        int am;
        if (row_max<NT, WAVE, TPI>(cur, ti, m, am, s_red, phase)) {  // uniform over the example
          bad = true;
          break;
        }
        double z = 0.0, td = 0.0;
        f4v e[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float d = cur[u][j] - m;
            const float ex = expf(d);
            e[u][j] = ex;
            z += (double)ex;
            if (ex != 0.0f) td += (double)ex * (double)d;
          }
        red_sum2<WAVE>(z, td, s_red, phase);
        const double rz = 1.0 / z;
        hsum += (double)logf((float)z) - td * rz;
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[u][j] += (double)e[u][j] * rz;
#pragma unroll
        for (int u = 0; u < NT; ++u) cur[u] = nxt[u];
      }
      if (bad) break;
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double pb = acc[u][j] / dD;
          if constexpr (REF)
            mix[u][j] += w * (double)logf((float)pb);
          else
            mix[u][j] += w * pb;
        }
      hmix += w * (hsum / dD);
      c = cn;
    }

    if (bad) {
      if (a.logp) {
        f4v nn[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) nn[u] = f4v{fnan, fnan, fnan, fnan};
        store_row<NT, VEC, TPI>(a.logp + o * C, nn, ti, C);
      }
      if (ti == 0) {
        if (a.expected_entropy) a.expected_entropy[o] = fnan;
        ++tot.n_nonf;
      }
      continue;
    }

    if (a.logp) {  // uniform over the grid
      f4v lp[NT];
      if constexpr (REF) {
        // t - logsumexp(t) over the classes, fp64
        double mx = (double)ninf;
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * (ti + TPI * u) + j < C && mix[u][j] > mx) mx = mix[u][j];
        red_max64<WAVE>(mx, s_red, phase);
        double se = 0.0, unused = 0.0;
        if (mx != (double)ninf) {
#pragma unroll
          for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (4 * (ti + TPI * u) + j < C) se += exp(mix[u][j] - mx);
        }
        red_sum2<WAVE>(se, unused, s_red, phase);
        const double lse = mx + log(se);
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            lp[u][j] = mx != (double)ninf ? (float)(mix[u][j] - lse) : ninf;
      } else {
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            lp[u][j] = 4 * (ti + TPI * u) + j < C ? logf((float)mix[u][j]) : 0.0f;
      }
      store_row<NT, VEC, TPI>(a.logp + o * C, lp, ti, C);
    }
    if (ti == 0) {
      if (a.expected_entropy) a.expected_entropy[o] = (float)hmix;
      ++tot.n;
      tot.sum += hmix;
    }
  }
  block_total(tot, partials + (int64_t)g * gridDim.x + blockIdx.x);
}

// The public structs against Acc.
struct ScoreOut {
  using T = bdl_member_score_t;
  static __device__ __forceinline__ Acc load(const T& o) {
    Acc s;
    s.n = o.n;
    s.n_nonf = o.n_nonfinite;
    s.n_wrong = o.n_wrong;
    s.sum = o.nll_sum;
    return s;
  }
  static __device__ __forceinline__ void store(T* o, const Acc& s) {
    o->n = s.n;
    o->n_nonfinite = s.n_nonf;
    o->n_wrong = s.n_wrong;
    o->nll_sum = s.sum;
  }
};

struct MixOut {
  using T = bdl_mixture_totals;
  static __device__ __forceinline__ Acc load(const T& o) {
    Acc s;
    s.n = o.n;
    s.n_nonf = o.n_nonfinite;
    s.n_wrong = 0;
    s.sum = o.expected_entropy_sum;
    return s;
  }
  static __device__ __forceinline__ void store(T* o, const Acc& s) {
    o->n = s.n;
    o->n_nonfinite = s.n_nonf;
    o->expected_entropy_sum = s.sum;
  }
};

// One workgroup per pair: thread t adds the pair's partials t, t + 256, ... in
// order, the wave butterfly, the waves in order; added to — reset: written
// over — out[pair].
template <class O>
__global__ __launch_bounds__(kBlock) void bdl_mixture_combine_kernel(
    const Acc* __restrict__ partials, int nw, typename O::T* __restrict__ out, int reset) {
  const Acc* __restrict__ part = partials + (int64_t)blockIdx.x * nw;
  Acc s = Acc::zero();
  for (int i = threadIdx.x; i < nw; i += kBlock) s.add(part[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s.n += __shfl_xor(s.n, off, 64);
    s.n_nonf += __shfl_xor(s.n_nonf, off, 64);
    s.n_wrong += __shfl_xor(s.n_wrong, off, 64);
  }
  s.sum = wave_sum(s.sum);
  __shared__ Acc s_tot;
  block_total(s, &s_tot);
  if (threadIdx.x == 0) {
    Acc r = s_tot;
    if (!reset) {
      Acc o = O::load(out[blockIdx.x]);
      o.add(r);
      r = o;
    }
    O::store(out + blockIdx.x, r);
  }
}

template <int NT, bool VEC, bool WAVE>
void launch_score(const SArgs& a, dim3 grid, Acc* partials, hipStream_t st) {
  hipLaunchKernelGGL((bdl_member_score_kernel<NT, VEC, WAVE>), grid, dim3(kBlock), 0, st, a,
                     partials);
}

template <bool VEC>
void score_by_classes(const SArgs& a, dim3 grid, Acc* partials, hipStream_t st) {
  const int groups4 = (a.classes + 3) / 4;
  if (a.classes <= BDL_MIXTURE_WAVE_CLASSES)
    launch_score<1, VEC, true>(a, grid, partials, st);
  else if (groups4 <= kBlock)
    launch_score<1, VEC, false>(a, grid, partials, st);
  else if (groups4 <= 2 * kBlock)
    launch_score<2, VEC, false>(a, grid, partials, st);
  else
    launch_score<4, VEC, false>(a, grid, partials, st);
}

template <int NT, bool VEC, bool WAVE>
void launch_mix(const MArgs& a, bool ref, dim3 grid, Acc* partials, hipStream_t st) {
  if (ref)
    hipLaunchKernelGGL((bdl_mixture_kernel<NT, VEC, WAVE, true>), grid, dim3(kBlock), 0, st, a,
                       partials);
  else
    hipLaunchKernelGGL((bdl_mixture_kernel<NT, VEC, WAVE, false>), grid, dim3(kBlock), 0, st, a,
                       partials);
}

template <bool VEC>
void mix_by_classes(const MArgs& a, bool ref, dim3 grid, Acc* partials, hipStream_t st) {
  const int groups4 = (a.classes + 3) / 4;
  if (a.classes <= BDL_MIXTURE_WAVE_CLASSES)
    launch_mix<1, VEC, true>(a, ref, grid, partials, st);
  else if (groups4 <= kBlock)
    launch_mix<1, VEC, false>(a, ref, grid, partials, st);
  else if (groups4 <= 2 * kBlock)
    launch_mix<2, VEC, false>(a, ref, grid, partials, st);
  else
    launch_mix<4, VEC, false>(a, ref, grid, partials, st);
}

static_assert(BDL_MIXTURE_MAX_CLASSES == 4 * 4 * kBlock, "the largest instance covers the limit");
static_assert(BDL_MIXTURE_WAVE_CLASSES == 4 * 64, "a wave's lanes own one class group each");
static_assert(sizeof(Acc) == 32 && sizeof(bdl_member_score_t) == 32 &&
                  sizeof(bdl_mixture_totals) == 24,
              "no padding");

int64_t workspace_bytes(int64_t pairs, int64_t grid_blocks) {
  const int64_t g = grid_blocks > 0 ? grid_blocks : BDL_MIXTURE_MAX_GRID;
  return pairs * g * (int64_t)sizeof(Acc);
}

// grid_blocks, or the default: one workgroup per row slot of a pair, up to
// four per CU over all pairs
int blocks_per_pair(int32_t grid_blocks, int64_t batch, int32_t classes, int64_t pairs) {
  if (grid_blocks > 0) return grid_blocks;
  const int64_t ipb = classes <= BDL_MIXTURE_WAVE_CLASSES ? kWaves : 1;
  const int64_t slots = (batch + ipb - 1) / ipb;
  const int64_t share = ((int64_t)cu_count() * 4 + pairs - 1) / pairs;
  return (int)capped_grid(std::min(slots, share), BDL_MIXTURE_MAX_GRID);
}

struct Span {
  const char* name;
  const void* p;
  uint64_t bytes;
};

// spans[first_written ..] against the spans before them; nullptr: none overlap
template <int N>
bool spans_overlap(const Span (&spans)[N], int first_written, std::string& what) {
  for (int i = first_written; i < N; ++i)
    for (int j = 0; j < i; ++j)
      if (overlap(spans[i].p, spans[j].p, spans[i].bytes, spans[j].bytes)) {
        what = std::string(spans[i].name) + " overlaps " + spans[j].name;
        return true;
      }
  return false;
}

// members * groups * batch * classes * 4 fits int64 (every factor >= 1)
bool logits_fit(int64_t members, int64_t groups, int64_t batch, int64_t classes) {
  int64_t lim = INT64_MAX / 4;
  lim /= members;
  lim /= groups;
  lim /= classes;
  return batch <= lim;
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_member_score_workspace_bytes(int32_t members, int32_t groups, int32_t grid_blocks) {
  if (members < 1 || groups < 1 || (int64_t)members * groups > BDL_MIXTURE_MAX_PAIRS) return 0;
  if (grid_blocks < 0 || grid_blocks > BDL_MIXTURE_MAX_GRID) return 0;
  return workspace_bytes((int64_t)members * groups, grid_blocks);
}

int64_t bdl_mixture_workspace_bytes(int32_t groups, int32_t grid_blocks) {
  if (groups < 1 || groups > BDL_MIXTURE_MAX_PAIRS) return 0;
  if (grid_blocks < 0 || grid_blocks > BDL_MIXTURE_MAX_GRID) return 0;
  return workspace_bytes(groups, grid_blocks);
}

int bdl_member_score(const bdl_member_score_args* d, void* stream) {
  const std::string me = "bdl_member_score: ";
  if (const int rc = no_redirect("bdl_member_score")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->logits) return fail(BDL_ERR_NULL, me + "null logits");
  if (!d->labels) return fail(BDL_ERR_NULL, me + "null labels");
  if (!d->scores) return fail(BDL_ERR_NULL, me + "null scores");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->members < 1) return fail(BDL_ERR_ARG, me + "members must be >= 1");
  if (d->groups < 1) return fail(BDL_ERR_ARG, me + "groups must be >= 1");
  if ((int64_t)d->members * d->groups > BDL_MIXTURE_MAX_PAIRS)
    return fail(BDL_ERR_ARG, me + "members * groups in [1, " +
                                 std::to_string(BDL_MIXTURE_MAX_PAIRS) + "]");
  if (d->batch < 1) return fail(BDL_ERR_ARG, me + "batch must be >= 1");
  if (d->classes < 1 || d->classes > BDL_MIXTURE_MAX_CLASSES)
    return fail(BDL_ERR_ARG, me + "classes in [1, " + std::to_string(BDL_MIXTURE_MAX_CLASSES) + "]");
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_MIXTURE_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_MIXTURE_MAX_GRID) + "]");
  if (d->flags & ~BDL_MIXTURE_RESET) return fail(BDL_ERR_ARG, me + "unknown flag");
  if (!logits_fit(d->members, d->groups, d->batch, d->classes))
    return fail(BDL_ERR_ARG, me + "members * groups * batch * classes overflows the element index");
  if (misaligned(d->logits, 15)) return fail(BDL_ERR_ALIGN, me + "logits not 16-B aligned");
  if (misaligned(d->workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  if (misaligned(d->labels, 7)) return fail(BDL_ERR_ALIGN, me + "labels not 8-B aligned");
  if (misaligned(d->scores, 7)) return fail(BDL_ERR_ALIGN, me + "scores not 8-B aligned");

  const int64_t pairs = (int64_t)d->members * d->groups;
  const Span spans[] = {
      {"logits", d->logits, (uint64_t)pairs * (uint64_t)d->batch * (uint64_t)d->classes * 4},
      {"labels", d->labels, (uint64_t)d->batch * 8},
      {"scores", d->scores, (uint64_t)pairs * sizeof(bdl_member_score_t)},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(pairs, d->grid_blocks)},
  };
  std::string what;
  if (spans_overlap(spans, 2, what)) return fail(BDL_ERR_ARG, me + what);

  SArgs a;
  a.logits = d->logits;
  a.labels = d->labels;
  a.batch = d->batch;
  a.classes = d->classes;
  const int bpp = blocks_per_pair(d->grid_blocks, d->batch, d->classes, pairs);
  const dim3 grid(bpp, (unsigned)pairs);
  Acc* partials = reinterpret_cast<Acc*>(d->workspace);
  hipStream_t st = (hipStream_t)stream;
  if (d->classes % 4 == 0)
    score_by_classes<true>(a, grid, partials, st);
  else
    score_by_classes<false>(a, grid, partials, st);
  hipLaunchKernelGGL(bdl_mixture_combine_kernel<ScoreOut>, dim3((unsigned)pairs), dim3(kBlock), 0,
                     st, partials, bpp, d->scores, (int)(d->flags & BDL_MIXTURE_RESET));
  return launched("bdl_member_score");
}

int bdl_mixture(const bdl_mixture_args* d, void* stream) {
  const std::string me = "bdl_mixture: ";
  if (const int rc = no_redirect("bdl_mixture")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->logits) return fail(BDL_ERR_NULL, me + "null logits");
  if (!d->weights) return fail(BDL_ERR_NULL, me + "null weights");
  if (!d->totals) return fail(BDL_ERR_NULL, me + "null totals");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->components < 1) return fail(BDL_ERR_ARG, me + "components must be >= 1");
  if (d->draws < 1) return fail(BDL_ERR_ARG, me + "draws must be >= 1");
  if ((int64_t)d->components * d->draws > INT32_MAX)
    return fail(BDL_ERR_ARG, me + "components * draws overflows the member index");
  if (d->groups < 1 || d->groups > BDL_MIXTURE_MAX_PAIRS)
    return fail(BDL_ERR_ARG, me + "groups in [1, " + std::to_string(BDL_MIXTURE_MAX_PAIRS) + "]");
  if (d->batch < 1) return fail(BDL_ERR_ARG, me + "batch must be >= 1");
  if (d->classes < 1 || d->classes > BDL_MIXTURE_MAX_CLASSES)
    return fail(BDL_ERR_ARG, me + "classes in [1, " + std::to_string(BDL_MIXTURE_MAX_CLASSES) + "]");
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_MIXTURE_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_MIXTURE_MAX_GRID) + "]");
  if (d->flags & ~BDL_MIXTURE_RESET) return fail(BDL_ERR_ARG, me + "unknown flag");
  if (d->combine != BDL_MIX_ARITHMETIC && d->combine != BDL_MIX_REFERENCE)
    return fail(BDL_ERR_ARG, me + "unknown combine");
  const int64_t members = (int64_t)d->components * d->draws;
  if (!logits_fit(members, d->groups, d->batch, d->classes))
    return fail(BDL_ERR_ARG, me + "members * groups * batch * classes overflows the element index");
  if (misaligned(d->logits, 15)) return fail(BDL_ERR_ALIGN, me + "logits not 16-B aligned");
  if (misaligned(d->logp, 15)) return fail(BDL_ERR_ALIGN, me + "logp not 16-B aligned");
  if (misaligned(d->workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  if (misaligned(d->weights, 7)) return fail(BDL_ERR_ALIGN, me + "weights not 8-B aligned");
  if (misaligned(d->labels, 7)) return fail(BDL_ERR_ALIGN, me + "labels not 8-B aligned");
  if (misaligned(d->expected_entropy, 7))
    return fail(BDL_ERR_ALIGN, me + "expected_entropy not 8-B aligned");
  if (misaligned(d->totals, 7)) return fail(BDL_ERR_ALIGN, me + "totals not 8-B aligned");

  const uint64_t gb = (uint64_t)d->groups * (uint64_t)d->batch;
  const Span spans[] = {
      {"logits", d->logits, gb * (uint64_t)members * (uint64_t)d->classes * 4},
      {"weights", d->weights, (uint64_t)d->components * (uint64_t)d->groups * 8},
      {"labels", d->labels, (uint64_t)d->batch * 8},
      {"logp", d->logp, gb * (uint64_t)d->classes * 4},
      {"expected_entropy", d->expected_entropy, gb * 4},
      {"totals", d->totals, (uint64_t)d->groups * sizeof(bdl_mixture_totals)},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->groups, d->grid_blocks)},
  };
  std::string what;
  if (spans_overlap(spans, 3, what)) return fail(BDL_ERR_ARG, me + what);

  MArgs a;
  a.logits = d->logits;
  a.weights = d->weights;
  a.logp = d->logp;
  a.expected_entropy = d->expected_entropy;
  a.batch = d->batch;
  a.member_stride = (int64_t)d->groups * d->batch * d->classes;
  a.components = d->components;
  a.draws = d->draws;
  a.groups = d->groups;
  a.classes = d->classes;
  const int bpg = blocks_per_pair(d->grid_blocks, d->batch, d->classes, d->groups);
  const dim3 grid(bpg, (unsigned)d->groups);
  Acc* partials = reinterpret_cast<Acc*>(d->workspace);
  hipStream_t st = (hipStream_t)stream;
  const bool ref = d->combine == BDL_MIX_REFERENCE;
  if (d->classes % 4 == 0)
    mix_by_classes<true>(a, ref, grid, partials, st);
  else
    mix_by_classes<false>(a, ref, grid, partials, st);
  hipLaunchKernelGGL(bdl_mixture_combine_kernel<MixOut>, dim3((unsigned)d->groups), dim3(kBlock),
                     0, st, partials, bpg, d->totals, (int)(d->flags & BDL_MIXTURE_RESET));
  return launched("bdl_mixture");
}

}  // extern "C"
