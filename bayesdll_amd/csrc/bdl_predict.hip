// bdl_predict.hip — predictive uncertainty and calibration from member logits
// (include/bdl_predict.h: the definitions, the arithmetic contract, the
// geometry).
//
// One kernel template, bdl_predict_kernel<NT, VEC, WAVE>.  An example is
// handled by 64 threads (WAVE: classes <= 256, four examples per workgroup,
// wave shuffles only) or by the whole workgroup (two LDS reductions per member
// row).  Thread ti of an example owns the 16-B class groups ti, ti + TPI, ...
// (NT of them, TPI = 64 or 256) of EVERY member row, so the fp64 mixture
// accumulator and the vote counts of its classes stay in its registers for the
// whole member loop; the next member's row is loaded before the current one is
// reduced.  A labelled example's probabilities are binned without atomics: lane
// j of a wave owns bin j (num_bins <= 64) and collects, element slot by element
// slot, the (bin, hit, p) of the wave's lanes in lane order (wave shuffles).  A
// workgroup's totals of a group go through LDS in wave order into its partial;
// the combine adds a group's partials in a fixed order into totals[g].
#include "bdl_chain_common.hpp"
#include "bdl_predict.h"

namespace bdl {
namespace {

constexpr int kWaves = kBlock / 64;

struct PArgs {
  const float* __restrict__ logits;
  const int64_t* __restrict__ labels;
  float* __restrict__ logp;
  float* __restrict__ entropy;
  float* __restrict__ expected_entropy;
  float* __restrict__ mutual_info;
  float* __restrict__ confidence;
  float* __restrict__ nll;
  int32_t* __restrict__ pred;
  int32_t* __restrict__ disagree;
  int64_t batch;
  int64_t member_stride;  // groups * batch * classes
  int32_t members, groups, classes, nb;
  float edges[BDL_PREDICT_MAX_BINS];
};

// The scalar fields of bdl_predict_totals, as a thread / a wave holds them.
struct Tot {
  int64_t n, n_lab, n_nonf, n_wrong, dis;
  double nll, ent, ee, mi, mi_wrong;

  static __device__ __forceinline__ Tot zero() {
    Tot s;
    s.n = s.n_lab = s.n_nonf = s.n_wrong = s.dis = 0;
    s.nll = s.ent = s.ee = s.mi = s.mi_wrong = 0.0;
    return s;
  }
  __device__ __forceinline__ void add(const Tot& o) {
    n += o.n;
    n_lab += o.n_lab;
    n_nonf += o.n_nonf;
    n_wrong += o.n_wrong;
    dis += o.dis;
    nll += o.nll;
    ent += o.ent;
    ee += o.ee;
    mi += o.mi;
    mi_wrong += o.mi_wrong;
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

// the larger value wins, the lower index among equals; flags are or-ed
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

// Every thread of the example gets the two fp64 sums (butterfly, then the
// waves in order).
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

// The class groups q, q + TPI, ... of one member row; a class >= C reads as a
// masked one (-inf).  VEC: C % 4 == 0, every group is whole and 16-B aligned.
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

struct Bins {
  int64_t cnt, hits;
  double conf;
};

// The workgroup's totals (every wave's scalars in its lane 0, bin j in lane j
// of every wave) summed in wave order and written to — ADD: added to — *out.
__device__ __forceinline__ void block_total(const Tot& tot, const Bins& bn,
                                            bdl_predict_totals* __restrict__ out, bool add) {
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
      Tot o;
      o.n = out->n;
      o.n_lab = out->n_labelled;
      o.n_nonf = out->n_nonfinite;
      o.n_wrong = out->n_wrong;
      o.dis = out->disagree_sum;
      o.nll = out->nll_sum;
      o.ent = out->entropy_sum;
      o.ee = out->expected_entropy_sum;
      o.mi = out->mi_sum;
      o.mi_wrong = out->mi_sum_wrong;
      o.add(s);
      s = o;
    }
    out->n = s.n;
    out->n_labelled = s.n_lab;
    out->n_nonfinite = s.n_nonf;
    out->n_wrong = s.n_wrong;
    out->disagree_sum = s.dis;
    out->nll_sum = s.nll;
    out->entropy_sum = s.ent;
    out->expected_entropy_sum = s.ee;
    out->mi_sum = s.mi;
    out->mi_sum_wrong = s.mi_wrong;
  }
}

// partials[g * nw + r]: the share of group g of the workgroup that is r
// workgroups on from the group's first (r < nw = min(grid, ceil(B / IPB))).
template <int NT, bool VEC, bool WAVE>
__global__ __launch_bounds__(kBlock) void bdl_predict_kernel(
    const PArgs a, bdl_predict_totals* __restrict__ partials, int nw) {
  __shared__ RedScratch s_red;
  constexpr int TPI = WAVE ? 64 : kBlock;   // threads per example
  constexpr int IPB = WAVE ? kWaves : 1;    // examples per workgroup iteration
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ti = WAVE ? lane : t;
  const int C = a.classes, M = a.members;
  const int Q = (C + 3) >> 2;  // class groups of a row
  const float ninf = -__builtin_inff();
  const float fnan = __builtin_nanf("");
  const double dM = (double)M;
  int phase = 0;

  for (int g = 0; g < a.groups; ++g) {
    const uint32_t r = rotated_block(g);
    if ((int64_t)r * IPB >= a.batch) continue;  // workgroup-uniform: no example of this group
    Tot tot = Tot::zero();
    Bins bn = {0, 0, 0.0};
    const int64_t bstride = (int64_t)gridDim.x * IPB;
    for (int64_t b = (int64_t)r * IPB + (WAVE ? wave : 0); b < a.batch; b += bstride) {
      const int64_t o = (int64_t)g * a.batch + b;
      const float* __restrict__ row = a.logits + o * C;
      const int64_t lab = a.labels ? a.labels[b] : -1;
      const bool labelled = lab >= 0 && lab < C;

      double acc[NT][4];
      int votes[NT][4];
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[u][j] = 0.0;
          votes[u][j] = 0;
        }
      double hsum = 0.0;
      bool bad = false;
      f4v cur[NT], nxt[NT];
      load_row<NT, VEC, TPI>(cur, row, ti, C);
      for (int i = 0; i < M; ++i) {
        if (i + 1 < M) load_row<NT, VEC, TPI>(nxt, row + (int64_t)(i + 1) * a.member_stride, ti, C);
        // the row's maximum, its lowest index; a NaN or a +inf anywhere
        float m = ninf;
        int am = INT32_MAX, nonf = 0;
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float x = cur[u][j];
            if (x != x || x == __builtin_inff())
              nonf = 1;
            else if (x > m) {
              m = x;
              am = 4 * (ti + TPI * u) + j;
            }
          }
        red_max<WAVE>(m, am, nonf, s_red, phase);
        if (nonf || m == ninf) {  // uniform over the example's threads
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
          for (int j = 0; j < 4; ++j) {
            acc[u][j] += (double)e[u][j] * rz;
            votes[u][j] += (4 * (ti + TPI * u) + j == am) ? 1 : 0;
          }
#pragma unroll
        for (int u = 0; u < NT; ++u) cur[u] = nxt[u];
      }

      if (bad) {
        if (a.logp) {
          f4v nn[NT];
#pragma unroll
          for (int u = 0; u < NT; ++u) nn[u] = f4v{fnan, fnan, fnan, fnan};
          store_row<NT, VEC, TPI>(a.logp + o * C, nn, ti, C);
        }
        if (ti == 0) {
          if (a.entropy) a.entropy[o] = fnan;
          if (a.expected_entropy) a.expected_entropy[o] = fnan;
          if (a.mutual_info) a.mutual_info[o] = fnan;
          if (a.confidence) a.confidence[o] = fnan;
          if (a.nll) a.nll[o] = fnan;
          if (a.pred) a.pred[o] = -1;
          if (a.disagree) a.disagree[o] = -1;
          ++tot.n_nonf;
        }
        continue;
      }

      // the mixture: pbar32, logp, the entropy terms, the vote
      f4v p[NT], lp[NT];
      float best = -1.0f;
      int pred = INT32_MAX, none = 0;
      double ent = 0.0, lpl = 0.0;
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 4 * (ti + TPI * u) + j;
          float pc = 0.0f, lc = 0.0f;
          if (c < C) {
            pc = (float)(acc[u][j] / dM);
            lc = logf(pc);
            if (pc != 0.0f) ent += (double)pc * (double)lc;
            if (c == lab) lpl = (double)lc;
            if (pc > best) {
              best = pc;
              pred = c;
            }
          }
          p[u][j] = pc;
          lp[u][j] = lc;
        }
      if (a.logp) store_row<NT, VEC, TPI>(a.logp + o * C, lp, ti, C);
      red_max<WAVE>(best, pred, none, s_red, phase);
      red_sum2<WAVE>(ent, lpl, s_red, phase);
      double vp = 0.0, unused = 0.0;
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * (ti + TPI * u) + j == pred) vp = (double)votes[u][j];
      red_sum2<WAVE>(vp, unused, s_red, phase);

      const double ent64 = -ent, ee64 = hsum / dM, mi64 = ent64 - ee64;
      const int dis = M - (int)vp;
      const float nllv = labelled ? -(float)lpl : fnan;
      const bool wrong = labelled && pred != (int)lab;
      if (ti == 0) {
        if (a.entropy) a.entropy[o] = (float)ent64;
        if (a.expected_entropy) a.expected_entropy[o] = (float)ee64;
        if (a.mutual_info) a.mutual_info[o] = (float)mi64;
        if (a.confidence) a.confidence[o] = best;
        if (a.nll) a.nll[o] = nllv;
        if (a.pred) a.pred[o] = pred;
        if (a.disagree) a.disagree[o] = dis;
        ++tot.n;
        tot.dis += dis;
        tot.ent += ent64;
        tot.ee += ee64;
        tot.mi += mi64;
        if (labelled) {
          ++tot.n_lab;
          tot.nll += (double)nllv;
          if (wrong) {
            ++tot.n_wrong;
            tot.mi_wrong += mi64;
          }
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
            int k = 0xff;  // no bin: no lane takes it
            if (c < C) {
              k = 0;
              for (int q = 0; q < a.nb - 1; ++q) k += (p[u][j] >= a.edges[q]) ? 1 : 0;
              k |= (c == lab) ? 0x100 : 0;
            }
            const float pj = p[u][j];
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
    }
    block_total(tot, bn, partials + (int64_t)g * nw + r, false);
  }
}

// One workgroup per group: wave w adds the w-th quarter of the group's
// partials in order (lane j bin j, lane 0 the scalars too), block_total the
// quarters in order and into totals[g].
__global__ __launch_bounds__(kBlock) void bdl_predict_combine_kernel(
    const bdl_predict_totals* __restrict__ partials, int nw, bdl_predict_totals* __restrict__ totals,
    int reset) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bdl_predict_totals* __restrict__ part = partials + (int64_t)blockIdx.x * nw;
  Tot tot = Tot::zero();
  Bins bn = {0, 0, 0.0};
  const int lo = (int)((int64_t)w * nw / kWaves), hi = (int)((int64_t)(w + 1) * nw / kWaves);
  for (int i = lo; i < hi; ++i) {
    bn.cnt += part[i].bin_count[lane];
    bn.hits += part[i].bin_hits[lane];
    bn.conf += part[i].bin_conf[lane];
    if (lane == 0) {
      Tot o;
      o.n = part[i].n;
      o.n_lab = part[i].n_labelled;
      o.n_nonf = part[i].n_nonfinite;
      o.n_wrong = part[i].n_wrong;
      o.dis = part[i].disagree_sum;
      o.nll = part[i].nll_sum;
      o.ent = part[i].entropy_sum;
      o.ee = part[i].expected_entropy_sum;
      o.mi = part[i].mi_sum;
      o.mi_wrong = part[i].mi_sum_wrong;
      tot.add(o);
    }
  }
  block_total(tot, bn, totals + blockIdx.x, !reset);
}

template <int NT, bool VEC, bool WAVE>
void launch(const PArgs& a, int grid, int nw, bdl_predict_totals* partials, hipStream_t st) {
  hipLaunchKernelGGL((bdl_predict_kernel<NT, VEC, WAVE>), dim3(grid), dim3(kBlock), 0, st, a,
                     partials, nw);
}

template <bool VEC>
void launch_by_classes(const PArgs& a, int grid, int nw, bdl_predict_totals* partials,
                       hipStream_t st) {
  const int groups4 = (a.classes + 3) / 4;
  if (a.classes <= BDL_PREDICT_WAVE_CLASSES)
    launch<1, VEC, true>(a, grid, nw, partials, st);
  else if (groups4 <= kBlock)
    launch<1, VEC, false>(a, grid, nw, partials, st);
  else if (groups4 <= 2 * kBlock)
    launch<2, VEC, false>(a, grid, nw, partials, st);
  else if (groups4 <= 4 * kBlock)
    launch<4, VEC, false>(a, grid, nw, partials, st);
  else
    launch<8, VEC, false>(a, grid, nw, partials, st);
}

static_assert(BDL_PREDICT_MAX_CLASSES == 8 * 4 * kBlock, "the largest instance covers the limit");
static_assert(BDL_PREDICT_WAVE_CLASSES == 4 * 64, "a wave's lanes own one class group each");
static_assert(sizeof(bdl_predict_totals) == 80 + 24 * BDL_PREDICT_MAX_BINS, "no padding");

int64_t workspace_bytes(int64_t groups, int64_t grid_blocks) {
  const int64_t g = grid_blocks > 0 ? grid_blocks : BDL_PREDICT_MAX_GRID;
  return groups * g * (int64_t)sizeof(bdl_predict_totals);
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_predict_workspace_bytes(int32_t groups, int32_t grid_blocks) {
  if (groups < 1 || groups > BDL_PREDICT_MAX_GROUPS) return 0;
  if (grid_blocks < 0 || grid_blocks > BDL_PREDICT_MAX_GRID) return 0;
  return workspace_bytes(groups, grid_blocks);
}

int bdl_predict(const bdl_predict_args* d, void* stream) {
  const std::string me = "bdl_predict: ";
  if (const int rc = no_redirect("bdl_predict")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->logits) return fail(BDL_ERR_NULL, me + "null logits");
  if (!d->totals) return fail(BDL_ERR_NULL, me + "null totals");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->members < 1) return fail(BDL_ERR_ARG, me + "members must be >= 1");
  if (d->groups < 1 || d->groups > BDL_PREDICT_MAX_GROUPS)
    return fail(BDL_ERR_ARG, me + "groups in [1, " + std::to_string(BDL_PREDICT_MAX_GROUPS) + "]");
  if (d->batch < 1) return fail(BDL_ERR_ARG, me + "batch must be >= 1");
  if (d->classes < 1 || d->classes > BDL_PREDICT_MAX_CLASSES)
    return fail(BDL_ERR_ARG, me + "classes in [1, " + std::to_string(BDL_PREDICT_MAX_CLASSES) + "]");
  if (d->num_bins < 1 || d->num_bins > BDL_PREDICT_MAX_BINS)
    return fail(BDL_ERR_ARG, me + "num_bins in [1, " + std::to_string(BDL_PREDICT_MAX_BINS) + "]");
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_PREDICT_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_PREDICT_MAX_GRID) + "]");
  if (d->flags & ~BDL_PREDICT_RESET) return fail(BDL_ERR_ARG, me + "unknown flag");
  // every byte offset of logits fits int64
  int64_t lim = INT64_MAX / 4;
  lim /= d->members;
  lim /= d->groups;
  lim /= d->classes;
  if (d->batch > lim)
    return fail(BDL_ERR_ARG, me + "members * groups * batch * classes overflows the element index");
  float prev = 0.0f;
  for (int j = 0; j + 1 < d->num_bins; ++j) {
    const float e = d->edges[j];
    if (!(e > prev) || !(e < 1.0f))
      return fail(BDL_ERR_ARG, me + "edges must be strictly increasing in (0, 1)");
    prev = e;
  }
  if (misaligned(d->logits, 15)) return fail(BDL_ERR_ALIGN, me + "logits not 16-B aligned");
  if (misaligned(d->logp, 15)) return fail(BDL_ERR_ALIGN, me + "logp not 16-B aligned");
  if (misaligned(d->workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  if (misaligned(d->labels, 7)) return fail(BDL_ERR_ALIGN, me + "labels not 8-B aligned");
  if (misaligned(d->totals, 7)) return fail(BDL_ERR_ALIGN, me + "totals not 8-B aligned");

  const uint64_t gb = (uint64_t)d->groups * (uint64_t)d->batch;
  struct Span {
    const char* name;
    const void* p;
    uint64_t bytes;
  };
  const Span spans[] = {
      {"logits", d->logits, gb * (uint64_t)d->members * (uint64_t)d->classes * 4},
      {"labels", d->labels, (uint64_t)d->batch * 8},
      {"logp", d->logp, gb * (uint64_t)d->classes * 4},
      {"entropy", d->entropy, gb * 4},
      {"expected_entropy", d->expected_entropy, gb * 4},
      {"mutual_info", d->mutual_info, gb * 4},
      {"confidence", d->confidence, gb * 4},
      {"nll", d->nll, gb * 4},
      {"pred", d->pred, gb * 4},
      {"disagree", d->disagree, gb * 4},
      {"totals", d->totals, (uint64_t)d->groups * sizeof(bdl_predict_totals)},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->groups, d->grid_blocks)},
  };
  constexpr int kSpans = (int)(sizeof(spans) / sizeof(spans[0]));
  for (int i = 3; i < 10; ++i)
    if (misaligned(spans[i].p, 7))
      return fail(BDL_ERR_ALIGN, me + spans[i].name + " not 8-B aligned");
  for (int i = 2; i < kSpans; ++i)  // every written span against the inputs and the other ones
    for (int j = 0; j < i; ++j)
      if (overlap(spans[i].p, spans[j].p, spans[i].bytes, spans[j].bytes))
        return fail(BDL_ERR_ARG, me + spans[i].name + " overlaps " + spans[j].name);

  PArgs a;
  a.logits = d->logits;
  a.labels = d->labels;
  a.logp = d->logp;
  a.entropy = d->entropy;
  a.expected_entropy = d->expected_entropy;
  a.mutual_info = d->mutual_info;
  a.confidence = d->confidence;
  a.nll = d->nll;
  a.pred = d->pred;
  a.disagree = d->disagree;
  a.batch = d->batch;
  a.member_stride = (int64_t)d->groups * d->batch * d->classes;
  a.members = d->members;
  a.groups = d->groups;
  a.classes = d->classes;
  a.nb = d->num_bins;
  for (int j = 0; j < BDL_PREDICT_MAX_BINS; ++j) a.edges[j] = j + 1 < d->num_bins ? d->edges[j] : 2.0f;

  const int64_t ipb = d->classes <= BDL_PREDICT_WAVE_CLASSES ? kWaves : 1;
  const int64_t per_group = (d->batch + ipb - 1) / ipb;  // workgroups a group can use
  int grid = d->grid_blocks;
  if (grid == 0) {
    // one workgroup per example slot of every group (groups <= 65535: no overflow)
    const int64_t want = std::min<int64_t>(per_group, BDL_PREDICT_MAX_GRID) * d->groups;
    grid = (int)capped_grid(std::min<int64_t>(want, (int64_t)cu_count() * 4), BDL_PREDICT_MAX_GRID);
  }
  const int nw = (int)std::min<int64_t>(grid, per_group);
  bdl_predict_totals* partials = reinterpret_cast<bdl_predict_totals*>(d->workspace);
  hipStream_t st = (hipStream_t)stream;
  if (d->classes % 4 == 0)
    launch_by_classes<true>(a, grid, nw, partials, st);
  else
    launch_by_classes<false>(a, grid, nw, partials, st);
  hipLaunchKernelGGL(bdl_predict_combine_kernel, dim3(d->groups), dim3(kBlock), 0, st, partials, nw,
                     d->totals, (int)(d->flags & BDL_PREDICT_RESET));
  return launched("bdl_predict");
}

}  // extern "C"
