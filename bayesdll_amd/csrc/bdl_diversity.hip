// bdl_diversity.hip — pairwise diversity of an ensemble's voters from their
// logits (include/bdl_diversity.h: the definitions, the arithmetic contract,
// the geometry).
//
// One kernel template, bdl_diversity_kernel<NP, VEC, WAVE>.  An example is
// handled by a team: one wave (WAVE: voters <= 16 and classes <= 64, four
// examples per workgroup) or the workgroup.  Pass 1: a wave per voter row, its
// maximum, argmax and non-finite flag, then its fp64 Z, by wave shuffles; the
// row's m, 1/Z, log Z and argmax go to LDS.  Pass 2, per tile of 64 classes:
// the team writes p and lp of every voter into LDS (rows 68 floats apart) and
// thread ti runs over the tile for its NP pairs ti, ti + team size, ... in
// 16-B LDS reads.  The pair accumulators live in registers over all examples of
// the workgroup; a WAVE workgroup adds its four waves' in wave order through
// LDS.  Every workgroup with an example writes one partial; the combine adds
// the partials word by word in workgroup order into the totals.
#include "bdl_chain_common.hpp"
#include "bdl_diversity.h"

namespace bdl {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kTile = BDL_DIVERSITY_TILE;
constexpr int kStride = BDL_DIVERSITY_LDS_STRIDE;
constexpr int kMaxP = BDL_DIVERSITY_MAX_VOTERS;
constexpr int kWaveP = BDL_DIVERSITY_WAVE_VOTERS;
constexpr int kHeaderWords = (int)(sizeof(bdl_diversity_header) / 8);

static_assert(kTile == 64 && kStride % 64 == 4, "16 rows x 16 B at one class cover the 64 banks");
static_assert(kWaves * kWaveP == kMaxP, "the four waves' teams share the workgroup team's tile");
static_assert(kMaxP * (kMaxP - 1) / 2 <= 8 * kBlock, "at most 8 pairs per thread");
static_assert(kWaveP * (kWaveP - 1) / 2 <= 2 * 64, "at most 2 pairs per lane");
static_assert(kHeaderWords == 4, "the matrices start 32 B into the totals");

struct DArgs {
  const float* __restrict__ logits;
  const int64_t* __restrict__ labels;
  int64_t batch;
  int64_t voter_stride;  // batch * classes
  int32_t voters, classes;
};

// The workgroup team uses all kMaxP rows; wave w's team the rows [16 w, 16 w + 16).
struct Lds {
  float p[kMaxP * kStride];
  float lp[kMaxP * kStride];
  double rz[kMaxP];  // 1 / Z_i
  float m[kMaxP];
  float lz[kMaxP];   // logf((float)Z_i)
  int arg[kMaxP];
  int bad[kWaves];
  int64_t stage[kWaves][64];
};

__device__ __forceinline__ f4v pload4(const float* p) { return *(const gf4v*)p; }

// the larger value wins, the lower index among equals
__device__ __forceinline__ void take_max(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

__device__ __forceinline__ void see(float x, int c, float& m, int& am, int& nonf) {
  if (x != x || x == __builtin_inff())
    nonf = 1;
  else if (x > m) {  // a lane's classes ascend: the strict comparison keeps the lowest
    m = x;
    am = c;
  }
}

// One wave, one voter row: its maximum and the lowest index of it; false if it
// holds a NaN, a +inf or no finite entry; else Z, the fp64 sum of expf(x - m)
// (a lane's classes ascending, then the butterfly).
template <bool VEC>
__device__ __forceinline__ bool row_stats(const float* __restrict__ row, int C, int lane, float& m,
                                          int& am, double& z) {
  const float ninf = -__builtin_inff();
  m = ninf;
  am = INT32_MAX;
  int nonf = 0;
  if constexpr (VEC) {
    for (int c0 = 4 * lane; c0 < C; c0 += 4 * 64) {
      const f4v v = pload4(row + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) see(v[j], c0 + j, m, am, nonf);
    }
  } else {
    for (int c = lane; c < C; c += 64) see(sload(row + c), c, m, am, nonf);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(m, off, 64);
    const int oi = __shfl_xor(am, off, 64);
    nonf |= __shfl_xor(nonf, off, 64);
    take_max(m, am, ov, oi);
  }
  if (nonf || m == ninf) return false;  // uniform over the wave
  z = 0.0;
  if constexpr (VEC) {
    for (int c0 = 4 * lane; c0 < C; c0 += 4 * 64) {
      const f4v v = pload4(row + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) z += (double)expf(v[j] - m);
    }
  } else {
    for (int c = lane; c < C; c += 64) z += (double)expf(sload(row + c) - m);
  }
  z = wave_sum(z);
  return true;
}

// WAVE: the four waves' values of a lane added in wave order, in every wave.
template <bool WAVE>
__device__ __forceinline__ int64_t team_total(int64_t v, Lds& s, int lane, int wave) {
  if constexpr (WAVE) {
    s.stage[wave][lane] = v;
    __syncthreads();
    v = s.stage[0][lane];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) v += s.stage[k][lane];
    __syncthreads();
  }
  return v;
}

template <bool WAVE>
__device__ __forceinline__ double team_total(double v, Lds& s, int lane, int wave) {
  if constexpr (WAVE) {
    s.stage[wave][lane] = __double_as_longlong(v);
    __syncthreads();
    v = __longlong_as_double(s.stage[0][lane]);
#pragma unroll
    for (int k = 1; k < kWaves; ++k) v += __longlong_as_double(s.stage[k][lane]);
    __syncthreads();
  }
  return v;
}

// partials + r * part_words: the share of workgroup r (r < nw, the workgroups
// that have an example), in the layout of the totals.
template <int NP, bool VEC, bool WAVE>
__global__ __launch_bounds__(kBlock) void bdl_diversity_kernel(const DArgs a,
                                                               int64_t* __restrict__ partials,
                                                               int64_t part_words, int nw) {
  __shared__ __attribute__((aligned(16))) Lds s;
  constexpr int TPI = WAVE ? 64 : kBlock;  // threads of a team
  constexpr int IPB = WAVE ? kWaves : 1;   // examples per workgroup trip
  if ((int)blockIdx.x >= nw) return;       // workgroup-uniform: no example
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ti = WAVE ? lane : t;
  const int P = a.voters, C = a.classes;
  const int npairs = P * (P - 1) / 2;
  const int vbase = WAVE ? wave * kWaveP : 0;  // the team's rows of the LDS arrays
  const float ninf = -__builtin_inff();
  float* __restrict__ sp = s.p + vbase * kStride;
  float* __restrict__ slp = s.lp + vbase * kStride;

  // the pairs (i < j, row-major) this thread owns
  int pi[NP], pj[NP];
  bool own[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int q = ti + TPI * u;
    own[u] = q < npairs;
    int i = 0, rem = own[u] ? q : 0;
    while (rem >= P - 1 - i) {
      rem -= P - 1 - i;
      ++i;
    }
    pi[u] = i;
    pj[u] = i + 1 + rem;
  }

  int64_t dis[NP], bw[NP], unb_ij[NP], unb_ji[NP];
  double tv[NP], kij[NP], kji[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    dis[u] = bw[u] = unb_ij[u] = unb_ji[u] = 0;
    tv[u] = kij[u] = kji[u] = 0.0;
  }
  int64_t err = 0, n = 0, n_lab = 0, n_nonf = 0;

  const int64_t bstride = (int64_t)gridDim.x * IPB;
  for (int64_t b0 = (int64_t)blockIdx.x * IPB; b0 < a.batch; b0 += bstride) {
    // every barrier below is reached by all four waves: a wave without an
    // example (WAVE, the last trip) and a non-finite example skip the work only
    const int64_t b = b0 + (WAVE ? wave : 0);
    const bool active = b < a.batch;
    if (active) {
      int badw = 0;
      for (int i = WAVE ? 0 : wave; i < P; i += WAVE ? 1 : kWaves) {
        float m;
        int am;
        double z;
        const bool ok =
            row_stats<VEC>(a.logits + (int64_t)i * a.voter_stride + b * C, C, lane, m, am, z);
        badw |= ok ? 0 : 1;
        if (ok && lane == 0) {
          s.m[vbase + i] = m;
          s.rz[vbase + i] = 1.0 / z;
          s.lz[vbase + i] = logf((float)z);
          s.arg[vbase + i] = am;
        }
      }
      if (lane == 0) s.bad[wave] = badw;
    }
    __syncthreads();
    const bool bad = WAVE ? s.bad[wave] != 0 : (s.bad[0] | s.bad[1] | s.bad[2] | s.bad[3]) != 0;
    const bool live = active && !bad;  // team-uniform
    const int64_t lab = (active && a.labels) ? a.labels[b] : -1;
    const bool labelled = lab >= 0 && lab < C;
    if (live) {
#pragma unroll
      for (int u = 0; u < NP; ++u)
        if (own[u]) {
          const int ai = s.arg[vbase + pi[u]], aj = s.arg[vbase + pj[u]];
          dis[u] += ai != aj ? 1 : 0;
          bw[u] += (labelled && ai != lab && aj != lab) ? 1 : 0;
        }
      if (ti < P) err += (labelled && s.arg[vbase + ti] != lab) ? 1 : 0;
      if (ti == 0) {
        ++n;
        n_lab += labelled ? 1 : 0;
      }
    } else if (active && ti == 0) {
      ++n_nonf;
    }

    // this example's sums; bit 0 of ub: KL(i || j) is infinite, bit 1: KL(j || i)
    double tve[NP], kije[NP], kjie[NP];
    int ub[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      tve[u] = kije[u] = kjie[u] = 0.0;
      ub[u] = 0;
    }
    for (int c0 = 0; c0 < C; c0 += kTile) {
      if (live) {
        // p and lp of every voter at the tile's classes; a class >= C reads as masked
        if constexpr (VEC) {
          for (int sl = ti; sl < P * (kTile / 4); sl += TPI) {
            const int i = sl >> 4, c = c0 + 4 * (sl & 15);
            f4v x = {ninf, ninf, ninf, ninf};
            if (c < C) x = vload(a.logits + (int64_t)i * a.voter_stride + b * C + c);
            const float m = s.m[vbase + i], lz = s.lz[vbase + i];
            const double rz = s.rz[vbase + i];
            f4v pv, lv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float d = x[j] - m;
              pv[j] = (float)((double)expf(d) * rz);
              lv[j] = d - lz;
            }
            const int o = i * kStride + 4 * (sl & 15);
            *reinterpret_cast<f4v*>(sp + o) = pv;
            *reinterpret_cast<f4v*>(slp + o) = lv;
          }
        } else {
          for (int sl = ti; sl < P * kTile; sl += TPI) {
            const int i = sl >> 6, c = c0 + (sl & 63);
            const float x = c < C ? sload(a.logits + (int64_t)i * a.voter_stride + b * C + c) : ninf;
            const float d = x - s.m[vbase + i];
            const int o = i * kStride + (sl & 63);
            sp[o] = (float)((double)expf(d) * s.rz[vbase + i]);
            slp[o] = d - s.lz[vbase + i];
          }
        }
      }
      __syncthreads();
      if (live) {
        const int steps = (((C - c0 < kTile) ? C - c0 : kTile) + 3) >> 2;
        for (int g = 0; g < steps; ++g) {
#pragma unroll
          for (int u = 0; u < NP; ++u)
            if (own[u]) {
              const int oi = pi[u] * kStride + 4 * g, oj = pj[u] * kStride + 4 * g;
              const f4v p_i = *reinterpret_cast<const f4v*>(sp + oi);
              const f4v p_j = *reinterpret_cast<const f4v*>(sp + oj);
              const f4v l_i = *reinterpret_cast<const f4v*>(slp + oi);
              const f4v l_j = *reinterpret_cast<const f4v*>(slp + oj);
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                tve[u] += (double)__builtin_fabsf(p_i[k] - p_j[k]);
                const bool mi = l_i[k] == ninf, mj = l_j[k] == ninf;
                // lp_j - lp_i is -(lp_i - lp_j) exactly; a masked side's term is 0
                // (its p is 0); an infinite one is dropped with the example (ub)
                const double dl = (double)(l_i[k] - l_j[k]);
                kije[u] = __builtin_fma((double)p_i[k], mi ? 0.0 : dl, kije[u]);
                kjie[u] = __builtin_fma((double)p_j[k], mj ? 0.0 : -dl, kjie[u]);
                ub[u] |= ((mj && !mi) ? 1 : 0) | ((mi && !mj) ? 2 : 0);
              }
            }
        }
      }
      __syncthreads();  // before the next tile, or the next example's pass 1, is written
    }
    if (live) {
#pragma unroll
      for (int u = 0; u < NP; ++u)
        if (own[u]) {
          tv[u] += 0.5 * tve[u];
          if (ub[u] & 1)
            ++unb_ij[u];
          else
            kij[u] += kije[u];
          if (ub[u] & 2)
            ++unb_ji[u];
          else
            kji[u] += kjie[u];
        }
    }
  }

  int64_t* __restrict__ part = partials + (int64_t)blockIdx.x * part_words;
  const int64_t PP = (int64_t)P * P;
  int64_t* __restrict__ o_dis = part + kHeaderWords;
  int64_t* __restrict__ o_bw = o_dis + PP;
  int64_t* __restrict__ o_unb = o_bw + PP;
  double* __restrict__ o_tv = reinterpret_cast<double*>(o_unb + PP);
  double* __restrict__ o_kl = o_tv + PP;
  const bool writer = !WAVE || wave == 0;
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int64_t d = team_total<WAVE>(dis[u], s, lane, wave);
    const int64_t w = team_total<WAVE>(bw[u], s, lane, wave);
    const int64_t uij = team_total<WAVE>(unb_ij[u], s, lane, wave);
    const int64_t uji = team_total<WAVE>(unb_ji[u], s, lane, wave);
    const double v = team_total<WAVE>(tv[u], s, lane, wave);
    const double k1 = team_total<WAVE>(kij[u], s, lane, wave);
    const double k2 = team_total<WAVE>(kji[u], s, lane, wave);
    if (writer && own[u]) {
      const int ij = pi[u] * P + pj[u], ji = pj[u] * P + pi[u];
      o_dis[ij] = o_dis[ji] = d;
      o_bw[ij] = o_bw[ji] = w;
      o_unb[ij] = uij;
      o_unb[ji] = uji;
      o_tv[ij] = o_tv[ji] = v;
      o_kl[ij] = k1;
      o_kl[ji] = k2;
    }
  }
  err = team_total<WAVE>(err, s, lane, wave);
  n = team_total<WAVE>(n, s, lane, wave);
  n_lab = team_total<WAVE>(n_lab, s, lane, wave);
  n_nonf = team_total<WAVE>(n_nonf, s, lane, wave);
  if (writer && ti < P) {
    const int ii = ti * P + ti;
    o_dis[ii] = 0;
    o_bw[ii] = err;
    o_unb[ii] = 0;
    o_tv[ii] = 0.0;
    o_kl[ii] = 0.0;
  }
  if (writer && ti == 0) {
    part[0] = n;
    part[1] = n_lab;
    part[2] = n_nonf;
    part[3] = P;
  }
}

// Thread w: 8-B word w of the partials in workgroup order, added to — reset:
// written over — word w of the totals.  Words below int_words are int64 (the
// header, disagree, both_wrong, kl_unbounded), the others double.
__global__ __launch_bounds__(kBlock) void bdl_diversity_combine_kernel(
    const int64_t* __restrict__ partials, int64_t part_words, int nw, int64_t* __restrict__ totals,
    int words, int int_words, int P, int reset) {
  const int w = blockIdx.x * kBlock + threadIdx.x;
  if (w >= words) return;
  if (w == 3) {
    totals[w] = P;
  } else if (w < int_words) {
    int64_t v = 0;
    for (int i = 0; i < nw; ++i) v += partials[i * part_words + w];
    if (!reset) v += totals[w];
    totals[w] = v;
  } else {
    double v = 0.0;
    for (int i = 0; i < nw; ++i) v += __longlong_as_double(partials[i * part_words + w]);
    if (!reset) v = __longlong_as_double(totals[w]) + v;
    totals[w] = __double_as_longlong(v);
  }
}

template <int NP, bool VEC, bool WAVE>
void launch(const DArgs& a, int grid, int nw, int64_t* partials, int64_t part_words,
            hipStream_t st) {
  hipLaunchKernelGGL((bdl_diversity_kernel<NP, VEC, WAVE>), dim3(grid), dim3(kBlock), 0, st, a,
                     partials, part_words, nw);
}

bool wave_instance(int voters, int classes) { return voters <= kWaveP && classes <= kTile; }

template <bool VEC>
void launch_by_pairs(const DArgs& a, int grid, int nw, int64_t* partials, int64_t part_words,
                     hipStream_t st) {
  const int npairs = a.voters * (a.voters - 1) / 2;
  if (wave_instance(a.voters, a.classes)) {
    if (npairs <= 64)
      launch<1, VEC, true>(a, grid, nw, partials, part_words, st);
    else
      launch<2, VEC, true>(a, grid, nw, partials, part_words, st);
  } else if (npairs <= kBlock) {
    launch<1, VEC, false>(a, grid, nw, partials, part_words, st);
  } else if (npairs <= 2 * kBlock) {
    launch<2, VEC, false>(a, grid, nw, partials, part_words, st);
  } else if (npairs <= 4 * kBlock) {
    launch<4, VEC, false>(a, grid, nw, partials, part_words, st);
  } else {
    launch<8, VEC, false>(a, grid, nw, partials, part_words, st);
  }
}

int64_t totals_words(int64_t voters) { return kHeaderWords + 5 * voters * voters; }
// a partial starts 16-B aligned
int64_t partial_words(int64_t voters) { return (totals_words(voters) + 1) & ~(int64_t)1; }

// the workgroups the default grid may use at most
int64_t default_grid_cap(int64_t voters) {
  return capped_grid(BDL_DIVERSITY_DEFAULT_WORKSPACE / (8 * partial_words(voters)),
                     BDL_DIVERSITY_MAX_GRID);
}

int64_t workspace_bytes(int64_t voters, int64_t grid_blocks) {
  const int64_t g = grid_blocks > 0 ? grid_blocks : default_grid_cap(voters);
  return g * 8 * partial_words(voters);
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_diversity_totals_bytes(int32_t voters) {
  if (voters < 2 || voters > BDL_DIVERSITY_MAX_VOTERS) return 0;
  return 8 * totals_words(voters);
}

int64_t bdl_diversity_workspace_bytes(int32_t voters, int32_t grid_blocks) {
  if (voters < 2 || voters > BDL_DIVERSITY_MAX_VOTERS) return 0;
  if (grid_blocks < 0 || grid_blocks > BDL_DIVERSITY_MAX_GRID) return 0;
  return workspace_bytes(voters, grid_blocks);
}

int bdl_diversity(const bdl_diversity_args* d, void* stream) {
  const std::string me = "bdl_diversity: ";
  if (const int rc = no_redirect("bdl_diversity")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->logits) return fail(BDL_ERR_NULL, me + "null logits");
  if (!d->totals) return fail(BDL_ERR_NULL, me + "null totals");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->voters < 2 || d->voters > BDL_DIVERSITY_MAX_VOTERS)
    return fail(BDL_ERR_ARG, me + "voters in [2, " + std::to_string(BDL_DIVERSITY_MAX_VOTERS) + "]");
  if (d->batch < 1) return fail(BDL_ERR_ARG, me + "batch must be >= 1");
  if (d->classes < 1 || d->classes > BDL_DIVERSITY_MAX_CLASSES)
    return fail(BDL_ERR_ARG,
                me + "classes in [1, " + std::to_string(BDL_DIVERSITY_MAX_CLASSES) + "]");
  if (d->grid_blocks < 0 || d->grid_blocks > BDL_DIVERSITY_MAX_GRID)
    return fail(BDL_ERR_ARG,
                me + "grid_blocks in [0, " + std::to_string(BDL_DIVERSITY_MAX_GRID) + "]");
  if (d->flags & ~BDL_DIVERSITY_RESET) return fail(BDL_ERR_ARG, me + "unknown flag");
  // every byte offset of logits fits int64
  int64_t lim = INT64_MAX / 4;
  lim /= d->voters;
  lim /= d->classes;
  if (d->batch > lim)
    return fail(BDL_ERR_ARG, me + "voters * batch * classes overflows the element index");
  if (misaligned(d->logits, 15)) return fail(BDL_ERR_ALIGN, me + "logits not 16-B aligned");
  if (misaligned(d->workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  if (misaligned(d->labels, 7)) return fail(BDL_ERR_ALIGN, me + "labels not 8-B aligned");
  if (misaligned(d->totals, 7)) return fail(BDL_ERR_ALIGN, me + "totals not 8-B aligned");

  struct Span {
    const char* name;
    const void* p;
    uint64_t bytes;
  };
  const Span spans[] = {
      {"logits", d->logits, (uint64_t)d->voters * (uint64_t)d->batch * (uint64_t)d->classes * 4},
      {"labels", d->labels, (uint64_t)d->batch * 8},
      {"totals", d->totals, (uint64_t)(8 * totals_words(d->voters))},
      {"workspace", d->workspace, (uint64_t)workspace_bytes(d->voters, d->grid_blocks)},
  };
  for (int i = 2; i < 4; ++i)  // every written span against the inputs and the other one
    for (int j = 0; j < i; ++j)
      if (overlap(spans[i].p, spans[j].p, spans[i].bytes, spans[j].bytes))
        return fail(BDL_ERR_ARG, me + spans[i].name + " overlaps " + spans[j].name);

  DArgs a;
  a.logits = d->logits;
  a.labels = d->labels;
  a.batch = d->batch;
  a.voter_stride = d->batch * d->classes;
  a.voters = d->voters;
  a.classes = d->classes;

  const int64_t ipb = wave_instance(d->voters, d->classes) ? kWaves : 1;
  const int64_t trips = (d->batch + ipb - 1) / ipb;  // workgroups that can have an example
  int grid = d->grid_blocks;
  if (grid == 0)
    grid = (int)capped_grid(std::min<int64_t>(trips, (int64_t)cu_count() * 2),
                            default_grid_cap(d->voters));
  const int nw = (int)std::min<int64_t>(grid, trips);
  int64_t* partials = reinterpret_cast<int64_t*>(d->workspace);
  const int64_t pw = partial_words(d->voters);
  hipStream_t st = (hipStream_t)stream;
  if (d->classes % 4 == 0)
    launch_by_pairs<true>(a, grid, nw, partials, pw, st);
  else
    launch_by_pairs<false>(a, grid, nw, partials, pw, st);
  const int words = (int)totals_words(d->voters);
  const int int_words = kHeaderWords + 3 * d->voters * d->voters;
  hipLaunchKernelGGL(bdl_diversity_combine_kernel, dim3((words + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, st, partials, pw, nw, reinterpret_cast<int64_t*>(d->totals),
                     words, int_words, (int)d->voters, (int)(d->flags & BDL_DIVERSITY_RESET));
  return launched("bdl_diversity");
}

}  // extern "C"
