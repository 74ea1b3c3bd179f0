// bdl_chain_elem.hpp — the per-element arithmetic of the cross-chain reports
// (include/bdl_diag.h, include/bdl_ess.h) and the adapters between their public
// summary structs and Extreme.  bdl_diag.hip / bdl_ess.hip (the whole-vector
// sweeps) and bdl_layers.hip (the per-tensor tables) instantiate these ONE
// definitions, so an element's value cannot differ between them; so do the two
// folds (bdl_ess.hip of theta, bdl_fn.hip of the probe probabilities).
//
// A: the unit's own kernel-argument struct.  The diagnostic reads ratio,
// inv_ratio, var_floor, c1, fk, fkm1 (K and K - 1 as fp32) and thr0..2 of it;
// the ESS report fS1, fnb1, fKnb (S - 1, nb - 1 and K * nb as fp32) and
// thr0..2.
#pragma once
#include "bdl_chain_common.hpp"
#include "bdl_diag.h"
#include "bdl_ess.h"

namespace bdl {

using DiagStat = Extreme<true>;   // of rhat: every evaluated one is >= 0
using EssStat = Extreme<false>;   // of ess: every evaluated one is finite

// bdl_diag_summary <-> DiagStat
struct DiagSummary {
  static constexpr bool kMax = true;
  static __device__ __forceinline__ DiagStat load(const bdl_diag_summary& p) {
    DiagStat s;
    s.n_eval = p.n_eval;
    s.n_deg = p.n_degenerate;
    s.n_nonf = p.n_nonfinite;
    s.hit0 = p.n_above[0];
    s.hit1 = p.n_above[1];
    s.hit2 = p.n_above[2];
    s.arg = p.argmax;
    s.sum = p.rhat_sum;
    s.ext = p.rhat_max;
    return s;
  }
  static __device__ __forceinline__ void store(bdl_diag_summary* __restrict__ out,
                                               const DiagStat& s) {
    out->n_eval = s.n_eval;
    out->n_degenerate = s.n_deg;
    out->n_nonfinite = s.n_nonf;
    out->argmax = s.arg;
    out->n_above[0] = s.hit0;
    out->n_above[1] = s.hit1;
    out->n_above[2] = s.hit2;
    out->rhat_sum = s.sum;
    out->rhat_max = s.ext;
    out->pad = 0.0f;
  }
};

// bdl_ess_summary <-> EssStat
struct EssSummary {
  static constexpr bool kMax = false;
  static __device__ __forceinline__ EssStat load(const bdl_ess_summary& p) {
    EssStat s;
    s.n_eval = p.n_eval;
    s.n_deg = p.n_degenerate;
    s.n_nonf = p.n_nonfinite;
    s.hit0 = p.n_below[0];
    s.hit1 = p.n_below[1];
    s.hit2 = p.n_below[2];
    s.arg = p.argmin;
    s.sum = p.ess_sum;
    s.ext = p.ess_min;
    return s;
  }
  static __device__ __forceinline__ void store(bdl_ess_summary* __restrict__ out,
                                               const EssStat& s) {
    out->n_eval = s.n_eval;
    out->n_degenerate = s.n_deg;
    out->n_nonfinite = s.n_nonf;
    out->argmin = s.arg;
    out->n_below[0] = s.hit0;
    out->n_below[1] = s.hit1;
    out->n_below[2] = s.hit2;
    out->ess_sum = s.sum;
    out->ess_min = s.ext;
    out->pad = 0.0f;
  }
};

// ------------------------------------------------------------------- R-hat
// One chain's contribution to a group's running sums (include/bdl_diag.h).
template <int VAR, bool RECIP, class A>
__device__ __forceinline__ void diag_accum4(const A& a, const f4v m0, const f4v m, const f4v q,
                                            f4v& S1, f4v& S2, f4v& SW) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float d = m[j] - m0[j];
    S1[j] = S1[j] + d;
    const float t = d * d;
    S2[j] = S2[j] + t;
    SW[j] = SW[j] + posterior_var<VAR, RECIP>(m[j], q[j], a.ratio, a.inv_ratio, a.var_floor);
  }
}

// One element from its sums: outputs and the lane's statistics.
template <class A>
__device__ __forceinline__ void diag_finish_elem(const A& a, float m0, float S1, float S2,
                                                 float SW, int64_t idx, float& pm, float& pv,
                                                 float& rh, DiagStat& s) {
  const float q = S1 / a.fk;
  pm = m0 + q;
  const float p = S1 * S1;
  const float r = p / a.fk;
  const float u = S2 - r;
  const float ss = u < 0.0f ? 0.0f : u;
  const float Bn = ss / a.fkm1;
  const float W = SW / a.fk;
  const float wa = W * a.c1;
  const float b = wa + Bn;
  const float c = b / W;
  const float rhat = sqrtf(c);
  const float e = ss / a.fk;
  pv = W + e;
  if (S2 == 0.0f) {
    rh = __builtin_nanf("");
    ++s.n_deg;
  } else {
    rh = rhat;
    if (!__builtin_isfinite(rhat))
      ++s.n_nonf;
    else
      count_value(s, rhat, idx, a.thr0, a.thr1, a.thr2);
  }
}

// --------------------------------------------------------------------- ESS
// One element of the batch-means fold (include/bdl_ess.h, one rounding per
// line): the sample x into its Welford mean / M2, its open batch sum and, on a
// CLOSE, the M2 of the batch means.  bdl_ess.hip folds theta with it,
// bdl_fn.hip the probe probabilities.
template <int FLAGS>
__device__ __forceinline__ void ess_fold_elem(float x, float& sm, float& M, float& bs, float& B,
                                              float fs, float fb, float c) {
  constexpr bool kFirstSample = FLAGS & BDL_ESS_FIRST_SAMPLE;
  constexpr bool kFirstInBatch = FLAGS & BDL_ESS_FIRST_IN_BATCH;
  constexpr bool kClose = FLAGS & BDL_ESS_CLOSE;
  constexpr bool kFirstBatch = FLAGS & BDL_ESS_FIRST_BATCH;
  if constexpr (kFirstSample) {
    sm = x;
    M = 0.0f;
  } else {
    const float d = x - sm;
    const float q = d / fs;
    sm = sm + q;
    const float d2 = x - sm;
    const float t = d * d2;
    M = M + t;
  }
  if constexpr (kFirstInBatch)
    bs = x;
  else
    bs = bs + x;
  if constexpr (kClose) {
    if constexpr (kFirstBatch) {
      B = 0.0f;
    } else {
      const float y = bs / fb;
      const float ee = y - sm;
      const float t = ee * ee;
      const float u = t * c;
      B = B + u;
    }
  }
}

__device__ __forceinline__ void ess_accum4(const f4v m, const f4v q, f4v& SW, f4v& SV) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    SW[j] = SW[j] + m[j];
    SV[j] = SV[j] + q[j];
  }
}

// One element from its sums: outputs and the lane's statistics.
template <class A>
__device__ __forceinline__ void ess_finish_elem(const A& a, float SW, float SV, int64_t idx,
                                                float& es, float& mc, EssStat& s) {
  const float w = SW / a.fS1;
  const float v = SV / a.fnb1;
  const float r = w / v;
  const float ess = r * a.fKnb;
  const float g = v / a.fKnb;
  mc = sqrtf(g);
  if (SV == 0.0f) {
    es = __builtin_nanf("");
    ++s.n_deg;
  } else {
    es = ess;
    if (!__builtin_isfinite(ess))
      ++s.n_nonf;
    else
      count_value(s, ess, idx, a.thr0, a.thr1, a.thr2);
  }
}

}  // namespace bdl
