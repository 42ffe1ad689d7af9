// The LSTM cell, once.  Every kernel that applies it -- the unit op
// (elementwise.hip), the loop route (lstm_seq.hip), the persistent route
// (lstm_persist.hip) and the fused decode step (lstm_step.hip) -- calls
// these two functions, so all routes share their rounding points.  A
// caller keeps its addressing, forms the pre-activations and dh its own
// way, and rounds and stores the results.
//
// Gate order i, f, o, g; fp32 throughout.  The expressions are plain C++
// (no explicit fmaf): every caller gets the compiler's same contraction.
#pragma once

#include "common.h"

namespace cosamd {

struct LstmCellFwd {
  float gi, gf, go, gg;   // activated gates (the backward cache)
  float c, h;
};

// xi..xg: pre-activations; cont gates the carried cell state.
__device__ __forceinline__ LstmCellFwd lstm_cell_fwd(
    float xi, float xf, float xo, float xg, float c_prev, float ct) {
  LstmCellFwd r;
  r.gi = 1.f / (1.f + __expf(-xi));
  r.gf = 1.f / (1.f + __expf(-xf));
  r.go = 1.f / (1.f + __expf(-xo));
  r.gg = tanhf(xg);
  r.c = r.gf * c_prev * ct + r.gi * r.gg;
  r.h = r.go * tanhf(r.c);
  return r;
}

struct LstmCellBwd {
  float di, df, dO, dg;   // pre-activation gate gradients
  float dc_prev;
};

// dhv: gradient into h_t (top diff plus the recurrent term); dc_next: the
// cell-state gradient arriving from t + 1.
__device__ __forceinline__ LstmCellBwd lstm_cell_bwd(
    float gi, float gf, float go, float gg, float c_t, float c_prev,
    float ct, float dhv, float dc_next) {
  float tc = tanhf(c_t);
  float dc = dc_next + dhv * go * (1.f - tc * tc);
  float dov = dhv * tc;
  float div = dc * gg;
  float dgv = dc * gi;
  float dfv = dc * c_prev * ct;
  LstmCellBwd r;
  r.dc_prev = dc * gf * ct;
  r.di = div * gi * (1.f - gi);
  r.df = dfv * gf * (1.f - gf);
  r.dO = dov * go * (1.f - go);
  r.dg = dgv * (1.f - gg * gg);
  return r;
}

}  // namespace cosamd
