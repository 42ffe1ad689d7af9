// Space-to-depth input pack for strided small-C convolutions (conv1-class
// layers: 3 channels, 11x11, stride 4).
//
// A stride-st convolution over C channels equals a stride-1, pad-0
// convolution with an R'xS' kernel (R' = ceil(R/st), S' = ceil(S/st))
// over the C' = st*st*C channels of the rearranged input
//
//   X'[n][h'][w'][(dy*st+dx)*C + c] = x[n][c][st*h'+dy-ph][st*w'+dx-pw]
//
// (zero where the source coordinate is outside the image), H' = P+R'-1,
// W' = Q+S'-1.  When C' % 8 == 0 the DMA-staged implicit GEMMs
// (gemm_conv_fwd / gemm_conv_dw) take X' as an ordinary channels-last
// input, so the layer needs no col matrix and no small-C staging.
//
// One block builds the [wt][C'] slab of one (n, h') output row in LDS
// and streams it out with 16-byte stores.  The source is read through
// its four element strides, so NCHW-contiguous, channels-last and
// strided-view inputs are packed in place: work items run along w for
// a planar source (one source row per (dy, c) pair) and along (w, c)
// for a channel-minor one, so the loads are contiguous in both.  Every
// element of X' is written, padding zeros included.

#include "common.h"

namespace cosamd {

typedef unsigned short u16;
typedef short s2d_short8 __attribute__((ext_vector_type(8)));

constexpr int kS2dTile = 8192;        // LDS slab, bf16 elements (16 KB)
constexpr int kS2dThreads = 256;

template <int ST>
__global__ __launch_bounds__(kS2dThreads) void s2d_pack_kernel(
    const u16* __restrict__ x, u16* __restrict__ out, int H, int W, int C,
    int st_rt, int ph, int pw, int Hp, int Wp, int WT, int nchunks,
    int64_t sN, int64_t sC, int64_t sH, int64_t sW) {
  __shared__ __attribute__((aligned(16))) u16 tile[kS2dTile];
  const int st = ST ? ST : st_rt;
  const int Cp = st * st * C;
  int b = blockIdx.x;
  int chunk = b % nchunks;
  int t = b / nchunks;
  int hp = t % Hp;
  int n = t / Hp;
  int w0 = chunk * WT;
  int wt = min(WT, Wp - w0);
  int Wf = wt * st;                   // source columns covered (with pad)
  const u16* xn = x + (int64_t)n * sN;

  // 8 source elements per work item: one unaligned 16-byte load where
  // the run is contiguous and inside the image (gfx950 takes unaligned
  // vector loads natively), guarded 2-byte loads at the edges.  Wide
  // loads matter: with 2-byte loads the kernel is bound by the bytes a
  // CU can keep in flight, not by HBM.
  if (sC == 1) {
    // channel-minor source: (w, c) is one contiguous run per source row
    int run = Wf * C;
    int ngrp = (run + 7) >> 3;
    bool vec = sW == C;
    for (int it = threadIdx.x; it < st * ngrp; it += kS2dThreads) {
      int dy = it / ngrp;
      int j0 = (it - dy * ngrp) * 8;
      int hs = hp * st + dy - ph;
      bool rowok = hs >= 0 && hs < H;
      int64_t rbase = (int64_t)hs * sH;
      int wf0 = j0 / C, c0 = j0 - wf0 * C;
      int e0 = (w0 * st - pw) * C + j0;     // offset within the source row
      u16 v[8] = {};
      if (vec && rowok && e0 >= 0 && e0 + 8 <= W * C) {
        __builtin_memcpy(v, xn + rbase + e0, 16);
      } else if (rowok) {
        int wf = wf0, c = c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int ws = w0 * st + wf - pw;
          if (wf < Wf && ws >= 0 && ws < W)
            v[j] = xn[rbase + (int64_t)ws * sW + c];
          if (++c == C) { c = 0; ++wf; }
        }
      }
      int wf = wf0, c = c0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (wf < Wf) {
          int wq = wf / st, dx = wf - wq * st;
          tile[wq * Cp + (dy * st + dx) * C + c] = v[j];
        }
        if (++c == C) { c = 0; ++wf; }
      }
    }
  } else {
    // planar source: each (dy, c) pair is one source row, runs along w
    int ngrp = (Wf + 7) >> 3;
    bool vec = sW == 1;
    for (int it = threadIdx.x; it < st * C * ngrp; it += kS2dThreads) {
      int pair = it / ngrp;
      int wf0 = (it - pair * ngrp) * 8;
      int dy = pair / C, c = pair - dy * C;
      int hs = hp * st + dy - ph;
      bool rowok = hs >= 0 && hs < H;
      int64_t rbase = (int64_t)c * sC + (int64_t)hs * sH;
      int ws0 = w0 * st + wf0 - pw;
      u16 v[8] = {};
      if (vec && rowok && ws0 >= 0 && ws0 + 8 <= W) {
        __builtin_memcpy(v, xn + rbase + ws0, 16);
      } else if (rowok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int ws = ws0 + j;
          if (wf0 + j < Wf && ws >= 0 && ws < W)
            v[j] = xn[rbase + (int64_t)ws * sW];
        }
      }
      int obase = dy * st * C + c;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int wf = wf0 + j;
        if (wf < Wf) {
          int wq = wf / st, dx = wf - wq * st;
          tile[wq * Cp + dx * C + obase] = v[j];
        }
      }
    }
  }
  __syncthreads();

  // Cp % 8 == 0: the slab is a whole number of 16-byte vectors and its
  // global base is 16-byte aligned
  u16* orow = out + (((int64_t)n * Hp + hp) * Wp + w0) * Cp;
  int nvec = (wt * Cp) >> 3;
  for (int v = threadIdx.x; v < nvec; v += kS2dThreads)
    *reinterpret_cast<s2d_short8*>(orow + v * 8) =
        *reinterpret_cast<const s2d_short8*>(tile + v * 8);
}

void s2d_pack(const void* x, void* out, int N, int H, int W, int C, int st,
              int ph, int pw, int Hp, int Wp, int64_t sN, int64_t sC,
              int64_t sH, int64_t sW, hipStream_t stream) {
  int Cp = st * st * C;
  if (Cp % 8 != 0 || Cp > kS2dTile)
    throw std::runtime_error("s2d_pack: st*st*C must be a multiple of 8 "
                             "and at most 8192");
  int WT = (int)hmin<int64_t>(Wp, kS2dTile / Cp);
  int nchunks = (Wp + WT - 1) / WT;
  int64_t blocks = (int64_t)N * Hp * nchunks;
  if (blocks <= 0) return;
  if (blocks >= (1ll << 31))
    throw std::runtime_error("s2d_pack: grid too large");
  const u16* xs = reinterpret_cast<const u16*>(x);
  u16* os = reinterpret_cast<u16*>(out);
#define COS_S2D_PACK(ST)                                                   \
  s2d_pack_kernel<ST><<<(unsigned)blocks, kS2dThreads, 0, stream>>>(       \
      xs, os, H, W, C, st, ph, pw, Hp, Wp, WT, nchunks, sN, sC, sH, sW)
  if (st == 4)      COS_S2D_PACK(4);
  else if (st == 2) COS_S2D_PACK(2);
  else              COS_S2D_PACK(0);
#undef COS_S2D_PACK
}

}  // namespace cosamd
