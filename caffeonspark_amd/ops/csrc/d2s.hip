// Depth-to-space route for strided Deconvolution (transposed convolution),
// the mirror image of the space-to-depth route in s2d.hip.
//
// A stride-st transposed convolution of x[N][Ci][H][W] with the caffe
// weight Wd[Ci][Co][R][S] splits into st*st output phases.  Phase
// (py, px) holds the output pixels with (oh+ph) % st == py and
// (ow+pw) % st == px, and all phases together are ONE stride-1
// convolution of x with an R'xS' kernel (R' = ceil(R/st), S' = ceil(S/st)),
// pads (R'-1, S'-1) and st*st*Co output channels:
//
//   Z[n][h'][w'][(py*st+px)*Co + co] =
//     sum_{r',s',ci} x[n][ci][h'-(R'-1)+r'][w'-(S'-1)+s']
//                    * wrD[(py*st+px)*Co + co][(r'*S'+s')*Ci + ci]
//   wrD[(py*st+px)*Co + co][(r'*S'+s')*Ci + ci] =
//     Wd[ci][co][py + st*(R'-1-r')][px + st*(S'-1-s')]
//
// (a zero "phantom" tap where that row >= R or column >= S), H' = H+R'-1,
// W' = W+S'-1.  gemm_conv_fwd computes Z with bias and ReLU fused; the
// output is then a pure permutation of Z:
//
//   y[n][co][oh][ow] =
//     Z[n][(oh+ph)/st][(ow+pw)/st][(((oh+ph)%st)*st + (ow+pw)%st)*Co + co]
//
// d2s_pack_weight builds wrD, d2s_unpack applies the permutation.

#include "common.h"

namespace cosamd {

typedef unsigned short u16;
typedef short d2s_short8 __attribute__((ext_vector_type(8)));

constexpr int kD2sThreads = 256;

// One work item per (row, tap, channel octet) of the live
// [st*st*Co][R'*S'*Ci] region: 8 source reads Co*R*S apart, one 16-byte
// store.  Every live element is written, phantom zeros included, so the
// buffer needs no memset between calls; pad rows and columns are never
// touched.
__global__ __launch_bounds__(kD2sThreads) void d2s_pack_weight_kernel(
    const u16* __restrict__ src, u16* __restrict__ dst, int Ci, int Co,
    int R, int S, int st, int Rp, int Sp, int Kpad, int64_t total) {
  int Ci8 = Ci >> 3;
  int taps = Rp * Sp;
  int64_t cstride = (int64_t)Co * R * S;
  for (int64_t i = (int64_t)blockIdx.x * kD2sThreads + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * kD2sThreads) {
    int c8 = (int)(i % Ci8);
    int64_t t = i / Ci8;
    int tap = (int)(t % taps);
    int row = (int)(t / taps);
    int co = row % Co, phase = row / Co;
    int py = phase / st, px = phase - py * st;
    int rp = tap / Sp, sp = tap - rp * Sp;
    int r = py + st * (Rp - 1 - rp);
    int s = px + st * (Sp - 1 - sp);
    d2s_short8 v = {};
    if (r < R && s < S) {
      const u16* p = src + ((int64_t)(c8 * 8) * Co + co) * R * S + r * S + s;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (short)p[j * cstride];
    }
    *reinterpret_cast<d2s_short8*>(dst + (int64_t)row * Kpad + tap * Ci +
                                   c8 * 8) = v;
  }
}

void d2s_pack_weight(const void* src, void* dst, int Ci, int Co, int R,
                     int S, int st, int Kpad, hipStream_t stream) {
  if (Ci % 8 != 0 || Kpad % 8 != 0 || st < 2)
    throw std::runtime_error("d2s_pack_weight: Ci and Kpad must be "
                             "multiples of 8 and st >= 2");
  int Rp = (R + st - 1) / st, Sp = (S + st - 1) / st;
  int64_t total = (int64_t)st * st * Co * Rp * Sp * (Ci / 8);
  if (total <= 0) return;
  if ((int64_t)st * st * Co >= (1ll << 31) ||
      (int64_t)Rp * Sp * Ci > Kpad)
    throw std::runtime_error("d2s_pack_weight: bad geometry");
  int blocks = (int)hmin<int64_t>(2048, (total + kD2sThreads - 1) /
                                            kD2sThreads);
  d2s_pack_weight_kernel<<<blocks, kD2sThreads, 0, stream>>>(
      reinterpret_cast<const u16*>(src), reinterpret_cast<u16*>(dst), Ci,
      Co, R, S, st, Rp, Sp, Kpad, total);
}

// Z -> y.  For a fixed (n, oh) the source is runs of st*Co contiguous
// elements, st*st*Co apart (one run per w'), and the destination row is
// those runs back to back, shifted by -pw*Co and cropped to Wo*Co.  One
// work item moves 8 consecutive elements of a destination row.
//   VEC: Co % 8 == 0 and y dense channels-last, so an aligned group of 8
//     never straddles a run and both sides are 16-byte aligned: one
//     16-byte load and one 16-byte store.
//   otherwise: 2-byte accesses, y written through its four strides.
template <bool VEC>
__global__ __launch_bounds__(kD2sThreads) void d2s_unpack_kernel(
    const u16* __restrict__ z, u16* __restrict__ y, int Co, int Ho, int Wo,
    int st, int ph, int pw, int Hp, int Wp, int ngrp, int64_t total,
    int64_t sN, int64_t sC, int64_t sH, int64_t sW) {
  int64_t i = (int64_t)blockIdx.x * kD2sThreads + threadIdx.x;
  if (i >= total) return;
  int g = (int)(i % ngrp);
  int64_t row = i / ngrp;
  int oh = (int)(row % Ho);
  int n = (int)(row / Ho);
  int hq = (oh + ph) / st, py = (oh + ph) - hq * st;
  int run = st * Co;                      // one w' of one phase row
  int Cz = st * run;                      // st*st*Co
  const u16* zrow = z + ((int64_t)n * Hp + hq) * Wp * Cz + py * run;
  u16* yrow = y + (int64_t)n * sN + (int64_t)oh * sH;
  int e0 = g * 8;                         // element of the [Wo][Co] row
  int f0 = e0 + pw * Co;                  // same, before the crop
  int wq = f0 / run, rem = f0 - wq * run;
  if (VEC) {
    *reinterpret_cast<d2s_short8*>(yrow + e0) =
        *reinterpret_cast<const d2s_short8*>(zrow + (int64_t)wq * Cz + rem);
  } else {
    int ow = e0 / Co, co = e0 - ow * Co;
    int lim = Wo * Co - e0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < lim)
        yrow[(int64_t)ow * sW + (int64_t)co * sC] =
            zrow[(int64_t)wq * Cz + rem];
      if (++co == Co) { co = 0; ++ow; }
      if (++rem == run) { rem = 0; ++wq; }
    }
  }
}

void d2s_unpack(const void* z, void* y, int N, int Co, int Ho, int Wo,
                int st, int ph, int pw, int Hp, int Wp, int64_t sN,
                int64_t sC, int64_t sH, int64_t sW, hipStream_t stream) {
  if (st < 2 || ph < 0 || pw < 0 || Co <= 0 ||
      (int64_t)st * st * Co >= (1ll << 31) ||
      (int64_t)(Wo + pw) * Co >= (1ll << 31))
    throw std::runtime_error("d2s_unpack: bad geometry");
  if (N <= 0 || Ho <= 0 || Wo <= 0) return;
  // the last source row / column read must lie inside Z
  if ((Ho - 1 + ph) / st >= Hp || (Wo - 1 + pw) / st >= Wp)
    throw std::runtime_error("d2s_unpack: output window exceeds Z");
  int ngrp = (int)(((int64_t)Wo * Co + 7) / 8);
  int64_t total = (int64_t)N * Ho * ngrp;
  int64_t blocks = (total + kD2sThreads - 1) / kD2sThreads;
  if (blocks >= (1ll << 31))
    throw std::runtime_error("d2s_unpack: grid too large");
  bool vec = Co % 8 == 0 && sC == 1 && sW == Co && sH % 8 == 0 &&
             sN % 8 == 0 &&
             (((uintptr_t)z | (uintptr_t)y) % 16 == 0);
  const u16* zs = reinterpret_cast<const u16*>(z);
  u16* ys = reinterpret_cast<u16*>(y);
  if (vec)
    d2s_unpack_kernel<true><<<(unsigned)blocks, kD2sThreads, 0, stream>>>(
        zs, ys, Co, Ho, Wo, st, ph, pw, Hp, Wp, ngrp, total, sN, sC, sH, sW);
  else
    d2s_unpack_kernel<false><<<(unsigned)blocks, kD2sThreads, 0, stream>>>(
        zs, ys, Co, Ho, Wo, st, ph, pw, Hp, Wp, ngrp, total, sN, sC, sH, sW);
}

}  // namespace cosamd
