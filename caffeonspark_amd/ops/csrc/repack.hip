// Fused conv-weight repack: ONE launch refreshes every conv layer's
// GEMM-ready weight layouts per step, replacing per-layer permute-copy
// + transpose kernels (GoogLeNet: 57 convs -> ~120 tiny launches/step,
// each dominated by wave-ramp overhead).
//
// Per descriptor: src  [Kout][Cg][R][S] bf16 (the solver's bf16 shadow
//                 view of the caffe-layout master weight)
//                 dst  [>=Kout][Kpad]   (forward GEMM B operand,
//                 [k][(r*S+s)*Cg + c]; pad columns stay zero)
//                 dstT [>=Kpad][Kout]   (optional, 0 = skip: the dx
//                 GEMM's transposed operand)
//                 dstF [G][>=Cg][K2p]   (optional, 0 = skip: flipped
//                 per-group layout [g][c][(RS-1-rs)*Kg + k%Kg] for the
//                 implicit-dx GEMM; pad columns stay zero)
// Table rows: [src, dst, dstT, Kout, Cg, R, S, Kpad, dstF, K2p, G, Cgp,
// st] (Cgp = the padded row count of one dstF group slab).
//
// st >= 2 marks a space-to-depth descriptor (s2d.hip): the layer runs
// as a stride-1 R'xS' convolution over C' = st*st*Cg channels, and dst
// holds the matching column order
//   dst[k][(r'*S'+s')*C' + (dy*st+dx)*Cg + c] = src[k][c][st*r'+dy][st*s'+dx]
// with R' = ceil(R/st), S' = ceil(S/st).  Only real taps are written:
// the phantom taps (st*r'+dy >= R or st*s'+dx >= S) and the pad columns
// keep the zeros the buffer was allocated with.  dstT/dstF are not used
// on that route.  The dw GEMM's output comes back in the same column
// order and dw_unpack_s2d undoes it.

#include "common.h"

namespace cosamd {

typedef unsigned short u16;

// column of tap (c, r, s) in the space-to-depth weight layout
__device__ __forceinline__ int s2d_col(int c, int r, int s, int Cg, int S,
                                       int st) {
  int Sp = (S + st - 1) / st;
  int rp = r / st, dy = r - rp * st;
  int sp = s / st, dx = s - sp * st;
  return ((rp * Sp + sp) * st * st + dy * st + dx) * Cg + c;
}

__global__ void repack_weights_kernel(const int64_t* __restrict__ table,
                                      int ndesc) {
  const int64_t* e = table + (int64_t)blockIdx.y * 13;
  const u16* src = reinterpret_cast<const u16*>(e[0]);
  u16* dst = reinterpret_cast<u16*>(e[1]);
  u16* dstT = reinterpret_cast<u16*>(e[2]);
  int Kout = (int)e[3], Cg = (int)e[4], R = (int)e[5], S = (int)e[6];
  int Kpad = (int)e[7];
  u16* dstF = reinterpret_cast<u16*>(e[8]);
  int K2p = (int)e[9];
  int G = (int)e[10], Cgp = (int)e[11];
  int st = (int)e[12];
  int Kg = G > 0 ? Kout / G : Kout;
  int RS = R * S;
  int Kcol = RS * Cg;
  int64_t total = (int64_t)Kout * Kcol;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int k = (int)(i / Kcol);
    int col = (int)(i % Kcol);
    int rs = col / Cg, c = col % Cg;
    u16 v = src[((int64_t)k * Cg + c) * RS + rs];
    if (st >= 2) {
      dst[(int64_t)k * Kpad + s2d_col(c, rs / S, rs % S, Cg, S, st)] = v;
      continue;
    }
    dst[(int64_t)k * Kpad + col] = v;
    if (dstT != nullptr) dstT[(int64_t)col * Kout + k] = v;
    if (dstF != nullptr) {
      int g = k / Kg;
      dstF[((int64_t)g * Cgp + c) * K2p +
           (RS - 1 - rs) * Kg + (k - g * Kg)] = v;
    }
  }
}

void repack_weights(const int64_t* table, int ndesc, int64_t max_total,
                    hipStream_t stream) {
  if (ndesc <= 0) return;
  int bx = (int)hmin<int64_t>(512, (max_total + 255) / 256);
  dim3 grid(bx, ndesc);
  repack_weights_kernel<<<grid, 256, 0, stream>>>(table, ndesc);
}

// stand-alone space-to-depth weight pack for weights the solver does not
// manage (and for the first step, before the fused refresh has run);
// dst must have been allocated zeroed
__global__ void s2d_pack_weight_kernel(const u16* __restrict__ src,
                                       u16* __restrict__ dst, int Kout,
                                       int Cg, int R, int S, int st,
                                       int Kpad) {
  int RS = R * S;
  int64_t total = (int64_t)Kout * Cg * RS;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int k = (int)(i / (Cg * RS));
    int crs = (int)(i % (Cg * RS));
    int c = crs / RS, rs = crs % RS;
    dst[(int64_t)k * Kpad + s2d_col(c, rs / S, rs % S, Cg, S, st)] = src[i];
  }
}

void s2d_pack_weight(const void* src, void* dst, int Kout, int Cg, int R,
                     int S, int st, int Kpad, hipStream_t stream) {
  int64_t total = (int64_t)Kout * R * S * Cg;
  if (total <= 0) return;
  int blocks = (int)hmin<int64_t>(2048, (total + 255) / 256);
  s2d_pack_weight_kernel<<<blocks, 256, 0, stream>>>(
      reinterpret_cast<const u16*>(src), reinterpret_cast<u16*>(dst), Kout,
      Cg, R, S, st, Kpad);
}

// space-to-depth dw unpack: dwp[Kout][Kpad] in the s2d column order ->
// caffe layout [Kout][Cg][R][S] (overwrite or +=); the phantom-tap and
// pad columns are dropped
__global__ void dw_unpack_s2d_kernel(const float* __restrict__ dwp,
                                     float* __restrict__ arena, int Kout,
                                     int Cg, int R, int S, int st,
                                     int Kpad, int accumulate) {
  int RS = R * S;
  int64_t total = (int64_t)Kout * Cg * RS;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int k = (int)(i / (Cg * RS));
    int crs = (int)(i % (Cg * RS));
    int c = crs / RS, rs = crs % RS;
    float v = dwp[(int64_t)k * Kpad + s2d_col(c, rs / S, rs % S, Cg, S, st)];
    if (accumulate)
      arena[i] += v;
    else
      arena[i] = v;
  }
}

void dw_unpack_s2d(const float* dwp, float* arena, int Kout, int Cg, int R,
                   int S, int st, int Kpad, bool accumulate,
                   hipStream_t stream) {
  int64_t total = (int64_t)Kout * R * S * Cg;
  if (total <= 0) return;
  int blocks = (int)hmin<int64_t>(2048, (total + 255) / 256);
  dw_unpack_s2d_kernel<<<blocks, 256, 0, stream>>>(
      dwp, arena, Kout, Cg, R, S, st, Kpad, accumulate ? 1 : 0);
}

// conv weight-gradient unpack + arena accumulate: the dw GEMM produces
// dwp[Kout][Kpad] in the GEMM's [k][(r*S+s)*Cg + c] layout; this writes
// it into the caffe-layout fp32 arena slice [Kout][Cg][R][S] in one
// pass (overwrite or +=), replacing a permute-contiguous copy plus the
// arena accumulate.
__global__ void dw_unpack_acc_kernel(const float* __restrict__ dwp,
                                     float* __restrict__ arena,
                                     int Kout, int Cg, int R, int S,
                                     int Kpad, int accumulate) {
  int RS = R * S;
  int Kcol = RS * Cg;
  int64_t total = (int64_t)Kout * Kcol;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int k = (int)(i / Kcol);
    int crs = (int)(i % Kcol);   // arena-order within one filter
    int c = crs / RS, rs = crs % RS;
    float v = dwp[(int64_t)k * Kpad + rs * Cg + c];
    if (accumulate)
      arena[i] += v;
    else
      arena[i] = v;
  }
}

void dw_unpack_acc(const float* dwp, float* arena, int Kout, int Cg,
                   int R, int S, int Kpad, bool accumulate,
                   hipStream_t stream) {
  int64_t total = (int64_t)Kout * R * S * Cg;
  int blocks = (int)hmin<int64_t>(2048, (total + 255) / 256);
  dw_unpack_acc_kernel<<<blocks, 256, 0, stream>>>(
      dwp, arena, Kout, Cg, R, S, Kpad, accumulate ? 1 : 0);
}

}  // namespace cosamd
