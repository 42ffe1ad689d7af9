// Fused single-token LSTM step for decode (T == 1, N <= 16 streams).
//
//   pre[g][n][j] = b[gH+j] + sum over segments  a_seg[n][:] . W_seg[gH+j][:]
//   segments: (x, W_xc [4H,D]), (cont_n * h_prev, W_hc [4H,H]),
//             (x_static, W_xsc [4H,Ds]);  gates g = i,f,o,g
//   c = cont*f*c_prev + i*g (fp32),  h = o*tanh(c) (bf16)
//
// At this M the op is pure weight streaming (LRCN: 16-24 MB of bf16 per
// layer per token), so the weights go straight from memory to registers in
// 16-byte loads and are read exactly once: one wave owns the four gate rows
// of one hidden unit, each lane takes every 64th 8-element chunk of the
// rows, and LOADS chunks per lane are in flight before the first is used.
// The small activation panel ([NB][D+H+Ds] bf16, cont already applied to
// the h segment) is staged once per block in LDS and shared by the block's
// four waves.  Pre-activations stay fp32 from the first product to the
// epilogue (the unrolled route rounds xg and gates to bf16 in between).
// No MFMA, no atomics, no grid barrier: every (n, j) is written by one wave.

#include "common.h"

#include <stdexcept>
#include <string>

namespace cosamd {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kStepWaves = 4;            // hidden units per block
constexpr int kStepThreads = kStepWaves * kWave;
constexpr int kStepLoads = 4;            // chunks in flight per lane and row
constexpr int kStepLdsMax = 128 * 1024;  // panel budget (gfx950: 160 KB/CU)

struct StepArgs {
  const u32x4* x;        // [N][D]   bf16
  const u32x4* h_prev;   // [N][H]   bf16
  const u32x4* xs;       // [N][Ds]  bf16 (Ds may be 0)
  const u32x4* w_xc;     // [4H][D]  bf16
  const u32x4* w_hc;     // [4H][H]  bf16
  const u32x4* w_xsc;    // [4H][Ds] bf16
  const unsigned short* bias;  // [4H] bf16
  const float* cont;     // [N]
  const float* c_prev;   // [N][H]
  float* c_out;          // [N][H]
  unsigned short* h_out; // [N][H] bf16
  int N, D, H, Ds;
};

__device__ __forceinline__ float bf_lo(unsigned int v) {
  return __uint_as_float(v << 16);
}
__device__ __forceinline__ float bf_hi(unsigned int v) {
  return __uint_as_float(v & 0xffff0000u);
}
__device__ __forceinline__ unsigned int f2bf_bits(float v) {
  bf16 b = __float2bfloat16(v);
  return (unsigned int)(*reinterpret_cast<unsigned short*>(&b));
}
__device__ __forceinline__ unsigned int scale_pair(unsigned int v, float s) {
  return f2bf_bits(bf_lo(v) * s) | (f2bf_bits(bf_hi(v) * s) << 16);
}

template <int NB>
__global__ __launch_bounds__(kStepThreads) void lstm_step_kernel(StepArgs p) {
  extern __shared__ u32x4 panel[];        // [NB][KC] 8-element chunks
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  const int dc = p.D >> 3, hc = p.H >> 3, sc = p.Ds >> 3;
  const int KC = dc + hc + sc;

  // ---- stage the activation panel (rows n >= N are zero)
  for (int idx = tid; idx < NB * KC; idx += kStepThreads) {
    int n = idx / KC, q = idx - n * KC;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (n < p.N) {
      if (q < dc) {
        v = p.x[(size_t)n * dc + q];
      } else if (q < dc + hc) {
        v = p.h_prev[(size_t)n * hc + (q - dc)];
        float ct = p.cont[n];
        if (ct != 1.f) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = scale_pair(v[e], ct);
        }
      } else {
        v = p.xs[(size_t)n * sc + (q - dc - hc)];
      }
    }
    panel[idx] = v;
  }
  __syncthreads();

  const int j = blockIdx.x * kStepWaves + wave;   // wave-uniform
  if (j >= p.H) return;

  float acc[4][NB];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[g][n] = 0.f;

  for (int q0 = lane; q0 < KC; q0 += kWave * kStepLoads) {
    u32x4 w[kStepLoads][4];
    // all loads of this pass are issued before the first use
#pragma unroll
    for (int u = 0; u < kStepLoads; ++u) {
      int q = q0 + u * kWave;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (q < KC) {
          size_t row = (size_t)g * p.H + j;
          const u32x4* src;
          if (q < dc) src = p.w_xc + row * dc + q;
          else if (q < dc + hc) src = p.w_hc + row * hc + (q - dc);
          else src = p.w_xsc + row * sc + (q - dc - hc);
          v = *src;
        }
        w[u][g] = v;
      }
    }
#pragma unroll
    for (int u = 0; u < kStepLoads; ++u) {
      int q = q0 + u * kWave;
      if (q < KC) {
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          u32x4 a = panel[n * KC + q];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float a0 = bf_lo(a[e]), a1 = bf_hi(a[e]);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              acc[g][n] = fmaf(a0, bf_lo(w[u][g][e]), acc[g][n]);
              acc[g][n] = fmaf(a1, bf_hi(w[u][g][e]), acc[g][n]);
            }
          }
        }
      }
    }
  }

  // ---- reduce across the wave, then lane n applies the LSTM unit
  float pre[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      float v = acc[g][n];
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1)
        v += __shfl_xor(v, off, kWave);
      if (lane == n) pre[g] = v;
    }
  }
  if (lane < p.N) {
    const int n = lane;
    const unsigned short* b = p.bias;
    float xi = pre[0] + bf_lo(b[j]);
    float xf = pre[1] + bf_lo(b[p.H + j]);
    float xo = pre[2] + bf_lo(b[2 * p.H + j]);
    float xg = pre[3] + bf_lo(b[3 * p.H + j]);
    float gi = 1.f / (1.f + __expf(-xi));
    float gf = 1.f / (1.f + __expf(-xf));
    float go = 1.f / (1.f + __expf(-xo));
    float gg = tanhf(xg);
    size_t o = (size_t)n * p.H + j;
    float c = gf * p.c_prev[o] * p.cont[n] + gi * gg;
    p.c_out[o] = c;
    p.h_out[o] = (unsigned short)f2bf_bits(go * tanhf(c));
  }
}

template <int NB>
void launch_step(const StepArgs& a, size_t lds, hipStream_t stream) {
  // above 64 KB the dynamic LDS size is opt-in per function (and device)
  if (lds > 64 * 1024)
    COS_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&lstm_step_kernel<NB>),
        hipFuncAttributeMaxDynamicSharedMemorySize, kStepLdsMax));
  int grid = ceil_div(a.H, kStepWaves);
  lstm_step_kernel<NB><<<grid, kStepThreads, lds, stream>>>(a);
  COS_CHECK_HIP(hipGetLastError());
}

int step_nb(int N) {
  int nb = 1;
  while (nb < N) nb *= 2;
  return nb;
}

}  // namespace

// LDS bytes the step kernel needs for these dims, or -1 when the shape is
// outside what it serves (N > 16, a length that is no multiple of 8, or a
// panel beyond the LDS budget).
int64_t lstm_step_lds_bytes(int N, int D, int H, int Ds) {
  if (N < 1 || N > 16 || D < 8 || H < 8 || Ds < 0) return -1;
  if ((D | H | Ds) & 7) return -1;
  int64_t bytes = (int64_t)step_nb(N) * (D + H + Ds) * 2;
  return bytes <= kStepLdsMax ? bytes : -1;
}

void lstm_step(const void* x, const void* h_prev, const void* xs,
               const void* w_xc, const void* w_hc, const void* w_xsc,
               const void* bias, const float* cont, const float* c_prev,
               float* c_out, void* h_out, int N, int D, int H, int Ds,
               hipStream_t stream) {
  int64_t lds = lstm_step_lds_bytes(N, D, H, Ds);
  if (lds < 0)
    throw std::runtime_error("lstm_step: shape outside the fused kernel");
  StepArgs a;
  a.x = static_cast<const u32x4*>(x);
  a.h_prev = static_cast<const u32x4*>(h_prev);
  a.xs = static_cast<const u32x4*>(xs);
  a.w_xc = static_cast<const u32x4*>(w_xc);
  a.w_hc = static_cast<const u32x4*>(w_hc);
  a.w_xsc = static_cast<const u32x4*>(w_xsc);
  a.bias = static_cast<const unsigned short*>(bias);
  a.cont = cont;
  a.c_prev = c_prev;
  a.c_out = c_out;
  a.h_out = static_cast<unsigned short*>(h_out);
  a.N = N; a.D = D; a.H = H; a.Ds = Ds;
  switch (step_nb(N)) {
    case 1: launch_step<1>(a, lds, stream); break;
    case 2: launch_step<2>(a, lds, stream); break;
    case 4: launch_step<4>(a, lds, stream); break;
    case 8: launch_step<8>(a, lds, stream); break;
    default: launch_step<16>(a, lds, stream); break;
  }
}

}  // namespace cosamd
