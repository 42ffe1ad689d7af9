// Exact-fp32 GEMM for gfx950 on the f32-input MFMA (v_mfma_f32_32x32x2_f32),
// plus the fp32 im2col / col2im pair the fp32 convolution lowering uses.
//
// C[M,N] = op(A) * op(B) (+ bias[n]) (ReLU), fp32 in / fp32 accumulate /
// fp32 out.  Operand convention matches gemm_bf16:
//   A is [M,K] row-major (lda), or [K,M] when trans_a;
//   B is [N,K] row-major (ldb, the Caffe weight layout), or [K,N] when
//   trans_b;  C is [M,N] (ldc).
// The MFMA result is bit-for-bit a k-ordered fmaf chain, so this path keeps
// fp32 Caffe numerics (one rounding per product, no reduced precision).
//
// Block: 256 threads = 4 waves in a 2x2 grid, 128x128 C tile, each wave a
// 64x64 quadrant as 2x2 MFMA tiles of 32x32 -> four independent 16-register
// accumulators per wave.  K advances in LDS tiles of 16.  Both operands sit
// in LDS k-major ([k][row], row stride 130 floats): an MFMA operand read is
// 32 consecutive floats per lane half (conflict-free), and the transposing
// store of a k-contiguous global tile lands on bank (2k + r) mod 32, also
// conflict-free.  The next tile's global loads are issued before the MFMAs
// of the current one (register prefetch, one LDS buffer).
//
// Every global load is a guarded 4-byte load: callers pass row sub-views, so
// only 4-byte alignment is ever proven and M/N/K are arbitrary.  Out-of-range
// elements are staged as zeros, which also covers any K tail.
//
// Split-K: gridDim.z slices the k-tiles; slices add into a zeroed C with
// fp32 atomics, slice 0 carries the bias.  ReLU cannot be combined with it.

#include "common.h"

#include <stdexcept>
#include <string>

namespace cosamd {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kBM = 128;        // block tile rows (M) and cols (N)
constexpr int kBK = 16;         // LDS tile depth
constexpr int kLd = kBM + 2;    // LDS row stride in floats (see header)
constexpr int kThreads = 256;
constexpr int kPerThread = kBM * kBK / kThreads;   // 8 floats per operand

// Global -> register stage of one [128 rows][kBK] operand tile.
// KCONTIG: element (r,k) lives at p[r*ld + k]; otherwise at p[k*ld + r].
// Either way consecutive lanes walk the contiguous axis.
template <bool KCONTIG>
__device__ __forceinline__ void tile_coords(int tid, int i, int& r, int& k) {
  if (KCONTIG) {
    k = tid & (kBK - 1);
    r = (tid >> 4) + (kThreads / kBK) * i;
  } else {
    r = tid & (kBM - 1);
    k = (tid >> 7) + (kThreads / kBM) * i;
  }
}

template <bool KCONTIG>
__device__ __forceinline__ void load_tile(const float* __restrict__ p,
                                          int64_t ld, int r0, int k0,
                                          int rows, int kend, int tid,
                                          float (&reg)[kPerThread]) {
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    int r, k;
    tile_coords<KCONTIG>(tid, i, r, k);
    int gr = r0 + r, gk = k0 + k;
    float v = 0.f;
    if (gr < rows && gk < kend)
      v = KCONTIG ? p[(int64_t)gr * ld + gk] : p[(int64_t)gk * ld + gr];
    reg[i] = v;
  }
}

template <bool KCONTIG>
__device__ __forceinline__ void store_tile(float* __restrict__ s, int tid,
                                           const float (&reg)[kPerThread]) {
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    int r, k;
    tile_coords<KCONTIG>(tid, i, r, k);
    s[k * kLd + r] = reg[i];
  }
}

// TA / TB are the caller's trans flags: A is k-contiguous when !TA, B is
// k-contiguous when !TB.  ATOMIC selects the split-K epilogue.
template <bool TA, bool TB, bool ATOMIC>
__global__ __launch_bounds__(kThreads) void gemm_f32_kernel(
    const float* __restrict__ A, const float* __restrict__ B,
    float* __restrict__ C, const float* __restrict__ bias, int M, int N,
    int K, int64_t lda, int64_t ldb, int64_t ldc, int ktiles_per_split,
    int relu) {
  __shared__ float As[kBK * kLd];
  __shared__ float Bs[kBK * kLd];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave >> 1) * 64;   // wave quadrant origin inside the tile
  const int wn = (wave & 1) * 64;
  const int m0 = blockIdx.x * kBM;
  const int n0 = blockIdx.y * kBM;

  const int kbeg = blockIdx.z * ktiles_per_split * kBK;
  if (kbeg >= K) return;             // uniform for the whole block
  int kend = kbeg + ktiles_per_split * kBK;
  if (kend > K) kend = K;
  const int nkt = (kend - kbeg + kBK - 1) / kBK;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float ra[kPerThread], rb[kPerThread];
  load_tile<!TA>(A, lda, m0, kbeg, M, kend, tid, ra);
  load_tile<!TB>(B, ldb, n0, kbeg, N, kend, tid, rb);

  const int l31 = lane & 31;
  const int kh = lane >> 5;          // which of the two k of an MFMA step

  for (int kt = 0; kt < nkt; ++kt) {
    store_tile<!TA>(As, tid, ra);
    store_tile<!TB>(Bs, tid, rb);
    __syncthreads();
    if (kt + 1 < nkt) {
      int k0 = kbeg + (kt + 1) * kBK;
      load_tile<!TA>(A, lda, m0, k0, M, kend, tid, ra);
      load_tile<!TB>(B, ldb, n0, k0, N, kend, tid, rb);
    }
#pragma unroll
    for (int kk = 0; kk < kBK; kk += 2) {
      const float* ap = As + (kk + kh) * kLd + wm + l31;
      const float* bp = Bs + (kk + kh) * kLd + wn + l31;
      float a0 = ap[0], a1 = ap[32];
      float b0 = bp[0], b1 = bp[32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // C/D map of the 32x32 MFMA: col = lane & 31,
  // row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const bool add_bias = bias != nullptr && (!ATOMIC || blockIdx.z == 0);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int col = n0 + wn + j * 32 + l31;
    if (col >= N) continue;
    float bv = add_bias ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row >= M) continue;
        float v = acc[i][j][r] + bv;
        float* dst = C + (int64_t)row * ldc + col;
        if (ATOMIC) {
          atomicAdd(dst, v);
        } else {
          if (relu) v = v > 0.f ? v : 0.f;
          *dst = v;
        }
      }
    }
  }
}

template <bool TA, bool TB>
void launch_gemm_f32(const float* A, const float* B, float* C,
                     const float* bias, int M, int N, int K, int64_t lda,
                     int64_t ldb, int64_t ldc, int splitk, bool relu,
                     hipStream_t stream) {
  int ktiles = ceil_div(K, kBK);
  int per = ceil_div(ktiles, splitk);
  splitk = ceil_div(ktiles, per);    // no empty slices
  dim3 grid(ceil_div(M, kBM), ceil_div(N, kBM), splitk);
  if (splitk > 1) {
    hipLaunchKernelGGL((gemm_f32_kernel<TA, TB, true>), grid, dim3(kThreads),
                       0, stream, A, B, C, bias, M, N, K, lda, ldb, ldc, per,
                       0);
  } else {
    hipLaunchKernelGGL((gemm_f32_kernel<TA, TB, false>), grid,
                       dim3(kThreads), 0, stream, A, B, C, bias, M, N, K, lda,
                       ldb, ldc, per, relu ? 1 : 0);
  }
  COS_CHECK_HIP(hipGetLastError());
}

// ---- fp32 conv lowering -------------------------------------------------
// col is [N*P*Q][R*S*Cg] with k order (r, s, c), channel fastest: on
// channels-last activations both kernels then read and write runs of Cg
// consecutive floats.  The weight operand is the matching [Kg][R][S][Cg]
// permutation (ops/gpu.py).  x and dx are addressed through element
// strides, so any layout works in place; NCHW is merely uncoalesced.

struct ConvGeom {
  int N, H, W, P, Q, R, S, sh, sw, ph, pw, dh, dw, c0, Cg;
  int64_t sN, sC, sH, sW;
};

// One thread owns V consecutive k of the col row (V = 4 only where the
// launcher proved 16-byte alignment of every run) and walks a contiguous
// chunk of rows: (r, s, c) is decoded once per thread and (n, p, q) advances
// by carries, so the row loop holds no division.
template <int V>
__global__ __launch_bounds__(128) void im2col_f32_kernel(
    const float* __restrict__ x, float* __restrict__ col, ConvGeom g,
    int rows, int rows_per_block) {
  const int kdim = g.Cg * g.R * g.S;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= kdim / V) return;
  const int kk = j * V;
  const int c = kk % g.Cg;
  const int s = (kk / g.Cg) % g.S;
  const int r = kk / (g.Cg * g.S);
  const int h_off = r * g.dh - g.ph, w_off = s * g.dw - g.pw;
  const int row0 = blockIdx.y * rows_per_block;
  const int row1 = row0 + rows_per_block < rows ? row0 + rows_per_block : rows;
  int q = row0 % g.Q;
  int p = (row0 / g.Q) % g.P;
  int n = row0 / (g.Q * g.P);
  const float* xc = x + (g.c0 + c) * g.sC;
  for (int row = row0; row < row1; ++row) {
    int h = p * g.sh + h_off, w = q * g.sw + w_off;
    bool in = h >= 0 && h < g.H && w >= 0 && w < g.W;
    const float* src = xc + n * g.sN + h * g.sH + w * g.sW;
    float* dst = col + (int64_t)row * kdim + kk;
    if (V == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) v = *reinterpret_cast<const float4*>(src);
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      *dst = in ? *src : 0.f;
    }
    if (++q == g.Q) {
      q = 0;
      if (++p == g.P) { p = 0; ++n; }
    }
  }
}

// gather form of col2im: one thread per dx element sums the (r,s) taps that
// reach it, so the result is deterministic and needs no zeroed target
__global__ __launch_bounds__(256) void col2im_f32_kernel(
    const float* __restrict__ dcol, float* __restrict__ dx, ConvGeom g,
    int64_t total) {
  const int kdim = g.Cg * g.R * g.S;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(idx % g.Cg);
    int w = (int)((idx / g.Cg) % g.W);
    int h = (int)((idx / ((int64_t)g.Cg * g.W)) % g.H);
    int n = (int)(idx / ((int64_t)g.Cg * g.W * g.H));
    float acc = 0.f;
    for (int r = 0; r < g.R; ++r) {
      int hp = h + g.ph - r * g.dh;
      if (hp < 0 || hp % g.sh) continue;
      int p = hp / g.sh;
      if (p >= g.P) continue;
      for (int s = 0; s < g.S; ++s) {
        int wq = w + g.pw - s * g.dw;
        if (wq < 0 || wq % g.sw) continue;
        int q = wq / g.sw;
        if (q >= g.Q) continue;
        int64_t row = ((int64_t)n * g.P + p) * g.Q + q;
        acc += dcol[row * kdim + (r * g.S + s) * g.Cg + c];
      }
    }
    dx[n * g.sN + (g.c0 + c) * g.sC + h * g.sH + w * g.sW] = acc;
  }
}

int grid_for(int64_t total) {
  int64_t blocks = (total + 255) / 256;
  return (int)hmin<int64_t>(hmax<int64_t>(blocks, 1), 256 * 32);
}

}  // namespace

void gemm_f32(const float* A, const float* B, float* C, const float* bias,
              int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
              bool trans_a, bool trans_b, int splitk, bool relu,
              hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0)
    throw std::runtime_error("gemm_f32: M, N, K must be positive");
  if (splitk < 1) splitk = 1;
  if (splitk > 1 && relu)
    throw std::runtime_error("gemm_f32: ReLU cannot be fused with split-K");
  if (trans_a) {
    if (trans_b)
      launch_gemm_f32<true, true>(A, B, C, bias, M, N, K, lda, ldb, ldc,
                                  splitk, relu, stream);
    else
      launch_gemm_f32<true, false>(A, B, C, bias, M, N, K, lda, ldb, ldc,
                                   splitk, relu, stream);
  } else {
    if (trans_b)
      launch_gemm_f32<false, true>(A, B, C, bias, M, N, K, lda, ldb, ldc,
                                   splitk, relu, stream);
    else
      launch_gemm_f32<false, false>(A, B, C, bias, M, N, K, lda, ldb, ldc,
                                    splitk, relu, stream);
  }
}

void im2col_f32(const float* x, float* col, int N, int H, int W, int P,
                int Q, int R, int S, int sh, int sw, int ph, int pw, int dh,
                int dw, int c0, int Cg, int64_t sN, int64_t sC, int64_t sH,
                int64_t sW, hipStream_t stream) {
  ConvGeom g{N, H, W, P, Q, R, S, sh, sw, ph, pw, dh, dw, c0, Cg,
             sN, sC, sH, sW};
  int64_t rows64 = (int64_t)N * P * Q;
  int kdim = Cg * R * S;
  if (rows64 <= 0 || kdim <= 0) return;
  if (rows64 >= (1ll << 31) || (int64_t)P * Q >= (1ll << 31))
    throw std::runtime_error("im2col_f32: too many output pixels");
  int rows = (int)rows64;
  // 16-byte runs: channels-last input (unit channel stride), every run of
  // four channels starting on a multiple of four floats from aligned bases
  bool vec4 = sC == 1 && Cg % 4 == 0 && c0 % 4 == 0 && sN % 4 == 0 &&
              sH % 4 == 0 && sW % 4 == 0 &&
              reinterpret_cast<uintptr_t>(x) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(col) % 16 == 0;
  int kv = vec4 ? kdim / 4 : kdim;
  int gx = ceil_div(kv, 128);
  // ~16 rows per block amortise the per-thread decode; cap the grid
  int gy = hmin<int>(hmax<int>(ceil_div(rows, 16), 1), 16384);
  int rpb = ceil_div(rows, gy);
  gy = ceil_div(rows, rpb);
  if (vec4)
    hipLaunchKernelGGL(im2col_f32_kernel<4>, dim3(gx, gy), dim3(128), 0,
                       stream, x, col, g, rows, rpb);
  else
    hipLaunchKernelGGL(im2col_f32_kernel<1>, dim3(gx, gy), dim3(128), 0,
                       stream, x, col, g, rows, rpb);
  COS_CHECK_HIP(hipGetLastError());
}

void col2im_f32(const float* dcol, float* dx, int N, int H, int W, int P,
                int Q, int R, int S, int sh, int sw, int ph, int pw, int dh,
                int dw, int c0, int Cg, int64_t sN, int64_t sC, int64_t sH,
                int64_t sW, hipStream_t stream) {
  ConvGeom g{N, H, W, P, Q, R, S, sh, sw, ph, pw, dh, dw, c0, Cg,
             sN, sC, sH, sW};
  int64_t total = (int64_t)N * Cg * H * W;
  if (total <= 0) return;
  hipLaunchKernelGGL(col2im_f32_kernel, dim3(grid_for(total)), dim3(256), 0,
                     stream, dcol, dx, g, total);
  COS_CHECK_HIP(hipGetLastError());
}

}  // namespace cosamd
