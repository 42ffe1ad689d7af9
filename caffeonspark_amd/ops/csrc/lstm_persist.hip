// Persistent whole-sequence LSTM for gfx950, v2: hidden-slice-owned.
//
// ONE kernel runs all T timesteps.  Each block owns a 16-wide slice of
// the hidden dimension and computes, for its slice, ALL FOUR gate
// columns over the FULL K (the four 16-row weight strips i/f/o/g stay
// stationary in VGPR MFMA fragments, ~128 VGPRs/lane), so
//   * gate sums never cross blocks: no fp32 atomics, no gate buffer --
//     cross-wave K-partials reduce through LDS inside the block;
//   * the LSTM unit math for the slice (lstm_cell.h, shared with the
//     other routes) is block-local, and the cell state c (forward) / dc
//     and dh (backward) live in LDS across the whole sequence;
//   * exactly ONE grid barrier per timestep (between writing h_in_{t+1}
//     / dxg_t and the other blocks' reads of them) -- v1's
//     4H-column-partitioned design needed two plus 16 MB/t of atomics.
// The barrier is store-slot arrival polled by block 0's threads, with a
// watchdog that sets an error flag and NaN-poisons the output instead
// of hanging if blocks are not co-resident (the Python glue checks the
// flag asynchronously and gates this path to single-process runs).
//
// Reference scope: recurrent LSTM path of lrcn_cos.prototxt (SURVEY.md
// §5 long-context: time-major, cont gating).

#include "common.h"
#include "lstm_cell.h"

namespace cosamd {

typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

namespace {

// Grid barrier with store-slot arrival (each block plain-stores its
// running barrier index into its own slot; block 0's threads poll all
// slots in parallel and release the generation word).  Flat same-address
// atomic arrival measured ~25 us at 252 blocks; this lands ~2-4 us.
// bar layout (unsigned words): [0..255] slots, [256] gen, [258] err.
__device__ __forceinline__ bool grid_sync(unsigned* bar, unsigned nblk,
                                          int* err, unsigned my_count) {
  unsigned* arr = bar;
  unsigned* gen = bar + 256;
  __syncthreads();
  if (blockIdx.x == 0) {
    unsigned slot = threadIdx.x;
    if (slot == 0) {
      __threadfence();
      __hip_atomic_store(arr, my_count, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    long spins = 0;
    for (;;) {
      unsigned v = (slot < nblk)
          ? __hip_atomic_load(arr + slot, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT)
          : my_count;
      int ok = __syncthreads_count((int)(v >= my_count));
      if (ok == (int)blockDim.x) break;
      if (++spins > (1L << 22)) {
        if (slot == 0)
          __hip_atomic_store(err, 1, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
      if (spins > 2048) __builtin_amdgcn_s_sleep(2);
    }
    if (slot == 0) {
      __hip_atomic_load(arr, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(gen, my_count, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  } else {
    if (threadIdx.x == 0) {
      __threadfence();
      __hip_atomic_store(arr + blockIdx.x, my_count, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_AGENT);
      long spins = 0;
      while (__hip_atomic_load(gen, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT) < my_count) {
        if (spins > 2048) __builtin_amdgcn_s_sleep(4);
        if (++spins > (1L << 24)) {
          __hip_atomic_store(err, 1, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_SYSTEM);
          break;
        }
        if (__hip_atomic_load(err, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT))
          break;
      }
      __hip_atomic_load(gen, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  }
  return __hip_atomic_load(err, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT) == 0;
}

// One k-step's A fragments for the 64-row tile: a[mf] = 8 elements at
// column k of row mf*16 + lrow of A (row pitch ld), zero past column kmax.
__device__ __forceinline__ void load_a(bf16x8v (&a)[4], const u16* A, int ld,
                                       int kmax, int k, int lrow) {
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
    int m = mf * 16 + lrow;
    if (k + 8 <= kmax) {
      a[mf] = *reinterpret_cast<const bf16x8v*>(A + (int64_t)m * ld + k);
    } else {
      bf16 z = f2bf(0.f);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[mf][j] = z;
    }
  }
}

// Sum the four waves' k-partials (NV floats per lane, held as NV/4 MFMA
// accumulators) into wave 0's registers, pairwise through LDS: waves 1
// and 3 hand theirs to 0 and 2 (red0, red1), then 2 hands its sum to 0
// (red0).  Three barriers; the caller scatters wave 0's acc and barriers.
template <int NV>
__device__ __forceinline__ void wave_reduce(f32x4v (&acc)[NV / 4],
                                            f32x4v* red0, f32x4v* red1,
                                            int wave, int lane) {
  constexpr int NQ = NV / 4;
  f32x4v* to0 = red0 + lane * NQ;
  f32x4v* mine = (wave >> 1) ? red1 + lane * NQ : to0;
  if (wave & 1) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) mine[q] = acc[q];
  }
  __syncthreads();
  if (!(wave & 1)) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] += mine[q];
  }
  __syncthreads();
  if (wave == 2) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) to0[q] = acc[q];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] += to0[q];
  }
}

}  // namespace

// ------------------------------------------------------------- forward
// grid = ceil(H/16) blocks, 256 threads (4 waves k-partitioned).
// Per wave: 4 weight strips (i/f/o/g rows of its k-window) stationary;
// per t: full-K gate MFMA -> cross-wave LDS reduce -> block-local unit.
__global__ __launch_bounds__(256, 1) void lstm_persist_fwd_kernel(
    const u16* __restrict__ xg, const u16* __restrict__ w_hc,
    const u16* __restrict__ cont, u16* __restrict__ h,
    float* __restrict__ c, float* __restrict__ act,
    u16* __restrict__ h_in, int T, int N, int H,
    unsigned* bar, int* err) {
  __shared__ f32x4v red0[64 * 16], red1[64 * 16];  // wave partials
  __shared__ float gates[64 * 64];                // [n][strip*16 + jj]
  __shared__ float c_lds[64 * 16];                // cell state, persists
  int H4 = 4 * H;
  int nblk = gridDim.x;
  int j0 = blockIdx.x * 16;
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int lrow = lane & 15, lk8 = (lane >> 4) * 8;
  int Hp4 = ((H + 127) & ~127) >> 2;      // per-wave K window (mult 32)
  int ksteps = Hp4 >> 5;
  int kw0 = wave * Hp4;

  // stationary weights: strip s covers gate-rows s*H + [j0, j0+16)
  bf16x8v wf[4][8];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    for (int ks = 0; ks < 8; ++ks) {
      int row = s * H + j0 + lrow;
      int k = kw0 + ks * 32 + lk8;
      if (ks < ksteps && (j0 + lrow) < H && k + 8 <= H) {
        wf[s][ks] = *reinterpret_cast<const bf16x8v*>(
            w_hc + (int64_t)row * H + k);
      } else {
        bf16 z = f2bf(0.f);
#pragma unroll
        for (int j = 0; j < 8; ++j) wf[s][ks][j] = z;
      }
    }
  }
  for (int i = threadIdx.x; i < 64 * 16; i += blockDim.x)
    c_lds[i] = 0.f;
  __syncthreads();

  int64_t nh = (int64_t)N * H;
  unsigned sync_idx = 0;
  for (int t = 0; t < T; ++t) {
    // ---- gate GEMM over the full K for this block's 64 gate columns
    const u16* A = h_in + (int64_t)t * nh;
    f32x4v acc[16] = {};      // [mf * 4 + strip]
    // software-pipelined a-loads: fetch ks+1 while ks's MFMAs run (the
    // 4-MFMA bursts are too short to hide the L2 load chain otherwise)
    bf16x8v a_cur[4], a_nxt[4];
    load_a(a_cur, A, H, H, kw0 + lk8, lrow);
    for (int ks = 0; ks < ksteps; ++ks) {
      if (ks + 1 < ksteps)
        load_a(a_nxt, A, H, H, kw0 + (ks + 1) * 32 + lk8, lrow);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[mf * 4 + s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_cur[mf], wf[s][ks < 8 ? ks : 0], acc[mf * 4 + s], 0, 0, 0);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf) a_cur[mf] = a_nxt[mf];
    }
    // ---- cross-wave reduce, wave 0 scatters the sums into gates[]
    wave_reduce<64>(acc, red0, red1, wave, lane);
    if (wave == 0) {
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = (lane >> 4) * 4 + mf * 16 + r;
            gates[row * 64 + s * 16 + lrow] = acc[mf * 4 + s][r];
          }
    }
    __syncthreads();

    // ---- block-local fused unit over (n < N) x (16 slice cols)
    const u16* cont_t = cont + (int64_t)t * N;
    const u16* xg_t = xg + (int64_t)t * N * H4;
    float* c_t = c + (int64_t)t * nh;
    u16* h_t = h + (int64_t)t * nh;
    float* act_t = act + (int64_t)t * N * H4;
    u16* h_in_next = (t + 1 < T) ? h_in + (int64_t)(t + 1) * nh : nullptr;
    const u16* cont_next = (t + 1 < T) ? cont + (int64_t)(t + 1) * N
                                       : nullptr;
    for (int i = threadIdx.x; i < N * 16; i += blockDim.x) {
      int n = i >> 4;
      int jj = i & 15;
      int jg = j0 + jj;
      if (jg >= H) continue;
      int64_t g0 = (int64_t)n * H4 + jg;
      const float* hg = gates + n * 64 + jj;
      LstmCellFwd r = lstm_cell_fwd(
          ldbf(xg_t + g0) + hg[0], ldbf(xg_t + g0 + H) + hg[16],
          ldbf(xg_t + g0 + 2 * H) + hg[32],
          ldbf(xg_t + g0 + 3 * H) + hg[48], c_lds[i], ldbf(cont_t + n));
      c_lds[i] = r.c;
      int64_t hi = (int64_t)n * H + jg;
      c_t[hi] = r.c;
      stbf(h_t + hi, r.h);
      float* ap = act_t + g0;
      ap[0] = r.gi; ap[H] = r.gf; ap[2 * H] = r.go; ap[3 * H] = r.gg;
      if (h_in_next != nullptr)
        stbf(h_in_next + hi, r.h * ldbf(cont_next + n));
    }
    if (!grid_sync(bar, nblk, err, ++sync_idx)) {
      if (threadIdx.x == 0) h[(int64_t)t * nh] = 0x7FC0;  // bf16 NaN
      return;
    }
  }
}

// ------------------------------------------------------------ backward
// grid = ceil(H/16); block owns dh slice [j0, j0+16): unit math (dgates)
// is slice-local (dh/dc persist in LDS), then ONE barrier publishes
// dxg_t before every block's dh GEMM over the full 4H.
__global__ __launch_bounds__(256, 1) void lstm_persist_bwd_kernel(
    const u16* __restrict__ dy, const u16* __restrict__ w_hcT,
    const u16* __restrict__ cont, const u16* __restrict__ h,
    const float* __restrict__ c, const float* __restrict__ act,
    u16* __restrict__ dxg, int T, int N, int H,
    unsigned* bar, int* err) {
  __shared__ f32x4v red0[64 * 4], red1[64 * 4];
  __shared__ float dh_lds[64 * 16];
  __shared__ float dc_lds[64 * 16];
  int H4 = 4 * H;
  int nblk = gridDim.x;
  int j0 = blockIdx.x * 16;
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int lrow = lane & 15, lk8 = (lane >> 4) * 8;
  int Hp4 = ((H4 + 127) & ~127) >> 2;     // per-wave K window over 4H
  int ksteps = Hp4 >> 5;
  int kw0 = wave * Hp4;

  // stationary weights: w_hcT[H][4H], rows = this block's dh columns
  // (16 rows), k over 4H -- up to 32 k-steps/wave (128 VGPRs)
  bf16x8v wf[32];
  for (int ks = 0; ks < 32; ++ks) {
    int row = j0 + lrow;
    int k = kw0 + ks * 32 + lk8;
    if (ks < ksteps && row < H && k + 8 <= H4) {
      wf[ks] = *reinterpret_cast<const bf16x8v*>(
          w_hcT + (int64_t)row * H4 + k);
    } else {
      bf16 z = f2bf(0.f);
#pragma unroll
      for (int j = 0; j < 8; ++j) wf[ks][j] = z;
    }
  }
  for (int i = threadIdx.x; i < 64 * 16; i += blockDim.x) {
    dh_lds[i] = 0.f;
    dc_lds[i] = 0.f;
  }
  __syncthreads();

  int64_t nh = (int64_t)N * H;
  unsigned sync_idx = 0;
  for (int t = T - 1; t >= 0; --t) {
    // ---- slice-local unit: dgates_t from dy_t + dh_lds/dc_lds
    const u16* cont_t = cont + (int64_t)t * N;
    const u16* cont_t1 = (t + 1 < T) ? cont + (int64_t)(t + 1) * N
                                     : nullptr;
    const float* c_t = c + (int64_t)t * nh;
    const float* c_prev = (t > 0) ? c + (int64_t)(t - 1) * nh : nullptr;
    const float* act_t = act + (int64_t)t * N * H4;
    const u16* dy_t = dy + (int64_t)t * nh;
    u16* dxg_t = dxg + (int64_t)t * N * H4;
    for (int i = threadIdx.x; i < N * 16; i += blockDim.x) {
      int n = i >> 4;
      int jj = i & 15;
      int jg = j0 + jj;
      if (jg >= H) continue;
      int64_t g0 = (int64_t)n * H4 + jg;
      int64_t hi = (int64_t)n * H + jg;
      const float* a = act_t + g0;
      float dhrec = (t + 1 < T) ? dh_lds[i] * ldbf(cont_t1 + n) : 0.f;
      float dhv = ldbf(dy_t + hi) + dhrec;
      float cp = (c_prev != nullptr) ? c_prev[hi] : 0.f;
      LstmCellBwd r = lstm_cell_bwd(
          a[0], a[H], a[2 * H], a[3 * H], c_t[hi], cp, ldbf(cont_t + n),
          dhv, dc_lds[i]);
      dc_lds[i] = r.dc_prev;       // dc for t-1 (slice-local)
      u16* dg = dxg_t + g0;
      stbf(dg, r.di);
      stbf(dg + H, r.df);
      stbf(dg + 2 * H, r.dO);
      stbf(dg + 3 * H, r.dg);
    }
    if (!grid_sync(bar, nblk, err, ++sync_idx)) {
      if (threadIdx.x == 0) dxg[(int64_t)t * N * H4] = 0x7FC0;
      return;
    }

    // ---- dh GEMM for t-1: dh_slice = dxg_t @ w_hcT^T (full 4H K)
    if (t > 0) {
      f32x4v acc[4] = {};     // [mf] x 16 cols
      bf16x8v a_cur[4], a_nxt[4];
      load_a(a_cur, dxg_t, H4, H4, kw0 + lk8, lrow);
      for (int ks = 0; ks < ksteps; ++ks) {
        if (ks + 1 < ksteps)
          load_a(a_nxt, dxg_t, H4, H4, kw0 + (ks + 1) * 32 + lk8, lrow);
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
          acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_cur[mf], wf[ks < 32 ? ks : 0], acc[mf], 0, 0, 0);
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) a_cur[mf] = a_nxt[mf];
      }
      // cross-wave reduce, wave 0 scatters the sums into dh_lds
      wave_reduce<16>(acc, red0, red1, wave, lane);
      if (wave == 0) {
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = (lane >> 4) * 4 + mf * 16 + r;
            dh_lds[row * 16 + lrow] = acc[mf][r];
          }
      }
      __syncthreads();
    }
  }
}

// --------------------------------------------------------------- hosts
// returns 0 ok, 1 = not applicable (shape); watchdog aborts are read
// asynchronously from bar[258] by the Python glue.

int lstm_persist_fwd(const void* xg, const void* w_hc, const void* cont,
                     void* h, float* c, float* act, void* h_in,
                     int T, int N, int H, void* bar, hipStream_t stream) {
  if (N > 64 || H % 8 != 0 || H > 1024) return 1;  // wf[4][8] k-window
  int nblk = (H + 15) / 16;
  if (nblk < 2 || nblk > 256) return 1;
  int64_t nh = (int64_t)N * H;
  COS_CHECK_HIP(hipMemsetAsync(h_in, 0, nh * 2, stream));
  unsigned* cnt = reinterpret_cast<unsigned*>(bar);
  lstm_persist_fwd_kernel<<<nblk, 256, 0, stream>>>(
      (const u16*)xg, (const u16*)w_hc, (const u16*)cont, (u16*)h, c, act,
      (u16*)h_in, T, N, H, cnt, (int*)(cnt + 258));
  return 0;
}

int lstm_persist_bwd(const void* dy, const void* w_hcT, const void* cont,
                     const void* h, const float* c, const float* act,
                     void* dxg, int T, int N, int H, void* bar,
                     hipStream_t stream) {
  if (N > 64 || H % 8 != 0 || H > 1024) return 1;  // wf[32] k-window
  int nblk = (H + 15) / 16;
  if (nblk < 2 || nblk > 256) return 1;
  unsigned* cnt = reinterpret_cast<unsigned*>(bar);
  lstm_persist_bwd_kernel<<<nblk, 256, 0, stream>>>(
      (const u16*)dy, (const u16*)w_hcT, (const u16*)cont, (const u16*)h,
      c, act, (u16*)dxg, T, N, H, cnt, (int*)(cnt + 258));
  return 0;
}

}  // namespace cosamd
