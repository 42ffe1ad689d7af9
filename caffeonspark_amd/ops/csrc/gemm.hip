// bf16 MFMA GEMM for gfx950 (CDNA4) — the compute core of conv (im2col) and
// inner-product layers, forward and backward.
//
// C[M,N] = A' @ B' with A',B' presented as [rows][K] panels:
//   TRANS_A=false: A global layout [M][K] (lda = row stride)
//   TRANS_A=true : A global layout [K][M] (lda = row stride of the K-major
//                  matrix) — staged transposed into LDS
// (same for B with N rows).  All four combinations are used by the layer
// catalog (fc fwd = NT-direct/direct, fc dx = direct/trans, dw = trans/trans).
//
// Every kernel works on BK=32 K-tiles held in LDS in ONE canonical layout
// ([row][32] bf16, 16-byte chunks XOR-swizzled by swz_chunk) and is
// assembled from the same pieces:
//   decode_tile      blockIdx -> XCD-swizzled (bm, bn, tile_m, tile_n)
//   stage_*          global -> LDS; the only part that differs per operand
//   load_frags_mfma  LDS -> fragments -> 16x16x32 bf16 MFMA (fp32 acc)
//   TileCfg          block tile x wave grid -> per-wave fragment and DMA counts
//   pipelined_loop   counted-vmcnt K loop for the DMA-staged kernels
//                    (gemm_conv_dw_tr_kernel has its own [k][col] image,
//                    transposed fragment reads and ring; see there)
//   epilogue_bf16    bias + ReLU + alpha, bf16 store or RMW accumulate
//   epilogue_bf16_vec  the same through LDS with 16-byte accesses (conv)
//   epilogue_f32     fp32 plain store or atomic add (split-K)
//   epilogue_f32_vec   the plain store through LDS with 16-byte accesses
//
// Kernels, their staging policies, and who launches them:
//   gemm_kernel<TA, TB, STORE_MODE, WAVES>       gemm_bf16[_batched]
//     128x128 tile; interior aligned NN tiles run pipelined_loop at depth 2
//     with ADirect (direct-to-LDS DMA), everything else a guarded loop.
//     All 16 TAxTBxSTORE_MODE combinations at WAVES=4, NN also at WAVES=8.
//   gemm_conv_fwd_kernel<TileCfg, DEPTH>         gemm_conv_fwd
//     pipelined_loop with AImplicit (im2col gather DMA) on a block tile
//     chosen per launch by conv_fwd_plan (COS_CONV_CFGS lists every
//     instantiation).  N tile: the one of 48/64/96/128 columns with the
//     least padding, the wider on a tie; COS_CONV_BN=48/64/96/128 forces
//     one (0/unset: automatic); unlike COS_CONVQ it is read on every
//     call, because the tests flip it under conv2d_forward/backward, which
//     take no tile argument.  128 columns keep the fixed-tile rule:
//     8 waves, depth 4 (one barrier per tile) when w8 and 4*BK <= K <=
//     COS_CONVQ, else 8 waves depth 2 when w8, else 4 waves.  Narrower
//     tiles take rows, waves and depth from the sweep in
//     profiles/alexnet_1gpu_conv_tiles.md (256-row blocks for 48 and 64
//     columns at large M).  All widths give bit-identical results.
//     A grouped convolution is one launch: blockIdx.y is the group, and
//     three strides move the input channel window, the B rows and the C
//     columns per group (bias advances by N).
//     Epilogue: epilogue_bf16_vec (accumulators transposed through the
//     freed LDS, 16-byte stores / read-add-write, float4 bias) when N, ldc
//     and the group's column offset are multiples of 8 and C and bias are
//     16-byte aligned; the element-wise epilogue_bf16 otherwise.  Both
//     store the same bits.
//   gemm_conv_fwd_sc_kernel<WAVES>               gemm_conv_fwd_sc
//     small-C gather through registers, own __syncthreads loop; <8>/<4>.
//   gemm_wide_tt_kernel<STORE, BStage>           launch_wide_tt
//     128x256 tile, 8 waves, trans/trans weight gradients with optional
//     fused db.  BStage = BGuarded (TT branch of gemm_bf16_batched),
//     BImplicit (gemm_conv_dw's fallback), BImplicitSC (gemm_conv_dw_sc);
//     each with STORE 1 (single split, plain store) or 2 (split-K
//     atomics).  Both operands staged through registers (u32 k-pair
//     ds_write scatter), one LDS buffer, two barriers per tile.
//   gemm_conv_dw_tr_kernel<STORE, DEPTH>         gemm_conv_dw
//     same tile, contract and epilogue as gemm_wide_tt_kernel<., BImplicit>
//     without db; both operands DMA-staged in their K-major layout into a
//     DEPTH-stage ring (counted vmcnt, one barrier per tile), fragments by
//     ds_read_b64_tr_b16.  Taken when db == nullptr and every 16-byte
//     source chunk is aligned and whole (M, lda, C, c0, Cg, Kcol % 8 == 0,
//     A and X 16-byte aligned); COS_DW_TR=0 forces the fallback.
//   gemm_fc_kernel<TBM, TRB, DEPTH>              gemm_fc
//     InnerProduct forward (TRB false) and data gradient (TRB true) for
//     M <= 256: a 256x128 (M <= 128: 128x128) tile that covers all of M,
//     8 waves, both operands DMA-staged into a depth-4 ring with
//     gemm_conv_dw_tr_kernel's loop, W read as it lies (transposing LDS
//     reads for dx), zero-page edges, split-K into fp32 slabs
//     (epilogue_f32_vec) that fc_slab_finalize sums.  fc_gemm_plan picks
//     route and split; COS_FC_STREAM=0 keeps gemm_kernel.  See its section.
// w8 (use_w8): 8-wave blocks when M or N <= 256, forced by COS_GEMM_W8.
//
// Replaces the reference's cuBLAS calls inside conv/ip layers (SURVEY.md
// §3.6 rows "Convolution fwd/bwd", "InnerProduct") with a hand-written
// CDNA4 kernel per the rebuild's north star.

#include "common.h"

#include <type_traits>

namespace cosamd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short short8v __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int NTHREADS = 256;

// LDS chunk swizzle: a row's four 16-byte k-chunks are stored rotated by
// XOR with ((row>>1)&3).  Without it, a fragment ds_read_b128's lane
// groups (16 lanes = 16 rows, same k-chunk) land on only 2 of the 8
// bank-quads (addr = row*64B + chunk*16B, 16*row mod 32 banks ∈ {0,16}),
// an 8-way conflict; the swizzle spreads them across all 8 quads (2-way,
// which CDNA4 serves conflict-free).  LDS stays linear so the
// global_load_lds fast path just pre-swizzles the per-lane SOURCE address
// (cdna_hip_programming.md §5: swizzle must be both-sides-or-neither).
__device__ __forceinline__ int swz_chunk(int row, int chunk) {
  return chunk ^ ((row >> 1) & 3);
}

// ---------------------------------------------------------- shared pieces

struct Tile { int bm, bn, tile_m, tile_n; };

// XCD-aware block swizzle -> output tile of a TBM x TBN tiling
template <int TBN, int TBM = BM>
__device__ __forceinline__ Tile decode_tile(int M, int N) {
  int mblocks = (M + TBM - 1) / TBM;
  int nblocks = (N + TBN - 1) / TBN;
  int bid = xcd_swizzle(blockIdx.x, mblocks * nblocks);
  Tile t;
  t.bm = bid / nblocks;
  t.bn = bid % nblocks;
  t.tile_m = t.bm * TBM;
  t.tile_n = t.bn * TBN;
  return t;
}

// rows / 16-row m-fragments per wave of the 128x128 kernels:
// WAVES=4: 2x2 wave grid of 64x64; WAVES=8: 4x2 grid of 32x64
constexpr int mrows_of(int waves) { return BM / (waves / 2); }
constexpr int mfrags_of(int waves) { return mrows_of(waves) / 16; }

// Block tile TBM x TBN x BK on a WM x WN wave grid: each wave owns
// MROWS x NCOLS outputs as MF x NF 16x16 fragments.  An operand tile is
// staged in 1 KB chunks (16 rows of BK), one DMA wave-instruction each;
// every wave issues the same A_CPW + B_CPW of them per tile so that the
// pipelined loop's counted wait is one literal.  Where the B tile's
// chunks (3 for 48 rows, 6 for 96) do not divide over the waves, the LDS
// image is rounded up to B_CPW * WAVES chunks and the surplus instructions
// fetch the zero page into the unread tail.
template <int TBM_, int TBN_, int WM_, int WN_>
struct TileCfg {
  static constexpr int TBM = TBM_, TBN = TBN_, WM = WM_, WN = WN_;
  static constexpr int WAVES = WM * WN;
  static constexpr int MROWS = TBM / WM, NCOLS = TBN / WN;
  static constexpr int MF = MROWS / 16, NF = NCOLS / 16;
  static constexpr int A_CHUNKS = TBM / 16, B_CHUNKS = TBN / 16;
  static constexpr int A_CPW = A_CHUNKS / WAVES;
  static constexpr int B_CPW = (B_CHUNKS + WAVES - 1) / WAVES;
  static constexpr int A_ELEMS = TBM * BK;
  static constexpr int B_ELEMS = B_CPW * WAVES * 512;
  static_assert(MROWS % 16 == 0 && NCOLS % 16 == 0, "whole fragments");
  static_assert(A_CHUNKS % WAVES == 0, "A chunks divide over the waves");
};
// the 128x128 tile of gemm_kernel and the fixed-tile conv kernels
template <int WAVES>
using Tile128 = TileCfg<BM, BN, WAVES / 2, 2>;

// One K-tile of compute for a wave: MF + NF fragments (wave tile
// MROWS x NCOLS at (wm, wn)) from the canonical swizzled LDS layout, then
// the MF x NF MFMA block.  PRIO brackets the MFMAs with s_setprio for the
// pipelined loops, where other waves are issuing DMA at the same time.
template <int MF, int MROWS, bool PRIO, int NF = 4, int NCOLS = 64>
__device__ __forceinline__ void load_frags_mfma(
    const bf16* As, const bf16* Bs, int wm, int wn, int lane,
    f32x4 (&acc)[MF][NF]) {
  int lrow = lane & 15, lchunk = lane >> 4;
  bf16x8 afrag[MF], bfrag[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    int rb = wn * NCOLS + f * 16 + lrow;
    bfrag[f] = *reinterpret_cast<const bf16x8*>(
        Bs + rb * BK + (swz_chunk(rb, lchunk) << 3));
  }
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    int ra = wm * MROWS + f * 16 + lrow;
    afrag[f] = *reinterpret_cast<const bf16x8*>(
        As + ra * BK + (swz_chunk(ra, lchunk) << 3));
  }
  if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int fm = 0; fm < MF; ++fm)
#pragma unroll
    for (int fn = 0; fn < NF; ++fn)
      acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          afrag[fm], bfrag[fn], acc[fm][fn], 0, 0, 0);
  if (PRIO) __builtin_amdgcn_s_setprio(0);
}

// bf16 epilogue: v = acc * alpha + bias[col], optional ReLU, then either
// a plain store or (accum) a read-modify-write add — the dx fan-in:
// exclusive tiles and a single split make the plain RMW race-free.
// Accum is bool for a runtime choice, or std::true_type/false_type so
// the unused branch never reaches the optimizer.
template <int MF, int MROWS, int NF = 4, int NCOLS = 64, class Accum>
__device__ __forceinline__ void epilogue_bf16(
    const f32x4 (&acc)[MF][NF], bf16* C, const float* bias, int M, int N,
    int ldc, int tile_m, int tile_n, int wm, int wn, int lane, int relu,
    float alpha, Accum accum) {
  int crow0 = tile_m + wm * MROWS + ((lane >> 4) << 2);
  int ccol0 = tile_n + wn * NCOLS + (lane & 15);
#pragma unroll
  for (int fm = 0; fm < MF; ++fm) {
#pragma unroll
    for (int fn = 0; fn < NF; ++fn) {
      int col = ccol0 + fn * 16;
      if (col >= N) continue;
      float badd = (bias != nullptr) ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = crow0 + fm * 16 + r;
        if (row >= M) continue;
        float v = acc[fm][fn][r] * alpha + badd;
        if (relu && v < 0.f) v = 0.f;
        int64_t off = (int64_t)row * ldc + col;
        if (accum) v += bf2f(C[off]);
        C[off] = f2bf(v);
      }
    }
  }
}

// 16-byte form of epilogue_bf16 for the conv kernel (alpha = 1): each wave
// transposes its accumulators, one 16-row fragment band at a time, through
// a private LDS slab so that a lane holds 8 consecutive channels of one
// output row; bias comes as two float4, the store (and the accumulating
// read-add-write) is one 16-byte access.  Same floats, same order of bias,
// ReLU, accumulate and rounding as the element-wise form.  The caller
// guarantees N, ldc and the column offset are multiples of 8 and C and
// bias 16-byte aligned, and that nothing else uses `lds` any more.
// The slab's row stride of NCOLS + 4 floats puts the four row groups a
// wave-instruction writes (rows r, r+4, r+8, r+12) on alternating halves
// of the 32 banks: 2-way, the minimum for 256 bytes.
template <class Cfg>
constexpr int vec_slab_floats() { return Cfg::WAVES * 16 * (Cfg::NCOLS + 4); }

template <class Cfg>
__device__ __forceinline__ void epilogue_bf16_vec(
    const f32x4 (&acc)[Cfg::MF][Cfg::NF], float* lds, bf16* C,
    const float* bias, int M, int N, int ldc, int tile_m, int tile_n, int wm,
    int wn, int wave, int lane, int relu, int accum) {
  constexpr int LD = Cfg::NCOLS + 4;
  constexpr int GPR = Cfg::NCOLS / 8;        // 8-column groups per row
  constexpr int TASKS = 16 * GPR;            // (row, group) pairs per band
  float* slab = lds + wave * 16 * LD;
  int wr = (lane >> 4) << 2, wc = lane & 15;
#pragma unroll
  for (int fm = 0; fm < Cfg::MF; ++fm) {
#pragma unroll
    for (int fn = 0; fn < Cfg::NF; ++fn)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[(wr + r) * LD + fn * 16 + wc] = acc[fm][fn][r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t0 = 0; t0 < TASKS; t0 += 64) {
      int t = t0 + lane;
      int row = t / GPR, cg = t - row * GPR;
      int grow = tile_m + wm * Cfg::MROWS + fm * 16 + row;
      int col = tile_n + wn * Cfg::NCOLS + cg * 8;
      if ((TASKS % 64 == 0 || t < TASKS) && grow < M && col < N) {
        f32x4 lo = *reinterpret_cast<const f32x4*>(slab + row * LD + cg * 8);
        f32x4 hi =
            *reinterpret_cast<const f32x4*>(slab + row * LD + cg * 8 + 4);
        float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        if (bias != nullptr) {
          f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + col);
          f32x4 b1 = *reinterpret_cast<const f32x4*>(bias + col + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { v[j] += b0[j]; v[4 + j] += b1[j]; }
        }
        if (relu) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = v[j] < 0.f ? 0.f : v[j];
        }
        short8v* dst =
            reinterpret_cast<short8v*>(C + (int64_t)grow * ldc + col);
        bf16 o[8];
        if (accum) {
          short8v old = *dst;
          __builtin_memcpy(o, &old, 16);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += bf2f(o[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(v[j]);
        short8v out;
        __builtin_memcpy(&out, o, 16);
        *dst = out;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// fp32 epilogue: STORE 1 = plain store (exclusive tiles), 2 = atomic add
// (split-K).  BIAS adds the bias/ReLU terms of gemm_kernel; the wide dw
// kernels have none (their bias slot carries the fused db output).
template <int STORE, bool BIAS, int MF, int MROWS>
__device__ __forceinline__ void epilogue_f32(
    const f32x4 (&acc)[MF][4], float* C, const float* bias, int M, int N,
    int ldc, int tile_m, int tile_n, int wm, int wn, int lane, int relu,
    float alpha) {
  int crow0 = tile_m + wm * MROWS + ((lane >> 4) << 2);
  int ccol0 = tile_n + wn * 64 + (lane & 15);
#pragma unroll
  for (int fm = 0; fm < MF; ++fm) {
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      int col = ccol0 + fn * 16;
      if (col >= N) continue;
      float badd = (BIAS && bias != nullptr) ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = crow0 + fm * 16 + r;
        if (row >= M) continue;
        float v = acc[fm][fn][r] * alpha;
        if (BIAS) {
          v += badd;
          if (relu && v < 0.f) v = 0.f;
        }
        if (STORE == 1)
          C[(int64_t)row * ldc + col] = v;
        else
          atomicAdd(C + (int64_t)row * ldc + col, v);
      }
    }
  }
}

// 16-byte form of epilogue_f32's plain store (no bias), for gemm_fc_kernel's
// slabs (tried on gemm_wide_tt_kernel's dW store too: no gain at the three
// AlexNet FC shapes, profiles/alexnet_1gpu_fc_stream.md): a wave
// transposes its accumulators, one 16-row band at a time, through a
// private LDS slab (16 rows of NCOLS + 4 floats, as epilogue_bf16_vec) so
// that a lane holds 4 consecutive columns of one row and a store
// instruction covers whole 256-byte (NCOLS = 64) row segments instead of
// 64-byte ones.  The same floats reach the same addresses.  The caller
// guarantees N, ldc and col0 are multiples of 4, C is 16-byte aligned and
// nothing else uses `slab` any more.  row0 / col0: the wave tile's origin.
template <int NCOLS>
constexpr int f32_slab_floats() { return 16 * (NCOLS + 4); }

template <int MF, int NF, int NCOLS>
__device__ __forceinline__ void epilogue_f32_vec(
    const f32x4 (&acc)[MF][NF], float* slab, float* C, int M, int N, int ldc,
    int row0, int col0, int lane, float alpha) {
  constexpr int LD = NCOLS + 4;
  constexpr int GPR = NCOLS / 4;             // 4-column groups per row
  constexpr int TASKS = 16 * GPR;            // (row, group) pairs per band
  static_assert(TASKS % 64 == 0, "whole wave-instructions per band");
  int wr = (lane >> 4) << 2, wc = lane & 15;
#pragma unroll
  for (int fm = 0; fm < MF; ++fm) {
#pragma unroll
    for (int fn = 0; fn < NF; ++fn)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[(wr + r) * LD + fn * 16 + wc] = acc[fm][fn][r] * alpha;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t0 = 0; t0 < TASKS; t0 += 64) {
      int t = t0 + lane;
      int row = t / GPR, cg = t - row * GPR;
      int grow = row0 + fm * 16 + row;
      int col = col0 + cg * 4;
      if (grow < M && col < N)
        *reinterpret_cast<f32x4*>(C + (int64_t)grow * ldc + col) =
            *reinterpret_cast<const f32x4*>(slab + row * LD + cg * 4);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------- staging

// direct ([rows][K]) guarded staging: vectorized 8-wide along K when the
// 16-byte slot is fully in-bounds, scalar otherwise; zero-fills the rest.
__device__ __forceinline__ void stage_direct_guarded(
    bf16* lds_, const bf16* g_, int row0, int rows, int ld,
    int k0, int kend, int tid, int nthreads = NTHREADS) {
  auto* lds = reinterpret_cast<unsigned short*>(lds_);
  auto* g = reinterpret_cast<const unsigned short*>(g_);
  // 4096 elements, 512 slots of 8
  for (int slot = tid; slot < 512; slot += nthreads) {
    int row = slot >> 2;            // 4 slots of 8 per 32-wide row
    int kk = (slot & 3) * 8;
    int grow = row0 + row;
    int gk = k0 + kk;
    unsigned short* dst = lds + row * BK + (swz_chunk(row, slot & 3) << 3);
    if (grow < rows && gk + 8 <= kend && ((ld | gk) % 8 == 0)) {
      *reinterpret_cast<short8v*>(dst) =
          *reinterpret_cast<const short8v*>(g + (int64_t)grow * ld + gk);
    } else if (grow < rows) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dst[j] = (gk + j < kend) ? g[(int64_t)grow * ld + gk + j] : 0;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = 0;
    }
  }
}

// ---- transposed ([K][rows]) operand staging into the CANONICAL layout
// with u32 k-pair packing: each slot loads the same 8 output-dim columns
// of TWO adjacent K-rows (two coalesced 16-byte global reads), packs
// (k, k+1) element pairs into u32s, and writes 8 ds_write_b32 — half
// the write instructions at 4x wider grain than the previous 16 scalar
// b16 scatters, and ~4-way instead of 16-way bank conflicts (row*64B
// strides alias banks; the k-pair dimension now spreads them).
// Fragment reads stay the standard swizzled b128 path.

// the shared tail of the stage_trans_pair_* gathers: rows m0..m0+7 of
// k-pair kp, (k, k+1) packed into one u32 per row
__device__ __forceinline__ void write_kpairs(
    unsigned short* lds, int m0, int kp, const unsigned short (&va)[8],
    const unsigned short (&vb)[8]) {
  int kk = kp * 2;
  int chunk0 = kk >> 3, kin = kk & 7;    // position inside a 16B chunk
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int row = m0 + j;
    unsigned int packed = (unsigned int)va[j] |
                          ((unsigned int)vb[j] << 16);
    *reinterpret_cast<unsigned int*>(
        lds + row * BK + (swz_chunk(row, chunk0) << 3) + kin) = packed;
  }
}

__device__ __forceinline__ void stage_trans_pair_guarded(
    bf16* lds_, const bf16* g_, int row0, int rows, int ld,
    int k0, int kend, int tid, int nthreads = NTHREADS,
    int tile_rows = BM) {
  auto* lds = reinterpret_cast<unsigned short*>(lds_);
  auto* g = reinterpret_cast<const unsigned short*>(g_);
  int rslots = tile_rows >> 3;          // 8-column octets per k-pair
  int nslots = 16 * rslots;             // 16 k-pairs per BK=32 tile
  for (int slot = tid; slot < nslots; slot += nthreads) {
    int kp = slot & 15;                 // k-pair index (adjacent lanes
    int m0 = (slot >> 4) * 8;           //   get distinct kp: bank spread)
    unsigned short va[8], vb[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      unsigned short* v = h ? vb : va;
      int gk = k0 + kp * 2 + h;
      int gr = row0 + m0;
      if (gk < kend && gr + 8 <= rows && ((ld | gr) % 8 == 0)) {
        *reinterpret_cast<short8v*>(v) =
            *reinterpret_cast<const short8v*>(g + (int64_t)gk * ld + gr);
      } else if (gk < kend) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (gr + j < rows) ? g[(int64_t)gk * ld + gr + j] : 0;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0;
      }
    }
    write_kpairs(lds, m0, kp, va, vb);
  }
}

// CHUNKS 1 KB chunks (16 rows each) over WAVES waves.  With a zpage, a
// chunk past CHUNKS (TileCfg's surplus) or past the operand's `rows`
// still issues its instruction, from the zero page.
template <int WAVES = 4, int CHUNKS = 8>
__device__ __forceinline__ void stage_direct_fast(
    bf16* lds, const bf16* g, int row0, int ld, int k0, int tid,
    const bf16* zpage = nullptr, int rows = 0) {
  int wave = tid >> 6, lane = tid & 63;
  constexpr int CPW = (CHUNKS + WAVES - 1) / WAVES;  // chunks per wave
#pragma unroll
  for (int it = 0; it < CPW; ++it) {
    int chunk = wave * CPW + it;         // chunks of 512 elements
    int idx = chunk * 512 + lane * 8;    // linear element index in tile
    int row = idx >> 5;                  // /32
    int kk = swz_chunk(row, (idx & 31) >> 3) << 3;  // pre-swizzled source
    const bf16* src = g + (int64_t)(row0 + row) * ld + k0 + kk;
    if (zpage != nullptr && (chunk >= CHUNKS || row0 + row >= rows))
      src = zpage;
    auto* gp = (const __attribute__((address_space(1))) unsigned int*)src;
    auto* lp = (__attribute__((address_space(3))) unsigned int*)(
        lds + chunk * 512);
    __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
  }
}

// ----------------------------------------- implicit-im2col conv staging
// The col matrix's 8-element k-runs (one (r,s) tap, 8 consecutive
// channels) are contiguous channel spans of the NHWC input whenever
// Cg % 8 == 0, so the GEMM stages its col operand straight from x —
// zero-filling padding taps — and the col matrix (AlexNet conv2 alone:
// ~900 MB written + read twice per step) never materializes.

struct CGeom {
  int H, W, C;                       // input NHWC dims (C = all channels)
  int Q, PQ;                         // output width, P*Q
  int sh, sw, ph, pw, dil, S;
  int c0, Cg;                        // group channel window
  int Kcol;                          // R*S*Cg (zero beyond)
  // magic reciprocals: floor(n/d) == (n * m) >> 40 for n < 2^20
  unsigned long long mPQ, mQ, mCg, mS;
};

__device__ __forceinline__ unsigned mdiv(unsigned n,
                                         unsigned long long m) {
  return (unsigned)(((unsigned long long)n * m) >> 40);
}

static inline unsigned long long magic40(unsigned d) {
  return ((1ull << 40) + d - 1) / d;
}

// per-block output-pixel decode: rinfo[row] = {n*H*W, p*sh-ph, q*sw-pw}
__device__ __forceinline__ void decode_rows(int* rinfo, const CGeom& gm,
                                            int tile_m, int M, int rows,
                                            int tid) {
  for (int i = tid; i < rows; i += blockDim.x) {
    int m = tile_m + i;
    if (m >= M) m = M - 1;            // junk rows: valid addrs, masked out
    unsigned n = mdiv(m, gm.mPQ);
    unsigned pq = m - n * gm.PQ;
    unsigned p = mdiv(pq, gm.mQ);
    unsigned q = pq - p * gm.Q;
    rinfo[i * 3] = (int)(n * gm.H * gm.W);
    rinfo[i * 3 + 1] = (int)p * gm.sh - gm.ph;
    rinfo[i * 3 + 2] = (int)q * gm.sw - gm.pw;
  }
}

// A-operand staging for the forward conv GEMM: same LDS layout and DMA
// placement as stage_direct_fast, but the per-lane source address is the
// im2col gather.  Out-of-image (or k >= Kcol) lanes redirect their DMA
// to a 16-byte zero page instead of branching: the instruction always
// issues, so the pipeline's counted s_waitcnt vmcnt(N) stays exact (a
// divergent skip would desynchronize the count), and no LDS zero-fill
// writes are needed.
template <int WAVES, int CHUNKS = 8>
__device__ __forceinline__ void stage_implicit_fast(
    bf16* lds_, const bf16* X, const bf16* zpage, const CGeom& gm,
    const int* rinfo, int k0, int tid) {
  auto* lds = reinterpret_cast<unsigned short*>(lds_);
  int wave = tid >> 6, lane = tid & 63;
  constexpr int CPW = CHUNKS / WAVES;
#pragma unroll
  for (int it = 0; it < CPW; ++it) {
    int chunk = wave * CPW + it;
    int idx = chunk * 512 + lane * 8;
    int row = idx >> 5;
    int kk = swz_chunk(row, (idx & 31) >> 3) << 3;
    int k = k0 + kk;
    unsigned rs = mdiv(k, gm.mCg);
    int c = k - rs * gm.Cg;
    unsigned r = mdiv(rs, gm.mS);
    int s = rs - r * gm.S;
    int h = rinfo[row * 3 + 1] + (int)r * gm.dil;
    int w = rinfo[row * 3 + 2] + s * gm.dil;
    bool ok = (k < gm.Kcol) && (h >= 0) && (h < gm.H) && (w >= 0) &&
              (w < gm.W);
    int64_t off = ((int64_t)rinfo[row * 3] +
                   (int64_t)(h * gm.W + w)) * gm.C + gm.c0 + c;
    const bf16* src = ok ? X + off : zpage;
    auto* lp = (__attribute__((address_space(3))) unsigned int*)(
        lds + chunk * 512);
    auto* gp = (const __attribute__((address_space(1))) unsigned int*)src;
    __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
  }
}

// B-operand staging for the dw trans/trans GEMM: canonical u32 k-pair
// layout like stage_trans_pair_guarded, but each 8-column octet (one
// (r,s) tap, 8 channels) is gathered from x for two adjacent output
// pixels (the k-pair).
__device__ __forceinline__ void stage_trans_pair_implicit(
    bf16* lds_, const bf16* X, const CGeom& gm, int row0,
    int k0, int kend, int tid, int nthreads, int tile_rows) {
  auto* lds = reinterpret_cast<unsigned short*>(lds_);
  int rslots = tile_rows >> 3;
  int nslots = 16 * rslots;
  for (int slot = tid; slot < nslots; slot += nthreads) {
    int kp = slot & 15;
    int m0 = (slot >> 4) * 8;
    int gr = row0 + m0;                 // col-matrix column octet base
    unsigned rs = mdiv(gr, gm.mCg);
    int c = gr - rs * gm.Cg;
    unsigned r = mdiv(rs, gm.mS);
    int s = rs - r * gm.S;
    bool col_ok = gr < gm.Kcol;         // octet fully in/out (Kcol%8==0)
    int hr = (int)r * gm.dil - gm.ph;
    int ws = s * gm.dil - gm.pw;
    unsigned short va[8] = {}, vb[8] = {};
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      unsigned short* v = hh ? vb : va;
      int gk = k0 + kp * 2 + hh;        // output-pixel (npq) index
      if (gk < kend && col_ok) {
        unsigned n = mdiv(gk, gm.mPQ);
        unsigned pq = gk - n * gm.PQ;
        unsigned p = mdiv(pq, gm.mQ);
        unsigned q = pq - p * gm.Q;
        int hi = (int)p * gm.sh + hr;
        int wi = (int)q * gm.sw + ws;
        if (hi >= 0 && hi < gm.H && wi >= 0 && wi < gm.W) {
          const unsigned short* src =
              reinterpret_cast<const unsigned short*>(X) +
              ((int64_t)(n * gm.H + hi) * gm.W + wi) * gm.C + gm.c0 + c;
          *reinterpret_cast<short8v*>(v) =
              *reinterpret_cast<const short8v*>(src);
        }
      }
    }
    write_kpairs(lds, m0, kp, va, vb);
  }
}

// ---- small-C implicit staging (conv1-class layers, C % 8 != 0).
// With dil==1, c0==0 and full channels, the col matrix's k axis within
// one filter row r is a CONTIGUOUS span of the input row (k = r*S*C +
// s*C + c), so an 8-element slot is one unaligned 16-byte load (gfx950
// supports it natively), merging two loads when the slot straddles a
// filter-row boundary (S*C >= 8 keeps it to at most one straddle).
// CGeom field reuse for the _sc kernels: Cg/mCg hold S*C, S/mS hold C.

// NN A-operand [row=npq][k] into the canonical swizzled layout
__device__ __forceinline__ void stage_implicit_sc(
    bf16* lds_, const bf16* X, const CGeom& gm, const int* rinfo,
    int k0, int tid, int nthreads) {
  auto* lds = reinterpret_cast<unsigned short*>(lds_);
  auto* x = reinterpret_cast<const unsigned short*>(X);
  int SC = gm.Cg, C = gm.S;
  for (int slot = tid; slot < 512; slot += nthreads) {
    int row = slot >> 2;
    int kk = (slot & 3) * 8;
    int k = k0 + kk;
    unsigned short* dst = lds + row * BK + (swz_chunk(row, slot & 3) << 3);
    unsigned r0 = mdiv(k, gm.mCg);          // filter row
    int t0 = k - r0 * SC;                   // s*C + c within the row
    int h = rinfo[row * 3 + 1] + (int)r0;
    int w0 = rinfo[row * 3 + 2];
    int sp = SC - t0;                       // elements before r0+1
    // fully-interior slot: the spanned w range [w0, w0+S) is in-image
    bool interior = k + 8 <= gm.Kcol && h >= 0 && w0 >= 0 &&
                    w0 * C + SC <= gm.W * C &&
                    (sp >= 8 ? h < gm.H : h + 1 < gm.H);
    if (interior) {
      const unsigned short* a0 =
          x + ((int64_t)rinfo[row * 3] + (int64_t)h * gm.W) * C +
          w0 * C + t0;
      if (sp >= 8) {
        __builtin_memcpy(dst, a0, 16);
      } else {
        unsigned short lo[8], hi[8];
        __builtin_memcpy(lo, a0, 16);
        const unsigned short* a1 =
            x + ((int64_t)rinfo[row * 3] + (int64_t)(h + 1) * gm.W) * C +
            w0 * C;
        __builtin_memcpy(hi, a1, 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = j < sp ? lo[j] : hi[j - sp];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int kj = k + j;
        unsigned short v = 0;
        if (kj < gm.Kcol) {
          unsigned r = mdiv(kj, gm.mCg);
          int t = kj - r * SC;
          unsigned s = mdiv(t, gm.mS);
          int c = t - s * C;
          int hh = rinfo[row * 3 + 1] + (int)r;
          int ww = w0 + (int)s;
          if (hh >= 0 && hh < gm.H && ww >= 0 && ww < gm.W)
            v = x[((int64_t)rinfo[row * 3] +
                   (int64_t)hh * gm.W + ww) * C + c];
        }
        dst[j] = v;
      }
    }
  }
}

// TT B-operand [k=npq][col] u32 k-pair canonical layout
__device__ __forceinline__ void stage_trans_pair_implicit_sc(
    bf16* lds_, const bf16* X, const CGeom& gm, int row0,
    int k0, int kend, int tid, int nthreads, int tile_rows) {
  auto* lds = reinterpret_cast<unsigned short*>(lds_);
  auto* x = reinterpret_cast<const unsigned short*>(X);
  int SC = gm.Cg, C = gm.S;
  int rslots = tile_rows >> 3;
  int nslots = 16 * rslots;
  for (int slot = tid; slot < nslots; slot += nthreads) {
    int kp = slot & 15;
    int m0 = (slot >> 4) * 8;
    int gr = row0 + m0;                  // col-matrix column octet base
    unsigned r0 = mdiv(gr, gm.mCg);
    int t0 = gr - r0 * SC;
    int sp = SC - t0;
    unsigned short va[8] = {}, vb[8] = {};
#pragma unroll
    for (int hh2 = 0; hh2 < 2; ++hh2) {
      unsigned short* v = hh2 ? vb : va;
      int gk = k0 + kp * 2 + hh2;        // output-pixel index
      if (gk >= kend) continue;
      unsigned n = mdiv(gk, gm.mPQ);
      unsigned pq = gk - n * gm.PQ;
      unsigned p = mdiv(pq, gm.mQ);
      unsigned q = pq - p * gm.Q;
      int h = (int)p * gm.sh - gm.ph + (int)r0;
      int w0 = (int)q * gm.sw - gm.pw;
      bool interior = gr + 8 <= gm.Kcol && h >= 0 && w0 >= 0 &&
                      w0 * C + SC <= gm.W * C &&
                      (sp >= 8 ? h < gm.H : h + 1 < gm.H);
      int64_t nHW = (int64_t)(n * gm.H);
      if (interior) {
        const unsigned short* a0 =
            x + (nHW + h) * (int64_t)gm.W * C + w0 * C + t0;
        if (sp >= 8) {
          __builtin_memcpy(v, a0, 16);
        } else {
          unsigned short lo[8], hi[8];
          __builtin_memcpy(lo, a0, 16);
          const unsigned short* a1 =
              x + (nHW + h + 1) * (int64_t)gm.W * C + w0 * C;
          __builtin_memcpy(hi, a1, 16);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = j < sp ? lo[j] : hi[j - sp];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int kj = gr + j;
          if (kj >= gm.Kcol) continue;
          unsigned r = mdiv(kj, gm.mCg);
          int t = kj - r * SC;
          unsigned s = mdiv(t, gm.mS);
          int c = t - s * C;
          int hh = (int)p * gm.sh - gm.ph + (int)r;
          int ww = w0 + (int)s;
          if (hh >= 0 && hh < gm.H && ww >= 0 && ww < gm.W)
            v[j] = x[(nHW + hh) * (int64_t)gm.W * C + ww * C + c];
        }
      }
    }
    write_kpairs(lds, m0, kp, va, vb);
  }
}

// ---------------------------------------------- wide-N trans/trans kernel
// Specialized for the skinny trans/trans weight-gradient GEMMs
// (dw[Kout][Kcol] = dy^T @ col, K = N*P*Q huge): BN=256 halves the
// A-operand re-read factor vs the 128x128 kernel; fp32 atomic split-K.
// The col operand (B) comes from one of three staging policies.

constexpr int WBN = 256;
constexpr int WNT = 512;  // 8 waves: 2 (M) x 4 (N)

struct BGuarded {         // materialized [K][N] matrix
  const bf16* B;
  int ldb;
  __device__ __forceinline__ void stage(bf16* lds, int row0, int N, int k0,
                                        int kend, int tid) const {
    stage_trans_pair_guarded(lds, B, row0, N, ldb, k0, kend, tid, WNT, WBN);
  }
};

struct BImplicit {        // im2col gather from the NHWC input, Cg % 8 == 0
  const bf16* X;
  CGeom gm;
  __device__ __forceinline__ void stage(bf16* lds, int row0, int, int k0,
                                        int kend, int tid) const {
    stage_trans_pair_implicit(lds, X, gm, row0, k0, kend, tid, WNT, WBN);
  }
};

struct BImplicitSC {      // small-C contiguous-run gather
  const bf16* X;
  CGeom gm;
  __device__ __forceinline__ void stage(bf16* lds, int row0, int, int k0,
                                        int kend, int tid) const {
    stage_trans_pair_implicit_sc(lds, X, gm, row0, k0, kend, tid, WNT, WBN);
  }
};

template <int STORE, class BStage>  // STORE as in epilogue_f32
__global__ __launch_bounds__(WNT, 1) void gemm_wide_tt_kernel(
    const bf16* __restrict__ A, float* __restrict__ C, int M, int N, int K,
    int lda, int ldc, int ksplit, float alpha, float* __restrict__ db,
    BStage bstage) {
  __shared__ bf16 As[BM * BK];
  __shared__ bf16 Bs[WBN * BK];

  Tile t = decode_tile<WBN>(M, N);
  int tile_m = t.tile_m, tile_n = t.tile_n;
  int k_begin = blockIdx.y * ksplit;
  int k_end = min(K, k_begin + ksplit);

  int tid = threadIdx.x;
  int wave = tid >> 6, lane = tid & 63;
  int wm = wave >> 2, wn = wave & 3;     // 2x4 wave grid, 64x64 each

  f32x4 acc[4][4] = {};

  // fused bias gradient: db[m] += sum_k A[k][m] — the A tiles are in
  // LDS anyway; the bn==0 blocks of each k-split cover every k exactly
  // once (colsum was 4-5%% of the AlexNet/GoogLeNet steps as separate
  // ramp-bound launches over the same dy operand)
  bool do_db = (db != nullptr) && (t.bn == 0);
  for (int k0 = k_begin; k0 < k_end; k0 += BK) {
    stage_trans_pair_guarded(As, A, tile_m, M, lda, k0, k_end, tid, WNT,
                             BM);
    bstage.stage(Bs, tile_n, N, k0, k_end, tid);
    __syncthreads();
    if (do_db && tid < BM && tile_m + tid < M) {
      float acc_b = 0.f;
      const bf16* row = As + tid * BK;
#pragma unroll
      for (int kk = 0; kk < BK; ++kk)
        acc_b += bf2f(row[(swz_chunk(tid, kk >> 3) << 3) | (kk & 7)]);
      atomicAdd(db + tile_m + tid, acc_b);
    }
    load_frags_mfma<4, 64, false>(As, Bs, wm, wn, lane, acc);
    __syncthreads();
  }

  epilogue_f32<STORE, false, 4, 64>(acc, C, nullptr, M, N, ldc, tile_m,
                                    tile_n, wm, wn, lane, 0, alpha);
}

// ------------------------------------------------- pipelined K loop
// Shared by the kernels whose operands are both staged by direct-to-LDS
// DMA.  A ring of DEPTH LDS buffers, prefetching DEPTH/2 tiles ahead: the
// DMA of tile t+PF is issued BEFORE computing tile t, and the pre-barrier
// wait is a COUNTED `s_waitcnt vmcnt(N)` (the loads just issued stay in
// flight across the barrier) rather than __syncthreads' full drain —
// cdna_hip_programming.md §5.5 T3/T4: "never drain vmcnt to 0 in the
// main loop".
//   DEPTH=2: a trailing barrier keeps stage(t+1) off buf[t&1] until all
//     waves finished reading it (the ds_reads completed before their
//     MFMAs, so no counter drain is needed at that barrier).
//   DEPTH=4: one barrier per tile — the buffer written at iter t+1 (slot
//     (t+3)&3) was last read at iter t-1, and barrier_t separates them.
//     65.5 KB of LDS, still 2 blocks/CU within CDNA4's 160 KB.
// Needs k_end - k_begin to be a multiple of BK and at least PF tiles (the
// hosts pad to two): the prologue and the tail assume PF tiles exist.

struct ADirect {          // [rows][K] matrix
  const bf16* A;
  int row0, ld;
  template <int WAVES, int CHUNKS>
  __device__ __forceinline__ void stage(bf16* lds, int k0, int tid) const {
    stage_direct_fast<WAVES, CHUNKS>(lds, A, row0, ld, k0, tid);
  }
};

struct AImplicit {        // im2col gather from the NHWC input
  const bf16* X;
  const bf16* zpage;
  const CGeom& gm;
  const int* rinfo;
  template <int WAVES, int CHUNKS>
  __device__ __forceinline__ void stage(bf16* lds, int k0, int tid) const {
    stage_implicit_fast<WAVES, CHUNKS>(lds, X, zpage, gm, rinfo, k0, tid);
  }
};

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Asb / Bsb: the ring's DEPTH stages of Cfg::A_ELEMS / Cfg::B_ELEMS each.
// zpage / b_rows: stage_direct_fast's guard for B (nullptr: none).
template <class Cfg, int DEPTH, class AStage>
__device__ __forceinline__ void pipelined_loop(
    bf16* Asb, bf16* Bsb, const AStage& astage, const bf16* B,
    const bf16* zpage, int b_rows, int tile_n, int ldb, int k_begin,
    int k_end, int tid, int wm, int wn, int lane,
    f32x4 (&acc)[Cfg::MF][Cfg::NF]) {
  constexpr int WAVES = Cfg::WAVES;
  constexpr int PF = DEPTH / 2;              // tiles in flight ahead
  // each wave issues A_CPW + B_CPW DMA loads per tile; the PF prefetched
  // tiles' loads stay outstanding while the current tile's are waited for
  constexpr int VMCNT = PF * (Cfg::A_CPW + Cfg::B_CPW);
#pragma unroll
  for (int p = 0; p < PF; ++p)
    if (p == 0 || k_begin + p * BK < k_end) {
      astage.template stage<WAVES, Cfg::A_CHUNKS>(
          Asb + p * Cfg::A_ELEMS, k_begin + p * BK, tid);
      stage_direct_fast<WAVES, Cfg::B_CHUNKS>(
          Bsb + p * Cfg::B_ELEMS, B, tile_n, ldb, k_begin + p * BK, tid,
          zpage, b_rows);
    }
  int cur = 0;                               // ring slot of tile k0
  auto compute = [&](int slot) {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    load_frags_mfma<Cfg::MF, Cfg::MROWS, true, Cfg::NF, Cfg::NCOLS>(
        Asb + slot * Cfg::A_ELEMS, Bsb + slot * Cfg::B_ELEMS, wm, wn, lane,
        acc);
  };
  int k0 = k_begin;
  for (; k0 + PF * BK < k_end; k0 += BK) {
    int nxt = (cur + PF) & (DEPTH - 1);
    astage.template stage<WAVES, Cfg::A_CHUNKS>(
        Asb + nxt * Cfg::A_ELEMS, k0 + PF * BK, tid);
    stage_direct_fast<WAVES, Cfg::B_CHUNKS>(
        Bsb + nxt * Cfg::B_ELEMS, B, tile_n, ldb, k0 + PF * BK, tid, zpage,
        b_rows);
    wait_vmcnt<VMCNT>();
    compute(cur);
    if (DEPTH == 2) __builtin_amdgcn_s_barrier();
    cur = (cur + 1) & (DEPTH - 1);
  }
  // the last PF tiles: nothing more is issued, so fewer loads stay in
  // flight behind the awaited tile and the count shrinks with them
  static_assert(PF == 1 || PF == 2, "tail waits written out for PF <= 2");
  if (PF == 2) {
    wait_vmcnt<VMCNT / 2>();
    compute(cur);
    cur = (cur + 1) & (DEPTH - 1);
  }
  wait_vmcnt<0>();
  compute(cur);
}

// ------------------------------------------------------------------ kernel

// WAVES=4: 2x2 wave grid of 64x64 (2 blocks/CU = 8 waves/CU);
// WAVES=8: 4x2 grid of 32x64 (2 blocks/CU = 16 waves/CU — doubles the
// wave-level parallelism hiding the staging/fragment latency).
// STORE_MODE: 0 = bf16 store, 3 = bf16 RMW accumulate, 1 = fp32 store,
// 2 = fp32 atomic add (split-K).
template <bool TRANS_A, bool TRANS_B, int STORE_MODE, int WAVES = 4>
__global__ __launch_bounds__(WAVES * 64, 2) void gemm_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    void* __restrict__ C, const float* __restrict__ bias,
    int M, int N, int K, int lda, int ldb, int ldc,
    int ksplit, int relu, float alpha, int m_alloc, int n_alloc,
    int64_t sA, int64_t sB, int64_t sC) {
  // batched operation (blockIdx.z = batch index, strides in elements for
  // A/B and BYTES for C since its type depends on STORE_MODE)
  A += (int64_t)blockIdx.z * sA;
  B += (int64_t)blockIdx.z * sB;
  C = (void*)((char*)C + (int64_t)blockIdx.z * sC);
  __shared__ bf16 Asb[2][BM * BK];
  __shared__ bf16 Bsb[2][BN * BK];

  Tile t = decode_tile<BN>(M, N);
  int tile_m = t.tile_m, tile_n = t.tile_n;
  int k_begin = blockIdx.y * ksplit;
  int k_end = min(K, k_begin + ksplit);

  constexpr int NT = WAVES * 64;
  constexpr int MROWS = mrows_of(WAVES), MF = mfrags_of(WAVES);
  int tid = threadIdx.x;
  int wave = tid >> 6, lane = tid & 63;
  int wm = wave >> 1, wn = wave & 1;     // (WAVES/2) x 2 wave grid

  f32x4 acc[MF][4] = {};

  // fast path only needs the STAGED rows to be readable: callers may
  // over-allocate operand buffers (m_alloc/n_alloc >= M/N) so edge tiles
  // stage junk rows whose outputs the epilogue guards discard
  bool a_fast = !TRANS_A && (tile_m + BM <= m_alloc) && (lda % 8 == 0) &&
                ((k_end - k_begin) % BK == 0) && (k_begin % 8 == 0);
  bool b_fast = !TRANS_B && (tile_n + BN <= n_alloc) && (ldb % 8 == 0) &&
                ((k_end - k_begin) % BK == 0) && (k_begin % 8 == 0);

  if (a_fast && b_fast && (k_end - k_begin) >= 2 * BK) {
    pipelined_loop<Tile128<WAVES>, 2>(
        &Asb[0][0], &Bsb[0][0], ADirect{A, tile_m, lda}, B, nullptr, 0,
        tile_n, ldb, k_begin, k_end, tid, wm, wn, lane, acc);
  } else {
    bf16* As = Asb[0];
    bf16* Bs = Bsb[0];
    for (int k0 = k_begin; k0 < k_end; k0 += BK) {
      if (a_fast) {
        stage_direct_fast<WAVES>(As, A, tile_m, lda, k0, tid);
      } else if (TRANS_A) {
        stage_trans_pair_guarded(As, A, tile_m, M, lda, k0, k_end, tid,
                                 NT);
      } else {
        stage_direct_guarded(As, A, tile_m, M, lda, k0, k_end, tid, NT);
      }
      if (b_fast) {
        stage_direct_fast<WAVES>(Bs, B, tile_n, ldb, k0, tid);
      } else if (TRANS_B) {
        stage_trans_pair_guarded(Bs, B, tile_n, N, ldb, k0, k_end, tid,
                                 NT);
      } else {
        stage_direct_guarded(Bs, B, tile_n, N, ldb, k0, k_end, tid, NT);
      }
      __syncthreads();
      load_frags_mfma<MF, MROWS, false>(As, Bs, wm, wn, lane, acc);
      __syncthreads();
    }
  }

  if (STORE_MODE == 0 || STORE_MODE == 3)
    epilogue_bf16<MF, MROWS>(acc, reinterpret_cast<bf16*>(C), bias, M, N,
                             ldc, tile_m, tile_n, wm, wn, lane, relu, alpha,
                             std::bool_constant<STORE_MODE == 3>{});
  else
    epilogue_f32<STORE_MODE, true, MF, MROWS>(
        acc, reinterpret_cast<float*>(C), bias, M, N, ldc, tile_m, tile_n,
        wm, wn, lane, relu, alpha);
}

// ------------------------------------------------------ forward conv GEMMs

// forward conv GEMM: C[NPQ, Kg] = im2col(x) @ Wr^T, bias+ReLU fused.
// Always the pipelined loop: the implicit A staging zero-fills
// k >= Kcol, so K runs over Kpad (32-aligned by the host) with no
// guarded edge cases, and Wr's padded rows/columns are zero.
//
// Cfg is the block tile (TileCfg): N tiles of 48, 64, 96 and 128 columns
// so that a layer's output width is padded to 16, not to 128.  The k
// order of every output element is the same in all of them (one
// 16x16x32 MFMA per K tile, ascending), so they agree bit for bit.
//
// blockIdx.y is the group of a grouped convolution: group g reads input
// channels from c0 + g*gs_c, B rows from g*gs_b, bias from g*N, and
// writes C columns from g*gs_n — one launch where the host used to loop.
//
// One __shared__ object for ring and rinfo: a second object beside a
// DMA-staged array can make the compiler drain vmcnt before LDS reads.
template <class Cfg, int DEPTH>
__global__ __launch_bounds__(Cfg::WAVES * 64, 2) void gemm_conv_fwd_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ B,
    bf16* __restrict__ C, const float* __restrict__ bias,
    const bf16* __restrict__ zpage,
    int M, int N, int K, int ldb, int ldc, int relu, int accum,
    CGeom gm, int gs_c, int gs_b, int gs_n, int vec) {
  // B holds pad128(N) rows per group (zero beyond N); a forced narrow
  // tile can round N up past that, and those rows come from zpage
  int b_rows = (N + 127) / 128 * 128;
  constexpr int RING = DEPTH * (Cfg::A_ELEMS + Cfg::B_ELEMS);
  constexpr int STAGING = RING + Cfg::TBM * 3 * (sizeof(int) / sizeof(bf16));
  // the vector epilogue's slabs reuse the ring (and rinfo) after the loop
  constexpr int SLABS = vec_slab_floats<Cfg>() * (sizeof(float) / sizeof(bf16));
  __shared__ __attribute__((aligned(16)))
  bf16 smem[STAGING > SLABS ? STAGING : SLABS];
  bf16* Asb = smem;
  bf16* Bsb = smem + DEPTH * Cfg::A_ELEMS;
  int* rinfo = reinterpret_cast<int*>(smem + RING);

  int g = blockIdx.y;
  gm.c0 += g * gs_c;
  B += (int64_t)g * gs_b * ldb;
  C += g * gs_n;
  if (bias != nullptr) bias += g * N;

  Tile t = decode_tile<Cfg::TBN, Cfg::TBM>(M, N);
  int tid = threadIdx.x;
  int wave = tid >> 6, lane = tid & 63;
  int wm = wave / Cfg::WN, wn = wave % Cfg::WN;

  decode_rows(rinfo, gm, t.tile_m, M, Cfg::TBM, tid);
  __syncthreads();

  f32x4 acc[Cfg::MF][Cfg::NF] = {};
  pipelined_loop<Cfg, DEPTH>(Asb, Bsb, AImplicit{X, zpage, gm, rinfo}, B,
                             zpage, b_rows, t.tile_n, ldb, 0, K, tid, wm,
                             wn, lane, acc);
  if (vec) {
    __syncthreads();                 // every wave is done reading the ring
    epilogue_bf16_vec<Cfg>(acc, reinterpret_cast<float*>(smem), C, bias, M,
                           N, ldc, t.tile_m, t.tile_n, wm, wn, wave, lane,
                           relu, accum);
  } else {
    epilogue_bf16<Cfg::MF, Cfg::MROWS, Cfg::NF, Cfg::NCOLS>(
        acc, C, bias, M, N, ldc, t.tile_m, t.tile_n, wm, wn, lane, relu,
        1.f, accum != 0);
  }
}

// small-C forward conv GEMM: double-buffered __syncthreads pipeline
// (the ds_write staging has no counted-vmcnt scheme to preserve)
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 2) void gemm_conv_fwd_sc_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ B,
    bf16* __restrict__ C, const float* __restrict__ bias,
    int M, int N, int K, int ldb, int ldc, int relu, CGeom gm) {
  __shared__ bf16 Asb[2][BM * BK];
  __shared__ bf16 Bsb[2][BN * BK];
  __shared__ int rinfo[BM * 3];

  Tile tl = decode_tile<BN>(M, N);
  constexpr int NT = WAVES * 64;
  constexpr int MROWS = mrows_of(WAVES), MF = mfrags_of(WAVES);
  int tid = threadIdx.x;
  int wave = tid >> 6, lane = tid & 63;
  int wm = wave >> 1, wn = wave & 1;

  decode_rows(rinfo, gm, tl.tile_m, M, BM, tid);
  __syncthreads();

  f32x4 acc[MF][4] = {};
  // double-buffered, ONE barrier per tile: staging t+1 (into buf^1)
  // overlaps compute of t; the end-of-iteration barrier covers both
  // "staging t+1 done" and "all reads of buf[t&1] done" before the
  // next iteration's stage(t+2) overwrites it
  int T = K / BK;
  stage_implicit_sc(Asb[0], X, gm, rinfo, 0, tid, NT);
  stage_direct_fast<WAVES>(Bsb[0], B, tl.tile_n, ldb, 0, tid);
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) {
      stage_implicit_sc(Asb[(t + 1) & 1], X, gm, rinfo, (t + 1) * BK,
                        tid, NT);
      stage_direct_fast<WAVES>(Bsb[(t + 1) & 1], B, tl.tile_n, ldb,
                               (t + 1) * BK, tid);
    }
    load_frags_mfma<MF, MROWS, false>(Asb[t & 1], Bsb[t & 1], wm, wn, lane,
                                      acc);
    __syncthreads();
  }

  epilogue_bf16<MF, MROWS>(acc, C, bias, M, N, ldc, tl.tile_m, tl.tile_n,
                           wm, wn, lane, relu, 1.f, std::false_type{});
}

// ------------------------------------- DMA-staged conv dW (trans/trans)
// gemm_wide_tt_kernel<., BImplicit> with both operands staged by
// direct-to-LDS DMA in their natural K-major layout and transposed on
// the way out of LDS by ds_read_b64_tr_b16: no staging registers, no
// ds_write scatter, and a counted-vmcnt ring instead of two full drains
// per tile.
//
// LDS image of one K tile (one ring stage, 24 KB): three [32 k][128 col]
// bf16 sub-images of 256-byte rows — A (dy, 128 m), then the two
// 128-column halves of the 256-wide col tile.  Within a sub-image the
// sixteen 16-byte chunks of a row are XOR-swizzled (dw_tr_off below;
// tests/test_conv_dw_tr_layout.py mirrors it and checks bijection,
// fragment contents and bank conflicts).  DMA writes LDS linearly, so
// the swizzle sits on the SOURCE side as in stage_direct_fast: the lane
// filling chunk position (row, ch') fetches global chunk ch' ^ f(row).
//
// Fragment read: per 16-lane group g = lane>>4 a transposed read takes a
// block of 4 k-rows x 16 columns; lane 4q+p supplies the address of row
// q, columns 4p..4p+3, and lane i receives column i.  Two reads (k-rows
// 8g..8g+3 and 8g+4..8g+7 at columns c0..c0+15) hand lane (i, g) the 8
// consecutive k of row c0+i: the 16x16x32 operand load_frags_mfma builds
// from one ds_read_b128.  Needs EXEC all ones (no divergence around the
// reads) and 8-byte-aligned addresses.

constexpr int TR_SUB = 32 * 256;          // bytes of one [32][128] image
constexpr int TR_STAGE = 3 * TR_SUB;      // A + two B halves
// Ring depth 3 (72 KB, two blocks per CU).  Measured on the five AlexNet
// dW shapes at the default split (profiles/alexnet_1gpu_dw_tr.md): depth
// 2, 3 and 4 are within 2% of each other there; 4 (96 KB, one block per
// CU) is 9-27% slower once the grid exceeds one block per CU.
constexpr int DW_TR_DEPTH = 3;

// byte offset of 16-byte chunk ch (0..15) of k-row `row` (0..31) inside
// a [32][128] sub-image.  Mirrored by dw_tr_off in
// tests/test_conv_dw_tr_layout.py — change both together.
__device__ __forceinline__ int dw_tr_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// One transposed read, as inline assembly rather than
// __builtin_amdgcn_ds_read_tr16_b64_v4bf16: the compiler cannot tell an
// LDS read of one ring stage from the DMA in flight into another, so
// before every LDS read it can see it drains vmcnt to 0 — which would
// wait for the tiles just prefetched and undo the ring.  Reads it cannot
// see get no such wait; wait_frags_tr supplies the lgkmcnt wait they need.
__device__ __forceinline__ bf16x4 ds_read_tr16(unsigned addr) {
  bf16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}

// all of a tile's transposed reads have landed; the operands tie the
// wait to the registers so no consumer is scheduled above it
__device__ __forceinline__ void wait_frags_tr(bf16x4 (&a)[4][2],
                                              bf16x4 (&b)[4][2]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]),
                 "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[3][0]), "+v"(a[3][1]),
                 "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[1][0]), "+v"(b[1][1]),
                 "+v"(b[2][0]), "+v"(b[2][1]), "+v"(b[3][0]), "+v"(b[3][1])
               :: "memory");
}

// Sibling of pipelined_loop rather than a generalisation of it: here the
// DMA of tile t+DEPTH-1 is issued AFTER barrier t (into the slot tile t-1
// was read from), which gives DEPTH-1 tiles of prefetch on one barrier
// per tile at any depth, and every DMA always issues — tiles past the
// split's end fetch the zero page — so the counted wait is exact for any
// tile count >= 1 (pipelined_loop needs >= 2 and a power-of-two ring).
template <int STORE, int DEPTH>
__global__ __launch_bounds__(WNT, DEPTH <= 3 ? 4 : 2)
void gemm_conv_dw_tr_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ X,
    const bf16* __restrict__ zpage, float* __restrict__ C, int M, int N,
    int K, int lda, int ldc, int ksplit, float alpha, CGeom gm) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[DEPTH * TR_STAGE];

  Tile t = decode_tile<WBN>(M, N);
  int tile_m = t.tile_m, tile_n = t.tile_n;
  int k_begin = blockIdx.y * ksplit;
  int k_end = min(K, k_begin + ksplit);

  int tid = threadIdx.x;
  int wave = tid >> 6, lane = tid & 63;
  int wm = wave >> 2, wn = wave & 3;     // 2x4 wave grid, 64x64 each

  // ---- staging: wave w's DMA fills bytes [1024w, 1024w+1024) of each
  // sub-image, i.e. k-rows 4w..4w+3; lane l fills chunk position
  // (4w + l/16, l%16) and so fetches source chunk sch of that k-row.
  // Everything but the output pixel (the k-row) is fixed per lane.
  int srow = wave * 4 + (lane >> 4);
  int sch = (dw_tr_off(srow, lane & 15) >> 4) & 15;
  int am = tile_m + sch * 8;             // A column octet (M % 8 == 0)
  bool a_ok = am < M;
  int hr[2], ws[2], cc[2];
  bool col_ok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int gr = tile_n + j * 128 + sch * 8;  // col-matrix column octet
    unsigned rs = mdiv(gr, gm.mCg);
    int c = gr - rs * gm.Cg;
    unsigned r = mdiv(rs, gm.mS);
    int s = rs - r * gm.S;
    col_ok[j] = gr < gm.Kcol;            // octet fully in/out (Kcol%8==0)
    hr[j] = (int)r * gm.dil - gm.ph;
    ws[j] = s * gm.dil - gm.pw;
    cc[j] = gm.c0 + c;
  }
  const unsigned short* xs = reinterpret_cast<const unsigned short*>(X);
  const unsigned short* as = reinterpret_cast<const unsigned short*>(A);
  typedef const __attribute__((address_space(1))) unsigned int* gptr;
  typedef __attribute__((address_space(3))) unsigned int* lptr;

  // Branch-free: every lane computes its address and then selects it or
  // the zero page, so each DMA issues once with EXEC all ones.  (Left to
  // itself the compiler branches around the 64-bit address arithmetic
  // and issues the DMA once per side of the branch; keep_v pins the
  // computed offset in front of the select.)
  auto keep_v = [](int64_t v) {
    asm volatile("" : "+v"(v));
    return v;
  };
  auto stage = [&](int slot, int k0) {
    unsigned char* base = smem + slot * TR_STAGE + wave * 1024;
    int k = k0 + srow;                   // output pixel (npq) index
    bool k_ok = k < k_end;
    int64_t aoff = keep_v((int64_t)k * lda + am);
    const void* asrc = (k_ok & a_ok) ? (const void*)(as + aoff)
                                      : (const void*)zpage;
    __builtin_amdgcn_global_load_lds((gptr)asrc, (lptr)base, 16, 0, 0);
    unsigned n = mdiv(k, gm.mPQ);
    unsigned pq = k - n * gm.PQ;
    unsigned p = mdiv(pq, gm.mQ);
    unsigned q = pq - p * gm.Q;
    int nH = (int)n * gm.H, ph0 = (int)p * gm.sh, qw0 = (int)q * gm.sw;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int hi = ph0 + hr[j], wi = qw0 + ws[j];
      // unsigned compares fold the >= 0 tests; & not &&: no branches
      bool ok = k_ok & col_ok[j] & ((unsigned)hi < (unsigned)gm.H) &
                ((unsigned)wi < (unsigned)gm.W);
      // pixel index in 32 bits (the magic division already needs
      // NPQ < 2^20, and NHW is about stride^2 times that), element
      // offset in 64
      int64_t boff = keep_v((int64_t)((nH + hi) * gm.W + wi) * gm.C + cc[j]);
      const void* bsrc = ok ? (const void*)(xs + boff) : (const void*)zpage;
      __builtin_amdgcn_global_load_lds(
          (gptr)bsrc, (lptr)(base + (1 + j) * TR_SUB), 16, 0, 0);
    }
  };

  // ---- fragment read addresses (fixed per lane): group g reads k-rows
  // 8g+4h+q; lane 4q+p of the group supplies columns 4p..4p+3, i.e.
  // 8-byte half p&1 of chunk c0 + p/2 — addressed through dw_tr_off
  // because the XOR can swap the two chunks of a row's 32 bytes.
  // Fragment f's chunk is c0 + 2f with bits 1-2 of c0 clear, and the
  // swizzle is an XOR too, so its address is fragment 0's ^ (f << 5):
  // four address registers instead of sixteen.
  int fq = (lane >> 2) & 3, fp = lane & 3, fg = lane >> 4;
  int a_addr[2], b_addr[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int row = 8 * fg + 4 * h + fq;
    a_addr[h] = dw_tr_off(row, wm * 8 + (fp >> 1)) + 8 * (fp & 1);
    b_addr[h] = (1 + (wn >> 1)) * TR_SUB +
                dw_tr_off(row, (wn & 1) * 8 + (fp >> 1)) + 8 * (fp & 1);
  }

  unsigned lds0 = (unsigned)(uintptr_t)(
      (__attribute__((address_space(3))) unsigned char*)smem);

  f32x4 acc[4][4] = {};

  constexpr int PF = DEPTH - 1;          // tiles in flight ahead
  constexpr int VMCNT = 3 * (PF - 1);    // 3 DMAs per wave per tile
  int tiles = (k_end - k_begin + BK - 1) / BK;
#pragma unroll
  for (int p = 0; p < PF; ++p) stage(p, k_begin + p * BK);
  int cur = 0;                           // ring slot of tile i
  for (int i = 0; i < tiles; ++i) {
    wait_vmcnt<VMCNT>();                 // this wave's part of tile i landed
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();        // everyone's did; tile i-1 is read
    int nxt = cur == 0 ? DEPTH - 1 : cur - 1;   // (i + PF) % DEPTH
    stage(nxt, k_begin + (i + PF) * BK);
    int img = cur * TR_STAGE;            // multiple of 128: keeps the XOR
    bf16x4 ar[4][2], br[4][2];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        br[f][h] = ds_read_tr16(lds0 + ((img + b_addr[h]) ^ (f << 5)));
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        ar[f][h] = ds_read_tr16(lds0 + ((img + a_addr[h]) ^ (f << 5)));
    wait_frags_tr(ar, br);
    bf16x8 afrag[4], bfrag[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      afrag[f] = __builtin_shufflevector(ar[f][0], ar[f][1], 0, 1, 2, 3, 4,
                                         5, 6, 7);
      bfrag[f] = __builtin_shufflevector(br[f][0], br[f][1], 0, 1, 2, 3, 4,
                                         5, 6, 7);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int fn = 0; fn < 4; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag[fm], bfrag[fn], acc[fm][fn], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    cur = cur + 1 == DEPTH ? 0 : cur + 1;
  }
  wait_vmcnt<0>();                       // the zero-page tail DMAs

  epilogue_f32<STORE, false, 4, 64>(acc, C, nullptr, M, N, ldc, tile_m,
                                    tile_n, wm, wn, lane, 0, alpha);
}

// ------------------------------------------------------------------- host

// 8-wave blocks win on skinny shapes (one of M/N <= 256: fc6 +12%,
// conv2/conv5 fwd +6-7%, conv1 +6% measured) and lose on fat ones
// (conv3 -15%); COS_GEMM_W8=0/1 forces either variant for A/B.
static bool use_w8(int M, int N) {
  static const int w8_env = [] {
    const char* e = getenv("COS_GEMM_W8");
    return e ? (e[0] == '1' ? 1 : 0) : -1;
  }();
  return (w8_env == -1) ? (M <= 256 || N <= 256) : (w8_env == 1);
}

// split-K block arithmetic: K elements per split (BK-aligned so split
// boundaries fall on tile boundaries) and the resulting grid.y
struct SplitK { int ksplit, zblocks; };

static SplitK split_k(int K, int splitk) {
  splitk = max(1, splitk);
  int ksplit = (K + splitk - 1) / splitk;
  ksplit = ((ksplit + BK - 1) / BK) * BK;
  return {ksplit, (K + ksplit - 1) / ksplit};
}

// plain store only when asked for AND every output element is written
// by exactly one block; atomics otherwise
template <class BStage>
static void launch_wide_tt(const bf16* A, float* C, int M, int N, int K,
                           int lda, int ldc, int store_mode, SplitK sk,
                           float alpha, float* db, BStage bstage,
                           hipStream_t stream) {
  int mblocks = (M + BM - 1) / BM, nblocks = (N + WBN - 1) / WBN;
  dim3 grid(mblocks * nblocks, sk.zblocks);
  if (store_mode == 1 && sk.zblocks == 1)
    gemm_wide_tt_kernel<1><<<grid, WNT, 0, stream>>>(
        A, C, M, N, K, lda, ldc, sk.ksplit, alpha, db, bstage);
  else
    gemm_wide_tt_kernel<2><<<grid, WNT, 0, stream>>>(
        A, C, M, N, K, lda, ldc, sk.ksplit, alpha, db, bstage);
}

void gemm_bf16_batched(const void* A_, const void* B_, void* C,
                       const float* bias, int M, int N, int K, int lda,
                       int ldb, int ldc, bool trans_a, bool trans_b,
                       int store_mode, int splitk, bool relu, float alpha,
                       int m_alloc, int n_alloc, int batch, int64_t sA,
                       int64_t sB, int64_t sC_bytes, hipStream_t stream) {
  if (m_alloc < M) m_alloc = M;
  if (n_alloc < N) n_alloc = N;
  const bf16* A = reinterpret_cast<const bf16*>(A_);
  const bf16* B = reinterpret_cast<const bf16*>(B_);
  int mblocks = (M + BM - 1) / BM, nblocks = (N + BN - 1) / BN;
  SplitK sk = split_k(K, splitk);
  int ksplit = sk.ksplit;
  if (sk.zblocks > 1 && store_mode != 2)
    throw std::runtime_error("gemm: split-K requires atomic store mode");
  // store_mode 3 = bf16 RMW accumulate (single split only)
  dim3 grid(mblocks * nblocks, sk.zblocks, batch);
  dim3 block(NTHREADS);

#define COS_GEMM_CASE(TA, TB, SM)                                          \
  gemm_kernel<TA, TB, SM><<<grid, block, 0, stream>>>(                      \
      A, B, C, bias, M, N, K, lda, ldb, ldc, ksplit, relu ? 1 : 0, alpha,    \
      m_alloc, n_alloc, sA, sB, sC_bytes)

#define COS_GEMM_CASE8(SM)                                                 \
  gemm_kernel<false, false, SM, 8><<<grid, dim3(512), 0, stream>>>(        \
      A, B, C, bias, M, N, K, lda, ldb, ldc, ksplit, relu ? 1 : 0, alpha,   \
      m_alloc, n_alloc, sA, sB, sC_bytes)

#define COS_GEMM_SM(TA, TB)                                                 \
  do {                                                                      \
    if (store_mode == 0)      COS_GEMM_CASE(TA, TB, 0);                     \
    else if (store_mode == 1) COS_GEMM_CASE(TA, TB, 1);                     \
    else if (store_mode == 3) COS_GEMM_CASE(TA, TB, 3);                     \
    else                      COS_GEMM_CASE(TA, TB, 2);                     \
  } while (0)

  if (trans_a && trans_b && store_mode >= 1 && N > 128 && batch == 1) {
    // bias = fused db
    launch_wide_tt(A, reinterpret_cast<float*>(C), M, N, K, lda, ldc,
                   store_mode, sk, alpha, const_cast<float*>(bias),
                   BGuarded{B, ldb}, stream);
    return;
  }
  // every split-K block runs the fp32 epilogue: a bias would be added and
  // the ReLU applied once per split, on partial sums
  if (sk.zblocks > 1 && (bias != nullptr || relu))
    throw std::runtime_error(
        "gemm: split-K cannot fuse bias or ReLU; finish with bias_act_cast");
  if (!trans_a && !trans_b) {
    if (use_w8(M, N)) {
      if (store_mode == 0)      COS_GEMM_CASE8(0);
      else if (store_mode == 1) COS_GEMM_CASE8(1);
      else if (store_mode == 3) COS_GEMM_CASE8(3);
      else                      COS_GEMM_CASE8(2);
      return;
    }
    COS_GEMM_SM(false, false);
  }
  else if (!trans_a && trans_b)  COS_GEMM_SM(false, true);
  else if (trans_a && !trans_b)  COS_GEMM_SM(true, false);
  else                           COS_GEMM_SM(true, true);
#undef COS_GEMM_SM
#undef COS_GEMM_CASE
#undef COS_GEMM_CASE8
}

static CGeom make_geom(const int* g) {
  // g = [H, W, C, P, Q, sh, sw, ph, pw, dil, S, c0, Cg, Kcol]
  CGeom gm;
  gm.H = g[0]; gm.W = g[1]; gm.C = g[2];
  gm.Q = g[4]; gm.PQ = g[3] * g[4];
  gm.sh = g[5]; gm.sw = g[6]; gm.ph = g[7]; gm.pw = g[8];
  gm.dil = g[9]; gm.S = g[10];
  gm.c0 = g[11]; gm.Cg = g[12]; gm.Kcol = g[13];
  gm.mPQ = magic40(gm.PQ);
  gm.mQ = magic40(gm.Q);
  gm.mCg = magic40(gm.Cg);
  gm.mS = magic40(gm.S);
  return gm;
}

// Every instantiation of gemm_conv_fwd_kernel: CFG_(id, TBM, TBN, WM, WN,
// DEPTH).  The ids are what gemm_conv_fwd's cfg argument and
// tools/conv_tile_bench.py name; 0-2 are the fixed 128-wide kernels
// <8,4>, <8,2> and <4,2>.  Ids 12-17 lost the sweep everywhere
// (profiles/alexnet_1gpu_conv_tiles.md); they are compiled only with
// -DCOS_CONV_SWEEP, to repeat it.
#ifdef COS_CONV_SWEEP
#define COS_CONV_SWEEP_CFGS(CFG_)                                           \
  CFG_(12, 128, 96, 4, 2, 4)  CFG_(13, 256, 96, 4, 2, 2)                    \
  CFG_(14, 256, 64, 4, 1, 2)  CFG_(15, 256, 48, 4, 1, 2)                    \
  CFG_(16, 128, 96, 2, 2, 4)  CFG_(17, 128, 64, 2, 2, 4)
#else
#define COS_CONV_SWEEP_CFGS(CFG_)
#endif
#define COS_CONV_CFGS(CFG_)                                                 \
  CFG_(0, 128, 128, 4, 2, 4)  CFG_(1, 128, 128, 4, 2, 2)                    \
  CFG_(2, 128, 128, 2, 2, 2)  CFG_(3, 128, 96, 2, 2, 2)                     \
  CFG_(4, 128, 96, 4, 2, 2)   CFG_(5, 128, 64, 2, 2, 2)                     \
  CFG_(6, 128, 64, 4, 2, 2)   CFG_(7, 128, 64, 4, 2, 4)                     \
  CFG_(8, 256, 64, 4, 2, 2)   CFG_(9, 128, 48, 4, 1, 2)                     \
  CFG_(10, 128, 48, 4, 1, 4)  CFG_(11, 256, 48, 8, 1, 2)                    \
  COS_CONV_SWEEP_CFGS(CFG_)

struct ConvCfg { int id, bm, bn, waves, depth; };

static const ConvCfg kConvCfgs[] = {
#define CFG_(ID, TBM, TBN, WM, WN, DEPTH) {ID, TBM, TBN, WM * WN, DEPTH},
    COS_CONV_CFGS(CFG_)
#undef CFG_
};
constexpr int kNumConvCfgs = sizeof(kConvCfgs) / sizeof(kConvCfgs[0]);

// Which instantiations take the 16-byte epilogue when the operands allow
// it.  Measured per tile and shape against the element-wise one ("The
// 16-byte epilogue" in the same profile) it was 1-22 % faster for every
// tile at every shape, so none is excluded; a tile that loses gets its
// id listed here.
static bool conv_vec(int id) {
  (void)id;
  return true;
}

int conv_fwd_num_cfgs() { return kNumConvCfgs; }
ConvCfg conv_fwd_cfg(int id) {
  if (id < 0 || id >= kNumConvCfgs)
    throw std::runtime_error("conv_fwd_cfg: no such configuration");
  return kConvCfgs[id];
}

// N tile with the least padding, ceil(N/BN)*BN minimal, the wider on a
// tie; COS_CONV_BN = 48/64/96/128 forces one (0 or unset: automatic).
static int conv_bn(int N) {
  // read per call, unlike COS_CONVQ: conv2d_forward/backward take no tile
  // argument, and the tests flip the width under them inside one process
  const char* e = getenv("COS_CONV_BN");
  int forced = e ? atoi(e) : 0;
  if (forced != 0 && forced != 48 && forced != 64 && forced != 96 &&
      forced != 128)
    throw std::runtime_error("COS_CONV_BN must be 0, 48, 64, 96 or 128");
  if (forced) return forced;
  int best = 128, best_pad = (N + 127) / 128 * 128;
  for (int bn : {96, 64, 48}) {
    int pad = (N + bn - 1) / bn * bn;
    if (pad < best_pad) { best = bn; best_pad = pad; }
  }
  return best;
}

// The configuration gemm_conv_fwd runs [M, N, K] with (N per group).
// BN = 128 is the fixed-tile rule: 8 waves for skinny shapes (use_w8),
// the one-barrier depth-4 ring inside the COS_CONVQ K gate.
ConvCfg conv_fwd_plan(int M, int N, int K) {
  static const int quad = [] {
    // COS_CONVQ: 0 = off, otherwise a max-K gate (1 = "all shapes").
    // Default 1152: same-box A/B is +2.2% CIFAR, neutral AlexNet/
    // GoogLeNet/LRCN; ungated it was -3% AlexNet (long-K shapes).
    const char* e = getenv("COS_CONVQ");
    if (!e) return 1152;
    int v = atoi(e);
    return v == 1 ? 1 << 30 : v;
  }();
  bool w8 = use_w8(M, N);
  bool q = quad && K >= 4 * BK && K <= quad;
  // The narrow tiles follow the sweep in
  // profiles/alexnet_1gpu_conv_tiles.md: 32x48 wave tiles at depth 2 for
  // 96 columns (the depth-4 ring lost at K = 448 and 1152), 256-row
  // blocks for 64 and 48 columns once M is large enough to fill the chip
  // with them.  Small M was not swept; it keeps 128 rows and, for 64 and
  // 48 columns, the fixed tile's depth rule (the COS_CONVQ gate).
  bool big_m = M >= 8192;
  int id;
  switch (conv_bn(N)) {
    case 96: id = w8 ? 4 : 3; break;
    case 64: id = big_m ? 8 : w8 ? (q ? 7 : 6) : 5; break;
    case 48: id = big_m ? 11 : q ? 10 : 9; break;
    default: id = w8 ? (q ? 0 : 1) : 2; break;
  }
  return kConvCfgs[id];
}

// groups > 1 runs a grouped convolution in one launch; see the kernel
// for the three strides.  cfg >= 0 forces an instantiation (the sweep).
// vec: 0 element-wise epilogue, 1 the 16-byte one where the operands
// allow it, -1 automatic (conv_vec).
void gemm_conv_fwd(const void* X, const void* B, void* C,
                   const float* bias, const void* zpage, int M, int N,
                   int K, int ldb, int ldc, bool relu, bool accum,
                   const int* geom, int groups, int gs_c, int gs_b,
                   int gs_n, int cfg, int vec, hipStream_t stream) {
  CGeom gm = make_geom(geom);
  if (K % BK != 0 || K < 2 * BK)
    throw std::runtime_error("gemm_conv_fwd: K must be whole 32-wide tiles, "
                             "at least two");
  if (cfg >= kNumConvCfgs)
    throw std::runtime_error("gemm_conv_fwd: no such configuration");
  ConvCfg p = cfg >= 0 ? kConvCfgs[cfg] : conv_fwd_plan(M, N, K);
  int mblocks = (M + p.bm - 1) / p.bm, nblocks = (N + p.bn - 1) / p.bn;
  dim3 grid(mblocks * nblocks, max(1, groups));
  // the 16-byte epilogue needs whole, aligned 8-channel runs
  bool vec_ok = ((N | ldc | (groups > 1 ? gs_n : 0)) % 8 == 0) &&
                (((uintptr_t)C | (uintptr_t)bias) % 16 == 0);
  int use_vec = vec_ok && (vec < 0 ? conv_vec(p.id) : vec != 0);
  switch (p.id) {
#define CFG_(ID, TBM, TBN, WM, WN, DEPTH)                                   \
    case ID:                                                                \
      gemm_conv_fwd_kernel<TileCfg<TBM, TBN, WM, WN>, DEPTH>                \
          <<<grid, WM * WN * 64, 0, stream>>>(                              \
              (const bf16*)X, (const bf16*)B, (bf16*)C, bias,               \
              (const bf16*)zpage, M, N, K, ldb, ldc, relu ? 1 : 0,          \
              accum ? 1 : 0, gm, gs_c, gs_b, gs_n, use_vec);                \
      break;
    COS_CONV_CFGS(CFG_)
#undef CFG_
  }
}

void gemm_conv_fwd_sc(const void* X, const void* B, void* C,
                      const float* bias, int M, int N, int K, int ldb,
                      int ldc, bool relu, const int* geom,
                      hipStream_t stream) {
  CGeom gm = make_geom(geom);
  int mblocks = (M + BM - 1) / BM, nblocks = (N + BN - 1) / BN;
  dim3 grid(mblocks * nblocks);
  if (use_w8(M, N))
    gemm_conv_fwd_sc_kernel<8><<<grid, dim3(512), 0, stream>>>(
        (const bf16*)X, (const bf16*)B, (bf16*)C, bias, M, N, K, ldb,
        ldc, relu ? 1 : 0, gm);
  else
    gemm_conv_fwd_sc_kernel<4><<<grid, dim3(256), 0, stream>>>(
        (const bf16*)X, (const bf16*)B, (bf16*)C, bias, M, N, K, ldb,
        ldc, relu ? 1 : 0, gm);
}

void gemm_conv_dw_sc(const void* A, const void* X, float* C, int M,
                     int N, int K, int lda, int ldc, int store_mode,
                     int splitk, float alpha, float* db, const int* geom,
                     hipStream_t stream) {
  launch_wide_tt((const bf16*)A, C, M, N, K, lda, ldc, store_mode,
                 split_k(K, splitk), alpha, db,
                 BImplicitSC{(const bf16*)X, make_geom(geom)}, stream);
}

// The DMA-staged kernel needs every 16-byte source chunk aligned and
// wholly inside or outside its operand; anything else, and a fused db,
// runs the register-staged kernel.  COS_DW_TR=0 forces the latter (A/B).
void gemm_conv_dw(const void* A, const void* X, float* C,
                  const void* zpage, int M, int N, int K, int lda, int ldc,
                  int store_mode, int splitk, float alpha, float* db,
                  const int* geom, hipStream_t stream) {
  // read per call, not cached: the tests flip it inside one process
  const char* tr_e = getenv("COS_DW_TR");
  bool tr_env = !(tr_e && tr_e[0] == '0');
  CGeom gm = make_geom(geom);
  SplitK sk = split_k(K, splitk);
  bool tr = tr_env && db == nullptr && zpage != nullptr &&
            ((M | lda | gm.C | gm.c0 | gm.Cg | gm.Kcol) % 8 == 0) &&
            (((uintptr_t)A | (uintptr_t)X) % 16 == 0);
  if (!tr) {
    launch_wide_tt((const bf16*)A, C, M, N, K, lda, ldc, store_mode, sk,
                   alpha, db, BImplicit{(const bf16*)X, gm}, stream);
    return;
  }
  int mblocks = (M + BM - 1) / BM, nblocks = (N + WBN - 1) / WBN;
  dim3 grid(mblocks * nblocks, sk.zblocks);
  if (store_mode == 1 && sk.zblocks == 1)
    gemm_conv_dw_tr_kernel<1, DW_TR_DEPTH><<<grid, WNT, 0, stream>>>(
        (const bf16*)A, (const bf16*)X, (const bf16*)zpage, C, M, N, K, lda,
        ldc, sk.ksplit, alpha, gm);
  else
    gemm_conv_dw_tr_kernel<2, DW_TR_DEPTH><<<grid, WNT, 0, stream>>>(
        (const bf16*)A, (const bf16*)X, (const bf16*)zpage, C, M, N, K, lda,
        ldc, sk.ksplit, alpha, gm);
}

void gemm_bf16(const void* A_, const void* B_, void* C, const float* bias,
               int M, int N, int K, int lda, int ldb, int ldc,
               bool trans_a, bool trans_b, int store_mode, int splitk,
               bool relu, float alpha, int m_alloc, int n_alloc,
               hipStream_t stream) {
  gemm_bf16_batched(A_, B_, C, bias, M, N, K, lda, ldb, ldc, trans_a,
                    trans_b, store_mode, splitk, relu, alpha, m_alloc,
                    n_alloc, 1, 0, 0, 0, stream);
}

// ------------------------------------- weight-streaming InnerProduct GEMM
// C[M,N] = A[M,K] @ B' for skinny activations (M <= 256): the forward pass
// (B = W stored [N][K], TRB false) and the data gradient (B = W stored
// [K][N], N contiguous, TRB true) of an InnerProduct layer.  These GEMMs
// are bound by the bytes of W, so:
//   - one block covers all of M (TBM = 256, or 128 when M <= 128): every
//     weight byte is fetched by exactly one block, once;
//   - both operands are staged by direct-to-LDS DMA into a DEPTH-stage ring
//     (DEPTH - 1 tiles, 72 KB at depth 4, in flight per CU), with the
//     counted-vmcnt loop of gemm_conv_dw_tr_kernel: every DMA always
//     issues — rows beyond M or N, k beyond the split's end and the tiles
//     prefetched past it fetch the zero page — so the count is exact for
//     any tile count >= 1 and edges need no padded copies.  K % 8 == 0
//     keeps every 16-byte chunk wholly inside or outside its operand;
//   - TRB stages W as it lies, [32 k][128 col] in gemm_conv_dw_tr_kernel's
//     swizzled image, and reads fragments with ds_read_b64_tr_b16: no
//     transposed copy of W exists;
//   - split-K writes slabs, not atomics: split s stores its fp32 partial
//     tile with plain 16-byte stores into slab s of a [sk][M][N] workspace,
//     every element of every slab; fc_slab_finalize (elementwise.hip) sums
//     them in ascending s, so the result is the same bits on every run.
//     A single split stores bf16 directly with bias and ReLU fused.
// LDS image of a stage: A, [TBM][32] canonical (swz_chunk), then B, 8 KB:
// canonical [128][32] or the transposed [32][128] image.  All LDS reads are
// inline assembly for the reason given at ds_read_tr16.

constexpr int FC_BN = 128;
constexpr int FC_DEPTH = 4;

struct FcPlan { int route, bm, bn, depth, sk; };

__device__ __forceinline__ bf16x8 ds_read_b128_asm(unsigned addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}

template <int TBM, bool TRB, int DEPTH>
__global__ __launch_bounds__(512, 1) void gemm_fc_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    const bf16* __restrict__ zpage, bf16* __restrict__ Cb,
    float* __restrict__ Cs, const float* __restrict__ bias, int M, int N,
    int K, int lda, int ldb, int ldc, int ksplit, int relu, int vec) {
  constexpr int WM = TBM / 64, WN = 8 / WM;      // 4x2 or 2x4 waves
  using Cfg = TileCfg<TBM, FC_BN, WM, WN>;       // 64 x (64 | 32) per wave
  constexpr int MF = Cfg::MF, NF = Cfg::NF, NCOLS = Cfg::NCOLS;
  constexpr int A_BYTES = TBM * BK * 2, B_BYTES = FC_BN * BK * 2;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int A_CPW = Cfg::A_CPW;              // 1 KB A chunks per wave
  static_assert(MF == 4 && Cfg::B_CHUNKS == 8, "one B chunk per wave");
  static_assert(DEPTH * STAGE >= vec_slab_floats<Cfg>() * 4 &&
                DEPTH * STAGE >= 8 * f32_slab_floats<NCOLS>() * 4,
                "the epilogue slabs fit in the ring");
  __shared__ __attribute__((aligned(16))) unsigned char smem[DEPTH * STAGE];

  int tile_n = blockIdx.x * FC_BN;
  int k_begin = blockIdx.y * ksplit;
  int k_end = min(K, k_begin + ksplit);

  int tid = threadIdx.x;
  int wave = tid >> 6, lane = tid & 63;
  int wm = wave / WN, wn = wave % WN;

  // ---- staging, fixed per lane but for the K tile.  A chunk c holds rows
  // 16c..16c+15; lane l fills chunk position (row l/4, l%4) and so fetches
  // the source chunk the swizzle maps there (stage_direct_fast).
  const unsigned short* as = reinterpret_cast<const unsigned short*>(A);
  const unsigned short* bs = reinterpret_cast<const unsigned short*>(B);
  int64_t a_off[A_CPW];
  int a_kk[A_CPW];
  bool a_ok[A_CPW];
#pragma unroll
  for (int it = 0; it < A_CPW; ++it) {
    int row = (wave * A_CPW + it) * 16 + (lane >> 2);
    a_kk[it] = swz_chunk(row, lane & 3) << 3;
    a_ok[it] = row < M;
    a_off[it] = (int64_t)row * lda + a_kk[it];
  }
  int64_t b_off;
  int b_kk;
  bool b_ok;
  if (TRB) {
    // wave w fills k-rows 4w..4w+3 of the [32][128] image
    int srow = wave * 4 + (lane >> 4);
    int sch = (dw_tr_off(srow, lane & 15) >> 4) & 15;
    int col = tile_n + sch * 8;                  // N % 8 == 0: whole octets
    b_kk = srow;
    b_ok = col < N;
    b_off = (int64_t)srow * ldb + col;
  } else {
    int row = wave * 16 + (lane >> 2);
    b_kk = swz_chunk(row, lane & 3) << 3;
    b_ok = tile_n + row < N;
    b_off = (int64_t)(tile_n + row) * ldb + b_kk;
  }
  typedef const __attribute__((address_space(1))) unsigned int* gptr;
  typedef __attribute__((address_space(3))) unsigned int* lptr;
  // branch-free select, as in gemm_conv_dw_tr_kernel: one DMA per chunk
  // with EXEC all ones, whatever the guards say
  auto keep_v = [](int64_t v) {
    asm volatile("" : "+v"(v));
    return v;
  };
  auto stage = [&](int slot, int k0) {
    unsigned char* base = smem + slot * STAGE;
#pragma unroll
    for (int it = 0; it < A_CPW; ++it) {
      bool ok = a_ok[it] & (k0 + a_kk[it] < k_end);
      int64_t off = keep_v(a_off[it] + k0);
      const void* src = ok ? (const void*)(as + off) : (const void*)zpage;
      __builtin_amdgcn_global_load_lds(
          (gptr)src, (lptr)(base + (wave * A_CPW + it) * 1024), 16, 0, 0);
    }
    bool ok = b_ok & (k0 + b_kk < k_end);
    int64_t off = keep_v(b_off + (TRB ? (int64_t)k0 * ldb : (int64_t)k0));
    const void* src = ok ? (const void*)(bs + off) : (const void*)zpage;
    __builtin_amdgcn_global_load_lds(
        (gptr)src, (lptr)(base + A_BYTES + wave * 1024), 16, 0, 0);
  };

  // ---- fragment read addresses inside a stage (fixed per lane)
  int lrow = lane & 15, lchunk = lane >> 4;
  int a_addr[MF], b_addr[NF][2];
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    int ra = wm * 64 + f * 16 + lrow;
    a_addr[f] = ra * 64 + (swz_chunk(ra, lchunk) << 4);
  }
  if (TRB) {
    // group g = lane>>4 reads k-rows 8g+4h+q; lane 4q+p of the group
    // supplies columns 4p..4p+3 of fragment f's 16 columns
    int fq = (lane >> 2) & 3, fp = lane & 3;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        b_addr[f][h] = A_BYTES +
            dw_tr_off(8 * lchunk + 4 * h + fq,
                      (wn * NCOLS + f * 16) / 8 + (fp >> 1)) + 8 * (fp & 1);
  } else {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int rb = wn * NCOLS + f * 16 + lrow;
      b_addr[f][0] = b_addr[f][1] =
          A_BYTES + rb * 64 + (swz_chunk(rb, lchunk) << 4);
    }
  }
  unsigned lds0 = (unsigned)(uintptr_t)(
      (__attribute__((address_space(3))) unsigned char*)smem);

  f32x4 acc[MF][NF] = {};

  constexpr int PF = DEPTH - 1;              // tiles in flight ahead
  constexpr int VMCNT = (A_CPW + 1) * (PF - 1);
  int tiles = (k_end - k_begin + BK - 1) / BK;
#pragma unroll
  for (int p = 0; p < PF; ++p) stage(p, k_begin + p * BK);
  int cur = 0;                               // ring slot of tile i
  for (int i = 0; i < tiles; ++i) {
    wait_vmcnt<VMCNT>();                     // this wave's part of tile i
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();            // everyone's; tile i-1 is read
    int nxt = cur == 0 ? DEPTH - 1 : cur - 1;     // (i + PF) % DEPTH
    stage(nxt, k_begin + (i + PF) * BK);
    unsigned img = lds0 + cur * STAGE;
    bf16x8 afrag[MF], bfrag[NF];
    if (TRB) {
      bf16x4 br[NF][2];
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          br[f][h] = ds_read_tr16(img + b_addr[f][h]);
#pragma unroll
      for (int f = 0; f < MF; ++f) afrag[f] = ds_read_b128_asm(img + a_addr[f]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        asm volatile("" : "+v"(br[f][0]), "+v"(br[f][1]));
        bfrag[f] = __builtin_shufflevector(br[f][0], br[f][1], 0, 1, 2, 3, 4,
                                           5, 6, 7);
      }
    } else {
#pragma unroll
      for (int f = 0; f < NF; ++f)
        bfrag[f] = ds_read_b128_asm(img + b_addr[f][0]);
#pragma unroll
      for (int f = 0; f < MF; ++f) afrag[f] = ds_read_b128_asm(img + a_addr[f]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int f = 0; f < NF; ++f) asm volatile("" : "+v"(bfrag[f]));
    }
    // the reads have landed: tie every fragment behind the wait so that
    // no MFMA is scheduled above it
#pragma unroll
    for (int f = 0; f < MF; ++f) asm volatile("" : "+v"(afrag[f]));
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int fm = 0; fm < MF; ++fm)
#pragma unroll
      for (int fn = 0; fn < NF; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag[fm], bfrag[fn], acc[fm][fn], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    cur = cur + 1 == DEPTH ? 0 : cur + 1;
  }
  wait_vmcnt<0>();                           // the zero-page tail DMAs

  float* lds_f = reinterpret_cast<float*>(smem);
  if (Cs != nullptr) {
    // split s: plain stores into slab s, every element of it
    float* slab = Cs + (int64_t)blockIdx.y * M * N;
    if (vec) {
      __syncthreads();     // every wave's DMA has landed and its reads too
      epilogue_f32_vec<MF, NF, NCOLS>(
          acc, lds_f + wave * f32_slab_floats<NCOLS>(), slab, M, N, N,
          wm * 64, tile_n + wn * NCOLS, lane, 1.f);
    } else {
      int crow0 = wm * 64 + (lchunk << 2), ccol0 = tile_n + wn * NCOLS + lrow;
#pragma unroll
      for (int fm = 0; fm < MF; ++fm)
#pragma unroll
        for (int fn = 0; fn < NF; ++fn)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = crow0 + fm * 16 + r, col = ccol0 + fn * 16;
            if (row < M && col < N)
              slab[(int64_t)row * N + col] = acc[fm][fn][r];
          }
    }
  } else if (vec) {
    __syncthreads();
    epilogue_bf16_vec<Cfg>(acc, lds_f, Cb, bias, M, N, ldc, 0, tile_n, wm, wn,
                           wave, lane, relu, 0);
  } else {
    epilogue_bf16<MF, 64, NF, NCOLS>(acc, Cb, bias, M, N, ldc, 0, tile_n, wm,
                                     wn, lane, relu, 1.f, std::false_type{});
  }
}

// The plan for [M, N, K] of kind 0 (forward, W is [N][K]) or 1 (data
// gradient, W is [K][N]): route 1 = gemm_fc_kernel, 0 = the caller's
// legacy route.  `aligned`: A and B are 16-byte aligned with leading
// dimensions that are multiples of 8 (the caller's to check; the launcher
// checks again).  C may lie anyhow: only the 16-byte epilogue asks more.  COS_FC_STREAM=0 sends everything to the legacy route; it
// is read per call because the tests flip it inside one process.
// sk: about one block per CU in a single wave of blocks, every split at
// least 256 of K, at most 16 slabs.
FcPlan fc_gemm_plan(int M, int N, int K, int kind, bool aligned) {
  const char* e = getenv("COS_FC_STREAM");
  bool on = !(e && e[0] == '0');
  FcPlan p{0, 0, FC_BN, FC_DEPTH, 1};
  if (!on || !aligned || M < 1 || M > 256 || N < 1 || K < 8 || K % 8 != 0 ||
      (kind == 1 && N % 8 != 0) || (kind != 0 && kind != 1))
    return p;
  p.route = 1;
  p.bm = M <= 128 ? 128 : 256;
  int ntiles = (N + FC_BN - 1) / FC_BN;
  p.sk = hmax(1, hmin(hmin(K / 256, 256 / ntiles), 16));
  return p;
}

// sk <= 0: the plan's.  sk == 1 stores bf16 into C (bias, ReLU fused);
// sk > 1 fills `slabs` ([zblocks][M][N] fp32, at least sk of them) and
// returns the number of slabs written (the K tiles may divide into fewer
// than sk), for fc_slab_finalize to sum.
int gemm_fc(const void* A, const void* B, void* C, float* slabs,
            const float* bias, const void* zpage, int M, int N, int K,
            int lda, int ldb, int ldc, int kind, int sk, bool relu,
            hipStream_t stream) {
  bool aligned = (((uintptr_t)A | (uintptr_t)B | (uintptr_t)zpage) % 16 ==
                  0) && ((lda | ldb) % 8 == 0);
  FcPlan p = fc_gemm_plan(M, N, K, kind, aligned);
  if (!p.route || zpage == nullptr || lda < K || ldc < N ||
      ldb < (kind == 1 ? N : K))
    throw std::runtime_error("gemm_fc: shape or alignment outside the "
                             "streaming kernel (see fc_gemm_plan)");
  SplitK s = split_k(K, sk > 0 ? sk : p.sk);
  if (s.zblocks > 1 && slabs == nullptr)
    throw std::runtime_error("gemm_fc: split-K needs the slab workspace");
  float* cs = s.zblocks > 1 ? slabs : nullptr;
  int vec = cs != nullptr
                ? (N % 4 == 0 && (uintptr_t)cs % 16 == 0)
                : ((N | ldc) % 8 == 0 && (uintptr_t)C % 16 == 0 &&
                   (bias == nullptr || (uintptr_t)bias % 16 == 0));
  dim3 grid((N + FC_BN - 1) / FC_BN, s.zblocks);
#define COS_FC_CASE(TBM, TRB)                                               \
  gemm_fc_kernel<TBM, TRB, FC_DEPTH><<<grid, 512, 0, stream>>>(             \
      (const bf16*)A, (const bf16*)B, (const bf16*)zpage, (bf16*)C, cs,     \
      bias, M, N, K, lda, ldb, ldc, s.ksplit, relu ? 1 : 0, vec)
  if (p.bm == 128) {
    if (kind == 1) COS_FC_CASE(128, true); else COS_FC_CASE(128, false);
  } else {
    if (kind == 1) COS_FC_CASE(256, true); else COS_FC_CASE(256, false);
  }
#undef COS_FC_CASE
  return s.zblocks;
}

}  // namespace cosamd
