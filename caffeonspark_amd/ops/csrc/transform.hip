// Device-side DataTransformer: crop / mirror / mean / scale for a whole
// batch of raw uint8 images in one launch.
//
//   out[n][c][h][w] = (float(src_n[c][h_off+h][w_off + (mirror ? ow-1-w : w)])
//                      - mean) * scale
//
// src holds the raw bytes of all N images back to back, each either
// planar (CHW, raw Datum) or channel-minor (HWC, decoded image); a table
// row per image gives its byte offset, size, layout and the drawn crop /
// mirror parameters, so images of one batch may differ in all of them.
// The arithmetic is one fp32 subtract and one fp32 multiply (skipped when
// scale == 1), exactly the host transformer's, so the result is
// bit-identical to it; bf16 output rounds to nearest even.
//
// One block handles an [RT rows][WT columns] chunk of one image's crop.
// It first copies the source bytes of the chunk into LDS run by run (a
// run is one source row of the chunk: WT bytes per (c, row) of a planar
// image, WT*C bytes per row of a channel-minor one) with unaligned
// 16-byte loads and guarded byte loads at run tails, then walks the
// output in its own memory order, 8 elements per work item, gathering
// the bytes from LDS (which absorbs both the layout change and the
// mirror) and storing 16 bytes at a time where the output run is
// contiguous and aligned.  All offsets inside one image are 32-bit; the
// host checks that they fit.

#include "common.h"

#include <stdexcept>
#include <string>

namespace cosamd {

namespace {

typedef unsigned short xf_u16;
typedef unsigned char xf_u8;

constexpr int kXfTile = 16384;        // LDS byte tile
constexpr int kXfThreads = 256;
constexpr int kXfBlockElems = 8192;   // target output elements per block
constexpr int kXfCols = 7;            // table columns

struct XfArgs {
  const xf_u8* src;
  int64_t src_bytes;
  const int64_t* table;
  const float* mean;
  void* out;
  int64_t osN;
  float scale;
  int mean_mode;
  int C, oh, ow;
  int osC, osH, osW;
  int RT, WT, nhc, nwc;
};

template <typename T> struct XfOut;
template <> struct XfOut<float> {
  static __device__ __forceinline__ float cvt(float v) { return v; }
};
template <> struct XfOut<xf_u16> {
  static __device__ __forceinline__ xf_u16 cvt(float v) {
    bf16 h = f2bf(v);
    xf_u16 b;
    __builtin_memcpy(&b, &h, 2);
    return b;
  }
};

template <typename OutT>
__global__ __launch_bounds__(kXfThreads) void data_transform_kernel(
    XfArgs a) {
  __shared__ __attribute__((aligned(16))) xf_u8 tile[kXfTile];
  constexpr int kVec = 16 / (int)sizeof(OutT);   // elements per 16-byte store
  typedef OutT vec_t __attribute__((ext_vector_type(kVec)));
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

  const int C = a.C, oh = a.oh, ow = a.ow;
  int b = blockIdx.x;
  int wc = b % a.nwc;
  int t = b / a.nwc;
  int hc = t % a.nhc;
  int n = t / a.nhc;

  const int64_t* row = a.table + (int64_t)n * kXfCols;
  int64_t boff = row[0], H64 = row[1], W64 = row[2];
  int64_t hoff64 = row[4], woff64 = row[5];
  bool planar = row[3] != 0, mirror = row[6] != 0;
  // the host validates the same table before the launch; a row that does
  // not describe a crop inside its image inside src is skipped whole
  if (H64 <= 0 || W64 <= 0 || (int64_t)C * H64 * W64 >= (1ll << 31) ||
      boff < 0 || boff + (int64_t)C * H64 * W64 > a.src_bytes ||
      hoff64 < 0 || hoff64 + oh > H64 || woff64 < 0 || woff64 + ow > W64)
    return;
  const int H = (int)H64, W = (int)W64;
  const int h0 = hc * a.RT, w0 = wc * a.WT;
  const int rt = min(a.RT, oh - h0), wt = min(a.WT, ow - w0);
  const int hs0 = (int)hoff64 + h0;
  // source columns behind output columns [w0, w0+wt)
  const int ws0 = (int)woff64 + (mirror ? ow - w0 - wt : w0);
  const xf_u8* img = a.src + boff;

  // ---- source bytes -> LDS, one 16-byte group per work item ------------
  const int nruns = planar ? C * rt : rt;
  const int runlen = planar ? wt : wt * C;
  const int rstride = (runlen + 15) & ~15;
  const int ngrp = rstride >> 4;
  for (int it = threadIdx.x; it < nruns * ngrp; it += kXfThreads) {
    int run = it / ngrp;
    int j0 = (it - run * ngrp) << 4;
    int soff;
    if (planar) {
      int c = run / rt, r = run - c * rt;
      soff = (c * H + hs0 + r) * W + ws0;
    } else {
      soff = ((hs0 + run) * W + ws0) * C;
    }
    const xf_u8* p = img + soff + j0;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (j0 + 16 <= runlen) {
      __builtin_memcpy(&v, p, 16);
    } else {
      int left = runlen - j0;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < left) v[j >> 2] |= (unsigned)p[j] << ((j & 3) * 8);
    }
    *reinterpret_cast<u32x4*>(tile + run * rstride + j0) = v;
  }
  __syncthreads();

  // ---- LDS -> transformed output ---------------------------------------
  const int lC = planar ? rt * rstride : 1;
  const int lW = planar ? 1 : C;
  const int mode = a.mean_mode;
  const float scale = a.scale;
  const bool do_scale = scale != 1.0f;
  const float* mean = a.mean;
  OutT* oimg = reinterpret_cast<OutT*>(a.out) + (int64_t)n * a.osN;

  // one element: channel c, chunk row r, chunk column wl
  auto xform = [&](int c, int r, int wl) -> OutT {
    int wsl = mirror ? wt - 1 - wl : wl;
    float v = (float)tile[c * lC + r * rstride + wsl * lW];
    if (mode == 1) v = v - mean[c];
    else if (mode == 2) v = v - mean[(c * H + hs0 + r) * W + ws0 + wsl];
    if (do_scale) v = v * scale;
    return XfOut<OutT>::cvt(v);
  };

  if (a.osC == 1 && C > 1) {
    // channel-minor output: (w, c) is one run per output row
    const int run = wt * C;
    const int ngo = (run + 7) >> 3;
    const bool dense = a.osW == C;
    for (int it = threadIdx.x; it < rt * ngo; it += kXfThreads) {
      int r = it / ngo;
      int j0 = (it - r * ngo) << 3;
      int wl0 = j0 / C, c0 = j0 - wl0 * C;
      int rowoff = (h0 + r) * a.osH;
      OutT* p = oimg + rowoff + w0 * a.osW + j0;   // valid when dense
      if (dense && j0 + 8 <= run &&
          (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        vec_t o[8 / kVec];
        int wl = wl0, c = c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          o[j / kVec][j % kVec] = xform(c, r, wl);
          if (++c == C) { c = 0; ++wl; }
        }
#pragma unroll
        for (int k = 0; k < 8 / kVec; ++k)
          reinterpret_cast<vec_t*>(p)[k] = o[k];
      } else {
        int wl = wl0, c = c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (wl < wt)
            oimg[rowoff + (w0 + wl) * a.osW + c] = xform(c, r, wl);
          if (++c == C) { c = 0; ++wl; }
        }
      }
    }
  } else {
    // planar (or generic strided) output: each (c, row) pair is one run
    const int ngo = (wt + 7) >> 3;
    const bool dense = a.osW == 1;
    for (int it = threadIdx.x; it < C * rt * ngo; it += kXfThreads) {
      int pair = it / ngo;
      int wl0 = (it - pair * ngo) << 3;
      int c = pair / rt, r = pair - c * rt;
      int rowoff = c * a.osC + (h0 + r) * a.osH;
      OutT* p = oimg + rowoff + w0 + wl0;          // valid when dense
      if (dense && wl0 + 8 <= wt &&
          (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        vec_t o[8 / kVec];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j / kVec][j % kVec] = xform(c, r, wl0 + j);
#pragma unroll
        for (int k = 0; k < 8 / kVec; ++k)
          reinterpret_cast<vec_t*>(p)[k] = o[k];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int wl = wl0 + j;
          if (wl < wt)
            oimg[rowoff + (w0 + wl) * a.osW] = xform(c, r, wl);
        }
      }
    }
  }
}

[[noreturn]] void xf_fail(const std::string& what) {
  throw std::runtime_error("data_transform: " + what);
}

}  // namespace

// table is the device copy the kernel reads, table_host the same rows on
// the host: every row is validated here, before the launch, so the kernel
// never reads outside src or mean nor writes outside out.
void data_transform(const void* src, int64_t src_bytes, const int64_t* table,
                    const int64_t* table_host, int N, const float* mean,
                    int mean_mode, int64_t mean_numel, int mC, int mH,
                    int mW, float scale, void* out, bool out_bf16, int C,
                    int oh, int ow, int64_t osN, int64_t osC, int64_t osH,
                    int64_t osW, hipStream_t stream) {
  if (N == 0) return;
  if (N < 0 || C < 1 || oh < 1 || ow < 1) xf_fail("bad output shape");
  if (C * 16 > kXfTile) xf_fail("too many channels");
  if (mean_mode < 0 || mean_mode > 2) xf_fail("mean_mode must be 0, 1 or 2");
  if (mean_mode == 1 && mean_numel != C)
    xf_fail("per-channel mean must have C values");
  if (mean_mode == 2 && (mC != C || mean_numel != (int64_t)mC * mH * mW))
    xf_fail("mean image must be [C,H,W]");
  if (osN < 0 || osC < 0 || osH < 0 || osW < 0 ||
      (C - 1) * osC + (oh - 1) * osH + (ow - 1) * osW >= (1ll << 31))
    xf_fail("output strides out of range");
  for (int n = 0; n < N; ++n) {
    const int64_t* r = table_host + (int64_t)n * kXfCols;
    int64_t off = r[0], H = r[1], W = r[2];
    std::string at = " (image " + std::to_string(n) + ")";
    if (H <= 0 || W <= 0 || H >= (1ll << 31) || W >= (1ll << 31) ||
        C * H * W >= (1ll << 31))
      xf_fail("bad image size" + at);
    if (off < 0 || off + C * H * W > src_bytes)
      xf_fail("image bytes outside src" + at);
    if ((r[3] != 0 && r[3] != 1) || (r[6] != 0 && r[6] != 1))
      xf_fail("planar and mirror must be 0 or 1" + at);
    if (r[4] < 0 || r[4] + oh > H || r[5] < 0 || r[5] + ow > W)
      xf_fail("crop outside the image" + at);
    if (mean_mode == 2 && (H != mH || W != mW))
      xf_fail("mean image shape differs from the image's" + at);
  }

  int wt_max = ((kXfTile / C) / 16) * 16;
  int WT = (int)hmin<int64_t>(ow, wt_max);
  int rowb = C * ((WT + 15) & ~15);           // LDS bytes per chunk row
  int RT = hmin(kXfTile / rowb, hmax(1, kXfBlockElems / (C * WT)));
  RT = hmax(1, hmin(RT, oh));
  int nhc = (oh + RT - 1) / RT, nwc = (ow + WT - 1) / WT;
  int64_t blocks = (int64_t)N * nhc * nwc;
  if (blocks >= (1ll << 31)) xf_fail("grid too large");

  XfArgs a;
  a.src = reinterpret_cast<const xf_u8*>(src);
  a.src_bytes = src_bytes;
  a.table = table;
  a.mean = mean;
  a.out = out;
  a.osN = osN;
  a.scale = scale;
  a.mean_mode = mean_mode;
  a.C = C; a.oh = oh; a.ow = ow;
  a.osC = (int)osC; a.osH = (int)osH; a.osW = (int)osW;
  a.RT = RT; a.WT = WT; a.nhc = nhc; a.nwc = nwc;
  if (out_bf16)
    data_transform_kernel<xf_u16>
        <<<(unsigned)blocks, kXfThreads, 0, stream>>>(a);
  else
    data_transform_kernel<float>
        <<<(unsigned)blocks, kXfThreads, 0, stream>>>(a);
}

}  // namespace cosamd
