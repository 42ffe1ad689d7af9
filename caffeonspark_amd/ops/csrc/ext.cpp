// Torch-facing bindings for the gfx950 kernel library.  Shape logic lives in
// Python (ops/gpu.py); this layer validates tensors and launches kernels on
// the current HIP stream.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace cosamd {

void gemm_bf16(const void* A, const void* B, void* C, const float* bias,
               int M, int N, int K, int lda, int ldb, int ldc,
               bool trans_a, bool trans_b, int store_mode, int splitk,
               bool relu, float alpha, int m_alloc, int n_alloc,
               hipStream_t stream);
struct FcPlan { int route, bm, bn, depth, sk; };
FcPlan fc_gemm_plan(int M, int N, int K, int kind, bool aligned);
int gemm_fc(const void* A, const void* B, void* C, float* slabs,
            const float* bias, const void* zpage, int M, int N, int K,
            int lda, int ldb, int ldc, int kind, int sk, bool relu,
            hipStream_t stream);
void fc_slab_finalize(const float* slabs, int sk, const float* bias,
                      void* out, int M, int N, int ldo, bool relu,
                      hipStream_t stream);
void gemm_f32(const float* A, const float* B, float* C, const float* bias,
              int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
              bool trans_a, bool trans_b, int splitk, bool relu,
              hipStream_t stream);
void im2col_f32(const float* x, float* col, int N, int H, int W, int P,
                int Q, int R, int S, int sh, int sw, int ph, int pw, int dh,
                int dw, int c0, int Cg, int64_t sN, int64_t sC, int64_t sH,
                int64_t sW, hipStream_t stream);
void col2im_f32(const float* dcol, float* dx, int N, int H, int W, int P,
                int Q, int R, int S, int sh, int sw, int ph, int pw, int dh,
                int dw, int c0, int Cg, int64_t sN, int64_t sC, int64_t sH,
                int64_t sW, hipStream_t stream);
void gemm_conv_fwd(const void* X, const void* B, void* C,
                   const float* bias, const void* zpage, int M, int N,
                   int K, int ldb, int ldc, bool relu, bool accum,
                   const int* geom, int groups, int gs_c, int gs_b,
                   int gs_n, int cfg, int vec, hipStream_t stream);
struct ConvCfg { int id, bm, bn, waves, depth; };
ConvCfg conv_fwd_plan(int M, int N, int K);
int conv_fwd_num_cfgs();
ConvCfg conv_fwd_cfg(int id);
void gemm_conv_dw(const void* A, const void* X, float* C,
                  const void* zpage, int M, int N, int K, int lda, int ldc,
                  int store_mode, int splitk, float alpha, float* db,
                  const int* geom, hipStream_t stream);
void gemm_conv_fwd_sc(const void* X, const void* B, void* C,
                      const float* bias, int M, int N, int K, int ldb,
                      int ldc, bool relu, const int* geom,
                      hipStream_t stream);
void gemm_conv_dw_sc(const void* A, const void* X, float* C, int M,
                     int N, int K, int lda, int ldc, int store_mode,
                     int splitk, float alpha, float* db, const int* geom,
                     hipStream_t stream);
void repack_weights(const int64_t* table, int ndesc, int64_t max_total,
                    hipStream_t stream);
void dw_unpack_acc(const float* dwp, float* arena, int Kout, int Cg,
                   int R, int S, int Kpad, bool accumulate,
                   hipStream_t stream);
void s2d_pack(const void* x, void* out, int N, int H, int W, int C, int st,
              int ph, int pw, int Hp, int Wp, int64_t sN, int64_t sC,
              int64_t sH, int64_t sW, hipStream_t stream);
void s2d_pack_weight(const void* src, void* dst, int Kout, int Cg, int R,
                     int S, int st, int Kpad, hipStream_t stream);
void d2s_pack_weight(const void* src, void* dst, int Ci, int Co, int R,
                     int S, int st, int Kpad, hipStream_t stream);
void d2s_unpack(const void* z, void* y, int N, int Co, int Ho, int Wo,
                int st, int ph, int pw, int Hp, int Wp, int64_t sN,
                int64_t sC, int64_t sH, int64_t sW, hipStream_t stream);
void data_transform(const void* src, int64_t src_bytes, const int64_t* table,
                    const int64_t* table_host, int N, const float* mean,
                    int mean_mode, int64_t mean_numel, int mC, int mH,
                    int mW, float scale, void* out, bool out_bf16, int C,
                    int oh, int ow, int64_t osN, int64_t osC, int64_t osH,
                    int64_t osW, hipStream_t stream);
void dw_unpack_s2d(const float* dwp, float* arena, int Kout, int Cg, int R,
                   int S, int st, int Kpad, bool accumulate,
                   hipStream_t stream);
int lstm_persist_fwd(const void* xg, const void* w_hc, const void* cont,
                     void* h, float* c, float* act, void* h_in, float* hg,
                     int T, int N, int H, void* bar, hipStream_t stream);
int lstm_persist_bwd(const void* dy, const void* w_hcT, const void* cont,
                     const void* h, const float* c, const float* act,
                     void* dxg, float* dh_acc, float* dc_a, float* dc_b,
                     int T, int N, int H, void* bar, hipStream_t stream);
void wino_conv(const void* x, const float* w, const float* bias, void* y,
               void* U, void* V, void* Mbuf, int N, int H, int W, int Cin,
               int K, int wK, int wC, int u_rows_alloc, bool flip,
               bool relu, hipStream_t stream);
void bn_stats(const void* x, float* sum, float* sumsq, int64_t rows, int C,
              hipStream_t stream);
void bn_bwd_sums(const void* dy, const void* xhat, float* s1, float* s2,
                 int64_t rows, int C, hipStream_t stream);
void bn_norm(const void* x, void* y, const float* mean, const float* invstd,
             int64_t rows, int C, hipStream_t stream);
void bn_bwd(const void* xhat, const void* dy, void* dx,
            const float* invstd, const float* s1, const float* s2,
            float inv_m, int64_t rows, int C, hipStream_t stream);
void im2col_t(const void* x, void* colT, int N, int H, int W, int C,
              int P, int Q, int R, int S, int sh, int sw, int ph, int pw,
              int dil, int Kpad, int c0, int Cg, hipStream_t stream);
void im2col_nhwc(const void* x, void* col, int N, int H, int W, int C,
                 int P, int Q, int R, int S, int sh, int sw, int ph, int pw,
                 int dil, int Kpad, int c0, int Ct, hipStream_t stream);
void col2im_nhwc(const void* dcol, void* dx, int N, int H, int W, int C,
                 int P, int Q, int R, int S, int sh, int sw, int ph, int pw,
                 int dil, int Kpad, int c0, int Ct, hipStream_t stream);
void maxpool_fwd(const void* x, void* y, void* idx, bool idx16, int N,
                 int H, int W, int C, int P, int Q, int kh, int kw, int sh,
                 int sw, int ph, int pw, hipStream_t stream);
void maxpool_bwd(const void* dy, const void* idx, bool idx16, void* dx,
                 int N, int H, int W, int C, int P, int Q, int kh, int kw,
                 int sh, int sw, int ph, int pw, hipStream_t stream);
void maxpool_bwd8_relu_db(const void* dy, const void* idx, const void* top,
                          void* dx, float* db, int N, int H, int W, int C,
                          int P, int Q, int kh, int kw, int sh, int sw,
                          int ph, int pw, int blocks, hipStream_t stream);
void avgpool_fwd(const void* x, void* y, int N, int H, int W, int C,
                 int P, int Q, int kh, int kw, int sh, int sw, int ph, int pw,
                 hipStream_t stream);
void avgpool_bwd(const void* dy, void* dx, int N, int H, int W, int C,
                 int P, int Q, int kh, int kw, int sh, int sw, int ph, int pw,
                 hipStream_t stream);
void lrn_fwd(const void* x, void* y, float* scale, int64_t npix, int C,
             int local_size, float alpha, float beta, float k,
             hipStream_t stream);
void lrn_bwd(const void* x, const void* y, const float* scale, const void* dy,
             void* dx, void* ratio, int64_t npix, int C, int local_size,
             float alpha, float beta, hipStream_t stream);
void relu_fwd(const void* x, void* y, float slope, int64_t n,
              hipStream_t stream);
void relu_bwd(const void* y, const void* dy, void* dx, float slope, int64_t n,
              hipStream_t stream);
void relu_bwd_strided(const void* y, const void* dy, void* dx, float slope,
                      int64_t rows, int C, int ldy, int lddy,
                      hipStream_t stream);
void relu_colsum_bwd(const void* y, const void* dy, void* dx, float* db,
                     float slope, int64_t rows, int cols, int ldy,
                     int lddy, hipStream_t stream);
void dropout_fwd(const void* x, void* y, void* mask, float ratio,
                 const void* seed, int64_t n, hipStream_t stream);
void seed_bump(void* s, hipStream_t stream);
void mul_bf16(const void* a, const void* b, void* y, int64_t n,
              hipStream_t stream);
void sgd_update(float* p, const float* g, float* v, float lr, float mu,
                float wd, int64_t n, hipStream_t stream);
void nesterov_update_multi(float* p, const float* g, float* v,
                           const int64_t* seg_off, const float* seg_lr,
                           const float* seg_wd, int nseg, float mu,
                           int64_t total, void* sh, hipStream_t stream);
void adam_update_multi(float* p, const float* g, float* m, float* v,
                       const int64_t* seg_off, const float* seg_lr,
                       const float* seg_wd, int nseg, float b1, float b2,
                       float eps, int64_t total, void* sh,
                       hipStream_t stream);
void sgd_update_multi(float* p, const float* g, float* v,
                      const int64_t* seg_off, const float* seg_lr,
                      const float* seg_wd, int nseg, float mu,
                      int64_t total, void* sh, hipStream_t stream);
void relu_db_dense(const void* y, const void* dy, void* dx, float* db,
                   float slope, int64_t rows, int C, int row_blocks,
                   hipStream_t stream);
void colsum(const void* in, float* out, int64_t rows, int cols, int ld,
            hipStream_t stream);
void transpose_bf16(const void* in, void* out, int64_t R, int64_t C,
                    hipStream_t stream);
void bias_act_cast(const float* in, const float* bias, void* out,
                   int64_t rows, int cols, bool relu, hipStream_t stream);
void lstm_unit_fwd(const float* c_prev, const void* gates, const void* cont,
                   float* c_out, void* h_out, float* act, int64_t n, int H,
                   hipStream_t stream);
void lstm_unit_bwd(const float* c_prev, const float* c_out, const float* act,
                   const void* cont, const float* dc_next, const void* dh,
                   float* dc_prev, void* dgates, int64_t n, int H,
                   hipStream_t stream);
void embed_fwd(const float* idx, const void* w, void* y, int64_t n, int E,
               int V, hipStream_t stream);
void embed_bwd(const float* idx, const void* dy, float* dw, int64_t n, int E,
               int V, hipStream_t stream);
void lstm_seq_fwd(const void* xg, const void* w_hc, const void* cont,
                  void* h, float* c, float* act, void* h_in, float* hg,
                  int T, int N, int H, int n_alloc_whc, hipStream_t stream);
void lstm_seq_bwd(const void* dy, const void* w_hcT, const void* cont,
                  const void* h, const float* c, const float* act,
                  void* dxg, void* dh_rec, float* dh_f, float* dc_a,
                  float* dc_b, int T, int N, int H, int n_alloc_whcT,
                  hipStream_t stream);
int64_t lstm_step_lds_bytes(int N, int D, int H, int Ds);
void lstm_step(const void* x, const void* h_prev, const void* xs,
               const void* w_xc, const void* w_hc, const void* w_xsc,
               const void* bias, const float* cont, const float* c_prev,
               float* c_out, void* h_out, int N, int D, int H, int Ds,
               hipStream_t stream);
void softmax_loss_fwd(const void* x, const float* label, float* prob,
                      float* rowloss, float* loss, int* count,
                      int64_t nrows, int C, int ignore, bool has_ignore,
                      hipStream_t stream);
void softmax_loss_bwd(const float* prob, const float* label, void* dx,
                      float scale, int64_t nrows, int C, int ignore,
                      bool has_ignore, hipStream_t stream);

}  // namespace cosamd

namespace {

using at::Tensor;

hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

#define CHECK_BF16(t) \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16")
#define CHECK_F32(t) \
  TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be fp32")
#define CHECK_CUDA(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU")

void py_gemm(Tensor A, Tensor B, Tensor C, c10::optional<Tensor> bias,
             int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
             int64_t ldc, bool trans_a, bool trans_b, int64_t store_mode,
             int64_t splitk, bool relu, double alpha, int64_t m_alloc,
             int64_t n_alloc) {
  CHECK_CUDA(A); CHECK_BF16(A); CHECK_BF16(B);
  const float* bptr = nullptr;
  if (bias.has_value()) {
    CHECK_F32(bias.value());
    bptr = bias.value().data_ptr<float>();
  }
  cosamd::gemm_bf16(
      A.data_ptr(), B.data_ptr(), C.data_ptr(), bptr, (int)M, (int)N, (int)K, (int)lda, (int)ldb, (int)ldc,
      trans_a, trans_b, (int)store_mode, (int)splitk, relu, (float)alpha,
      (int)m_alloc, (int)n_alloc, cur_stream());
}

// (route, BM, BN, ring depth, sk) of the InnerProduct GEMM [M, N, K];
// kind 0 forward, 1 data gradient; route 1 = gemm_fc, 0 = legacy
std::vector<int64_t> py_fc_gemm_plan(int64_t M, int64_t N, int64_t K,
                                     int64_t kind, bool aligned) {
  cosamd::FcPlan p = cosamd::fc_gemm_plan((int)M, (int)N, (int)K, (int)kind,
                                          aligned);
  return {p.route, p.bm, p.bn, p.depth, p.sk};
}

// C = A @ op(B) by the weight-streaming kernel; A, B and C may be views
// (lda / ldb / ldc in elements), so their extents are checked against
// their storage here.  Returns the number of slabs written (1: C holds
// the result; more: finish with fc_slab_finalize).
int64_t py_gemm_fc(Tensor A, Tensor B, Tensor C, c10::optional<Tensor> slabs,
                   c10::optional<Tensor> bias, Tensor zpage, int64_t M,
                   int64_t N, int64_t K, int64_t lda, int64_t ldb,
                   int64_t ldc, int64_t kind, int64_t sk, bool relu) {
  CHECK_CUDA(A); CHECK_CUDA(B); CHECK_CUDA(C); CHECK_CUDA(zpage);
  CHECK_BF16(A); CHECK_BF16(B); CHECK_BF16(C); CHECK_BF16(zpage);
  TORCH_CHECK(zpage.numel() >= 8, "zpage must hold 16 zero bytes");
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && sk <= 65535, "gemm_fc: bad size");
  auto span = [](const Tensor& t) {
    return (int64_t)(t.storage().nbytes() / t.element_size()) -
           t.storage_offset();
  };
  int64_t br = kind == 1 ? K : N, bc = kind == 1 ? N : K;
  TORCH_CHECK(lda >= K && ldb >= bc && ldc >= N,
              "gemm_fc: leading dimension smaller than the row");
  TORCH_CHECK((M - 1) * lda + K <= span(A), "gemm_fc: A too small");
  TORCH_CHECK((br - 1) * ldb + bc <= span(B), "gemm_fc: B too small");
  TORCH_CHECK((M - 1) * ldc + N <= span(C), "gemm_fc: C too small");
  float* sp = nullptr;
  if (slabs.has_value()) {
    const Tensor& s = slabs.value();
    CHECK_CUDA(s); CHECK_F32(s);
    int64_t want = sk > 0 ? sk : cosamd::fc_gemm_plan(
        (int)M, (int)N, (int)K, (int)kind, true).sk;
    // split_k() of gemm.hip: whole 32-wide tiles per split
    int64_t ksplit = ((K + want - 1) / want + 31) / 32 * 32;
    int64_t need = (K + ksplit - 1) / ksplit;
    TORCH_CHECK(s.is_contiguous() && s.numel() >= need * M * N,
                "gemm_fc: slabs must hold one [M, N] slab per split");
    sp = s.data_ptr<float>();
  }
  const float* bptr = nullptr;
  if (bias.has_value()) {
    const Tensor& b = bias.value();
    CHECK_CUDA(b); CHECK_F32(b);
    TORCH_CHECK(b.is_contiguous() && b.numel() >= N,
                "gemm_fc: bias must hold N contiguous floats");
    bptr = b.data_ptr<float>();
  }
  return cosamd::gemm_fc(A.data_ptr(), B.data_ptr(), C.data_ptr(), sp, bptr,
                         zpage.data_ptr(), (int)M, (int)N, (int)K, (int)lda,
                         (int)ldb, (int)ldc, (int)kind, (int)sk, relu,
                         cur_stream());
}

void py_fc_slab_finalize(Tensor slabs, int64_t sk, c10::optional<Tensor> bias,
                         Tensor out, int64_t M, int64_t N, int64_t ldo,
                         bool relu) {
  CHECK_CUDA(slabs); CHECK_F32(slabs); CHECK_CUDA(out); CHECK_BF16(out);
  TORCH_CHECK(sk >= 1 && slabs.is_contiguous() &&
              slabs.numel() >= sk * M * N, "fc_slab_finalize: slabs too small");
  TORCH_CHECK(ldo >= N && (M - 1) * ldo + N <=
              (int64_t)(out.storage().nbytes() / 2) - out.storage_offset(),
              "fc_slab_finalize: out too small");
  const float* bptr = nullptr;
  if (bias.has_value()) {
    CHECK_F32(bias.value());
    TORCH_CHECK(bias.value().is_contiguous() && bias.value().numel() >= N,
                "fc_slab_finalize: bias must hold N contiguous floats");
    bptr = bias.value().data_ptr<float>();
  }
  cosamd::fc_slab_finalize(slabs.data_ptr<float>(), (int)sk, bptr,
                           out.data_ptr(), (int)M, (int)N, (int)ldo, relu,
                           cur_stream());
}

// elements addressable from t's first element to the end of its storage
int64_t span_f32(const Tensor& t) {
  return (int64_t)(t.storage().nbytes() / sizeof(float)) - t.storage_offset();
}

// fp32 GEMM on the f32 MFMA (gemm_f32.hip).  Same operand convention and
// argument order as `gemm`, minus the bf16-only arguments.  A, B and C may be
// row sub-views: only the leading dimensions describe them, so every
// operand's extent is checked against its storage before the launch.
void py_gemm_f32(Tensor A, Tensor B, Tensor C, c10::optional<Tensor> bias,
                 int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                 int64_t ldc, bool trans_a, bool trans_b, int64_t splitk,
                 bool relu) {
  CHECK_CUDA(A); CHECK_CUDA(B); CHECK_CUDA(C);
  CHECK_F32(A); CHECK_F32(B); CHECK_F32(C);
  const int64_t lim = 1ll << 31;
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && M < lim && N < lim && K < lim,
              "gemm_f32: bad M/N/K");
  int64_t ar = trans_a ? K : M, ac = trans_a ? M : K;
  int64_t br = trans_b ? K : N, bc = trans_b ? N : K;
  TORCH_CHECK(lda >= ac && ldb >= bc && ldc >= N,
              "gemm_f32: leading dimension smaller than the row");
  TORCH_CHECK((ar - 1) * lda + ac <= span_f32(A), "gemm_f32: A too small");
  TORCH_CHECK((br - 1) * ldb + bc <= span_f32(B), "gemm_f32: B too small");
  TORCH_CHECK((M - 1) * ldc + N <= span_f32(C), "gemm_f32: C too small");
  TORCH_CHECK(splitk >= 1 && splitk <= 65535, "gemm_f32: bad splitk");
  TORCH_CHECK((N + 127) / 128 <= 65535, "gemm_f32: N too large");
  const float* bptr = nullptr;
  if (bias.has_value()) {
    const Tensor& b = bias.value();
    CHECK_CUDA(b); CHECK_F32(b);
    TORCH_CHECK(b.is_contiguous() && b.numel() >= N,
                "gemm_f32: bias must hold N contiguous floats");
    bptr = b.data_ptr<float>();
  }
  cosamd::gemm_f32(A.data_ptr<float>(), B.data_ptr<float>(),
                   C.data_ptr<float>(), bptr, (int)M, (int)N, (int)K, lda,
                   ldb, ldc, trans_a, trans_b, (int)splitk, relu,
                   cur_stream());
}

// fp32 im2col / col2im (gemm_f32.hip).  x / dx are logical-NCHW 4-D tensors
// read or written through their strides; col is the dense
// [N*P*Q][R*S*Cg] matrix (channel fastest) of channels c0 .. c0+Cg-1.
void check_conv_f32(const Tensor& x, const Tensor& col, int64_t P, int64_t Q,
                    int64_t R, int64_t S, int64_t sh, int64_t sw, int64_t ph,
                    int64_t pw, int64_t dh, int64_t dw, int64_t c0,
                    int64_t Cg) {
  CHECK_CUDA(x); CHECK_CUDA(col); CHECK_F32(x); CHECK_F32(col);
  TORCH_CHECK(x.dim() == 4, "x must be 4-D");
  const int64_t lim = 1ll << 31;
  int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(N > 0 && H > 0 && W > 0 && N < lim && H < lim && W < lim,
              "bad input shape");
  TORCH_CHECK(P > 0 && Q > 0 && R > 0 && S > 0 && sh > 0 && sw > 0 &&
              ph >= 0 && pw >= 0 && dh > 0 && dw > 0 && c0 >= 0 && Cg > 0 &&
              c0 + Cg <= C, "bad conv geometry");
  TORCH_CHECK(N * P * Q < lim && Cg * R * S < lim, "conv too large");
  int64_t last = 0;
  for (int d = 0; d < 4; ++d) {
    TORCH_CHECK(x.stride(d) >= 0, "negative stride");
    last += (x.size(d) - 1) * x.stride(d);
  }
  TORCH_CHECK(last < span_f32(x), "x view exceeds its storage");
  TORCH_CHECK(col.is_contiguous() && col.numel() >= N * P * Q * Cg * R * S,
              "col too small");
}

void py_im2col_f32(Tensor x, Tensor col, int64_t P, int64_t Q, int64_t R,
                   int64_t S, int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                   int64_t dh, int64_t dw, int64_t c0, int64_t Cg) {
  check_conv_f32(x, col, P, Q, R, S, sh, sw, ph, pw, dh, dw, c0, Cg);
  cosamd::im2col_f32(x.data_ptr<float>(), col.data_ptr<float>(),
                     (int)x.size(0), (int)x.size(2), (int)x.size(3), (int)P,
                     (int)Q, (int)R, (int)S, (int)sh, (int)sw, (int)ph,
                     (int)pw, (int)dh, (int)dw, (int)c0, (int)Cg,
                     x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                     cur_stream());
}

void py_col2im_f32(Tensor dcol, Tensor dx, int64_t P, int64_t Q, int64_t R,
                   int64_t S, int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                   int64_t dh, int64_t dw, int64_t c0, int64_t Cg) {
  check_conv_f32(dx, dcol, P, Q, R, S, sh, sw, ph, pw, dh, dw, c0, Cg);
  cosamd::col2im_f32(dcol.data_ptr<float>(), dx.data_ptr<float>(),
                     (int)dx.size(0), (int)dx.size(2), (int)dx.size(3),
                     (int)P, (int)Q, (int)R, (int)S, (int)sh, (int)sw,
                     (int)ph, (int)pw, (int)dh, (int)dw, (int)c0, (int)Cg,
                     dx.stride(0), dx.stride(1), dx.stride(2), dx.stride(3),
                     cur_stream());
}

void py_gemm_conv_fwd(Tensor X, Tensor B, Tensor C,
                      c10::optional<Tensor> bias, Tensor zpage,
                      int64_t M, int64_t N, int64_t K, int64_t ldb,
                      int64_t ldc, bool relu, bool accum,
                      std::vector<int64_t> geom, int64_t groups,
                      int64_t gs_c, int64_t gs_b, int64_t gs_n,
                      int64_t cfg, int64_t vec) {
  CHECK_CUDA(X); CHECK_BF16(X); CHECK_BF16(B); CHECK_BF16(C);
  TORCH_CHECK(groups >= 1, "groups must be positive");
  const float* bptr = nullptr;
  if (bias.has_value()) {
    CHECK_F32(bias.value());
    bptr = bias.value().data_ptr<float>();
  }
  int g[14];
  TORCH_CHECK(geom.size() == 14, "geom must have 14 ints");
  for (int i = 0; i < 14; ++i) g[i] = (int)geom[i];
  cosamd::gemm_conv_fwd(X.data_ptr(), B.data_ptr(), C.data_ptr(), bptr,
                        zpage.data_ptr(), (int)M, (int)N, (int)K,
                        (int)ldb, (int)ldc, relu, accum, g, (int)groups,
                        (int)gs_c, (int)gs_b, (int)gs_n, (int)cfg, (int)vec,
                        cur_stream());
}

// (BM, BN, waves, ring depth) gemm_conv_fwd picks for [M, N, K]
std::vector<int64_t> py_conv_fwd_plan(int64_t M, int64_t N, int64_t K) {
  cosamd::ConvCfg p = cosamd::conv_fwd_plan((int)M, (int)N, (int)K);
  return {p.bm, p.bn, p.waves, p.depth};
}

// the same four numbers for every configuration id (the cfg argument)
std::vector<std::vector<int64_t>> py_conv_fwd_cfgs() {
  std::vector<std::vector<int64_t>> out;
  for (int i = 0; i < cosamd::conv_fwd_num_cfgs(); ++i) {
    cosamd::ConvCfg p = cosamd::conv_fwd_cfg(i);
    out.push_back({p.bm, p.bn, p.waves, p.depth});
  }
  return out;
}

void py_gemm_conv_dw(Tensor A, Tensor X, Tensor C,
                     c10::optional<Tensor> db, Tensor zpage, int64_t M,
                     int64_t N,
                     int64_t K, int64_t lda, int64_t ldc,
                     int64_t store_mode, int64_t splitk, double alpha,
                     std::vector<int64_t> geom) {
  CHECK_CUDA(A); CHECK_BF16(A); CHECK_BF16(X); CHECK_F32(C);
  CHECK_CUDA(zpage); CHECK_BF16(zpage);
  TORCH_CHECK(zpage.numel() >= 8, "zpage must hold 16 zero bytes");
  float* dbp = nullptr;
  if (db.has_value()) {
    CHECK_F32(db.value());
    dbp = db.value().data_ptr<float>();
  }
  int g[14];
  TORCH_CHECK(geom.size() == 14, "geom must have 14 ints");
  for (int i = 0; i < 14; ++i) g[i] = (int)geom[i];
  cosamd::gemm_conv_dw(A.data_ptr(), X.data_ptr(), C.data_ptr<float>(),
                       zpage.data_ptr(), (int)M, (int)N, (int)K, (int)lda, (int)ldc,
                       (int)store_mode, (int)splitk, (float)alpha, dbp,
                       g, cur_stream());
}

void py_relu_colsum_bwd(Tensor y, Tensor dy, Tensor dx, Tensor db,
                        double slope, int64_t rows, int64_t cols,
                        int64_t ldy, int64_t lddy) {
  CHECK_CUDA(y); CHECK_BF16(y); CHECK_BF16(dy); CHECK_BF16(dx);
  CHECK_F32(db);
  cosamd::relu_colsum_bwd(y.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                          db.data_ptr<float>(), (float)slope, rows,
                          (int)cols, (int)ldy, (int)lddy, cur_stream());
}

// dense [rows][C] fast route; row_blocks 0 = auto (see relu_db_dense)
void py_relu_db_dense(Tensor y, Tensor dy, Tensor dx, Tensor db,
                      double slope, int64_t rows, int64_t C,
                      int64_t row_blocks) {
  CHECK_CUDA(y); CHECK_BF16(y); CHECK_BF16(dy); CHECK_BF16(dx);
  CHECK_F32(db);
  TORCH_CHECK(C > 0 && C % 8 == 0, "relu_db_dense needs C % 8 == 0");
  TORCH_CHECK(rows >= 0 && y.numel() >= rows * C && dy.numel() >= rows * C &&
              dx.numel() >= rows * C && db.numel() >= C,
              "relu_db_dense: tensors smaller than rows x C");
  TORCH_CHECK(y.is_contiguous() && dy.is_contiguous() &&
              dx.is_contiguous() && db.is_contiguous(),
              "relu_db_dense needs dense [rows][C] tensors");
  TORCH_CHECK(row_blocks >= 0 && row_blocks <= 65535, "row_blocks");
  cosamd::relu_db_dense(y.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                        db.data_ptr<float>(), (float)slope, rows, (int)C,
                        (int)row_blocks, cur_stream());
}

void py_gemm_conv_fwd_sc(Tensor X, Tensor B, Tensor C,
                         c10::optional<Tensor> bias, int64_t M,
                         int64_t N, int64_t K, int64_t ldb, int64_t ldc,
                         bool relu, std::vector<int64_t> geom) {
  CHECK_CUDA(X); CHECK_BF16(X); CHECK_BF16(B); CHECK_BF16(C);
  const float* bptr = nullptr;
  if (bias.has_value()) {
    CHECK_F32(bias.value());
    bptr = bias.value().data_ptr<float>();
  }
  int g[14];
  TORCH_CHECK(geom.size() == 14, "geom must have 14 ints");
  for (int i = 0; i < 14; ++i) g[i] = (int)geom[i];
  cosamd::gemm_conv_fwd_sc(X.data_ptr(), B.data_ptr(), C.data_ptr(),
                           bptr, (int)M, (int)N, (int)K, (int)ldb,
                           (int)ldc, relu, g, cur_stream());
}

void py_gemm_conv_dw_sc(Tensor A, Tensor X, Tensor C,
                        c10::optional<Tensor> db, int64_t M, int64_t N,
                        int64_t K, int64_t lda, int64_t ldc,
                        int64_t store_mode, int64_t splitk, double alpha,
                        std::vector<int64_t> geom) {
  CHECK_CUDA(A); CHECK_BF16(A); CHECK_BF16(X); CHECK_F32(C);
  float* dbp = nullptr;
  if (db.has_value()) {
    CHECK_F32(db.value());
    dbp = db.value().data_ptr<float>();
  }
  int g[14];
  TORCH_CHECK(geom.size() == 14, "geom must have 14 ints");
  for (int i = 0; i < 14; ++i) g[i] = (int)geom[i];
  cosamd::gemm_conv_dw_sc(A.data_ptr(), X.data_ptr(),
                          C.data_ptr<float>(), (int)M, (int)N, (int)K,
                          (int)lda, (int)ldc, (int)store_mode,
                          (int)splitk, (float)alpha, dbp, g,
                          cur_stream());
}

void py_im2col(Tensor x, Tensor col, int64_t N, int64_t H, int64_t W,
               int64_t C, int64_t P, int64_t Q, int64_t R, int64_t S,
               int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dil,
               int64_t Kpad, int64_t c0, int64_t Ct) {
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_BF16(col);
  cosamd::im2col_nhwc(x.data_ptr(), col.data_ptr(), N, H, W, C, P, Q, R, S,
                      sh, sw, ph, pw, dil, Kpad, c0, Ct, cur_stream());
}

void py_col2im(Tensor dcol, Tensor dx, int64_t N, int64_t H, int64_t W,
               int64_t C, int64_t P, int64_t Q, int64_t R, int64_t S,
               int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dil,
               int64_t Kpad, int64_t c0, int64_t Ct) {
  CHECK_CUDA(dcol); CHECK_BF16(dcol); CHECK_BF16(dx);
  cosamd::col2im_nhwc(dcol.data_ptr(), dx.data_ptr(), N, H, W, C, P, Q, R, S,
                      sh, sw, ph, pw, dil, Kpad, c0, Ct, cur_stream());
}

void py_maxpool_fwd(Tensor x, Tensor y, Tensor idx, int64_t N, int64_t H,
                    int64_t W, int64_t C, int64_t P, int64_t Q, int64_t kh,
                    int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                    int64_t pw) {
  CHECK_CUDA(x); CHECK_BF16(x);
  cosamd::maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(),
                      idx.scalar_type() == at::kChar, N, H,
                      W, C, P, Q, kh, kw, sh, sw, ph, pw, cur_stream());
}

void py_maxpool_bwd(Tensor dy, Tensor idx, Tensor dx, int64_t N, int64_t H,
                    int64_t W, int64_t C, int64_t P, int64_t Q, int64_t kh,
                    int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                    int64_t pw) {
  cosamd::maxpool_bwd(dy.data_ptr(), idx.data_ptr(),
                      idx.scalar_type() == at::kChar, dx.data_ptr(), N, H,
                      W, C, P, Q, kh, kw, sh, sw, ph, pw, cur_stream());
}

// dy, idx, top: [N,P,Q,C]; dx: [N,H,W,C]; blocks 0 = auto
void py_maxpool_bwd8_relu_db(Tensor dy, Tensor idx, Tensor top, Tensor dx,
                             Tensor db, int64_t N, int64_t H, int64_t W,
                             int64_t C, int64_t P, int64_t Q, int64_t kh,
                             int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                             int64_t pw, int64_t blocks) {
  CHECK_CUDA(dy); CHECK_BF16(dy); CHECK_BF16(top); CHECK_BF16(dx);
  CHECK_F32(db);
  TORCH_CHECK(idx.scalar_type() == at::kChar, "int8 argmax only");
  TORCH_CHECK(C > 0 && C % 8 == 0 && C <= 8192, "needs C % 8 == 0, <= 8192");
  int64_t npq = N * P * Q * C, nhw = N * H * W * C;
  TORCH_CHECK(dy.numel() == npq && idx.numel() == npq &&
              top.numel() == npq && dx.numel() == nhw && db.numel() >= C,
              "maxpool_bwd8_relu_db: tensor sizes do not match the geometry");
  TORCH_CHECK(nhw / 8 < (int64_t(1) << 32), "activation too large");
  TORCH_CHECK(blocks >= 0 && blocks <= 65535, "blocks");
  cosamd::maxpool_bwd8_relu_db(dy.data_ptr(), idx.data_ptr(), top.data_ptr(),
                               dx.data_ptr(), db.data_ptr<float>(), N, H, W,
                               C, P, Q, kh, kw, sh, sw, ph, pw, (int)blocks,
                               cur_stream());
}

void py_avgpool_fwd(Tensor x, Tensor y, int64_t N, int64_t H, int64_t W,
                    int64_t C, int64_t P, int64_t Q, int64_t kh, int64_t kw,
                    int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
  cosamd::avgpool_fwd(x.data_ptr(), y.data_ptr(), N, H, W, C, P, Q, kh, kw,
                      sh, sw, ph, pw, cur_stream());
}

void py_avgpool_bwd(Tensor dy, Tensor dx, int64_t N, int64_t H, int64_t W,
                    int64_t C, int64_t P, int64_t Q, int64_t kh, int64_t kw,
                    int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
  cosamd::avgpool_bwd(dy.data_ptr(), dx.data_ptr(), N, H, W, C, P, Q, kh, kw,
                      sh, sw, ph, pw, cur_stream());
}

void py_lrn_fwd(Tensor x, Tensor y, Tensor scale, int64_t npix, int64_t C,
                int64_t local_size, double alpha, double beta, double k) {
  CHECK_F32(scale);
  cosamd::lrn_fwd(x.data_ptr(), y.data_ptr(), scale.data_ptr<float>(), npix,
                  C, local_size, alpha, beta, k, cur_stream());
}

void py_lrn_bwd(Tensor x, Tensor y, Tensor scale, Tensor dy, Tensor dx,
                Tensor ratio, int64_t npix, int64_t C, int64_t local_size,
                double alpha, double beta) {
  cosamd::lrn_bwd(x.data_ptr(), y.data_ptr(), scale.data_ptr<float>(),
                  dy.data_ptr(), dx.data_ptr(), ratio.data_ptr(), npix, C,
                  local_size, alpha, beta, cur_stream());
}

void py_relu_fwd(Tensor x, Tensor y, double slope) {
  CHECK_BF16(x);
  cosamd::relu_fwd(x.data_ptr(), y.data_ptr(), (float)slope, x.numel(),
                   cur_stream());
}

void py_relu_bwd(Tensor y, Tensor dy, Tensor dx, double slope) {
  cosamd::relu_bwd(y.data_ptr(), dy.data_ptr(), dx.data_ptr(), (float)slope,
                   y.numel(), cur_stream());
}

void py_dropout_fwd(Tensor x, Tensor y, Tensor mask, double ratio,
                    Tensor seed) {
  cosamd::dropout_fwd(x.data_ptr(), y.data_ptr(), mask.data_ptr(), ratio,
                      seed.data_ptr(), x.numel(), cur_stream());
}

void py_mul(Tensor a, Tensor b, Tensor y) {
  cosamd::mul_bf16(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(),
                   cur_stream());
}

void py_sgd_update_multi(Tensor p, Tensor g, Tensor v, Tensor seg_off,
                         Tensor seg_lr, Tensor seg_wd, double mu,
                         c10::optional<Tensor> sh) {
  CHECK_F32(p); CHECK_F32(g); CHECK_F32(v);
  void* shp = nullptr;
  if (sh.has_value()) { CHECK_BF16(sh.value()); shp = sh->data_ptr(); }
  cosamd::sgd_update_multi(p.data_ptr<float>(), g.data_ptr<float>(),
                           v.data_ptr<float>(),
                           seg_off.data_ptr<int64_t>(),
                           seg_lr.data_ptr<float>(),
                           seg_wd.data_ptr<float>(),
                           (int)seg_lr.numel(), mu, p.numel(), shp,
                           cur_stream());
}

void py_nesterov_update_multi(Tensor p, Tensor g, Tensor v, Tensor seg_off,
                              Tensor seg_lr, Tensor seg_wd, double mu,
                              c10::optional<Tensor> sh) {
  CHECK_F32(p); CHECK_F32(g); CHECK_F32(v);
  void* shp = nullptr;
  if (sh.has_value()) { CHECK_BF16(sh.value()); shp = sh->data_ptr(); }
  cosamd::nesterov_update_multi(p.data_ptr<float>(), g.data_ptr<float>(),
                                v.data_ptr<float>(),
                                seg_off.data_ptr<int64_t>(),
                                seg_lr.data_ptr<float>(),
                                seg_wd.data_ptr<float>(),
                                (int)seg_lr.numel(), mu, p.numel(), shp,
                                cur_stream());
}

void py_adam_update_multi(Tensor p, Tensor g, Tensor m, Tensor v,
                          Tensor seg_off, Tensor seg_lr, Tensor seg_wd,
                          double b1, double b2, double eps,
                          c10::optional<Tensor> sh) {
  CHECK_F32(p); CHECK_F32(g); CHECK_F32(m); CHECK_F32(v);
  void* shp = nullptr;
  if (sh.has_value()) { CHECK_BF16(sh.value()); shp = sh->data_ptr(); }
  cosamd::adam_update_multi(p.data_ptr<float>(), g.data_ptr<float>(),
                            m.data_ptr<float>(), v.data_ptr<float>(),
                            seg_off.data_ptr<int64_t>(),
                            seg_lr.data_ptr<float>(),
                            seg_wd.data_ptr<float>(),
                            (int)seg_lr.numel(), b1, b2, eps, p.numel(),
                            shp, cur_stream());
}

void py_sgd_update(Tensor p, Tensor g, Tensor v, double lr, double mu,
                   double wd) {
  CHECK_F32(p); CHECK_F32(g); CHECK_F32(v);
  cosamd::sgd_update(p.data_ptr<float>(), g.data_ptr<float>(),
                     v.data_ptr<float>(), lr, mu, wd, p.numel(),
                     cur_stream());
}

void py_bias_act_cast(Tensor in, c10::optional<Tensor> bias, Tensor out,
                      bool relu) {
  CHECK_F32(in);
  const float* bptr = bias.has_value() ? bias.value().data_ptr<float>()
                                       : nullptr;
  cosamd::bias_act_cast(in.data_ptr<float>(), bptr, out.data_ptr(),
                        in.size(0), in.size(1), relu, cur_stream());
}

void py_dw_unpack_acc(Tensor dwp, Tensor arena, int64_t Kout, int64_t Cg,
                      int64_t R, int64_t S, int64_t Kpad,
                      bool accumulate) {
  cosamd::dw_unpack_acc(dwp.data_ptr<float>(), arena.data_ptr<float>(),
                        (int)Kout, (int)Cg, (int)R, (int)S, (int)Kpad,
                        accumulate, cur_stream());
}

void py_repack_weights(Tensor table, int64_t ndesc, int64_t max_total) {
  cosamd::repack_weights(table.data_ptr<int64_t>(), (int)ndesc, max_total,
                         cur_stream());
}

// space-to-depth pack: x is read in place through its element strides
// (NCHW-contiguous, channels-last or a strided view); out is the dense
// channels-last [N][Hp][Wp][st*st*C] buffer, fully overwritten
void py_s2d_pack(Tensor x, Tensor out, int64_t st, int64_t ph, int64_t pw,
                 int64_t Hp, int64_t Wp) {
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CUDA(out); CHECK_BF16(out);
  TORCH_CHECK(x.dim() == 4, "x must be 4-D");
  int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(st >= 2 && ph >= 0 && pw >= 0, "bad s2d geometry");
  TORCH_CHECK(out.is_contiguous() &&
              out.numel() == N * Hp * Wp * st * st * C,
              "out must be dense [N][Hp][Wp][st*st*C]");
  cosamd::s2d_pack(x.data_ptr(), out.data_ptr(), (int)N, (int)H, (int)W,
                   (int)C, (int)st, (int)ph, (int)pw, (int)Hp, (int)Wp,
                   x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                   cur_stream());
}

// device-side DataTransformer: src is the packed uint8 bytes of the batch,
// table the [N,7] int64 rows (byte_offset, H, W, planar, h_off, w_off,
// mirror) on the device and table_host the same rows on the host, where
// they are validated before the launch; out is any [N,C,oh,ow] view,
// written through its strides
void py_data_transform(Tensor src, Tensor table, Tensor table_host,
                       c10::optional<Tensor> mean, int64_t mean_mode,
                       double scale, Tensor out) {
  CHECK_CUDA(src); CHECK_CUDA(table); CHECK_CUDA(out);
  TORCH_CHECK(src.scalar_type() == at::kByte && src.dim() == 1 &&
              src.is_contiguous(), "src must be a dense 1-D uint8 buffer");
  TORCH_CHECK(out.dim() == 4, "out must be 4-D");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 ||
              out.scalar_type() == at::kFloat, "out must be bf16 or fp32");
  int64_t N = out.size(0);
  TORCH_CHECK(table.scalar_type() == at::kLong && table.is_contiguous() &&
              table.dim() == 2 && table.size(0) == N && table.size(1) == 7,
              "table must be a dense [N,7] int64 tensor");
  TORCH_CHECK(!table_host.is_cuda() &&
              table_host.scalar_type() == at::kLong &&
              table_host.is_contiguous() &&
              table_host.sizes() == table.sizes(),
              "table_host must be the host copy of table");
  TORCH_CHECK(N < (1ll << 31) && out.size(1) < (1ll << 31) &&
              out.size(2) < (1ll << 31) && out.size(3) < (1ll << 31),
              "out too large");
  const float* mptr = nullptr;
  int64_t mnumel = 0;
  int mC = 0, mH = 0, mW = 0;
  if (mean_mode != 0) {
    TORCH_CHECK(mean.has_value(), "mean_mode != 0 needs a mean");
    const Tensor& m = mean.value();
    CHECK_CUDA(m); CHECK_F32(m);
    TORCH_CHECK(m.is_contiguous(), "mean must be contiguous");
    if (mean_mode == 2) {
      TORCH_CHECK(m.dim() == 3 && m.size(1) < (1ll << 31) &&
                  m.size(2) < (1ll << 31), "mean image must be [C,H,W]");
      mC = (int)m.size(0); mH = (int)m.size(1); mW = (int)m.size(2);
    }
    mptr = m.data_ptr<float>();
    mnumel = m.numel();
  }
  cosamd::data_transform(
      src.data_ptr(), src.numel(), table.data_ptr<int64_t>(),
      table_host.data_ptr<int64_t>(), (int)N, mptr, (int)mean_mode, mnumel,
      mC, mH, mW, (float)scale, out.data_ptr(),
      out.scalar_type() == at::kBFloat16, (int)out.size(1),
      (int)out.size(2), (int)out.size(3), out.stride(0), out.stride(1),
      out.stride(2), out.stride(3), cur_stream());
}

void py_s2d_pack_weight(Tensor src, Tensor dst, int64_t Kout, int64_t Cg,
                        int64_t R, int64_t S, int64_t st, int64_t Kpad) {
  CHECK_CUDA(src); CHECK_BF16(src); CHECK_CUDA(dst); CHECK_BF16(dst);
  int64_t Rp = (R + st - 1) / st, Sp = (S + st - 1) / st;
  TORCH_CHECK(st >= 2 && src.is_contiguous() &&
              src.numel() == Kout * Cg * R * S, "bad s2d weight source");
  TORCH_CHECK(dst.is_contiguous() && dst.dim() == 2 &&
              dst.size(0) >= Kout && dst.size(1) == Kpad &&
              Kpad >= Rp * Sp * st * st * Cg, "bad s2d weight buffer");
  cosamd::s2d_pack_weight(src.data_ptr(), dst.data_ptr(), (int)Kout,
                          (int)Cg, (int)R, (int)S, (int)st, (int)Kpad,
                          cur_stream());
}

// depth-to-space weight pack (d2s.hip): src is the caffe deconvolution
// weight [Ci][Co][R][S]; dst the GEMM B operand [>= st*st*Co][Kpad], whose
// live [st*st*Co][R'*S'*Ci] region is fully overwritten
void py_d2s_pack_weight(Tensor src, Tensor dst, int64_t Ci, int64_t Co,
                        int64_t R, int64_t S, int64_t st, int64_t Kpad) {
  CHECK_CUDA(src); CHECK_BF16(src); CHECK_CUDA(dst); CHECK_BF16(dst);
  TORCH_CHECK(st >= 2 && Ci > 0 && Co > 0 && R > 0 && S > 0 &&
              Ci % 8 == 0 && Kpad % 8 == 0, "bad d2s weight geometry");
  int64_t Rp = (R + st - 1) / st, Sp = (S + st - 1) / st;
  const int64_t lim = 1ll << 31;
  TORCH_CHECK(Ci < lim && Co < lim && R < lim && S < lim && st < lim &&
              Kpad < lim && st * st * Co < lim && Rp * Sp * Ci < lim,
              "d2s weight too large");
  TORCH_CHECK(src.is_contiguous() && src.numel() == Ci * Co * R * S,
              "bad d2s weight source");
  TORCH_CHECK(dst.is_contiguous() && dst.dim() == 2 &&
              dst.size(0) >= st * st * Co && dst.size(1) == Kpad &&
              Kpad >= Rp * Sp * Ci, "bad d2s weight buffer");
  TORCH_CHECK((uintptr_t)dst.data_ptr() % 16 == 0,
              "d2s weight buffer must be 16-byte aligned");
  cosamd::d2s_pack_weight(src.data_ptr(), dst.data_ptr(), (int)Ci, (int)Co,
                          (int)R, (int)S, (int)st, (int)Kpad, cur_stream());
}

// depth-to-space unpack (d2s.hip): z is the dense GEMM output
// [N][Hp][Wp][st*st*Co]; y any [N][Co][Ho][Wo] view, written through its
// strides
void py_d2s_unpack(Tensor z, Tensor y, int64_t st, int64_t ph, int64_t pw,
                   int64_t Hp, int64_t Wp) {
  CHECK_CUDA(z); CHECK_BF16(z); CHECK_CUDA(y); CHECK_BF16(y);
  TORCH_CHECK(y.dim() == 4, "y must be 4-D");
  const int64_t lim = 1ll << 31;
  int64_t N = y.size(0), Co = y.size(1), Ho = y.size(2), Wo = y.size(3);
  TORCH_CHECK(st >= 2 && st < lim && ph >= 0 && pw >= 0 && ph < lim &&
              pw < lim && Hp > 0 && Wp > 0 && Hp < lim && Wp < lim,
              "bad d2s geometry");
  TORCH_CHECK(N < lim && Co < lim && Ho < lim && Wo < lim, "y too large");
  TORCH_CHECK(z.is_contiguous() && z.numel() == N * Hp * Wp * st * st * Co,
              "z must be dense [N][Hp][Wp][st*st*Co]");
  int64_t last = 0;
  for (int d = 0; d < 4; ++d) {
    TORCH_CHECK(y.stride(d) >= 0, "negative stride");
    last += (y.size(d) - 1) * y.stride(d);
  }
  TORCH_CHECK(y.numel() == 0 ||
              last < (int64_t)(y.storage().nbytes() / 2) - y.storage_offset(),
              "y view exceeds its storage");
  cosamd::d2s_unpack(z.data_ptr(), y.data_ptr(), (int)N, (int)Co, (int)Ho,
                     (int)Wo, (int)st, (int)ph, (int)pw, (int)Hp, (int)Wp,
                     y.stride(0), y.stride(1), y.stride(2), y.stride(3),
                     cur_stream());
}

void py_dw_unpack_s2d(Tensor dwp, Tensor arena, int64_t Kout, int64_t Cg,
                      int64_t R, int64_t S, int64_t st, int64_t Kpad,
                      bool accumulate) {
  CHECK_CUDA(dwp); CHECK_F32(dwp); CHECK_CUDA(arena); CHECK_F32(arena);
  int64_t Rp = (R + st - 1) / st, Sp = (S + st - 1) / st;
  TORCH_CHECK(st >= 2 && dwp.is_contiguous() &&
              dwp.numel() >= Kout * Kpad &&
              Kpad >= Rp * Sp * st * st * Cg, "bad s2d dw buffer");
  TORCH_CHECK(arena.is_contiguous() &&
              arena.numel() == Kout * Cg * R * S, "bad s2d dw target");
  cosamd::dw_unpack_s2d(dwp.data_ptr<float>(), arena.data_ptr<float>(),
                        (int)Kout, (int)Cg, (int)R, (int)S, (int)st,
                        (int)Kpad, accumulate, cur_stream());
}

int64_t py_lstm_persist_fwd(Tensor xg, Tensor w_hc, Tensor cont,
                            Tensor h, Tensor c, Tensor act, Tensor h_in,
                            Tensor hg, int64_t T, int64_t N, int64_t H,
                            Tensor bar) {
  return cosamd::lstm_persist_fwd(
      xg.data_ptr(), w_hc.data_ptr(), cont.data_ptr(), h.data_ptr(),
      c.data_ptr<float>(), act.data_ptr<float>(), h_in.data_ptr(),
      hg.data_ptr<float>(), (int)T, (int)N, (int)H, bar.data_ptr(),
      cur_stream());
}

int64_t py_lstm_persist_bwd(Tensor dy, Tensor w_hcT, Tensor cont,
                            Tensor h, Tensor c, Tensor act, Tensor dxg,
                            Tensor dh_acc, Tensor dc_a, Tensor dc_b,
                            int64_t T, int64_t N, int64_t H, Tensor bar) {
  return cosamd::lstm_persist_bwd(
      dy.data_ptr(), w_hcT.data_ptr(), cont.data_ptr(), h.data_ptr(),
      c.data_ptr<float>(), act.data_ptr<float>(), dxg.data_ptr(),
      dh_acc.data_ptr<float>(), dc_a.data_ptr<float>(),
      dc_b.data_ptr<float>(), (int)T, (int)N, (int)H, bar.data_ptr(),
      cur_stream());
}

void py_transpose(Tensor in, Tensor out, int64_t R, int64_t C) {
  CHECK_BF16(in); CHECK_BF16(out);
  cosamd::transpose_bf16(in.data_ptr(), out.data_ptr(), R, C, cur_stream());
}

void py_colsum(Tensor in, Tensor out, int64_t rows, int64_t cols,
               int64_t ld) {
  CHECK_F32(out);
  cosamd::colsum(in.data_ptr(), out.data_ptr<float>(), rows, cols, ld,
                 cur_stream());
}

void py_lstm_unit_fwd(Tensor c_prev, Tensor gates, Tensor cont, Tensor c_out,
                      Tensor h_out, Tensor act) {
  CHECK_F32(c_prev); CHECK_BF16(gates);
  int64_t n = c_prev.numel();
  int H = c_prev.size(-1);
  cosamd::lstm_unit_fwd(c_prev.data_ptr<float>(), gates.data_ptr(),
                        cont.data_ptr(), c_out.data_ptr<float>(),
                        h_out.data_ptr(), act.data_ptr<float>(), n, H,
                        cur_stream());
}

void py_lstm_unit_bwd(Tensor c_prev, Tensor c_out, Tensor act, Tensor cont,
                      Tensor dc_next, Tensor dh, Tensor dc_prev,
                      Tensor dgates) {
  int64_t n = c_prev.numel();
  int H = c_prev.size(-1);
  cosamd::lstm_unit_bwd(c_prev.data_ptr<float>(), c_out.data_ptr<float>(),
                        act.data_ptr<float>(), cont.data_ptr(),
                        dc_next.data_ptr<float>(), dh.data_ptr(),
                        dc_prev.data_ptr<float>(), dgates.data_ptr(), n, H,
                        cur_stream());
}

int64_t py_lstm_step_lds_bytes(int64_t N, int64_t D, int64_t H, int64_t Ds) {
  const int64_t lim = 1 << 24;
  if (N < 0 || D < 0 || H < 0 || Ds < 0 || N >= lim || D >= lim ||
      H >= lim || Ds >= lim)
    return -1;
  return cosamd::lstm_step_lds_bytes((int)N, (int)D, (int)H, (int)Ds);
}

// one decode token of one LSTM layer; every operand is checked against the
// extent the kernel reads or writes (16-byte loads: aligned, contiguous)
void py_lstm_step(Tensor x, Tensor h_prev, c10::optional<Tensor> xs,
                  Tensor w_xc, Tensor w_hc, c10::optional<Tensor> w_xsc,
                  Tensor bias, Tensor cont, Tensor c_prev, Tensor c_out,
                  Tensor h_out) {
  TORCH_CHECK(x.dim() == 2 && h_prev.dim() == 2, "lstm_step: 2-D x, h_prev");
  int64_t N = x.size(0), D = x.size(1), H = h_prev.size(1);
  int64_t Ds = xs.has_value() ? xs.value().size(-1) : 0;
  TORCH_CHECK(xs.has_value() == w_xsc.has_value(),
              "lstm_step: x_static and W_xsc go together");
  TORCH_CHECK(py_lstm_step_lds_bytes(N, D, H, Ds) >= 0,
              "lstm_step: shape outside the fused kernel");
  auto bf = [&](const Tensor& t, int64_t r, int64_t c, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.is_contiguous() && t.numel() == r * c &&
                reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                "lstm_step: ", what, " must be contiguous 16-byte aligned "
                "bf16 of ", r, "x", c);
  };
  auto f32 = [&](const Tensor& t, int64_t n, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                t.is_contiguous() && t.numel() == n,
                "lstm_step: ", what, " must be contiguous fp32 of ", n);
  };
  bf(x, N, D, "x"); bf(h_prev, N, H, "h_prev");
  bf(w_xc, 4 * H, D, "W_xc"); bf(w_hc, 4 * H, H, "W_hc");
  bf(h_out, N, H, "h_out");
  TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kBFloat16 &&
              bias.is_contiguous() && bias.numel() == 4 * H,
              "lstm_step: bias must be contiguous bf16 of 4H");
  const void* xsp = nullptr;
  const void* wsp = nullptr;
  if (Ds) {
    bf(xs.value(), N, Ds, "x_static"); bf(w_xsc.value(), 4 * H, Ds, "W_xsc");
    xsp = xs.value().data_ptr();
    wsp = w_xsc.value().data_ptr();
  }
  f32(cont, N, "cont"); f32(c_prev, N * H, "c_prev"); f32(c_out, N * H, "c");
  TORCH_CHECK(h_out.data_ptr() != h_prev.data_ptr() &&
              c_out.data_ptr() != c_prev.data_ptr(),
              "lstm_step: outputs must not alias the previous state");
  cosamd::lstm_step(x.data_ptr(), h_prev.data_ptr(), xsp, w_xc.data_ptr(),
                    w_hc.data_ptr(), wsp, bias.data_ptr(),
                    cont.data_ptr<float>(), c_prev.data_ptr<float>(),
                    c_out.data_ptr<float>(), h_out.data_ptr(), (int)N,
                    (int)D, (int)H, (int)Ds, cur_stream());
}

void py_embed_fwd(Tensor idx, Tensor w, Tensor y, int64_t V) {
  CHECK_F32(idx); CHECK_BF16(w);
  cosamd::embed_fwd(idx.data_ptr<float>(), w.data_ptr(), y.data_ptr(),
                    idx.numel(), w.size(1), V, cur_stream());
}

void py_embed_bwd(Tensor idx, Tensor dy, Tensor dw, int64_t V) {
  CHECK_F32(dw);
  cosamd::embed_bwd(idx.data_ptr<float>(), dy.data_ptr(),
                    dw.data_ptr<float>(), idx.numel(), dw.size(1), V,
                    cur_stream());
}

void py_lstm_seq_fwd(Tensor xg, Tensor w_hc, Tensor cont, Tensor h,
                     Tensor c, Tensor act, Tensor h_in, Tensor hg,
                     int64_t T, int64_t N, int64_t H, int64_t n_alloc) {
  CHECK_BF16(xg); CHECK_BF16(w_hc); CHECK_F32(c); CHECK_F32(act);
  CHECK_F32(hg);
  cosamd::lstm_seq_fwd(xg.data_ptr(), w_hc.data_ptr(), cont.data_ptr(),
                       h.data_ptr(), c.data_ptr<float>(),
                       act.data_ptr<float>(), h_in.data_ptr(),
                       hg.data_ptr<float>(), T, N, H, n_alloc,
                       cur_stream());
}

void py_lstm_seq_bwd(Tensor dy, Tensor w_hcT, Tensor cont, Tensor h,
                     Tensor c, Tensor act, Tensor dxg, Tensor dh_rec,
                     Tensor dh_f, Tensor dc_a, Tensor dc_b, int64_t T,
                     int64_t N, int64_t H, int64_t n_alloc) {
  CHECK_BF16(dy); CHECK_BF16(w_hcT); CHECK_F32(dh_f);
  cosamd::lstm_seq_bwd(dy.data_ptr(), w_hcT.data_ptr(), cont.data_ptr(),
                       h.data_ptr(), c.data_ptr<float>(),
                       act.data_ptr<float>(), dxg.data_ptr(),
                       dh_rec.data_ptr(), dh_f.data_ptr<float>(),
                       dc_a.data_ptr<float>(), dc_b.data_ptr<float>(),
                       T, N, H, n_alloc, cur_stream());
}

void py_softmax_loss_fwd(Tensor x, Tensor label, Tensor prob,
                         Tensor rowloss, Tensor loss, Tensor count,
                         int64_t ignore, bool has_ignore) {
  CHECK_BF16(x); CHECK_F32(label); CHECK_F32(prob); CHECK_F32(rowloss);
  TORCH_CHECK(rowloss.is_contiguous() && rowloss.numel() >= x.size(0),
              "rowloss must hold one value per row");
  cosamd::softmax_loss_fwd(x.data_ptr(), label.data_ptr<float>(),
                           prob.data_ptr<float>(),
                           rowloss.data_ptr<float>(), loss.data_ptr<float>(),
                           count.data_ptr<int>(), x.size(0), x.size(1),
                           (int)ignore, has_ignore, cur_stream());
}

void py_softmax_loss_bwd(Tensor prob, Tensor label, Tensor dx, double scale,
                         int64_t ignore, bool has_ignore) {
  cosamd::softmax_loss_bwd(prob.data_ptr<float>(), label.data_ptr<float>(),
                           dx.data_ptr(), scale, prob.size(0), prob.size(1),
                           (int)ignore, has_ignore, cur_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("gemm", &py_gemm);
  m.def("fc_gemm_plan", &py_fc_gemm_plan, py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("kind"), py::arg("aligned") = true);
  m.def("gemm_fc", &py_gemm_fc);
  m.def("fc_slab_finalize", &py_fc_slab_finalize);
  m.def("gemm_f32", &py_gemm_f32);
  m.def("im2col_f32", &py_im2col_f32);
  m.def("col2im_f32", &py_col2im_f32);
  m.def("relu_colsum_bwd", &py_relu_colsum_bwd);
  m.def("relu_db_dense", &py_relu_db_dense);
  // the 13 leading arguments are one group's GEMM; groups > 1 launches
  // every group at once (strides: input channels, B rows, C columns)
  m.def("gemm_conv_fwd", &py_gemm_conv_fwd, py::arg("X"), py::arg("B"),
        py::arg("C"), py::arg("bias"), py::arg("zpage"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("ldb"), py::arg("ldc"),
        py::arg("relu"), py::arg("accum"), py::arg("geom"),
        py::arg("groups") = 1, py::arg("gs_c") = 0, py::arg("gs_b") = 0,
        py::arg("gs_n") = 0, py::arg("cfg") = -1, py::arg("vec") = -1);
  m.def("conv_fwd_plan", &py_conv_fwd_plan);
  m.def("conv_fwd_cfgs", &py_conv_fwd_cfgs);
  m.def("gemm_conv_dw", &py_gemm_conv_dw);
  m.def("gemm_conv_fwd_sc", &py_gemm_conv_fwd_sc);
  m.def("gemm_conv_dw_sc", &py_gemm_conv_dw_sc);
  m.def("im2col", &py_im2col);
  m.def("bn_stats", [](Tensor x, Tensor sum, Tensor sq, int64_t rows,
                       int64_t C) {
    cosamd::bn_stats(x.data_ptr(), sum.data_ptr<float>(),
                     sq.data_ptr<float>(), rows, C, cur_stream());
  });
  m.def("bn_bwd_sums", [](Tensor dy, Tensor xhat, Tensor s1, Tensor s2,
                          int64_t rows, int64_t C) {
    cosamd::bn_bwd_sums(dy.data_ptr(), xhat.data_ptr(),
                        s1.data_ptr<float>(), s2.data_ptr<float>(), rows,
                        C, cur_stream());
  });
  m.def("bn_norm", [](Tensor x, Tensor y, Tensor mean, Tensor invstd,
                      int64_t rows, int64_t C) {
    cosamd::bn_norm(x.data_ptr(), y.data_ptr(), mean.data_ptr<float>(),
                    invstd.data_ptr<float>(), rows, C, cur_stream());
  });
  m.def("bn_bwd", [](Tensor xhat, Tensor dy, Tensor dx, Tensor invstd,
                     Tensor s1, Tensor s2, double inv_m, int64_t rows,
                     int64_t C) {
    cosamd::bn_bwd(xhat.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                   invstd.data_ptr<float>(), s1.data_ptr<float>(),
                   s2.data_ptr<float>(), (float)inv_m, rows, C,
                   cur_stream());
  });
  m.def("wino_conv", [](Tensor x, Tensor w, c10::optional<Tensor> bias,
                        Tensor y, Tensor U, Tensor V, Tensor M, int64_t N,
                        int64_t H, int64_t W, int64_t Cin, int64_t K,
                        int64_t wK, int64_t wC, int64_t u_rows_alloc,
                        bool flip, bool relu) {
    cosamd::wino_conv(x.data_ptr(), w.data_ptr<float>(),
                      bias ? bias->data_ptr<float>() : nullptr,
                      y.data_ptr(), U.data_ptr(), V.data_ptr(),
                      M.data_ptr(), N, H, W, Cin, K, wK, wC, u_rows_alloc,
                      flip, relu, cur_stream());
  });
  m.def("im2col_t", [](Tensor x, Tensor colT, int64_t N, int64_t H,
                       int64_t W, int64_t C, int64_t P, int64_t Q,
                       int64_t R, int64_t S, int64_t sh, int64_t sw,
                       int64_t ph, int64_t pw, int64_t dil, int64_t Kpad,
                       int64_t c0, int64_t Cg) {
    cosamd::im2col_t(x.data_ptr(), colT.data_ptr(), N, H, W, C, P, Q, R,
                     S, sh, sw, ph, pw, dil, Kpad, c0, Cg, cur_stream());
  });
  m.def("col2im", &py_col2im);
  m.def("maxpool_fwd", &py_maxpool_fwd);
  m.def("maxpool_bwd", &py_maxpool_bwd);
  m.def("maxpool_bwd8_relu_db", &py_maxpool_bwd8_relu_db);
  m.def("avgpool_fwd", &py_avgpool_fwd);
  m.def("avgpool_bwd", &py_avgpool_bwd);
  m.def("lrn_fwd", &py_lrn_fwd);
  m.def("lrn_bwd", &py_lrn_bwd);
  m.def("relu_fwd", &py_relu_fwd);
  m.def("relu_bwd", &py_relu_bwd);
  m.def("dropout_fwd", &py_dropout_fwd);
  m.def("relu_bwd_strided", [](Tensor y, Tensor dy, Tensor dx, double slope,
                               int64_t rows, int64_t C, int64_t ldy,
                               int64_t lddy) {
    cosamd::relu_bwd_strided(y.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                             (float)slope, rows, C, ldy, lddy,
                             cur_stream());
  });
  m.def("seed_bump", [](Tensor s) {
    cosamd::seed_bump(s.data_ptr(), cur_stream());
  });
  m.def("mul", &py_mul);
  m.def("sgd_update", &py_sgd_update);
  m.def("sgd_update_multi", &py_sgd_update_multi);
  m.def("nesterov_update_multi", &py_nesterov_update_multi);
  m.def("adam_update_multi", &py_adam_update_multi);
  m.def("colsum", &py_colsum);
  m.def("transpose", &py_transpose);
  m.def("repack_weights", &py_repack_weights);
  m.def("dw_unpack_acc", &py_dw_unpack_acc);
  m.def("s2d_pack", &py_s2d_pack);
  m.def("s2d_pack_weight", &py_s2d_pack_weight);
  m.def("d2s_pack_weight", &py_d2s_pack_weight);
  m.def("d2s_unpack", &py_d2s_unpack);
  m.def("data_transform", &py_data_transform);
  m.def("dw_unpack_s2d", &py_dw_unpack_s2d);
  m.def("lstm_persist_fwd", &py_lstm_persist_fwd);
  m.def("lstm_persist_bwd", &py_lstm_persist_bwd);
  m.def("bias_act_cast", &py_bias_act_cast);
  m.def("lstm_seq_fwd", &py_lstm_seq_fwd);
  m.def("lstm_seq_bwd", &py_lstm_seq_bwd);
  m.def("lstm_unit_fwd", &py_lstm_unit_fwd);
  m.def("lstm_unit_bwd", &py_lstm_unit_bwd);
  m.def("lstm_step", &py_lstm_step);
  m.def("lstm_step_lds_bytes", &py_lstm_step_lds_bytes);
  m.def("embed_fwd", &py_embed_fwd);
  m.def("embed_bwd", &py_embed_bwd);
  m.def("softmax_loss_fwd", &py_softmax_loss_fwd);
  m.def("softmax_loss_bwd", &py_softmax_loss_bwd);
}
